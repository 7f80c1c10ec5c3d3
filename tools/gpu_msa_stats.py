"""Times the empirical-parameter and alignment-statistics calls on device 0 and prints one JSON line per shape and
form:

  partition   pllhip_empirical_frequencies + pllhip_empirical_subst_rates on a partition with pattern tips: wall
              clock of each call (median of --repeat), the kernel time of the call (pllhip_msa_stats_last_times), and
              that against the traffic model -- tips * sites bytes of codes, read once, at 8 TB/s.
              Baseline: what the parent of this feature had to do for the same numbers, the loops of pll_msa.c in
              numpy over the host's tipchars (run once).
  alignment   pllhip_msa_compute_stats(ALL but the duplicate searches) on the raw rows: wall clock, upload, kernel.
  vectors     the partition form without PLL_ATTRIB_PATTERN_TIP (tips are vectors on the device), at --vector-sites
              sites: the traffic model is tips * sites * states * 8 bytes (rate 0 only).  Baseline: every tip vector
              copied down (pllhip_get_clv) and the same loops in numpy.

Shapes are the tip shapes of the benchmark configurations: c2 = 100 x 1 M DNA, c3 = 200 x 1 M protein, c5 = 50 x
200 k at 61 states; characters are iid with a few percent ambiguity codes and gaps.

usage: python tools/gpu_msa_stats.py [--shapes c2,c3,c5] [--forms partition,alignment,vectors] [--repeat N]
                                     [--vector-sites N] [--no-baseline] [--seed S] [--out FILE.jsonl]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pll-modules_amd"))
import pllhip_ctypes as pc  # noqa: E402

PEAK = 8e12
DNA = b"ACGT" * 12 + b"RYN-"
AA = b"ARNDCQEGHILKMFPSTWYV" * 3 + b"BZX-"
S61 = bytes(range(48, 48 + 61)) * 2 + b"-!"
SHAPES = {"c2": (4, 100, 1_000_000, "nt"), "c3": (20, 200, 1_000_000, "aa"), "c5": (61, 50, 200_000, "s61")}


def alphabet(lib, name):
    if name == "nt":
        return lib.char_map("pll_map_nt"), DNA
    if name == "aa":
        return lib.char_map("pll_map_aa"), AA
    m = [0] * 256
    for k in range(61):
        m[48 + k] = 1 << k
    m[ord("-")] = (1 << 61) - 1
    m[ord("!")] = (1 << 3) | (1 << 40)
    return m, S61


def median_ms(fn, repeat):
    """(median wall ms, last result, median kernel ms) of fn(); the first call warms up"""
    wall, kern, res = [], [], None
    for r in range(repeat + 1):
        t0 = time.perf_counter()
        res = fn()
        dt = (time.perf_counter() - t0) * 1e3
        if r:
            wall.append(dt)
            kern.append(LIB.msa_stats_last_times()[1])
    return float(np.median(wall)), res, float(np.median(kern))


def numpy_loops(masks_of_tip, T, L, S, w):
    """frequencies and exchangeabilities the way pll_msa.c walks the tips, in numpy: per tip the state masks of its
    sites, per state a pass over them"""
    full = np.uint64((1 << S) - 1)
    cnt = np.zeros((S, L), dtype=np.int64)
    freq = np.zeros(S)
    for t in range(T):
        m, gap = masks_of_tip(t)
        pop = np.zeros(L, dtype=np.int64)
        bits = []
        for k in range(S):
            b = ((m >> np.uint64(k)) & np.uint64(1)).astype(np.int64)
            bits.append(b)
            pop += b
        share = w / np.maximum(pop, 1)
        keep = ~(m == full if gap is None else gap)
        for k in range(S):
            freq[k] += float(np.dot(bits[k], share))
            cnt[k] += bits[k] * keep
    freq /= float(w.sum()) * T
    pair = (cnt * w.astype(np.int64)) @ cnt.T
    return freq, pair[np.triu_indices(S, 1)]


def build(lib, S, T, L, cmap, chars, seed, coded):
    rng = np.random.default_rng(seed)
    inst = pc.Instance(lib, T, S, L, 4, attributes=pc.PLL_ATTRIB_PATTERN_TIP if coded else 0, scalers=False,
                       prob_matrices=1, clv_buffers=1)
    rows = []
    for t in range(T):
        row = rng.choice(np.frombuffer(chars, dtype=np.uint8), size=L)
        inst.set_tip_states(t, cmap, row.tobytes())
        rows.append(row)
    w = rng.integers(1, 4, size=L).astype(np.uint32)
    inst.set_pattern_weights(w)
    return inst, rows, w


def rates_of(pairs):
    last = float(pairs[-1]) if pairs[-1] else 1.0
    out = np.clip(pairs.astype(np.float64) / last, 0.01, 50.0)
    out[-1] = 1.0
    return out


def run_partition(lib, name, S, T, L, cmap, chars, a, coded):
    inst, rows, w = build(lib, S, T, L, cmap, chars, a.seed, coded)
    with inst:
        f_ms, freqs, f_kern = median_ms(lambda: lib.empirical_frequencies(inst.p), a.repeat)
        r_ms, rates, r_kern = median_ms(lambda: lib.empirical_subst_rates(inst.p), a.repeat)
        if freqs is None or rates is None:
            raise RuntimeError(f"[{lib.errno}] {lib.errmsg}")
        p = inst.p.contents
        t0 = time.perf_counter()
        if a.no_baseline:
            base = None
        elif coded:
            tipmap = np.ctypeslib.as_array(p.tipmap, shape=(256,)).astype(np.uint64)
            base = numpy_loops(lambda t: (tipmap[np.ctypeslib.as_array(p.tipchars[t], shape=(L,))], None), T, L, S, w)
        else:
            buf = np.zeros((L, 4, p.states_padded))

            def vector_tip(t):
                if not lib.lib.pllhip_get_clv(inst.p, t, buf.ctypes.data_as(pc.c_double_p)):
                    raise RuntimeError(lib.errmsg)
                v = buf[:, 0, :S]
                m = np.zeros(L, dtype=np.uint64)
                for k in range(S):
                    m |= (v[:, k] > 0).astype(np.uint64) << np.uint64(k)
                return m, np.all(v >= 1e-7, axis=1)
            base = numpy_loops(vector_tip, T, L, S, w)
        base_ms = (time.perf_counter() - t0) * 1e3
        if base is not None and not (np.allclose(base[0], freqs, rtol=1e-9) and np.array_equal(rates_of(base[1]), rates)):
            raise RuntimeError(f"{name}: the numpy baseline and the device disagree")
    model = float(T) * L * (1 if coded else S * 8)
    return {"shape": name, "form": "partition" if coded else "vectors", "states": S, "taxa": T, "sites": L,
            "frequencies_ms": round(f_ms, 3), "frequencies_kernel_ms": round(f_kern, 4),
            "subst_rates_ms": round(r_ms, 3), "subst_rates_kernel_ms": round(r_kern, 4),
            "baseline_numpy_ms": None if base is None else round(base_ms, 1), "model_bytes": model,
            "model_ms_at_8TBps": round(model / PEAK * 1e3, 4),
            "kernel_frac_of_8TBps": round(model / (f_kern * 1e-3) / PEAK, 4)}


def run_alignment(lib, name, S, T, L, cmap, chars, a):
    rng = np.random.default_rng(a.seed)
    bufs = [C.create_string_buffer(rng.choice(np.frombuffer(chars, dtype=np.uint8), size=L).tobytes(), L + 1)
            for _ in range(T)]
    seqs = (C.c_void_p * T)(*[C.addressof(b) for b in bufs])
    msa = pc.Msa(T, L, seqs, None)
    cmap = (C.c_ulonglong * 256)(*[int(x) for x in cmap])
    w = rng.integers(1, 4, size=L).astype(np.uint32)
    mask = pc.MSA_STATS_ALL & ~(pc.MSA_STATS_DUP_TAXA | pc.MSA_STATS_DUP_SEQS)
    parts = []

    def call():
        st = lib.lib.pllhip_msa_compute_stats(C.byref(msa), S, cmap, w.ctypes.data_as(pc.c_uint_p), mask)
        if not st:
            raise RuntimeError(f"[{lib.errno}] {lib.errmsg}")
        lib.lib.pllhip_msa_destroy_stats(st)
        parts.append(lib.msa_stats_last_times())
        return True
    ms, _, kern = median_ms(call, a.repeat)
    up = float(np.median([p[0] for p in parts[1:]]))
    model = float(T) * L
    return {"shape": name, "form": "alignment", "states": S, "taxa": T, "sites": L, "call_ms": round(ms, 3),
            "upload_ms": round(up, 3), "kernel_ms": round(kern, 4), "upload_GBps": round(model / (up * 1e-3) / 1e9, 2),
            "model_bytes": model, "model_ms_at_8TBps": round(model / PEAK * 1e3, 4),
            "kernel_frac_of_8TBps": round(model / (kern * 1e-3) / PEAK, 4)}


def main():
    global LIB
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c2,c3,c5")
    ap.add_argument("--forms", default="partition,alignment,vectors")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--vector-sites", type=int, default=65536)
    ap.add_argument("--no-baseline", action="store_true", help="skip the numpy baseline")
    ap.add_argument("--seed", type=int, default=17)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    a = ap.parse_args()
    LIB = lib = pc.PllLib(pc.PRODUCT_LIB)
    if lib.lib.pllhip_device_count() < 1:
        raise SystemExit("no HIP device visible: this tool measures on the GPU only")
    for name in a.shapes.split(","):
        S, T, L, alpha = SHAPES[name]
        cmap, chars = alphabet(lib, alpha)
        for form in a.forms.split(","):
            if form == "partition":
                res = run_partition(lib, name, S, T, L, cmap, chars, a, True)
            elif form == "vectors":
                res = run_partition(lib, name, S, T, min(L, a.vector_sites), cmap, chars, a, False)
            else:
                res = run_alignment(lib, name, S, T, L, cmap, chars, a)
            line = json.dumps(res)
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")


LIB = None

if __name__ == "__main__":
    main()
