"""Times pll_compress_site_patterns_msa on device 0 and prints one JSON line per shape: the median of the whole call
(wall clock around the library call), its split into upload / kernels / download from the HIP events of the call
(pllhip_compress_last_times; "kernels" is the sum of the two device segments, without the host's read of the pattern
count between them), the table's probe steps and full column compares (pllhip_compress_last_counts), and the kernel
time against the byte model of DESIGN.md section 14:

    T L              the hash pass reads every character once
  + 2 T (L - P)      every site that joins a group compares its column with the owner's
  + 2 T P            the gather reads and writes the first occurrences
  + 8 slots + 40 L   the table (set to empty once) and the per-site arrays

as a fraction of 8 TB/s.  Shapes: c2 = 100 x 1 M DNA, c3 = 200 x 1 M protein, every column drawn from L / 2 random
columns (about 43 % of the sites are first occurrences); ident = 100 x 1 M identical columns; c3u = 200 x 1 M protein
with iid characters (every column distinct: no compare runs, so c3 - c3u is what the compares of c3 cost).

usage: python tools/gpu_compress.py [--shapes c2,c3,c3u,ident] [--repeat N] [--seed S] [--out FILE.jsonl]"""
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

DNA = b"ACGTacgtACGTacgt-N?RY"
AA = b"ARNDCQEGHILKMFPSTWYVARNDCQEGHILKMFPSTWYVarndcqeghilkmfpstwyvBZX*-?"
SHAPES = {"c2": (100, 1_000_000, DNA, "pll_map_nt", 0.5), "c3": (200, 1_000_000, AA, "pll_map_aa", 0.5),
          "ident": (100, 1_000_000, DNA, "pll_map_nt", 0.0), "c3u": (200, 1_000_000, AA, "pll_map_aa", None)}
PEAK = 8e12


def draw(rng, alphabet, T, L, share):
    if share is None:                            # iid characters
        return rng.choice(np.frombuffer(alphabet, dtype=np.uint8), size=(T, L))
    npat = max(1, int(L * share))
    base = rng.choice(np.frombuffer(alphabet, dtype=np.uint8), size=(T, npat))
    return np.ascontiguousarray(base[:, rng.integers(0, npat, size=L)])


def run(lib, name, T, L, alphabet, mapname, share, repeat, seed):
    rows = draw(np.random.default_rng(seed), alphabet, T, L, share)
    cmap = lib.char_map(mapname)
    spm = np.zeros(L, dtype=np.uint32)
    wall, parts, P = [], [], 0
    for r in range(repeat + 1):                  # the first call warms up
        bufs = [C.create_string_buffer(rows[t].tobytes(), L + 1) for t in range(T)]
        seqs = (C.c_void_p * T)(*[C.addressof(b) for b in bufs])
        msa = pc.Msa(T, L, seqs, None)
        t0 = time.perf_counter()
        w = lib.lib.pll_compress_site_patterns_msa(C.byref(msa), cmap, spm.ctypes.data_as(pc.c_uint_p))
        dt = (time.perf_counter() - t0) * 1e3
        if not w:
            raise RuntimeError(f"[{lib.errno}] {lib.errmsg}")
        P = msa.length
        total = int(np.ctypeslib.as_array(w, shape=(P,)).sum(dtype=np.uint64))
        pc._libc_free(w)
        if total != L:
            raise RuntimeError(f"weights sum to {total}, not {L}")
        if r:
            wall.append(dt)
            parts.append(lib.compress_last_times())
            probes, compares = lib.compress_last_counts()
    up, kern, down = (float(np.median([p[k] for p in parts])) for k in range(3))
    slots = 2
    while slots < 2 * L:
        slots *= 2
    model = float(T) * L + 2.0 * T * (L - P) + 2.0 * T * P + 8.0 * slots + 40.0 * L
    return {"shape": name, "taxa": T, "sites": L, "patterns": P, "call_ms": round(float(np.median(wall)), 3),
            "call_ms_min": round(min(wall), 3), "upload_ms": round(up, 3), "kernel_ms": round(kern, 3),
            "download_ms": round(down, 3), "host_ms": round(float(np.median(wall)) - up - kern - down, 3),
            "probe_steps": probes, "compares": compares,
            "upload_GBps": round(T * L / (up * 1e-3) / 1e9, 2), "model_bytes": model,
            "kernel_frac_of_8TBps": round(model / (kern * 1e-3) / PEAK, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c2,c3,c3u,ident")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--seed", type=int, default=17)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    a = ap.parse_args()
    lib = pc.PllLib(pc.PRODUCT_LIB)
    if lib.lib.pllhip_device_count() < 1:
        raise SystemExit("no HIP device visible: this tool measures on the GPU only")
    for name in a.shapes.split(","):
        res = run(lib, name, *SHAPES[name], a.repeat, a.seed)
        line = json.dumps(res)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
