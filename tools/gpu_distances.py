"""Times pairwise distances and neighbour joining on device 0 and prints one JSON line per shape (DESIGN.md section
23):

  pllhip_distances_msa (JC) on raw rows: wall clock of the call (median of --repeat) and the stages of
  pllhip_distances_last_times -- rows and site list up, the code kernel, the integer product, the distance kernel.
  The product is held against its own operation count: 2 * 64 * 64 * columns integer operations per tile on or above
  the diagonal (what the kernel issues, padding included).
  pllhip_distmat_nj on the result: wall clock, launches included.
  Baseline: the only route the parent of this feature offers for the same counts, X diag(w) X^T in numpy (float64
  BLAS, exact here), on the first --baseline-sites sites; its time is reported with that site count, not scaled.

Shapes are the tip shapes of the benchmark configurations: c2 = 100 x 1 M DNA, c3 = 200 x 1 M protein, c5 = 50 x
200 k at 61 states; characters are iid with a few percent ambiguity codes and gaps, weights 1 .. 3.

usage: python tools/gpu_distances.py [--shapes c2,c3,c5] [--repeat N] [--baseline-sites N] [--seed S] [--out FILE.jsonl]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pll-modules_amd"))
import pllhip_ctypes as pc  # noqa: E402

DNA = b"ACGT" * 12 + b"RYN-"
AA = b"ARNDCQEGHILKMFPSTWYV" * 3 + b"BZX-"
S61 = bytes(range(48, 48 + 61)) * 2 + b"-!"
TILE = 64          # rows and columns of a wave's tile (DST_TILE of csrc/kernels_distance.hpp)
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


def numpy_counts(rows, cmap, S, w):
    """N as [T * S][T * S] float64 (exact: every sum is far below 2^53)"""
    table = np.array([int(x) for x in cmap], dtype=np.uint64) & np.uint64((1 << S) - 1)
    masks = table[rows]
    X = np.stack([(masks == np.uint64(1 << k)) for k in range(S)], axis=1).astype(np.float64).reshape(-1, rows.shape[1])
    return (X * w[None, :].astype(np.float64)) @ X.T


def run(lib, name, a):
    S, T, L, alpha = SHAPES[name]
    cmap, chars = alphabet(lib, alpha)
    rng = np.random.default_rng(a.seed)
    rows = rng.choice(np.frombuffer(chars, dtype=np.uint8), size=(T, L))
    w = rng.integers(1, 4, size=L).astype(np.uint32)
    wall, stages, nj_ms, dm = [], [], [], None
    for r in range(a.repeat + 1):
        if dm is not None:
            dm.close()
        t0 = time.perf_counter()
        dm = pc.distances_msa(lib, rows, S, cmap, w, method=pc.DIST_JC, flags=pc.DIST_KEEP_COUNTS if r == 0 else 0)
        dt = (time.perf_counter() - t0) * 1e3
        if dm is None:
            raise RuntimeError(f"[{lib.errno}] {lib.errmsg}")
        if r == 0:
            base_sites = min(L, a.baseline_sites)
            t0 = time.perf_counter()
            base = numpy_counts(rows[:, :base_sites], cmap, S, w[:base_sites]) if base_sites else None
            base_ms = (time.perf_counter() - t0) * 1e3
            if base is not None and base_sites == L:
                for i, j in ((0, 1), (T - 1, 2), (3, 3)):
                    if not np.array_equal(dm.counts(i, j), base[i * S:(i + 1) * S, j * S:(j + 1) * S].astype(np.int32)):
                        raise RuntimeError(f"{name}: the numpy baseline and the device disagree on block ({i}, {j})")
            continue
        wall.append(dt)
        stages.append(dm.last_times()[:4])
        t0 = time.perf_counter()
        if dm.nj_joins() is None:
            raise RuntimeError(f"[{lib.errno}] {lib.errmsg}")
        nj_ms.append((time.perf_counter() - t0) * 1e3)
    dm.close()
    up, codes, counts, estimate = (float(np.median([s[k] for s in stages])) for k in range(4))
    columns = (L + 63) // 64 * 64                         # (weights up to 127: one staged column per site)
    tiles = (T * S + TILE - 1) // TILE
    ops = 2.0 * TILE * TILE * columns * (tiles * (tiles + 1) // 2)
    return {"shape": name, "states": S, "taxa": T, "sites": L, "call_ms": round(float(np.median(wall)), 3),
            "upload_ms": round(up, 3), "codes_ms": round(codes, 4), "counts_ms": round(counts, 4),
            "estimate_ms": round(estimate, 4), "nj_ms": round(float(np.median(nj_ms)), 3),
            "gram_int_ops": ops, "gram_Tops": round(ops / (counts * 1e-3) / 1e12, 3),
            "baseline_numpy_ms": None if base is None else round(base_ms, 1), "baseline_sites": base_sites}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c2,c3,c5")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--baseline-sites", type=int, default=20000, help="sites of the numpy baseline (0: none)")
    ap.add_argument("--seed", type=int, default=17)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    a = ap.parse_args()
    lib = pc.PllLib(pc.PRODUCT_LIB)
    if lib.lib.pllhip_device_count() < 1:
        raise SystemExit("no HIP device visible: this tool measures on the GPU only")
    for name in a.shapes.split(","):
        line = json.dumps(run(lib, name, a))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
