"""Times the three stages of pllhip_sitelh_rell on device 0 and prints one JSON line per case:

  unit        T trees x S patterns, B replicates, unit weights (N = S draws per replicate)
  compressed  the same sizes with the weights of a compressed alignment: geometric weights (mean --mean-weight), a
              few heavy patterns, so N = a multiple of S and the draws go through the binary search

Per line: the stage times between device events (pllhip_rell_last_times; median of --repeat calls after a warm-up),
the wall time of the call, and each stage's share of its roof:

  draw      B * N counter draws, each one 4-byte atomic increment, plus B * S * 4 bytes cleared; roof: the HBM rate
            (8 TB/s) over those bytes -- a lower bound no atomic path reaches, printed to show the distance
  product   2 * B16 * S16 * T16 flops (the padded operands) at the sustained FP64 matrix rate the chip holds under a
            full load (47.5 TFLOP/s), and its bytes at 8 TB/s: counts read once per 128 trees,
            rows of L once per 64 replicates, chunk partials written and read once
  stats     B * T * 8 bytes of R read three times, E written and read once, at 8 TB/s

No GPU, no numbers: the tool fails.

usage: python tools/gpu_rell.py [--trees T] [--patterns S] [--replicates B] [--batch N] [--repeat N]
                                [--cases unit,compressed] [--mean-weight W] [--out FILE.jsonl]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pll-modules_amd"))
import pllhip_ctypes as pc  # noqa: E402

HBM = 8e12
FP64_MATRIX = 47.5e12


def pad16(n):
    return (n + 15) // 16 * 16


def chunk_len(S):
    return pad16(max(1024, (S + 63) // 64))


def weights_of(case, S, mean_weight):
    if case == "unit":
        return None
    rng = np.random.default_rng(12)
    w = rng.geometric(1.0 / mean_weight, S).astype(np.uint32)
    w[rng.integers(0, S, 8)] = 70000
    return w


def run(lib, case, T, S, B, batch, repeat, mean_weight):
    rng = np.random.default_rng(11)
    w = weights_of(case, S, mean_weight)
    N = S if w is None else int(w.astype(np.int64).sum())
    base = -rng.gamma(2.0, 4.0, S)
    with pc.SiteLikelihoods(lib, S, w) as sl:
        if not sl.h:
            raise RuntimeError(lib.errmsg)
        for t in range(T):
            if sl.add(base + 0.3 * rng.standard_normal(S)) != t:
                raise RuntimeError(lib.errmsg)
        times, wall, res = [], [], None
        for r in range(repeat + 1):                       # round 0 warms up
            t0 = time.perf_counter()
            res = sl.rell(B, 1234, 0, batch)
            dt = (time.perf_counter() - t0) * 1e3
            if res is None:
                raise RuntimeError(lib.errmsg)
            if r:
                times.append(res.times)
                wall.append(dt)
    draw, product, stats = (float(x) for x in np.median(np.array(times), axis=0))
    B16, S16, T16 = pad16(B), pad16(S), pad16(T)
    nchunks = (S16 + chunk_len(S) - 1) // chunk_len(S)
    draw_bytes = B * S16 * 4 + B * N * 4
    flops = 2.0 * B16 * S16 * T16
    product_bytes = (B16 * S16 * 4 * ((T16 + 127) // 128) + T16 * S16 * 8 * ((B16 + 63) // 64)
                     + 2 * nchunks * B16 * T16 * 8)
    stats_bytes = 5 * B * T * 8
    return {"case": case, "trees": T, "patterns": S, "replicates": B, "draws_per_replicate": N, "batch": int(res.batch),
            "passes": (B + res.batch - 1) // res.batch, "chunks": nchunks, "repeat": repeat,
            "wall_ms": float(np.median(wall)), "draw_ms": draw, "product_ms": product, "stats_ms": stats,
            "draw_bytes": draw_bytes, "draw_share_of_hbm_roof": draw_bytes / HBM * 1e3 / draw,
            "draws_per_ns": B * N / (draw * 1e6),
            "product_flops": flops, "product_tflops": flops / (product * 1e9),
            "product_share_of_fp64_matrix_roof": flops / FP64_MATRIX * 1e3 / product,
            "product_bytes": product_bytes, "product_share_of_hbm_roof": product_bytes / HBM * 1e3 / product,
            "stats_share_of_hbm_roof": stats_bytes / HBM * 1e3 / stats,
            "best": int(res.best), "bp_of_best": int(res.bp_count[res.best])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trees", type=int, default=100)
    ap.add_argument("--patterns", type=int, default=1_000_000)
    ap.add_argument("--replicates", type=int, default=1000)
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--cases", default="unit,compressed")
    ap.add_argument("--mean-weight", type=float, default=4.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = pc.PllLib(pc.PRODUCT_LIB)
    if lib.lib.pllhip_device_count() < 1:
        raise SystemExit("gpu_rell.py: no HIP device visible; there is no fallback")
    out = open(a.out, "a") if a.out else None
    for case in a.cases.split(","):
        line = json.dumps(run(lib, case, a.trees, a.patterns, a.replicates, a.batch, a.repeat, a.mean_weight))
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    if out:
        out.close()


if __name__ == "__main__":
    main()
