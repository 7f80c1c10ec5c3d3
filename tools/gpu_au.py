"""Times the three stages of pllhip_sitelh_au on device 0, and pllhip_sitelh_rell on the same set in the same session
as the yardstick, and prints one JSON line per case:

  unit        T trees x S patterns, B replicates per scale, unit weights (N = S)
  compressed  the same sizes with the weights of a compressed alignment: geometric weights (mean --mean-weight), a
              few heavy patterns, so N = a multiple of S and the draws go through the bucket table and the search

Per line: the stage times between device events (pllhip_au_last_times and pllhip_rell_last_times; median of --repeat
calls after a warm-up), the wall time of the calls, the draw rate, and the ratio of the AU call's device time to the
RELL call's next to the modelled ratio sum_k n_k / N (9.5 for the default scales: the draws dominate both calls, and
the AU test makes that many times as many).

No GPU, no numbers: the tool fails.

usage: python tools/gpu_au.py [--trees T] [--patterns S] [--replicates B] [--batch N] [--repeat N]
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


def pad16(n):
    return (n + 15) // 16 * 16


def weights_of(case, S, mean_weight):
    if case == "unit":
        return None
    rng = np.random.default_rng(12)
    w = rng.geometric(1.0 / mean_weight, S).astype(np.uint32)
    w[rng.integers(0, S, 8)] = 70000
    return w


def timed(call, repeat):
    """(median stage times, median wall ms, last result) of repeat calls after a warm-up"""
    times, wall, res = [], [], None
    for r in range(repeat + 1):
        t0 = time.perf_counter()
        res = call()
        dt = (time.perf_counter() - t0) * 1e3
        if res is None:
            return None
        if r:
            times.append(res.times)
            wall.append(dt)
    return [float(x) for x in np.median(np.array(times), axis=0)], float(np.median(wall)), res


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
        rell = timed(lambda: sl.rell(B, 1234, 0, batch), repeat)
        au = timed(lambda: sl.au(B, 1234, None, 0, batch), repeat)
        if rell is None or au is None:
            raise RuntimeError(lib.errmsg)
    (rdraw, rproduct, rstats), rwall, _ = rell
    (draw, product, stats), wall, res = au
    draws = int(res.draws.sum())
    rows = res.scales * B
    return {"case": case, "trees": T, "patterns": S, "replicates": B, "scales": int(res.scales), "sites": N,
            "draws_per_scale": [int(n) for n in res.draws], "batch": int(res.batch),
            "passes": (rows + res.batch - 1) // res.batch, "repeat": repeat,
            "wall_ms": wall, "draw_ms": draw, "product_ms": product, "stats_ms": stats,
            "draws_per_ns": B * draws / (draw * 1e6),
            "product_tflops": 2.0 * pad16(rows) * pad16(S) * pad16(T) / (product * 1e9),
            "rell_wall_ms": rwall, "rell_draw_ms": rdraw, "rell_product_ms": rproduct, "rell_stats_ms": rstats,
            "rell_draws_per_ns": B * N / (rdraw * 1e6),
            "ratio_to_rell": (draw + product + stats) / (rdraw + rproduct + rstats),
            "ratio_to_rell_draws_only": draw / rdraw, "modelled_ratio": draws / N,
            "best": int(res.best), "p_au_of_best": float(res.p_au[res.best]), "used_of_best": int(res.used[res.best])}


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
        raise SystemExit("gpu_au.py: no HIP device visible; there is no fallback")
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
