"""Times pll_fastparsimony_stepwise at the C2, C3 and C5 shapes on device 0 and prints one JSON line per shape:
wall time of the stepwise call, the bytes of the traffic model in DESIGN.md ("Parsimony") and the fraction of
8 TB/s they stand for.  Alignments are simulated along a random tree (pllhip_ctypes.simulated_codes), tips coded
(PLL_ATTRIB_PATTERN_TIP), unit weights.

With --spr it times, per shape, one unconstrained pll_fastparsimony_stepwise_spr_round on the stepwise tree instead:
round_ms, prunes, whether the tree changed (the API does not count moves), the batch, the bytes of the round's
traffic model (about 2N prunes x 2N edges x 5 vectors) and the fraction of 8 TB/s they stand
for.

usage: python tools/gpu_parsimony.py [--shapes c2,c3,c5] [--repeat N] [--seed S] [--spr]"""
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

SHAPES = {"c2": (100, 1_000_000, 4), "c3": (200, 1_000_000, 20), "c5": (50, 200_000, 61)}
PEAK = 8e12


def run(lib, name, tips, sites, S, repeat, seed):
    L = lib.lib
    tree = pc.Tree(tips, seed_topology=seed)
    codes = pc.simulated_codes(tree, sites, S, seed=seed + 1)
    inst = pc.Instance(lib, tips, S, sites, 1, attributes=pc.PLL_ATTRIB_PATTERN_TIP, clv_buffers=0,
                       prob_matrices=1, scalers=False)
    charmap = pc.state_charmap(S)
    with inst:
        for t in range(tips):
            inst.set_tip_states(t, charmap, (codes[t] + 48).tobytes())
        t0 = time.perf_counter()
        p = L.pll_fastparsimony_init(inst.p)
        init_ms = (time.perf_counter() - t0) * 1e3
    if not p:
        raise RuntimeError(lib.errmsg)
    arr = (C.c_void_p * 1)(p)
    times, score = [], C.c_uint(0)
    for r in range(repeat + 1):                  # the first call warms up
        t0 = time.perf_counter()
        tr = L.pll_fastparsimony_stepwise(arr, None, C.byref(score), 1, seed + r)
        dt = (time.perf_counter() - t0) * 1e3
        if not tr:
            raise RuntimeError(lib.errmsg)
        L.pll_utree_destroy(tr, None)
        if r:
            times.append(dt)
    L.pll_parsimony_destroy(p)
    ms = float(np.median(times))
    model = float(tips) ** 2 * sites * S / 8
    return {"shape": name, "tips": tips, "sites": sites, "states": S, "steps": tips - 3, "ms": round(ms, 3),
            "ms_min": round(min(times), 3), "init_ms": round(init_ms, 3), "score": score.value,
            "model_bytes": model, "model_frac_of_8TBps": round(model / (ms * 1e-3) / PEAK, 4)}


def run_spr(lib, name, tips, sites, S, seed):
    L = lib.lib
    tree = pc.Tree(tips, seed_topology=seed)
    codes = pc.simulated_codes(tree, sites, S, seed=seed + 1)
    inst = pc.Instance(lib, tips, S, sites, 1, attributes=pc.PLL_ATTRIB_PATTERN_TIP, clv_buffers=0,
                       prob_matrices=1, scalers=False)
    charmap = pc.state_charmap(S)
    with inst:
        for t in range(tips):
            inst.set_tip_states(t, charmap, (codes[t] + 48).tobytes())
        p = L.pll_fastparsimony_init(inst.p)
    if not p:
        raise RuntimeError(lib.errmsg)
    arr = (C.c_void_p * 1)(p)
    score, cost = C.c_uint(0), C.c_uint(0)
    tr = L.pll_fastparsimony_stepwise(arr, None, C.byref(score), 1, seed)
    if not tr:
        raise RuntimeError(lib.errmsg)
    nwk0 = C.string_at(L.pll_utree_export_newick(tr.contents.vroot, None)).decode()
    t0 = time.perf_counter()
    ok = L.pll_fastparsimony_stepwise_spr_round(tr, arr, 1, None, seed, None, C.byref(cost))
    ms = (time.perf_counter() - t0) * 1e3
    if not ok:
        raise RuntimeError(lib.errmsg)
    nwk1 = C.string_at(L.pll_utree_export_newick(tr.contents.vroot, None)).decode()
    L.pll_utree_destroy(tr, None)
    L.pll_parsimony_destroy(p)
    nw = -(-(-(-sites // 32)) // 64) * 64
    batch = int(os.environ.get("PLLHIP_PARS_SPR_BATCH", "0")) or min(64, -(-2048 // (nw // 64)))
    prunes = 2 * tips - 4
    model = float(prunes) * (2 * tips - 2) * 5 * S * nw * 4
    return {"shape": name, "tips": tips, "sites": sites, "states": S, "round_ms": round(ms, 3), "prunes": prunes,
            "tree_changed": nwk0 != nwk1, "stepwise_score": score.value, "round_score": cost.value,
            "batch": batch, "model_bytes": model, "frac": round(model / (ms * 1e-3) / PEAK, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c2,c3,c5")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--seed", type=int, default=17)
    ap.add_argument("--spr", action="store_true")
    a = ap.parse_args()
    lib = pc.PllLib(pc.PRODUCT_LIB)
    for name in a.shapes.split(","):
        res = run_spr(lib, name, *SHAPES[name], a.seed) if a.spr else run(lib, name, *SHAPES[name], a.repeat, a.seed)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
