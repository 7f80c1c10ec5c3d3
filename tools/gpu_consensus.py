"""Times the consensus of a tree set (pllhip_treeset_consensus) on device 0 and prints one JSON
line per shape.

The B trees are one random tree of T tips after --moves random prune-and-regraft moves of a tip each (the trees of
tools/gpu_tree_support.py).  Per repetition a fresh set takes the trees and answers one query, so that the splits are
resident; then
  mr    majority rule (threshold 0.5): candidates, ranking, the majority taken as it stands
  mre   extended majority rule (threshold 0.0): every distinct split ranked, then the greedy selection in rounds
upload / kernel / download are pllhip_treeset_last_times, wall is the whole call; the two counters are
pllhip_treeset_last_consensus_counts (candidate-accepted tests, pairwise tests).  Medians over --repeat repetitions.

The reference's single-thread seconds for the same (T, B) come from `record_consensus time T B`
(tests/golden/record_consensus.c) on the build machine.

usage: python tools/gpu_consensus.py [--shapes 200x100,1000x200,1000x1000] [--repeat 3] [--moves 10] [--seed 1]"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pll-modules_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import pllhip_ctypes as pc  # noqa: E402
from gpu_tree_support import Topology  # noqa: E402


def run(lib, T, B, repeat, moves, seed):
    rng = random.Random(seed)
    labels = ["x%d" % i for i in range(T)]
    base = Topology(T, rng)
    newicks = [base.moved(moves, rng).newick() for _ in range(B)]
    rows = {"%s_%s_ms" % (m, k): [] for m in ("mr", "mre") for k in ("upload", "kernel", "download", "wall")}
    res = {"tips": T, "trees": B, "moves": moves, "repeat": repeat}
    for _ in range(repeat):
        with pc.TreeSet(lib, T, labels) as ts:
            for n in newicks:
                if not ts.add(n):
                    raise RuntimeError(lib.errmsg)
            if ts.splits(0) is None:                           # the trees go to the device here
                raise RuntimeError(lib.errmsg)
            res["ingest_kernel_ms"] = round(ts.last_times()[1], 3)
            for mode, cut in (("mr", 0.5), ("mre", 0.0)):
                t0 = time.perf_counter()
                out = ts.consensus(cut)
                wall = (time.perf_counter() - t0) * 1e3
                if out is None:
                    raise RuntimeError(lib.errmsg)
                for k, v in zip(("upload", "kernel", "download", "wall"), ts.last_times() + (wall,)):
                    rows["%s_%s_ms" % (mode, k)].append(v)
                res[mode + "_splits"] = len(out[0])
                res[mode + "_accepted_tests"], res[mode + "_pair_tests"] = ts.last_consensus_counts()
    res.update({k: round(float(np.median(v)), 3) for k, v in rows.items()})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="200x100,1000x200,1000x1000")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--moves", type=int, default=10)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    sys.setrecursionlimit(20000)
    lib = pc.PllLib(pc.PRODUCT_LIB)
    for shape in a.shapes.split(","):
        T, B = (int(v) for v in shape.split("x"))
        print(json.dumps(run(lib, T, B, a.repeat, a.moves, a.seed)), flush=True)


if __name__ == "__main__":
    main()
