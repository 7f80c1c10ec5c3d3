"""Times the tree set (pllhip_treeset_*) on device 0 and prints one JSON line per shape.

A reference tree of T tips is drawn by random insertion; each of the B trees is the reference after --moves random
prune-and-regraft moves of a tip.  Per repetition a fresh set takes the B trees (add_ms: the host's flattening, Newick
parsing included), then
  first   TBE support on the fresh set: the trees go to the device (plans and programs up, splits, table, ids) and
          the transfer kernel runs; upload / kernel / download are pllhip_treeset_last_times
  tbe     the same call again: the transfer kernel alone, and its rate against the model of section 16,
          (T-3) * B * (2T-3) lane steps
  fbp, rf_to, rf_matrix   the other queries on the resident set
Medians over --repeat repetitions.

usage: python tools/gpu_tree_support.py [--shapes 500x100,2000x1000,5000x200] [--repeat 3] [--moves 10] [--seed 1]"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pll-modules_amd"))
import pllhip_ctypes as pc  # noqa: E402


class Topology:
    """an unrooted binary tree as child lists: node 2T-3 is the top (three children), tips are 0 .. T-1"""

    def __init__(self, T, rng):
        self.T, self.top = T, 2 * T - 3
        self.kids, self.parent = {self.top: [0, 1, 2]}, {0: self.top, 1: self.top, 2: self.top}
        for tip in range(3, T):
            self._graft(tip, T + tip - 3, rng.choice(list(self.parent)))

    def _graft(self, tip, inner, at):
        p = self.parent[at]
        self.kids[p][self.kids[p].index(at)] = inner
        self.kids[inner] = [at, tip]
        self.parent.update({inner: p, at: inner, tip: inner})

    def moved(self, moves, rng):
        """a copy with `moves` tips pruned and regrafted"""
        c = object.__new__(Topology)
        c.T, c.top, c.kids, c.parent = self.T, self.top, {k: v[:] for k, v in self.kids.items()}, dict(self.parent)
        nodes = list(c.parent)
        while moves:
            tip = rng.randrange(c.T)
            p = c.parent[tip]
            if p == c.top:
                continue
            at = rng.choice(nodes)
            if at in (tip, p):
                continue
            sibling = [k for k in c.kids[p] if k != tip][0]
            g = c.parent[p]
            c.kids[g][c.kids[g].index(p)] = sibling
            c.parent[sibling] = g
            c._graft(tip, p, at)
            moves -= 1
        return c

    def newick(self):
        def text(n):
            return "x%d" % n if n < self.T else "(" + ",".join(text(k) for k in self.kids[n]) + ")"
        return text(self.top) + ";"


def run(lib, T, B, repeat, moves, seed):
    rng = random.Random(seed)
    labels = ["x%d" % i for i in range(T)]
    ref = Topology(T, rng)
    ref_newick = ref.newick()
    newicks = [ref.moved(moves, rng).newick() for _ in range(B)]
    keys = ("add_ms", "first_upload_ms", "first_kernel_ms", "first_download_ms", "first_wall_ms", "tbe_upload_ms",
            "tbe_kernel_ms", "tbe_download_ms", "tbe_wall_ms", "fbp_wall_ms", "rf_to_wall_ms", "rf_matrix_wall_ms",
            "rf_matrix_kernel_ms")
    rows = {k: [] for k in keys}
    mean_tbe = mean_fbp = None
    for _ in range(repeat):
        with pc.TreeSet(lib, T, labels) as ts:
            t0 = time.perf_counter()
            for n in newicks:
                if not ts.add(n):
                    raise RuntimeError(lib.errmsg)
            rows["add_ms"].append((time.perf_counter() - t0) * 1e3)
            for phase in ("first", "tbe"):
                t0 = time.perf_counter()
                res = ts.support(ref_newick, pc.SUPPORT_TBE)
                wall = (time.perf_counter() - t0) * 1e3
                if res is None:
                    raise RuntimeError(lib.errmsg)
                up, kern, down = ts.last_times()
                for k, v in zip(("upload", "kernel", "download", "wall"), (up, kern, down, wall)):
                    rows["%s_%s_ms" % (phase, k)].append(v)
            mean_tbe = float(res[0].mean())
            probes, compares = ts.last_counts()
            for name, call in (("fbp", lambda: ts.support(ref_newick, pc.SUPPORT_FBP)), ("rf_to", lambda: ts.rf_to(ref_newick)),
                               ("rf_matrix", ts.rf_matrix)):
                t0 = time.perf_counter()
                out = call()
                rows[name + "_wall_ms"].append((time.perf_counter() - t0) * 1e3)
                if out is None:
                    raise RuntimeError(lib.errmsg)
                if name == "fbp":
                    mean_fbp = float(out[0].mean())
            rows["rf_matrix_kernel_ms"].append(ts.last_times()[1])
    res = {"tips": T, "trees": B, "moves": moves, "repeat": repeat}
    res.update({k: round(float(np.median(v)), 3) for k, v in rows.items()})
    lane_steps = float(T - 3) * B * (2 * T - 3)
    res.update({"tbe_lane_steps": lane_steps, "tbe_lane_steps_per_s": round(lane_steps / (res["tbe_kernel_ms"] * 1e-3), 1),
                "split_bytes": float(B) * (T - 3) * ((T + 31) // 32) * 4, "probe_steps": probes, "compares": compares,
                "mean_tbe": round(mean_tbe, 6), "mean_fbp": round(mean_fbp, 6)})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="500x100,2000x1000,5000x200")
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
