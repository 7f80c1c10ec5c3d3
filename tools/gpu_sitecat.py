"""Times the site-category calls on device 0 and prints one JSON line per shape:

  table      pllhip_sitecat_edge on an (inner, inner) edge: the time of the family's table kernel between device events
             (pllhip_sitecat_last_times) and the wall time of the call, next to pll_compute_edge_loglikelihood on the
             same partition and edge, alternating in the same process -- its wall time without a per-site buffer (launch,
             kernel, one wait) and with one (plus the copy of sites doubles to the host).  Byte model: both read the
             same two vectors; the table kernel writes R (2 R with p-inv) doubles and a count per site instead of one
             double: (2 R S + R) / (2 R S + 1) without p-inv.
  posterior  one pllhip_sitecat_posteriors without the full table: posterior and reduction kernels between events
  em         pllhip_sitecat_em_weights with epsilon 0 and --em-iterations updates: wall time per evaluation (one launch
             and one wait each), against 8 N (R + 1) bytes at the 5.8 TB/s the project sustains (README)
  fit        a fit to epsilon 1e-3 from equal weights: evaluations and wall time -- what replaces one full evaluation
             per trial point of a numerical optimiser

Medians of --repeat after a warm-up.  Shapes are those of the benchmark configurations (c2 = DNA, c3 = protein, c5 = 61
states; four rate categories, coded tips, iid characters) on --taxa taxa: one edge is timed, so a small tree serves.
No GPU, no numbers: the tool fails.

usage: python tools/gpu_sitecat.py [--shapes c2,c3] [--sites N] [--taxa N] [--repeat N] [--pinv P] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pll-modules_amd"))
import pllhip_ctypes as pc  # noqa: E402

SUSTAINED = 5.8e12


def wall(call):
    t0 = time.perf_counter()
    out = call()
    return (time.perf_counter() - t0) * 1e3, out


def run(lib, name, sites, taxa, repeat, pinv, em_iterations):
    states, R, _, _ = pc.CONFIGS[name]
    tree = pc.Tree(taxa, 42, 43)
    kw = {"mixture_pinv": [pinv]} if pinv > 0 else {}
    with pc.build_instance(lib, states=states, rate_cats=R, ntips=taxa, nsites=sites, coded=True, tree=tree, **kw) as inst:
        pc.full_traversal(inst)
        top = tree.ops[-1]
        child, m = next((c, k) for c, k in ((top[2], top[3]), (top[5], top[6])) if c >= taxa)
        edge = (tree.root_a, tree.scaler_of(tree.root_a), child, tree.scaler_of(child), m)
        t = {k: [] for k in ("table_kernel", "table_wall", "edge_wall", "edge_persite_wall", "posterior", "em_eval",
                             "fit_wall")}
        fit = None
        for r in range(repeat + 1):                       # round 0 warms every path up
            tw, sc = wall(lambda: pc.SiteCat.edge(inst, *edge))
            with sc:
                tk = sc.last_times()[0]
                ew, lnl = wall(lambda: inst.edge_lnl(*edge))
                ep, _ = wall(lambda: inst.edge_lnl(*edge, persite=True))
                po = sc.posteriors()
                tp = sc.last_times()[1]
                em = sc.em_weights(0.0, em_iterations, start=np.full(R, 1.0 / R))
                te = sc.last_times()[2] / (em.iterations + 1)
                tf, fit = wall(lambda: sc.em_weights(1e-3, 1000, start=np.full(R, 1.0 / R)))
            if r:
                for k, v in zip(t, (tk, tw, ew, ep, tp, te, tf)):
                    t[k].append(v)
        med = {k: float(np.median(v)) for k, v in t.items()}
        planes = 2 if pinv > 0 else 1
        vec = 2 * R * states * 8
        em_bytes = 8 * sites * (planes * R + 1)
        return {"shape": name, "states": states, "rate_cats": R, "taxa": taxa, "sites": sites, "pinv": pinv,
                "repeat": repeat, "kernel": lib.lib.pllhip_partials_kernel_name(inst.p).decode(),
                "table_kernel_ms": med["table_kernel"], "table_wall_ms": med["table_wall"],
                "edge_lnl_wall_ms": med["edge_wall"], "edge_lnl_persite_wall_ms": med["edge_persite_wall"],
                "edge_lnl_wall_spread_ms": float(np.max(t["edge_wall"]) - np.min(t["edge_wall"])),
                "table_kernel_over_edge_wall": med["table_kernel"] / med["edge_wall"],
                "byte_ratio": (vec + planes * R * 8 + 4) / (vec + 8),
                "posterior_ms": med["posterior"],
                "em_evaluation_ms": med["em_eval"], "em_bytes": em_bytes,
                "em_model_ms_at_5.8TBs": em_bytes / SUSTAINED * 1e3,
                "em_over_model": med["em_eval"] / (em_bytes / SUSTAINED * 1e3),
                "fit_evaluations": int(fit.iterations + 1), "fit_wall_ms": med["fit_wall"],
                "lnl_agrees": bool(abs(po.loglh - lnl) <= 1e-9 * abs(lnl))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c2,c3")
    ap.add_argument("--sites", type=int, default=1_000_000)
    ap.add_argument("--taxa", type=int, default=8)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--pinv", type=float, default=0.0)
    ap.add_argument("--em-iterations", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = pc.PllLib(pc.PRODUCT_LIB)
    if lib.lib.pllhip_device_count() < 1:
        raise SystemExit("gpu_sitecat.py: no HIP device visible; there is no fallback")
    out = open(a.out, "a") if a.out else None
    for name in a.shapes.split(","):
        line = json.dumps(run(lib, name, a.sites, a.taxa, a.repeat, a.pinv, a.em_iterations))
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    if out:
        out.close()


if __name__ == "__main__":
    main()
