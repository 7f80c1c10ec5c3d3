"""Times the substitution-mapping calls on device 0 and prints one JSON line per shape:

  edge    pllhip_substmap_edge on an (inner, inner) edge, without and with PLLHIP_SUBST_SITES: the device time of the
          scale pass, the pair kernel and the reduction between HIP events (pllhip_substmap_last_times) and the wall
          time of the call; in the same process, alternating, the table kernel of pllhip_sitecat_edge on the same edge
          (pllhip_sitecat_last_times) and the wall time of pll_compute_edge_loglikelihood.  Byte model: the table
          kernel and the pair kernel each read the two vectors once, so a call should cost about two table kernels.
  tree    pllhip_eval_substitution_map on a --tree-taxa tree with --tree-sites sites: wall time per branch (every
          branch is one wait of the host), next to one pass of pllhip_eval_optimize_branches with max_iters = 1 on the
          same tree.

Medians of --repeat after a warm-up, with the spread (max - min).  Shapes are those of the benchmark configurations
(c2 = DNA, c3 = protein; four rate categories, coded tips, iid characters).  No GPU, no numbers: the tool fails.

usage: python tools/gpu_substmap.py [--shapes c2,c3] [--sites N] [--taxa N] [--tree-taxa N] [--tree-sites N]
                                    [--repeat N] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pll-modules_amd"))
import pllhip_ctypes as pc  # noqa: E402


def wall(call):
    t0 = time.perf_counter()
    out = call()
    return (time.perf_counter() - t0) * 1e3, out


def stats(values):
    return {"median": float(np.median(values)), "spread": float(np.max(values) - np.min(values))}


def run_edge(lib, name, sites, taxa, repeat):
    states, R, _, _ = pc.CONFIGS[name]
    tree = pc.Tree(taxa, 42, 43)
    with pc.build_instance(lib, states=states, rate_cats=R, ntips=taxa, nsites=sites, coded=True, tree=tree) as inst:
        pc.full_traversal(inst)
        top = tree.ops[-1]
        child, m = next((c, k) for c, k in ((top[2], top[3]), (top[5], top[6])) if c >= taxa)
        edge = (tree.root_a, tree.scaler_of(tree.root_a), child, tree.scaler_of(child), m)
        keys = ("scale", "pairs", "reduce", "wall", "scale_sites", "pairs_sites", "reduce_sites", "wall_sites",
                "table_kernel", "edge_lnl_wall")
        t = {k: [] for k in keys}
        for r in range(repeat + 1):                       # round 0 warms every path up
            row = []
            for flags in (0, pc.PLLHIP_SUBST_SITES):
                w, ep = wall(lambda: pc.EdgePairs.edge(inst, *edge, flags))
                with ep:
                    row += list(ep.last_times()) + [w]
                    total = float(ep.posterior.sum())
            with pc.SiteCat.edge(inst, *edge) as sc:
                row.append(sc.last_times()[0])
            row.append(wall(lambda: inst.edge_lnl(*edge))[0])
            if r:
                for k, v in zip(keys, row):
                    t[k].append(v)
        out = {"what": "edge", "shape": name, "states": states, "rate_cats": R, "taxa": taxa, "sites": sites,
               "repeat": repeat, "kernel": lib.lib.pllhip_partials_kernel_name(inst.p).decode(),
               "posterior_sum_over_sites": total / sites}
        for k in keys:
            s = stats(t[k])
            out[k + "_ms"], out[k + "_spread_ms"] = s["median"], s["spread"]
        out["pairs_over_table_kernel"] = out["pairs_ms"] / out["table_kernel_ms"]
        out["call_device_over_table_kernel"] = (out["scale_ms"] + out["pairs_ms"] + out["reduce_ms"]) / out["table_kernel_ms"]
        return out


def run_tree(lib, name, sites, taxa, repeat):
    states, R, _, _ = pc.CONFIGS[name]
    tree = pc.Tree(taxa, 42, 43)
    codes = pc.random_codes(taxa, sites, states, 44)
    subst, freqs = (pc.DNA_GTR_RATES, pc.DNA_FREQS) if states == 4 else pc.protein_model()
    with pc.Evaluation(lib, tree.newick(), nparts=1) as ev:
        ev.add_partition(0, states, sites, R, codes, subst, freqs, 0.5)
        ev.loglh()
        t = {"map": [], "branches_pass": []}
        branches = 2 * taxa - 3
        for r in range(repeat + 1):
            ev.loglh()
            w, res = wall(lambda: ev.L.pllhip_eval_substitution_map(ev.ev, 0))
            if not res:
                raise SystemExit(f"gpu_substmap.py: {lib.errmsg}")
            total = sum(res.contents.branches[0][m].total for m in range(branches))
            ev.L.pllhip_eval_destroy_substitution_map(res)
            wb, _ = wall(lambda: ev.optimize_branches(iters=1))
            if r:
                t["map"].append(w)
                t["branches_pass"].append(wb)
        m, b = stats(t["map"]), stats(t["branches_pass"])
        return {"what": "tree", "shape": name, "states": states, "rate_cats": R, "taxa": taxa, "sites": sites,
                "repeat": repeat, "branches": branches, "substitution_map_ms": m["median"],
                "substitution_map_spread_ms": m["spread"], "per_branch_ms": m["median"] / branches,
                "optimize_branches_one_pass_ms": b["median"], "optimize_branches_spread_ms": b["spread"],
                "expected_substitutions_per_site": total / sites}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c2,c3")
    ap.add_argument("--sites", type=int, default=1_000_000)
    ap.add_argument("--taxa", type=int, default=8)
    ap.add_argument("--tree-taxa", type=int, default=100)
    ap.add_argument("--tree-sites", type=int, default=50_000)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = pc.PllLib(pc.PRODUCT_LIB)
    if lib.lib.pllhip_device_count() < 1:
        raise SystemExit("gpu_substmap.py: no HIP device visible; there is no fallback")
    out = open(a.out, "a") if a.out else None
    for name in a.shapes.split(","):
        for line in (run_edge(lib, name, a.sites, a.taxa, a.repeat), run_tree(lib, name, a.tree_sites, a.tree_taxa, a.repeat)):
            text = json.dumps(line)
            print(text, flush=True)
            if out:
                out.write(text + "\n")
                out.flush()
    if out:
        out.close()


if __name__ == "__main__":
    main()
