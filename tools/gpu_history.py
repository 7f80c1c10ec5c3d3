"""Times pllhip_sample_histories_edges on device 0 next to the ancestral draw it extends and the full traversal that
produced the vectors, on the same instance, and prints one JSON line per (shape, replicates).

Per line: the traversal (all P-matrices, every operation, the edge log-likelihood: wall time of pc.full_traversal,
median of --repeat after a warm-up); pllhip_sample_ancestral_edges alone (its walk kernels between device events:
`ancestral_kernel_ms`, the figure a change to the shared code must leave alone); the histories call (wall), its table
kernel, walk kernels and history kernels between device events and its copies (pllhip_history_last_times); the host
time of the tables (the call's wall time less the device stages is mostly this and the copies); the events drawn.

Shapes are those of the benchmark configurations: c2 = 100 taxa x 1 M sites DNA, c3 = 200 x 1 M protein, four rate
categories.  No GPU, no numbers: the tool fails.

usage: python tools/gpu_history.py [--shapes c3,c2] [--replicates 1,16] [--sites N] [--repeat N] [--out FILE.jsonl]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pll-modules_amd"))
import pllhip_ctypes as pc  # noqa: E402


def run(lib, name, sites, replicate_list, repeat, emit):
    states, R, taxa, _ = pc.CONFIGS[name]
    tree = pc.Tree(taxa, 42, 43)
    with pc.build_instance(lib, states, R, taxa, sites, tree=tree, pinv=0.1) as inst:
        trav = []
        for r in range(repeat + 1):                       # round 0 warms up
            t0 = time.perf_counter()
            pc.full_traversal(inst)
            if r:
                trav.append((time.perf_counter() - t0) * 1e3)
        t = inst.tree
        sc = (lambda n: t.scaler_of(n)) if inst.nscalers else (lambda n: pc.PLL_SCALE_BUFFER_NONE)
        root_edge = (t.root_a, sc(t.root_a), t.root_b, sc(t.root_b))
        pa, ch, mi = pc.tree_edges(t, t.root_a)
        lengths = np.asarray(t.brlens, dtype=np.float64)[mi]
        for replicates in replicate_list:
            out = np.zeros((replicates, 2 * taxa - 2, sites), dtype=np.uint8)
            comp = np.zeros((replicates, sites), dtype=np.uint8)
            anc = []
            for r in range(repeat + 1):
                pc.sample_ancestral_edges(inst, root_edge, pa, ch, mi, 1234 + r, replicates, flags=pc.PLLHIP_ANCS_COMPONENT,
                                          out=out, component=comp)
                if r:
                    anc.append(pc.ancsample_last_times(lib)[1])
            del out, comp
            wall, table, walk, hist, copy, h = [], [], [], [], [], None
            for r in range(repeat + 1):
                t0 = time.perf_counter()
                h = pc.sample_histories_edges(inst, root_edge, pa, ch, mi, lengths, 1234 + r, replicates, flags=0,
                                              want_out=False, want_component=False)
                dt = (time.perf_counter() - t0) * 1e3
                if r:
                    tb, wk, hk, cm = pc.history_last_times(lib)
                    wall.append(dt)
                    table.append(tb)
                    walk.append(wk)
                    hist.append(hk)
                    copy.append(cm)
            hk, wk, tv = float(np.median(hist)), float(np.median(walk)), float(np.median(trav))
            events = int(h.counts.sum())
            emit({"shape": name, "states": states, "rate_cats": R, "taxa": taxa, "sites": sites, "replicates": replicates,
                  "repeat": repeat, "edges": len(pa), "traversal_ms": tv, "ancestral_kernel_ms": float(np.median(anc)),
                  "ancestral_kernel_ms_runs": [float(x) for x in anc], "wall_ms": float(np.median(wall)),
                  "table_ms": float(np.median(table)), "walk_ms": wk, "history_ms": hk, "copy_ms": float(np.median(copy)),
                  "history_over_walk": hk / wk, "history_over_traversal": hk / tv,
                  "paths_per_s": sites * replicates * len(pa) / hk * 1e3, "substitutions": events,
                  "substitutions_per_site_and_replicate": events / (sites * replicates),
                  "dropped_edges": int(h.dropped_edges.sum()), "dropped": int(h.dropped)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c3,c2")
    ap.add_argument("--replicates", default="1,16")
    ap.add_argument("--sites", type=int, default=0, help="patterns (default: the configuration's)")
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = pc.PllLib(pc.PRODUCT_LIB)
    if lib.lib.pllhip_device_count() < 1:
        raise SystemExit("gpu_history.py: no HIP device visible; there is no fallback")
    out = open(a.out, "a") if a.out else None

    def emit(line):
        text = json.dumps(line)
        print(text, flush=True)
        if out:
            out.write(text + "\n")
            out.flush()

    for name in a.shapes.split(","):
        run(lib, name, a.sites or pc.CONFIGS[name][3], [int(x) for x in a.replicates.split(",")], a.repeat, emit)
    if out:
        out.close()


if __name__ == "__main__":
    main()
