"""Times pllhip_sample_ancestral_edges on device 0 against the full traversal that produced the vectors it reads, on the
same instance, and prints one JSON line per (shape, replicates).

Per line: the traversal (all P-matrices, every operation, the edge log-likelihood: wall time of pc.full_traversal,
median of --repeat after a warm-up), the call (wall), the table kernel and the walk kernels between device events and
the copies (pllhip_ancsample_last_times).  The yardstick: the walk reads every inner vector once per group of eight
replicates, the traversal writes every inner vector once and reads every inner child once; both byte counts and the
bytes per second they imply are on the line (tips are codes: a byte per site, left out of both).

Shapes are those of the benchmark configurations: c2 = 100 taxa x 1 M sites DNA, c3 = 200 x 1 M protein, four rate
categories.  No GPU, no numbers: the tool fails.

usage: python tools/gpu_ancsample.py [--shapes c3,c2] [--replicates 1,16] [--sites N] [--repeat N] [--out FILE.jsonl]"""
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
        vector = sites * R * inst.Sp * 8
        inner_read = 1 + int((ch >= taxa).sum())          # the root, and every child that is no tip
        trav_bytes = vector * ((taxa - 2) + (inner_read - 2))
        for replicates in replicate_list:
            out = np.zeros((replicates, 2 * taxa - 2, sites), dtype=np.uint8)
            comp = np.zeros((replicates, sites), dtype=np.uint8)
            wall, table, kernel, copy, chunks, dropped = [], [], [], [], 0, 0
            for r in range(repeat + 1):
                t0 = time.perf_counter()
                _, _, dropped = pc.sample_ancestral_edges(inst, root_edge, pa, ch, mi, 1234 + r, replicates,
                                                          flags=pc.PLLHIP_ANCS_COMPONENT, out=out, component=comp)
                dt = (time.perf_counter() - t0) * 1e3
                tb, km, cm, chunks = pc.ancsample_last_times(lib)
                if r:
                    wall.append(dt)
                    table.append(tb)
                    kernel.append(km)
                    copy.append(cm)
            k, tv = float(np.median(kernel)), float(np.median(trav))
            walk_bytes = vector * inner_read * ((replicates + 7) // 8)
            emit({"shape": name, "states": states, "rate_cats": R, "taxa": taxa, "sites": sites, "replicates": replicates,
                  "repeat": repeat, "chunks": int(chunks), "dropped": int(dropped), "traversal_ms": tv,
                  "traversal_bytes": int(trav_bytes), "traversal_GBps": trav_bytes / tv / 1e6,
                  "wall_ms": float(np.median(wall)), "table_ms": float(np.median(table)), "kernel_ms": k,
                  "copy_ms": float(np.median(copy)), "walk_bytes": int(walk_bytes), "walk_GBps": walk_bytes / k / 1e6,
                  "kernel_over_traversal": k / tv, "out_bytes": int(out.size + comp.size),
                  "draws_per_s": sites * replicates * (len(pa) + 2) / k * 1e3,
                  "state_histogram_head": np.bincount(out[0, taxa], minlength=4)[:4].tolist()})


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
        raise SystemExit("gpu_ancsample.py: no HIP device visible; there is no fallback")
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
