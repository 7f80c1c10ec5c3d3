"""Times pllhip_simulate_edges on device 0 and prints one JSON line per shape.

Per line: wall time of the call (median of --repeat after a warm-up), the time of the table kernel and of the evolve
kernels between device events and of the copies (pllhip_simulate_last_times), the bytes of the output and bytes
written per second against the kernel time and against the wall time, and the draws (sites x edges x replicates) per
second of the kernel.

Baseline, with --baseline: numpy's pllhip_ctypes.simulated_codes for the same tree and site count on this host -- the
toy process (equal rates, two rate classes), not the partition's model; it is what the repository simulated with before.

Shapes are those of the benchmark configurations: c2 = 100 taxa x 1 M sites DNA, c3 = 200 x 1 M protein, c5 = 50 x
200 k at 61 states, four rate categories.  No GPU, no numbers: the tool fails.

usage: python tools/gpu_simulate.py [--shapes c2,c3,c5] [--replicates N] [--sites N] [--repeat N] [--inner]
                                    [--baseline] [--out FILE.jsonl]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pll-modules_amd"))
import pllhip_ctypes as pc  # noqa: E402


def run(lib, name, sites, replicates, repeat, inner, with_baseline):
    states, R, taxa, _ = pc.CONFIGS[name]
    tree = pc.Tree(taxa, 42, 43)
    flags = pc.PLLHIP_SIM_INNER if inner else 0
    # the partition's own alignment plays no part: a few sites are enough
    with pc.build_instance(lib, states, R, taxa, 64, tree=tree, pinv=0.1) as inst:
        inst.update_pmatrices(np.arange(tree.nedges), tree.brlens)
        pa, ch, mi = pc.tree_edges(tree)
        rows = (2 * taxa - 2) if inner else taxa
        out = np.zeros((replicates, rows, sites), dtype=np.uint8)
        wall, tables, kernel, copy, chunks = [], [], [], [], 0
        for r in range(repeat + 1):                       # round 0 warms up
            t0 = time.perf_counter()
            pc.simulate_edges(inst, taxa, pa, ch, mi, 1234 + r, sites, replicates, flags=flags, out=out)
            dt = (time.perf_counter() - t0) * 1e3
            tb, km, cm, chunks = pc.simulate_last_times(lib)
            if r:
                wall.append(dt)
                tables.append(tb)
                kernel.append(km)
                copy.append(cm)
        nbytes = out.size
        draws = sites * replicates * (len(pa) + 3)
        k = float(np.median(kernel))
        w = float(np.median(wall))
        line = {"shape": name, "states": states, "rate_cats": R, "taxa": taxa, "sites": sites, "replicates": replicates,
                "inner": bool(inner), "repeat": repeat, "chunks": int(chunks), "wall_ms": w,
                "tables_ms": float(np.median(tables)), "kernel_ms": k, "copy_ms": float(np.median(copy)),
                "bytes": int(nbytes), "kernel_GBps": nbytes / k / 1e6, "wall_GBps": nbytes / w / 1e6,
                "kernel_draws_per_s": draws / k * 1e3, "state_histogram_head": np.bincount(out[0, 0], minlength=4)[:4].tolist()}
        if with_baseline:
            t0 = time.perf_counter()
            pc.simulated_codes(tree, sites, states)
            line["numpy_toy_ms_per_replicate"] = (time.perf_counter() - t0) * 1e3
            line["numpy_toy_over_wall_per_replicate"] = line["numpy_toy_ms_per_replicate"] / (w / replicates)
        return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c2,c3,c5")
    ap.add_argument("--replicates", type=int, default=4)
    ap.add_argument("--sites", type=int, default=0, help="columns per replicate (default: the configuration's)")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--inner", action="store_true")
    ap.add_argument("--baseline", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = pc.PllLib(pc.PRODUCT_LIB)
    if lib.lib.pllhip_device_count() < 1:
        raise SystemExit("gpu_simulate.py: no HIP device visible; there is no fallback")
    out = open(a.out, "a") if a.out else None
    for name in a.shapes.split(","):
        sites = a.sites or pc.CONFIGS[name][3]
        line = json.dumps(run(lib, name, sites, a.replicates, a.repeat, a.inner, a.baseline))
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    if out:
        out.close()


if __name__ == "__main__":
    main()
