"""Times marginal ancestral states for a whole tree on device 0 and prints one JSON line per shape and form
(DESIGN.md section 19):

  summary   pllhip_eval_compute_ancestral(ev, 0): one state and one probability per site and inner node
  probs     pllhip_eval_compute_ancestral(ev, PLLHIP_ANC_PROBS): also the sites x states table (at --probs-sites sites)

Per line: wall time of the call (median of --repeat after a warm-up; the call ends in its own wait), the time of
the batch's kernels between device events (pllhip_node_ancestral_last_times), and that against the traffic model
at 8 TB/s -- per node two vectors read (a coded tip: one byte per site) and sites * 9 or sites * (9 + 8 S) bytes
written.  The re-rooting traversals between the nodes are part of the wall time, not of the kernel time.

Baseline, in the same process and alternating with the new path: what the library offered before for the same
result -- the re-rooting loop with one incremental evaluation and one pll_compute_node_ancestral per node (a
sites x states table over the host link and a wait each), plus numpy's argmax / max over the table.

Shapes are those of the benchmark configurations: c2 = 100 taxa x 1 M sites DNA, c3 = 200 x 1 M protein, c5 = 50 x
200 k at 61 states, four rate categories, coded tips, iid characters.  No GPU, no numbers: the tool fails.

usage: python tools/gpu_ancestral.py [--shapes c2,c3,c5] [--forms summary,probs] [--repeat N] [--probs-sites N]
                                     [--sites N] [--no-baseline] [--out FILE.jsonl]"""
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

PEAK = 8e12


def model_of(states):
    if states == 4:
        return pc.DNA_GTR_RATES, pc.DNA_FREQS, 0.841
    if states == 20:
        return (*pc.protein_model(), 0.5)
    return (*pc.codon_model(), 0.5)


def inner_records(ev):
    """inner records in the driver's node order: a full post-order from vroot"""
    out = []

    def addr(p):
        return C.addressof(p.contents)

    def walk(rec):
        if rec.contents.next:
            s = rec.contents.next
            while addr(s) != addr(rec):
                walk(s.contents.back)
                s = s.contents.next
            out.append(rec)

    vroot = ev.utree.contents.vroot
    walk(vroot.contents.back)
    walk(vroot)
    return out


def new_path(ev, flags):
    L = ev.L
    t0 = time.perf_counter()
    ptr = L.pllhip_eval_compute_ancestral(ev.ev, flags)
    dt = (time.perf_counter() - t0) * 1e3
    if not ptr:
        raise RuntimeError(ev.lib.errmsg)
    ms, chunks = C.c_double(0), C.c_ulonglong(0)
    L.pllhip_node_ancestral_last_times(C.byref(ms), C.byref(chunks))
    probe = (int(ptr.contents.states[0][0]), float(ptr.contents.state_probs[0][0]))
    L.pllhip_eval_destroy_ancestral(ptr)
    return dt, ms.value, chunks.value, probe


def baseline(ev, recs, table, want_probs):
    """the loop a caller had to write before: re-root, evaluate incrementally, fetch the node's table, summarise it"""
    L, inst = ev.L, ev.parts[0]
    old = L.pllhip_eval_root(ev.ev)
    rows = table.reshape(inst.N, inst.S)
    keep, probe = [], None
    t0 = time.perf_counter()
    for rec in recs:
        L.pllhip_eval_set_root(ev.ev, rec)
        ev.loglh(True)
        n, b = rec.contents, rec.contents.back.contents
        if not L.pll_compute_node_ancestral(inst.p, n.clv_index, n.scaler_index, b.clv_index, b.scaler_index,
                                            n.pmatrix_index, inst.params_p, table.ctypes.data_as(pc.c_double_p)):
            raise RuntimeError(ev.lib.errmsg)
        st = np.argmax(rows, axis=1).astype(np.uint8)
        keep = [st, rows.max(axis=1), rows.copy() if want_probs else None]
        if probe is None:
            probe = (int(keep[0][0]), float(keep[1][0]))
    dt = (time.perf_counter() - t0) * 1e3
    L.pllhip_eval_set_root(ev.ev, old)
    return dt, probe


def traffic_bytes(recs, ntips, N, R, S, want_probs):
    total = 0
    for rec in recs:
        n, b = rec.contents, rec.contents.back.contents
        for clv in (n.clv_index, b.clv_index):
            total += N if clv < ntips else N * R * S * 8
        total += N * (9 + (8 * S if want_probs else 0))
    return total


def run(lib, name, form, sites, repeat, with_baseline):
    states, R, taxa, _ = pc.CONFIGS[name]
    subst, freqs, alpha = model_of(states)
    want_probs = form == "probs"
    flags = pc.PLLHIP_ANC_PROBS if want_probs else 0
    tree = pc.Tree(taxa, 42, 43)
    with pc.Evaluation(lib, tree.newick(), nparts=1) as ev:
        ev.add_partition(0, states, sites, R, pc.random_codes(taxa, sites, states), subst, freqs, alpha)
        ev.loglh()
        recs = inner_records(ev)
        table = np.zeros(sites * states) if with_baseline else None
        new_wall, new_kern, base_wall, chunks, probes = [], [], [], 0, None
        for r in range(repeat + 1):                       # round 0 warms both paths up
            dt, ms, chunks, pa = new_path(ev, flags)
            if with_baseline:
                bt, pb = baseline(ev, recs, table, want_probs)
                probes = (pa, pb)
            if r:
                new_wall.append(dt)
                new_kern.append(ms)
                if with_baseline:
                    base_wall.append(bt)
        model = traffic_bytes(recs, taxa, sites, R, states, want_probs)
        line = {"shape": name, "form": form, "states": states, "rate_cats": R, "taxa": taxa, "sites": sites,
                "nodes": len(recs), "repeat": repeat, "chunks": int(chunks),
                "new_wall_ms": float(np.median(new_wall)), "new_kernel_ms": float(np.median(new_kern)),
                "model_bytes": int(model), "model_ms_at_8TBs": model / PEAK * 1e3,
                "kernel_over_model": float(np.median(new_kern)) / (model / PEAK * 1e3),
                "kernel": lib.lib.pllhip_partials_kernel_name(ev.parts[0].p).decode()}
        if with_baseline:
            line["baseline_wall_ms"] = float(np.median(base_wall))
            line["baseline_over_new"] = line["baseline_wall_ms"] / line["new_wall_ms"]
            # (first node, first site: same state; probabilities to the tolerance of the test-suite)
            line["agree"] = bool(probes[0][0] == probes[1][0] and abs(probes[0][1] - probes[1][1]) < 1e-6)
        return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c2,c3,c5")
    ap.add_argument("--forms", default="summary,probs")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--sites", type=int, default=0, help="sites of the summary form (default: the configuration's)")
    ap.add_argument("--probs-sites", type=int, default=125_000)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = pc.PllLib(pc.PRODUCT_LIB)
    if lib.lib.pllhip_device_count() < 1:
        raise SystemExit("gpu_ancestral.py: no HIP device visible; there is no fallback")
    out = open(a.out, "a") if a.out else None
    for name in a.shapes.split(","):
        for form in a.forms.split(","):
            sites = a.probs_sites if form == "probs" else (a.sites or pc.CONFIGS[name][3])
            line = json.dumps(run(lib, name, form, sites, a.repeat, not a.no_baseline))
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
    if out:
        out.close()


if __name__ == "__main__":
    main()
