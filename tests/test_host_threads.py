"""Several host threads of one process inside the library at once: pll-modules' parallel mode (N worker threads, each
with a private partition or a private slice of one, meeting only in parallel_reduce_cb: src/tree/pll_tree.h:274-276,
src/tree/treeinfo.c:215-227; INTEGRATION.md section 4, "Threads").

The workers are Python threads; ctypes.CDLL calls release the interpreter lock, so the threads really are inside the
library together.  A worker that raises records the exception and breaks the barrier, threads are joined with a timeout,
and a test fails on any recorded exception or on a thread that is still alive: trouble ends the test, nothing is tried
twice.

  test_driver_from_worker_threads    the C evaluation driver with a reduce callback per thread against the
                                     single-evaluator run (oracle on the CPU, libpll_hip.so on the GPU)
  test_concurrent_partitions_...     private partitions of four threads: every byte equals the serial run's
  test_concurrent_subsystems_...     four threads in four different entry points of the library
"""
import threading
import time
import traceback

import numpy as np
import pytest

import pllhip_ctypes as pc
import test_compress_patterns as cp
import test_tree_support_gpu as tsg
import test_tree_support_restatement as rs
from _evaldriver_worker import NTIPS, PARTS, build, run
from test_multirank import check_driver_ranks

JOIN_TIMEOUT_S = 300


class Group:
    """W threads behind one barrier; run() returns what every worker returned or fails the test"""

    def __init__(self, W):
        self.W = W
        self.barrier = threading.Barrier(W, timeout=120)
        self.slots = [None] * W
        self.errors = []
        self._lock = threading.Lock()

    def fail(self, rank, exc):
        with self._lock:
            self.errors.append((rank, "".join(traceback.format_exception(type(exc), exc, exc.__traceback__))))
        self.barrier.abort()

    def run(self, work):
        """work(rank) in W threads; the list of their results"""
        results = [None] * self.W

        def body(rank):
            try:
                results[rank] = work(rank)
            except BaseException as exc:                  # noqa: BLE001 -- whatever it is, the peers must not wait for it
                self.fail(rank, exc)

        threads = [threading.Thread(target=body, args=(r,), daemon=True) for r in range(self.W)]
        for t in threads:
            t.start()
        deadline = time.monotonic() + JOIN_TIMEOUT_S
        for t in threads:
            t.join(max(0.0, deadline - time.monotonic()))
        alive = [r for r, t in enumerate(threads) if t.is_alive()]
        if alive:
            self.barrier.abort()
        assert not self.errors, "\n".join(f"worker {r}:\n{text}" for r, text in self.errors)
        assert not alive, f"workers {alive} did not come back"
        return results

    def reduce_cb(self, rank, calls):
        """the all-reduce of the reference's callback interface among the threads of this group: payloads combined in
        rank order, so that every thread holds bit-identical values"""
        combine = {0: np.add, 1: np.maximum, 2: np.minimum}      # PLLMOD_COMMON_REDUCE_SUM / MAX / MIN

        def cb(ctx, data, n, op):
            try:
                mine = np.ctypeslib.as_array(data, shape=(n,))
                self.slots[rank] = mine.copy()
                self.barrier.wait()
                total = self.slots[0].copy()
                for r in range(1, self.W):
                    total = combine[op](total, self.slots[r])
                self.barrier.wait()                       # nobody's next payload replaces a slot somebody still reads
                mine[:] = total
                calls.append((n, op))
            except BaseException as exc:                  # noqa: BLE001 -- an exception cannot travel through the C caller
                self.fail(rank, exc)

        return pc.REDUCE_CB(cb)


# ---------------------------------------------------------------------------------------------------------------------
# the evaluation driver, one evaluator per thread
# ---------------------------------------------------------------------------------------------------------------------
DRIVER_CASES = [("sites", 2), ("parts", 2), ("scaled-sites", 2), ("unlinked-parts", 2), ("unlinked-sites", 2),
                ("sites", 3), ("unlinked-sites", 3)]       # three workers: 700, 333 and 501 sites in uneven slices


def drive_from_threads(lib, mode, W):
    linkage = 2 if mode.startswith("unlinked") else 1 if mode.startswith("scaled") else 0
    split = mode.split("-")[-1]
    flags = 4 if split == "sites" else 0                   # as tests/_evaldriver_worker.py: several trial lengths per scan
    tree = pc.Tree(NTIPS, 42, 43)
    group = Group(W)

    def work(rank):
        if split == "sites":
            owned = set(range(len(PARTS)))
            site_range = lambda k, n: (n * rank // W, n * (rank + 1) // W)      # noqa: E731
        else:
            owned = {k for k in range(len(PARTS)) if k % W == rank}
            site_range = lambda k, n: (0, n)                                    # noqa: E731
        calls = []
        with build(lib, tree, owned, site_range, group.reduce_cb(rank, calls), flags, linkage) as ev:
            out = run(ev)
        out["reduce_calls"] = len(calls)
        out["payloads"] = sorted(set(n for n, _ in calls))
        return out

    ranks = group.run(work)
    with build(lib, tree, set(range(len(PARTS))), lambda k, n: (0, n), None, flags, linkage) as ev:
        ranks[0]["single"] = run(ev)
    check_driver_ranks(ranks)


@pytest.mark.parametrize("mode,W", DRIVER_CASES)
@pytest.mark.parametrize("which", ["oracle", pytest.param("product", marks=pytest.mark.gpu)])
def test_driver_from_worker_threads(request, which, mode, W):
    """W threads, each with its own evaluator over its slice of the sites ("sites") or its share of the partitions
    ("parts"), reproduce the single evaluator; every thread holds the same numbers.  With a reduce callback the driver
    keeps Newton-Raphson on the host, so no two device loops meet on the card."""
    drive_from_threads(request.getfixturevalue(which), mode, W)


# ---------------------------------------------------------------------------------------------------------------------
# private partitions of four threads
# ---------------------------------------------------------------------------------------------------------------------
# one partition per kernel family: 4 states, 20 states, 33 .. 64 states, 2 .. 32 states with vector tips
MIXED = [dict(states=4, rate_cats=4, ntips=12, nsites=1500, coded=True),
         dict(states=20, rate_cats=4, ntips=12, nsites=700, coded=True),
         dict(states=61, rate_cats=4, ntips=10, nsites=200, coded=True),
         dict(states=7, rate_cats=3, ntips=12, nsites=900, coded=False)]
# four of one family: their first launches of that family meet
SAME_FAMILY = [dict(states=20, rate_cats=4, ntips=12, nsites=700, coded=True, seed_shift=k) for k in range(4)]
ROUNDS = 3
TRIAL_LENGTHS = (0.02, 0.4, 1.5)


def three_rounds(inst, base):
    """everything three traversals of a partition produce, as bytes; `base`: the branch lengths of round 0"""
    t = inst.tree
    sa, sb = t.scaler_of(t.root_a), t.scaler_of(t.root_b)
    st = inst.alloc_sumtable()
    out = []
    try:
        for k in range(ROUNDS):
            t.brlens = base * (1.0 + 0.1 * k)
            out.append(np.float64(pc.full_traversal(inst)).tobytes())
            lnl, persite = inst.edge_lnl(t.root_a, sa, t.root_b, sb, t.root_matrix, persite=True)
            out += [np.float64(lnl).tobytes(), persite.tobytes()]
            inst.update_sumtable(t.root_a, t.root_b, sa, sb, st)
            for length in TRIAL_LENGTHS:
                out.append(np.array(inst.derivatives(sa, sb, length, st), dtype=np.float64).tobytes())
            for node, scaler in ((t.root_a, sa), (t.root_b, sb)):
                out.append(np.ascontiguousarray(inst.get_clv(node)).tobytes())
                if scaler != pc.PLL_SCALE_BUFFER_NONE:
                    out.append(inst.get_scaler(scaler).tobytes())
    finally:
        inst.free_sumtable(st)
        t.brlens = base
    return out


def serial_pass(insts):
    return [three_rounds(inst, inst.tree.brlens.copy()) for inst in insts]


def threaded_pass(product, specs, insts=None):
    """every thread runs the three rounds on insts[rank], or -- insts None -- on an instance it creates and destroys
    itself; the threads leave one barrier together, so that their first launches coincide"""
    group = Group(len(specs))

    def work(rank):
        if insts is not None:
            group.barrier.wait()
            return three_rounds(insts[rank], insts[rank].tree.brlens.copy())
        group.barrier.wait()
        with pc.build_instance(product, **specs[rank]) as inst:
            return three_rounds(inst, inst.tree.brlens.copy())

    return group.run(work)


def assert_same_bytes(got, want):
    assert len(got) == len(want)
    for rank, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w), rank
        for item, (a, b) in enumerate(zip(g, w)):
            assert a == b, f"partition {rank}: item {item} of the concurrent run differs from the serial run"


@pytest.mark.gpu
@pytest.mark.parametrize("own_lifecycle", [False, True], ids=["shared-lifetime", "own-lifetime"])
@pytest.mark.parametrize("specs", [MIXED, SAME_FAMILY], ids=["mixed", "same-family"])
def test_concurrent_partitions_equal_the_serial_run_bitwise(product, specs, own_lifecycle):
    """four threads, a private partition each: log-likelihoods (per site too), derivatives, vectors and scaler counts
    of three traversals are the bytes of the same calls made one after the other.  The engine is deterministic from run
    to run and across schedules; other threads in the library must not change that.  own-lifetime: every thread also
    creates and destroys its partition, so that engines come and go while others launch."""
    insts = [pc.build_instance(product, **spec) for spec in specs]     # all alive in both passes
    try:
        want = serial_pass(insts)
        if own_lifecycle:
            for inst in insts:
                inst.close()
            got = threaded_pass(product, specs)
        else:
            got = threaded_pass(product, specs, insts)
    finally:
        for inst in insts:
            inst.close()
    assert_same_bytes(got, want)


# ---------------------------------------------------------------------------------------------------------------------
# four threads in four entry points
# ---------------------------------------------------------------------------------------------------------------------
def subsystem_jobs(product):
    """four jobs on inputs of their own; each returns (what it computed, counts of its last call, times of its last
    call) -- the `last call` queries are per thread"""
    nt = product.char_map("pll_map_nt")
    compress_rows = [r.tobytes() for r in cp.draw(np.random.default_rng(501), cp.DNA, 7, 1000, 40)]
    stats_rows = [r.tobytes() for r in cp.draw(np.random.default_rng(502), b"ACGTacgt-NRY", 20, 2000, 300)]
    labels, _, ref, trees = tsg.make_case(40, 30, seed=503)
    ref_newick, newicks = rs.to_newick(ref), [rs.to_newick(t) for t in trees]
    spec = dict(states=4, rate_cats=4, ntips=12, nsites=1500, coded=True, seed_shift=5)

    def compress():
        res = product.compress_site_patterns(compress_rows, nt, msa_form=True)
        assert res.ok, (res.errno, res.errmsg)
        # (probe steps depend on which of two patterns that share a slot claimed it first; the full compares do not:
        # one per site that joined a group)
        return ((res.length, res.rows, res.weights.tobytes(), res.site_pattern_map.tobytes()), (res.compares,),
                product.compress_last_times())

    def stats():
        got = product.msa_compute_stats(stats_rows, 4, nt)
        assert got is not None, (product.errno, product.errmsg)
        got = {k: (v.tobytes() if isinstance(v, np.ndarray) else v) for k, v in got.items()}
        return got, (), product.msa_stats_last_times()

    def tree_set():
        with pc.TreeSet(product, len(labels), labels) as ts:
            assert ts.h, (product.errno, product.errmsg)
            for text in newicks:
                assert ts.add(text), (product.errno, product.errmsg)
            rf = ts.rf_matrix()
            fbp, tbe = ts.support(ref_newick, pc.SUPPORT_FBP), ts.support(ref_newick, pc.SUPPORT_TBE)
            assert rf is not None and fbp is not None and tbe is not None, (product.errno, product.errmsg)
            out = (rf.tobytes(), fbp[0].tobytes(), fbp[1].tobytes(), tbe[0].tobytes(), tbe[1].tobytes())
            return out, (ts.last_counts()[1],), ts.last_times()

    def likelihood():
        with pc.build_instance(product, **spec) as inst:
            return np.float64(pc.full_traversal(inst)).tobytes(), (), ()

    return [compress, stats, tree_set, likelihood]


@pytest.mark.gpu
def test_concurrent_subsystems_equal_the_serial_run(product):
    """site-pattern compression, alignment statistics, a tree set and a likelihood traversal at the same time, each in
    a thread of its own: results equal the same calls made one after the other, and what a thread reads back as the
    counts and times of `the last call` is its own call's"""
    jobs = subsystem_jobs(product)
    want = [job() for job in jobs]
    main_times = (product.compress_last_times(), product.msa_stats_last_times())
    group = Group(len(jobs))

    def work(rank):
        group.barrier.wait()
        return jobs[rank]()

    got = group.run(work)
    for rank, ((value, counts, times), (want_value, want_counts, want_times)) in enumerate(zip(got, want)):
        assert value == want_value, rank
        assert counts == want_counts, rank
        assert len(times) == len(want_times), rank
        if times:
            # (upload, kernels[, download]) ms: a thread that had made no call of its own would read zeros
            assert min(times) >= 0.0 and times[1] > 0.0 and sum(times) > 0.0, (rank, times)
    # ... and the workers' calls left the main thread's record alone
    assert (product.compress_last_times(), product.msa_stats_last_times()) == main_times
