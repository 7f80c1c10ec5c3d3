"""Inputs and the host reference of the loop-control tests of the device-resident Newton-Raphson loop
(tests/test_newton_loop_control.py; the several-partition cases of tests/test_eval_driver.py).

Every input is a 9-tip partition on pc.Tree(9, 42, 43), rooted at its first edge whose two ends are inner nodes, and a
loop (start, tolerance, max_newton) on that edge whose course the tests assert on the host loop before they compare:

  LONG_257      identical sequences at all tips, start 8.5334, max_newton 300: every derivative pair has f > 0 and
                f' <= 0 with -f / |f'| near -8, so every step is clamped to -dxmax = -10 / 300 and the loop walks down to
                bl_min, where it converges at the bracket after exactly 257 scans
  LONG_301      the same from 10.0: 301 scans, more than the 96 iterates the trail keeps
  LONG_256/255  the same from 10.0 with max_newton 255 / 254: 256 / 255 scans, the limit not reached
  LIMIT_257     simulated sequences, start 0.1, tolerance 0, max_newton 255: never converges; the host loop gives up
                after 256 evaluations, the device after max_newton + 2 = 257 scans (PLLHIP_ERROR_NEWTON_LIMIT, 910)
  ORDINARY      simulated sequences, start 5.0, max_newton 32: an interior optimum after 18 to 29 scans (20 and 22 for
                the pairs of partitions), the first 13 to 15 of them in the f' <= 0 branch
  NONFINITE     a vector tip whose vector is all zero at one site (no invariant sites): the site likelihood is 0, both
                derivatives are not finite: PLLHIP_ERROR_NEWTON_DERIVATIVES (911) after one scan"""
import math
from collections import namedtuple

import numpy as np

import pllhip_ctypes as pc

BL_MIN, BL_MAX, TOL = 1e-4, 10.0, 1e-5
CONVERGED, LIMIT, NONFINITE = 0, 910, 911
TRAIL_MAX = 96

Loop = namedtuple("Loop", "data start tol max_newton status scans")
LONG_257 = Loop("identical", 8.5334, TOL, 300, CONVERGED, 257)
LONG_301 = Loop("identical", 10.0, TOL, 300, CONVERGED, 301)
LONG_256 = Loop("identical", 10.0, TOL, 255, CONVERGED, 256)
LONG_255 = Loop("identical", 10.0, TOL, 254, CONVERGED, 255)
LIMIT_257 = Loop("simulated", 0.1, 0.0, 255, LIMIT, 257)
ORDINARY = Loop("simulated", 5.0, TOL, 32, CONVERGED, None)
NONFINITE_1 = Loop("zero_site", 0.1, TOL, 32, NONFINITE, 1)

# what one run of the host loop did: how it ended, where, the iterate after every evaluation, the evaluations made,
# how many of them took the f' <= 0 branch from the start on, how many steps were cut to +-dxmax, whether the last step
# ended at the bracket (dx = xl - x or xh - x) and whether the loop stopped on |f| < tol
Course = namedtuple("Course", "status x trail evaluations leading_nonpositive clamped at_bracket by_f")


def host_newton(deriv, x, bl_min, bl_max, tol, max_newton):
    """the step rule of newton() (csrc/host/pllhip_eval.c; reference: src/optimize/opt_algorithms.c:133-261) in Python
    floats (IEEE doubles, no contraction), as _host_newton of tests/test_eval_driver.py, but it returns how the loop ended
    instead of raising"""
    dxmax = bl_max / max_newton
    xl, xh = bl_min, bl_max
    x = max(min(x, bl_max), bl_min)
    trail = []
    it = leading = clamped = 0
    lead = True
    while True:
        if it > max_newton:
            return Course(LIMIT, x, trail, it, leading, clamped, False, False)
        it += 1
        f, df = deriv(x)
        if not math.isfinite(f) or not math.isfinite(df):
            trail.append(x)
            return Course(NONFINITE, x, trail, it, leading, clamped, False, False)
        if df > 0.0:
            lead = False
            if abs(f) < tol:
                trail.append(x)
                return Course(CONVERGED, x, trail, it, leading, clamped, False, True)
            if f < 0.0:
                xl = x
            else:
                xh = x
            dx = -f / df
        else:
            leading += 1 if lead else 0
            dx = -f / abs(df)
        clamped += 1 if abs(dx) > dxmax else 0
        dx = max(min(dx, dxmax), -dxmax)
        bracket = False
        if x + dx < xl:
            dx, bracket = xl - x, True
        if x + dx > xh:
            dx, bracket = xh - x, True
        if abs(dx) < tol:
            trail.append(x)
            return Course(CONVERGED, x, trail, it, leading, clamped, bracket, False)
        x += dx
        x = max(min(x, bl_max), bl_min)
        trail.append(x)


def device_scans(course):
    """scans of the device loop for this course: it makes the scan on which it finds the limit exceeded"""
    return course.evaluations + (1 if course.status == LIMIT else 0)


def rooted_tree():
    tree = pc.Tree(9, 42, 43)
    edge = next(k for k, (u, v) in enumerate(tree.edges) if u >= tree.ntips and v >= tree.ntips)
    tree.set_root_edge(edge)
    return tree


def sites_of(states):
    return 5000 if states <= 20 else 800


def workgroups(states, nsites, rate_cats=4):
    """workgroups of the loop's launch: the derivative scan's own grid (pll_core.hip, scan_grid: reduce_grid -- the
    family's reduce_need under its cap -- under four per CU and under what the chip holds of the loop kernel at once,
    neither of which binds at these sizes).  A loop of one workgroup hands nothing over."""
    if states == 4:
        return (nsites * rate_cats + 1023) // 1024
    return ((nsites + 31) // 32 + 3) // 4


class Part:
    """one partition on the rooted tree, its sumtable on the root edge; load() gives it another alignment -- the
    engine, and with it the loop's control block, the reduction tickets and the counter of the iterate ranges, stays"""

    def __init__(self, lib, states, coded=True, seed_shift=0):
        self.states, self.seed_shift = states, seed_shift
        self.tree = rooted_tree()
        self.nsites = sites_of(states)
        assert workgroups(states, self.nsites) > 1
        self.inst = pc.build_instance(lib, states=states, rate_cats=4, ntips=self.tree.ntips, nsites=self.nsites,
                                      coded=coded, tree=self.tree, seed_shift=seed_shift)
        self.sa, self.sb = self.tree.scaler_of(self.tree.root_a), self.tree.scaler_of(self.tree.root_b)
        self.st = self.inst.alloc_sumtable()
        self.data = None

    def close(self):
        self.inst.free_sumtable(self.st)
        self.inst.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def load(self, data):
        """"identical", "simulated" or "zero_site" (vector tips only); traversal and sumtable follow"""
        a, tree = self.inst, self.tree
        if data != self.data:
            if data == "identical":
                codes = np.tile(pc.random_codes(1, self.nsites, self.states, 44 + self.seed_shift), (tree.ntips, 1))
            else:
                codes = pc.simulated_codes(tree, self.nsites, self.states, 45 + self.seed_shift)
            cmap = pc.state_charmap(self.states)
            for t in range(tree.ntips):
                a.set_tip_states(t, cmap, (codes[t] + 48).tobytes())
            if data == "zero_site":
                vec = np.zeros((self.nsites, self.states))
                vec[np.arange(self.nsites), codes[3]] = 1.0
                vec[self.nsites // 2] = 0.0
                a.set_tip_clv(3, vec.ravel())
            self.data = data
        pc.full_traversal(a)
        a.update_sumtable(tree.root_a, tree.root_b, self.sa, self.sb, self.st)
        return self

    def derivatives(self, x):
        return self.inst.derivatives(self.sa, self.sb, x, self.st)

    def newton(self, loop):
        return self.inst.newton_branch(self.sa, self.sb, self.st, loop.start, BL_MIN, BL_MAX, loop.tol, loop.max_newton)


def host_course(deriv, loop):
    return host_newton(deriv, loop.start, BL_MIN, BL_MAX, loop.tol, loop.max_newton)


def course_ending_on_f(deriv):
    """A loop on the simulated sequences that stops on |f| < tol at an interior optimum: (loop, course).  Newton steps
    near the optimum square: |f| after a step d is about C d^2 with C of the order of f', which is in the thousands
    here, so |f| < tol comes before |step| < tol only when a step falls between tol and sqrt(tol / C) -- which of the
    two ends a loop hangs on the last bits of the derivatives.  With tol = 1e-8 about two starts in five end on |f|
    (the window is wider on the logarithmic scale on which the steps shrink); the first of 24 starts that does is
    taken, decided by the host loop alone."""
    for k in range(24):
        loop = Loop("simulated", 0.05 + 0.4 * k, 1e-8, 32, CONVERGED, None)
        course = host_course(deriv, loop)
        if course.status == CONVERGED and course.by_f and 0.01 < course.x < 1.0:
            return loop, course
    raise AssertionError("no start gives a host loop that ends on |f| < tol")


def run_and_compare(run, loop, course):
    """run(loop) -> (length, iterations, trail) of the device loop, or NewtonError: against the host course"""
    if course.status == CONVERGED:
        compare(*run(loop), course)
        return
    try:
        run(loop)
    except pc.NewtonError as err:
        assert err.errno == course.status, (str(err), course.status)
        compare(err.length, err.iterations, err.trail, course)
    else:
        raise AssertionError(f"the device loop converged, the host loop ended with {course.status}")


def check_course(course, loop):
    """the precondition of a test: the host loop did on this input what the case is about"""
    assert course.status == loop.status, (loop, course.status, course.evaluations)
    if loop.scans is not None:
        assert device_scans(course) == loop.scans, (loop, course.evaluations)
    if loop.data == "identical":
        # every scan in the f' <= 0 branch, every step but the last ones cut to dxmax, the end at the lower bracket
        # (the step onto the bracket, x += xl - x, is rounded: the last iterate is bl_min to an ulp or so)
        assert course.leading_nonpositive == course.evaluations and course.at_bracket, course[3:]
        assert abs(course.x - BL_MIN) < 1e-12 and course.clamped >= course.evaluations - 2, (course.x, course[3:])
    if loop is LIMIT_257:
        assert course.evaluations == loop.max_newton + 1
    if loop is ORDINARY:
        assert course.evaluations <= loop.max_newton and course.leading_nonpositive >= 10, course[3:]
        assert 0.01 < course.x < 1.0 and not course.at_bracket, (course.x, course[3:])


def compare(got_length, got_iterations, got_trail, course):
    """the device loop against the host course, bit for bit: scans, final length, the first min(scans, 96) iterates"""
    scans = device_scans(course)
    assert got_iterations == scans, (got_iterations, scans)
    assert got_length == course.x, (got_length, course.x)
    keep = min(course.evaluations, TRAIL_MAX)
    assert len(got_trail) == min(scans, TRAIL_MAX)
    assert list(got_trail[:keep]) == course.trail[:keep]
    if course.status == LIMIT and scans <= TRAIL_MAX:
        assert got_trail[scans - 1] == course.x        # the scan that finds the limit exceeded leaves the iterate alone
