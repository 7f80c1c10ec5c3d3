"""Loop control of the device-resident Newton-Raphson loop (include/pllhip.h, pllhip_newton_branch) on one partition:
loops of more scans than any range of 256 iterate values holds, loops one after the other on the same control block,
every way a loop can end, and the state they leave behind.  The workgroups of a loop hand iterates to one another
through one word of the control block that the host does not write between loops (csrc/newton_range.hpp); a loop that
finds a value of an earlier loop there runs on with a stale iterate.

The reference is the host loop (tests/newton_cases.py, host_newton) over the partition's own blocking
pll_compute_likelihood_derivatives, bit for bit: scans, final length, the first min(scans, 96) iterates.  Every test
asserts on the host loop's course that its input still does what the case is about before it compares.  Scans of the
host loop on the product's derivatives (MI355X), all four families alike: 257, 301, 256 and 255 for the walks down to
bl_min, 256 evaluations (257 device scans) for the loop that meets the limit, 1 for the non-finite derivatives; the
ordinary loop makes 26 (4 states), 29 (20), 18 (61) and 28 (10), 15, 15, 13 and 15 of them before the first f' > 0 --
the counts the oracle's derivatives give too: no starting length had to be moved.

The several-partition cases are in tests/test_eval_driver.py (test_device_newton_back_to_back_over_several_partitions)."""
import math

import pytest

import newton_cases as nc
import pllhip_ctypes as pc

pytestmark = pytest.mark.gpu

FAMILIES = [4, 20, 61, 10]
FIRST_LOOPS = [nc.LONG_257, nc.LONG_301, nc.LONG_256, nc.LONG_255, nc.LIMIT_257, nc.NONFINITE_1]


def _id(loop):
    return {nc.CONVERGED: "converged", nc.LIMIT: "limit", nc.NONFINITE: "nonfinite"}[loop.status] + f"_after_{loop.scans}"


@pytest.mark.parametrize("first", FIRST_LOOPS, ids=_id)
@pytest.mark.parametrize("states", FAMILIES)
def test_loops_back_to_back(product, states, first):
    """loop A, then an ordinary loop B on the same partition: B makes the host loop's iterates whatever A left in the
    control block -- the last value of a range of 257 or 301, of 256 or 255, of a loop that met the limit after 257
    scans, of one that ended on non-finite derivatives after 1 --, so does a third loop, and the blocking derivative
    call afterwards returns what it returned before A: the tickets of the reductions are where they have to be"""
    with nc.Part(product, states, coded=first.data != "zero_site") as p:
        # B's reference first, before anything A may have left behind
        p.load(nc.ORDINARY.data)
        before = p.derivatives(0.3)
        course_b = nc.host_course(p.derivatives, nc.ORDINARY)
        nc.check_course(course_b, nc.ORDINARY)
        print(f"states {states}: the ordinary loop makes {course_b.evaluations} scans, "
              f"{course_b.leading_nonpositive} of them before the first f' > 0")

        p.load(first.data)
        course_a = nc.host_course(p.derivatives, first)
        nc.check_course(course_a, first)
        print(f"states {states}: {_id(first)}: {course_a.evaluations} evaluations of the host loop, "
              f"{nc.device_scans(course_a)} scans of the device loop")
        nc.run_and_compare(p.newton, first, course_a)

        p.load(nc.ORDINARY.data)
        nc.run_and_compare(p.newton, nc.ORDINARY, course_b)
        nc.run_and_compare(p.newton, nc.ORDINARY, course_b)
        assert p.derivatives(0.3) == before


@pytest.mark.parametrize("states", FAMILIES)
def test_a_long_loop_keeps_its_first_96_iterates(product, states):
    """301 scans: *iterations says so, the final length is the host loop's, and the trail holds the iterates after the
    first 96 scans -- before and after another loop has used the mapped result buffer"""
    with nc.Part(product, states) as p:
        p.load(nc.LONG_301.data)
        course = nc.host_course(p.derivatives, nc.LONG_301)
        nc.check_course(course, nc.LONG_301)
        for _ in range(2):
            length, iterations, trail = p.newton(nc.LONG_301)
            assert iterations == 301 and len(trail) == 96
            assert list(trail) == course.trail[:96]
            assert length == course.x


@pytest.mark.parametrize("states", FAMILIES)
def test_every_exit_of_the_loop(product, states):
    """converged at bl_min from above (the step ends at the bracket), converged on |f| < tol and on |step| < tol at an
    interior optimum, the iteration limit (910: max_newton + 2 scans, the host loop gives up before its evaluation
    max_newton + 2), max_newton at the bound (accepted) and beyond it (912, nothing ran); non-finite derivatives (911)
    are test_non_finite_derivatives_end_the_loop"""
    with nc.Part(product, states) as p:
        p.load("identical")
        at_bracket = nc.Loop("identical", 0.5, nc.TOL, 32, nc.CONVERGED, None)
        course = nc.host_course(p.derivatives, at_bracket)
        nc.check_course(course, at_bracket)
        assert course.trail[-3] > course.trail[-2] and course.evaluations < 8
        nc.run_and_compare(p.newton, at_bracket, course)

        p.load("simulated")
        on_f, course_f = nc.course_ending_on_f(p.derivatives)
        print(f"states {states}: start {on_f.start:.2f} ends on |f| < tol after {course_f.evaluations} scans")
        nc.run_and_compare(p.newton, on_f, course_f)

        course_b = nc.host_course(p.derivatives, nc.ORDINARY)
        nc.check_course(course_b, nc.ORDINARY)
        on_step = nc.ORDINARY
        if course_b.by_f:          # (which of the two tests ends the ordinary loop hangs on the last bits: see course_ending_on_f)
            on_step = next(l for l in (nc.ORDINARY._replace(start=s) for s in (4.0, 3.0, 6.0, 2.0, 7.0, 8.0))
                           if not nc.host_course(p.derivatives, l).by_f)
            course_b = nc.host_course(p.derivatives, on_step)
            assert course_b.status == nc.CONVERGED and not course_b.at_bracket
        nc.run_and_compare(p.newton, on_step, course_b)

        course_l = nc.host_course(p.derivatives, nc.LIMIT_257)
        nc.check_course(course_l, nc.LIMIT_257)
        with pytest.raises(pc.NewtonError, match="910") as err:
            p.newton(nc.LIMIT_257)
        assert err.value.iterations == nc.LIMIT_257.max_newton + 2 == course_l.evaluations + 1 == 257
        assert err.value.length == course_l.x
        assert list(err.value.trail) == course_l.trail[:96]

        # the bound: from the optimum the loop needs a scan or two at any step cap
        at_bound = nc.Loop("simulated", course_b.x, nc.TOL, pc.PLLHIP_NEWTON_MAX_ITERATIONS, nc.CONVERGED, None)
        course = nc.host_course(p.derivatives, at_bound)
        assert course.status == nc.CONVERGED and course.evaluations <= 3
        nc.run_and_compare(p.newton, at_bound, course)
        with pytest.raises(pc.NewtonError, match="912") as err:
            p.newton(at_bound._replace(max_newton=pc.PLLHIP_NEWTON_MAX_ITERATIONS + 1))
        assert err.value.iterations == 0 and math.isnan(err.value.length)
        nc.run_and_compare(p.newton, on_step, course_b)


@pytest.mark.parametrize("states", FAMILIES)
def test_non_finite_derivatives_end_the_loop(product, states):
    """a tip vector that is all zero at one site: the site's likelihood is 0 and both derivatives of the blocking call
    are not finite; the loop ends after its first scan with PLLHIP_ERROR_NEWTON_DERIVATIVES, the iterate where it was"""
    with nc.Part(product, states, coded=False) as p:
        p.load("zero_site")
        f, df = p.derivatives(nc.NONFINITE_1.start)
        assert not math.isfinite(f) or not math.isfinite(df), (f, df)
        course = nc.host_course(p.derivatives, nc.NONFINITE_1)
        nc.check_course(course, nc.NONFINITE_1)
        with pytest.raises(pc.NewtonError, match="911") as err:
            p.newton(nc.NONFINITE_1)
        assert err.value.iterations == 1
        assert err.value.length == nc.NONFINITE_1.start
        assert list(err.value.trail) == [nc.NONFINITE_1.start]
