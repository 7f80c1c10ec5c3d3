"""The CPU oracle against the reference's own golden vectors.

Two layers of pinning:
 1. `test_reference_programs_*`: the reference's OWN test programs blopt-minimal.c /
    blopt-5states.c and its OWN optimiser sources (src/optimize/*.c), compiled where
    they lie against include/pll.h and linked with the oracle by oracle/Makefile.ref
    (build() makes oracle/_ref/ where a pll-modules checkout is present), are run and
    their stdout is compared byte for byte with the reference's golden .out files
    (tests/golden/) -- the same check test/runtest.py performs.
 2. `test_fixture_*`: the same numbers through the C ABI from Python with the
    committed fixtures (tests/golden/blopt_fixtures.json), runnable anywhere.
"""
import os
import subprocess

import pytest

import common


def _run(name, args):
    exe = common.ref_program(name)
    return subprocess.run([exe, *args], check=True, capture_output=True, text=True, env=common.ref_env()).stdout


@pytest.mark.parametrize("name,args", [("blopt-minimal", []), ("blopt-minimal", ["avx"]),
                                       ("blopt-5states", []), ("blopt-5states", ["tv"])])
def test_reference_programs_reproduce_golden_output(oracle, name, args):
    out = _run(name, args)
    golden = open(os.path.join(common.GOLDEN, name + ".out")).read()
    assert out == golden


@pytest.mark.parametrize("name,coded", [("blopt-minimal", False), ("blopt-5states", False),
                                        ("blopt-5states", True)])
def test_fixture_through_c_abi(oracle, name, coded):
    expected, got = common.run_golden_case(oracle, name, coded=coded)
    common.check_golden(expected, got)


def test_gamma_rates_mean_mode(oracle):
    # Yang-1994 mean discretisation, alpha = 0.841, K = 4
    r = oracle.gamma_cats(0.841, 4)
    assert abs(r.mean() - 1.0) < 1e-7
    for got, exp in zip(r, [0.10424838, 0.42313162, 0.96769858, 2.50492142]):
        assert abs(got - exp) < 5e-7
