"""The chain planner (pll-modules_amd/csrc/chain_plan.cpp) on the CPU: tests/chain_plan_host_check.cpp plans every case
of tests/golden/chain_plans.txt again, compares each plan exactly with the recorded one and holds it against the
planner's invariants -- built with -fsanitize=address,undefined as a program of its own and run here."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plans_match_recorded_under_sanitizers(tmp_path):
    csrc = os.path.join(ROOT, "pll-modules_amd", "csrc")
    exe = str(tmp_path / "chain_plan_host_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-static-libasan", "-static-libubsan",
           "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-o", exe,
           os.path.join(ROOT, "tests", "chain_plan_host_check.cpp"), os.path.join(csrc, "chain_plan.cpp")]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "chain_plans.txt")], capture_output=True, text=True,
                         timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().endswith("ok")


def test_module_knows_nothing_of_the_engine():
    """the planner's boundary: pll.h and standard headers, no engine, no HIP, no environment, no statics"""
    csrc = os.path.join(ROOT, "pll-modules_amd", "csrc")
    for name in ("chain_plan.hpp", "chain_plan.cpp"):
        with open(os.path.join(csrc, name)) as f:
            text = f.read()
        includes = [line.split()[1] for line in text.splitlines() if line.startswith("#include")]
        assert all(i.startswith("<") or i in ('"pll.h"', '"chain_plan.hpp"') for i in includes), (name, includes)
        for word in ("Engine", "hip", "getenv", "static "):
            assert word not in text, (name, word)
