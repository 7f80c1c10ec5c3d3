"""The ledger of unstored vectors (pll-modules_amd/csrc/unstored.cpp) on the CPU: tests/unstored_host_check.cpp drives it
with hand-built operation lists, compares what it answers with written-out values and holds its fields against its
invariants after every change -- built with -fsanitize=address,undefined as a program of its own and run here."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ledger_rules_under_sanitizers(tmp_path):
    csrc = os.path.join(ROOT, "pll-modules_amd", "csrc")
    exe = str(tmp_path / "unstored_host_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-static-libasan", "-static-libubsan",
           "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-o", exe,
           os.path.join(ROOT, "tests", "unstored_host_check.cpp"), os.path.join(csrc, "unstored.cpp")]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().endswith("ok")


def test_module_knows_nothing_of_the_engine():
    """the ledger's boundary: pll.h, pllhip.h (the two statistics records) and standard headers, no engine, no HIP, no
    environment, no statics"""
    csrc = os.path.join(ROOT, "pll-modules_amd", "csrc")
    for name in ("unstored.hpp", "unstored.cpp"):
        with open(os.path.join(csrc, name)) as f:
            text = f.read()
        includes = [line.split()[1] for line in text.splitlines() if line.startswith("#include")]
        assert all(i.startswith("<") or i in ('"pll.h"', '"pllhip.h"', '"unstored.hpp"') for i in includes), (name, includes)
        # (the public header and its names -- pllhip.h, pllhip_*_stats -- are the one place "hip" may stand in)
        for word in ("Engine", "hip", "getenv", "static "):
            assert word not in text.replace("pllhip", ""), (name, word)
