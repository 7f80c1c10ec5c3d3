"""The iterate ranges of the device-resident Newton-Raphson loop (pll-modules_amd/csrc/newton_range.hpp) on the CPU:
tests/newton_range_host_check.cpp drives the rule through sequences of loops -- max_newton 1, 30, 254, 255, 256, 300, the
bound and random ones, the counter from 0 and from just below 2^32 -- and holds every value a loop publishes or waits
for against a brute-force set of the values its control block can hold when it starts.  The rule before (sequence number
times 256) goes through the same checker, which has to reject it for the loop that follows one of 257 scans.  Built with
-fsanitize=address,undefined as a program of its own and run here."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ranges_never_meet_what_the_block_holds_under_sanitizers(tmp_path):
    csrc = os.path.join(ROOT, "pll-modules_amd", "csrc")
    exe = str(tmp_path / "newton_range_host_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-static-libasan", "-static-libubsan",
           "-I" + csrc, "-o", exe, os.path.join(ROOT, "tests", "newton_range_host_check.cpp")]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.strip().splitlines()
    assert lines[-1] == "ok"
    # the negative control: what the checker said of the rule before
    assert lines[0] == ("sequence number * 256: loop 1 waits for 513 after 1 scans: "
                        "loop 0 (max_newton 255) leaves it after 257 scans"), lines


def test_header_knows_nothing_of_the_engine():
    """standard headers only, so that the program above can test it"""
    with open(os.path.join(ROOT, "pll-modules_amd", "csrc", "newton_range.hpp")) as f:
        text = f.read()
    includes = [line.split()[1] for line in text.splitlines() if line.startswith("#include")]
    assert includes and all(i.startswith("<") for i in includes), includes
    for word in ("Engine *", "hip/", "hipError", "getenv", "static "):
        assert word not in text, word
