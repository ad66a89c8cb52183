"""The T_ref count behind the one-plane test (csrc/cvd_bitslice.h, CVD_BS_TREF_FAST) on the
host: tests/tref_host_check.cpp compares the step's c with the exact four-plane formulation at
every layout phase, every received word and kUni false and true, over random, zero, c = 2,
c = 4 and pass-the-test-with-c-=-1 vectors, and asserts that a vector with c > 1 is always a
suspect.  Built as the header stands and with the knob off (the exact count in every lane):
both must pass and print the same digest of every step's planes, mu and c."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "tref_host_check.cpp")


def _run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", *flags, "-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.match(r"ok checked=(\d+) fast=(\d) c1=(\d+) c2=(\d+) c4=(\d+) suspects=(\d+) suspects_c1=(\d+) "
                 r"digest=([0-9a-f]{16})", out.stdout)
    assert m, out.stdout
    return [int(x) for x in m.groups()[:7]], m.group(8)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_tref_fast_count_equals_exact_count(tmp_path):
    on, d_on = _run(tmp_path, "tref_on", [])
    off, d_off = _run(tmp_path, "tref_off", ["-DCVD_BS_TREF_FAST=0"])
    assert on[1] == 1 and off[1] == 0
    assert on[0] == off[0] and on[2:] == off[2:] and d_on == d_off
    checked, _, c1, c2, c4, suspects, suspects_c1 = on
    # every kind of input occurred: c = 2, c = 4, and suspects whose exact count is 1
    assert c1 > 0 and c2 > 0 and c4 > 0 and suspects_c1 > 0
    assert suspects == c2 + c4 + suspects_c1


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_tref_host_check_clean_under_sanitizers(tmp_path):
    """the stand-alone program under AddressSanitizer and UBSan (host code only)"""
    exe = str(tmp_path / "tref_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-Wall", "-Werror", "-o", exe, SRC])
    out = subprocess.run([exe, "40"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok checked=")
