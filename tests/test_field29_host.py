"""The 29-bit-limb field and curve arithmetic (field29.cuh, curve29.cuh) against the saturated-limb implementation
(field.cuh, curve.cuh) on the host: tests/emu/test_field29.cpp and tests/emu/test_curve29.cpp, built by the system
C++ compiler with bound tracking on (F29_TRACK asserts every precondition) and run as child processes."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name,expect", [("field29", ["Fq29: ok", "Fr29: ok"]),
                                         ("curve29", ["bn256 (Fq29): ok", "grumpkin (Fr29): ok"])])
def test_f29_against_saturated(name, expect, tmp_path):
    exe = str(tmp_path / f"test_{name}")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-x", "c++", os.path.join(ROOT, "tests", "emu", f"test_{name}.cpp"),
                           "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and all(line in res.stdout.splitlines() for line in expect), res.stdout + res.stderr
