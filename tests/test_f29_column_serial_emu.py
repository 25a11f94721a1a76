"""The column-serial multipliers of field29.cuh (f29_mul, f29_sqr, f29_mul2_add, f29_redc: one multiply-add chain per column,
seeded with the carry of the column before) against the in-place forms they replace, on the host:
tests/emu/test_f29_column_serial.cpp compares every column and every output limb on operands at the documented limits
(tests/emu/f29_operands.h) for both fields.  Built by the system C++ compiler and run as a child process, once plain and once
under the undefined-behaviour and address sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emu", "test_f29_column_serial.cpp")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=undefined"]],
                         ids=["plain", "sanitized"])
def test_column_serial_against_in_place(flags, tmp_path):
    exe = str(tmp_path / "test_f29_column_serial")
    subprocess.check_call(["g++", *flags, "-std=c++17", "-pthread", "-x", "c++", SRC, "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    lines = res.stdout.splitlines()
    assert res.returncode == 0 and len(lines) == 2, res.stdout + res.stderr
    assert lines[0].startswith("Fq29: ") and lines[0].endswith(": ok") and lines[1].startswith("Fr29: ") and lines[1].endswith(": ok"), res.stdout
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr
