"""The route every MSM entry point takes, as the C ABI shows it (tests/msm_route_trace.py), on the device library: the same
fixed list of calls as on the emulation, held to the same tests/golden/msm_route_trace.txt, and the rows the emulation cannot
run: commits of 300 pairs through 20-bit tables, and the 16-bit windows of a sharded partial that names no width.  Nothing here
runs more than 2^12 pairs.

The rows that differ between emulation and device by construction are those whose width is planned from COLLECTED bit-length
statistics (DEVICE_ROWS).  k_digits samples the bit lengths into an LDS histogram and flushes it behind a __syncthreads; it is a
plain launch, whose lanes the emulation runs one after the other on one thread (tests/emu/emu.h: emu_launch), so there every lane
flushes its bins before the lanes after it have counted: the emulation's statistics are incomplete, and the width planned from
them is another.  The statistics never affect a result, and the route -- that they are collected and consumed at all -- is the
same.  For those rows the test compares everything but the width, and checks that the windows cover the scalars of one of the
two paths (256 bits, or the 128 of the halves of the GLV split: with other statistics choose_glv may decide otherwise too).
What a given histogram makes of a route is pinned on the host (tests/emu/test_msm_route.cpp: "stats").
(plan_reduction's smaller workgroups under emulation change only kappa and gamma, which the ABI does not show.)"""
import re

import pytest

import msm_route_trace
from msm_route_trace import assert_same_lines, golden_lines

DEVICE_ROWS = {"stats 2 same length n=4096", "stats 4 glv n=3000", "stats 5 glv n=3000 again"}
PLAN = re.compile(r"plan=(\d+),(\d+)")


def _device_view(lines):
    """the trace with the widths of DEVICE_ROWS blanked, after checking them for consistency"""
    out = []
    for line in lines:
        if line.split(":")[0] in DEVICE_ROWS:
            c, w = map(int, PLAN.search(line).groups())
            assert 4 <= c <= 16 and w in (-(-256 // c), -(-128 // c)), line
            line = PLAN.sub("plan=*", line)
        out.append(line)
    return out


@pytest.mark.gpu
def test_routes_through_the_abi_are_the_recorded_ones(gpu_lib):
    assert_same_lines(_device_view(msm_route_trace.run(gpu_lib)), _device_view(golden_lines()))


@pytest.mark.gpu
def test_wide_tables_and_the_width_of_a_sharded_partial(gpu_lib):
    """A key of 2^12 points with 20-bit tables and MIRA_TUNE_TABLE_MIN_N = 1, n = 300: mira_msm_last_plan (0, 64),
    mira_msm_last_table_bits 20, partials of shape (0, 64), the oracle's point -- as capi.hip's table branch has always
    answered.  Before the tables are built, a sharded partial with width 0 takes 16-bit windows whatever its length."""
    assert_same_lines(msm_route_trace.run_wide_tables(gpu_lib), [
        "plain key sharded partial first=10 n=300 width=0: rc=0 plan=16,16 table=0 shape=16,16 ok=1",
        "tables-20 device n=300: rc=0 plan=0,64 table=20 shape=- ok=1",
        "tables-20 host n=300: rc=0 plan=0,64 table=20 shape=- ok=1",
        "tables-20 partial first=10 n=300 width=0: rc=0 plan=0,64 table=20 shape=0,64 ok=1",
        "tables-20 partial to device first=10 n=300 width=0: rc=0 plan=0,64 table=20 shape=0,64 ok=1",
    ])
