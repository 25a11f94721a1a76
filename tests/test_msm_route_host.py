"""The MSM route (mira_amd/csrc/msm_route.hip) on the host, on its own: tests/emu/test_msm_route.cpp, built by the system C++
compiler like the planner's program and run as a child process, prints what the route decides over a grid of keys, lengths,
counts and request flags, for the wide tables with n > 0, through a GLV copy that cannot be built and through trials under
scripted timings.  The output must match tests/golden/msm_route_decisions.txt line for line.  After a deliberate change of a
routing rule, regenerate that file from the program's output and review its diff.

That file pins the route from now on.  What ties it to the library as it was before the route had a file of its own is the
ABI trace (tests/msm_route_trace.py, tests/golden/msm_route_trace.txt, recorded on the library before the move): the rows
whose label starts with '@' are in both files, and their plan / table / shape columns must be equal."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SHARED_ROW = re.compile(r"^@(\S+) ([^:]+): (?:rc=0 )?plan=(\S+) table=(\S+) shape=(\S+)")
# every mode of the trace's matrix, its trials-off shapes and its empty requests over keys with wide tables
SHARED_MODES = {"glv-auto-off", "plain", "glv-auto", "glv-precomputed", "one-set", "two-sets", "two-sets-width-11", "handle-width-10", "process-width-7",
                "wide-opt-in", "trials-off", "tables-20", "tables-20-min-n-1", "tables-20-min-n-0", "tables-20-and-sets", "tables-20-and-sets-shared-min-n-1"}


def _lines(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return f.read().splitlines()


def _shared_rows(lines):
    rows = {}
    for line in lines:
        m = SHARED_ROW.match(line)
        if m:
            assert (m.group(1), m.group(2)) not in rows, line
            rows[(m.group(1), m.group(2))] = m.groups()[2:]
    return rows


def test_route_decisions_are_pinned(tmp_path):
    exe = str(tmp_path / "test_msm_route")
    csrc = os.path.join(ROOT, "mira_amd", "csrc")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-DMIRA_CPU_EMU", "-pthread", "-x", "c++", os.path.join(ROOT, "tests", "emu", "test_msm_route.cpp"),
                           os.path.join(csrc, "msm_route.hip"), os.path.join(csrc, "msm_plan.hip"), "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    want = _lines("msm_route_decisions.txt")
    got = res.stdout.splitlines()
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"line {i + 1}:\n  got  {g}\n  want {w}"
    assert len(got) == len(want), f"{len(got)} lines, want {len(want)}"


def test_route_decisions_agree_with_the_abi_trace():
    decided = _shared_rows(_lines("msm_route_decisions.txt"))
    traced = _shared_rows(_lines("msm_route_trace.txt"))
    assert set(decided) == set(traced), sorted(set(decided) ^ set(traced))
    assert {mode for mode, _ in traced} == SHARED_MODES
    for row, columns in traced.items():
        assert decided[row] == columns, (row, decided[row], columns)
