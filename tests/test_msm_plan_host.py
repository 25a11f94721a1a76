"""The MSM planner (mira_amd/csrc/msm_plan.hip) on the host, on its own: tests/emu/test_msm_plan.cpp, built by the system C++
compiler and run as a child process, prints the planner's decisions over a grid of commit shapes -- widths, windows, pieces,
plain path or GLV split, which shared-bucket set -- and the widths and sets the trial machines walk under scripted timings.
They must match tests/golden/msm_plan_decisions.txt line for line.  After a deliberate change of the measured tables or of a
rule, regenerate that file from the program's output and review its diff."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_planner_decisions_are_pinned(tmp_path):
    exe = str(tmp_path / "test_msm_plan")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-DMIRA_CPU_EMU", "-pthread", "-x", "c++",
                           os.path.join(ROOT, "tests", "emu", "test_msm_plan.cpp"), os.path.join(ROOT, "mira_amd", "csrc", "msm_plan.hip"),
                           "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    with open(os.path.join(ROOT, "tests", "golden", "msm_plan_decisions.txt")) as f:
        want = f.read().splitlines()
    got = res.stdout.splitlines()
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"line {i + 1}:\n  got  {g}\n  want {w}"
    assert len(got) == len(want), f"{len(got)} lines, want {len(want)}"
