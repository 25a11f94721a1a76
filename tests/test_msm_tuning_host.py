"""A key's MSM tuning as bytes (mira_amd/csrc/msm_tuning.hip) on the host, on its own: tests/emu/test_msm_tuning.cpp, built by
the system C++ compiler from the three host-only sources (planner, route, serialiser) like the route's program, finishes trials
under scripted timings, exports, imports into fresh keys and looks at what the unchanged route then decides; it offers the
reader every malformed blob include/mira_gpu.h names, every truncation and every single changed byte of a valid one.  The
second build runs the same program under AddressSanitizer and UBSan: the reader takes bytes from disk, and a read beyond them
shows there."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["finish, export, import", "statistics slot", "round trip", "batch", "set trial", "identity", "malformed", "robustness", "lru"]


def _build(exe, extra=()):
    csrc = os.path.join(ROOT, "mira_amd", "csrc")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-DMIRA_CPU_EMU", "-pthread", *extra, "-x", "c++", os.path.join(ROOT, "tests", "emu", "test_msm_tuning.cpp"),
                           os.path.join(csrc, "msm_tuning.hip"), os.path.join(csrc, "msm_route.hip"), os.path.join(csrc, "msm_plan.hip"), "-o", exe])
    return exe


def _run(exe, env=None):
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = res.stdout.splitlines()
    assert [line for line in lines if not line.startswith("ok ")] == ["all ok"], res.stdout
    for case in CASES:
        assert any(line.startswith("ok " + case) for line in lines), (case, res.stdout)


def test_tuning_blobs_on_the_host(tmp_path):
    _run(_build(str(tmp_path / "test_msm_tuning")))


def test_tuning_blobs_under_the_sanitizers(tmp_path):
    exe = _build(str(tmp_path / "test_msm_tuning_san"), ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan"])
    _run(exe, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1"))   # (out-of-bounds reads are the point, not leaks)
