"""The segment geometry of k_accumulate (tests/segment_geometry.py) on the CPU emulation: the bound tracking, the bucket walk, the
indices of the staged stream and the host-side buffer sizing are the same code there; the copies into LDS are memcpy.  The shaped
cases at every L of the sweep, a short dense list, every launch sequence at a few L, and tests/emu/test_segment_sweep.cpp -- a
program of its own over the emulation build of the library sources -- under AddressSanitizer and UBSan, for the workspaces."""
import os
import subprocess

import pytest

import segment_geometry as SG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DENSE_L = (1, 3, 16, 17, 33, 65)
SEQUENCE_L = (3, 17, 33)


ARGS = [list(DENSE_L), [0, 1, 5], list(SEQUENCE_L)]


@pytest.fixture(scope="module")
def child(emu_lib):
    """One process runs every case on one library and one set of keys: the emulation holds k_accumulate to its own rules with
    assertions (a staged block begins 16-byte aligned and holds an entry of its lane's segment), and an assertion ends the process.
    -> (the finished process, what it printed per case)"""
    import json
    import sys
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "segment_geometry.py"), emu_lib.path, json.dumps(ARGS)], capture_output=True, text=True, timeout=1800)
    sections, at = {}, None
    for line in res.stdout.splitlines():
        if line.startswith("run "):
            at = line[4:]
        sections.setdefault(at, []).append(line)
    return res, sections


def ran(child, name):
    res, sections = child
    assert name in SG.specs(*ARGS)
    lines = sections.get(name)
    if lines and f"ok {name}" in lines:
        return
    if lines and f"failed {name}" in lines:
        pytest.fail("\n".join(lines)[-4000:], pytrace=False)
    if lines:                                                              # it began and neither passed nor raised: the process ended in it
        pytest.fail(f"exit status {res.returncode} in case {name}\n" + "\n".join(lines)[-2000:] + "\n" + res.stderr[-4000:], pytrace=False)
    last = [c for c in sections if c][-1] if any(sections) else None
    pytest.fail(f"not reached: the child ended with exit status {res.returncode} in the earlier case {last}\n{res.stderr[-1500:]}", pytrace=False)


def test_the_model_on_a_hand_made_list():
    """L = 5 over runs 3, -, 4, 1, 9: segments [0,5) [5,10) [10,15) [15,17)"""
    segs = list(SG.segments(5, [3, 0, 4, 1, 9]))
    assert [(s.start, s.end, s.a, s.span, s.nb) for s in segs] == [(0, 5, 0, 5, 1), (5, 10, 1, 6, 1), (10, 15, 2, 7, 1), (15, 17, 3, 5, 1)]
    assert [s.run_end_offsets for s in segs] == [[3], [3, 4], [], []] and segs[-1].overhang == 12 + 16 - 17
    segs = list(SG.segments(33, [40, 26]))
    assert [(s.a, s.span, s.nb, s.cls) for s in segs] == [(0, 33, 3, (0, 3, 1)), (1, 34, 3, (1, 3, 2))] and segs[1].run_end_offsets == [8]
    assert SG.segment_length(10, 1000) == 10 and SG.segment_length(10, 196608 * 10 + 1) == 11
    assert SG.class_of(0, 64) == (0, 4, 0) and SG.class_of(3, 68) == (3, 4, 2) and (3, 1, 1) not in SG.reachable_classes()


def test_the_builders_give_the_counts_they_were_asked_for():
    v = SG.shaped("x", 8, [2, 0, 1] + [1] * 130, 1)
    assert v.n == 133 and v.counts[:3] == [2, 0, 1] and v.counts[127] == 0 and v.counts[128] == 1 and v.total == 133
    d = SG.dense("y", 9, 50, 2, full=True)
    assert d.total == 50 * 29 and max(d.values) < 1 << 253


def test_the_cases_reach_every_class():
    reachable, reached = SG.check_coverage()
    assert reachable == reached
    assert {c.vector.c for c in SG.cases()} == {8, 13} and {c.curve for c in SG.cases()} == {0, 1}
    assert all(1000 <= c.vector.n <= 4100 for c in SG.cases() + SG.dense_cases())
    assert set(SG.SWEEP) >= {1, 2, 3, 5, 10, 13, 15, 16, 17, 19, 31, 32, 33, 47, 48, 49, 65} and max(SG.SWEEP) <= 65


def test_unsupported_values_of_the_knob_are_refused(emu_lib):
    SG.check_knob_refusals(emu_lib)


@pytest.mark.parametrize("k", range(len(SG.cases())), ids=[c.name for c in SG.cases()])
def test_shaped(child, k):
    ran(child, f"shaped {k}")


@pytest.mark.parametrize("vector", ARGS[1])
def test_dense(child, vector):
    """the dense vector at L = 1, 3, 16, 17, 33, 65; the full ones behind a trim"""
    ran(child, f"dense {vector}")


@pytest.mark.parametrize("name", SG.OTHER_SEQUENCES)
def test_launch_sequences(child, name):
    """the GLV split, the wide front, a shared-bucket set, a batch of 3, passes and host chunks at L = 3, 17, 33"""
    ran(child, f"sequence {name}")


def test_segment_sweep_under_the_sanitizers(tmp_path):
    """tests/emu/test_segment_sweep.cpp: synthetic vectors committed at every L of the sweep, each point compared with the same commit
    at the default L; its purpose is the sanitizers' view of the workspaces at segment lengths nobody ran before"""
    csrc = os.path.join(ROOT, "mira_amd", "csrc")
    srcs = ["capi.hip", "msm_plan.hip", "msm_route.hip", "msm_tuning.hip", "msm_bn256.hip", "msm_grumpkin.hip", "ntt.hip", "fold.hip", "lookup.hip", "decide.hip",
            "setup.hip", "graph.hip", "graph_compile.hip", "graph_jit.hip"]
    flags = ["-O1", "-g", "-std=c++17", "-DMIRA_CPU_EMU", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
             "-Wno-unknown-pragmas", "-Wno-attributes"]
    units = [os.path.join(ROOT, "tests", "emu", "test_segment_sweep.cpp")] + [os.path.join(csrc, s) for s in srcs]
    objs = [str(tmp_path / (os.path.basename(u) + ".o")) for u in units]
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:     # one compiler per translation unit: the two curves' kernels dominate
        list(pool.map(lambda uo: subprocess.check_call(["g++", *flags, "-x", "c++", "-c", uo[0], "-o", uo[1]], cwd=csrc), zip(units, objs)))
    exe = str(tmp_path / "test_segment_sweep_san")
    subprocess.check_call(["g++", "-pthread", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", *objs, "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=1500, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-6000:]
    lines = res.stdout.splitlines()
    assert lines[-1] == "all ok" and sum(1 for line in lines if line.startswith("ok L=")) == len(SG.SWEEP), res.stdout[-3000:]
    for L in SG.SWEEP:
        assert any(line.startswith(f"ok L={L} ") for line in lines), (L, res.stdout[-3000:])
