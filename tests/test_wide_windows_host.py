"""Host-side rules of the 17- to 20-bit per-window MSM windows: what the setters and the combine take, and the shape of the
bucket reduction, whose k_set_finish must keep its node array in the 160 KiB of LDS of a CU at every width."""
import ctypes
import os
import subprocess

import numpy as np

from mira_amd import _lib
from mira_amd import commitment as cm
from oracle import cref as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_width_setters(emu_lib):
    from mira_amd._lib import MIRA_E_BAD_ARG
    key = cm.CommitmentKey(0, C.synth_bases(0, 8), lib=emu_lib)
    for c in (17, 18, 19, 20, 0, 16, 4):
        key.set_window_bits(c)
    assert emu_lib.c.mira_msm_set_handle_window_bits(key.handle, 21) == MIRA_E_BAD_ARG
    assert emu_lib.c.mira_msm_set_handle_window_bits(key.handle, 3) == MIRA_E_BAD_ARG
    assert emu_lib.c.mira_msm_set_window_bits(17) == MIRA_E_BAD_ARG            # the process-wide default stays 4..16
    for cmax in (20, 17, 16):
        key.set_max_window_bits(cmax)
    for bad in (15, 21, 0):
        assert emu_lib.c.mira_msm_set_handle_max_window_bits(key.handle, bad) == MIRA_E_BAD_ARG
    assert emu_lib.c.mira_msm_set_handle_max_window_bits(987654321, 20) == MIRA_E_BAD_ARG
    c = ctypes.c_int32()
    emu_lib.check(emu_lib.c.mira_msm_plan_window_bits(1 << 26, ctypes.byref(c)))
    assert 4 <= c.value <= 16                                                  # the key-less default never goes wide
    # a partial of a rank that asked for 21 bits is refused
    d = emu_lib.alloc(32)
    out = np.zeros(_lib.MIRA_PARTIAL_U64, dtype=np.uint64)
    wb, nw = ctypes.c_int32(21), ctypes.c_int32()
    assert emu_lib.c.mira_msm_partial_device(key.handle, 0, ctypes.c_void_p(d), 1, out.ctypes.data_as(ctypes.c_void_p),
                                             ctypes.byref(wb), ctypes.byref(nw)) == MIRA_E_BAD_ARG
    emu_lib.free(d); key.close()


def test_combine_takes_20_bit_partials(emu_lib):
    """combine_partials at c = 20: 13 windows, here the identity in all but window 1, which holds a point P -- the result is
    2^20 P."""
    cid = 0
    bs = C.synth_bases(cid, 1)
    key = cm.CommitmentKey(cid, bs, lib=emu_lib)
    d = emu_lib.alloc(32)
    two20 = np.zeros((1, 4), dtype=np.uint64)
    two20[0, 0] = 1 << 20
    emu_lib.upload(d, C.to_mont(C.FIELD_FR, two20))
    one = np.zeros((1, 4), dtype=np.uint64)
    one[0, 0] = 1
    part0, c0, w0 = key.commit_partial_device(0, d, 1, window_bits=4)          # 2^20 P as a 4-bit partial: the oracle's point
    want = cm.combine_partials(cid, part0[None, :], c0, w0, lib=emu_lib)
    emu_lib.upload(d, C.to_mont(C.FIELD_FR, one))
    p1, c1, w1 = key.commit_partial_device(0, d, 1, window_bits=4)            # P in window 0 of a 4-bit partial
    moved = np.zeros_like(p1)
    moved[16:32] = p1[0:16]                                                   # ... moved to window 1 of a 20-bit one
    assert (cm.combine_partials(cid, moved[None, :], 20, 13, lib=emu_lib) == want).all()
    assert (want == C.commit(cid, bs, C.to_mont(C.FIELD_FR, two20))).all()
    with __import__("pytest").raises(_lib.MiraError):
        cm.combine_partials(cid, moved[None, :], 21, 13, lib=emu_lib)
    emu_lib.free(d); key.close()


def test_reduction_lds_fits_a_cu(tmp_path):
    exe = str(tmp_path / "wide_reduction")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-DMIRA_CPU_EMU", "-pthread", "-x", "c++",
                           os.path.join(ROOT, "tests", "emu", "test_wide_reduction.cpp"), os.path.join(ROOT, "mira_amd", "csrc", "msm_plan.hip"),
                           "-o", exe])
    rows = [dict(kv.split("=") for kv in line.split()) for line in subprocess.check_output([exe], text=True).splitlines()]
    widths = {int(r["c"]) for r in rows}
    assert set(range(17, 21)) <= widths
    for r in rows:
        assert int(r["set_finish"]) <= 160 * 1024, r
        assert int(r["bucket_tree"]) <= 160 * 1024, r
    wide = [r for r in rows if int(r["c"]) >= 17]
    assert {r["count"] for r in wide} >= {"1", "2"}                            # batches of wide commits too
    assert all(int(r["gamma"]) <= 6 for r in wide)


def test_batch_launches_fit_one_scan(tmp_path):
    """A batch over a key that opted into wide windows: the plan of each launch is made for its own count of commitments, whose
    model (the commit of n x count pairs) favours wider windows than the single commitment's plan that sized the launch.  No
    launch may hold more bucket counters than one scan takes (3 x 2^23 pairs once planned 20 bits: 20.4 M counters, refused)."""
    exe = str(tmp_path / "wide_batch_plan")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-DMIRA_CPU_EMU", "-pthread", "-x", "c++",
                           os.path.join(ROOT, "tests", "emu", "test_wide_batch_plan.cpp"), os.path.join(ROOT, "mira_amd", "csrc", "msm_plan.hip"),
                           "-o", exe])
    rows = [dict(kv.split("=") for kv in line.split()) for line in subprocess.check_output([exe], text=True).splitlines()]
    assert len(rows) > 1000
    for r in rows:
        assert int(r["counters"]) <= 1 << 24, r
        assert int(r["c"]) <= int(r["cmax"]), r
        if r["glv"] == "1":
            assert int(r["c"]) <= 16, r
    # the opt-in still reaches wide widths in batches where they fit
    assert any(int(r["c"]) >= 17 and int(r["count"]) > 1 for r in rows if r["cmax"] == "20")
    # keys that did not opt in keep their widths
    assert all(int(r["c"]) <= 16 for r in rows if r["cmax"] == "16")
