"""Per-window MSM windows of 17 to 20 bits (csrc/msm_host.cuh: the two-level front), on the test-only host emulation of the
kernel sources (tests/emu/emu.h).  2^16 .. 2^19 emulated buckets per window are slow, so MIRA_TUNE_WIDE_FRONT_MIN_C drives
narrow widths through the same kernels: int32 digits, the per-window coarse histogram and its scan, level 1 by coarse bin,
the bucket counts from the level-1 output, their scan with the {L, T} plan, the heavy counters and the identity markers, and
level 2 by bucket.  A real c = 17 commit runs here too (on a short vector).  The GPU suite (test_gpu_wide_windows.py) covers
17 .. 20 bits at full size."""
import ctypes

import numpy as np
import pytest

from mira_amd import _lib
from mira_amd import commitment as cm
from oracle import cref as C


@pytest.fixture
def tune(emu_lib):
    used = []

    def set_knob(knob, value):
        used.append(knob)
        emu_lib.tune(knob, value)
    yield set_knob
    for knob in used:
        emu_lib.tune(knob, -1)


def _field(cid):
    return C.FIELD_FR if cid == 0 else C.FIELD_FQ


def _mont(cid, ints):
    """little-endian 64-bit limbs of small integers -> Montgomery form of the curve's scalar field"""
    a = np.zeros((len(ints), 4), dtype=np.uint64)
    a[:, 0] = np.asarray(ints, dtype=np.uint64)
    return C.to_mont(_field(cid), a)


def _vectors(cid, n, seed):
    """dense, witness-like (zeros and 32-bit values), all ones, repeated scalars"""
    rng = np.random.default_rng(seed)
    dense = C.synth_scalars(cid, n, seed=seed)
    wit = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    wit[rng.random(n) < 0.6] = 0
    rep = C.synth_scalars(cid, n, seed=seed + 1)
    rep[n // 4: 3 * n // 4] = rep[0]
    return {"dense": dense, "witness": _mont(cid, wit), "ones": _mont(cid, np.ones(n, dtype=np.uint64)), "repeated": rep}


def _last_plan(lib):
    c, w = ctypes.c_int32(), ctypes.c_int32()
    lib.check(lib.c.mira_msm_last_plan(ctypes.byref(c), ctypes.byref(w)))
    return c.value, w.value


@pytest.mark.parametrize("cid", [0, 1])
def test_wide_front_drives_narrow_widths(emu_lib, tune, cid):
    """Widths 6, 9 and 12 through the two-level front: every kind of vector gives the oracle's point, and the commit ran through
    the front's stages (not k_hist / k_scatter)."""
    n = 333
    bs = C.synth_bases(cid, n, seed=200 + cid)
    bs[17] = 0                                                   # an identity base
    key = cm.CommitmentKey(cid, bs, lib=emu_lib)
    tune(_lib.TUNE_WIDE_FRONT_MIN_C, 5)
    vecs = _vectors(cid, n, 210 + cid)
    for c in (6, 9, 12):
        key.set_window_bits(c)
        for name, sc in vecs.items():
            assert (key.commit(sc) == C.msm_pippenger(cid, sc, bs)).all(), (c, name)
        assert _last_plan(emu_lib) == (c, -(-256 // c))
        emu_lib.check(emu_lib.c.mira_set_timing(1))
        assert (key.commit(vecs["dense"]) == C.msm_pippenger(cid, vecs["dense"], bs)).all()
        names = [name for name, _ in emu_lib.timings()]
        emu_lib.check(emu_lib.c.mira_set_timing(0))
        assert "bucket_count" in names and "sort_level2" in names and "scatter" not in names, names
    key.set_window_bits(0)
    key.close()


def test_wide_front_in_point_chunks(emu_lib, tune):
    """The front inside the point-chunk loop: a commit cut by MIRA_TUNE_PASS_ENTRIES_LOG (scalars in device memory, a prefix,
    a batch), host scalars in copy chunks, a host batch -- every later chunk adds into the buckets of the ones before."""
    cid, n = 0, 420
    bs = C.synth_bases(cid, n, seed=220)
    bs[300] = 0
    key = cm.CommitmentKey(cid, bs, lib=emu_lib)
    vecs = _vectors(cid, n, 221)
    vs = [vecs["dense"], vecs["witness"]]
    want = [C.commit(cid, bs, v) for v in vs]
    d = emu_lib.alloc(2 * n * 32)
    for b, v in enumerate(vs):
        emu_lib.upload(d + b * n * 32, v)
    tune(_lib.TUNE_WIDE_FRONT_MIN_C, 5)
    key.set_window_bits(9)
    tune(_lib.TUNE_PASS_ENTRIES_LOG, 13)                        # 8191 entries per pass: chunks of 256 points under 29 windows
    assert (key.commit_device(d, n) == want[0]).all()
    assert (key.commit_device(d + n * 32, 333) == C.commit(cid, bs[:333], vs[1][:333])).all()
    assert (key.commit_batch_device(d, n, 2) == np.stack(want)).all()
    tune(_lib.TUNE_PASS_ENTRIES_LOG, -1)
    tune(_lib.TUNE_HOST_CHUNK_MIN_N, 64)                         # host scalars: copy chunks of 32, 64, 128 ... points
    assert (key.commit(vs[0]) == want[0]).all()
    assert (key.commit(vs[1]) == want[1]).all()
    assert (key.commit_batch(vs) == np.stack(want)).all()
    key.set_window_bits(0)
    emu_lib.free(d); key.close()


@pytest.mark.parametrize("cid", [0, 1])
def test_wide_front_partial_and_combine(emu_lib, tune, cid):
    """A rank's partial through the front (the public format: one point per window), and combine_partials over two chunks."""
    n = 300
    bs, sc = C.synth_bases(cid, n, seed=230 + cid), C.synth_scalars(cid, n, seed=232 + cid)
    key = cm.CommitmentKey(cid, bs, lib=emu_lib)
    d = emu_lib.alloc(n * 32)
    emu_lib.upload(d, sc)
    tune(_lib.TUNE_WIDE_FRONT_MIN_C, 5)
    p0, c0, w0 = key.commit_partial_device(0, d, 120, window_bits=7)
    p1, c1, w1 = key.commit_partial_device(120, d + 120 * 32, n - 120, window_bits=7)
    assert (c0, w0) == (c1, w1) == (7, 37)
    assert (cm.combine_partials(cid, np.stack([p0, p1]), c0, w0, lib=emu_lib) == C.commit(cid, bs, sc)).all()
    emu_lib.free(d); key.close()


def test_real_17_bit_commit(emu_lib):
    """One commit at c = 17 proper (int32 digits beyond the int16 range, 16 windows of 2^16 buckets, chunks of 8 buckets in
    the reduction) on a short vector, and its partial."""
    cid, n = 1, 48
    bs = C.synth_bases(cid, n, seed=240)
    sc = C.synth_scalars(cid, n, seed=241)
    sc[5] = sc[6]
    key = cm.CommitmentKey(cid, bs, lib=emu_lib)
    key.set_window_bits(17)
    assert (key.commit(sc) == C.commit(cid, bs, sc)).all()
    assert _last_plan(emu_lib) == (17, 16)
    d = emu_lib.alloc(n * 32)
    emu_lib.upload(d, sc)
    part, c, w = key.commit_partial_device(0, d, n, window_bits=17)
    assert (c, w) == (17, 16)
    assert (cm.combine_partials(cid, part[None, :], c, w, lib=emu_lib) == C.commit(cid, bs, sc)).all()
    emu_lib.free(d); key.close()
