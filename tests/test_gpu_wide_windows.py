"""GPU parity tests of the 17- to 20-bit per-window MSM windows (csrc/msm_host.cuh: the two-level front; CommitmentKey::commit,
reference src/commitment.rs:78-87): bit-exact against the C oracle and against the 16-bit path, on plain keys (no endomorphism
copy: wide windows are a plain-path feature)."""
import ctypes

import numpy as np
import pytest

from mira_amd import _lib
from mira_amd import commitment as cm
from oracle import cref as C

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def plain_keys(gpu_lib):
    gpu_lib.tune(_lib.TUNE_GLV_AUTO_MAX_LOG, 0)
    yield
    gpu_lib.tune(_lib.TUNE_GLV_AUTO_MAX_LOG, -1)


def _last_plan(lib):
    c, w = ctypes.c_int32(), ctypes.c_int32()
    lib.check(lib.c.mira_msm_last_plan(ctypes.byref(c), ctypes.byref(w)))
    return c.value, w.value


@pytest.mark.parametrize("cid", [0, 1])
def test_wide_widths_match_oracle(gpu_lib, cid):
    """c = 17 .. 20 at 2^20 pairs: dense and witness-like scalars, in device and in host memory (point chunks), against the oracle."""
    n = 1 << 20
    key = cm.CommitmentKey.synthetic(cid, n, seed=301 + cid)
    bases = key.bases()
    vecs = [C.synth_scalars(cid, n, seed=310 + cid, kind=0), C.synth_scalars(cid, n, seed=312 + cid, kind=1)]
    want = [C.commit(cid, bases, v) for v in vecs]
    d = gpu_lib.alloc(n * 32)
    for c in (17, 18, 19, 20):
        key.set_window_bits(c)
        for v, w in zip(vecs, want):
            gpu_lib.upload(d, v)
            assert (key.commit_device(d, n) == w).all(), c
            assert _last_plan(gpu_lib) == (c, -(-256 // c))
            assert (key.commit(v) == w).all(), c                                     # host scalars
    key.set_window_bits(0)
    gpu_lib.free(d); key.close()


def test_wide_widths_agree_at_2p26(gpu_lib):
    """At 2^26 pairs every width from 16 to 20 gives the same point (2^26 x 13 entries: one pass at c = 20)."""
    cid, n = 0, 1 << 26
    key = cm.CommitmentKey.synthetic(cid, n, seed=320)
    d = cm.synth_scalars_device(cid, n, seed=321)
    key.set_window_bits(16)
    want = key.commit_device(d, n)
    for c in (17, 18, 19, 20):
        key.set_window_bits(c)
        assert (key.commit_device(d, n) == want).all(), c
    key.set_window_bits(0)
    gpu_lib.free(d); key.close()


def test_wide_chunk_partials_combine(gpu_lib):
    """c = 20 partials of three uneven point chunks combine to the whole commitment."""
    cid, n = 1, (1 << 20) + 777
    key = cm.CommitmentKey.synthetic(cid, n, seed=330)
    d = cm.synth_scalars_device(cid, n, seed=331, kind=1)
    want = C.commit(cid, key.bases(), gpu_lib.download(d, (n, 4)))
    cuts = [0, 100_003, 700_000, n]
    parts = []
    for lo, hi in zip(cuts, cuts[1:]):
        p, c, w = key.commit_partial_device(lo, d + lo * 32, hi - lo, window_bits=20)
        assert (c, w) == (20, 13)
        parts.append(p)
    assert (cm.combine_partials(cid, np.stack(parts), 20, 13) == want).all()
    gpu_lib.free(d); key.close()


def test_wide_batch(gpu_lib):
    """A batch of three commitments at c = 18 gives each the point of its own commit."""
    cid, n = 0, (1 << 19) + 3
    key = cm.CommitmentKey.synthetic(cid, n, seed=340)
    d = gpu_lib.alloc(3 * n * 32)
    vs = [C.synth_scalars(cid, n, seed=341 + b, kind=b % 2) for b in range(3)]
    for b, v in enumerate(vs):
        gpu_lib.upload(d + b * n * 32, v)
    key.set_window_bits(18)
    single = np.stack([key.commit_device(d + b * n * 32, n) for b in range(3)])
    assert (key.commit_batch_device(d, n, 3) == single).all()
    assert (key.commit_batch(vs) == single).all()                                       # host vectors
    assert (single[1] == C.commit(cid, key.bases(), vs[1])).all()
    key.set_window_bits(0)
    gpu_lib.free(d); key.close()


@pytest.mark.parametrize("log_n", [24, 26])
def test_opt_in_planner_goes_wide(gpu_lib, log_n):
    """A key with set_max_window_bits(20) gets a width in 17..20 from the planner at 2^24 and 2^26 pairs (the measured table,
    profiles/r05_wide_windows.txt, puts 20 bits 4 and 10 % ahead of 16 there); one without keeps <= 16.  Both commits give the
    same point."""
    cid, n = 0, 1 << log_n
    d = cm.synth_scalars_device(cid, n, seed=350)
    plain = cm.CommitmentKey.synthetic(cid, n, seed=351)
    want = plain.commit_device(d, n)
    assert _last_plan(gpu_lib)[0] <= 16
    plain.close()
    wide = cm.CommitmentKey.synthetic(cid, n, seed=351)
    wide.set_max_window_bits(20)
    assert (wide.commit_device(d, n) == want).all()
    assert 17 <= _last_plan(gpu_lib)[0] <= 20
    wide.close()
    gpu_lib.free(d)


def test_opt_in_planner_batch(gpu_lib):
    """A batch over a key with set_max_window_bits(20): each launch's width is planned for its own count of commitments and
    capped so that its bucket counters fit one scan (3 x 2^23 pairs once planned 20 bits -- 20.4 M counters -- and the launch
    refused the batch).  Same points as the batch over the key without the opt-in, device and host vectors."""
    cid, n = 0, 1 << 23
    key = cm.CommitmentKey.synthetic(cid, n, seed=360)
    d = cm.synth_scalars_device(cid, 3 * n, seed=361, kind=0)
    want = key.commit_batch_device(d, n, 3)
    assert _last_plan(gpu_lib)[0] <= 16
    key.set_max_window_bits(20)
    assert (key.commit_batch_device(d, n, 3) == want).all()
    c, w = _last_plan(gpu_lib)
    assert c <= 20 and 3 * w * (1 << (c - 1)) <= 1 << 24, (c, w)
    assert (key.commit_device(d + n * 32, n) == want[1]).all()
    vs = [gpu_lib.download(d + b * n * 32, (n, 4)) for b in range(3)]
    assert (key.commit_batch(vs) == want).all()                                        # host vectors
    key.close()
    gpu_lib.free(d)
