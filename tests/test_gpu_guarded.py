"""-m gpu: guard bands (tests/guarded.py) around every device-resident call of the GPU build.  Every operand of a call lies
inside one allocation between 64 KiB bands of unique, non-canonical guard elements, at byte offsets 0, 32 and 96 from a
256-byte boundary; every call must give exact values (Python integers, the C oracle), leave both bands of every operand
untouched and leave its inputs alone.  On the device a tail lane that stores one element past n lands in allocator slack and
faults nothing: these are the runs that would show it.

The device-resident transforms (mira_fft_bn256_fr_device, mira_ifft_bn256_fr_device, mira_ntt_bn256_fr_device -- what bench.py
times and a resident fold step calls) work in place on the caller's buffer, where the host entry points transform the library's
own larger staging buffer: every log_n from 0 to 20 on the default policy (7, 14 and 19 run nowhere else), 2^22 through an uneven
grid of 37 workgroups, the forced schedules, primitive roots other than the standard one, and one fold, one fft_device of
2^13 points and one commit of 1025 pairs on a stream of the caller's (mira_set_stream)."""
import ctypes

import pytest

import edge_operands as E
import guarded as GD

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("field", E.FIELDS)
def test_fold(gpu_lib, field):
    GD.check_fold(gpu_lib, field)


@pytest.mark.parametrize("field", E.FIELDS)
def test_lincomb(gpu_lib, field):
    GD.check_lincomb(gpu_lib, field)


@pytest.mark.parametrize("field", E.FIELDS)
def test_batch_invert(gpu_lib, field):
    GD.check_batch_invert(gpu_lib, field)


@pytest.mark.parametrize("field", E.FIELDS)
def test_lookup(gpu_lib, field):
    GD.check_lookup(gpu_lib, field)


@pytest.mark.parametrize("field", E.FIELDS)
def test_deciders(gpu_lib, field):
    GD.check_deciders(gpu_lib, field)


@pytest.mark.parametrize("field", E.FIELDS)
def test_pow_tree(gpu_lib, field):
    GD.check_pow_tree(gpu_lib, field)


@pytest.mark.parametrize("field", E.FIELDS)
def test_graph(gpu_lib, field):
    GD.check_graph(gpu_lib, field)


@pytest.mark.parametrize("curve", [0, 1])
def test_generators(gpu_lib, curve):
    GD.check_generators(gpu_lib, curve)


@pytest.mark.parametrize("curve", [0, 1])
def test_msm_io(gpu_lib, curve):
    GD.check_msm_io(gpu_lib, curve)


def test_copy(gpu_lib):
    GD.check_copy(gpu_lib)


# ---- the device-resident transforms ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(21))
def test_ntt_device(gpu_lib, k):
    GD.check_ntt_device(gpu_lib, k)


def test_ntt_device_uneven_grid(gpu_lib):
    """2^22 points through 37 workgroups: the block-groups come from the per-XCD counters, with uneven homes"""
    GD.check_ntt_device(gpu_lib, 22, grid=37)


@pytest.mark.parametrize("wave", [0, 1])
@pytest.mark.parametrize("k", [13, 16])
def test_ntt_device_forced_kernel(gpu_lib, k, wave):
    GD.check_ntt_device(gpu_lib, k, wave=wave)


@pytest.mark.parametrize("k,max_log_line", [(16, 6), (12, 12)], ids=["three passes, the last in place", "the 128 KiB line"])
def test_ntt_device_forced_lines(gpu_lib, k, max_log_line):
    GD.check_ntt_device(gpu_lib, k, max_log_line=max_log_line)


@pytest.mark.parametrize("k", [5, 11, 14, 20])
def test_ntt_other_primitive_roots(gpu_lib, k):
    GD.check_ntt_roots(gpu_lib, k)


# ---- the caller's stream --------------------------------------------------------------------------------------------------------
def test_set_stream(gpu_lib):
    """mira_set_stream with a stream of torch's -- the integration path include/mira_gpu.h documents -- then back to the
    library's own stream, whatever happened in between: the library is shared by the whole session"""
    import torch
    lib = gpu_lib
    stream = torch.cuda.Stream()
    lib.check(lib.c.mira_set_stream(ctypes.c_void_p(stream.cuda_stream)))
    try:
        GD.check_fold(lib, E.FIELD_FR, lengths=(1025,), offsets=(1,))
        GD.check_ntt_device(lib, 13, ops=("fft_device",), offsets=(3,))
        GD.check_commit_device(lib, 0, 1025)
    finally:
        lib.check(lib.c.mira_set_stream(None))
    GD.check_fold(lib, E.FIELD_FR, lengths=(1025,), offsets=(1,))
    del stream
