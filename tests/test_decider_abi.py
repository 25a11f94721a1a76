"""The decider entry points of the product library without a device: no CPU fallback, every one of them reports NO_DEVICE."""
import ctypes

import numpy as np
import pytest


def test_deciders_fail_loudly_without_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from mira_amd import _lib
    from mira_amd import decider as D
    from mira_amd.graph_evaluator import GraphEvaluator
    lib = _lib.load()
    buf = np.zeros((4, 4), dtype=np.uint64)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    out, first, h = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    idx = np.zeros(1, dtype=np.uint64)
    ip = idx.ctypes.data_as(ctypes.c_void_p)
    calls = [
        lambda: lib.c.mira_count_ne_device(1, p, p, 4, ctypes.byref(out), ctypes.byref(first)),
        lambda: lib.c.mira_count_ne_device(1, None, None, 0, ctypes.byref(out), None),
        lambda: lib.c.mira_sum_sub_device(0, p, None, 4, p),
        lambda: lib.c.mira_graph_check_compiled(1, None, 0, None, 0, 4, None, ctypes.byref(out), ctypes.byref(first)),
        lambda: lib.c.mira_perm_compile(1, ip, ip, None, 1, 1, ctypes.byref(h)),
        lambda: lib.c.mira_perm_check_device(1, p, 1, p, 0, ctypes.byref(out), ctypes.byref(first)),
        lambda: lib.c.mira_perm_free(1),
    ]
    for k, call in enumerate(calls):
        assert call() == _lib.MIRA_E_NO_DEVICE, k
        assert b"no CPU fallback" in lib.c.mira_last_error()
    for call in (lambda: D.count_ne_device(1, 0, None, 0, lib=lib), lambda: D.sum_sub_device(1, 0, None, 0, lib=lib),
                 lambda: D.PermutationMatrix(1, [(0, 0)], 1, lib=lib), lambda: GraphEvaluator(1).check_device([], [], 0, lib=lib)):
        with pytest.raises(_lib.MiraError) as err:
            call()
        assert err.value.code == _lib.MIRA_E_NO_DEVICE
