"""Bindings of the lookup argument's witness rounds (src/plonk/lookup.rs:213-366) on device-resident vectors:

* `batch_invert_device`, `evaluate_m_device`, `evaluate_h_g_device`: the C ABI of include/mira_gpu.h
  (`mira_batch_invert_device`, `mira_lookup_m_device`, `mira_lookup_h_g_device`);
* `LookupEvalDomain`: the column index space of the reference's `LookupEvalDomain` (src/plonk/eval.rs:84-133) --
  selectors, fixed columns, then the advice columns of the witness -- resolved to device pointers;
* `LookupArguments`: `evaluate_coefficient_1` (ls | ts | ms, lookup.rs:323-346) and `evaluate_coefficient_2` (hs | gs,
  :357-366) with every L_i / T_i a compiled `GraphEvaluator`, written straight into a witness vector in HBM.

Vectors are 32-byte Montgomery elements on the device; challenges are plain Python integers below the modulus."""
import ctypes

import numpy as np

from . import _lib
from .graph_evaluator import COL_BOOL, COL_FIELD, MODULUS, to_montgomery

FIELD_FQ, FIELD_FR = 0, 1


def batch_invert_device(field, d_out, d_in, n, lib=None):
    """out[i] = in[i]^-1, 0 -> 0, over n device elements; d_out == d_in inverts in place."""
    lib = lib or _lib.load()
    lib.check(lib.c.mira_batch_invert_device(field, ctypes.c_void_p(d_out), ctypes.c_void_p(d_in), n))


def evaluate_m_device(field, d_m, d_l, n_l, d_t, n_t, lib=None):
    """evaluate_m (lookup.rs:278-307): m[i] = how many l equal t[i], at t[i]'s first occurrence in t, else 0."""
    lib = lib or _lib.load()
    lib.check(lib.c.mira_lookup_m_device(field, ctypes.c_void_p(d_m), ctypes.c_void_p(d_l), n_l, ctypes.c_void_p(d_t), n_t))


def evaluate_h_g_device(field, d_h, d_g, d_l, n_l, d_t, d_m, n_t, r, lib=None):
    """evaluate_h_g (lookup.rs:309-321): h = 1 / (l + r) over n_l, g = m / (t + r) over n_t, 0 where a denominator is 0."""
    lib = lib or _lib.load()
    if not 0 <= r < MODULUS[field]:
        raise ValueError("r must be a canonical field element")
    rm = to_montgomery([r], field)
    lib.check(lib.c.mira_lookup_h_g_device(field, ctypes.c_void_p(d_h), ctypes.c_void_p(d_g), ctypes.c_void_p(d_l), n_l,
                                           ctypes.c_void_p(d_t), ctypes.c_void_p(d_m), n_t, rm.ctypes.data_as(ctypes.c_void_p)))


class LookupEvalDomain:
    """selectors: device byte columns; fixed, advice: device field columns (num_rows elements each).  `columns()` is the
    column table of `GraphEvaluator.evaluate_device` in the index space eval_column_var resolves L_i and T_i in."""

    def __init__(self, selectors, fixed, advice):
        self.selectors, self.fixed, self.advice = list(selectors), list(fixed), list(advice)

    def columns(self):
        return [(p, COL_BOOL) for p in self.selectors] + [(p, COL_FIELD) for p in self.fixed + self.advice]


class LookupArguments:
    """The device side of `Arguments` (lookup.rs): one compiled GraphEvaluator per lookup polynomial L_i and per table
    polynomial T_i (as many of each: evaluate_coefficient_1 zips them)."""

    def __init__(self, field, lookup_evaluators, table_evaluators):
        if len(lookup_evaluators) != len(table_evaluators):
            raise ValueError("one table polynomial per lookup polynomial")
        self.field = field
        self.lookup_evaluators, self.table_evaluators = list(lookup_evaluators), list(table_evaluators)

    @property
    def num_lookups(self):
        return len(self.lookup_evaluators)

    def evaluate_coefficient_1_device(self, domain, r, num_rows, d_dst, lib=None):
        """evaluate_coefficient_1 (lookup.rs:323-346) into d_dst: ls | ts | ms, num_rows elements each (3 * num_lookups
        vectors; concat_vec! order) -- W2 of run_sps_protocol_3, the tail of W1 after the advice in run_sps_protocol_2."""
        lib = lib or _lib.load()
        n, cols, step = self.num_lookups, domain.columns(), num_rows * 32
        for i, ev in enumerate(self.lookup_evaluators + self.table_evaluators):
            ev.evaluate_device(cols, [r], num_rows, d_out=d_dst + i * step, lib=lib)
        for i in range(n):
            evaluate_m_device(self.field, d_dst + (2 * n + i) * step, d_dst + i * step, num_rows, d_dst + (n + i) * step, num_rows, lib=lib)

    def evaluate_coefficient_2_device(self, d_ltm, r, num_rows, d_dst, lib=None):
        """evaluate_coefficient_2 (lookup.rs:357-366): from ls | ts | ms at d_ltm, hs | gs into d_dst (2 * num_lookups
        vectors) -- W3 of run_sps_protocol_3, W2 of run_sps_protocol_2."""
        lib = lib or _lib.load()
        n, step = self.num_lookups, num_rows * 32
        for i in range(n):
            evaluate_h_g_device(self.field, d_dst + i * step, d_dst + (n + i) * step, d_ltm + i * step, num_rows,
                                d_ltm + (n + i) * step, d_ltm + (2 * n + i) * step, num_rows, r, lib=lib)
