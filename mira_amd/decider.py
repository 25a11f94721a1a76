"""Bindings of the deciders on device-resident vectors: what `IVC::verify`
(src/ivc/incrementally_verifiable_computation.rs:617-680) asks of the witness vectors a fold step left in HBM, without
copying them to the host.

* `count_ne_device`, `sum_sub_device`, `PermutationMatrix`: the C ABI of include/mira_gpu.h (`mira_count_ne_device`,
  `mira_sum_sub_device`, `mira_perm_compile` / `mira_perm_check_device` / `mira_perm_free`); the row sweep itself is
  `GraphEvaluator.check_device` (`mira_graph_check_compiled`);
* `is_sat_device`, `is_sat_relaxed_device`, `is_sat_perm_device`, `is_sat_log_derivative_device`: the checks of
  `PlonkStructure::is_sat`, `is_sat_relaxed`, `is_sat_perm` and `is_sat_log_derivative` (src/plonk/mod.rs:434-622) in the
  reference's order, raising the reference's errors (`Error`, src/plonk/mod.rs) at the first failing CHECK with the counts
  the reference reports.

Vectors are 32-byte Montgomery elements on the device; challenges and matrix values are plain Python integers below the
modulus; commitments are (8,) uint64 affine points as `CommitmentKey.commit_device` returns them."""
import ctypes

import numpy as np

from . import _lib
from .graph_evaluator import to_montgomery

FIELD_FQ, FIELD_FR = 0, 1
NONE = (1 << 64) - 1                       # `first` when nothing differs


# ---------------------------------------------------------------- the reference's errors (src/plonk/mod.rs `Error`)
class DeciderError(Exception):
    pass


class EvaluationMismatch(DeciderError):
    """Error::EvaluationMismatch { mismatch_count, total_row }; first_row: the lowest row that differs (the reference warn!s every one)"""

    def __init__(self, mismatch_count, total_row, first_row):
        super().__init__(f"evaluation mismatch: {mismatch_count} of {total_row} rows, first at row {first_row}")
        self.mismatch_count, self.total_row, self.first_row = mismatch_count, total_row, first_row


class LogDerivativeNotSat(DeciderError):
    """Error::LogDerivativeNotSat"""


class CommitmentMismatch(DeciderError):
    """Error::CommitmentMismatch { mismatch_count }"""

    def __init__(self, mismatch_count):
        super().__init__(f"commitment of witness mismatch: {mismatch_count}")
        self.mismatch_count = mismatch_count


class ECommitmentMismatch(DeciderError):
    """Error::ECommitmentMismatch"""


class PermCheckFail(DeciderError):
    """Error::PermCheckFail { mismatch_count }; first: the lowest index of Z with y_i != Z_i"""

    def __init__(self, mismatch_count, first=None):
        super().__init__(f"permutation check fail: {mismatch_count}")
        self.mismatch_count, self.first = mismatch_count, first


# ---------------------------------------------------------------- thin wrappers
def count_ne_device(field, d_a, d_b, n, lib=None):
    """-> (count of i < n with a[i] != b[i], smallest such i or NONE); d_b None: a[i] != 0."""
    lib = lib or _lib.load()
    count, first = ctypes.c_uint64(), ctypes.c_uint64()
    lib.check(lib.c.mira_count_ne_device(field, ctypes.c_void_p(d_a), ctypes.c_void_p(d_b), n, ctypes.byref(count), ctypes.byref(first)))
    return count.value, first.value


def sum_sub_device(field, d_a, d_b, n, lib=None):
    """-> sum a[i] - sum b[i] (d_b None: sum a[i]) as (4,) uint64 limbs, canonical Montgomery: all zero iff the sums agree."""
    lib = lib or _lib.load()
    out = np.empty(4, dtype=np.uint64)
    lib.check(lib.c.mira_sum_sub_device(field, ctypes.c_void_p(d_a), ctypes.c_void_p(d_b), n, out.ctypes.data_as(ctypes.c_void_p)))
    return out


def _elements(values, field):
    """ints below the modulus, or (n, 4) uint64 Montgomery limbs as they are"""
    if isinstance(values, np.ndarray) and values.dtype == np.uint64:
        return np.ascontiguousarray(values).reshape(-1, 4)
    return to_montgomery(list(values), field)


class PermutationMatrix:
    """A SparseMatrix of the reference (src/polynomial/sparse.rs: triples (row, col, value) of an n x n matrix) compiled
    for the device once per circuit -- PlonkStructure::permutation_matrix is fixed.  triples: (row, col) pairs, value ONE
    (what construct_permutation_matrix emits, src/plonk/util.rs:128-174), or (row, col, value) with integer values.
    Triples in any order; duplicates of (row, col) add."""

    def __init__(self, field, triples, n, lib=None):
        self.lib = lib or _lib.load()
        self.field, self.n = field, n
        triples = [tuple(t) for t in triples]
        rows = np.array([t[0] for t in triples], dtype=np.uint64)
        cols = np.array([t[1] for t in triples], dtype=np.uint64)
        values = None
        if any(len(t) > 2 and t[2] is not None for t in triples):
            values = to_montgomery([1 if len(t) < 3 or t[2] is None else t[2] for t in triples], field)
        h = ctypes.c_uint64()
        self.lib.check(self.lib.c.mira_perm_compile(field, rows.ctypes.data_as(ctypes.c_void_p), cols.ctypes.data_as(ctypes.c_void_p),
                                                    None if values is None else values.ctypes.data_as(ctypes.c_void_p), len(triples), n, ctypes.byref(h)))
        self.handle = h.value

    def check_device(self, instance, d_w, n_w):
        """y = P Z with Z = instance (host: ints or (num_io, 4) Montgomery limbs) || the n_w device elements at d_w
        -> (count of y_i != Z_i, smallest such i or NONE)"""
        inst = _elements(instance, self.field)
        count, first = ctypes.c_uint64(), ctypes.c_uint64()
        self.lib.check(self.lib.c.mira_perm_check_device(self.handle, inst.ctypes.data_as(ctypes.c_void_p) if len(inst) else None, len(inst),
                                                         ctypes.c_void_p(d_w), n_w, ctypes.byref(count), ctypes.byref(first)))
        return count.value, first.value

    def close(self):
        h, self.handle = getattr(self, "handle", None), None
        if h is not None:
            self.lib.c.mira_perm_free(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---------------------------------------------------------------- deciders
def is_sat_log_derivative_device(field, d_W, rows, num_lookups, has_vector_lookup, lib=None):
    """is_sat_log_derivative (src/plonk/mod.rs:592-622): sum_i h_i == sum_i g_i for every lookup.  d_W: the device pointers
    of the witness vectors; (h, g) live in W[2] with a vector lookup, else in W[1], h of lookup j at vector 2 j and g at
    2 j + 1 of `rows` elements each."""
    if has_vector_lookup:
        w = d_W[2]
    elif num_lookups > 0:
        w = d_W[1]
    else:
        return True
    step = rows * 32
    return all(not sum_sub_device(field, w + 2 * j * step, w + (2 * j + 1) * step, rows, lib=lib).any() for j in range(num_lookups))


def _check_common(key, evaluator, columns, challenges, rows, d_W, W_lens, W_commitments, d_expected, lookup, lib):
    count, first = evaluator.check_device(columns, challenges, rows, d_expected=d_expected, lib=lib)
    if count:
        raise EvaluationMismatch(count, rows, first)
    num_lookups, has_vector_lookup = lookup or (0, False)
    if not is_sat_log_derivative_device(evaluator.field, d_W, rows, num_lookups, has_vector_lookup, lib=lib):
        raise LogDerivativeNotSat()
    if not len(d_W) == len(W_lens) == len(W_commitments):
        raise ValueError("one length and one commitment per witness vector")       # zip_eq
    bad = sum(1 for d, n, c in zip(d_W, W_lens, W_commitments) if (key.commit_device(d, n) != np.asarray(c, dtype=np.uint64)).any())
    if bad:
        raise CommitmentMismatch(bad)


def is_sat_device(key, evaluator, columns, challenges, rows, d_W, W_lens, W_commitments, lookup=None, lib=None):
    """PlonkStructure::is_sat (src/plonk/mod.rs:434-493) after its first line: `U.sps_verify(ro_nark)` re-derives the
    challenges with Poseidon on the host and stays the caller's.

    evaluator: the GraphEvaluator of the compressed gate polynomial; columns: its column table over the witness on the
    device (PlonkEvalDomain(..., W1s = W, W2s = []).columns()); challenges: U.challenges; d_W / W_lens / W_commitments:
    device pointer, length in elements and commitment of every witness vector; lookup: (num_lookups, has_vector_lookup)
    or None for a circuit without lookups.  Raises EvaluationMismatch, LogDerivativeNotSat or CommitmentMismatch, in that
    order; returns None when the pair is satisfied."""
    _check_common(key, evaluator, columns, challenges, rows, d_W, W_lens, W_commitments, None, lookup, lib)


def is_sat_relaxed_device(key, evaluator, columns, challenges, rows, d_W, W_lens, W_commitments, d_E, E_commitment, lookup=None, lib=None):
    """PlonkStructure::is_sat_relaxed (src/plonk/mod.rs:495-560).  evaluator: the GraphEvaluator of the HOMOGENEOUS gate
    polynomial; challenges: U.challenges followed by U.u; d_E: the error vector on the device (`rows` elements).  Raises
    EvaluationMismatch, LogDerivativeNotSat, CommitmentMismatch or ECommitmentMismatch, in that order."""
    _check_common(key, evaluator, columns, challenges, rows, d_W, W_lens, W_commitments, d_E, lookup, lib)
    if (key.commit_device(d_E, rows) != np.asarray(E_commitment, dtype=np.uint64)).any():
        raise ECommitmentMismatch()


def is_sat_perm_device(perm, instance, d_W0, rows, num_advice):
    """PlonkStructure::is_sat_perm (src/plonk/mod.rs:563-589): Z = U.instance || W.W[0][..rows * num_advice]; raises
    PermCheckFail with the number of indices where P Z differs from Z."""
    count, first = perm.check_device(instance, d_W0, rows * num_advice)
    if count:
        raise PermCheckFail(count, first)
