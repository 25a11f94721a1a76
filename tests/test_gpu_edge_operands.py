"""-m gpu: worst-case field operands (tests/edge_operands.py) through every field-arithmetic kernel of the GPU build, byte for
byte against Python integers (the transforms: against the C oracle, which tests/test_edge_operands_emu.py pins to a
Python-integer NTT on the same patterns).  The GPU build has no bound tracking: these are the runs that would show a limb
bound of field29.cuh, a subtraction bias or a final reduction that holds on the host compiler and not on gfx950.

Shapes are the smallest that reach each code path:
* NTT over Fr -- fft, ifft, the coset transforms and best_fft with the inverse omega at 2^1, 2^2, 2^6 and 2^8 (wave-level full
  lines), 2^9 (the largest default single line), 2^10 and 2^12 (two passes), 2^12 as a single line and in three passes, 2^13,
  2^16, each on the default kernel choice and with either kernel forced, and 2^16 through an uneven grid of 5 workgroups; every
  size also transforms the oracle's ifft of the extreme vector, so that exact 0 and p - 1 leave the final reduction;
* fold_witness over all operand pairs x every r, results of exactly 0 and p - 1, fold_error / fold_relaxed_witness with 16
  terms at lengths 1, 255, 256, 257, 1025, in place and out of place, both fields;
* lincomb (16 vectors) and lincomb_multi (8 outputs), pow_tree_reduce at 2^1, 2^6, 2^11 leaves with shared and per-point leaves;
* the graph evaluator's one-shot, compiled, batched and run-time specialised engines over 2^10 rows, every row against
  pyref.eval_expression;
* batch_invert and lookup h / g with planted zero denominators at the level boundaries of the inversion plan, 2, 8 and 64
  elements per lane."""
import pytest

import edge_operands as E

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("k", [1, 2, 6, 8, 9, 10, 12, 13, 16])
def test_ntt(gpu_lib, k):
    for wave in (-1, 1, 0):
        E.check_ntt(gpu_lib, k, wave=wave, width=1 if k == 16 else 4 if k == 13 else 8)     # single-v patterns around 1, 4 or all 8 chosen v


@pytest.mark.parametrize("max_log_line", [12, 4])
def test_ntt_4096_points_single_line_and_three_passes(gpu_lib, max_log_line):
    for wave in (-1, 1, 0):
        E.check_ntt(gpu_lib, 12, wave=wave, max_log_line=max_log_line, width=2)


def test_ntt_uneven_grid(gpu_lib):
    """5 workgroups share the block-groups (wave-level kernel) or lines (workgroup-level kernel) of 2^16 points through the counters"""
    for wave in (-1, 1, 0):
        E.check_ntt(gpu_lib, 16, wave=wave, grid=5, width=1)
    E.check_ntt(gpu_lib, 16, wave=1, grid=5, max_log_line=6, width=1, ops=("fft", "ifft"))     # three passes of 64-point lines


@pytest.mark.parametrize("field", E.FIELDS)
def test_fold_witness_all_pairs(gpu_lib, field):
    E.check_fold_pairs(gpu_lib, field)


@pytest.mark.parametrize("field", E.FIELDS)
def test_fold_witness_to_exact_zero_and_p_minus_1(gpu_lib, field):
    E.check_fold_targets(gpu_lib, field)


@pytest.mark.parametrize("field", E.FIELDS)
def test_fold_error_and_relaxed_witness_lengths(gpu_lib, field):
    E.check_fold_lengths(gpu_lib, field)


@pytest.mark.parametrize("field", E.FIELDS)
def test_lincomb_and_lincomb_multi(gpu_lib, field):
    E.check_lincomb(gpu_lib, field)


@pytest.mark.parametrize("field", E.FIELDS)
def test_pow_tree_reduce(gpu_lib, field):
    E.check_pow_tree(gpu_lib, field, sizes=(1, 6, 11, 12))                  # 2^12 leaves: a second kernel round


@pytest.mark.parametrize("chunk", [None, 2, 64])
@pytest.mark.parametrize("field", E.FIELDS)
def test_batch_invert(gpu_lib, field, chunk):
    E.check_batch_invert(gpu_lib, field, chunk)


@pytest.mark.parametrize("chunk", [None, 2, 64])
@pytest.mark.parametrize("field", E.FIELDS)
def test_lookup_h_g(gpu_lib, field, chunk):
    E.check_lookup_h_g(gpu_lib, field, chunk)


@pytest.mark.parametrize("group", ["gate", "chain"])
@pytest.mark.parametrize("field", E.FIELDS)
def test_graph_engines(gpu_lib, field, group):
    """the one-shot interpreter, the compiled engine and its batch"""
    E.check_graph(gpu_lib, field, group)


@pytest.mark.parametrize("group,only", [("gate", [0, 1]), ("chain", None)], ids=["gate", "chain"])
@pytest.mark.parametrize("field", E.FIELDS)
def test_graph_specialised(gpu_lib, field, group, only):
    """Kernels of their own (mira_graph_specialize).  Of the gate-like graphs the 1-term and the 5-term one (72 and 97
    calculations): a specialised kernel is one straight-line statement per calculation, so the 24-term graph (510) would add
    ten seconds of run-time compilation per field and no operation, operand source or rotation that these do not have; it runs
    through the other engines above."""
    E.check_graph(gpu_lib, field, group, specialise=True, only=only)
