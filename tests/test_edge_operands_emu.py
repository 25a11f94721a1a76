"""Worst-case field operands (tests/edge_operands.py) through every field-arithmetic kernel on the CPU emulation, whose
F29_TRACK build asserts the limb bounds of field29.cuh on the values actually seen: NTT, the fold and lincomb family, the
ProtoGalaxy tree, the graph engines, the batch inversion and the lookup argument's h / g.  Every result is compared byte for
byte with Python integers (the transforms: with the C oracle, pinned here to a Python-integer NTT on the same patterns).

Each group of cases runs in a child process: an assert of the emulation aborts the process, and the test then reports the
case instead of taking the session down."""
import os
import subprocess
import sys

import pytest

import edge_operands as E
from mira_amd.graph_evaluator import MODULUS
from oracle import cref as C
from oracle import pyref as P

HERE = os.path.dirname(os.path.abspath(__file__))


def run_child(emu_lib, *specs, timeout=600):
    res = subprocess.run([sys.executable, os.path.join(HERE, "edge_operands.py"), emu_lib.path, *specs], capture_output=True, text=True, timeout=timeout)
    done = [line for line in res.stdout.splitlines() if line.startswith("ok ")]
    assert res.returncode == 0 and done == [f"ok {s}" for s in specs], \
        f"exit status {res.returncode} in case {specs[len(done)] if len(done) < len(specs) else '-'}\n{res.stdout[-2000:]}\n{res.stderr[-4000:]}"


def spec(name, **kwargs):
    import json
    return name + (":" + json.dumps(kwargs, sort_keys=True) if kwargs else "")


# ---- the operands themselves ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", E.FIELDS)
def test_the_list(field):
    p, reps = MODULUS[field], E.representations(field)
    assert len(reps) == len(set(reps)) == 36 and all(0 <= r < p for r in reps)
    for must in (0, 1, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, (1 << 253) - 1, 1 << 253, (1 << 232) - 1, 1 << 232, (1 << 224) - 1, (1 << 29) - 1, 1 << 29):
        assert must in reps
    ones = E.all_ones_limbs(field)
    assert ones in reps and all((ones >> (29 * i)) & 0x1FFFFFFF == 0x1FFFFFFF for i in range(8)) and ones >> 232 == (p >> 232) - 1
    for v in (1, p - 1, 2, (p + 1) // 2):                                  # the Montgomery forms of 1, -1, 2 and 1/2
        assert E.from_value(v, field) in reps and E.to_value(E.from_value(v, field), field) == v
    from helpers import ints_to_mont, mont_to_ints                        # the conversions agree with the suite's own
    assert mont_to_ints(E.to_array(reps), p) == [E.to_value(r, field) for r in reps]
    assert (ints_to_mont([E.to_value(r, field) for r in reps], p) == E.to_array(reps)).all()
    assert E.from_array(E.to_array(reps)) == reps


def test_the_patterns():
    field, n = E.FIELD_FR, 75
    p, reps = MODULUS[field], E.representations(field)
    pats = E.patterns(field, 5, n, seed=3)
    assert pats["constant"] == [5] * n and pats["alt_zero"][:3] == [5, 0, 5] and pats["alt_pm1"][:3] == [5, p - 1, 5]
    assert pats["ends"][0] == pats["ends"][-1] == 5 and not any(pats["ends"][1:-1])
    assert E.holds_all(pats["cycled"], field) and pats["cycled"][0] == reps[3] and set(pats["picked"]) <= set(reps)
    assert pats["picked"] == E.picked(reps, n, 3) and all(len(v) == n for v in pats.values())


# ---- the C oracle's transforms against Python integers on these patterns, so that it can stand in above 2^6 ----------------------
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 6])
def test_oracle_transforms_on_extreme_operands(k):
    mod = P.R_MOD
    cases = E.ntt_inputs(k, width=len(E.ntt_chosen()))
    if k == 6:
        assert E.holds_all(cases[0][1], E.FIELD_FR)
    for label, vec in cases:
        a, vals = E.to_array(vec), [E.to_value(r, E.FIELD_FR) for r in vec]

        def want(fn, *args):
            v = list(vals)
            fn(v, *args)
            return E.to_array(E.from_value(x, E.FIELD_FR) for x in v)
        assert (C.fft(a, k) == want(P.fft, k)).all(), label
        assert (C.ifft(a, k) == want(P.ifft, k)).all(), label
        assert (C.coset_fft(a, k) == want(P.coset_fft)).all(), label
        assert (C.coset_ifft(a, k) == want(P.coset_ifft)).all(), label
        assert (C.best_fft(a, C.get_omega_or_inv(k, True), k) == want(P.best_fft, P.get_omega_or_inv(k, True), k)).all(), label
    x, out = E.ntt_roundtrip_case(k)                                       # asserts the exact 0 and p - 1 in the oracle's output
    v = [E.to_value(r, E.FIELD_FR) for r in E.from_array(x)]
    P.fft(v, k)
    assert (E.to_array(E.from_value(t, E.FIELD_FR) for t in v) == out).all()


# ---- the kernels ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wave", [-1, 1, 0])
@pytest.mark.parametrize("k", [1, 2, 5, 6, 8, 9, 10, 12, 13])
def test_emu_ntt(emu_lib, k, wave):
    """fft and ifft on the patterns around one representation per size and on the oracle's ifft of the extreme vector, on the
    default kernel choice and with either kernel forced; the coset transforms and best_fft with the inverse omega on the default
    choice.  An emulated transform takes up to a second and a half from 2^10 points up, so the patterns thin out there: two for
    the coset transforms, and the cycled list alone where the forced kernel is the default one anyway (the wave-level kernel up
    to 2^8, the workgroup-level one above)."""
    same_as_default = (wave == 1 and k <= 8) or (wave == 0 and k > 8)
    limit = 1 if same_as_default else 6
    specs = [spec("ntt", k=k, wave=wave, ops=["fft", "ifft"], limit=limit)]
    if wave == -1:
        specs.append(spec("ntt", k=k, wave=wave, ops=["coset_fft", "coset_ifft", "best_fft_inv"], limit=2 if k >= 10 else 6, roundtrip=False))
    run_child(emu_lib, *specs)


def test_emu_ntt_4096_points_single_line_and_three_passes(emu_lib):
    """MIRA_TUNE_NTT_MAX_LOG_LINE = 12: one workgroup walks twelve layers; = 4: three passes of 16-point lines, on the wave-level
    kernel and (one vector: 256 emulated workgroups per pass) on the workgroup-level one"""
    run_child(emu_lib, spec("ntt", k=12, max_log_line=12, ops=["fft", "ifft"], limit=2),
              spec("ntt", k=12, max_log_line=4, wave=1, ops=["fft", "ifft"], limit=2),
              spec("ntt", k=12, max_log_line=4, wave=0, ops=["fft"], limit=1, roundtrip=False))


@pytest.mark.parametrize("field", E.FIELDS)
def test_emu_fold(emu_lib, field):
    run_child(emu_lib, spec("fold_pairs", field=field), spec("fold_targets", field=field), spec("fold_lengths", field=field))


@pytest.mark.parametrize("field", E.FIELDS)
def test_emu_lincomb_and_pow_tree(emu_lib, field):
    run_child(emu_lib, spec("lincomb", field=field), spec("pow_tree", field=field))


@pytest.mark.parametrize("chunk", [None, 2, 64])
@pytest.mark.parametrize("field", E.FIELDS)
def test_emu_batch_invert_and_lookup_h_g(emu_lib, field, chunk):
    run_child(emu_lib, spec("batch_invert", field=field, chunk=chunk), spec("lookup_h_g", field=field, chunk=chunk))


@pytest.mark.parametrize("group", ["gate", "chain"])
@pytest.mark.parametrize("field", E.FIELDS)
def test_emu_graph_engines(emu_lib, field, group):
    run_child(emu_lib, spec("graph", field=field, group=group))


@pytest.mark.parametrize("field", E.FIELDS)
def test_emu_specialised_source_of_the_chained_expressions_compiles(emu_lib, field):
    """The emulation has no run-time compiler: as in test_graph_jit_source.py, the source mira_graph_specialize would build
    for the hand-written worst-case expressions is generated and compiled for gfx950; its values are the GPU suite's business."""
    from harness import graph_evaluator as G
    from test_graph_jit_source import _compiles
    label, e = E.graph_expressions(field, "chain")[-1]
    ev = G.GraphEvaluator.new(e, field)
    cols = [(1, G.COL_BOOL)] * 2 + [(1, G.COL_FIELD)] * 10
    src = ev.jit_source(cols, 3, lib=emu_lib)
    assert f"using F = {'Fq29' if field == E.FIELD_FQ else 'Fr29'};" in src and "mira_jit_eval" in src
    _compiles(src)
    ev.close()
