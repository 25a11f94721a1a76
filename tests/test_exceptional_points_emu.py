"""P = Q, P = -Q and the identity through every stage and mode of the MSM on the CPU emulation (tests/exceptional_points.py builds
the cases and drives them), with the emulation's branch census (F29_HIT in curve29.cuh / quad29.cuh, HOSTF_HIT in host_field.hpp,
counted per kernel and section by tests/emu/emu.h) as the proof that the cases reach what they are built for:

  (a) every result is byte for byte (sum_i s_i k_i mod r) G from Python integers;
  (b) every (kernel, section, function, exit) of REQUIRED below was taken at least once over the whole module.

tests/test_gpu_exceptional_points.py runs the same cases under the same knobs on the GPU, where the quad versions really share
their multiplications over DPP: what the census shows here is what that run executes."""
import pytest

import exceptional_points as X
from oracle import cref as C

# (mode, curve) pairs of the module.  The modes whose emulated commits take seconds run on one curve each; the GPU module runs
# every mode on both.
RUNS = [(mode, cid) for mode in ("plain", "plain_single_lane_tree", "glv", "host_chunks", "partials", "batch") for cid in (0, 1)] + \
       [("shared8", 0), ("shared13", 1), ("front", 0), ("staged", 1), ("tables20", 1)]

_done = {}           # (mode, cid) -> ([(label, got, expected)], census of that run)


def _run(emu_lib, mode, cid):
    if (mode, cid) not in _done:
        X.census_reset(emu_lib)
        res = X.run_tables(emu_lib, cid, int(mode[6:])) if mode.startswith("tables") else X.run_mode(emu_lib, mode, cid)
        _done[(mode, cid)] = (res, X.census_read(emu_lib))
    return _done[(mode, cid)]


# ---- the builder ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [0, 1])
def test_cases_against_the_oracle(cid):
    """The expected points come from Python integers alone; the C oracle's Pippenger -- with its own handling of equal and opposite
    points -- is pinned to them on every case of at most 2^12 pairs: the cases of every width that a mode of this module or of
    tests/test_gpu_exceptional_points.py runs, the batch vectors, both table cases and the 2^12-pair keys of the wide windows.  (The
    larger GPU-only shapes rest on the Python integers alone.)  cases() itself asserts that alt_identity alone expects the identity."""
    lam = X.eigenvalue(cid)
    assert (X.multiple_of_g(cid, lam)[4:] == X.multiple_of_g(cid, 1)[4:]).all() and (X.multiple_of_g(cid, lam)[:4] != X.multiple_of_g(cid, 1)[:4]).any()   # phi keeps y
    widths = {X.CASE_WIDTH.get(c, c) for ws, _, _ in X.MODES.values() for c in ws} | set(X.GLV_FORCED_WIDTHS) | set(X.WIDE_WIDTHS)
    assert widths == {5, 7, 8, 9, 10, 11, 12, 13, 16, 17, 20}
    for c in sorted(widths):
        every = X.cases(cid, c, True) + X.batch_case(cid, c)
        assert sum(1 for cs in every if not cs.expected().any()) == 1
        for cs in every:
            assert cs.n <= 1 << 12
            assert (C.msm_pippenger(cid, cs.scalar_array(), cs.bases()) == cs.expected()).all(), (c, cs.name)
    others = [X.table_case(cid, bits) for bits in (20, 22)] + [X.wide_case(cid, c, key) for c in X.WIDE_WIDTHS for key in ("all_g", "periodic")]
    for cs in others:
        assert cs.n <= 1 << 12 and cs.expected().any()
        assert (C.msm_pippenger(cid, cs.scalar_array(), cs.bases()) == cs.expected()).all(), cs.name


# ---- (a) ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,cid", RUNS)
def test_emu_results_are_the_integer_values(emu_lib, mode, cid):
    res, _ = _run(emu_lib, mode, cid)
    assert res
    bad = [label for label, got, want in res if not (got == want).all()]
    assert not bad, bad


# ---- (b) ------------------------------------------------------------------------------------------------------------------------
ADD = ("identity_in", "same", "opposite", "common")      # "opposite" is the exit whose result is the identity
DBL = ("identity_in", "common")
REQUIRED = [
    ("k_accumulate<F, false>", "", "add_affine", ADD),
    ("k_accumulate<F, true>", "", "add_affine", ADD),                      # a later point chunk adds into the sums of the ones before
    ("k_fixup_all<F>", "light", "add_quad", ADD),
    ("k_fixup_all<F>", "heavy_a", "add_quad", ADD),
    ("k_fixup_heavy_b<F>", "", "add_quad", ADD),
    ("k_bucket_tree<F, true>", "phase_a", "add_quad", ADD),
    ("k_bucket_tree<F, true>", "node_tree", "add_quad", ADD),
    ("k_bucket_tree<F, false>", "phase_a", "add", ADD),
    ("k_bucket_tree<F, false>", "node_tree", "add_quad", ADD),
    ("k_set_finish<F>", "node_tree", "add_quad", ADD),
    ("k_set_finish<F>", "horner", "add_quad", ADD),
    ("k_set_finish<F>", "horner", "double_quad", DBL),
    ("k_reduce_chunks<F, false>", "", "add", ADD),
    ("k_reduce_chunks<F, false>", "", "double", DBL),
    ("k_window_sum<F, false>", "", "add", ADD),
    ("k_table_step<F>", "", "double", ("common",)),
    ("host", "horner_pieces", "add_pt", ADD),
    ("host", "horner_pieces", "dbl_pt", DBL),
    ("host", "sum_partials", "add_pt", ADD),
]
# What the code cannot reach by construction:
#   - a doubling called from the same-point exit of an addition never sees the identity (the operands were checked), so
#     "identity_in" of double / double_quad is asked for only where a kernel doubles on its own: the Horner chains of k_set_finish
#     and k_reduce_chunks
#   - k_table_step and k_glv_bases never add: an identity base leaves k_table_step before its first doubling (the keys of the
#     table modes hold one), and k_glv_bases multiplies x by beta without any group operation
#   - dbl_pt's exit for y = 0 ("identity_out"): both groups have odd prime order, no point has order two
#   - k_reduce_chunks<F, true> and k_window_sum<F, true> are never launched (the table path reduces by single lanes)
#   - sum_partials never doubles on its own
UNREACHABLE = [("host", "horner_pieces", "dbl_pt", "identity_out"), ("host", "sum_partials", "dbl_pt", "identity_out"), ("host", "g1", "dbl_pt", "identity_out")]


def test_emu_census_covers_every_branch(emu_lib):
    total = {}
    for mode, cid in RUNS:
        for key, hits in _run(emu_lib, mode, cid)[1].items():
            total[key] = total.get(key, 0) + hits
    missing = [(kernel, section, fn, site) for kernel, section, fn, sites in REQUIRED for site in sites if not total.get((kernel, section, fn, site))]
    assert not missing, missing
    assert not [key for key in UNREACHABLE if total.get(key)]
    # every host addition and doubling runs inside one of the marked functions: none is counted without a section
    assert not [key for key in total if key[0] == "host" and not key[1]]
    # the kernels of the table whose launches the census saw are all named above: a new kernel that adds points shows up here
    known = {k for k, _, _, _ in REQUIRED}
    assert {key[0] for key in total} <= known, {key[0] for key in total} - known
