"""The gates of a circuit over a Lagrange combination of traces: mira_graph_eval_folded_device and mira_graph_eval_folded_reduce
(ProtoGalaxy's compute_G with FoldedTrace created on the fly, reference src/nifs/protogalaxy/poly/mod.rs:218-303 and
folded_trace.rs:53-131).

The check_* drivers below run on whichever library they are handed: tests/test_folded_eval_emu.py runs them on the CPU emulation
of the kernels (built with the bound tracking of field29.cuh, which aborts on a value outside the multiplier's budget),
tests/test_gpu_folded_eval.py on the GPU.  Expected values never come from the library under test: Python integers and
oracle.pyref.eval_expression for leaves and tree, pyref.pg_compute_G / pg_compute_K for the pipeline; where a driver compares two
entry points of the library with each other it says so.  Every comparison is on bytes.

The circuit: selector s (column 0), fixed f (1), advice a, b, c (2, 3, 4), one challenge, and the gates
    gate 0:  s * (a * b - c)
    gate 1:  s * (a + f - b[+1]) * ch0
    gate 2:  s[-1] * (a[-1] * a[+5] + f[-1])      the same folded column at two rotations, a rotation larger than a small row
                                                  count, a rotation on a shared column and on the selector
    gate 3:  a graph without calculations         (zero leaves)"""
import ctypes
import functools
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import edge_operands as E                                                    # noqa: E402
from harness import graph_evaluator as G                                     # noqa: E402
from mira_amd import _lib                                                    # noqa: E402
from mira_amd import graph_evaluator as engine                               # noqa: E402
from mira_amd.graph_evaluator import MODULUS                                 # noqa: E402
from oracle import pyref as P                                                # noqa: E402

FIELDS = E.FIELDS
NUM_COLUMNS, NUM_SHARED, NUM_ADVICE = 5, 2, 3
FOLDED = [False, False, True, True, True]
_s, _f, _a, _b, _c = (G.Polynomial(i) for i in range(5))
GATES = [G.Product(_s, G.Sum(G.Product(_a, _b), G.Negated(_c))),
         G.Product(G.Product(_s, G.Sum(G.Sum(_a, _f), G.Negated(G.Polynomial(3, 1)))), G.Challenge(0)),
         G.Product(G.Polynomial(0, -1), G.Sum(G.Product(G.Polynomial(2, -1), G.Polynomial(2, 5)), G.Polynomial(1, -1)))]
ROWS = (1, 2, 4, 128, 255, 256, 257, 512)
TRACES = (1, 2, 3, 16)
POINTS = (1, 2, 8)
# every row count with three of the twelve (traces, points) pairs by turns: every pair twice, every count with every trace count
# or point count of the lists at least once over the two fields' worth of turns
LEAF_CASES = [(rows, TRACES[(3 * i + q) % 4], POINTS[(i + q) % 3]) for i, rows in enumerate(ROWS) for q in range(3)]
assert {(t, p) for _, t, p in LEAF_CASES} == {(t, p) for t in TRACES for p in POINTS}
# (gates, k, points, MIRA_TUNE_FOLDED_GRID values): every gate count, every k and every point count of the lists; the largest k
# with one workgroup and with three walking its row blocks
REDUCE_CASES = [(1, 0, 1, (0,)), (2, 0, 8, (0,)), (2, 1, 8, (0,)), (4, 2, 32, (0,)), (1, 7, 8, (0,)), (2, 8, 1, (0,)), (1, 8, 32, (0,)), (4, 9, 1, (0,)),
                (2, 9, 8, (0, 3)), (1, 11, 1, (0, 1, 3))]
assert {g for g, _, _, _ in REDUCE_CASES} == {1, 2, 4} and {k for _, k, _, _ in REDUCE_CASES} == {0, 1, 2, 7, 8, 9, 11} and {p for _, _, p, _ in REDUCE_CASES} == {1, 8, 32}


def vp(x):
    return x.ctypes.data_as(ctypes.c_void_p)


def evaluators(field, count=3):
    """the first `count` gates; the fourth is a graph without calculations"""
    evs = [G.GraphEvaluator.new(g, field) for g in GATES[:min(count, 3)]]
    if count == 4:
        evs.append(engine.GraphEvaluator(field))
    return evs


def gate_tuples(count=3):
    return [g.to_tuple() for g in GATES[:min(count, 3)]] + ([("const", 0)] if count == 4 else [])


class Case:
    """`traces` traces of `rows` rows as Python integers (values, not representations) and the data of `points` evaluation points"""

    def __init__(self, field, rows, traces, points, seed, draw=None):
        self.field, self.rows, self.traces, self.points, self.mod = field, rows, traces, points, MODULUS[field]
        rng = random.Random(seed)
        draw = draw or (lambda: rng.getrandbits(256) % self.mod)
        self.sel = [rng.random() < 0.7 for _ in range(rows)]
        self.fix = [draw() for _ in range(rows)]
        self.adv = [[[draw() for _ in range(rows)] for _ in range(NUM_ADVICE)] for _ in range(traces)]       # [trace][column][row]
        self.coeffs = [[draw() for _ in range(traces)] for _ in range(points)]
        self.challenges = [[draw()] for _ in range(points)]

    def folded_getter(self, p):
        adv = [[sum(c * self.adv[j][col][r] for j, c in enumerate(self.coeffs[p])) % self.mod for r in range(self.rows)] for col in range(NUM_ADVICE)]
        return dict(selectors=[self.sel], fixed=[self.fix], advice=adv, challenges=self.challenges[p])

    def leaves(self, count=3):
        """[point][gate][row] by Python integers"""
        tuples = gate_tuples(count)
        out = []
        for p in range(self.points):
            getter = self.folded_getter(p)
            out.append([[P.eval_expression(t, getter, r, self.rows, self.mod) for r in range(self.rows)] for t in tuples])
        return out

    def array(self, values):
        return E.to_array(E.from_value(v, self.field) for v in values)


def tree(leaves, weights, mod):
    """sum_i leaf[i] * prod_{j : bit j of i} weights[j], level by level as itertools::tree_reduce pairs them"""
    nodes, height = list(leaves), 0
    while len(nodes) > 1:
        nodes = [(nodes[i] + nodes[i + 1] * weights[height]) % mod for i in range(0, len(nodes), 2)]
        height += 1
    return nodes[0]


@functools.lru_cache(maxsize=None)
def leaf_case(field, rows, traces, points):
    case = Case(field, rows, traces, points, seed=rows * 1000 + traces * 10 + points)
    return case, case.leaves(3)


@functools.lru_cache(maxsize=None)
def reduce_case(field, gates, k, points):
    case = Case(field, 1 << k, 2 + (k % 2), points, seed=7000 + 100 * k + 10 * gates + points)
    leaves = case.leaves(gates)
    rng = random.Random(k + gates)
    levels = k + gates.bit_length() - 1
    weights = [rng.getrandbits(256) % case.mod for _ in range(levels)]
    roots = [tree([v for gate in leaves[p] for v in gate], weights, case.mod) for p in range(case.points)]
    return case, leaves, weights, roots


class Placed:
    """a Case in device memory: one column table per trace"""

    def __init__(self, lib, case, same_buffers=False):
        self.lib, self.case, self.ptrs = lib, case, []
        sel, fix = self.put(np.array(case.sel, dtype=np.uint8)), self.put(case.array(case.fix))
        self.tables = []
        for j in range(case.traces):
            src = case.adv[0 if same_buffers else j]
            adv = self.tables[0][NUM_SHARED:] if same_buffers and j else [(self.put(case.array(col)), G.COL_FIELD) for col in src]
            self.tables.append([(sel, G.COL_BOOL), (fix, G.COL_FIELD)] + adv)

    def put(self, arr):
        p = self.lib.alloc(max(1, arr.nbytes))
        self.lib.upload(p, arr)
        self.ptrs.append(p)
        return p

    def empty(self, n):
        return self.put(np.full((max(1, n), 4), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64))

    def free(self):
        for p in self.ptrs:
            self.lib.free(p)
        self.ptrs = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()


def run_leaves(lib, evs, placed, case, tables=None, coeffs=None):
    n = case.points * len(evs) * case.rows
    d = placed.empty(n)
    G.GraphEvaluator.evaluate_folded_device(evs, tables or placed.tables, FOLDED, coeffs or case.coeffs, case.challenges, case.rows, d, lib=lib)
    return lib.download(d, (n, 4)) if n else np.zeros((0, 4), dtype=np.uint64)


def flat(case, leaves):
    return case.array(v for point in leaves for gate in point for v in gate)


def close(evs):
    for ev in evs:
        ev.close()


# ---- 1. leaves against Python integers ------------------------------------------------------------------------------------------
def check_leaves(lib, field, cases=LEAF_CASES):
    evs = evaluators(field)
    try:
        for rows, traces, points in cases:
            case, want = leaf_case(field, rows, traces, points)
            with Placed(lib, case) as pl:
                E.same_bytes(run_leaves(lib, evs, pl, case), flat(case, want), f"folded leaves field={field} rows={rows} traces={traces} points={points}")
    finally:
        close(evs)


# ---- 2. identities against mira_graph_eval_compiled -----------------------------------------------------------------------------
def check_identities(lib, field, rows=257):
    """compares two entry points of the library: the folded fetch with unit coefficients is the plain fetch"""
    evs = evaluators(field)
    try:
        def plain(pl, case, table, challenges):
            out = []
            for ev in evs:
                d = ev.evaluate_device(table, challenges, rows, lib=lib)
                pl.ptrs.append(d)
                out.append(lib.download(d, (rows, 4)))
            return np.concatenate(out)
        one = Case(field, rows, 1, 1, seed=31)
        one.coeffs = [[1]]
        with Placed(lib, one) as pl:
            E.same_bytes(run_leaves(lib, evs, pl, one), plain(pl, one, pl.tables[0], one.challenges[0]), f"one trace, coefficient 1, field={field}")
        four = Case(field, rows, 4, 4, seed=32)
        four.coeffs = [[1 if j == p else 0 for j in range(4)] for p in range(4)]
        with Placed(lib, four) as pl:
            want = np.concatenate([plain(pl, four, pl.tables[p], four.challenges[p]) for p in range(4)])
            E.same_bytes(run_leaves(lib, evs, pl, four), want, f"coeffs[p] = e_p, field={field}")
        same = Case(field, rows, 5, 2, seed=33)
        for row in same.coeffs:                                             # coefficients summing to one
            row[-1] = (1 - sum(row[:-1])) % same.mod
        with Placed(lib, same, same_buffers=True) as pl:
            want = np.concatenate([plain(pl, same, pl.tables[0], same.challenges[p]) for p in range(2)])
            E.same_bytes(run_leaves(lib, evs, pl, same), want, f"one trace five times, coefficients summing to 1, field={field}")
    finally:
        close(evs)


# ---- 3. worst-case operands -----------------------------------------------------------------------------------------------------
def check_worst_case(lib, field, rows=67, traces=16, points=4):
    """column values, coefficients and challenges from edge_operands' extreme representations (0, 1, p - 1, p - 2, 2^253, all-ones
    limbs ...): sixteen un-normalised terms of such a fold would leave the multiplier's budget, which the emulation's bound
    tracking reports by aborting"""
    reps = E.representations(field)
    cv = E._Convert(field)
    it = iter(range(1 << 30))
    case = Case(field, rows, traces, points, seed=5, draw=lambda: cv.value(reps[(7 * next(it)) % len(reps)]))
    case.coeffs[0] = [cv.value(MODULUS[field] - 1)] * traces                 # the largest representation in every term
    case.adv[0][0] = [cv.value(MODULUS[field] - 1)] * rows
    want = case.leaves(3)
    evs = evaluators(field)
    try:
        with Placed(lib, case) as pl:
            E.same_bytes(run_leaves(lib, evs, pl, case), flat(case, want), f"worst-case operands field={field}")
    finally:
        close(evs)


# ---- 4. reduce against the definition -------------------------------------------------------------------------------------------
def check_reduce(lib, field, cases=REDUCE_CASES):
    for gates, k, points, grids in cases:
        case, leaves, weights, roots = reduce_case(field, gates, k, points)
        evs = evaluators(field, gates)
        tag = f"folded reduce field={field} gates={gates} k={k} points={points}"
        try:
            with Placed(lib, case) as pl:
                for grid in grids:
                    with E.knobs(lib, FOLDED_GRID=grid):
                        got = G.GraphEvaluator.evaluate_folded_reduce(evs, pl.tables, FOLDED, case.coeffs, case.challenges, case.rows, weights, lib=lib)
                        E.same_bytes(got, case.array(roots), f"{tag} grid={grid}")
                        written = run_leaves(lib, evs, pl, case)
                    E.same_bytes(written, flat(case, leaves), f"{tag} grid={grid}: leaves")
                # the library's own tree over the leaves the other entry point wrote
                n = gates << k
                d = pl.put(written)
                out = np.zeros((points, 4), dtype=np.uint64)
                w = case.array(weights * points) if weights else np.zeros((1, 4), dtype=np.uint64)
                lib.check(lib.c.mira_pow_tree_reduce_device(field, ctypes.c_void_p(d), n, n, vp(w), points, vp(out)))
                E.same_bytes(out, case.array(roots), f"{tag}: mira_pow_tree_reduce_device over the written leaves")
        finally:
            close(evs)


# ---- 5. the pipeline ------------------------------------------------------------------------------------------------------------
def check_pipeline(lib, k, satisfied, num_traces):
    from harness import protogalaxy as PG
    from test_protogalaxy import MOD, build_case
    ints, traces, S, dev, ptrs = build_case(lib, k, seed=60 + k, satisfied=satisfied, num_traces=num_traces)
    try:
        rng = random.Random(300 + k)
        betas = [rng.getrandbits(250) % MOD for _ in range(16)]
        alpha, delta, f_alpha = (rng.getrandbits(250) % MOD for _ in range(3))
        bs = PG.beta_stroke(betas, alpha, delta)
        md = S.max_degree()
        got = PG.compute_G_fused(S, bs, dev[0], dev[1:], lib=lib)
        assert got == P.pg_compute_G(ints, bs, traces[0], traces[1:], md)
        assert got == PG.compute_G(S, bs, dev[0], dev[1:], lib=lib)
        assert len(got) == 1 << (num_traces * md).bit_length()
        if satisfied:
            for X in P.pg_cyclic_subgroup(num_traces.bit_length())[: num_traces + 1]:      # G vanishes on the Lagrange domain
                assert sum(c * pow(X, i, MOD) for i, c in enumerate(got)) % MOD == 0
            assert not any(PG.compute_G_fused(S, bs, dev[0], [dev[0]], lib=lib))            # zero_g (:457-478)
        else:
            assert any(got)
        assert PG.compute_K(S, f_alpha, bs, dev[0], dev[1:], lib=lib, fused=True) == P.pg_compute_K(ints, f_alpha, bs, traces[0], traces[1:], md)
    finally:
        for p in ptrs:
            lib.free(p)


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------
def check_refusals(lib, field):
    """every error of the two calls with its code, and nothing written to d_out / out"""
    rows, traces, points = 16, 3, 2
    case = Case(field, rows, traces, points, seed=9)
    evs, other = evaluators(field), evaluators(1 - field)
    sentinel = 0xA5A5A5A5A5A5A5A5
    with Placed(lib, case) as pl:
        d_out = pl.empty(points * 3 * rows)
        handles = [ev.compiled(1, NUM_COLUMNS, lib) for ev in evs]
        co, ch = G.to_montgomery([v for r in case.coeffs for v in r], field), G.to_montgomery([v for r in case.challenges for v in r], field)
        w = G.to_montgomery([3, 5, 7, 11, 13, 17], field)
        big = [c for t in pl.tables for c in t] + [pl.tables[0][c] for _ in range(16) for c in range(NUM_COLUMNS)]       # room for 17 traces

        def call(code, text, handles=handles, table=big, ncols=NUM_COLUMNS, ntraces=traces, folded=FOLDED, nchal=1, npoints=points, nrows=rows, gates=3,
                 reduce_only=False):
            hs = (ctypes.c_uint64 * len(handles))(*handles)
            cols = G.GraphEvaluator._column_table(table)
            flags = (ctypes.c_uint8 * len(folded))(*[1 if x else 0 for x in folded])
            out = np.full((256, 4), sentinel, dtype=np.uint64)
            rcs = [] if reduce_only else [lib.c.mira_graph_eval_folded_device(hs, gates, cols, ncols, ntraces, flags, vp(co), vp(ch), nchal, npoints, nrows, ctypes.c_void_p(d_out))]
            rcs.append(lib.c.mira_graph_eval_folded_reduce(hs, gates, cols, ncols, ntraces, flags, vp(co), vp(ch), nchal, npoints, nrows, vp(w), vp(out)))
            for rc in rcs:
                assert rc == code and text in (lib.c.mira_last_error() or b"").decode(), (rc, code, text, lib.c.mira_last_error())
            assert (out == sentinel).all() and (lib.download(d_out, (points * 3 * rows, 4)) == sentinel).all(), text
        call(_lib.MIRA_E_BAD_ARG, "unknown graph handle", handles=handles[:2] + [0xDEAD0000])
        call(_lib.MIRA_E_BAD_ARG, "one field", handles=handles[:2] + [other[0].compiled(1, NUM_COLUMNS, lib)])
        call(_lib.MIRA_E_BAD_ARG, "compiled for", handles=handles[:2] + [evs[0].compiled(1, NUM_COLUMNS + 1, lib)])
        call(_lib.MIRA_E_BAD_ARG, "compiled for", handles=handles[:2] + [evs[0].compiled(2, NUM_COLUMNS, lib)])
        hole = list(big)
        hole[1] = None                                                        # the fixed column, read by gates 1 and 2, of trace 0
        call(_lib.MIRA_E_BAD_ARG, "column variable index out of boundary", table=hole)
        hole = list(big)
        hole[2 * NUM_COLUMNS + 3] = None                                      # a folded column in trace 2
        call(_lib.MIRA_E_BAD_ARG, "column variable index out of boundary", table=hole)
        hole = list(big)
        hole[NUM_COLUMNS + 2] = (big[0][0], G.COL_BOOL)                       # a folded column of bytes
        call(_lib.MIRA_E_BAD_ARG, "MIRA_COL_FIELD", table=hole)
        call(_lib.MIRA_E_BAD_ARG, "MIRA_COL_FIELD", folded=[True] + FOLDED[1:])  # the selector declared a witness column
        for bad in (0, 17):
            call(_lib.MIRA_E_BAD_ARG, "num_traces", ntraces=bad)
        for bad in (0, 257):
            call(_lib.MIRA_E_BAD_ARG, "num_points", npoints=bad)
        call(_lib.MIRA_E_UNSUPPORTED, "2^31", nrows=(1 << 31) + 1)
        call(_lib.MIRA_E_UNSUPPORTED, "power-of-two", reduce_only=True)       # three gates
        call(_lib.MIRA_E_UNSUPPORTED, "power-of-two", reduce_only=True, gates=2, nrows=12)
        # no rows: success, `out` all zero, d_out untouched
        out = np.full((points, 4), sentinel, dtype=np.uint64)
        hs, cols, flags = (ctypes.c_uint64 * 3)(*handles), G.GraphEvaluator._column_table(big), (ctypes.c_uint8 * NUM_COLUMNS)(*[1 if x else 0 for x in FOLDED])
        lib.check(lib.c.mira_graph_eval_folded_reduce(hs, 3, cols, NUM_COLUMNS, traces, flags, vp(co), vp(ch), 1, points, 0, vp(w), vp(out)))
        lib.check(lib.c.mira_graph_eval_folded_device(hs, 3, cols, NUM_COLUMNS, traces, flags, vp(co), vp(ch), 1, points, 0, ctypes.c_void_p(d_out)))
        assert not out.any() and (lib.download(d_out, (points * 3 * rows, 4)) == sentinel).all()
        # and the calls still work after the refusals
        E.same_bytes(run_leaves(lib, evs, pl, case), flat(case, case.leaves(3)), f"after the refusals, field={field}")
    close(evs + other)


# ---- 7. guard bands -------------------------------------------------------------------------------------------------------------
def check_guarded(lib, field, lengths=(255, 256, 257), traces=3, points=2):
    """d_out, advice column a of every trace and the fixed column inside one allocation between guard bands (tests/guarded.py):
    rotations -1, +1 and +5 wrap at both ends, so an unreduced row reads guard fill -- non-canonical, it changes the value"""
    import guarded as GD
    evs = evaluators(field)
    try:
        for rows in lengths:
            case, want = leaf_case(field, rows, traces, points)
            for off in GD.OFFSETS:
                tag = f"folded guarded field={field} rows={rows} offset={off}"
                with Placed(lib, case) as pl, GD.Arena(lib) as A:
                    fix = A.place(case.array(case.fix), GD.shifted(off, 0), "fixed")
                    cols = [A.place(case.array(case.adv[j][0]), GD.shifted(off, j + 1), f"a of trace {j}") for j in range(traces)]
                    out = A.place(points * 3 * rows, GD.shifted(off, 2), "d_out")
                    tables = [[t[0], (fix.ptr, G.COL_FIELD), (cols[j].ptr, G.COL_FIELD)] + t[3:] for j, t in enumerate(pl.tables)]
                    G.GraphEvaluator.evaluate_folded_device(evs, tables, FOLDED, case.coeffs, case.challenges, rows, out.ptr, lib=lib)
                    got, = A.check(tag, [out])
                    GD.same(got, flat(case, want), tag)
                    if rows & (rows - 1) == 0:                               # the reduce call writes nothing the caller sees but `out`
                        weights = [3 + j for j in range(rows.bit_length() - 1)]
                        roots = G.GraphEvaluator.evaluate_folded_reduce(evs[:1], tables, FOLDED, case.coeffs, case.challenges, rows, weights, lib=lib)
                        A.check(tag + " reduce")
                        E.same_bytes(roots, case.array(tree(want[p][0], weights, case.mod) for p in range(points)), tag + " reduce")
    finally:
        close(evs)


# ---- 8. scratch state -----------------------------------------------------------------------------------------------------------
def check_scratch_state(lib, field):
    """the reduce call large (k = 11), small (k = 2), the workspaces released, large again: the node buffer and the tree's
    workspaces are written before they are read whatever they held"""
    large, small = reduce_case(field, 1, 11, 1), reduce_case(field, 4, 2, 32)

    def run(which):
        case, _, weights, roots = which
        gates = 1 if which is large else 4
        evs = evaluators(field, gates)
        try:
            with Placed(lib, case) as pl:
                got = G.GraphEvaluator.evaluate_folded_reduce(evs, pl.tables, FOLDED, case.coeffs, case.challenges, case.rows, weights, lib=lib)
        finally:
            close(evs)
        E.same_bytes(got, case.array(roots), f"scratch state field={field} k={case.rows.bit_length() - 1}")
        return got
    first = run(large)
    run(small)
    lib.trim(0)
    assert (run(large) == first).all()
    run(small)
    assert (run(large) == first).all()


# ---- 9. a specialised handle (GPU only: the emulation has no run-time compiler) -------------------------------------------------
def check_specialised(lib, skip):
    """the two small gates of test_protogalaxy.build_case with kernels of their own: the folded calls interpret them and return
    the values of the unspecialised run (and Python's)"""
    field = E.FIELD_FR
    case, want = leaf_case(field, 257, 3, 2)
    pow2 = Case(field, 256, 3, 2, seed=77)
    weights = list(range(3, 12))
    before, after = evaluators(field, 2), evaluators(field, 2)
    try:
        with Placed(lib, case) as pl, Placed(lib, pow2) as pl2:
            plain = run_leaves(lib, before, pl, case)
            plain_roots = G.GraphEvaluator.evaluate_folded_reduce(before, pl2.tables, FOLDED, pow2.coeffs, pow2.challenges, 256, weights, lib=lib)
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                if not G.GraphEvaluator.specialize(after, pl.tables[0], 1, lib=lib):
                    skip((lib.c.mira_last_error() or b"").decode())
            assert all(ev.is_specialized(1, NUM_COLUMNS, lib) for ev in after)
            E.same_bytes(run_leaves(lib, after, pl, case), plain, "specialised handles: leaves")
            E.same_bytes(plain, case.array(v for point in want for gate in point[:2] for v in gate), "specialised handles: leaves against Python")
            roots = G.GraphEvaluator.evaluate_folded_reduce(after, pl2.tables, FOLDED, pow2.coeffs, pow2.challenges, 256, weights, lib=lib)
            E.same_bytes(roots, plain_roots, "specialised handles: roots")
            leaves = pow2.leaves(2)
            E.same_bytes(roots, pow2.array(tree([v for gate in leaves[p] for v in gate], weights, pow2.mod) for p in range(2)), "specialised handles: roots against Python")
    finally:
        close(before + after)
