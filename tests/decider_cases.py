"""Shared bodies of the decider tests (CPU: tests/test_decider_emu.py on the emulation; GPU: tests/test_gpu_decider.py through
libmira_gpu.so): mira_count_ne_device, mira_sum_sub_device, mira_graph_check_compiled, mira_perm_* and the deciders of
mira_amd/decider.py against Python integers, the oracle's walk of the calculation list and the restatement of the
reference's permutation code in harness/permutation.py.  No entry point under test produces its own expectation.

Sizes: 0, 1, around one wave (63, 64) and one workgroup (255, 256, 257), and 1553 = 3 workgroups x 2 strides + 17, which
with MIRA_TUNE_DECIDE_GRID = 3 gives the partial records and the finish kernel several workgroups and a ragged tail."""
import random

import numpy as np

from graph_cases import gate_like_expression, mock_data, oracle_columns
from helpers import ints_to_mont, mont_to_ints
from harness import graph_evaluator as G
from harness import lookup as LK
from harness import permutation as PM
from mira_amd import _lib
from mira_amd import commitment as cm
from mira_amd import decider as D
from mira_amd import fold as FD
from oracle import cref as C
from oracle import pyref as P

MODS = {0: P.P_MOD, 1: P.R_MOD}
FIELDS = [0, 1]
SIZES = [0, 1, 63, 64, 255, 256, 257, 1553]
# (n, grid knob): every size with one workgroup and with the default grid; 1553 also with three workgroups
SHAPES = [(n, grid) for n in SIZES for grid in (1, -1)] + [(1553, 3)]
# workgroup boundaries of the device (256 lanes), of the emulation (8 lanes) and of the strides of three workgroups
EDGES = [7, 8, 255, 256, 511, 512, 767, 768, 1535, 1536]


def raw(vals):
    """256-bit integers -> (n, 4) uint64 limbs as they are (the compare kernels see representations, not values)"""
    return np.array([P.limbs4(v) for v in vals], dtype=np.uint64).reshape(-1, 4)


class Dev:
    def __init__(self, lib):
        self.lib, self.ptrs = lib, []

    def put(self, arr):
        arr = np.ascontiguousarray(arr, dtype=np.uint64).reshape(-1, 4)
        p = self.lib.alloc(max(1, len(arr)) * 32)
        if len(arr):
            self.lib.upload(p, arr)
        self.ptrs.append(p)
        return p

    def poke(self, p, i, limbs):
        self.lib.upload(p + i * 32, np.asarray(limbs, dtype=np.uint64).reshape(1, 4))

    def free(self):
        for p in self.ptrs:
            self.lib.free(p)
        self.ptrs = []


def expect_ne(a, b):
    bad = [i for i, (x, y) in enumerate(zip(a, b)) if x != y]
    return len(bad), (bad[0] if bad else D.NONE)


# ---------------------------------------------------------------- count_ne
def run_count_ne(lib, field, n, grid, seed=1):
    mod, rng, dev = MODS[field], random.Random(seed * 7919 + n), Dev(lib)
    lib.tune(_lib.TUNE_DECIDE_GRID, grid)
    try:
        a = [rng.randrange(mod) for _ in range(n)]
        d_a, d_b = dev.put(raw(a)), dev.put(raw(a))
        assert D.count_ne_device(field, d_a, d_b, n, lib=lib) == (0, D.NONE)                       # equal vectors
        if n == 0:
            assert D.count_ne_device(field, d_a, None, 0, lib=lib) == (0, D.NONE)
            assert D.count_ne_device(field, None, None, 0, lib=lib) == (0, D.NONE)
            return
        # a single mismatch at index 0, at n - 1 and at every workgroup boundary
        for i in sorted({0, n - 1} | {e for e in EDGES if e < n}):
            other = (a[i] + 1) % mod
            dev.poke(d_b, i, raw([other]))
            assert D.count_ne_device(field, d_a, d_b, n, lib=lib) == (1, i), i
            assert D.count_ne_device(field, d_b, d_a, n, lib=lib) == (1, i), i
            dev.poke(d_b, i, raw([a[i]]))
        # elements that differ only in the lowest limb / only in the top limb (both below the modulus: top limb < 0x30000000)
        i = rng.randrange(n)
        body = rng.getrandbits(192) << 32
        lo0, lo1 = (0x10000000 << 224) | body | 5, (0x10000000 << 224) | body | 4
        hi1 = (0x20000000 << 224) | body | 5
        for x, y in ((lo0, lo1), (lo0, hi1)):
            dev.poke(d_a, i, raw([x])); dev.poke(d_b, i, raw([y]))
            assert D.count_ne_device(field, d_a, d_b, n, lib=lib) == (1, i)
            dev.poke(d_b, i, raw([x]))
            assert D.count_ne_device(field, d_a, d_b, n, lib=lib) == (0, D.NONE)
        dev.poke(d_a, i, raw([a[i]])); dev.poke(d_b, i, raw([a[i]]))
        # a random mismatch set: count and first index are exact
        b = list(a)
        for j in rng.sample(range(n), rng.randrange(1, min(n, 40) + 1)):
            b[j] = (b[j] ^ (1 << rng.randrange(250))) % mod
        d_c = dev.put(raw(b))
        assert D.count_ne_device(field, d_a, d_c, n, lib=lib) == expect_ne(a, b)
        # d_b = NULL against a vector with exactly k non-zero elements
        k = rng.randrange(0, min(n, 17) + 1)
        z = [0] * n
        for j in rng.sample(range(n), k):
            z[j] = rng.randrange(1, mod)
        d_z = dev.put(raw(z))
        want = expect_ne(z, [0] * n)
        assert want[0] == k
        assert D.count_ne_device(field, d_z, None, n, lib=lib) == want
    finally:
        lib.tune(_lib.TUNE_DECIDE_GRID, -1)
        dev.free()


# ---------------------------------------------------------------- sum_sub
def run_sum_sub(lib, field, n, grid, seed=2):
    mod, rng, dev = MODS[field], random.Random(seed * 104729 + n), Dev(lib)
    lib.tune(_lib.TUNE_DECIDE_GRID, grid)
    try:
        def got(d_a, d_b):
            return mont_to_ints(D.sum_sub_device(field, d_a, d_b, n, lib=lib), mod)[0]
        top = [mod - 1] * n                                                                        # every addition wraps
        rnd = [rng.randrange(mod) for _ in range(n)]
        oth = [rng.randrange(mod) for _ in range(n)]
        perm = list(rnd)
        rng.shuffle(perm)
        d_top, d_zero, d_rnd, d_oth, d_perm = (dev.put(ints_to_mont(v, mod)) for v in (top, [0] * n, rnd, oth, perm))
        assert got(d_top, None) == sum(top) % mod
        assert got(d_top, d_zero) == sum(top) % mod
        assert got(d_zero, d_top) == -sum(top) % mod
        assert got(d_zero, None) == 0 and got(d_zero, d_zero) == 0
        assert got(d_rnd, None) == sum(rnd) % mod                                                  # d_b = NULL
        assert got(d_rnd, d_oth) == (sum(rnd) - sum(oth)) % mod
        assert got(d_top, d_oth) == (sum(top) - sum(oth)) % mod
        assert not D.sum_sub_device(field, d_rnd, d_perm, n, lib=lib).any()                        # b = a permuted: exactly 0
    finally:
        lib.tune(_lib.TUNE_DECIDE_GRID, -1)
        dev.free()


# ---------------------------------------------------------------- non-canonical inputs
def run_noncanonical(lib, field):
    import pytest
    mod, rng, dev, n = MODS[field], random.Random(3), Dev(lib), 257
    try:
        a = [rng.randrange(mod) for _ in range(n)]
        d_a = dev.put(ints_to_mont(a, mod))
        for bad in (mod, (1 << 256) - 1):
            for at in (0, 200, n - 1):
                d_x = dev.put(ints_to_mont(a, mod))
                dev.poke(d_x, at, raw([bad]))
                for call in (lambda: D.count_ne_device(field, d_x, d_a, n, lib=lib), lambda: D.count_ne_device(field, d_a, d_x, n, lib=lib),
                             lambda: D.count_ne_device(field, d_x, None, n, lib=lib), lambda: D.sum_sub_device(field, d_x, d_a, n, lib=lib),
                             lambda: D.sum_sub_device(field, d_a, d_x, n, lib=lib), lambda: D.sum_sub_device(field, d_x, None, n, lib=lib)):
                    with pytest.raises(_lib.MiraError) as err:
                        call()
                    assert err.value.code == _lib.MIRA_E_BAD_ARG
        assert D.count_ne_device(field, d_a, d_a, n, lib=lib) == (0, D.NONE)                       # the error word is cleared by the next call
    finally:
        dev.free()


# ---------------------------------------------------------------- permutation
def device_perm(lib, field, perm, Z, num_io, dev):
    d_w = dev.put(ints_to_mont(Z[num_io:], MODS[field]))
    return perm.check_device(Z[:num_io], d_w, len(Z) - num_io)


def want_perm(triples, Z, mod):
    count, first = PM.perm_mismatches(triples, Z, mod)
    return count, (D.NONE if first is None else first)


def as_csr(triples, rng, mod, splits=3):
    """The same matrix with `splits` of its entries (the first, the last and random ones) written as two duplicate triples
    (r, c, v) and (r, c, 1 - v), which add to ONE: rows of two entries and values != ONE, so it compiles to the general (CSR)
    form and not to one index per row."""
    out = list(triples)
    for k in sorted({0, len(triples) - 1} | set(rng.sample(range(len(triples)), splits)), reverse=True):
        r, c, one = out[k]
        assert one == 1
        v = rng.randrange(2, mod)
        out[k:k + 1] = [(r, c, v), (r, c, (1 - v) % mod)]
    return out


def run_perm_copy_constraints(lib, field, num_io, seed=4):
    """copy constraints through the harness Assembly -> construct_permutation_matrix, rows = 16, num_advice = 3"""
    mod, rng, dev = MODS[field], random.Random(seed + num_io), Dev(lib)
    k, rows, num_advice = 4, 16, 3
    N = num_io + rows * num_advice
    adv = lambda c: (PM.ADVICE, c)
    inst = (PM.INSTANCE, 0)
    # with an instance column the last advice column stays out of the permutation argument: fill_sparse_matrix's identity rows
    columns = [inst, adv(0), adv(1)] if num_io else [adv(0), adv(1), adv(2)]
    asm = PM.Assembly(rows, columns)
    head = inst if num_io else adv(2)
    asm.copy(head, 0, adv(0), 3); asm.copy(adv(0), 3, adv(1), 5)          # a 3-cycle: an instance cell and two advice cells
    asm.copy(adv(0), 7, adv(1), 7)                                         # a cycle that spans two advice columns
    for _ in range(12):
        (c1, r1), (c2, r2) = ((rng.choice(columns), rng.randrange(rows)) for _ in range(2))
        r1, r2 = (r % num_io if c == inst else r for c, r in ((c1, r1), (c2, r2)))
        asm.copy(c1, r1, c2, r2)
    triples = PM.construct_permutation_matrix(k, num_io, num_advice, asm)
    assert len(triples) == N and sorted(t[0] for t in triples) == list(range(N))       # one entry per row: the fast form
    # a Z that satisfies them: one value per cycle
    zcol = lambda c: c[1] + (1 if c[0] == PM.ADVICE and num_io else 0)
    Z = [rng.randrange(mod) for _ in range(N)]
    value = {}
    for ci, c in enumerate(columns):
        for r in range(rows):
            if c == inst and r >= num_io:
                continue
            Z[PM.cell_to_z_idx(zcol(c), r, rows, num_io)] = value.setdefault(asm.aux[ci][r], rng.randrange(mod))
    assert want_perm(triples, Z, mod) == (0, D.NONE)
    fast = D.PermutationMatrix(field, [(r, c) for r, c, _ in triples], N, lib=lib)
    ones = D.PermutationMatrix(field, triples, N, lib=lib)                            # explicit ONEs: still one entry of ONE per row
    split = as_csr(triples, rng, mod)                                                 # the same matrix as CSR
    general = D.PermutationMatrix(field, split, N, lib=lib)
    shuffled = list(split)
    rng.shuffle(shuffled)
    unordered = D.PermutationMatrix(field, shuffled, N, lib=lib)
    assert PM.matrix_multiply(split, Z, mod) == PM.matrix_multiply(triples, Z, mod)
    try:
        for pm in (fast, ones, general, unordered):
            assert device_perm(lib, field, pm, Z, num_io, dev) == (0, D.NONE)
        # break one cell of the 3-cycle: both neighbours' rows see it
        cell = PM.cell_to_z_idx(zcol(adv(0)), 3, rows, num_io)
        Zb = list(Z)
        Zb[cell] = (Zb[cell] + 1) % mod
        want = want_perm(triples, Zb, mod)
        assert want[0] == 2
        for pm in (fast, ones, general, unordered):
            assert device_perm(lib, field, pm, Zb, num_io, dev) == want
        # break c more cells, the instance cell and the last element among them
        for cell in [0, N - 1] + rng.sample(range(N), 5):
            Zb[cell] = (Zb[cell] + rng.randrange(1, mod)) % mod
        want = want_perm(triples, Zb, mod)
        assert want[0] >= 3
        for pm in (fast, ones, general, unordered):
            assert device_perm(lib, field, pm, Zb, num_io, dev) == want
        # num_io + n_w != N
        import pytest
        d_w = dev.put(ints_to_mont(Z[num_io:], mod))
        for bad_io, bad_nw in ((num_io, N - num_io - 1), (num_io + 1, N - num_io), (0, N + 1)):
            with pytest.raises(_lib.MiraError) as err:
                fast.check_device([0] * bad_io, d_w, bad_nw)
            assert err.value.code == _lib.MIRA_E_BAD_ARG
    finally:
        for pm in (fast, ones, general, unordered):
            pm.close()
        dev.free()


def run_perm_general(lib, field, seed=5):
    """matrix_multiply on arbitrary triples: a value != ONE, an empty row, a row with two entries, duplicate triples"""
    import pytest
    mod, rng, dev = MODS[field], random.Random(seed), Dev(lib)
    num_io, N = 2, 50
    v, a, b, c = (rng.randrange(2, mod) for _ in range(4))
    special = {3, 4, 8, 10, 11}
    triples = [(i, i, 1) for i in range(N) if i not in special]
    triples += [(3, 5, v), (4, 6, a), (4, 7, b), (8, 9, c), (8, 9, c)]               # rows 10 and 11 stay empty; (8, 9) twice
    rng.shuffle(triples)
    Z = [rng.randrange(mod) for _ in range(N)]
    Z[3], Z[4], Z[8], Z[10] = v * Z[5] % mod, (a * Z[6] + b * Z[7]) % mod, 2 * c * Z[9] % mod, 0
    pm = D.PermutationMatrix(field, triples, N, lib=lib)
    try:
        want = want_perm(triples, Z, mod)
        assert want == (1, 11)                                                      # the empty row 11 gives y = 0 != Z[11]
        assert device_perm(lib, field, pm, Z, num_io, dev) == want
        Z[11] = 0
        assert device_perm(lib, field, pm, Z, num_io, dev) == (0, D.NONE)
        for cell in (5, 7, 9, 1):                                                   # 5 -> row 3; 7 -> row 4; 9 -> row 8; 1 (instance, identity) -> none
            Z[cell] = (Z[cell] + 1) % mod
        want = want_perm(triples, Z, mod)
        assert want == (3, 3)
        assert device_perm(lib, field, pm, Z, num_io, dev) == want
        for bad in ([(0, N, 1)], [(N, 0, 1)], [(0, 0), (1, N)]):                      # "invalid matrix multiply"
            with pytest.raises(_lib.MiraError) as err:
                D.PermutationMatrix(field, bad, N, lib=lib)
            assert err.value.code == _lib.MIRA_E_BAD_ARG
    finally:
        pm.close()
        dev.free()


def run_perm_large(lib, field, grid=3, seed=6):
    """N = 1553 over three workgroups: disjoint 2- and 3-cycles, as one index per row and as CSR (entries split in two)"""
    mod, rng, dev = MODS[field], random.Random(seed), Dev(lib)
    num_io, N = 1, 1553
    order = list(range(N))
    rng.shuffle(order)
    sigma, Z, at = list(range(N)), [0] * N, 0
    while at < N:
        size = min(rng.choice([1, 2, 3]), N - at)
        cyc, val = order[at:at + size], rng.randrange(mod)
        for q, i in enumerate(cyc):
            sigma[i], Z[i] = cyc[(q + 1) % size], val
        at += size
    triples = [(i, sigma[i], 1) for i in range(N)]
    lib.tune(_lib.TUNE_DECIDE_GRID, grid)
    fast = D.PermutationMatrix(field, [(r, c) for r, c, _ in triples], N, lib=lib)
    general = D.PermutationMatrix(field, as_csr(triples, rng, mod, splits=40), N, lib=lib)
    try:
        for pm in (fast, general):
            assert device_perm(lib, field, pm, Z, num_io, dev) == (0, D.NONE)
        for cell in [0, N - 1, 767, 768, 1536] + rng.sample(range(N), 9):
            Z[cell] = (Z[cell] + 1) % mod
        want = want_perm(triples, Z, mod)
        assert want[0] >= 5
        for pm in (fast, general):
            assert device_perm(lib, field, pm, Z, num_io, dev) == want
    finally:
        lib.tune(_lib.TUNE_DECIDE_GRID, -1)
        fast.close(); general.close()
        dev.free()


# ---------------------------------------------------------------- graph_check
def run_graph_check(lib, field, specialize=False, seed=7):
    """mira_graph_check_compiled on a gate-sized graph over 2^5 rows.  e reads every column but the last advice column; that
    column is set to e's own value, so f = e - last vanishes on every row: a satisfied witness.
    specialize: the same through kernels of their own; returns the library's message when this machine has no run-time
    compiler, else None."""
    mod, rng, rows = MODS[field], random.Random(seed + field), 32
    nsel, nfix, nadv, nchal = 2, 2, 4, 2
    ncols = nsel + nfix + nadv
    ints, arrs = mock_data(field, rows, nsel, nfix, nadv, nchal, seed=seed * 31 + field)
    e = gate_like_expression(rng, 4, 4, ncols - 1, nchal)
    f = G.Sum(e, G.Negated(G.Polynomial(ncols - 1)))
    ev_e, ev_f = G.GraphEvaluator.new(e, field), G.GraphEvaluator.new(f, field)
    chal_m = ints_to_mont(ints["challenges"], mod)

    def oracle(ev, columns):
        code, consts, rots = ev.flatten()
        return C.graph_eval(field, code, ev.num_intermediates, consts, rots, columns, chal_m, rows)
    arrs["advice"][nadv - 1] = oracle(ev_e, oracle_columns(arrs))
    host_cols = oracle_columns(arrs)
    assert not oracle(ev_f, host_cols).any()
    if specialize:
        # only the column kinds matter to the compiler.  No run-time compiler on this machine: the caller skips with the
        # library's message; any other failure (these graphs are far below the length limit) is an error
        import ctypes
        kinds = [(None, G.COL_BOOL)] * nsel + [(None, G.COL_FIELD)] * (nfix + nadv)
        handles = (ctypes.c_uint64 * 2)(*[ev.compiled(nchal, ncols, lib) for ev in (ev_e, ev_f)])
        rc = lib.c.mira_graph_specialize(handles, 2, G.GraphEvaluator._column_table(kinds), ncols)
        if rc == _lib.MIRA_E_JIT_UNAVAILABLE:
            reason = (lib.c.mira_last_error() or b"").decode(errors="replace")
            ev_e.close(); ev_f.close()
            return reason
        lib.check(rc)
    ptrs, cols = [], []
    for s_ in arrs["selectors"]:
        p = lib.alloc(s_.nbytes); lib.upload(p, s_); ptrs.append(p); cols.append((p, G.COL_BOOL))
    for col in list(arrs["fixed"]) + list(arrs["advice"]):
        p = lib.alloc(col.nbytes); lib.upload(p, np.ascontiguousarray(col)); ptrs.append(p); cols.append((p, G.COL_FIELD))
    d_exp = lib.alloc(rows * 32); ptrs.append(d_exp)
    try:
        if specialize:
            assert ev_e.is_specialized(nchal, len(cols), lib=lib) and ev_f.is_specialized(nchal, len(cols), lib=lib)
        expected = host_cols[-1]
        lib.upload(d_exp, expected)
        assert ev_e.check_device(cols, ints["challenges"], rows, d_expected=d_exp, lib=lib) == (0, D.NONE)      # the evaluation itself
        r = rng.randrange(1, rows - 1)
        pert = expected.copy()
        for row in (0, 31, r):
            pert[row] = ints_to_mont([(mont_to_ints(pert[row:row + 1], mod)[0] + 1) % mod], mod)[0]
        lib.upload(d_exp, pert)
        assert ev_e.check_device(cols, ints["challenges"], rows, d_expected=d_exp, lib=lib) == (3, 0)
        assert ev_f.check_device(cols, ints["challenges"], rows, lib=lib) == (0, D.NONE)                        # d_expected = NULL, satisfied
        # one witness cell corrupted: the rows the oracle's walk finds (rotations may spread it)
        bad_row = rng.randrange(rows)
        for bad_col in range(nsel + nfix, ncols - 1):                                  # the first advice column the gate's value depends on
            corrupted = host_cols[bad_col].copy()
            corrupted[bad_row] = ints_to_mont([(mont_to_ints(corrupted[bad_row:bad_row + 1], mod)[0] + 12345) % mod], mod)[0]
            want_vals = oracle(ev_f, host_cols[:bad_col] + [corrupted] + host_cols[bad_col + 1:])
            bad_rows = [i for i in range(rows) if want_vals[i].any()]
            if bad_rows:
                break
        assert bad_rows
        lib.upload(cols[bad_col][0], corrupted)
        assert ev_f.check_device(cols, ints["challenges"], rows, lib=lib) == (len(bad_rows), bad_rows[0] if bad_rows else D.NONE)
        assert ev_f.check_device(cols, ints["challenges"], 0, lib=lib) == (0, D.NONE)                           # no rows: nothing to count
        return None
    finally:
        for p in ptrs:
            lib.free(p)
        ev_e.close(); ev_f.close()


# ---------------------------------------------------------------- end to end
def run_end_to_end(lib, field, seed=8):
    """is_sat on a trace of the reference's FiboCircuitWithLookup (2^5 rows), then one fold of the default accumulator with it
    and is_sat_relaxed on the folded pair -- each with the failures the reference reports.  field 1: bn256::Fr committed on
    BN256 G1, as the reference's test; field 0: the same circuit over Fq, committed on Grumpkin."""
    import pytest
    from lookup_fold_case import WIDTHS, DeviceTrace
    FIELD, MOD, CID = field, MODS[field], (0 if field == 1 else 1)
    log_rows, rng = 5, random.Random(seed)
    rows = 1 << log_rows
    seq = LK.get_sequence(1, 3, 2, 7)
    tr = LK.LookupTrace(log_rows, MOD, [rng.randrange(MOD) for _ in range(3)], seq=(seq[0], seq[1], seq[2], 7))
    cg, ctx, _, _ = LK.compressed_fibo_lookup()
    d = cg.degree
    c_ev = G.GraphEvaluator.new(cg.compressed, FIELD)
    f_ev = G.GraphEvaluator.new(cg.homogeneous, FIELD)
    add_only = G.GraphEvaluator.new(LK.fibo_lookup_gates()[0][0], FIELD)               # the addition gate alone: reads neither h nor g
    evs = [G.GraphEvaluator.new(t, FIELD) for t in cg.grouped.iter_from_first()]
    key = cm.CommitmentKey.synthetic(CID, 3 * rows, seed=0x4445 + log_rows, lib=lib)
    sel_host = [np.array(s, dtype=np.uint8) for s in tr.selectors]
    fix_host = ints_to_mont([v for col in tr.fixed for v in col], MOD).reshape(LK.NUM_FIXED, rows, 4)
    d_sel, d_fix = [], []
    for s in sel_host:
        p = lib.alloc(s.nbytes); lib.upload(p, s); d_sel.append(p)
    for fcol in fix_host:
        p = lib.alloc(fcol.nbytes); lib.upload(p, np.ascontiguousarray(fcol)); d_fix.append(p)
    lens = [n * rows for n in WIDTHS]
    lookup = (LK.NUM_LOOKUPS, True)
    # the shared DeviceTrace converts a trace's integers over Fr only: it is built empty and filled here, over either field
    acc, inc = DeviceTrace(lib, key, rows), DeviceTrace(lib, key, rows, None, tr.challenges, 1)
    inc.W_host = [ints_to_mont(w, MOD) for w in tr.W]
    for p, w in zip(inc.d_W, inc.W_host):
        lib.upload(p, w)
    inc.W_commits = np.stack([key.commit_device(p, len(w)) for p, w in zip(inc.d_W, inc.W_host)])
    poke = lambda p, i, v: lib.upload(p + i * 32, ints_to_mont([v % MOD], MOD))

    def oracle_rows(ev, trace, challenges, expected=None):
        """rows where the oracle's walk of ev over the trace's host vectors differs from `expected` (None: from zero)"""
        code, consts, rots = ev.flatten()
        flat = list(np.concatenate(trace.W_host).reshape(8, rows, 4))
        vals = C.graph_eval(FIELD, code, ev.num_intermediates, consts, rots, sel_host + list(fix_host) + flat + flat, ints_to_mont(challenges, MOD), rows)
        exp = np.zeros((rows, 4), dtype=np.uint64) if expected is None else expected
        return [i for i in range(rows) if (vals[i] != exp[i]).any()]
    try:
        dom = G.PlonkEvalDomain(LK.NUM_ADVICE, LK.NUM_LOOKUPS, tr.challenges, d_sel, d_fix, [(p, n) for p, n in zip(inc.d_W, lens)], [], rows)
        args = lambda ev=c_ev, commits=None: (key, ev, dom.columns(), tr.challenges, rows, inc.d_W, lens, inc.W_commits if commits is None else commits)
        assert oracle_rows(c_ev, inc, tr.challenges) == []
        D.is_sat_device(*args(), lookup=lookup, lib=lib)                                 # satisfied
        # an advice cell of an addition row
        row = tr.selectors[LK.S_ADD].index(True)
        good = tr.advice[0][row]
        inc.W_host[0][row] = ints_to_mont([(good + 1) % MOD], MOD)[0]
        poke(inc.d_W[0], row, good + 1)
        bad = oracle_rows(c_ev, inc, tr.challenges)
        assert bad == [row]
        with pytest.raises(D.EvaluationMismatch) as err:
            D.is_sat_device(*args(), lookup=lookup, lib=lib)
        assert (err.value.mismatch_count, err.value.total_row, err.value.first_row) == (len(bad), rows, bad[0])
        inc.W_host[0][row] = ints_to_mont([good], MOD)[0]
        poke(inc.d_W[0], row, good)
        D.is_sat_device(*args(), lookup=lookup, lib=lib)
        # an h cell: the sums differ -- and the gate h (l + r) - 1 reads h, so the evaluation check fires first
        hrow, good = 9, tr.lookup["h"][9]
        inc.W_host[2][hrow] = ints_to_mont([(good + 1) % MOD], MOD)[0]
        poke(inc.d_W[2], hrow, good + 1)
        assert not D.is_sat_log_derivative_device(FIELD, inc.d_W, rows, LK.NUM_LOOKUPS, True, lib=lib)
        bad = oracle_rows(c_ev, inc, tr.challenges)
        assert bad == [hrow]
        with pytest.raises(D.EvaluationMismatch) as err:
            D.is_sat_device(*args(), lookup=lookup, lib=lib)
        assert (err.value.mismatch_count, err.value.total_row, err.value.first_row) == (1, rows, hrow)
        with pytest.raises(D.LogDerivativeNotSat):                                       # a gate that does not read h: only the sums differ
            D.is_sat_device(*args(ev=add_only), lookup=lookup, lib=lib)
        inc.W_host[2][hrow] = ints_to_mont([good], MOD)[0]
        poke(inc.d_W[2], hrow, good)
        assert D.is_sat_log_derivative_device(FIELD, inc.d_W, rows, LK.NUM_LOOKUPS, True, lib=lib)
        # a commitment
        commits = inc.W_commits.copy()
        commits[1] = commits[0]
        with pytest.raises(D.CommitmentMismatch) as err:
            D.is_sat_device(*args(commits=commits), lookup=lookup, lib=lib)
        assert err.value.mismatch_count == 1
        D.is_sat_device(*args(), lookup=lookup, lib=lib)

        # ---- one fold of the default accumulator with the trace (tests/lookup_fold_case.py has every step checked)
        chal = acc.challenges + [acc.u] + inc.challenges + [inc.u]
        dom2 = G.PlonkEvalDomain(LK.NUM_ADVICE, LK.NUM_LOOKUPS, chal, d_sel, d_fix, [(p, n) for p, n in zip(acc.d_W, lens)], [(p, n) for p, n in zip(inc.d_W, lens)], rows)
        d_terms, commits = G.commit_cross_terms(key, evs, dom2, lib=lib)
        try:
            r = rng.randrange(MOD)
            r_m = ints_to_mont([r], MOD)[0]
            for i, n in enumerate(lens):
                FD.fold_witness_device(FIELD, acc.d_W[i], acc.d_W[i], inc.d_W[i], r_m, n, lib=lib)
            FD.fold_error_device(FIELD, acc.d_E, [d_terms + t * rows * 32 for t in range(d)], r_m, rows, lib=lib)
            new_wc, new_ec = FD.fold_instance_commitments(CID, acc.W_commits, inc.W_commits, r_m, acc.E_commit, commits, lib=lib)
        finally:
            lib.free(d_terms)
        acc.W_commits, acc.E_commit = np.asarray(new_wc), np.asarray(new_ec)
        acc.challenges = [(a + r * b) % MOD for a, b in zip(acc.challenges, inc.challenges)]
        acc.u = (acc.u + r) % MOD
        acc.W_host = [lib.download(p, (n, 4)) for p, n in zip(acc.d_W, lens)]
        acc.E_host = lib.download(acc.d_E, (rows, 4))
        chal_f = acc.challenges + [acc.u]
        dom_f = G.PlonkEvalDomain(LK.NUM_ADVICE, LK.NUM_LOOKUPS, chal_f, d_sel, d_fix, [(p, n) for p, n in zip(acc.d_W, lens)], [], rows)
        rargs = lambda e_commit=None: (key, f_ev, dom_f.columns(), chal_f, rows, acc.d_W, lens, acc.W_commits, acc.d_E, acc.E_commit if e_commit is None else e_commit)
        assert oracle_rows(f_ev, acc, chal_f, acc.E_host) == []
        D.is_sat_relaxed_device(*rargs(), lookup=lookup, lib=lib)
        erow = 17
        good = mont_to_ints(acc.E_host[erow:erow + 1], MOD)[0]
        poke(acc.d_E, erow, good + 1)
        with pytest.raises(D.EvaluationMismatch) as err:
            D.is_sat_relaxed_device(*rargs(), lookup=lookup, lib=lib)
        assert (err.value.mismatch_count, err.value.total_row, err.value.first_row) == (1, 32, erow)
        poke(acc.d_E, erow, good)
        with pytest.raises(D.ECommitmentMismatch):
            D.is_sat_relaxed_device(*rargs(e_commit=acc.W_commits[0]), lookup=lookup, lib=lib)
        commits = acc.W_commits.copy()
        commits[0], commits[2] = commits[2].copy(), commits[0].copy()
        with pytest.raises(D.CommitmentMismatch) as err:
            D.is_sat_relaxed_device(key, f_ev, dom_f.columns(), chal_f, rows, acc.d_W, lens, commits, acc.d_E, acc.E_commit, lookup=lookup, lib=lib)
        assert err.value.mismatch_count == 2
        D.is_sat_relaxed_device(*rargs(), lookup=lookup, lib=lib)
    finally:
        acc.free(); inc.free()
        for p in d_sel + d_fix:
            lib.free(p)
        for ev in evs + [c_ev, f_ev, add_only]:
            ev.close()
        key.close()
