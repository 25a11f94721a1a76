"""-m gpu: the lookup argument's witness rounds on the device -- m (evaluate_m), h and g (evaluate_h_g) and the batch inversion
under them (src/plonk/lookup.rs:278-366).

* FiboCircuitWithLookup (the reference's circuit at its own 2^5 rows, synthetic traces at 2^13 and 2^16): l and t from the
  compiled L / T graphs, then m, h, g, all through `LookupArguments` on the device -- W2 = l | t | m and W3 = h | g equal the
  host trace's vectors bit for bit, and so do their commitments (the oracle's MSM over the harness vectors);
* direct calls at 2^20 and 2^22 rows, distinct and duplicate-heavy inputs, both fields: m against a count on the host, h and g
  exactly on sampled rows, sum h = sum g, and a second run byte-identical."""
import random

import numpy as np
import pytest

from helpers import ints_to_mont, mont_to_ints
from harness import graph_evaluator as G
from harness import lookup as LK
from mira_amd import commitment as cm
from mira_amd import lookup as LU
from mira_amd.graph_evaluator import MODULUS
from oracle import cref as C
from oracle import pyref as P

pytestmark = pytest.mark.gpu

FIELD, CID, MOD = LU.FIELD_FR, cm.CURVE_BN256, P.R_MOD


@pytest.mark.parametrize("k", [5, 13, 16])
def test_lookup_arguments_match_host_trace(gpu_lib, k):
    lib, rows = gpu_lib, 1 << k
    rng = random.Random(0x700 + k)
    chal = [rng.randrange(MOD) for _ in range(3)]
    if k == 5:
        seq = LK.get_sequence(1, 3, 2, 7)
        tr = LK.LookupTrace(k, MOD, chal, seq=(seq[0], seq[1], seq[2], 7))
    else:
        tr = LK.LookupTrace(k, MOD, chal, seed=0x900 + k)
    _, _, L, T = LK.fibo_lookup_gates()
    args = LU.LookupArguments(FIELD, [G.GraphEvaluator.new(L, FIELD)], [G.GraphEvaluator.new(T, FIELD)])
    ptrs = []

    def put(arr):
        p = lib.alloc(max(32, arr.nbytes)); lib.upload(p, arr); ptrs.append(p)
        return p
    try:
        d_sel = [put(np.array(s, dtype=np.uint8)) for s in tr.selectors]
        d_fix = [put(ints_to_mont(col, MOD)) for col in tr.fixed]
        d_w1 = put(ints_to_mont(tr.W[0], MOD))
        d_w2, d_w3 = put(np.zeros((3 * rows, 4), dtype=np.uint64)), put(np.zeros((2 * rows, 4), dtype=np.uint64))
        dom = LU.LookupEvalDomain(d_sel, d_fix, [d_w1 + c * rows * 32 for c in range(LK.NUM_ADVICE)])
        args.evaluate_coefficient_1_device(dom, chal[0], rows, d_w2, lib=lib)            # round 2: r1 compresses the vector lookup
        args.evaluate_coefficient_2_device(d_w2, chal[1], rows, d_w3, lib=lib)           # round 3: r2 is the log-derivative point
        want2, want3 = ints_to_mont(tr.W[1], MOD), ints_to_mont(tr.W[2], MOD)
        got2, got3 = lib.download(d_w2, (3 * rows, 4)), lib.download(d_w3, (2 * rows, 4))
        assert (got2 == want2).all()
        assert (got3 == want3).all()
        key = cm.CommitmentKey.synthetic(CID, 3 * rows, seed=0x4C57 + k, lib=lib)
        try:
            bases = key.download()
            assert (key.commit_device(d_w2, 3 * rows) == C.commit(CID, bases, want2)).all()
            assert (key.commit_device(d_w3, 2 * rows) == C.commit(CID, bases[:2 * rows], want3)).all()
        finally:
            key.close()
    finally:
        for p in ptrs:
            lib.free(p)
        for ev in args.lookup_evaluators + args.table_evaluators:
            ev.close()


# ---- direct calls at scale ----------------------------------------------------------------------------------------------------
def rand_canonical(rng, n, mod):
    """n uniformly drawn canonical representations (the top word below the modulus' top word)"""
    a = rng.integers(0, 2 ** 63, size=(n, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(n, 4), dtype=np.uint64)
    a[:, 3] = rng.integers(0, mod >> 192, size=n, dtype=np.uint64)
    return a


def rep_sum(arr, mod):
    """sum of the representations mod p (= R * sum of the values: enough to compare two sums)"""
    a = np.ascontiguousarray(arr, dtype=np.uint64).view(np.uint32).reshape(-1, 8).astype(np.uint64)
    return sum(int(c) << (32 * k) for k, c in enumerate(a.sum(axis=0))) % mod


def mont_small(c, mod):
    return ints_to_mont([c], mod)[0]


@pytest.mark.parametrize("field", [LU.FIELD_FQ, LU.FIELD_FR])
@pytest.mark.parametrize("log_n", [20, 22])
@pytest.mark.parametrize("shape", ["distinct", "duplicates"])
def test_m_h_g_at_scale(gpu_lib, field, log_n, shape):
    lib, n, mod = gpu_lib, 1 << log_n, MODULUS[field]
    rng = np.random.default_rng(log_n * 10 + field + (100 if shape == "duplicates" else 0))
    if shape == "distinct":
        t = rand_canonical(rng, n, mod)                                       # distinct (collisions: probability ~2^-200)
        pick = rng.integers(0, n, size=n)
        l = t[pick]
        counts = np.bincount(pick, minlength=n)
        table = np.stack([mont_small(c, mod) for c in range(int(counts.max()) + 1)])
        want_m = table[counts]
    else:                                                                     # the reference circuit's table: 25 values + zeros
        t = np.zeros((n, 4), dtype=np.uint64)
        t[:25] = rand_canonical(rng, 25, mod)
        l = np.repeat(t[3:4], n, axis=0)
        want_m = np.zeros((n, 4), dtype=np.uint64)
        want_m[3] = mont_small(n, mod)
    r = int(random.Random(log_n + field).randrange(mod))
    ptrs = []

    def put(arr):
        p = lib.alloc(arr.nbytes); lib.upload(p, arr); ptrs.append(p)
        return p
    try:
        d_l, d_t = put(l), put(t)
        d_m, d_h, d_g = (put(np.zeros((n, 4), dtype=np.uint64)) for _ in range(3))
        outs = []
        for _ in range(2):
            LU.evaluate_m_device(field, d_m, d_l, n, d_t, n, lib=lib)
            LU.evaluate_h_g_device(field, d_h, d_g, d_l, n, d_t, d_m, n, r, lib=lib)
            outs.append([lib.download(p, (n, 4)) for p in (d_m, d_h, d_g)])
        m, h, g = outs[0]
        assert all((a == b).all() for a, b in zip(outs[0], outs[1]))             # byte-identical second run
        assert (m == want_m).all()
        sample = random.Random(n).sample(range(n), 4096) + [0, 3, 24, 25, n - 1]
        l_i, t_i, m_i = mont_to_ints(l[sample], mod), mont_to_ints(t[sample], mod), mont_to_ints(m[sample], mod)
        inv = lambda v: pow(v, mod - 2, mod) if v % mod else 0
        assert (h[sample] == ints_to_mont([inv((v + r) % mod) for v in l_i], mod)).all()
        assert (g[sample] == ints_to_mont([mv * inv((tv + r) % mod) % mod for mv, tv in zip(m_i, t_i)], mod)).all()
        assert rep_sum(h, mod) == rep_sum(g, mod)                                 # every l is in t: sum h = sum g
    finally:
        for p in ptrs:
            lib.free(p)


@pytest.mark.parametrize("field", [LU.FIELD_FQ, LU.FIELD_FR])
def test_batch_invert_at_scale(gpu_lib, field):
    lib, n, mod = gpu_lib, (1 << 20) + 3, MODULUS[field]
    rng = np.random.default_rng(0xB1 + field)
    x = rand_canonical(rng, n, mod)
    x[rng.integers(0, n, size=1000)] = 0
    d = lib.alloc(x.nbytes)
    d_out = lib.alloc(x.nbytes)
    try:
        lib.upload(d, x)
        LU.batch_invert_device(field, d_out, d, n, lib=lib)
        LU.batch_invert_device(field, d, d, n, lib=lib)                       # in place
        out, inplace = lib.download(d_out, (n, 4)), lib.download(d, (n, 4))
        assert (out == inplace).all()
        sample = random.Random(field).sample(range(n), 4096)
        xs = mont_to_ints(x[sample], mod)
        assert (out[sample] == ints_to_mont([pow(v, mod - 2, mod) if v else 0 for v in xs], mod)).all()
        assert (out[(x == 0).all(axis=1)] == 0).all()
    finally:
        lib.free(d)
        lib.free(d_out)
