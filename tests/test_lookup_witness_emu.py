"""The lookup argument's witness rounds on the CPU emulation of the kernels: mira_lookup_m_device, mira_lookup_h_g_device and
mira_batch_invert_device against a Python restatement of evaluate_m / evaluate_h_g (src/plonk/lookup.rs:278-321)."""
import ctypes
import random
from collections import Counter

import numpy as np
import pytest

from helpers import ints_to_mont, mont_to_ints
from mira_amd import _lib
from mira_amd import lookup as LU
from mira_amd.graph_evaluator import MODULUS

FIELDS = [LU.FIELD_FQ, LU.FIELD_FR]


# ---- the reference, restated ------------------------------------------------------------------------------------------------
def ref_m(l, t):
    """evaluate_m: counts of l per value, given at the first occurrence of the value in t"""
    counts, seen, m = Counter(l), set(), []
    for v in t:
        m.append(0 if v in seen else counts.get(v, 0))
        seen.add(v)
    return m


def ref_h_g(l, t, m, r, mod):
    inv = lambda v: pow(v, mod - 2, mod) if v % mod else 0
    return [inv((v + r) % mod) for v in l], [mv * inv((tv + r) % mod) % mod for mv, tv in zip(m, t)]


# ---- device plumbing --------------------------------------------------------------------------------------------------------
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

    def empty(self, n):
        return self.put(np.full((n, 4), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64))

    def get(self, p, n):
        return self.lib.download(p, (n, 4)) if n else np.zeros((0, 4), dtype=np.uint64)

    def free(self):
        for p in self.ptrs:
            self.lib.free(p)


@pytest.fixture
def dev(emu_lib):
    d = Dev(emu_lib)
    yield d
    d.free()
    emu_lib.tune(_lib.TUNE_LOOKUP_HASH, -1)
    emu_lib.tune(_lib.TUNE_INV_CHUNK, -1)


def run_m(dev, field, l_raw, t_raw):
    n_l, n_t = len(l_raw), len(t_raw)
    d_l, d_t, d_m = dev.put(l_raw), dev.put(t_raw), dev.empty(n_t)
    LU.evaluate_m_device(field, d_m, d_l, n_l, d_t, n_t, lib=dev.lib)
    return dev.get(d_m, n_t)


def run_h_g(dev, field, l_raw, t_raw, m_raw, r):
    n_l, n_t = len(l_raw), len(t_raw)
    d_l, d_t, d_m, d_h, d_g = dev.put(l_raw), dev.put(t_raw), dev.put(m_raw), dev.empty(n_l), dev.empty(n_t)
    LU.evaluate_h_g_device(field, d_h, d_g, d_l, n_l, d_t, d_m, n_t, r, lib=dev.lib)
    return dev.get(d_h, n_l), dev.get(d_g, n_t)


def lookup_case(rng, mod, n_l, n_t, distinct):
    """t: `distinct` values (some repeated, in random places), l: mostly values of t, some absent from it"""
    pool = [rng.randrange(mod) for _ in range(max(1, distinct))] + [0]
    t = [rng.choice(pool) for _ in range(n_t)]
    absent = [rng.randrange(mod) for _ in range(3)]
    l = [rng.choice(t) if t and rng.random() < 0.85 else rng.choice(absent + [0]) for _ in range(n_l)]
    return l, t


# ---- m ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("n_l,n_t,distinct", [(1, 1, 1), (0, 5, 3), (7, 13, 4), (13, 7, 7), (301, 257, 40), (1000, 999, 999), (2049, 64, 25)])
def test_m_matches_reference(dev, field, n_l, n_t, distinct):
    mod, rng = MODULUS[field], random.Random(field * 1000 + n_l * 7 + n_t)
    l, t = lookup_case(rng, mod, n_l, n_t, distinct)
    got = run_m(dev, field, ints_to_mont(l, mod), ints_to_mont(t, mod))
    assert mont_to_ints(got, mod) == ref_m(l, t)
    assert (got == ints_to_mont(ref_m(l, t), mod)).all()                       # canonical Montgomery bytes


@pytest.mark.parametrize("field", FIELDS)
def test_m_reference_circuit_shape(dev, field):
    """the reference circuit's table column: 25 values then zeros; most l are 0"""
    mod, rng = MODULUS[field], random.Random(0x25 + field)
    table = [rng.randrange(mod) for _ in range(25)]
    t = table + [0] * (1024 - 25)
    l = [0 if rng.random() < 0.8 else rng.choice(table) for _ in range(1024)]
    got = run_m(dev, field, ints_to_mont(l, mod), ints_to_mont(t, mod))
    want = ref_m(l, t)
    assert mont_to_ints(got, mod) == want
    assert want[25] == l.count(0) and all(v == 0 for v in want[26:])            # only the first zero carries the count


@pytest.mark.parametrize("field", FIELDS)
def test_m_hash_mode_one_same_bytes(dev, field):
    """every key probing from slot 0 (long chains) gives the same bytes as the hashed table"""
    mod, rng = MODULUS[field], random.Random(0x51 + field)
    l, t = lookup_case(rng, mod, 700, 500, 120)
    lm, tm = ints_to_mont(l, mod), ints_to_mont(t, mod)
    hashed = run_m(dev, field, lm, tm)
    dev.lib.tune(_lib.TUNE_LOOKUP_HASH, 1)
    linear = run_m(dev, field, lm, tm)
    assert (hashed == linear).all()
    assert mont_to_ints(linear, mod) == ref_m(l, t)


@pytest.mark.parametrize("field", FIELDS)
def test_m_keys_differ_in_top_word_only(dev, field):
    mod = MODULUS[field]
    base = ints_to_mont([123456789], mod)[0]
    rows = []
    for top in range(8):
        r = base.copy()
        r[3] = np.uint64(top)                                               # < the modulus' top word: canonical
        rows.append(r)
    t_raw = np.array(rows + rows[:3], dtype=np.uint64)
    l_raw = np.array([rows[k % 8] for k in range(37)] + [rows[0]] * 5, dtype=np.uint64)
    t, l = mont_to_ints(t_raw, mod), mont_to_ints(l_raw, mod)
    assert len(set(t)) == 8
    for mode in (-1, 1):
        dev.lib.tune(_lib.TUNE_LOOKUP_HASH, mode)
        assert mont_to_ints(run_m(dev, field, l_raw, t_raw), mod) == ref_m(l, t)


# ---- h, g ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("n_l,n_t", [(1, 1), (0, 3), (3, 0), (17, 9), (9, 17), (600, 451)])
def test_h_g_matches_reference(dev, field, n_l, n_t):
    mod, rng = MODULUS[field], random.Random(0x4867 + field + 3 * n_l + n_t)
    l, t = lookup_case(rng, mod, n_l, n_t, max(1, n_t // 3))
    r = rng.randrange(mod)
    # zero denominators on both sides: l_i = t_j = -r on some rows
    for i in range(0, n_l, 5):
        l[i] = (mod - r) % mod
    for i in range(1, n_t, 4):
        t[i] = (mod - r) % mod
    m = ref_m(l, t)
    h, g = run_h_g(dev, field, ints_to_mont(l, mod), ints_to_mont(t, mod), ints_to_mont(m, mod), r)
    want_h, want_g = ref_h_g(l, t, m, r, mod)
    assert (h == ints_to_mont(want_h, mod).reshape(-1, 4)).all()
    assert (g == ints_to_mont(want_g, mod).reshape(-1, 4)).all()


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("chunk", [2, 3, 5])
def test_h_g_levels_and_chunks(dev, field, chunk):
    """several levels of the inversion tree (elements per lane set low), zeros inside lanes' chunks"""
    mod, rng = MODULUS[field], random.Random(0x1E7 + chunk + field)
    dev.lib.tune(_lib.TUNE_INV_CHUNK, chunk)
    n = 2600
    l, t = lookup_case(rng, mod, n, n - 7, 300)
    r = rng.randrange(mod)
    for i in rng.sample(range(n), 200):
        l[i] = (mod - r) % mod
    m = ref_m(l, t)
    h, g = run_h_g(dev, field, ints_to_mont(l, mod), ints_to_mont(t, mod), ints_to_mont(m, mod), r)
    want_h, want_g = ref_h_g(l, t, m, r, mod)
    assert mont_to_ints(h, mod) == want_h and mont_to_ints(g, mod) == want_g


# ---- batch inversion ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("n,chunk", [(1, -1), (2, -1), (5, 2), (255, -1), (2048, -1), (2049, -1), (3001, 2), (4097, 3), (1500, 64)])
def test_batch_invert(dev, field, n, chunk):
    mod, rng = MODULUS[field], random.Random(0xB1 + n + field)
    dev.lib.tune(_lib.TUNE_INV_CHUNK, chunk)
    x = [rng.randrange(mod) if rng.random() < 0.8 else 0 for _ in range(n)]
    x[0] = 0 if n > 3 else x[0]
    d_in, d_out = dev.put(ints_to_mont(x, mod)), dev.empty(n)
    LU.batch_invert_device(field, d_out, d_in, n, lib=dev.lib)
    want = ints_to_mont([pow(v, mod - 2, mod) if v else 0 for v in x], mod)
    assert (dev.get(d_out, n) == want).all()
    assert (dev.get(d_in, n) == ints_to_mont(x, mod)).all()                      # the input is left alone
    LU.batch_invert_device(field, d_in, d_in, n, lib=dev.lib)                   # in place
    assert (dev.get(d_in, n) == want).all()


@pytest.mark.parametrize("field", FIELDS)
def test_batch_invert_all_zero_and_one(dev, field):
    mod = MODULUS[field]
    for vals in ([0] * 9, [1] * 9, [mod - 1] * 3):
        d = dev.put(ints_to_mont(vals, mod))
        LU.batch_invert_device(field, d, d, len(vals), lib=dev.lib)
        assert mont_to_ints(dev.get(d, len(vals)), mod) == [pow(v, mod - 2, mod) if v else 0 for v in vals]


# ---- determinism, arguments, workspaces ---------------------------------------------------------------------------------------
def test_two_runs_identical_bytes(dev):
    field, mod, rng = LU.FIELD_FR, MODULUS[LU.FIELD_FR], random.Random(0xD7)
    l, t = lookup_case(rng, mod, 900, 800, 100)
    lm, tm = ints_to_mont(l, mod), ints_to_mont(t, mod)
    m1, m2 = run_m(dev, field, lm, tm), run_m(dev, field, lm, tm)
    assert (m1 == m2).all()
    a, b = run_h_g(dev, field, lm, tm, m1, 5), run_h_g(dev, field, lm, tm, m1, 5)
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all()


@pytest.mark.parametrize("field", FIELDS)
def test_non_canonical_input_is_bad_arg(dev, field):
    mod, lib = MODULUS[field], dev.lib
    good = ints_to_mont([1, 2, 3, 4, 5], mod)
    bad = good.copy()
    bad[2] = [(mod >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)]       # exactly the modulus
    for l_raw, t_raw in ((bad, good), (good, bad)):
        with pytest.raises(_lib.MiraError) as e:
            run_m(dev, field, l_raw, t_raw)
        assert e.value.code == _lib.MIRA_E_BAD_ARG
        with pytest.raises(_lib.MiraError) as e:
            run_h_g(dev, field, l_raw, t_raw, good, 7)
        assert e.value.code == _lib.MIRA_E_BAD_ARG
    with pytest.raises(_lib.MiraError) as e:
        run_h_g(dev, field, good, good, bad, 7)                                 # m
    assert e.value.code == _lib.MIRA_E_BAD_ARG
    d = dev.put(bad)
    assert lib.c.mira_batch_invert_device(field, ctypes.c_void_p(d), ctypes.c_void_p(d), 5) == _lib.MIRA_E_BAD_ARG
    rm = np.array([(mod >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)], dtype=np.uint64)   # r = p
    dg = dev.put(good)
    dh, dgg = dev.empty(5), dev.empty(5)
    assert lib.c.mira_lookup_h_g_device(field, ctypes.c_void_p(dh), ctypes.c_void_p(dgg), ctypes.c_void_p(dg), 5, ctypes.c_void_p(dg),
                                        ctypes.c_void_p(dg), 5, rm.ctypes.data_as(ctypes.c_void_p)) == _lib.MIRA_E_BAD_ARG
    # and the library still works afterwards
    assert mont_to_ints(run_m(dev, field, good, good), mod) == [1] * 5


def test_argument_checks(dev):
    lib, c, vp = dev.lib, dev.lib.c, ctypes.c_void_p
    mod = MODULUS[LU.FIELD_FR]
    buf = dev.put(ints_to_mont(list(range(1, 33)), mod))                      # 32 elements
    r = ints_to_mont([3], mod)[0]
    rp = r.ctypes.data_as(vp)
    at = lambda k: vp(buf + 32 * k)
    BAD, UNS = _lib.MIRA_E_BAD_ARG, _lib.MIRA_E_UNSUPPORTED
    # n = 0 is a no-op, null pointers included
    assert c.mira_batch_invert_device(1, None, None, 0) == 0
    assert c.mira_lookup_m_device(1, None, None, 5, None, 0) == 0
    assert c.mira_lookup_h_g_device(1, None, None, None, 0, None, None, 0, rp) == 0
    # unknown field, null pointers
    assert c.mira_batch_invert_device(2, at(0), at(0), 4) == BAD
    assert c.mira_lookup_m_device(-1, at(8), at(0), 4, at(4), 4) == BAD
    assert c.mira_batch_invert_device(1, None, at(0), 4) == BAD
    assert c.mira_lookup_m_device(1, at(8), None, 4, at(4), 4) == BAD
    assert c.mira_lookup_m_device(1, None, at(0), 4, at(4), 4) == BAD
    assert c.mira_lookup_h_g_device(1, at(16), at(20), at(0), 4, at(4), None, 4, rp) == BAD
    assert c.mira_lookup_h_g_device(1, at(16), at(20), at(0), 4, at(4), at(8), 4, None) == BAD
    # overlapping outputs
    assert c.mira_batch_invert_device(1, at(1), at(0), 4) == BAD
    assert c.mira_lookup_m_device(1, at(3), at(0), 4, at(8), 4) == BAD
    assert c.mira_lookup_m_device(1, at(10), at(0), 4, at(8), 4) == BAD
    assert c.mira_lookup_h_g_device(1, at(2), at(20), at(0), 4, at(4), at(8), 4, rp) == BAD     # h over l
    assert c.mira_lookup_h_g_device(1, at(16), at(7), at(0), 4, at(4), at(8), 4, rp) == BAD     # g over t / m
    assert c.mira_lookup_h_g_device(1, at(16), at(18), at(0), 4, at(4), at(8), 4, rp) == BAD    # h over g
    # 2^32 elements or more
    assert c.mira_batch_invert_device(1, at(0), at(0), 1 << 32) == UNS
    assert c.mira_lookup_m_device(1, at(8), at(0), 1 << 32, at(4), 4) == UNS
    assert c.mira_lookup_h_g_device(1, at(16), at(20), at(0), 4, at(4), at(8), 1 << 32, rp) == UNS
    # a non-overlapping call on the same buffer goes through
    assert c.mira_lookup_h_g_device(1, at(16), at(20), at(0), 4, at(4), at(8), 4, rp) == 0


def test_stage_timers_and_trim(dev):
    lib = dev.lib
    field, mod = LU.FIELD_FQ, MODULUS[LU.FIELD_FQ]
    lib.check(lib.c.mira_set_timing(1))
    try:
        lm = ints_to_mont(list(range(100)), mod)
        m = run_m(dev, field, lm, lm)
        assert [n for n, _ in lib.timings()] == ["lookup_m"]
        run_h_g(dev, field, lm, lm, m, 1)
        assert [n for n, _ in lib.timings()] == ["lookup_h_g"]
        d = dev.put(lm)
        LU.batch_invert_device(field, d, d, 100, lib=lib)
        assert [n for n, _ in lib.timings()] == ["batch_invert"]
    finally:
        lib.check(lib.c.mira_set_timing(0))
    lib.trim(0)
    assert lib.trim(0) == 0
    assert mont_to_ints(run_m(dev, field, ints_to_mont([4, 4], mod), ints_to_mont([4, 4], mod)), mod) == [2, 0]   # workspaces come back
