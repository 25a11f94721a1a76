"""Wave groups and colliding hashes in the lookup multiplicities (csrc/lookup_kernels.cuh: k_lk_insert, k_lk_count; csrc/platform.h:
wave_group_leader, wave_shfl_u64).

On the device the lanes of a wave that hold one value are grouped by the 64-bit lk_hash of the value's eight stored words: the
group's lowest lane probes the table, the others take its slot after comparing their key with its element, and a lane whose key
differs from its leader's -- two values of one hash -- probes for itself.  Random keys never meet that branch (2^-64 a pair), and
the CPU emulation replaces the whole grouping by "every lane leads a group of one".  This module builds what reaches it:

    colliding_pairs()     distinct canonical keys of EQUAL lk_hash, found from a fixed seed by a birthday search.  Every step of the
                          hash, h = (h ^ word) * K; h ^= h >> 31, is a bijection of the state for a fixed word, and the word enters by
                          XOR: two 7-word prefixes whose states agree in their top 35 bits are completed by top words 0 and
                          s ^ s' < 2^29 (canonical: the moduli's top words are 0x30644e72), after which the states are equal.
                          2^21 prefixes give about 2^42 / 2^36 = 64 such pairs; nothing is stored as data.
    pair_cases()          the two keys of a pair in adjacent lanes, in two waves of a workgroup, in two workgroups; each repeated
                          within its wave in both orders (the hash group's leader holds A, the lower index of B sits in a later
                          lane, and the reverse); both counted in l with different counts; one of them absent from t and present
                          in l, which must count nowhere
    structure_cases()     t per wave: 64 equal values, 64 distinct ones, two alternating, groups of sizes 1, 2, 3 ... interleaved, a
                          value whose first occurrence is a late lane of wave 0 while an early lane of workgroup 1 holds it too,
                          at n_t = 1, 63, 65, 257, 4099 (tail waves run with part of the exec mask off); every third l absent from
                          t, so that lanes of k_lk_count leave before the ballot
    count_cases()         130 distinct hot values inside the first workgroup's 256 elements of l (more than the 64 entries of the
                          workgroup's LDS table: by pigeonhole slots collide there and the counts go straight to HBM), and one l of
                          2048 * 256 + 100 elements (the grid-stride loop's second, partial trip) with a value that every
                          workgroup counts

Keys are STORED representations (4 x u64, what the kernels hash and compare); the expected m is ref_m of
test_lookup_witness_emu.py (a Counter) over them, h and g are ref_h_g over their values.  Every case runs twice under each hash
mode with byte-identical m.  The emulation runs the same cases: the probe chains of equal-hash keys are real there, the groups
are not -- a non-leader that took its leader's slot without comparing keys cannot be seen there, only on the device."""
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
from mira_amd import lookup as LU                                            # noqa: E402
from mira_amd.graph_evaluator import MODULUS                                 # noqa: E402

M64 = (1 << 64) - 1
HASH_SEED, HASH_MUL = 0x9E3779B97F4A7C15, 0xFF51AFD7ED558CCD
SMALL = 4099                                            # up to here a case also runs with every key probing from slot 0
N_T = (1, 63, 65, 257, 4099)
BIG_N_L = 2048 * 256 + 100


# ---- lk_hash, restated ----------------------------------------------------------------------------------------------------------
def lk_hash(rep):
    """the hash of a stored representation: its eight 32-bit words, lowest first"""
    h = HASH_SEED
    for i in range(8):
        h = ((h ^ ((rep >> (32 * i)) & 0xFFFFFFFF)) * HASH_MUL) & M64
        h ^= h >> 31
    return h


def _states(words):
    """the state after the words of every row, (n, k) uint32 -> (n,) uint64 (numpy's uint64 product wraps like the kernel's)"""
    h = np.full(len(words), HASH_SEED, dtype=np.uint64)
    mul = np.uint64(HASH_MUL)
    with np.errstate(over="ignore"):
        for i in range(words.shape[1]):
            h = (h ^ words[:, i].astype(np.uint64)) * mul
            h ^= h >> np.uint64(31)
    return h


_pairs = None


def colliding_pairs(want=8, seed=0x10C0, draws=1 << 21):
    """-> at least `want` pairs (a, b) of stored representations: a != b, both below 2^253 (canonical in both fields), lk_hash equal"""
    global _pairs
    if _pairs is None:
        words = np.random.RandomState(seed).randint(0, 1 << 32, size=(draws, 7), dtype=np.uint64).astype(np.uint32)
        s = _states(words)
        order = np.argsort(s >> np.uint64(29), kind="stable")
        top = (s >> np.uint64(29))[order]
        out = []
        for k in np.nonzero(top[1:] == top[:-1])[0]:
            i, j = int(order[k]), int(order[k + 1])
            if (words[i] == words[j]).all():
                continue
            low = lambda r: sum(int(w) << (32 * q) for q, w in enumerate(words[r]))
            a, b = low(i), low(j) | ((int(s[i]) ^ int(s[j])) << 224)
            out.append((a, b))
        _pairs = out
    assert len(_pairs) >= want, f"the search gave {len(_pairs)} pairs, want {want}"
    for a, b in _pairs:
        assert a != b and lk_hash(a) == lk_hash(b), (hex(a), hex(b))
        assert max(a, b) < 1 << 253 < min(MODULUS.values())
    return _pairs


# ---- the cases ------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, l, t, h_g=False):
        self.name, self.l, self.t, self.h_g = name, l, t, h_g

    def __repr__(self):
        return self.name


@functools.lru_cache(maxsize=None)
def _fillers(field, n, seed):
    rng, p, out = random.Random(seed), MODULUS[field], set()
    while len(out) < n:
        out.add(rng.randrange(1 << 253, p))
    return tuple(sorted(out, key=lk_hash))


def fillers(field, n, seed):
    """n distinct canonical representations, none of a colliding pair (2^253 <= filler < p), in the order of their hashes"""
    return list(_fillers(field, n, seed))


def counted_l(t, absent, extra=()):
    """l: t[i] taken 1 + i % 4 times for every seventh index and the first ones, every third element absent from t, then `extra`"""
    picks = [t[i] for i in range(len(t)) if i < 40 or i % 7 == 0 for _ in range(1 + i % 4)]
    l = []
    for q, v in enumerate(picks):
        l.append(v)
        if q % 2 == 1:
            l.append(absent[(q // 2) % len(absent)])
    return l + list(extra)


def pair_cases(field):
    pairs = colliding_pairs()
    fill = fillers(field, 4200, 0xF111 + field)
    absent = fill[4100:]
    out = []

    def case(name, n_t, places, k, l_extra=None):
        a, b = pairs[k % len(pairs)]
        t = list(fill[:n_t])
        for at, which in places:
            t[at] = (a, b)[which]
        extra = [a] * 5 + [b] * 3 + [a, b] * 2 if l_extra is None else l_extra(a, b)
        l = counted_l(t, absent, extra)
        if l.count(a) == l.count(b):
            l.append(a)
        out.append(Case(f"pair {name}", l, t, h_g=True))

    case("adjacent lanes", 63, [(10, 0), (11, 1)], 0)
    case("adjacent lanes, B first", 65, [(10, 1), (11, 0)], 1)
    case("two waves of a workgroup", 257, [(5, 0), (64 + 5, 1)], 2)
    case("two workgroups", SMALL, [(7, 0), (256 + 7, 1)], 3)
    case("repeated in a wave, A leads", 257, [(64 + 3, 0), (64 + 9, 1), (64 + 20, 0), (64 + 30, 1), (64 + 63, 1)], 4)
    case("repeated in a wave, B leads", 257, [(128 + 0, 1), (128 + 1, 0), (128 + 40, 1), (128 + 41, 0), (128 + 42, 0)], 5)
    case("repeated across waves and workgroups", SMALL, [(62, 1), (63, 0), (64, 0), (65, 1), (255, 0), (256, 1), (4098, 0), (4097, 1)], 6)
    case("a wave of the two keys only", 65, [(i, (i // 3) % 2) for i in range(64)], 7)
    case("one key absent from t", 63, [(10, 0), (40, 0)], 0, l_extra=lambda a, b: [a] * 4 + [b] * 6 + [a, b, b])
    case("one key absent from t, the other in two workgroups", SMALL, [(300, 1), (2000, 1)], 1, l_extra=lambda a, b: [a] * 9 + [b] * 2)
    # every pair side by side in one wave: eight hash groups of two keys each
    t = list(fill[:257])
    extra = []
    for k, (a, b) in enumerate(pairs[:8]):
        for q, at in enumerate((4 * k, 4 * k + 1, 32 + 4 * k, 32 + 4 * k + 3)):
            t[at] = (a, b, b, a)[q]
        extra += [a] * (k + 1) + [b] * (2 * k + 3)
    l = counted_l(t, absent, extra)
    for a, b in pairs[:8]:
        if l.count(a) == l.count(b):
            l.append(b)
    out.append(Case("pair: eight pairs in one wave", l, t, h_g=True))
    for c in out:                                                          # what the names promise
        both = [v for v in set(c.l) if any(v in p for p in pairs)]
        assert both and all(c.l.count(a) != c.l.count(b) for a, b in pairs if a in c.l and b in c.l), c.name
    return out


STRUCTURES = ("equal", "distinct", "alternating", "groups", "late first")


def structure_t(field, kind, n_t):
    fill = fillers(field, 4200, 0x57C0 + field)
    if kind == "equal":
        return [fill[0]] * n_t
    if kind == "distinct":
        return fill[:n_t]
    if kind == "alternating":
        return [fill[i % 2] for i in range(n_t)]
    if kind == "groups":                                                  # per wave: values of 1, 2, 3 ... lanes, interleaved; other values in the next wave
        t = []
        for wave in range(-(-n_t // 64)):
            lanes, size = [], 1
            while len(lanes) < 64:
                lanes += [fill[(wave % 5) * 16 + size]] * size
                size += 1
            lanes = lanes[:64]
            random.Random(0x6209 + wave).shuffle(lanes)
            t += lanes
        return t[:n_t]
    if kind == "late first":                                              # first at lane 60 of wave 0; lanes 0 and 1 of workgroup 1 hold it too
        t = fill[1:n_t + 1]
        for at in (60, 256, 257, 1024):
            if at < n_t:
                t[at] = fill[0]
        return t
    raise ValueError(kind)


def structure_cases(field):
    absent = fillers(field, 4200, 0x57C0 + field)[4150:]
    return [Case(f"t {kind} n_t={n_t}", counted_l(t, absent), t) for kind in STRUCTURES for n_t in N_T for t in [structure_t(field, kind, n_t)]]


def count_cases(field, big=True):
    fill = fillers(field, 4200, 0xC027 + field)
    absent = fill[4150:]
    # 130 distinct values of t in the first 256 elements of l, twice each, in two orders
    t = fill[:300] + fill[:57]
    l = fill[:128] + fill[127::-1] + counted_l(t, absent)
    assert len(set(l[:256])) >= 65 and set(l[:256]) <= set(t)
    out = [Case("l: 128 hot values in one workgroup's share", l, t)]
    l = [fill[(3 * i) % 130] for i in range(256)] + [absent[0]] * 7 + [fill[i % 130] for i in range(300)]
    out.append(Case("l: 130 hot values, strided", l, t))
    if big:
        # 2048 workgroups of 256 lanes, a second trip of 100 elements: lanes 0 and 17 of every workgroup hold `hot`, every third
        # element is absent from t, the others walk over t
        t = [fill[(i * i) % 600] for i in range(SMALL)]
        ids = np.arange(BIG_N_L)
        which = (ids * 7 + ids // 256) % 600
        pool = fill[:600] + absent[:3] + [fill[700]]                      # 600 .. 602 absent, 603 = hot (fill[700] goes into t below)
        t[1000] = t[3000] = fill[700]
        which = np.where(ids % 3 == 2, 600 + (ids // 3) % 3, which)
        which = np.where((ids % 256 == 0) | (ids % 256 == 17), 603, which)
        l = [pool[k] for k in which.tolist()]
        assert l.count(fill[700]) == 2 * 2048 + 2 and fill[700] not in fill[:600]
        out.append(Case(f"l: {BIG_N_L} elements, a value every workgroup counts", l, t))
    return out


# ---- the driver -----------------------------------------------------------------------------------------------------------------
def check_case(lib, field, case):
    """m twice under the hashed table and, for the small cases, twice with every key probing from slot 0; h and g where the case asks"""
    from test_lookup_witness_emu import ref_h_g, ref_m
    cv, p = E._Convert(field), MODULUS[field]
    l, t = case.l, case.t
    n_l, n_t = len(l), len(t)
    m_ints = ref_m(l, t)
    in_t = set(t)
    assert sum(m_ints) == sum(1 for v in l if v in in_t)
    want = cv.array(m_ints)
    modes = (None, 1) if max(n_l, n_t) <= SMALL else (None,)
    with E.Dev(lib) as dev:
        d_l, d_t = dev.put(E.to_array(l)), dev.put(E.to_array(t))
        first = None
        for mode in modes:
            with E.knobs(lib, LOOKUP_HASH=mode):
                for run in (0, 1):
                    d_m = dev.empty(n_t)
                    LU.evaluate_m_device(field, d_m, d_l, n_l, d_t, n_t, lib=lib)
                    got = dev.get(d_m, n_t)
                    E.same_bytes(got, want, f"{case.name} field={field} hash={mode} run {run}: m")
                    first = got if first is None else first
                    assert got.tobytes() == first.tobytes()
        if case.h_g:
            r = cv.value(E.representations(field)[9])
            h_ints, g_ints = ref_h_g(cv.values(l), cv.values(t), m_ints, r, p)
            d_h, d_g = dev.empty(n_l), dev.empty(n_t)
            LU.evaluate_h_g_device(field, d_h, d_g, d_l, n_l, d_t, d_m, n_t, r, lib=lib)
            E.same_bytes(dev.get(d_h, n_l), cv.array(h_ints), f"{case.name} field={field}: h")
            E.same_bytes(dev.get(d_g, n_t), cv.array(g_ints), f"{case.name} field={field}: g")
