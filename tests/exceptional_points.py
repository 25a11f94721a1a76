"""Structured MSM inputs that drive the exceptional branches of the group law -- the same point twice, opposite points, the
identity on either side -- through every stage and mode of the MSM, and the driver that runs them.

Pseudorandom bases (128-bit multiples of G) never make two partial sums coincide or cancel, so xyzz29_add_affine, xyzz29_add,
xyzz29_double (curve29.cuh) and the DPP-quad versions (quad29.cuh) leave their common path only in k_accumulate, on a repeated
base.  Here every base is m G for m from a SMALL multiplier set and the scalars are few distinct values, so that buckets,
partial sums, tree nodes and window sums collide all the time:

    multipliers(cid, c)     0 (the identity, all zero), +-1, +-2, +-3, lambda m and lambda^2 m (phi(P_i) = P_j across the two
                            halves of the GLV key), 2^c m (a window sum equal to the Horner accumulator of the windows above)
    keys                    random draws, all G, alternating G / -G, periodic keys whose period divides the segment length of
                            k_accumulate (10 entries) and the 64-partial sub-jobs of the heavy fix-up: head, tail and sub-job
                            partials of one bucket come out equal, or opposite with a sign flip per period
    scalars                 small values, r - small values, digits from {0, 1, 2, 2^(c-1) - 1, 2^(c-1), 2^c - 2, 2^c - 1} per
                            window (the signed-digit carry boundary), one scalar for the whole vector, the GLV edge list

A case is four small things: a table of multipliers, an index per pair into it, a table of scalar values and an index per pair
into that -- arrays are built with numpy, and the expected point is (sum_i s_i k_i mod r) G in Python integers: ONE scalar
multiplication whatever n is, independent of Pippenger and of the C oracle.  Nothing expected comes from the library under
test.  run_mode() drives one mode of the MSM under a forced configuration through the C ABI of whichever library it is handed:
the CPU emulation (tests/test_exceptional_points_emu.py, which also reads the branch census of that run) or the GPU build
(tests/test_gpu_exceptional_points.py) -- the same cases under the same knobs, so the census says what the GPU run executed."""
import functools
import random

import numpy as np

from helpers import glv_edge_scalars, point_to_arr, scalar_field_id
from mira_amd import _lib
from mira_amd import commitment as cm
from oracle import cref as C
from oracle import pyref as P

SEGMENT = 10          # msm_plan.hip: minimum segment length of k_accumulate (every commit below ~2 M sorted entries has it)
SUBJOB = 64           # msm_kernels.cuh: HEAVY_SUB, partials per stage-A sub-job of a heavy run


# ---- the group, in Python integers ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def eigenvalue(cid):
    """lambda with phi(x, y) = (beta x, y) = lambda (x, y), derived as tools/glv_constants.py derives it: the smaller of the two
    cube roots of unity of the scalar field that pair with a cube root of unity beta of the base field on the generator"""
    cv = P.CURVES[cid]

    def cube_roots(mod):
        for g in range(2, 50):
            w = pow(g, (mod - 1) // 3, mod)
            if w != 1:
                return w, w * w % mod
        raise ValueError("no generator found")
    G = P.synth_base(0, cv)
    pair = [(b, l) for b in cube_roots(cv.p) for l in cube_roots(cv.r) if (b * G[0] % cv.p, G[1]) == P.ec_mul(l, G, cv)]
    assert len(pair) == 2
    beta, lam = min(pair, key=lambda x: x[1])
    assert (lam * lam + lam + 1) % cv.r == 0 and pow(beta, 3, cv.p) == 1
    return lam


@functools.lru_cache(maxsize=None)
def multiple_of_g(cid, m):
    """m G as the (8,) uint64 array of the C ABI (identity: all zero); one scalar multiplication per multiplier"""
    cv = P.CURVES[cid]
    arr = point_to_arr(P.ec_mul(m % cv.r, cv.gen, cv), cid)
    arr.setflags(write=False)
    return arr


def multipliers(cid, c):
    r, lam = P.CURVES[cid].r, eigenvalue(cid)
    ms = [0, 1, -1, 2, -2, 3, -3, lam, -lam, 2 * lam, lam * lam, -lam * lam, 2 * lam * lam, 1 << c, -(1 << c), 2 << c, 3 << c]
    return [m % r for m in ms]


def glv_edge(r):
    """the GLV edge list of test_glv_split_every_width (helpers.glv_edge_scalars) and the two neighbours it leaves out"""
    return glv_edge_scalars(r) + [(1 << 127) + 1, 1 << 128]


def window_digits(c):
    return [0, 1, 2, (1 << (c - 1)) - 1, 1 << (c - 1), (1 << c) - 2, (1 << c) - 1]


def digit_scalar(c, rng):
    """one digit of the list per window, below 2^252"""
    return sum(rng.choice(window_digits(c)) << (c * w) for w in range(252 // c))


# ---- cases ----------------------------------------------------------------------------------------------------------------------
class Case:
    """mults[key_idx[i]] G is base i, scalars[sc_idx[i]] its scalar"""

    def __init__(self, name, cid, mults, key_idx, scalars, sc_idx, cut=None):
        self.name, self.cid, self.cut = name, cid, cut          # cut: where the chunk-partials mode cuts the vector
        self.mults, self.scalars = [int(m) for m in mults], [int(s) for s in scalars]
        self.key_idx, self.sc_idx = np.asarray(key_idx, dtype=np.int64), np.asarray(sc_idx, dtype=np.int64)
        assert len(self.key_idx) == len(self.sc_idx)
        r = P.CURVES[cid].r
        assert all(0 <= m < r for m in self.mults) and all(0 <= s < r for s in self.scalars)

    @property
    def n(self):
        return len(self.key_idx)

    def bases(self):
        table = np.stack([multiple_of_g(self.cid, m) for m in self.mults])
        return np.ascontiguousarray(table[self.key_idx])

    def scalar_array(self):
        """(n, 4) uint64 Montgomery, converted by the oracle's to_mont on the whole array"""
        table = np.array([P.limbs4(s) for s in self.scalars], dtype=np.uint64).reshape(-1, 4)
        return C.to_mont(scalar_field_id(self.cid), np.ascontiguousarray(table[self.sc_idx]))

    def total(self):
        """sum_i s_i k_i mod r: pairs counted per (multiplier, scalar) combination, the sum in Python integers"""
        counts = np.bincount(self.key_idx * len(self.scalars) + self.sc_idx, minlength=len(self.mults) * len(self.scalars))
        r = P.CURVES[self.cid].r
        return sum(int(cnt) * self.mults[k // len(self.scalars)] * self.scalars[k % len(self.scalars)] for k, cnt in enumerate(counts) if cnt) % r

    def expected(self):
        return np.array(multiple_of_g(self.cid, self.total()))

    def identity_bases(self):
        """how many bases of the key are the identity (all zero)"""
        return int((np.array(self.mults, dtype=object)[self.key_idx] == 0).sum())


def _pick(rng, count, size):
    return [rng.randrange(count) for _ in range(size)]


def draw_case(name, cid, c, n, scalars, seed, sc_idx=None):
    """random draws from the multiplier set against the given scalar table (drawn too unless sc_idx names them)"""
    rng = random.Random(seed)
    ms = multipliers(cid, c)
    cs = Case(name, cid, ms, _pick(rng, len(ms), n), scalars, _pick(rng, len(scalars), n) if sc_idx is None else sc_idx)
    assert cs.identity_bases()             # the identity base goes wherever a key of draws goes: k_glv_bases, k_table_step, the gathers
    return cs


def grouped_case(name, cid, c, groups, extra=0, seed=0):
    """groups of consecutive pairs (scalar, key pattern): the pairs of one scalar value share a bucket in every window and, sorted
    by index, lie there in this order.  A key pattern is a list of multipliers, one per pair.  `extra` random draws follow so
    that the expected point is not the identity when the groups cancel."""
    ms = multipliers(cid, c)
    r = P.CURVES[cid].r
    rng = random.Random(seed)
    scalars, key_idx, sc_idx = [], [], []
    for s, pattern in groups:
        scalars.append(s % r)
        key_idx += [ms.index(m % r) for m in pattern]
        sc_idx += [len(scalars) - 1] * len(pattern)
    if extra:
        small = [1, 2, 3, 5, r - 1, r - 2]
        key_idx += _pick(rng, len(ms), extra)
        sc_idx += [len(scalars) + i for i in _pick(rng, len(small), extra)]
        scalars += small
    return Case(name, cid, ms, key_idx, scalars, sc_idx)


def pair_case(name, cid, pairs, cut=None):
    """a handful of (scalar, multiplier) pairs, any multiplier"""
    r = P.CURVES[cid].r
    mults = sorted({m % r for _, m in pairs})
    scalars = sorted({s % r for s, _ in pairs})
    cs = Case(name, cid, mults, [mults.index(m % r) for _, m in pairs], scalars, [scalars.index(s % r) for s, _ in pairs], cut=cut)
    assert cs.total() != 0
    return cs


def reduction_cases(cid, c):
    """Pairs placed bucket by bucket, one window per pattern (a digit d of window w is the scalar d 2^(c w); bucket d - 1 of that
    window then holds the base), against the bucket reduction of reduce_kernels.cuh and the host's chain of doublings:
      phase_a     buckets d and d - 1 of one chunk: the running sum meets its opposite (-G, then G) and the weighted sum meets the
                  opposite of the running sum (G, then G - 2 G)
      tree        buckets 0 and 2^j: the sums A and V of two sibling nodes are opposite, at every level j of the tree, whichever
                  chunk length and workgroup size the plan picks
      device_horner   buckets 2^(k+1) and 2^k hold G and -2 G: the doubled Horner accumulator of k_set_finish meets its opposite
      host_horner     the window sums of two neighbouring windows are G and -+2^c G: the accumulator of horner_pieces, doubled c
                  times, meets its opposite (then continues from the identity) and its equal
      partial_halves  two chunk partials with opposite sums in window 0 and equal sums in window 1 (sum_partials)"""
    wins = 252 // c
    at = lambda d, w: d << (c * w)
    phase, tree, horner = [], [], []
    for i, d in enumerate((1, 3, 5)):
        phase += [(at(d + 1, 2 * i), -1), (at(d, 2 * i), 1), (at(d + 1, 2 * i + 1), 1), (at(d, 2 * i + 1), -2)]
    for j in range(1, min(c - 1, wins + 1)):
        tree += [(at(1, j - 1), 1), (at((1 << j) + 1, j - 1), -1)]
    for k in range(1, min(c - 2, wins + 1)):
        horner += [(at((2 << k) + 1, k - 1), 1), (at((1 << k) + 1, k - 1), -2)]
    host = [(at(1, wins - 1), 1), (at(1, wins - 2), -(1 << c)), (at(1, wins - 3), 1), (at(1, wins - 4), 1 << c)]
    halves = [(3, 1)] * 5 + [(at(3, 1), 1)] * 5 + [(3, -1)] * 5 + [(at(3, 1), 1)] * 5
    return [pair_case("phase_a", cid, phase), pair_case("tree", cid, tree), pair_case("device_horner", cid, horner),
            pair_case("host_horner", cid, host), pair_case("partial_halves", cid, halves, cut=10)]


def all_of(m, count):
    return [m] * count


def alternating(m, count):
    return [m if i % 2 == 0 else -m for i in range(count)]


def flip_every(m, period, count):
    """`period` pairs of m G, `period` of -m G, ...: with period = SEGMENT the partials of consecutive segments are opposite,
    with period = SEGMENT * SUBJOB the sub-job sums of a heavy run are"""
    return [m if (i // period) % 2 == 0 else -m for i in range(count)]


def periodic(pattern, count):
    return [pattern[i % len(pattern)] for i in range(count)]


def heavy_run(m, signs):
    """one heavy bucket whose tail partial (the first segment) is the identity and whose sub-job sums are sign * 640 s m G: stage B
    of the heavy fix-up adds equal (+, +) or opposite (+, -) sub-job sums"""
    out = alternating(m, SEGMENT)
    for sg in signs:
        out += all_of(sg * m, SEGMENT * SUBJOB)
    return out


@functools.lru_cache(maxsize=None)
def cases(cid, c, heavy=True):
    """the cases of one curve and window width; every pair count of a group is a multiple of SEGMENT, so that the runs of the
    sorted entries start on segment boundaries.  At most one case -- alt_identity -- has the identity as its expected point."""
    r = P.CURVES[cid].r
    rng = random.Random(1000 * cid + c)
    small = [0, 1, 2, 3, 4, 5]
    near_r = [r - 1, r - 2, r - 3]
    light = [(3, all_of(1, 40)), (r - 2, flip_every(2, SEGMENT, 50)), (5, periodic([1, 2, 3, -1, 2], 60)), (7 << c, alternating(3, 30)),
             ((1 << (c - 1)) + 1, flip_every(1, SEGMENT, 70)), (r - 5, all_of(-3, 20))]
    medium = [(11 + 2 * j + (j << (2 * c)), (all_of(1, 100), flip_every(1, SEGMENT, 110), periodic([2, -1, 1, 1, 2], 90))[j % 3]) for j in range(9)]
    out = [
        draw_case("draws_small", cid, c, 300, small + near_r, seed=1),
        draw_case("draws_digits", cid, c, 300, [digit_scalar(c, rng) for _ in range(24)], seed=2),
        draw_case("draws_glv_edge", cid, c, 300, glv_edge(r), seed=3, sc_idx=[i % len(glv_edge(r)) for i in range(300)]),
        grouped_case("all_g_one_scalar", cid, c, [(digit_scalar(c, rng) | 1, all_of(1, 300))]),
        grouped_case("alt_identity", cid, c, [(digit_scalar(c, rng) | 1, alternating(1, 300))]),
        # light chains (2 .. 7 partials per bucket): equal partials, opposite ones, partials that are the identity; nine medium runs
        # (9 .. 11 partials) beside a heavy one (20): chains of the light section under the emulation
        grouped_case("chains", cid, c, light + medium + [(r - 7, all_of(2, 200))], extra=30, seed=4),
        # the medium runs alone: sub-jobs of the heavy section
        grouped_case("medium_alone", cid, c, medium, extra=30, seed=8),
    ]
    if heavy:
        s = digit_scalar(c, rng) | 1
        out += [
            grouped_case("heavy_equal_subjobs", cid, c, [(s, heavy_run(1, (1, 1)))], extra=50, seed=5),
            grouped_case("heavy_opposite_subjobs", cid, c, [(s, heavy_run(1, (1, -1)))], extra=50, seed=6),
            grouped_case("heavy_flip_per_segment", cid, c, [(s, flip_every(1, SEGMENT, SEGMENT * (2 * SUBJOB + 2)))], extra=50, seed=7),
        ]
    out += reduction_cases(cid, c)
    identities = [cs.name for cs in out if cs.total() == 0]
    assert identities == ["alt_identity"], identities          # an all-zero output passes one case at the most
    return out


def batch_case(cid, c, n=300):
    """one key of random draws and three scalar vectors over it (commit_batch wants equal lengths)"""
    r = P.CURVES[cid].r
    rng = random.Random(77 + cid)
    key = _pick(rng, len(multipliers(cid, c)), n)
    ms = multipliers(cid, c)
    vs = [Case("batch_small", cid, ms, key, [0, 1, 2, 3, r - 1, r - 2], _pick(rng, 6, n)),
          Case("batch_digits", cid, ms, key, [digit_scalar(c, rng) for _ in range(16)], _pick(rng, 16, n)),
          Case("batch_one_scalar", cid, ms, key, [digit_scalar(c, rng) | 1], [0] * n)]
    assert all(v.total() != 0 for v in vs) and vs[0].identity_bases()
    return vs


def big_case(name, cid, c, n, key, seed=0):
    """The shapes only hardware runs cheaply: n pairs over a key that is "all_g" or "periodic" -- period 30, segments of SEGMENT
    bases with sums S, -S, S: a chain of partials meets its opposite, goes on from the identity and meets its equal in the next
    period -- and 64 digit-built scalars dealt in blocks of 600 consecutive pairs, so that the entries of a bucket are whole periods
    in index order.  (Where a window does not start on a segment boundary -- n is the test's, not a multiple of SEGMENT -- the
    three segment sums of a period differ and still repeat every period; under all_g every partial of a bucket is the same point
    wherever the segments are cut.)"""
    rng = random.Random(seed)
    ms = multipliers(cid, c)
    i = np.arange(n)
    if key == "all_g":
        key_idx = np.full(n, ms.index(1))
    else:
        seg = [1, 2, 3, -1, 2, 1, 2, 3, -1, 2]
        pat = np.array([ms.index(m % P.CURVES[cid].r) for m in seg + [-m for m in seg] + seg])
        key_idx = pat[i % len(pat)]
    scalars = [digit_scalar(c, rng) | 1 for _ in range(64)]
    cs = Case(name, cid, ms, key_idx, scalars, (i // 600) % len(scalars))
    assert cs.total() != 0
    return cs


def medium_flood_case(cid, c=8, per_bucket=100):
    """More than 1 024 medium runs beside a heavy one -- the number from which the GPU build sums medium runs as chains of the light
    section (msm_kernels.cuh: MEDIUM_AS_CHAINS_FROM; the emulation build switches at 8): all G under uniformly drawn scalars,
    2^(c-1) * per_bucket pairs, so that a bucket holds 100 +- 10 entries of one and the same point -- at c = 8 some 3 300 of the
    4 096 buckets are medium runs wherever the segments are cut, some 80 heavy ones (the 64 of the sparse top window among them), the rest
    one or the other depending on the cuts -- and 200 pairs of one more scalar make a bucket per window heavy.  The counts are asserted below."""
    r = P.CURVES[cid].r
    rng = random.Random(31 + cid)
    n = (1 << (c - 1)) * per_bucket
    scalars = [rng.randrange(r) for _ in range(n)] + [digit_scalar(c, rng) | 1]
    cs = Case("medium_flood", cid, [1], np.zeros(n + 200, dtype=np.int64), scalars, np.concatenate([np.arange(n), np.full(200, n)]))
    assert cs.total() != 0
    # The placement, counted here and not left to the expectation: a run of `cnt` sorted entries cut into segments of SEGMENT has
    # floor((cnt - 1) / SEGMENT) or one more head partials behind its tail partial, wherever the cuts fall.  It is a medium run
    # (HEAVY_SPAN = 6 < partials <= MEDIUM_SPAN = 12) for certain from 7 SEGMENT + 1 to 11 SEGMENT entries, a heavy one for certain
    # from 13 SEGMENT + 1.  All windows are sorted and counted together (one launch of k_accumulate over W 2^(c-1) buckets).
    cnt = signed_digit_counts(cs, c)
    assert ((cnt >= 7 * SEGMENT + 1) & (cnt <= 11 * SEGMENT)).sum() >= 1024 and (cnt >= 13 * SEGMENT + 1).any()
    return cs


def signed_digit_counts(cs, c):
    """entries per (window, bucket) of a plain per-window commit of `cs` under c-bit windows, by the recoding of k_digits
    (msm_kernels.cuh): digits of c bits from the low end, raw + carry >= 2^(c-1) becomes raw + carry - 2^c with a carry into the
    next window; digit d != 0 goes to bucket |d| - 1"""
    limbs = np.array([P.limbs4(s) + [0] for s in cs.scalars], dtype=np.uint64)
    weight = np.bincount(cs.sc_idx, minlength=len(cs.scalars))
    wins, half = -(-256 // c), 1 << (c - 1)
    out = np.zeros((wins, half), dtype=np.int64)
    carry = np.zeros(len(cs.scalars), dtype=np.int64)
    for w in range(wins):
        limb, off = divmod(c * w, 64)
        raw = limbs[:, limb] >> np.uint64(off)
        if off + c > 64:
            raw = raw | (limbs[:, limb + 1] << np.uint64(64 - off))
        d = (raw & np.uint64((1 << c) - 1)).astype(np.int64) + carry
        carry = (d >= half).astype(np.int64)
        mag = np.where(carry == 1, (1 << c) - d, d)
        out[w] = np.bincount(mag, weights=weight, minlength=half + 1)[1:half + 1]
    return out


# ---- the driver -----------------------------------------------------------------------------------------------------------------
class Knobs:
    """mira_set_tuning / forced widths for the duration of a with block; everything is restored on exit"""

    def __init__(self, lib):
        self.lib, self.used = lib, []

    def __enter__(self):
        return self

    def tune(self, knob, value):
        self.used.append(knob)
        self.lib.tune(knob, value)

    def __exit__(self, *exc):
        for knob in self.used:
            self.lib.tune(knob, -1)
        self.lib.check(self.lib.c.mira_msm_set_window_bits(0))


# mode -> (window widths, heavy cases too, the cases it runs: None = all).  Width 0: the planner's choice.  The modes whose emulated
# commits take seconds (1024-lane sort kernels as OS threads, tables built per key) run a selection.
FEW = ("draws_small", "draws_digits", "all_g_one_scalar", "chains", "phase_a", "tree", "device_horner", "host_horner")
MODES = {
    "plain": ((0, 7), True, None),
    "plain_single_lane_tree": ((10,), False, None),
    "glv": ((0, 9), True, None),
    "shared8": ((8,), False, FEW),
    "shared13": ((13,), False, FEW),
    "front": ((9,), False, FEW[1:]),
    "staged": ((11,), False, FEW[1:]),
    "host_chunks": ((9,), False, None),
    "partials": ((9,), False, None),
    "batch": ((8,), False, None),
}
CASE_WIDTH = {0: 12}     # the multiplier 2^c of a planned commit: any width will do
GLV_FORCED_WIDTHS = (5, 13, 16)      # GPU module: the GLV path at forced widths beside the planned one and 9
WIDE_WIDTHS = (17, 20)               # GPU module: real wide windows


def wide_case(cid, c, key):
    """2^12 pairs of a structured key under a real wide window"""
    return big_case(f"wide_{key}", cid, c, 1 << 12, key, seed=c)


def run_case(lib, key, cs, mode, c):
    sc = cs.scalar_array()
    if mode == "partials":
        d = lib.alloc(cs.n * 32)
        lib.upload(d, sc)
        cut = cs.cut or (cs.n // 3) // SEGMENT * SEGMENT + 3
        parts = []
        for first, cnt in ((0, cut), (cut, cs.n - cut)):
            part, cc, ww = key.commit_partial_device(first, d + first * 32, cnt, window_bits=c)
            parts.append(part)
        lib.free(d)
        return cm.combine_partials(cs.cid, np.stack(parts), cc, ww, lib=lib)
    return key.commit(sc)


def run_mode(lib, mode, cid, widths=None, only=None):
    """every case of `mode` on curve `cid`: [(label, got, expected)]"""
    widths_default, heavy, selection = MODES[mode]
    only = only or selection
    out = []
    for c in widths or widths_default:
        with Knobs(lib) as k:
            cw = CASE_WIDTH.get(c, c)
            if mode in ("plain", "plain_single_lane_tree", "front", "staged", "host_chunks", "partials", "batch"):
                k.tune(_lib.TUNE_GLV_AUTO_MAX_LOG, 0)
            if mode == "plain_single_lane_tree":
                k.tune(_lib.TUNE_REDUCE_QUAD, 0); k.tune(_lib.TUNE_REDUCE_PIECES, 3); k.tune(_lib.TUNE_REDUCE_LAMBDA, 2)
            if mode == "plain" and c:
                k.tune(_lib.TUNE_REDUCE_QUAD, 1); k.tune(_lib.TUNE_REDUCE_PIECES, 2); k.tune(_lib.TUNE_REDUCE_LAMBDA, 1)
            if mode in ("shared8", "shared13"):
                k.tune(_lib.TUNE_TABLE_MIN_N, 1); k.tune(_lib.TUNE_SHARED_MIN_N, 1); k.tune(_lib.TUNE_TABLE_WIDTH, c)
            if mode == "front":
                k.tune(_lib.TUNE_WIDE_FRONT_MIN_C, 5)
            if mode == "staged":
                k.tune(_lib.TUNE_STAGED_MIN_N, 1)
            if mode == "host_chunks":
                k.tune(_lib.TUNE_HOST_CHUNK_MIN_N, 64)
            if mode == "batch":
                vs = batch_case(cid, cw)
                key = cm.CommitmentKey(cid, vs[0].bases(), lib=lib)
                key.set_window_bits(c)
                got = key.commit_batch([v.scalar_array() for v in vs])
                out += [(f"{mode}/c{c}/{v.name}", got[i], v.expected()) for i, v in enumerate(vs)]
                key.close()
                continue
            chosen = [cs for cs in cases(cid, cw, heavy) if not only or cs.name in only]
            assert any(cs.identity_bases() for cs in chosen), (mode, c)      # every mode and width sees a key with an identity base
            for cs in chosen:
                key = cm.CommitmentKey(cid, cs.bases(), lib=lib)
                if mode == "glv":
                    key.precompute(_lib.TABLE_GLV)
                if mode in ("shared8", "shared13"):
                    key.precompute(c)
                else:
                    key.set_window_bits(c)
                out.append((f"{mode}/c{c}/{cs.name}", run_case(lib, key, cs, mode, c), cs.expected()))
                key.close()
    return out


def run_big(lib, cs, c, knobs=()):
    """one larger case with its scalars in device and in host memory, under a forced width and knobs [(knob, value)]"""
    with Knobs(lib) as k:
        k.tune(_lib.TUNE_GLV_AUTO_MAX_LOG, 0)
        for knob, value in knobs:
            k.tune(knob, value)
        key = cm.CommitmentKey(cs.cid, cs.bases(), lib=lib)
        key.set_window_bits(c)
        sc = cs.scalar_array()
        d = lib.alloc(cs.n * 32)
        lib.upload(d, sc)
        want = cs.expected()
        out = [(f"{cs.name}/c{c}/device", key.commit_device(d, cs.n), want), (f"{cs.name}/c{c}/host", key.commit(sc), want)]
        lib.free(d)
        key.close()
    return out


def run_tables(lib, cid, bits):
    """the fixed-base window tables of `bits` (20 or 22) bits: one set of 2^(bits-1) buckets, k_reduce_chunks and k_window_sum"""
    out = []
    with Knobs(lib) as k:
        k.tune(_lib.TUNE_TABLE_MIN_N, 1)
        k.tune(_lib.TUNE_GLV_AUTO_MAX_LOG, 0)
        cs = table_case(cid, bits)
        key = cm.CommitmentKey(cid, cs.bases(), lib=lib)
        key.precompute(bits)
        out.append((f"tables{bits}/{cs.name}", key.commit(cs.scalar_array()), cs.expected()))
        key.close()
    return out


@functools.lru_cache(maxsize=None)
def table_case(cid, bits):
    """ONE commit over the tables (2^19 emulated buckets take half a minute).  A scalar d < 2^(bits-1) puts its base into bucket
    d - 1 of the one shared set; k_reduce_chunks folds chunks of 8 buckets (R_j = sum_i (8 j + i + 1) S_(8 j + i)), k_window_sum adds
    the chunks q, q + 512, ... of each of its 64 sums in lane q and then the lanes in a tree (lane x += lane x + 256, ...):
      chunks 1 and 7      buckets 9 and 8 hold -G and G (the running sum meets its opposite), 57 and 56 hold G and G (its equal)
      chunks 2 and 514    17 * 4113 G and 4113 * -17 G: lane 2's strided sum meets its opposite; chunks 3 and 515 its equal
      chunks 4 and 260    lanes 4 and 260 of the tree hold opposite sums; chunks 5 and 261 equal ones
    beside draws from the multiplier set (2^bits m: rows of different tables are equal points) with scalars around the digit
    boundaries, an identity base and a zero scalar"""
    r = P.CURVES[cid].r
    ms = multipliers(cid, bits)
    half = 1 << (bits - 1)
    pairs = [(10, -1), (9, 1), (58, 1), (57, 1)]
    for lo, hi, sign in ((2, 514, -1), (3, 515, 1), (4, 260, -1), (5, 261, 1)):
        pairs += [(8 * lo + 1, 8 * hi + 1), (8 * hi + 1, sign * (8 * lo + 1))]
    edge = [0, half - 1, half, half + 1, (1 << bits) - 1, 1 << bits, (1 << bits) + 1, r - 1, r - 2, (3 << bits) + 2, (half - 1) << bits]
    rng = random.Random(bits + cid)
    pairs += [(rng.choice(edge), rng.choice(ms)) for _ in range(180)]
    cs = pair_case("tables", cid, pairs)
    assert cs.identity_bases()             # k_table_step leaves before its first doubling on them
    return cs


# ---- the branch census of the emulation (mira_amd/csrc/f29_census.h, tests/emu/emu.h) ---------------------------------------------------
def census_reset(emu_lib):
    emu_lib.c.mira_emu_census_reset.restype = None
    emu_lib.c.mira_emu_census_reset()


def census_read(emu_lib):
    """{(kernel, section, function, exit): hits} since the last reset; kernel is the launch's own text ("k_accumulate<F, true>"),
    "host" between launches"""
    import ctypes
    fn = emu_lib.c.mira_emu_census_read
    fn.restype, fn.argtypes = ctypes.c_size_t, [ctypes.c_char_p, ctypes.c_size_t]
    size = fn(None, 0) + 1
    buf = ctypes.create_string_buffer(size)
    fn(buf, size)
    out = {}
    for line in buf.value.decode().splitlines():
        kernel, section, function, site, hits = line.split("|")
        out[(kernel.strip("()"), section, function, site)] = int(hits)
    return out
