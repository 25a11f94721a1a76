"""Worst-case field operands for the field-arithmetic kernels, and the drivers that run them.

The kernels compute in the 9 x 29-bit "loose" representation of field29.cuh, which is correct only while a set of limb
bounds holds (uncarried butterflies, subtraction biases, the multiplier's a * b <= 168 P^2, the final reduce_once).  A bound
off by one bit fails for about one uniformly drawn input in 2^29 .. 2^60, so pseudorandom test data never meets it.  This
module builds operands BY STORED REPRESENTATION -- the 256-bit integer (4 x u64) the C ABI reads, whose value is
rep * 2^-256 mod p -- because the limb patterns are what the bounds are about:

    representations(field)   the list: 0, 1, p-1, p-2, (p-1)/2, (p+1)/2, every 29-bit limb all ones, powers of two at the
                             limb boundaries of both limb widths and their predecessors, the Montgomery forms of 1, -1, 2, 1/2
    constant / alternating / ends / cycled / picked     vectors of n representations
    to_value / from_value    representation <-> canonical value, in Python integers
    to_array / from_array    list of representations <-> (n, 4) uint64

The check_* functions drive one kernel family each through the C ABI of whichever library they are handed (the GPU build,
or the CPU emulation whose F29_TRACK build asserts every limb bound on the values actually seen) and compare bytes with
expected values that come from Python integers -- for the transforms from the C oracle, which test_edge_operands_emu.py
pins to a Python-integer NTT on these same patterns first.  Nothing expected ever comes from the library under test.

    python tests/edge_operands.py LIBRARY CASE[:JSON-KWARGS] ...

runs checks in a process of their own (the emulation aborts the process when a bound assert fires)."""
import ctypes
import functools
import json
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from mira_amd import _lib                                                    # noqa: E402
from mira_amd import fft as F                                                # noqa: E402
from mira_amd import fold as FD                                              # noqa: E402
from mira_amd import lookup as LU                                            # noqa: E402
from mira_amd.graph_evaluator import MODULUS                                 # noqa: E402

FIELD_FQ, FIELD_FR = 0, 1
FIELDS = (FIELD_FQ, FIELD_FR)
R = 1 << 256


# ---- the operands ---------------------------------------------------------------------------------------------------------------
def to_value(rep, field):
    """the canonical value a stored representation stands for"""
    p = MODULUS[field]
    return rep * pow(R, -1, p) % p


def from_value(value, field):
    """the stored (Montgomery) representation of a value"""
    p = MODULUS[field]
    return value % p * R % p


def all_ones_limbs(field):
    """limbs 0 .. 7 of the 9 x 29-bit form all ones, the top limb one below the modulus': the largest such canonical element"""
    top = MODULUS[field] >> 232
    return ((top - 1) << 232) | ((1 << 232) - 1)


def representations(field):
    p = MODULUS[field]
    reps = [0, 1, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, all_ones_limbs(field), (1 << 232) - 1, 1 << 232, (1 << 253) - 1, 1 << 253]
    for i in range(1, 9):
        reps += [(1 << (29 * i)) - 1, 1 << (29 * i)]
    reps += [(1 << (32 * i)) - 1 for i in range(1, 8)]
    reps += [from_value(1, field), from_value(p - 1, field), from_value(2, field), from_value(pow(2, -1, p), field)]
    out = []
    for r in reps:
        if r < p and r not in out:
            out.append(r)
    return out


def to_array(reps):
    reps = list(reps)
    if not reps:
        return np.zeros((0, 4), dtype=np.uint64)
    return np.frombuffer(b"".join(int(r).to_bytes(32, "little") for r in reps), dtype="<u8").astype(np.uint64).reshape(-1, 4)


def from_array(arr):
    raw = np.ascontiguousarray(arr, dtype="<u8").reshape(-1, 4).tobytes()
    return [int.from_bytes(raw[k:k + 32], "little") for k in range(0, len(raw), 32)]


def constant(v, n):
    return [v] * n


def alternating(v, w, n):
    """v at the even indices, w at the odd ones"""
    return [v if i % 2 == 0 else w for i in range(n)]


def ends(v, n, fill=0):
    """a single v at index 0 and another at index n - 1"""
    out = [fill] * n
    out[0] = out[n - 1] = v
    return out


def cycled(reps, n, start=0):
    return [reps[(start + i) % len(reps)] for i in range(n)]


def picked(reps, n, seed):
    rng = random.Random(seed)
    return [rng.choice(reps) for _ in range(n)]


def patterns(field, v, n, seed=0):
    """the six vector patterns of length n around one representation v"""
    reps = representations(field)
    p = MODULUS[field]
    return {"constant": constant(v, n), "alt_zero": alternating(v, 0, n), "alt_pm1": alternating(v, p - 1, n), "ends": ends(v, n),
            "cycled": cycled(reps, n, seed), "picked": picked(reps, n, seed)}


def holds_all(vector, field):
    """every representation of the list occurs in `vector`"""
    return set(representations(field)) <= set(vector)


class _Convert:
    """memoised conversions of one field (the vectors here repeat a few dozen representations)"""

    def __init__(self, field):
        self.field, self.p = field, MODULUS[field]
        self.rinv = pow(R, -1, self.p)
        self._v, self._inv = {}, {}

    def value(self, rep):
        v = self._v.get(rep)
        if v is None:
            v = self._v[rep] = rep * self.rinv % self.p
        return v

    def values(self, reps):
        return [self.value(r) for r in reps]

    def rep(self, value):
        return value % self.p * R % self.p

    def array(self, values):
        return to_array(self.rep(v) for v in values)

    def inv(self, value):
        """0 -> 0, like the kernels"""
        value %= self.p
        w = self._inv.get(value)
        if w is None:
            w = self._inv[value] = pow(value, -1, self.p) if value else 0
        return w


# ---- plumbing -------------------------------------------------------------------------------------------------------------------
class Dev:
    """device buffers of one check, released together"""

    def __init__(self, lib):
        self.lib, self.ptrs = lib, []

    def put(self, reps_or_array):
        arr = reps_or_array if isinstance(reps_or_array, np.ndarray) else to_array(reps_or_array)
        p = self.lib.alloc(max(1, arr.nbytes))
        if arr.nbytes:
            self.lib.upload(p, arr)
        self.ptrs.append(p)
        return p

    def empty(self, n):
        return self.put(np.full((max(1, n), 4), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64))

    def get(self, p, n):
        return self.lib.download(p, (n, 4)) if n else np.zeros((0, 4), dtype=np.uint64)

    def free(self):
        for p in self.ptrs:
            self.lib.free(p)
        self.ptrs = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()


def same_bytes(got, want, label, inputs=None):
    """== on bytes; a mismatch names the case, the first index and the operands there"""
    got, want = np.ascontiguousarray(got, dtype=np.uint64).reshape(-1, 4), np.ascontiguousarray(want, dtype=np.uint64).reshape(-1, 4)
    assert got.shape == want.shape, (label, got.shape, want.shape)
    bad = np.nonzero((got != want).any(axis=1))[0]
    if len(bad):
        i = int(bad[0])
        at = {} if inputs is None else {k: (hex(v[i]) if len(v) > i else None) for k, v in inputs.items()}
        raise AssertionError(f"{label}: {len(bad)} of {len(got)} elements differ, first at {i}: got {hex(from_array(got[i])[0])} "
                             f"want {hex(from_array(want[i])[0])} operands {at}")


class knobs:
    """mira_set_tuning for the length of a `with` block; every knob goes back to its default"""

    def __init__(self, lib, **values):
        self.lib, self.values = lib, {getattr(_lib, "TUNE_" + k): v for k, v in values.items() if v is not None}

    def __enter__(self):
        try:
            for k, v in self.values.items():
                self.lib.tune(k, v)
        except Exception:
            self.__exit__()
            raise
        return self

    def __exit__(self, *exc):
        for k in self.values:
            self.lib.tune(k, -1)


# ---- NTT over Fr ----------------------------------------------------------------------------------------------------------------
NTT_OPS = ("fft", "ifft", "coset_fft", "coset_ifft", "best_fft_inv")


def ntt_reference(op, a, k):
    from oracle import cref as C
    if op == "best_fft_inv":
        return C.best_fft(a, C.get_omega_or_inv(k, True), k)
    return getattr(C, op)(a, k)


def ntt_run(lib, op, a, k):
    from oracle import cref as C
    if op == "best_fft_inv":
        return F.best_fft(a, C.get_omega_or_inv(k, True), k, lib=lib)
    if op in ("fft", "ifft"):
        return getattr(F, op)(a, k, lib=lib)
    return getattr(F, op)(a, lib=lib)


def ntt_chosen():
    """the representations the single-v patterns of a transform are built around (each size starts at another one)"""
    reps = representations(FIELD_FR)
    p = MODULUS[FIELD_FR]
    strong = [p - 1, all_ones_limbs(FIELD_FR), (1 << 253) - 1, from_value(p - 1, FIELD_FR), p - 2, 1 << 253, (p + 1) // 2, (1 << 232) - 1]
    assert all(v in reps for v in strong)
    return strong


def ntt_inputs(k, width):
    """-> [(label, list of representations)]: `width` single-v pattern sets (4 vectors each) beside the cycled list and a seeded pick"""
    n, reps = 1 << k, representations(FIELD_FR)
    out = [("cycled", cycled(reps, n, k))]
    if n >= len(reps):
        assert holds_all(out[0][1], FIELD_FR)
    strong = ntt_chosen()
    for j in range(width):
        v = strong[(k + j) % len(strong)]
        pats = patterns(FIELD_FR, v, n)
        out += [(f"{name}[{hex(v)}]", pats[name]) for name in ("alt_pm1", "constant", "alt_zero", "ends")]
    out.insert(2, ("picked", picked(reps, n, 0xE0 + k)))
    return out


@functools.lru_cache(maxsize=None)
def ntt_roundtrip_case(k):
    """input = the oracle's ifft of a vector of extreme representations: the forward transform's OUTPUTS are then those
    representations themselves, exact zeros and p - 1 out of the final reduction among them"""
    from oracle import cref as C
    n, reps, p = 1 << k, representations(FIELD_FR), MODULUS[FIELD_FR]
    target = cycled(reps, n) if n >= len(reps) else alternating(p - 1, 0, n)
    x = C.ifft(to_array(target), k)
    want = C.fft(x, k)
    got_reps = from_array(want)
    assert got_reps == target                                             # the oracle inverts its own inverse
    assert 0 in got_reps and p - 1 in got_reps                            # ... and the case has not degraded
    return x, want


_ntt_cases = {}


def ntt_cases(k, width, ops):
    """-> [(label, representations, input array, {op: the oracle's output})]; computed once per process and shared by the knob settings"""
    have = _ntt_cases.setdefault((k, width), [(label, vec, to_array(vec), {}) for label, vec in ntt_inputs(k, width)])
    for _, _, a, refs in have:
        for op in ops:
            if op not in refs:
                refs[op] = ntt_reference(op, a, k)
                refs[op].setflags(write=False)
    return have


def check_ntt(lib, k, ops=NTT_OPS, width=1, wave=None, max_log_line=None, grid=None, roundtrip=True, limit=None):
    """`limit`: only the first so many input vectors (the emulation takes seconds per transform from 2^10 points up: the order
    is the cycled list, v alternating with p - 1, the seeded pick, then constant v, v alternating with 0, v at both ends)"""
    with knobs(lib, NTT_WAVE=wave, NTT_MAX_LOG_LINE=max_log_line, NTT_GRID=grid):
        tag = f"ntt k={k} wave={wave} max_log_line={max_log_line} grid={grid}"
        for label, vec, a, refs in ntt_cases(k, width, ops)[:limit]:
            for op in ops:
                same_bytes(ntt_run(lib, op, a, k), refs[op], f"{tag} {op} {label}", {"in": vec})
        if roundtrip:
            x, want = ntt_roundtrip_case(k)
            same_bytes(ntt_run(lib, "fft", x, k), want, f"{tag} fft(ifft(extremes))")


# ---- fold_witness / fold_error / fold_relaxed_witness ---------------------------------------------------------------------------
FOLD_LENGTHS = (1, 255, 256, 257, 1025)


def ref_fold_witness(cv, w1, w2, r):
    rv = cv.value(r)
    return cv.array((cv.value(a) + rv * cv.value(b)) % cv.p for a, b in zip(w1, w2))


def ref_fold_error(cv, e, terms, r):
    rv, p = cv.value(r), cv.p
    acc, pw = cv.values(e), rv
    for t in terms:
        acc = [(a + pw * cv.value(x)) % p for a, x in zip(acc, t)]
        pw = pw * rv % p
    return cv.array(acc)


def check_fold_pairs(lib, field):
    """fold_witness over ALL operand pairs of the list, for every r of the list; out of place and in place by turns"""
    cv, reps = _Convert(field), representations(field)
    w1 = [a for a in reps for _ in reps]
    w2 = [b for _ in reps for b in reps]
    n = len(w1)
    assert holds_all(w1, field) and holds_all(w2, field) and set(zip(w1, w2)) == {(a, b) for a in reps for b in reps}
    with Dev(lib) as dev:
        d1, d2, d_out, d_tmp = dev.put(w1), dev.put(w2), dev.empty(n), dev.empty(n)
        for j, r in enumerate(reps):
            want = ref_fold_witness(cv, w1, w2, r)
            if j % 2 == 0:
                FD.fold_witness_device(field, d_out, d1, d2, to_array([r]), n, lib=lib)
                got = dev.get(d_out, n)
            else:
                lib.copy(d_tmp, d1, n * 32)
                FD.fold_witness_device(field, d_tmp, d_tmp, d2, to_array([r]), n, lib=lib)
                got = dev.get(d_tmp, n)
            same_bytes(got, want, f"fold_witness field={field} r={hex(r)}", {"w1": w1, "w2": w2})
        same_bytes(dev.get(d1, n), to_array(w1), "fold_witness left w1 alone")


def fold_targets(field):
    """results the target cases must hit: representation 0, representation p - 1, and the value p - 1"""
    p = MODULUS[field]
    return [0, p - 1, from_value(p - 1, field)]


def check_fold_targets(lib, field):
    """w1 = t - r * w2 for every r and w2 of the list: the fold's result is exactly t, for t = 0, the representation p - 1
    and the value -1 (w1 = -r * w2 and w1 = -1 - r * w2)"""
    cv, reps, p = _Convert(field), representations(field), MODULUS[field]
    targets = fold_targets(field)
    with Dev(lib) as dev:
        for r in reps:
            w2 = [b for _ in targets for b in reps]
            w1 = [cv.rep(cv.value(t) - cv.value(r) * cv.value(b)) for t in targets for b in reps]
            want = ref_fold_witness(cv, w1, w2, r)
            assert from_array(want) == [t for t in targets for _ in reps]       # the REFERENCE result holds the exact 0 and p - 1
            assert {0, p - 1} <= set(from_array(want)) and holds_all(w2, field)
            d1, d2 = dev.put(w1), dev.put(w2)
            FD.fold_witness_device(field, d1, d1, d2, to_array([r]), len(w1), lib=lib)
            same_bytes(dev.get(d1, len(w1)), want, f"fold_witness to 0 / p-1, field={field} r={hex(r)}", {"w1": w1, "w2": w2})
            dev.free()


def fold_error_rs(field):
    p = MODULUS[field]
    return [0, 1, p - 1, all_ones_limbs(field), from_value(1, field), from_value(p - 1, field)]


def check_fold_lengths(lib, field, terms=16):
    """fold_witness, fold_error (16 terms) and fold_relaxed_witness at lengths around the block size, in place and out of place"""
    cv, reps, p = _Convert(field), representations(field), MODULUS[field]
    for n in FOLD_LENGTHS:
        n_w = {1: 257, 255: 1, 256: 1025, 257: 255, 1025: 256}[n]           # the witness half of the relaxed fold has a length of its own
        for j, r in enumerate(fold_error_rs(field)):
            e = cycled(reps, n, j) if j != 2 else constant(p - 1, n)
            ts = [cycled(reps, n, 5 * k + j + 1) if j != 2 else constant(p - 1, n) for k in range(terms)]
            w1, w2 = cycled(reps, n_w, 3 + j), picked(reps, n_w, 0xF0 + n + j)
            if n >= len(reps):
                assert holds_all(e, field) or j == 2
            want_e, want_w = ref_fold_error(cv, e, ts, r), ref_fold_witness(cv, w1, w2, r)
            label = f"field={field} n={n} r={hex(r)}"
            with Dev(lib) as dev:
                d_e, d_ts = dev.put(e), [dev.put(t) for t in ts]
                FD.fold_error_device(field, d_e, d_ts, to_array([r]), n, lib=lib)
                same_bytes(dev.get(d_e, n), want_e, "fold_error " + label, {"e": e, "t0": ts[0]})
                # the relaxed form: out of place, then in place (w_out = w1, e_out = e)
                d_e, d_w1, d_w2, d_eo, d_wo = dev.put(e), dev.put(w1), dev.put(w2), dev.empty(n), dev.empty(n_w)
                FD.fold_relaxed_witness_device(field, d_wo, d_w1, d_w2, n_w, d_eo, d_e, d_ts, to_array([r]), n, lib=lib)
                same_bytes(dev.get(d_eo, n), want_e, "fold_relaxed e " + label, {"e": e, "t0": ts[0]})
                same_bytes(dev.get(d_wo, n_w), want_w, "fold_relaxed w " + label, {"w1": w1, "w2": w2})
                same_bytes(dev.get(d_e, n), to_array(e), "fold_relaxed left e alone")
                FD.fold_relaxed_witness_device(field, d_w1, d_w1, d_w2, n_w, d_e, d_e, d_ts, to_array([r]), n, lib=lib)
                same_bytes(dev.get(d_e, n), want_e, "fold_relaxed e in place " + label, {"e": e, "t0": ts[0]})
                same_bytes(dev.get(d_w1, n_w), want_w, "fold_relaxed w in place " + label, {"w1": w1, "w2": w2})
                # fold_witness at this length, out of place
                d_w1, d_wo = dev.put(w1), dev.empty(n_w)
                FD.fold_witness_device(field, d_wo, d_w1, d_w2, to_array([r]), n_w, lib=lib)
                same_bytes(dev.get(d_wo, n_w), want_w, "fold_witness " + label, {"w1": w1, "w2": w2})


# ---- lincomb, lincomb_multi -----------------------------------------------------------------------------------------------------
def check_lincomb(lib, field, n=1025, num_vecs=16, num_outs=8):
    cv, reps, p = _Convert(field), representations(field), MODULUS[field]
    vec_sets = {"list": [cycled(reps, n, 7 * k) for k in range(num_vecs)], "all p-1": [constant(p - 1, n) for _ in range(num_vecs)]}
    assert all(holds_all(v, field) for v in vec_sets["list"])
    coeff_sets = [cycled(reps, num_vecs, s) for s in range(0, len(reps), num_vecs)]
    assert holds_all([c for cs in coeff_sets for c in cs], field)
    coeff_sets += [constant(p - 1, num_vecs), constant(from_value(p - 1, field), num_vecs), constant(all_ones_limbs(field), num_vecs)]
    multi_sets = [cycled(reps, num_outs * num_vecs, 0), constant(p - 1, num_outs * num_vecs), picked(reps, num_outs * num_vecs, 0x11C)]
    assert holds_all(multi_sets[0], field)

    def ref(vecs, coeffs):
        cvals, cols = cv.values(coeffs), [cv.values(v) for v in vecs]
        return cv.array(sum(c * col[i] for c, col in zip(cvals, cols)) % p for i in range(n))
    with Dev(lib) as dev:
        for name, vecs in vec_sets.items():
            d_vecs = [dev.put(v) for v in vecs]
            vp = (ctypes.c_void_p * num_vecs)(*d_vecs)
            d_outs = [dev.empty(n) for _ in range(num_outs)]
            for coeffs in coeff_sets:
                c = to_array(coeffs)
                lib.check(lib.c.mira_lincomb_device(field, ctypes.c_void_p(d_outs[0]), vp, c.ctypes.data_as(ctypes.c_void_p), num_vecs, n))
                same_bytes(dev.get(d_outs[0], n), ref(vecs, coeffs), f"lincomb field={field} vectors={name} coeffs={hex(coeffs[0])}..", {"v0": vecs[0]})
            for coeffs in multi_sets:
                c = to_array(coeffs)
                op = (ctypes.c_void_p * num_outs)(*d_outs)
                lib.check(lib.c.mira_lincomb_multi_device(field, op, num_outs, vp, num_vecs, c.ctypes.data_as(ctypes.c_void_p), n))
                for m in range(num_outs):
                    same_bytes(dev.get(d_outs[m], n), ref(vecs, coeffs[m * num_vecs:(m + 1) * num_vecs]),
                               f"lincomb_multi field={field} vectors={name} out={m} coeffs={hex(coeffs[0])}..", {"v0": vecs[0]})


# ---- pow_tree_reduce ------------------------------------------------------------------------------------------------------------
def ref_pow_tree(cv, leaves, weights):
    """tree_reduce with node = left + right * weights[height]"""
    nodes = cv.values(leaves)
    for w in cv.values(weights):
        nodes = [(nodes[i] + nodes[i + 1] * w) % cv.p for i in range(0, len(nodes), 2)]
    assert len(nodes) == 1
    return nodes[0]


def check_pow_tree(lib, field, points=4, sizes=(1, 6, 11)):
    """2^1, 2^6 and 2^11 leaves: one kernel round of 2, 64 and 256 lanes (2^11: eight leaves per lane first); 2^12 adds a second
    round.  From 2^11 leaves up (a quarter of a second per tree on the emulation) without the seeded picks."""
    cv, reps, p = _Convert(field), representations(field), MODULUS[field]
    for levels in sizes:
        n = 1 << levels
        weight_sets = {"list": cycled(reps, points * levels, levels), "picked": picked(reps, points * levels, levels)}
        for w in (0, 1, p - 1, from_value(1, field), from_value(p - 1, field)):
            weight_sets[f"all {hex(w)}"] = constant(w, points * levels)
        leaf_sets = {"list": cycled(reps, points * n, levels), "picked": picked(reps, points * n, 0x7EE + levels), "all p-1": constant(p - 1, points * n)}
        if levels >= 11:
            del leaf_sets["picked"], weight_sets["picked"]
        if points * levels >= len(reps):
            assert holds_all(weight_sets["list"], field)
        if points * n >= len(reps):
            assert holds_all(leaf_sets["list"], field)
        with Dev(lib) as dev:
            for lname, leaves in leaf_sets.items():
                d = dev.put(leaves)
                for wname, weights in weight_sets.items():
                    wa = to_array(weights)
                    for stride in (0, n):
                        out = np.zeros((points, 4), dtype=np.uint64)
                        lib.check(lib.c.mira_pow_tree_reduce_device(field, ctypes.c_void_p(d), n, stride, wa.ctypes.data_as(ctypes.c_void_p), points,
                                                                    out.ctypes.data_as(ctypes.c_void_p)))
                        want = cv.array(ref_pow_tree(cv, leaves[q * stride:q * stride + n], weights[q * levels:(q + 1) * levels]) for q in range(points))
                        same_bytes(out, want, f"pow_tree field={field} leaves=2^{levels} {lname} weights={wname} stride={stride}")


# ---- batch inversion, lookup h / g ----------------------------------------------------------------------------------------------
INV_LENGTHS = (1, 2047, 2048, 2049, 16385)            # the level boundaries of the inversion plan at the default 8 elements per lane


def check_batch_invert(lib, field, chunk=None):
    cv, reps, p = _Convert(field), representations(field), MODULUS[field]
    with knobs(lib, INV_CHUNK=chunk):
        cases = [(f"n={n}", cycled(reps, n, n)) for n in INV_LENGTHS]
        cases += [(f"single {hex(v)}", [v]) for v in reps]                  # the list as input, one element per call ...
        cases += [("list", list(reps)), ("zeros", constant(0, 300)), ("all p-1", constant(p - 1, 2049)), ("alt 0", alternating(p - 1, 0, 2049))]
        assert all(holds_all(x, field) for label, x in cases if label in ("n=2047", "n=2048", "n=2049", "n=16385", "list"))
        for label, x in cases:
            n = len(x)
            want = cv.array(cv.inv(cv.value(v)) for v in x)
            with Dev(lib) as dev:
                d_in, d_out = dev.put(x), dev.empty(n)
                LU.batch_invert_device(field, d_out, d_in, n, lib=lib)
                same_bytes(dev.get(d_out, n), want, f"batch_invert field={field} chunk={chunk} {label}", {"x": x})
                same_bytes(dev.get(d_in, n), to_array(x), "batch_invert left its input alone")
                LU.batch_invert_device(field, d_in, d_in, n, lib=lib)
                same_bytes(dev.get(d_in, n), want, f"batch_invert in place field={field} chunk={chunk} {label}", {"x": x})


def lookup_ms(field, n):
    """multiplicities: 0, 1, p - 1 and n as field elements, and the representations 1 and p - 1"""
    p = MODULUS[field]
    return [0, from_value(1, field), from_value(p - 1, field), from_value(n, field), 1, p - 1]


def check_lookup_h_g(lib, field, chunk=None):
    """h = 1 / (l + r), g = m / (t + r): l and t from the list with l_i + r = 0 and t_i + r = 0 planted, for every r of the list
    (r = 0 beside zero elements and r = -1 beside elements equal to 1 among them), then the level boundaries of the plan"""
    cv, reps, p = _Convert(field), representations(field), MODULUS[field]

    def run(label, l, t, m, r):
        rv = cv.value(r)
        want_h = cv.array(cv.inv(cv.value(v) + rv) for v in l)
        want_g = cv.array(cv.value(mv) * cv.inv(cv.value(tv) + rv) for mv, tv in zip(m, t))
        with Dev(lib) as dev:
            d_l, d_t, d_m, d_h, d_g = dev.put(l), dev.put(t), dev.put(m), dev.empty(len(l)), dev.empty(len(t))
            LU.evaluate_h_g_device(field, d_h, d_g, d_l, len(l), d_t, d_m, len(t), rv, lib=lib)
            same_bytes(dev.get(d_h, len(l)), want_h, f"lookup h field={field} chunk={chunk} {label}", {"l": l})
            same_bytes(dev.get(d_g, len(t)), want_g, f"lookup g field={field} chunk={chunk} {label}", {"t": t, "m": m})
        return want_h, want_g

    def planted(vec, r, every):
        minus_r = cv.rep(-cv.value(r))
        return [minus_r if i % every == 0 else v for i, v in enumerate(vec)]
    with knobs(lib, INV_CHUNK=chunk):
        n_l, n_t = 300, 277
        for j, r in enumerate(reps):
            l, t = planted(cycled(reps, n_l, j), r, 5), planted(picked(reps, n_t, 0x10 + j), r, 4)
            assert holds_all(l + [cv.rep(-cv.value(r))], field)
            m = cycled(lookup_ms(field, n_t), n_t)
            want_h, want_g = run(f"r={hex(r)}", l, t, m, r)
            assert not want_h[0].any() and not want_g[0].any()             # the planted zero denominators give 0
        assert 0 in reps and from_value(p - 1, field) in reps and from_value(1, field) in reps    # r = 0 with zeros, r = -1 with ones
        for n in INV_LENGTHS:                                               # one inversion over n_l + n_t elements
            for n_l in sorted({(n + 1) // 2, n, 0}):
                n_t = n - n_l
                for r in (0, from_value(p - 1, field), all_ones_limbs(field)):
                    l, t = planted(cycled(reps, n_l, n), r, 7), planted(cycled(reps, n_t, n + 5), r, 9)
                    run(f"n_l={n_l} n_t={n_t} r={hex(r)}", l, t, cycled(lookup_ms(field, n), n_t), r)


# ---- the graph evaluator --------------------------------------------------------------------------------------------------------
GRAPH_ROWS = 1 << 10
GRAPH_SEEDS = {FIELD_FR: 1, FIELD_FQ: 2}               # tests/test_gpu_graph.py's seeds for these fields


def graph_data(field, n=GRAPH_ROWS):
    """2 selectors, 3 fixed and 7 advice columns and 3 challenges, every element from the list.  fixed[0] is the representation
    p - 1 on every row, fixed[1] the value p - 1, advice[5] zero: the hand-written expressions chain them.
    -> (int getter for pyref.eval_expression, array getter for the device)"""
    cv, reps, p = _Convert(field), representations(field), MODULUS[field]
    rng = random.Random(0x6A + field)
    sel = [[rng.random() < 0.5 for _ in range(n)] for _ in range(2)]
    fix = [constant(p - 1, n), constant(from_value(p - 1, field), n), cycled(reps, n, 1)]
    adv = [alternating(p - 1, 0, n), alternating(all_ones_limbs(field), p - 1, n), ends((1 << 253) - 1, n), picked(reps, n, 0x6B + field),
           cycled(reps, n, 17), constant(0, n), picked(reps, n, 0x6C + field)]
    chal = [p - 1, all_ones_limbs(field), from_value(pow(2, -1, p), field)]
    assert holds_all(fix[2], field) and holds_all(adv[4], field) and all(c in reps for c in chal)
    ints = dict(selectors=sel, fixed=[cv.values(c) for c in fix], advice=[cv.values(c) for c in adv], challenges=cv.values(chal))
    arrs = dict(selectors=[np.array(s, dtype=np.uint8) for s in sel], fixed=[to_array(c) for c in fix], advice=[to_array(c) for c in adv],
                challenges=ints["challenges"])
    return ints, arrs


def graph_expressions(field, group):
    """group "gate": the gate-like graphs of tests/test_gpu_graph.py (same seed, same sizes); "chain": small expressions that chain
    the worst case -- a depth-12 product and six squarings of (p - 1)-valued columns, a sum of 32 of them,
    Negated of 0 and of p - 1, Scaled by p - 1"""
    from graph_cases import gate_like_expression
    from harness import graph_evaluator as G
    p = MODULUS[field]
    if group == "gate":
        rng = random.Random(GRAPH_SEEDS[field])
        return [(f"gate-like {nterms} terms", gate_like_expression(rng, nterms, 7, 12, 3)) for nterms in (1, 5, 24)]
    col = lambda kind, k, rot=0: G.Polynomial({"fixed": 2, "advice": 5}[kind] + k, rot)
    pm1 = [col("fixed", 0), col("fixed", 1), col("fixed", 0, 1), col("fixed", 1, -1), col("advice", 1), col("advice", 1, 1)]   # reps p-1 / values p-1 / both by turns
    prod = pm1[0]
    for k in range(1, 13):
        prod = G.Product(prod, pm1[k % len(pm1)])
    tower = G.Sum(col("fixed", 0), col("advice", 0, -1))
    for _ in range(6):                                  # (the Python-integer reference walks the tree: 2^6 leaves per row)
        tower = G.Product(tower, tower)
    total = pm1[0]
    for k in range(1, 32):
        total = G.Sum(total, pm1[k % len(pm1)])
    zero, list_col = col("advice", 5), col("fixed", 2)
    negs = G.Sum(G.Sum(G.Negated(zero), G.Negated(col("fixed", 0))), G.Product(G.Negated(col("fixed", 1)), G.Negated(list_col)))
    scaled = G.Sum(G.Scaled(list_col, p - 1), G.Product(G.Scaled(col("fixed", 0), p - 1), G.Scaled(G.Challenge(0), p - 1)))
    return [("product of 13 columns at p-1", prod), ("six squarings", tower), ("sum of 32 columns at p-1", total), ("Negated of 0 and p-1", negs),
            ("Negated(0) alone", G.Negated(zero)), ("Negated(p-1) alone", G.Negated(col("fixed", 1))), ("Scaled by p-1", scaled),
            ("all of them", G.Sum(G.Sum(prod, tower), G.Sum(total, G.Sum(negs, scaled))))]


_graph_reference = {}


def graph_reference(field, group):
    """-> [(label, expression, expected (n, 4) array)], from Python integers on EVERY row; computed once per process"""
    from oracle import pyref as P
    key = (field, group)
    if key not in _graph_reference:
        cv = _Convert(field)
        ints, _ = graph_data(field)
        out = []
        for label, e in graph_expressions(field, group):
            tree = e.to_tuple()
            out.append((label, e, cv.array(P.eval_expression(tree, ints, row, GRAPH_ROWS, cv.p) for row in range(GRAPH_ROWS))))
        _graph_reference[key] = out
    return _graph_reference[key]


def check_graph(lib, field, group, specialise=False, only=None):
    """every expression of the group (or those at the indices `only`) through the one-shot interpreter (mira_graph_eval_device), the
    compiled engine (mira_graph_eval_compiled) and its batch; with `specialise`, through kernels of their own as well
    (mira_graph_specialize: GPU only -- the run-time compiler takes seconds per gate-sized graph)"""
    from harness import graph_evaluator as G
    n = GRAPH_ROWS
    _, arrs = graph_data(field)
    chal = arrs["challenges"]
    cases = graph_reference(field, group)
    cases = cases if only is None else [cases[k] for k in only]
    assert cases
    with Dev(lib) as dev:
        cols = [(dev.put(s), G.COL_BOOL) for s in arrs["selectors"]] + [(dev.put(c), G.COL_FIELD) for c in arrs["fixed"] + arrs["advice"]]
        table = G.GraphEvaluator._column_table(cols)
        chal_m = G.to_montgomery(chal, field)
        evs = [G.GraphEvaluator.new(e, field) for _, e, _ in cases]
        try:
            d_all = dev.empty(len(evs) * n)
            for (label, _, want), ev in zip(cases, evs):
                code, consts, rots = ev.flatten()
                g = _lib.MiraGraph(code.ctypes.data, len(code), ev.num_intermediates, len(consts), consts.ctypes.data, rots.ctypes.data, len(rots), 0)
                lib.check(lib.c.mira_graph_eval_device(field, ctypes.byref(g), table, len(cols), chal_m.ctypes.data_as(ctypes.c_void_p), len(chal), n,
                                                       ctypes.c_void_p(d_all)))
                same_bytes(dev.get(d_all, n), want, f"graph one-shot field={field} {label}")
                ev.evaluate_device(cols, chal, n, d_out=d_all, lib=lib)
                same_bytes(dev.get(d_all, n), want, f"graph compiled field={field} {label}")

            def batch(tag):
                G.GraphEvaluator.evaluate_batch_device(evs, cols, chal, n, [d_all + k * n * 32 for k in range(len(evs))], lib=lib)
                got = dev.get(d_all, len(evs) * n).reshape(len(evs), n, 4)
                for k, (label, _, want) in enumerate(cases):
                    same_bytes(got[k], want, f"graph {tag} field={field} {label}")
            batch("batch")
            if specialise:
                assert G.GraphEvaluator.specialize(evs, cols, len(chal), lib=lib), lib.c.mira_last_error()
                assert all(ev.is_specialized(len(chal), len(cols), lib=lib) for ev in evs)
                for (label, _, want), ev in zip(cases, evs):
                    ev.evaluate_device(cols, chal, n, d_out=d_all, lib=lib)
                    same_bytes(dev.get(d_all, n), want, f"graph specialised field={field} {label}")
                batch("specialised batch")
        finally:
            for ev in evs:
                ev.close()


CASES = {"ntt": check_ntt, "fold_pairs": check_fold_pairs, "fold_targets": check_fold_targets, "fold_lengths": check_fold_lengths,
         "lincomb": check_lincomb, "pow_tree": check_pow_tree, "batch_invert": check_batch_invert, "lookup_h_g": check_lookup_h_g,
         "graph": check_graph}


def main(argv):
    lib = _lib.MiraLib(argv[1])
    for spec in argv[2:]:
        name, _, kwargs = spec.partition(":")
        CASES[name](lib, **(json.loads(kwargs) if kwargs else {}))
        print(f"ok {spec}", flush=True)


if __name__ == "__main__":
    main(sys.argv)
