"""Guard bands around every device-resident call.

The value tests of this suite compare the n elements a call was asked to produce and nothing else, with most operands at the
base of an allocation of their own.  A tail lane that stores one element past n, a tile copy that runs a column too far or a
load of t[n] lands in allocator slack and is never seen.  Here every operand of a call lies inside ONE allocation:

    Arena(lib, guard_elems=2048)      one lib.alloc; place(array_or_n, offset_elems) lays operands out inside it
      * before and after every operand lie guard_elems guard elements of 32 bytes (64 KiB: the widest overrun a tail can make,
        256 lanes x 8 elements x 32 bytes);
      * offset_elems shifts an operand by 0, 1 or 3 elements from a 256-byte-aligned position (byte offsets 0, 32, 96): the
        kernels load 16-byte vectors, so element alignment is all the ABI promises;
      * every guard element is unique and non-canonical -- top limb 0xFFFFFFFFFFFFFFFF, the low limbs a counter of its position
        in the arena: a stray copy of neighbouring data is seen, and an over-read (>= 2^255 > p) trips the kernels' own checks
        of canonical inputs or changes a sum, a count or a value;
      * check(call, written=[...]) downloads the whole arena once, asserts every guard byte and every operand not named in
        `written` unchanged, and returns the written operands for the value comparison.  A failure names the call, the operand
        and the first changed byte relative to the operand's end or start.

The check_* drivers run one family of calls each at the lengths around the block sizes and at the three offsets, on whichever
library they are handed (the GPU build or the CPU emulation).  Expected values never come from the library: Python integers
(edge_operands' references, test_lookup_witness_emu's ref_m / ref_h_g, pyref.eval_expression, setup_ref) and, for the
transforms, the synthetic inputs and the commitments, the C oracle.  Every comparison is on bytes; there is no tolerance here."""
import contextlib
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import edge_operands as E                                                    # noqa: E402
from mira_amd import _lib                                                    # noqa: E402
from mira_amd import commitment as CM                                        # noqa: E402
from mira_amd import decider as DC                                           # noqa: E402
from mira_amd import fft as F                                                # noqa: E402
from mira_amd import fold as FD                                              # noqa: E402
from mira_amd import lookup as LU                                            # noqa: E402
from mira_amd.graph_evaluator import MODULUS                                 # noqa: E402

ELEM = 32
OFFSETS = (0, 1, 3)                                    # elements past a 256-byte boundary: byte offsets 0, 32, 96
ALL_ONES = 0xFFFFFFFFFFFFFFFF


def guard_fill(first, count):
    """guard elements first .. first + count - 1 of an arena, (count, 4) uint64: [i, i * golden ratio, i, all ones]"""
    i = np.arange(first, first + count, dtype=np.uint64)
    out = np.empty((count, 4), dtype=np.uint64)
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = i, i * np.uint64(0x9E3779B97F4A7C15), i, np.uint64(ALL_ONES)
    return out


class Operand:
    """`nbytes` bytes of an arena from element `start` on"""

    def __init__(self, arena, name, start, nbytes):
        self.arena, self.name, self.start, self.nbytes = arena, name, start, nbytes

    @property
    def lo(self):
        return self.start * ELEM

    @property
    def hi(self):
        return self.start * ELEM + self.nbytes

    @property
    def ptr(self):
        return self.arena.origin + self.lo


class Arena:
    def __init__(self, lib, guard_elems=2048):
        self.lib, self.guard = lib, guard_elems
        self.ops, self.pending, self.cursor = [], [], 0
        self.base = self.image = None

    # ---- layout ----
    def place(self, array_or_n, offset_elems=0, name=None):
        """an operand holding `array` (any dtype; its bytes) or of n elements of 32 bytes left as guard fill (an output: an element
        the call does not write stays non-canonical and fails the value comparison)"""
        assert self.base is None, "place every operand before the first use of the arena"
        assert 0 <= offset_elems < 8
        if isinstance(array_or_n, (int, np.integer)):
            data, nbytes = None, int(array_or_n) * ELEM
        else:
            data = np.ascontiguousarray(array_or_n).view(np.uint8).reshape(-1)
            nbytes = data.nbytes
        start = (self.cursor + self.guard + 7) // 8 * 8 + offset_elems
        op = Operand(self, name or f"operand{len(self.ops)}", start, nbytes)
        self.cursor = start + (nbytes + ELEM - 1) // ELEM
        self.ops.append(op)
        self.pending.append(data)
        return op

    def _ensure(self):
        if self.base is not None:
            return
        total = self.cursor + self.guard
        self.base = self.lib.alloc(total * ELEM + 256)
        self._origin = (self.base + 255) // 256 * 256                     # offsets count from a 256-byte boundary whatever the allocator gives
        self.image = guard_fill(0, total).view(np.uint8).reshape(-1).copy()
        for op, data in zip(self.ops, self.pending):
            if data is not None:
                self.image[op.lo:op.hi] = data
        self.pending = None
        self.lib.upload(self._origin, self.image)

    @property
    def origin(self):
        self._ensure()
        return self._origin

    def write(self, op, array, elem=0):
        """new contents for (part of) an operand, from element `elem` on"""
        self._ensure()
        data = np.ascontiguousarray(array).view(np.uint8).reshape(-1)
        lo = op.lo + elem * ELEM
        assert lo + data.nbytes <= op.hi
        self.image[lo:lo + data.nbytes] = data
        if data.nbytes:
            self.lib.upload(self.origin + lo, data)

    def clear(self, op):
        """back to guard fill (an output before the next call)"""
        self._ensure()
        first, count = op.start, (op.nbytes + ELEM - 1) // ELEM
        self.write(op, guard_fill(first, count).view(np.uint8).reshape(-1)[:op.nbytes])

    # ---- the check ----
    def _where(self, b):
        """names byte b of the arena: inside an operand, or in the guard band next to the nearer one"""
        before = after = None
        for op in self.ops:
            if op.lo <= b < op.hi:
                return f"operand '{op.name}' (not an output of this call) changed at byte {b - op.lo} of {op.nbytes}"
            if op.hi <= b and (before is None or op.hi > before.hi):
                before = op
            if op.lo > b and (after is None or op.lo < after.lo):
                after = op
        if before is not None and (after is None or b - before.hi < after.lo - b):
            return f"guard after operand '{before.name}' changed at byte +{b - before.hi} past its end (element +{(b - before.hi) // ELEM})"
        return f"guard before operand '{after.name}' changed at byte -{after.lo - b} before its start (element -{(after.lo - b + ELEM - 1) // ELEM})"

    def check(self, call, written=()):
        """-> [the bytes of each written operand as uint8 arrays]; everything else in the arena must be as it was"""
        self._ensure()
        got = self.lib.download(self.origin, self.image.shape, np.uint8)
        for op in written:
            self.image[op.lo:op.hi] = got[op.lo:op.hi]
        if not np.array_equal(got.view(np.uint64), self.image.view(np.uint64)):
            bad = np.nonzero(got != self.image)[0]
            raise AssertionError(f"{call}: {self._where(int(bad[0]))} first; {len(bad)} bytes changed in all, the last: {self._where(int(bad[-1]))}")
        return [got[op.lo:op.hi] for op in written]

    @contextlib.contextmanager
    def reading(self, call):
        """around a call that checks its inputs: every operand placed here is canonical, so a complaint about a non-canonical
        element means that the call read guard fill"""
        try:
            yield
        except _lib.MiraError as err:
            if "canonical" not in str(err):
                raise
            raise AssertionError(f"{call}: read outside its operands: it met a non-canonical element, which only the guard bands hold ({err})") from err

    def free(self):
        if self.base is not None:
            self.lib.free(self.base)
            self.base = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()


def elems(raw):
    return np.ascontiguousarray(raw).view(np.uint64).reshape(-1, 4)


def same(raw, want, label, inputs=None):
    E.same_bytes(elems(raw), want, label, inputs)


def shifted(offset, j):
    """operand j of a call at offset setting `offset`: the operands of one call take different offsets by turns"""
    return OFFSETS[(OFFSETS.index(offset) + j) % len(OFFSETS)]


def cycled_array(field, n, start=0):
    """E.to_array(E.cycled(representations(field), n, start)) without a Python loop over n"""
    reps = E.to_array(E.representations(field))
    return reps[(start + np.arange(n)) % len(reps)]


def vp(x):
    return x.ctypes.data_as(ctypes.c_void_p)


# ---- fold -----------------------------------------------------------------------------------------------------------------------
LENGTHS = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025)


def check_fold(lib, field, lengths=LENGTHS, offsets=OFFSETS):
    """fold_witness (out of place, in place), fold_error with 1 and 16 terms, fold_relaxed_witness with n_w != n (out of place, in place)"""
    cv, reps = E._Convert(field), E.representations(field)
    for n in lengths:
        n_w = n + 2 if n % 2 else max(1, n - 3)                           # the witness half has a length of its own, odd and even by turns
        r = reps[(5 + n) % len(reps)]
        ra = E.to_array([r])
        w1, w2, e = E.cycled(reps, n, n), E.picked(reps, n, 0xF0 + n), E.cycled(reps, n, 3)
        ts = [E.cycled(reps, n, 5 * k + 1) for k in range(16)]
        v1, v2 = E.cycled(reps, n_w, 11), E.cycled(reps, n_w, 23)
        want_w, want_v = E.ref_fold_witness(cv, w1, w2, r), E.ref_fold_witness(cv, v1, v2, r)
        want_e = {k: E.ref_fold_error(cv, e, ts[:k], r) for k in (1, 16)}
        for off in offsets:
            tag = f"field={field} n={n} offset={off}"
            with Arena(lib) as A:
                a1, a2, out = A.place(E.to_array(w1), shifted(off, 0), "w1"), A.place(E.to_array(w2), shifted(off, 1), "w2"), A.place(n, shifted(off, 2), "out")
                FD.fold_witness_device(field, out.ptr, a1.ptr, a2.ptr, ra, n, lib=lib)
                got, = A.check(f"fold_witness {tag}", [out])
                same(got, want_w, f"fold_witness {tag}", {"w1": w1, "w2": w2})
                FD.fold_witness_device(field, a1.ptr, a1.ptr, a2.ptr, ra, n, lib=lib)
                got, = A.check(f"fold_witness in place {tag}", [a1])
                same(got, want_w, f"fold_witness in place {tag}", {"w1": w1, "w2": w2})
            for terms in (1, 16):
                with Arena(lib) as A:
                    ae = A.place(E.to_array(e), shifted(off, 0), "e")
                    ats = [A.place(E.to_array(t), shifted(off, 1 + k), f"t{k}") for k, t in enumerate(ts[:terms])]
                    FD.fold_error_device(field, ae.ptr, [t.ptr for t in ats], ra, n, lib=lib)
                    got, = A.check(f"fold_error terms={terms} {tag}", [ae])
                    same(got, want_e[terms], f"fold_error terms={terms} {tag}", {"e": e, "t0": ts[0]})
            with Arena(lib) as A:
                b1, b2, wo = A.place(E.to_array(v1), shifted(off, 1), "w1"), A.place(E.to_array(v2), shifted(off, 2), "w2"), A.place(n_w, shifted(off, 0), "w_out")
                ae, eo = A.place(E.to_array(e), shifted(off, 2), "e"), A.place(n, shifted(off, 1), "e_out")
                ats = [A.place(E.to_array(t), shifted(off, k), f"t{k}") for k, t in enumerate(ts)]
                tp = [t.ptr for t in ats]
                FD.fold_relaxed_witness_device(field, wo.ptr, b1.ptr, b2.ptr, n_w, eo.ptr, ae.ptr, tp, ra, n, lib=lib)
                gw, ge = A.check(f"fold_relaxed n_w={n_w} {tag}", [wo, eo])
                same(gw, want_v, f"fold_relaxed w n_w={n_w} {tag}", {"w1": v1, "w2": v2})
                same(ge, want_e[16], f"fold_relaxed e {tag}", {"e": e, "t0": ts[0]})
                FD.fold_relaxed_witness_device(field, b1.ptr, b1.ptr, b2.ptr, n_w, ae.ptr, ae.ptr, tp, ra, n, lib=lib)
                gw, ge = A.check(f"fold_relaxed in place n_w={n_w} {tag}", [b1, ae])
                same(gw, want_v, f"fold_relaxed w in place n_w={n_w} {tag}", {"w1": v1, "w2": v2})
                same(ge, want_e[16], f"fold_relaxed e in place {tag}", {"e": e, "t0": ts[0]})


# ---- lincomb, lincomb_multi -----------------------------------------------------------------------------------------------------
def check_lincomb(lib, field, lengths=LENGTHS, offsets=OFFSETS, num_outs=8, num_vecs=16):
    """lincomb with K = 1 and 16 vectors, lincomb_multi with M = 8 outputs of J = 16 vectors"""
    cv, reps, p = E._Convert(field), E.representations(field), MODULUS[field]
    coeffs = E.cycled(reps, num_outs * num_vecs, 2)
    ca, cvals = E.to_array(coeffs), cv.values(coeffs)
    for n in lengths:
        vecs = [E.cycled(reps, n, 7 * k + n) for k in range(num_vecs)]
        cols = [cv.values(v) for v in vecs]

        def ref(row, count):
            return cv.array(sum(c * col[i] for c, col in zip(cvals[row * num_vecs:row * num_vecs + count], cols)) % p for i in range(n))
        want1, want16 = ref(0, 1), [ref(m, num_vecs) for m in range(num_outs)]
        for off in offsets:
            tag = f"field={field} n={n} offset={off}"
            with Arena(lib) as A:
                av = [A.place(E.to_array(v), shifted(off, k), f"v{k}") for k, v in enumerate(vecs)]
                outs = [A.place(n, shifted(off, k + 1), f"out{k}") for k in range(num_outs)]
                ptrs = (ctypes.c_void_p * num_vecs)(*[v.ptr for v in av])
                for count, want in ((1, want1), (num_vecs, want16[0])):
                    A.clear(outs[0])
                    lib.check(lib.c.mira_lincomb_device(field, ctypes.c_void_p(outs[0].ptr), ptrs, vp(ca), count, n))
                    got, = A.check(f"lincomb K={count} {tag}", [outs[0]])
                    same(got, want, f"lincomb K={count} {tag}", {"v0": vecs[0]})
                A.clear(outs[0])
                op = (ctypes.c_void_p * num_outs)(*[o.ptr for o in outs])
                lib.check(lib.c.mira_lincomb_multi_device(field, op, num_outs, ptrs, num_vecs, vp(ca), n))
                for m, got in enumerate(A.check(f"lincomb_multi {tag}", outs)):
                    same(got, want16[m], f"lincomb_multi out={m} {tag}", {"v0": vecs[0]})


# ---- batch inversion ------------------------------------------------------------------------------------------------------------
INV_LENGTHS = (1, 7, 2047, 2048, 2049, 16385)


def check_batch_invert(lib, field, lengths=INV_LENGTHS, offsets=OFFSETS, chunks=(None, 3)):
    cv, reps = E._Convert(field), E.representations(field)
    for n in lengths:
        x = E.cycled(reps, n, n)
        want = cv.array(cv.inv(cv.value(v)) for v in x)
        for chunk in chunks:
            with E.knobs(lib, INV_CHUNK=chunk):
                for off in offsets:
                    tag = f"field={field} n={n} chunk={chunk} offset={off}"
                    with Arena(lib) as A:
                        src, dst = A.place(E.to_array(x), shifted(off, 0), "in"), A.place(n, shifted(off, 1), "out")
                        with A.reading(f"batch_invert {tag}"):
                            LU.batch_invert_device(field, dst.ptr, src.ptr, n, lib=lib)
                        got, = A.check(f"batch_invert {tag}", [dst])
                        same(got, want, f"batch_invert {tag}", {"x": x})
                        with A.reading(f"batch_invert in place {tag}"):
                            LU.batch_invert_device(field, src.ptr, src.ptr, n, lib=lib)
                        got, = A.check(f"batch_invert in place {tag}", [src])
                        same(got, want, f"batch_invert in place {tag}", {"x": x})


# ---- the lookup argument's m, h and g -------------------------------------------------------------------------------------------
LOOKUP_SHAPES = ((1, 1), (65, 63), (257, 255), (1025, 2049), (2049, 64))


def lookup_case(field, n_l, n_t):
    """t: the list with repeats; l: mostly values of t, every seventh absent from it (representations 2^k + 5 are not of the list)"""
    reps = E.representations(field)
    distinct = max(1, min(len(reps), n_t // 2))
    t = E.picked(reps[:distinct], n_t, 0x70 + n_t) if n_t > 1 else [reps[3]]
    absent = [(1 << 200) + 5, (1 << 100) + 5, 6]
    assert not set(absent) & set(reps)
    l = [absent[i % 3] if i % 7 == 6 else t[(5 * i) % n_t] for i in range(n_l)]
    return l, t


def check_lookup(lib, field, shapes=LOOKUP_SHAPES, offsets=OFFSETS, hashes=(None, 1)):
    from test_lookup_witness_emu import ref_h_g, ref_m
    cv, p = E._Convert(field), MODULUS[field]
    for n_l, n_t in shapes:
        l, t = lookup_case(field, n_l, n_t)
        m_ints = ref_m(l, t)                                               # equality is decided on the representation
        assert n_l < 7 or (sum(m_ints) < n_l and len(set(t)) < max(2, n_t))     # absent values and repeats are there
        want_m = cv.array(m_ints)
        reps = E.representations(field)
        r = cv.value(reps[(n_l + 9) % len(reps)])
        h_ints, g_ints = ref_h_g(cv.values(l), cv.values(t), m_ints, r, p)
        want_h, want_g = cv.array(h_ints), cv.array(g_ints)
        for off in offsets:
            tag = f"field={field} n_l={n_l} n_t={n_t} offset={off}"
            for mode in hashes:
                with E.knobs(lib, LOOKUP_HASH=mode), Arena(lib) as A:
                    al, at, am = A.place(E.to_array(l), shifted(off, 0), "l"), A.place(E.to_array(t), shifted(off, 1), "t"), A.place(n_t, shifted(off, 2), "m")
                    with A.reading(f"lookup_m hash={mode} {tag}"):
                        LU.evaluate_m_device(field, am.ptr, al.ptr, n_l, at.ptr, n_t, lib=lib)
                    got, = A.check(f"lookup_m hash={mode} {tag}", [am])
                    same(got, want_m, f"lookup_m hash={mode} {tag}", {"t": t})
            with Arena(lib) as A:
                al, at, am = A.place(E.to_array(l), shifted(off, 0), "l"), A.place(E.to_array(t), shifted(off, 1), "t"), A.place(want_m, shifted(off, 2), "m")
                ah, ag = A.place(n_l, shifted(off, 1), "h"), A.place(n_t, shifted(off, 0), "g")
                with A.reading(f"lookup_h_g {tag}"):
                    LU.evaluate_h_g_device(field, ah.ptr, ag.ptr, al.ptr, n_l, at.ptr, am.ptr, n_t, r, lib=lib)
                gh, gg = A.check(f"lookup_h_g {tag}", [ah, ag])
                same(gh, want_h, f"lookup h {tag}", {"l": l})
                same(gg, want_g, f"lookup g {tag}", {"t": t})


# ---- the deciders ---------------------------------------------------------------------------------------------------------------
DECIDE_LENGTHS = (1, 255, 257, 1025, 4097)


def check_deciders(lib, field, lengths=DECIDE_LENGTHS, offsets=OFFSETS):
    """count_ne (b given and NULL), sum_sub (b given and NULL), perm_check: nothing is written, so every operand and every guard
    must be as it was -- and the guard fill after a[n - 1] (non-canonical, non-zero, unequal to everything) in no count or sum"""
    cv, reps, p = E._Convert(field), E.representations(field), MODULUS[field]
    for n in lengths:
        a = E.cycled(reps, n, n)
        b = [reps[(i + n + (i % 5 == 4 or i == n - 1)) % len(reps)] for i in range(n)]          # differs at every fifth index and at the last
        diff = [i for i in range(n) if a[i] != b[i]]
        nz = [i for i in range(n) if a[i] != 0]
        want_ne, want_nz = (len(diff), diff[0] if diff else DC.NONE), (len(nz), nz[0] if nz else DC.NONE)
        sa, sb = sum(cv.values(a)) % p, sum(cv.values(b)) % p
        want_sub, want_sum = cv.array([sa - sb]), cv.array([sa])
        # Z = 2 instance elements || the n elements of d_w; y_i = Z[src_i] for a permutation src that moves both ends of d_w
        num_io = 2
        inst = [reps[7], reps[8]]
        z = inst + a
        src = list(range(n + num_io))
        for i in range(0, n + num_io - 1, 3):                             # neighbours swapped at every third index ...
            src[i], src[i + 1] = src[i + 1], src[i]
        src[n + num_io - 1], src[0] = src[0], src[n + num_io - 1]          # ... and the last element of d_w with an instance element
        bad = [i for i in range(n + num_io) if z[src[i]] != z[i]]
        want_perm = (len(bad), bad[0] if bad else DC.NONE)
        perm = DC.PermutationMatrix(field, [(i, s) for i, s in enumerate(src)], n + num_io, lib=lib)
        try:
            for off in offsets:
                tag = f"field={field} n={n} offset={off}"
                with Arena(lib) as A:
                    aa, ab = A.place(E.to_array(a), shifted(off, 0), "a"), A.place(E.to_array(b), shifted(off, 1), "b")
                    with A.reading(f"count_ne {tag}"):
                        assert DC.count_ne_device(field, aa.ptr, ab.ptr, n, lib=lib) == want_ne, f"count_ne {tag}"
                    A.check(f"count_ne {tag}")
                    with A.reading(f"count_ne b=NULL {tag}"):
                        assert DC.count_ne_device(field, aa.ptr, None, n, lib=lib) == want_nz, f"count_ne b=NULL {tag}"
                    A.check(f"count_ne b=NULL {tag}")
                    with A.reading(f"sum_sub {tag}"):
                        same(DC.sum_sub_device(field, aa.ptr, ab.ptr, n, lib=lib), want_sub, f"sum_sub {tag}")
                    A.check(f"sum_sub {tag}")
                    with A.reading(f"sum_sub b=NULL {tag}"):
                        same(DC.sum_sub_device(field, aa.ptr, None, n, lib=lib), want_sum, f"sum_sub b=NULL {tag}")
                    A.check(f"sum_sub b=NULL {tag}")
                    with A.reading(f"perm_check {tag}"):
                        assert perm.check_device(E.to_array(inst), aa.ptr, n) == want_perm, f"perm_check {tag}"
                    A.check(f"perm_check {tag}")
        finally:
            perm.close()


# ---- pow_tree_reduce ------------------------------------------------------------------------------------------------------------
def check_pow_tree(lib, field, sizes=(1, 6, 11), offsets=OFFSETS, points=4):
    cv, reps = E._Convert(field), E.representations(field)
    for levels in sizes:
        n = 1 << levels
        leaves, weights = E.cycled(reps, points * n, levels), E.cycled(reps, points * levels, levels + 3)
        wa = E.to_array(weights)
        want = {s: cv.array(E.ref_pow_tree(cv, leaves[q * s:q * s + n], weights[q * levels:(q + 1) * levels]) for q in range(points)) for s in (0, n)}
        for off in offsets:
            for stride in (0, n):
                tag = f"pow_tree field={field} leaves=2^{levels} stride={stride} offset={off}"
                # stride 0: the operand ends after the n leaves every point shares
                with Arena(lib) as A:
                    al = A.place(E.to_array(leaves[:points * n if stride else n]), off, "leaves")
                    out = np.zeros((points, 4), dtype=np.uint64)
                    lib.check(lib.c.mira_pow_tree_reduce_device(field, ctypes.c_void_p(al.ptr), n, stride, vp(wa), points, vp(out)))
                    A.check(tag)
                    same(out, want[stride], tag)


# ---- the graph evaluator --------------------------------------------------------------------------------------------------------
def check_graph(lib, field, group="chain", offsets=OFFSETS):
    """one-shot, compiled and batched evaluation with every column and every output between guards: the chained expressions read
    columns at rotations +1 and -1, so row n - 1 reads row 0 and row 0 reads row n - 1 -- an unreduced row index reads guard fill,
    which is non-canonical and changes the value"""
    from harness import graph_evaluator as G
    n = E.GRAPH_ROWS
    _, arrs = E.graph_data(field)
    chal = arrs["challenges"]
    cases = E.graph_reference(field, group)
    chal_m = G.to_montgomery(chal, field)
    for off in offsets:
        tag = f"field={field} offset={off}"
        with Arena(lib) as A:
            kinds = [G.COL_BOOL] * len(arrs["selectors"]) + [G.COL_FIELD] * len(arrs["fixed"] + arrs["advice"])
            placed = [A.place(c, shifted(off, j), f"column{j}") for j, c in enumerate(arrs["selectors"] + arrs["fixed"] + arrs["advice"])]
            outs = [A.place(n, shifted(off, j + 1), f"out{j}") for j in range(len(cases))]
            cols = [(c.ptr, kind) for c, kind in zip(placed, kinds)]
            table = G.GraphEvaluator._column_table(cols)
            evs = [G.GraphEvaluator.new(e, field) for _, e, _ in cases]
            try:
                for (label, _, want), ev, out in zip(cases, evs, outs):
                    code, consts, rots = ev.flatten()
                    g = _lib.MiraGraph(code.ctypes.data, len(code), ev.num_intermediates, len(consts), consts.ctypes.data, rots.ctypes.data, len(rots), 0)
                    lib.check(lib.c.mira_graph_eval_device(field, ctypes.byref(g), table, len(cols), vp(chal_m), len(chal), n, ctypes.c_void_p(out.ptr)))
                    got, = A.check(f"graph one-shot {tag} {label}", [out])
                    same(got, want, f"graph one-shot {tag} {label}")
                    A.clear(out)
                    ev.evaluate_device(cols, chal, n, d_out=out.ptr, lib=lib)
                    got, = A.check(f"graph compiled {tag} {label}", [out])
                    same(got, want, f"graph compiled {tag} {label}")
                    A.clear(out)
                G.GraphEvaluator.evaluate_batch_device(evs, cols, chal, n, [o.ptr for o in outs], lib=lib)
                for (label, _, want), got in zip(cases, A.check(f"graph batch {tag}", outs)):
                    same(got, want, f"graph batch {tag} {label}")
            finally:
                for ev in evs:
                    ev.close()


# ---- the generators -------------------------------------------------------------------------------------------------------------
GEN_LENGTHS = (1, 63, 65, 257)
SETUP_LABEL = b"mira guarded"
_setup_reference = {}


def setup_reference(curve, n):
    """messages, hash_to_field outputs and points of the first n points of SETUP_LABEL's key, in the library's layouts; the longest
    request is computed once per process and its prefixes serve the others"""
    import setup_ref as R
    have = _setup_reference.get(curve)
    if have is None or len(have[0]) < n:
        msgs = R.messages(SETUP_LABEL, 0, n)
        us = [R.hash_to_field(m, curve) for m in msgs]
        pts = [R.map_pair(u0, u1, curve)[0] for u0, u1 in us]
        have = _setup_reference[curve] = (msgs, us, pts)
    msgs, us, pts = (x[:n] for x in have)
    raw = lambda b: np.frombuffer(b, dtype=np.uint8)
    return (raw(b"".join(msgs)), raw(b"".join(R.fe_bytes(u0, curve) + R.fe_bytes(u1, curve) for u0, u1 in us)),
            raw(b"".join(R.point_bytes(P, curve) for P in pts)))


def same_raw(got, want, label, unit):
    got, want = np.asarray(got, dtype=np.uint8).reshape(-1), np.asarray(want).view(np.uint8).reshape(-1)
    assert got.shape == want.shape, (label, got.shape, want.shape)
    if not (got == want).all():
        i = int(np.nonzero(got != want)[0][0]) // unit
        raise AssertionError(f"{label}: item {i} differs: got {got[i * unit:(i + 1) * unit].tobytes().hex()} want {want[i * unit:(i + 1) * unit].tobytes().hex()}")


def check_generators(lib, curve, lengths=GEN_LENGTHS, offsets=OFFSETS):
    from oracle import cref as C
    setup_reference(curve, max(lengths))
    for n in lengths:
        want_sc = {kind: C.synth_scalars(curve, n, kind=kind) for kind in (0, 1)}
        want_bases = C.synth_bases(curve, n)
        msgs, us, pts = setup_reference(curve, n)
        for off in offsets:
            tag = f"curve={curve} n={n} offset={off}"
            with Arena(lib) as A:
                sc, bs = A.place(n, shifted(off, 0), "scalars"), A.place(2 * n, shifted(off, 1), "bases")
                for kind in (0, 1):
                    A.clear(sc)
                    lib.check(lib.c.mira_synth_scalars_device(curve, n, 0, 0x4D495241, kind, ctypes.c_void_p(sc.ptr)))
                    got, = A.check(f"synth_scalars kind={kind} {tag}", [sc])
                    same_raw(got, want_sc[kind], f"synth_scalars kind={kind} {tag}", 32)
                lib.check(lib.c.mira_synth_bases_device(curve, n, 0, 0x42415345, ctypes.c_void_p(bs.ptr)))
                got, = A.check(f"synth_bases {tag}", [bs])
                same_raw(got, want_bases, f"synth_bases {tag}", 64)
            with Arena(lib) as A:
                am, au, ap, au2 = A.place(msgs, shifted(off, 0), "msgs"), A.place(2 * n, shifted(off, 1), "u"), A.place(2 * n, shifted(off, 2), "points"), \
                    A.place(us, shifted(off, 2), "u (mapped in place)")
                key = A.place(2 * n, shifted(off, 1), "key")
                lib.check(lib.c.mira_hash_to_field_device(curve, ctypes.c_void_p(am.ptr), n, ctypes.c_void_p(au.ptr)))
                got, = A.check(f"hash_to_field {tag}", [au])
                same_raw(got, us, f"hash_to_field {tag}", 32)
                lib.check(lib.c.mira_map_to_curve_device(curve, ctypes.c_void_p(au.ptr), n, ctypes.c_void_p(ap.ptr)))
                got, = A.check(f"map_to_curve {tag}", [ap])
                same_raw(got, pts, f"map_to_curve {tag}", 64)
                lib.check(lib.c.mira_map_to_curve_device(curve, ctypes.c_void_p(au2.ptr), n, ctypes.c_void_p(au2.ptr)))
                got, = A.check(f"map_to_curve in place {tag}", [au2])
                same_raw(got, pts, f"map_to_curve in place {tag}", 64)
                lib.check(lib.c.mira_setup_bases_device(curve, SETUP_LABEL, len(SETUP_LABEL), 0, n, ctypes.c_void_p(key.ptr)))
                got, = A.check(f"setup_bases {tag}", [key])
                same_raw(got, pts, f"setup_bases {tag}", 64)


# ---- MSM input and output -------------------------------------------------------------------------------------------------------
MSM_LENGTHS = (1, 63, 65, 1025, 8193)
_msm_reference = {}


def msm_reference(curve, n, nmax, count):
    """-> ([scalar vectors of n], [the oracle's commitments under the first n synthetic bases]): vector 0 cycles the extreme
    representations of the curve's scalar field, the others are the oracle's synthetic scalars (witness-like and uniform by
    turns); every length is a prefix of the vectors of nmax.  Once per process."""
    from oracle import cref as C
    if (curve, nmax, count) not in _msm_reference:
        field = E.FIELD_FR if curve == CM.CURVE_BN256 else E.FIELD_FQ
        _msm_reference[(curve, nmax, count)] = (C.synth_bases(curve, nmax), [cycled_array(field, nmax, nmax)] +
                                                [C.synth_scalars(curve, nmax, seed=0x6D00 + b, kind=b % 2) for b in range(1, count)])
    bases, full = _msm_reference[(curve, nmax, count)]
    if (curve, nmax, count, n) not in _msm_reference:
        vecs = [np.ascontiguousarray(v[:n]) for v in full]
        _msm_reference[(curve, nmax, count, n)] = (vecs, [C.commit(curve, bases[:n], v) for v in vecs])
    return _msm_reference[(curve, nmax, count, n)]


def check_msm_io(lib, curve, lengths=MSM_LENGTHS, offsets=OFFSETS, widths=(9, 0), count=3, partial_planned=None):
    """mira_msm_device, mira_msm_batch_device with stride_elems > n (the gap between two vectors is guard fill: a digit kernel that
    reads past a vector's end meets non-canonical scalars and the commitment changes) and mira_msm_partial_to_device (the window
    sums between guards), at a forced window width of 9 bits and at the planner's; odd n and odd offsets move a window's digits
    off the 8-byte alignment the histogram's four-digits-per-load path needs.  `partial_planned`: the (n, offset) pairs at which the
    partial runs at the planner's width too (None: all) -- a partial's default width is 16 bits whatever n, and the bucket reduction
    of 16 windows of 2^15 buckets takes the emulation five seconds a call"""
    nmax = max(lengths)
    key = CM.CommitmentKey.synthetic(curve, nmax, lib=lib)
    try:
        for n in lengths:
            vecs, commits = msm_reference(curve, n, nmax, count)
            stride = n + 5 if n > 1 else 3
            for c in widths:
                key.set_window_bits(c)
                for off in offsets:
                    tag = f"curve={curve} n={n} c={c} offset={off}"
                    with Arena(lib) as A:
                        single = A.place(vecs[0], shifted(off, 0), "scalars")
                        batch = A.place((count - 1) * stride + n, shifted(off, 1), "batch of scalars")
                        part = A.place(np.full(_lib.MIRA_PARTIAL_U64, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64), shifted(off, 2), "partial")
                        for b, v in enumerate(vecs):
                            A.write(batch, v, b * stride)
                        E.same_bytes(key.commit_device(single.ptr, n).reshape(2, 4), commits[0].reshape(2, 4), f"msm_device {tag}")
                        A.check(f"msm_device {tag}")
                        got = key.commit_batch_device(batch.ptr, n, count, stride)
                        A.check(f"msm_batch_device stride={stride} {tag}")
                        for b in range(count):
                            E.same_bytes(got[b].reshape(2, 4), commits[b].reshape(2, 4), f"msm_batch_device stride={stride} vector {b} {tag}")
                        if c == 0 and partial_planned is not None and (n, off) not in partial_planned:
                            continue
                        wb, nw = key.commit_partial_to_device(0, single.ptr, n, part.ptr, window_bits=c)
                        raw, = A.check(f"msm_partial_to_device {tag}", [part])
                        words = raw.view(np.uint64)
                        assert 0 < nw <= _lib.MIRA_MAX_WINDOWS and not words[nw * 16:].any(), f"msm_partial_to_device {tag}: words beyond the {nw} windows are not zero"
                        E.same_bytes(CM.combine_partials(curve, words, wb, nw, lib=lib).reshape(2, 4), commits[0].reshape(2, 4), f"msm_partial_to_device {tag}")
    finally:
        key.set_window_bits(0)
        key.close()


def check_commit_device(lib, curve, n, offset=1):
    """one mira_msm_device over a synthetic key of n points, the scalars between guards"""
    vecs, commits = msm_reference(curve, n, n, 1)
    key = CM.CommitmentKey.synthetic(curve, n, lib=lib)
    try:
        with Arena(lib) as A:
            sc = A.place(vecs[0], offset, "scalars")
            E.same_bytes(key.commit_device(sc.ptr, n).reshape(2, 4), commits[0].reshape(2, 4), f"msm_device curve={curve} n={n} offset={offset}")
            A.check(f"msm_device curve={curve} n={n} offset={offset}")
    finally:
        key.close()


# ---- mira_dev_copy --------------------------------------------------------------------------------------------------------------
def check_copy(lib, sizes=(1, 33, 4097), offsets=OFFSETS):
    for nbytes in sizes:
        data = (np.arange(nbytes) * 7 + 3).astype(np.uint8)
        for off in offsets:
            with Arena(lib) as A:
                src, dst = A.place(data, shifted(off, 0), "src"), A.place(np.zeros(nbytes, dtype=np.uint8), shifted(off, 1), "dst")
                lib.copy(dst.ptr, src.ptr, nbytes)
                got, = A.check(f"dev_copy bytes={nbytes} offset={off}", [dst])
                assert (got == data).all(), f"dev_copy bytes={nbytes} offset={off}"


# ---- the device-resident transforms ---------------------------------------------------------------------------------------------
NTT_DEVICE_OPS = ("fft_device", "ifft_device", "best_fft_device_inv")
_ntt_device_cases = {}


def ntt_device_cases(k):
    """-> [(label, input, {op: the oracle's output})] for the oracle's synthetic scalars and the cycled extreme list; once per process"""
    from oracle import cref as C
    if k not in _ntt_device_cases:
        n = 1 << k
        out = []
        for label, a in (("random", C.synth_scalars(0, n, seed=0x4E54 + k)), ("cycled", cycled_array(E.FIELD_FR, n, k))):
            refs = {"fft_device": C.fft(a, k), "ifft_device": C.ifft(a, k), "best_fft_device_inv": C.best_fft(a, C.get_omega_or_inv(k, True), k)}
            out.append((label, a, refs))
        _ntt_device_cases[k] = out
    return _ntt_device_cases[k]


def run_ntt_device(lib, op, ptr, k, omega=None):
    from oracle import cref as C
    if op == "fft_device":
        F.fft_device(ptr, k, lib=lib)
    elif op == "ifft_device":
        F.ifft_device(ptr, k, lib=lib)
    else:
        F.best_fft_device(ptr, C.get_omega_or_inv(k, True) if omega is None else omega, k, lib=lib)


def check_ntt_device(lib, k, ops=NTT_DEVICE_OPS, offsets=OFFSETS, wave=None, max_log_line=None, grid=None, single_tw_log=None):
    """mira_fft_bn256_fr_device, mira_ifft_bn256_fr_device and mira_ntt_bn256_fr_device (with the inverse omega) on a vector of 2^k
    elements between guards: the transform works in place on the caller's buffer, so an out-of-range store of a pass's index
    algebra or of a tile copy lands in a guard band here -- the host entry points transform the library's own, larger staging
    buffer.  One arena holds a copy of the vector per offset; every transform runs on each and one download checks them all."""
    with E.knobs(lib, NTT_WAVE=wave, NTT_MAX_LOG_LINE=max_log_line, NTT_GRID=grid, NTT_SINGLE_TW_LOG=single_tw_log):
        tag = f"ntt_device k={k} wave={wave} max_log_line={max_log_line} grid={grid} single_tw_log={single_tw_log}"
        for label, a, refs in ntt_device_cases(k):
            with Arena(lib) as A:
                placed = [A.place(a, off, f"a (offset {off})") for off in offsets]
                for op in ops:
                    for v in placed:
                        A.write(v, a)
                        run_ntt_device(lib, op, v.ptr, k)
                    for off, got in zip(offsets, A.check(f"{tag} {op} {label}", placed)):
                        same(got, refs[op], f"{tag} {op} {label} offset={off}")


# ---- other primitive roots ------------------------------------------------------------------------------------------------------
def root_power(k, e):
    """omega_k ^ e in Montgomery form, by Python integers"""
    from oracle import cref as C
    p = MODULUS[E.FIELD_FR]
    w = E.to_value(E.from_array(C.get_omega_or_inv(k, False))[0], E.FIELD_FR)
    assert pow(w, 1 << k, p) == 1 and (k == 0 or pow(w, 1 << (k - 1), p) == p - 1)
    return E.to_array([E.from_value(pow(w, e, p), E.FIELD_FR)])[0]


def root_exponents(k):
    """odd exponents: every omega^e is a primitive 2^k-th root"""
    n = 1 << k
    es = [3, 5, n - 3, n // 2 + 1]
    assert all(e % 2 == 1 and 0 < e < n for e in es) and len(set(es)) == 4
    return es


def check_ntt_roots(lib, k, max_log_line=None, offsets=OFFSETS):
    """best_fft (host buffer) and best_fft_device (between guards) with omega^e for e = 3, 5, n - 3, n / 2 + 1 (root_exponents), then 7, then 3 again: five
    distinct roots at one size followed by the first, so that the four-deep cache of twiddle tables evicts and rebuilds"""
    from oracle import cref as C
    n = 1 << k
    a = cycled_array(E.FIELD_FR, n, 2 * k + 1)
    with E.knobs(lib, NTT_MAX_LOG_LINE=max_log_line):
        es = root_exponents(k)
        order = es + [7, es[0]]
        assert len(set(order[:5])) == 5 and order[5] == order[0]
        want = {}
        with Arena(lib) as A:
            placed = [A.place(a, off, f"a (offset {off})") for off in offsets]
            for e in order:
                omega = root_power(k, e)
                if e not in want:
                    want[e] = C.best_fft(a, omega, k)
                tag = f"best_fft k={k} max_log_line={max_log_line} omega^{e}"
                same(F.best_fft(a, omega, k, lib=lib), want[e], tag)
                for v in placed:
                    A.write(v, a)
                    F.best_fft_device(v.ptr, omega, k, lib=lib)
                for off, got in zip(offsets, A.check(f"{tag} device", placed)):
                    same(got, want[e], f"{tag} device offset={off}")
