"""Segment geometry of k_accumulate (csrc/msm_kernels.cuh): the staged entry stream, aimed at.

A lane of k_accumulate owns one SEGMENT of L consecutive sorted entries, [start, end) with start = t L, and reads them from LDS in
blocks of ACC_STAGE = 16 entries copied from the 16-byte aligned address stage_at = start & ~3: the first block at kernel start,
the second there too if stage_at + 16 < end, every later one in the iteration that reads the first entry of a block.  Under the
CPU emulation the copy is a memcpy and the waits are nothing, but the indices, the request condition and the bucket walk are the
same code.  The segment length is L = max(min_L, ceil(total / 196608)) (k_scan_c), min_L = MIRA_TUNE_MIN_SEGMENT (10 by default),
so every commit below about 2 M entries runs at L = 10: start & 3 is 0 or 2 there and no segment needs a second block.  This
module sets the knob and chooses the entries:

    segments(L, counts)     the geometry MODEL, restated in plain Python from the rule above: for every segment a = start & 3,
                            span = end - stage_at, nb = ceil(span / 16) blocks, span % 16, the offsets (run_end - stage_at) % 16
                            of the run ends inside it, and how far its last block reaches past the last entry.  `counts`: entries
                            per bucket in sort order (window-major, then |digit| - 1).
    shaped(...)             scalars with ONE non-zero digit each, an unsigned digit below 2^(c-1): no carries, the counts per bucket
                            are exactly the list of run lengths the case chose -- many runs of length 1 in a row, runs of every
                            length 1 .. 2 L + 1, stretches of empty buckets between runs (the `run_end <= j` search), a run that ends
                            exactly on a segment end and one that starts exactly on a segment start, runs cut into 2, 6, 7, 12
                            (light, medium), 13 (heavy, one sub-job) and 65 (heavy, two sub-jobs) head partials, and a tail of runs
                            that gives the last segment a chosen alignment and length
    dense(...)              uniform unsigned digits below 2^(c-1) in every window; `full`: none of them zero, so that the entries
                            fill the sorted buffer to its last word and the last segment's block reads into ACC_STAGE_PAD
    CASES                   for every L of SWEEP the shaped variants, then tails until every class is reached (check_coverage)
    SEQUENCES               every launch sequence that ends in k_accumulate, each held to its path by mira_msm_last_plan /
                            mira_msm_last_table_bits (workspace_state.check_path): plain per-window, the GLV split, the wide front,
                            a shared-bucket table set, a batch of 3, and the ADD = true instantiation both ways (a commit cut into
                            passes, host scalars cut into chunks)

The wide-table sequence (msm_launch_table, 20-bit tables) does NOT honour the knob: it sizes its segments from its own constant
Lmin = 16 and is left to its existing tests.  The model speaks for the per-window sequences (plain, wide front), whose sort order
is the one it takes; the others run the same vectors for their values.

Expected points come from the C oracle, once per vector (the point does not depend on L).  The coverage assertion is a condition
of the cases, not a measurement: it runs on the model alone, before any commit."""
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import edge_operands as E                                                    # noqa: E402
import workspace_state as WS                                                 # noqa: E402
from mira_amd import _lib                                                    # noqa: E402
from mira_amd import commitment as CM                                        # noqa: E402

ACC_STAGE = 16
LANES = 256 * 4 * 3 * 64                                # resident lanes: one segment each (msm_plan.hip)
NMAX = 4100                                             # points of the keys; the longest vector
SWEEP = (1, 2, 3, 5, 10, 13, 15, 16, 17, 19, 31, 32, 33, 47, 48, 49, 65)
REDUCED = (3, 15, 17, 31, 33, 65)                       # the other launch sequences: odd values on both sides of 16 and 32
CUTS = (2, 6, 7, 12, 13, 65)                            # head partials of a cut run: <= 6 light, <= 12 medium, <= 64 one sub-job
SCALAR_BITS = 253                                       # every built scalar is below 2^253 < both moduli


# ---- the model ------------------------------------------------------------------------------------------------------------------
def segment_length(min_l, total):
    return max(min_l, -(-total // LANES))


class Segment:
    __slots__ = ("t", "start", "end", "a", "span", "nb", "run_end_offsets", "shared_iteration", "overhang")

    @property
    def cls(self):
        return class_of(self.a, self.span)


def segments(L, counts):
    """the segments of k_accumulate over sorted entries with `counts` per bucket, in order"""
    ends, total = [], 0
    for k in counts:
        if k:
            total += k
            ends.append(total)                                              # where a run ends (empty buckets end nothing)
    at = 0
    for t in range(-(-total // L)):
        s = Segment()
        s.t, s.start, s.end = t, t * L, min(t * L + L, total)
        stage_at = s.start & ~3
        s.a, s.span = s.start & 3, s.end - stage_at
        s.nb = -(-s.span // ACC_STAGE)
        while ends[at] <= s.start:
            at += 1
        s.run_end_offsets, k = [], at
        while ends[k] < s.end:                                              # j == run_end for start < j < end
            s.run_end_offsets.append((ends[k] - stage_at) % ACC_STAGE)
            k += 1
        # iteration j reads entry r = min(j + 2, end - 1) - stage_at and requests the block behind r's when r % 16 == 0
        s.shared_iteration = any((e + 2 - stage_at) % ACC_STAGE == 0 and e + 2 < s.end and (e + 2 - stage_at) + ACC_STAGE < s.span
                                 for e in ends[at:k])
        s.overhang = stage_at + s.nb * ACC_STAGE - total                    # > 0: the last block reaches past the last entry
        yield s


def reachable_classes(max_l=65):
    """(a, nb in 1, 2, 3, >= 4, span % 16 in 0, 1, other) over every L <= max_l, every alignment t L & 3 and every length of a last segment"""
    out = set()
    for L in range(1, max_l + 1):
        for t in range(4):
            a = (t * L) & 3
            for ln in range(1, L + 1):
                out.add(class_of(a, a + ln))
    return out


# ---- the scalar builders --------------------------------------------------------------------------------------------------------
def field_of(curve):
    return E.FIELD_FR if curve == CM.CURVE_BN256 else E.FIELD_FQ


def windows(c):
    return -(-256 // c)


class Vector:
    """scalars (values), their stored array for one curve, the counts per bucket of the per-window sort"""

    def __init__(self, name, c, values, counts):
        self.name, self.c, self.values, self.counts, self.n = name, c, values, counts, len(values)
        self._arr, self._point = {}, {}
        assert 1 <= self.n <= NMAX and max(values) < 1 << SCALAR_BITS, (name, self.n)

    def array(self, curve):
        if curve not in self._arr:
            self._arr[curve] = E.to_array(E.from_value(v, field_of(curve)) for v in self.values)
            self._arr[curve].setflags(write=False)
        return self._arr[curve]

    def point(self, curve, bases):
        if curve not in self._point:
            from oracle import cref as C
            self._point[curve] = C.commit(curve, bases[:self.n], np.ascontiguousarray(self.array(curve)))
        return self._point[curve]

    @property
    def total(self):
        return sum(self.counts)

    def __repr__(self):
        return self.name


def counts_of(c, values):
    """what the sort sees: the unsigned c-bit digits of the values (all below 2^(c-1): nothing is recoded), per window and bucket"""
    W, B = windows(c), 1 << (c - 1)
    counts = [0] * (W * B)
    for v in values:
        w = 0
        while v:
            d = v & ((1 << c) - 1)
            assert d < B
            if d:
                counts[w * B + d - 1] += 1
            v >>= c
            w += 1
    return counts


def shaped(name, c, runs, seed):
    """runs: entries per bucket, laid over the buckets of the low windows in sort order (0: an empty bucket).  Every scalar has one
    non-zero digit; digit 2^(c-1) is never used, so the last bucket of a window stays empty"""
    B, max_w = 1 << (c - 1), 112 // c                                      # values below 2^112: the GLV split leaves them whole
    values, slot = [], 0
    for k in runs:
        if slot % B == B - 1:
            slot += 1
        w, b = divmod(slot, B)
        assert w < max_w, (name, "too many buckets")
        values += [(b + 1) << (c * w)] * k
        slot += 1
    random.Random(seed).shuffle(values)
    v = Vector(name, c, values, counts_of(c, values))
    assert [k for k in v.counts if k] == [k for k in runs if k]
    return v


def dense(name, c, n, seed, full=False):
    rng, W, B = random.Random(seed), windows(c), 1 << (c - 1)
    values = []
    for _ in range(n):
        v = 0
        for w in range(W):
            hi = min(B, 1 << max(0, SCALAR_BITS - c * w))                   # digits of window w below this keep the scalar below 2^253
            if hi > 1:
                v |= rng.randrange(1 if full else 0, hi) << (c * w)
        values.append(v)
    vec = Vector(name, c, values, counts_of(c, values))
    assert not full or vec.total == n * W                                   # the sorted buffer is filled to its last word
    return vec


class Runs:
    """a list of run lengths under construction, with the offset of the next entry"""

    def __init__(self, L, seed):
        self.L, self.runs, self.off, self.rng = L, [], 0, random.Random(seed)

    def add(self, k):
        if k > 0:
            self.runs.append(k)
            self.off += k

    def gap(self, buckets):
        self.runs += [0] * buckets

    def pad_to(self, residue):
        """the next run starts at an offset of this residue mod L"""
        self.add((residue - self.off) % self.L)

    def ones(self):
        for _ in range(2 * self.L + 3):
            self.add(1)

    def aligned(self):
        L = self.L
        self.pad_to(0)
        self.add(min(2, L))                                                 # starts exactly on a segment start
        self.add(L - 2)                                                     # ends exactly on a segment end
        self.add(L)                                                         # both
        self.gap(3)
        self.add(L + 1)

    def cut(self, partials):
        """a run with a tail partial and `partials` head partials: the last entry of a segment, partials - 1 whole segments, one entry"""
        L = self.L
        if L == 1:
            self.add(partials + 1)
        else:
            self.pad_to(L - 1)
            self.add((partials - 1) * L + 2)

    def lengths(self, part, parts):
        for i, k in enumerate(k for k in range(1, 2 * self.L + 2) if k % parts == part):
            self.add(k)
            if i % 5 == 4:
                self.gap((1, 2, 7)[(i // 5) % 3])

    def fill(self, at_least):
        while self.off < at_least:
            self.add(self.rng.randrange(1, 2 * self.L + 2))
            if self.rng.random() < 0.2:
                self.gap(self.rng.randrange(1, 4))

    def tail(self, t_mod4, ln):
        """runs up to a total of k L + ln entries, k = t_mod4 (mod 4): the last segment is number k and ln entries long"""
        L = self.L
        k = max(0, -(-(self.off + 1 - ln) // L))
        while k % 4 != t_mod4:
            k += 1
        rest = k * L + ln - self.off
        assert rest > 0 and self.off + rest <= NMAX, (L, self.off, rest)
        while rest > 0:
            r = min(rest, self.rng.randrange(1, 2 * L + 2))
            self.add(r)
            rest -= r


def shaped_bodies(L):
    """-> [(name, function that fills a Runs)]: one case for the short segments, the sections spread over several for the long ones"""
    cuts = [p for p in CUTS if (p - 1) * L + 2 <= 700 or p <= 13]

    def sections(r):
        r.ones()
        r.gap(5)
        r.aligned()
        for p in cuts:
            r.cut(p)
            r.gap(1)
    if L <= 17:
        def both(r):
            sections(r)
            r.lengths(0, 1)
        return [("all", both)]
    parts = 1 if L <= 33 else 2 if L <= 49 else 4
    return [("sections", sections)] + [(f"lengths {q}/{parts}", lambda r, q=q: r.lengths(q, parts)) for q in range(parts)]


_built = {}


class Case:
    def __init__(self, L, vector, curve):
        self.L, self.vector, self.curve = L, vector, curve
        self.name = f"L={L} c={vector.c} curve={curve} {vector.name} n={vector.n}"

    def segments(self):
        return segments(segment_length(self.L, self.vector.total), self.vector.counts)

    def __repr__(self):
        return self.name


def class_of(a, span):
    return (a, min(-(-span // ACC_STAGE), 4), span % ACC_STAGE if span % ACC_STAGE < 2 else 2)


def _tail_choices(L):
    """(t mod 4, ln) -> class of such a last segment"""
    return {(t, ln): class_of((t * L) & 3, ((t * L) & 3) + ln) for t in range(4) for ln in range(1, L + 1)}


def build_cases():
    """the shaped cases of every L of SWEEP, their last segments steered to classes not reached yet, then tail cases (shortest L first)
    until every reachable class is reached; width 13 for every fifth case, the curves by turns"""
    reached, cases = set(), []

    def make(L, name, body, want=None):
        at = len(cases)
        r = Runs(L, 0x5E6 + 131 * at)
        body(r)
        r.fill(1000)
        choices = _tail_choices(L)
        pick = next((k for k, cl in sorted(choices.items(), key=lambda kv: (-kv[0][1], kv[0][0])) if cl == want), None) if want else \
            next((k for k, cl in sorted(choices.items(), key=lambda kv: (-kv[0][1], kv[0][0])) if cl not in reached), (at % 4, L))
        r.tail(*pick)
        c = 13 if at % 5 == 4 else 8
        case = Case(L, shaped(f"shaped {name}", c, r.runs, 0xA11 + at), at % 2)
        cases.append(case)
        reached.update(s.cls for s in case.segments())

    for L in SWEEP:
        for name, body in shaped_bodies(L):
            make(L, name, body)
    for want in sorted(reachable_classes()):
        if want not in reached:
            L = next(L for L in SWEEP if want in _tail_choices(L).values())
            make(L, f"tail {want}", lambda r: r.ones(), want)
    return cases


def dense_vectors():
    if "dense" not in _built:
        _built["dense"] = _dense_vectors()
    return _built["dense"]


def _dense_vectors():
    return [dense("dense", 8, 1000, 0xD0), dense("dense full", 8, 4100, 0xD1, full=True), dense("dense full", 13, 1531, 0xD2, full=True),
            dense("dense", 13, 4099, 0xD3), dense("dense full", 16, 1025, 0xD4, full=True),
            dense("dense full", 9, 1023, 0xD5, full=True)]                  # 29 windows: an odd number of entries


def cases():
    if "cases" not in _built:
        _built["cases"] = build_cases()
    return _built["cases"]


def dense_cases(sweep=SWEEP, vectors=None):
    return [Case(L, v, (i + k) % 2) for k, v in enumerate(dense_vectors()) if vectors is None or k in vectors for i, L in enumerate(sweep)]


def check_coverage(verbose=True):
    """every reachable class in some segment of the cases; a run end at each of the 16 block offsets in a segment of two blocks or
    more, one of them in the iteration that requests a block; a last block that reaches 1 .. 15 entries past a FULL sorted buffer"""
    want = reachable_classes()
    got, offsets, shared, overhangs = set(), set(), 0, set()
    for case in cases():
        for s in case.segments():
            got.add(s.cls)
            if s.nb >= 2:
                offsets.update(s.run_end_offsets)
                shared += s.shared_iteration
    for case in dense_cases():
        v = case.vector
        segs = list(case.segments())
        got.update(s.cls for s in segs)
        if v.total == v.n * windows(v.c):
            overhangs.add(segs[-1].overhang)
    if verbose:
        print(f"segment geometry: {len(want)} classes reachable, {len(got & want)} reached; run ends at {len(offsets)} of 16 block offsets, "
              f"{shared} segments with a run end in a requesting iteration; overhangs of full buffers {sorted(overhangs)}")
    assert got >= want, f"classes not reached: {sorted(want - got)}"
    assert offsets == set(range(ACC_STAGE)), f"no run end at block offsets {sorted(set(range(ACC_STAGE)) - offsets)}"
    assert shared > 0
    assert {L for c in cases() for L in [c.L]} == set(SWEEP)
    assert any(1 <= o <= 15 for o in overhangs), overhangs
    return len(want), len(got & want)


# ---- the launch sequences -------------------------------------------------------------------------------------------------------
GLV = _lib.TABLE_GLV
SEQUENCES = {
    # name: (route, width the vectors are built for)
    "plain": WS.Route("plain", knobs=dict(GLV=0), width=8),
    "plain9": WS.Route("plain9", knobs=dict(GLV=0), width=9),
    "plain13": WS.Route("plain13", knobs=dict(GLV=0), width=13),
    "plain16": WS.Route("plain16", knobs=dict(GLV=0), width=16),
    "glv": WS.Route("glv", pre=(GLV,), width=9, on_key=True),
    "wide": WS.Route("wide", knobs=dict(GLV=0, WIDE_FRONT_MIN_C=9), width=10),
    "shared8": WS.Route("shared8", knobs=dict(SHARED_MIN_N=1, TABLE_WIDTH=8), pre=(12, 8)),
    "batch3": WS.Route("batch3", call="batch_device", knobs=dict(GLV=0), width=8),
    "passes": WS.Route("passes", knobs=dict(GLV=0, PASS_ENTRIES_LOG=14), width=8),          # at most 2^14 - 1 entries a pass: 448 scalars
    "hostchunks": WS.Route("hostchunks", call="host", knobs=dict(GLV=0, HOST_CHUNK_MIN_N=512), width=8),
}
OTHER_SEQUENCES = ("glv", "wide", "shared8", "batch3", "passes", "hostchunks")
PLAIN_OF_WIDTH = {8: "plain", 9: "plain9", 13: "plain13", 16: "plain16"}


def sequence_vectors(name, L):
    """three vectors of one length for a sequence at this L: shaped (every section that fits), dense, dense full"""
    key = ("seq", name, L)
    if key not in _built:
        route = SEQUENCES[name]
        c = route.width or 8
        r = Runs(L, 0x5EC + L)
        for _, body in shaped_bodies(L)[:2]:
            if r.off < 2200:
                body(r)
        r.fill(1000)
        r.tail(L % 4, max(1, L - 1 - L % 3))
        sh = shaped("shaped", c, r.runs, 0xB22 + L)
        _built[key] = [sh, dense("dense", c, sh.n, 0xB33 + L), dense("dense full", c, sh.n, 0xB44 + L, full=True)]
    return _built[key]


class Bench:
    """one library's keys of NMAX synthetic points per curve and precompute setting, and the oracle's bases"""

    def __init__(self, lib):
        from oracle import cref as C
        self.lib, self.keys = lib, {}
        self.bases = {curve: C.synth_bases(curve, NMAX) for curve in WS.CURVES}

    def key(self, curve, pre=()):
        if (curve, pre) not in self.keys:
            key = CM.CommitmentKey.synthetic(curve, NMAX, lib=self.lib)
            self.keys[(curve, pre)] = key
            for width in pre:
                key.precompute(width)
        return self.keys[(curve, pre)]

    def close(self):
        for key in self.keys.values():
            key.close()
        self.keys = {}

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def run(bench, name, curve, L, vectors, trim=False):
    """one commit of every vector (a batch: one submission of them all) through sequence `name` under MIRA_TUNE_MIN_SEGMENT = L"""
    lib, route = bench.lib, SEQUENCES[name]
    key = bench.key(curve, route.pre)
    n = vectors[0].n
    assert all(v.n == n for v in vectors)
    label = f"{name} L={L} curve={curve} n={n}"
    if trim:
        lib.trim(0)                                                         # the sorted buffer exactly as large as this commit needs
    try:
        with E.knobs(lib, MIN_SEGMENT=L, **route.knobs), E.Dev(lib) as dev:
            if route.width:
                key.set_window_bits(route.width) if route.on_key else lib.check(lib.c.mira_msm_set_window_bits(route.width))
            if route.call == "batch_device":
                stride = n + WS.GAP
                buf = np.full((len(vectors) * stride, 4), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
                for j, v in enumerate(vectors):
                    buf[j * stride:j * stride + n] = v.array(curve)
                got = key.commit_batch_device(dev.put(buf), n, len(vectors), stride)
                for j, v in enumerate(vectors):
                    WS.same_point(got[j], v.point(curve, bench.bases[curve]), f"{label} vector {j} ({v.name})")
                WS.check_path(lib, route, n, label)
                return
            for v in vectors:
                if route.call == "host":
                    got = key.commit(np.ascontiguousarray(v.array(curve)))
                else:
                    got = key.commit_device(dev.put(np.ascontiguousarray(v.array(curve))), n)
                WS.same_point(got, v.point(curve, bench.bases[curve]), f"{label} {v.name}")
                WS.check_path(lib, route, n, f"{label} {v.name}")
    finally:
        if route.width:
            key.set_window_bits(0) if route.on_key else lib.check(lib.c.mira_msm_set_window_bits(0))


def run_case(bench, case):
    v = case.vector
    run(bench, PLAIN_OF_WIDTH[v.c], case.curve, case.L, [v], trim=v.total == v.n * windows(v.c))


def run_sequence(bench, name, L, curve):
    vs = sequence_vectors(name, L)
    run(bench, name, curve, L, vs if name == "batch3" else [vs[0], vs[2]])


def check_knob_refusals(lib):
    """a minimum segment length of 0 cannot be planned with (the upper bound of segments divides by it), nor one that does not fit the
    planner's 32 bits: refused; negative values mean the default"""
    for bad in (0, (1 << 20) + 1, 1 << 32):
        rc = lib.c.mira_set_tuning(_lib.TUNE_MIN_SEGMENT, bad)
        assert rc == _lib.MIRA_E_BAD_ARG, f"MIRA_TUNE_MIN_SEGMENT = {bad}: rc={rc}"
    for ok in (1, 65, 1 << 20, -1):
        assert lib.c.mira_set_tuning(_lib.TUNE_MIN_SEGMENT, ok) == 0, ok


# ---- a process of its own -------------------------------------------------------------------------------------------------------
def specs(dense_l, dense_which, sequence_l):
    """what the emulation runs: every shaped case, a short dense list, every other sequence at a few L -> {spec: function of a Bench}"""
    out = {f"shaped {k}": (lambda b, c=c: run_case(b, c)) for k, c in enumerate(cases())}
    for v in dense_which:
        out[f"dense {v}"] = lambda b, v=v: [run_case(b, c) for c in dense_cases(dense_l, vectors=(v,))]
    for name in OTHER_SEQUENCES:
        out[f"sequence {name}"] = lambda b, name=name: [run_sequence(b, name, L, (L + len(name)) % 2) for L in sequence_l]
    return out


def main(argv):
    """python tests/segment_geometry.py                      the coverage figures and the list of cases
    python tests/segment_geometry.py LIBRARY JSON-ARGS    every spec of specs(*args) on that library, `ok SPEC` after each (`failed
    SPEC` behind the traceback of one that raised; an assertion of the emulation ends the process inside the spec it names)"""
    if len(argv) == 1:
        check_coverage()
        for case in cases():
            print(case)
        return 0
    import json
    import traceback
    lib, failed = _lib.MiraLib(argv[1]), 0
    with Bench(lib) as bench:
        for name, fn in specs(*json.loads(argv[2])).items():
            print(f"run {name}", flush=True)
            try:
                fn(bench)
            except Exception:
                failed += 1
                print(traceback.format_exc()[-3000:], flush=True)
                print(f"failed {name}", flush=True)
                continue
            print(f"ok {name}", flush=True)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
