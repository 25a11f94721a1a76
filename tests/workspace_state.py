"""What one call leaves behind in the library's internal workspaces, and what the next call makes of it.

The library keeps about forty grow-only device buffers in one process-wide Ctx (csrc/ctx.h), shared by every key and every call,
and the hot path never clears them: every counter, marker, tail key and partial a kernel reads has to be written earlier in the
SAME call (DESIGN.md lists which kernel owes what).  A kernel that reads something nobody wrote passes whenever the memory
happens to hold zero -- fresh pages do, so the first call after a growth always looks fine -- and an overrun of an internal
buffer lands in the slack an earlier, larger call left.  Three ways to make such a fault show:

    ROUTES                 one table of the routes through the shared MSM workspace, each forced at a small length by tuning knobs,
                           a window width and a precomputed copy of the key; every part below runs the same table
    poison                 (CPU emulation only) the child process runs under glibc's MALLOC_PERTURB_, so that every allocation comes
                           back filled with one byte, and behind TrimFirst, which releases every workspace (mira_trim(0)) before
                           every compute entry point: whatever a call touches is new and holds nothing but fill
    check_pairs            every route after every other: A at the large length, B at the small one (and the reverse order), on
                           another curve and another kind of vector; `fresh` (a trim) as A gives B buffers of exactly its own size
    check_*_sequence       the same for the other workspaces (transforms, lookup, inversion, deciders, trees, graphs, folds)
    check_schedule         a fixed, seeded list of calls drawn from all families on one library
    check_refusals         the error paths that run kernels before they refuse, and what the next valid call gives after them

Nothing expected ever comes from the library: commitments from the C oracle (one call per curve, length and vector -- the point
does not depend on the route), everything else from the references of edge_operands.py and guarded.py.  Every comparison is on
bytes.

    python tests/workspace_state.py LIBRARY plain|poison CASE[:JSON-KWARGS] ...

runs cases in a process of their own and prints `ok CASE` after each (`failed CASE` behind the traceback of one that raised: the
others still run, and the exit status is 1); `poison` proves first that the fill is active."""
import ctypes
import json
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import edge_operands as E                                                    # noqa: E402
import guarded as GD                                                         # noqa: E402
from mira_amd import _lib                                                    # noqa: E402
from mira_amd import commitment as CM                                        # noqa: E402
from mira_amd import decider as DC                                           # noqa: E402
from mira_amd import fft as F                                                # noqa: E402
from mira_amd import lookup as LU                                            # noqa: E402
from mira_amd.graph_evaluator import MODULUS                                 # noqa: E402

CURVES = (CM.CURVE_BN256, CM.CURVE_GRUMPKIN)
KINDS = ("dense", "witness", "heavy")
BATCH = 3                                               # vectors of a batch route: the three kinds
GAP = 5                                                 # a device batch's stride is its vectors' full length + GAP elements: > n at every n


# ---- the route table ------------------------------------------------------------------------------------------------------------
class Route:
    """name; call: which entry point commits; knobs: mira_set_tuning values by name; width: a forced window width, set for the process
    (mira_msm_set_window_bits) or on the key (`on_key`); pre: the precompute widths of the key it runs on; cost: "fast" -- a commit of
    1500 pairs stays under half a second on the emulation -- or "slow" (up to eight seconds)"""

    def __init__(self, name, call="device", knobs=None, width=0, on_key=False, pre=(), cost="fast"):
        self.name, self.call, self.knobs, self.width, self.on_key, self.pre, self.cost = name, call, dict(knobs or {}), width, on_key, tuple(pre), cost

    def __repr__(self):
        return self.name


PARTIAL_WIDTH = {"partial": 9, "partial_to_device": 10}   # a partial that names no width takes 16-bit windows whatever its length
ROUTES = [
    Route("planned", knobs=dict(PLAN_HIST_MIN_N=1)),                                        # the planner's own choice, trials and statistics on
    Route("plain", knobs=dict(GLV=0)),
    Route("c5", knobs=dict(GLV=0), width=5),
    Route("c13", knobs=dict(GLV=0), width=13, on_key=True, cost="slow"),
    Route("c16", knobs=dict(GLV=0), width=16, cost="slow"),
    Route("staged", knobs=dict(GLV=0, STAGED_MIN_N=1), width=11, cost="slow"),              # the two-level sort of the long commits
    Route("wide", knobs=dict(GLV=0, WIDE_FRONT_MIN_C=9), width=10, cost="slow"),            # the front of the 17- to 20-bit windows
    Route("glv", pre=(_lib.TABLE_GLV,)),
    Route("glv9", pre=(_lib.TABLE_GLV,), width=9, on_key=True),
    Route("shared12", knobs=dict(SHARED_MIN_N=1), pre=(12,)),
    Route("shared8", knobs=dict(SHARED_MIN_N=1, TABLE_WIDTH=8), pre=(12, 8)),               # a second set beside the first
    Route("hostchunks", call="host", knobs=dict(GLV=0, HOST_CHUNK_MIN_N=512)),
    Route("tables20", knobs=dict(TABLE_MIN_N=1), pre=(20,), cost="slow"),                   # 13 windows over one set of 2^19 buckets
    Route("batch_host", call="batch_host", knobs=dict(GLV=0, HOST_CHUNK_MIN_N=512), cost="slow"),
    Route("batch_device", call="batch_device", knobs=dict(GLV=0), cost="slow"),
    Route("partial", call="partial", knobs=dict(GLV=0), cost="slow"),
    Route("partial_to_device", call="partial_to_device", knobs=dict(GLV=0), cost="slow"),
    Route("passes", knobs=dict(GLV=0, PASS_ENTRIES_LOG=14), width=8),                       # at most 2^14 - 1 entries a pass: 448 scalars
    Route("c4", knobs=dict(GLV=0), width=4),                                                # eight buckets a window: every bucket is heavy
    # bit-length statistics (collected from MIRA_TUNE_PLAN_HIST_MIN_N pairs on, 2^15 by default): k_digits adds into one of the two
    # histograms of g.hist_dev and zeroes the other, k_set_finish ships it, the key keeps it and the next commit of the length plans from it
    Route("stats_plain", knobs=dict(GLV=0, PLAN_HIST_MIN_N=1)),                             # whole scalars (stat_kind 0)
    Route("stats_glv", knobs=dict(PLAN_HIST_MIN_N=1), pre=(_lib.TABLE_GLV,)),               # the halves of the split (stat_kind 1)
    Route("stats_shared", knobs=dict(SHARED_MIN_N=1, PLAN_HIST_MIN_N=1), pre=(12, 8)),      # collected beside a table set, which the model picks from them
]
ROUTE = {r.name: r for r in ROUTES}
assert len(ROUTE) == len(ROUTES)
FRESH = "fresh"                                         # the pseudo-route: mira_trim(0)


def route_names(*costs):
    return [r.name for r in ROUTES if not costs or r.cost in costs]


# ---- vectors, keys and the oracle's points --------------------------------------------------------------------------------------
_reference = {}


class Reference:
    """bases, the three scalar vectors and the oracle's commitments of every prefix asked for, for keys of nmax points; once per process"""

    def __init__(self, nmax):
        from oracle import cref as C
        self.nmax, self.C = nmax, C
        self.bases = {cid: C.synth_bases(cid, nmax) for cid in CURVES}
        self.vectors, self.points = {}, {}
        for cid in CURVES:
            dense = C.synth_scalars(cid, nmax, seed=0x5700 + cid, kind=0)
            heavy = dense.copy()
            heavy[1::2] = dense[1]                                          # half of it one repeated value: the heavy-run path writes its lists
            self.vectors[cid] = {"dense": dense, "witness": C.synth_scalars(cid, nmax, seed=0x5710 + cid, kind=1), "heavy": heavy}
            for v in self.vectors[cid].values():
                v.setflags(write=False)

    def vector(self, curve, kind, n):
        return np.ascontiguousarray(self.vectors[curve][kind][:n])

    def bit_lengths(self, curve, kind):
        key = ("bits", curve, kind)
        if key not in self.points:
            field = E.FIELD_FR if curve == CM.CURVE_BN256 else E.FIELD_FQ
            rinv, p = pow(E.R, -1, MODULUS[field]), MODULUS[field]
            self.points[key] = np.array([min(255, (r * rinv % p).bit_length()) for r in E.from_array(self.vectors[curve][kind])], dtype=np.int64)
        return self.points[key]

    def histogram(self, curve, kind, n):
        """what k_digits counts over the first n scalars: the bit lengths of the canonical values, of every block of 256 where there
        are fewer than eight blocks, else of every eighth block eight-fold -> (256 counts, scalars counted, weight)"""
        bits, blocks = self.bit_lengths(curve, kind)[:n], -(-n // 256)
        weight = 1 if blocks < 8 else 8
        taken = np.ones(n, dtype=bool) if blocks < 8 else (np.arange(n) // 256) % 8 == 0
        return np.bincount(bits[taken], minlength=256) * weight, int(taken.sum()), weight

    def point(self, curve, kind, n):
        key = (curve, kind, n)
        if key not in self.points:
            self.points[key] = self.C.commit(curve, self.bases[curve][:n], self.vector(curve, kind, n))
            self.points[key].setflags(write=False)
        return self.points[key]


def reference(nmax):
    if nmax not in _reference:
        _reference[nmax] = Reference(nmax)
    return _reference[nmax]


class Bench:
    """one library's side of the table: a synthetic key of nmax points per curve and precompute setting, the vectors on the device"""

    def __init__(self, lib, nmax):
        self.lib, self.nmax, self.ref = lib, nmax, reference(nmax)
        self.keys, self.d_vec, self.d_part = {}, {}, None
        self.stride = nmax + GAP
        # The emulation runs the lanes of k_digits one after the other, so each flushes its bins before the lanes behind it have
        # counted: its statistics are no histogram Python could restate.  There they are held to themselves -- what a commit leaves
        # must not depend on what ran before it -- and on the device to the histogram of the vector.
        self.exact_stats = "emu" not in os.path.basename(lib.path)
        self.seen_stats, self.primed = {}, set()

    def key(self, curve, pre=()):
        if (curve, pre) not in self.keys:
            key = CM.CommitmentKey.synthetic(curve, self.nmax, lib=self.lib)
            self.keys[(curve, pre)] = key
            for width in pre:
                key.precompute(width)
        return self.keys[(curve, pre)]

    def vectors(self, curve):
        """the three vectors on the device, `stride` elements apart, the gaps non-canonical"""
        if curve not in self.d_vec:
            buf = np.full((BATCH * self.stride, 4), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
            for j, kind in enumerate(KINDS):
                buf[j * self.stride:j * self.stride + self.nmax] = self.ref.vectors[curve][kind]
            self.d_vec[curve] = self.lib.alloc(buf.nbytes)
            self.lib.upload(self.d_vec[curve], buf)
        return self.d_vec[curve]

    def vector(self, curve, kind):
        return self.vectors(curve) + KINDS.index(kind) * self.stride * 32

    def partial(self):
        if self.d_part is None:
            self.d_part = self.lib.alloc(_lib.MIRA_PARTIAL_U64 * 8)
        return self.d_part

    def close(self):
        for key in self.keys.values():
            key.close()
        for p in list(self.d_vec.values()) + ([self.d_part] if self.d_part else []):
            self.lib.free(p)
        self.keys, self.d_vec, self.d_part = {}, {}, None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


_benches = {}


def shared_bench(lib, nmax):
    """the process's one Bench of this library and length (a child process runs many cases on the same keys); close_benches ends them"""
    key = (id(lib), nmax)
    if key not in _benches:
        _benches[key] = Bench(lib, nmax)
    return _benches[key]


def close_benches():
    for b in _benches.values():
        b.close()
    _benches.clear()


class Borrowed:
    """a Bench of the caller's for the length of a `with` block: it stays open"""

    def __init__(self, bench):
        self.bench = bench

    def __enter__(self):
        return self.bench

    def __exit__(self, *exc):
        pass


def same_point(got, want, label):
    E.same_bytes(np.asarray(got).reshape(2, 4), want.reshape(2, 4), label)


def last_plan(lib):
    c, w, t = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    lib.check(lib.c.mira_msm_last_plan(ctypes.byref(c), ctypes.byref(w)))
    lib.check(lib.c.mira_msm_last_table_bits(ctypes.byref(t)))
    return c.value, w.value, t.value


def check_path(lib, route, n, label):
    """the commit took the path the route is named after, by mira_msm_last_plan and mira_msm_last_table_bits: the forced width, the
    table set or the wide tables, windows over 256 bits on the plain path and over the 128 of the halves on the split one (a planned
    commit splits from a few hundred pairs on; 257 is the shortest this table runs besides a single pair)"""
    c, w, t = last_plan(lib)
    got = f"{label}: last plan c={c} W={w} table={t}"
    if route.name == "planned":
        return
    if 20 in route.pre:
        assert (c, w, t) == (0, 64, 20), got + ", not the 20-bit tables"
    elif 12 in route.pre:
        want = (route.knobs["TABLE_WIDTH"],) if "TABLE_WIDTH" in route.knobs else tuple(x for x in route.pre)
        assert c == 0 and t in want, got + f", not a table set of {want}"
    else:
        width = route.width or PARTIAL_WIDTH.get(route.name, 0)
        assert t == 0 and (not width or c == width), got + f", not {width}-bit windows of its own"
        split = _lib.TABLE_GLV in route.pre and (width or n >= 257)
        if split:
            assert 128 <= c * w < 200, got + ", not the GLV split"
        elif route.knobs.get("GLV") == 0:
            assert c * w >= 256, got + ", not the plain path"


def check_stats(bench, route, key, curve, n, kind, label):
    """the bit-length statistics the commit left on its key (the statistics slot of mira_msm_tuning_export)"""
    stats = key.tuning_records().stats
    assert stats is not None and stats["n"] == n, f"{label}: no statistics of this commit on the key ({stats and stats['n']})"
    want_kind = 1 if route.name == "stats_glv" else 0 if route.name in ("stats_plain", "stats_shared") else stats["kind"]
    assert stats["kind"] == want_kind, f"{label}: statistics of kind {stats['kind']}, want {want_kind}"
    hist = np.array(stats["hist"], dtype=np.int64)
    if not bench.exact_stats:
        first = bench.seen_stats.setdefault((route.name, curve, n, kind, stats["kind"]), hist)
        assert (hist == first).all(), f"{label}: the statistics differ from those the same commit left before, at bit lengths {np.nonzero(hist != first)[0][:8].tolist()}"
        return
    want, counted, weight = bench.ref.histogram(curve, kind, n)
    if stats["kind"] == 0:
        bad = np.nonzero(hist != want)[0]
        assert not len(bad), f"{label}: statistics differ at bit length {int(bad[0])}: got {int(hist[bad[0]])} want {int(want[bad[0]])} ({len(bad)} bins differ)"
    else:                                                                   # two halves a scalar, each below 2^128
        assert hist.sum() == 2 * counted * weight and not hist[129:].any(), f"{label}: {int(hist.sum())} halves counted, want {2 * counted * weight}"


def prime_stats(bench, calls):
    """(emulation) before a sequence begins: every statistics-collecting commit of it once behind a trim, which leaves both histograms
    new and zero -- what it leaves on its key then is what it must leave wherever it runs in the sequence"""
    if bench.exact_stats:
        return
    for name, curve, n, kind in calls:
        if name != FRESH and "PLAN_HIST_MIN_N" in ROUTE[name].knobs and n >= 1 and (name, curve, n, kind) not in bench.primed:
            bench.primed.add((name, curve, n, kind))
            for stat_kind in (0, 1):
                bench.seen_stats.pop((name, curve, n, kind, stat_kind), None)
            bench.lib.trim(0)
            run_route(bench, name, curve, n, kind, "[behind a trim] ")


def run_route(bench, name, curve, n, kind, tag=""):
    """one commit (a batch: three) of the first n points of the curve's key by this route, compared with the oracle"""
    lib, ref = bench.lib, bench.ref
    label = f"{tag}{name} curve={curve} n={n} {kind}"
    if name == FRESH:
        lib.trim(0)
        return
    route = ROUTE[name]
    key = bench.key(curve, route.pre)
    k0 = KINDS.index(kind)
    try:
        with E.knobs(lib, **route.knobs):
            if route.width:
                key.set_window_bits(route.width) if route.on_key else lib.check(lib.c.mira_msm_set_window_bits(route.width))
            if route.call == "device":
                same_point(key.commit_device(bench.vector(curve, kind), n), ref.point(curve, kind, n), label)
            elif route.call == "host":
                same_point(key.commit(ref.vector(curve, kind, n)), ref.point(curve, kind, n), label)
            elif route.call == "batch_host":
                kinds = [KINDS[(k0 + j) % BATCH] for j in range(BATCH)]
                got = key.commit_batch([ref.vector(curve, k, n) for k in kinds])
                for j, k in enumerate(kinds):
                    same_point(got[j], ref.point(curve, k, n), f"{label} vector {j} ({k})")
            elif route.call == "batch_device":                              # the three vectors as they lie, at a stride > n
                got = key.commit_batch_device(bench.vectors(curve), n, BATCH, bench.stride)
                for j, k in enumerate(KINDS):
                    same_point(got[j], ref.point(curve, k, n), f"{label} vector {j} ({k})")
            elif route.call == "partial":
                part, wb, nw = key.commit_partial_device(0, bench.vector(curve, kind), n, window_bits=PARTIAL_WIDTH[name])
                same_point(CM.combine_partials(curve, part, wb, nw, lib=lib), ref.point(curve, kind, n), label)
            elif route.call == "partial_to_device":
                wb, nw = key.commit_partial_to_device(0, bench.vector(curve, kind), n, bench.partial(), window_bits=PARTIAL_WIDTH[name])
                part = lib.download(bench.partial(), _lib.MIRA_PARTIAL_U64)
                same_point(CM.combine_partials(curve, part, wb, nw, lib=lib), ref.point(curve, kind, n), label)
            else:
                raise ValueError(route.call)
            check_path(lib, route, n, label)
            if "PLAN_HIST_MIN_N" in route.knobs and n >= 1:
                check_stats(bench, route, key, curve, n, kind, label)
    finally:
        if route.width:
            key.set_window_bits(0) if route.on_key else lib.check(lib.c.mira_msm_set_window_bits(0))


def check_routes(lib, n, routes=None, curves=CURVES, once=(), nmax=None):
    """every route (of `routes`) on both curves with the dense and the witness-like vector, and on one of them -- by turns -- with the
    half-repeated one; the routes of `once` with one vector a curve"""
    with Bench(lib, nmax or n) as bench:
        for name in routes or route_names():
            for curve in curves:
                at = route_names().index(name) + curve
                kinds = [KINDS[at % 3]] if name in once else ["dense", "witness"] + (["heavy"] if at % 2 == 0 else [])
                for kind in kinds:
                    run_route(bench, name, curve, n, kind)


def check_pairs(lib, a, bs, large, small, second=True, reverse=True, bench=None):
    """B after A for every B of `bs`: A at the large length on one key, then B at the small length on another -- of the other curve for
    half of the pairs, always with another kind of vector -- and B again, planned from its own first statistics; then the reverse
    order, small A and large B, so that B grows the buffers A has used.  Every point is compared."""
    ia = ([FRESH] + route_names()).index(a)
    with Borrowed(bench or shared_bench(lib, large)) as bench:
        assert bench.lib is lib and bench.nmax >= large
        plan = []
        for b in bs:
            ib = route_names().index(b)
            curve_a = (ia + ib) % 2
            curve_b = curve_a ^ ((ia + ib // 2) % 2)
            kind_a = KINDS[(ia + ib) % 3]
            kind_b = KINDS[(ia + ib + 1 + ib % 2) % 3]
            assert kind_a != kind_b
            plan.append((b, curve_a, curve_b, kind_a, kind_b))
        prime_stats(bench, [c for b, ca, cb, ka, kb in plan for c in ((a, ca, large, ka), (b, cb, small, kb), (a, ca, small, kb), (b, cb, large, ka))])
        for b, curve_a, curve_b, kind_a, kind_b in plan:
            tag = f"[{b} after {a}] "
            run_route(bench, a, curve_a, large, kind_a, tag + "A: ")
            run_route(bench, b, curve_b, small, kind_b, tag + "B: ")
            if second:
                run_route(bench, b, curve_b, small, kind_b, tag + "B again: ")
            if reverse:
                tag = f"[large {b} after small {a}] "
                run_route(bench, a, curve_a, small, kind_b, tag + "A: ")
                run_route(bench, b, curve_b, large, kind_a, tag + "B: ")


# ---- the other workspaces: large then small, small then large -------------------------------------------------------------------
def check_ntt_sequence(lib, big=13):
    """2^13 -> 2^5 -> 2^13 -> 2^9 points through g.ntt_tmp / g.ntt_stage and the four cached twiddle sets: the forced wave-level and
    workgroup-level kernels by turns, fft and coset_ifft by turns, and best_fft with other primitive roots between them, so that
    the cache of tables turns over (seven distinct tables, four places) and a table comes back after its eviction.  Every other
    transform of 2^13 points runs on a grid of two workgroups, which then draw their lines from the work counters of g.ntt_consts:
    the counters a pass leaves behind are the next transform's"""
    from oracle import cref as C
    steps = [(big, 0, "fft", None, 2), (5, 1, "coset_ifft", None, None), (9, None, "best_fft", 3, None), (big, 1, "coset_ifft", None, 2), (5, None, "best_fft", 5, None),
             (9, 0, "fft", None, 2), (9, None, "best_fft", 3, None), (big, None, "best_fft", (1 << big) - 3, None), (5, 0, "fft", None, None),
             (9, 1, "coset_ifft", None, 2), (big, 1, "fft", None, 2), (5, 1, "coset_ifft", None, None), (big, None, "best_fft", (1 << big) - 3, 2),
             (9, None, "best_fft", 5, None), (big, 0, "fft", None, 3)]
    want = {}
    for i, (k, wave, op, e, grid) in enumerate(steps):
        a = GD.cycled_array(E.FIELD_FR, 1 << k, k)
        omega = GD.root_power(k, e) if e is not None else None
        if (k, op, e) not in want:
            want[(k, op, e)] = C.best_fft(a, omega, k) if op == "best_fft" else getattr(C, op)(a, k)
        tag = f"ntt sequence step {i}: k={k} wave={wave} grid={grid} {op} omega^{e}"
        with E.knobs(lib, NTT_WAVE=wave, NTT_GRID=grid):
            if op == "best_fft":
                got = F.best_fft(a, omega, k, lib=lib)
            elif op == "fft":
                got = F.fft(a, k, lib=lib)
            else:
                got = F.coset_ifft(a, lib=lib)
            E.same_bytes(got, want[(k, op, e)], tag)
            if i % 3 == 0 and op != "coset_ifft":                           # the device-resident entry points by turns: in place on the caller's buffer
                with GD.Arena(lib) as A:
                    v = A.place(a, 1, "a")
                    F.best_fft_device(v.ptr, omega, k, lib=lib) if op == "best_fft" else F.fft_device(v.ptr, k, lib=lib)
                    got, = A.check(tag + " device", [v])
                    GD.same(got, want[(k, op, e)], tag + " device")


def check_lookup_sequence(lib, field):
    """m / h / g with a large table, small ones and a large one again: the hash table's capacity follows n_t, and the large table's
    slots beyond a small one's capacity still hold the large one's owners and counts when the next large one comes.  (Probing
    from slot 0 -- MIRA_TUNE_LOOKUP_HASH = 1 -- fills only the first slots, so the call before a change of capacity always hashes.)
    Then batch inversions of 4097 -> 3 -> 1025 elements with two chunk lengths."""
    for shape, hashes in (((1025, 2049), (1, None)), ((65, 63), (1, None)), ((2049, 64), (None, 1)), ((1, 1), (None,)), ((2049, 2049), (None, 1)),
                          ((257, 255), (None, 1)), ((1025, 2049), (None,))):
        GD.check_lookup(lib, field, shapes=(shape,), offsets=(1,), hashes=hashes)
    GD.check_batch_invert(lib, field, lengths=(4097, 3, 1025), offsets=(1,))


def perm_case(field, n, num_io, seed):
    """a permutation of n indices in cycles of 1 .. 3, a Z that satisfies it and one with a few broken cells
    -> (pairs, good Z, bad Z, (count, first) of the bad one), Z as representations; the expectation by Python"""
    rng, reps = random.Random(seed), E.representations(field)
    order = list(range(n))
    rng.shuffle(order)
    sigma, z, at = list(range(n)), [0] * n, 0
    while at < n:
        size = min(rng.choice([1, 2, 3]), n - at)
        cyc, val = order[at:at + size], rng.choice(reps)
        for q, i in enumerate(cyc):
            sigma[i], z[i] = cyc[(q + 1) % size], val
        at += size
    bad_z = list(z)
    for cell in [0, n - 1] + rng.sample(range(n), 5):
        bad_z[cell] = (1 << 200) + 5 + cell                                 # canonical, and no representation of the list
    bad = [i for i in range(n) if bad_z[sigma[i]] != bad_z[i]]
    assert bad and not [i for i in range(n) if z[sigma[i]] != z[i]]
    return [(i, sigma[i]) for i in range(n)], z, bad_z, (len(bad), bad[0])


def check_decider_sequence(lib, field):
    """count_ne / sum_sub / perm_check at 4097 -> 1 -> 1025 -> 255 -> 4097 elements, then is_sat_perm with two compiled matrices of
    1030 and 67 rows by turns, satisfied and broken by turns (g.decide_parts, g.decide_eval, g.decide_inst)"""
    GD.check_deciders(lib, field, lengths=(4097, 1, 1025, 255, 4097), offsets=(1,))
    cases = [(1030, 2, 0xD0), (67, 1, 0xD1)]
    perms, data = [], []
    try:
        for n, num_io, seed in cases:
            pairs, z, bad_z, want = perm_case(field, n, num_io, seed + field)
            perms.append(DC.PermutationMatrix(field, pairs, n, lib=lib))
            data.append((n, num_io, z, bad_z, want))
        with E.Dev(lib) as dev:
            for turn in range(6):
                which = turn % 2
                n, num_io, z, bad_z, want = data[which]
                broken = turn in (1, 2, 5)
                zz = bad_z if broken else z
                d_w = dev.put(zz[num_io:])
                tag = f"is_sat_perm turn {turn}: field={field} n={n} broken={broken}"
                inst = E.to_array(zz[:num_io])
                if broken:
                    try:
                        DC.is_sat_perm_device(perms[which], inst, d_w, n - num_io, 1)
                    except DC.PermCheckFail as err:
                        assert (err.mismatch_count, err.first) == want, (tag, err.mismatch_count, err.first, want)
                    else:
                        raise AssertionError(tag + ": a broken permutation passed")
                else:
                    DC.is_sat_perm_device(perms[which], inst, d_w, n - num_io, 1)
    finally:
        for pm in perms:
            pm.close()


def check_pow_tree_sequence(lib, field):
    """2^11 -> 2^1 -> 2^6 leaves (g.tree_w, g.tree_a, g.tree_b)"""
    GD.check_pow_tree(lib, field, sizes=(11, 1, 6), offsets=(1,))


def check_fold_sequence(lib, field):
    GD.check_fold(lib, field, lengths=(1025, 63, 1023), offsets=(1,))
    GD.check_lincomb(lib, field, lengths=(1025, 65, 1023), offsets=(3,))


_graph_cases = {}


def graph_case(field, rows):
    """three gate-like graphs over mock columns of `rows` rows, the oracle's walk of their calculation lists as the expectation"""
    from graph_cases import gate_like_expression, mock_data, oracle_columns
    from harness import graph_evaluator as G
    from oracle import cref as C
    if (field, rows) not in _graph_cases:
        nsel, nfix, nadv, nchal = 2, 3, 7, 3
        rng = random.Random(0x6AF + field)
        exprs = [gate_like_expression(rng, nterms, 5, nsel + nfix + nadv, nchal) for nterms in (1, 4, 9)]
        _, arrs = mock_data(field, rows, nsel, nfix, nadv, nchal, seed=0x6B0 + field)
        chal_m = G.to_montgomery(arrs["challenges"], field)
        want = []
        for e in exprs:
            ev = G.GraphEvaluator.new(e, field)
            code, consts, rots = ev.flatten()
            want.append(C.graph_eval(field, code, ev.num_intermediates, consts, rots, oracle_columns(arrs), chal_m, rows))
            ev.close()
        _graph_cases[(field, rows)] = (exprs, arrs, want)
    return _graph_cases[(field, rows)]


def check_graph_rows(lib, field, rows, evs=None, specialised=False, tag=""):
    """the three graphs over `rows` rows through the one-shot interpreter, the compiled engine and its batch; `evs`: the caller's
    compiled graphs (`specialised`: they have kernels of their own, and the compiled engine must take them)"""
    from harness import graph_evaluator as G
    exprs, arrs, want = graph_case(field, rows)
    chal = arrs["challenges"]
    chal_m = G.to_montgomery(chal, field)
    own = evs is None
    evs = [G.GraphEvaluator.new(e, field) for e in exprs] if own else evs
    engine = "specialised" if specialised else "compiled"
    try:
        with E.Dev(lib) as dev:
            cols = [(dev.put(s), G.COL_BOOL) for s in arrs["selectors"]] + [(dev.put(c), G.COL_FIELD) for c in arrs["fixed"] + arrs["advice"]]
            table = G.GraphEvaluator._column_table(cols)
            d_all = dev.empty(len(evs) * rows)
            for k, ev in enumerate(evs):
                code, consts, rots = ev.flatten()
                g = _lib.MiraGraph(code.ctypes.data, len(code), ev.num_intermediates, len(consts), consts.ctypes.data, rots.ctypes.data, len(rots), 0)
                lib.check(lib.c.mira_graph_eval_device(field, ctypes.byref(g), table, len(cols), chal_m.ctypes.data_as(ctypes.c_void_p), len(chal), rows,
                                                       ctypes.c_void_p(d_all)))
                E.same_bytes(dev.get(d_all, rows), want[k], f"{tag}graph one-shot field={field} rows={rows} graph {k}")
            if specialised:
                assert all(ev.is_specialized(len(chal), len(cols), lib=lib) for ev in evs)
            for k, ev in enumerate(evs):
                ev.evaluate_device(cols, chal, rows, d_out=d_all, lib=lib)
                E.same_bytes(dev.get(d_all, rows), want[k], f"{tag}graph {engine} field={field} rows={rows} graph {k}")
            G.GraphEvaluator.evaluate_batch_device(evs, cols, chal, rows, [d_all + k * rows * 32 for k in range(len(evs))], lib=lib)
            got = dev.get(d_all, len(evs) * rows).reshape(len(evs), rows, 4)
            for k in range(len(evs)):
                E.same_bytes(got[k], want[k], f"{tag}graph {engine} batch field={field} rows={rows} graph {k}")
    finally:
        if own:
            for ev in evs:
                ev.close()


def check_graph_sequence(lib, field, specialise=False, rows=(2048, 64, 2048, 300)):
    """2048 -> 64 -> 2048 -> 300 rows with one set of compiled graphs (g.graph_ws holds the intermediates of every lane of a launch);
    `specialise`: through kernels of their own (mira_graph_specialize: GPU only), compiled once for all row counts"""
    from harness import graph_evaluator as G
    exprs, arrs, _ = graph_case(field, rows[0])
    evs = [G.GraphEvaluator.new(e, field) for e in exprs]
    try:
        if specialise:
            kinds = [(None, G.COL_BOOL)] * len(arrs["selectors"]) + [(None, G.COL_FIELD)] * len(arrs["fixed"] + arrs["advice"])
            assert G.GraphEvaluator.specialize(evs, kinds, len(arrs["challenges"]), lib=lib), lib.c.mira_last_error()
        for i, n in enumerate(rows):
            check_graph_rows(lib, field, n, evs=evs, specialised=specialise, tag=f"step {i}: ")
    finally:
        for ev in evs:
            ev.close()


def check_setup(lib, curve, k=6, chunk=24):
    """a key of 2^k points by hash-to-curve, generated in chunks of `chunk` points through g.setup_stage"""
    import setup_cases as SC
    SC.check_key(lib, curve, k, SC.LABELS[1], chunk)
    SC.check_key(lib, curve, k, SC.LABELS[1], -1)


# ---- one interleaved schedule ---------------------------------------------------------------------------------------------------
def schedule(large, small, routes, calls=60, seed=0x5CED):
    """-> the fixed list of (family, kwargs): `calls` draws from all families, seeded"""
    rng = random.Random(seed)
    out = []
    for i in range(calls):
        family = rng.choice(["msm", "msm", "msm", "ntt", "fold", "lookup", "invert", "deciders", "graph", "pow_tree", "setup"])
        if family == "msm":
            out.append((family, dict(name=rng.choice(routes), curve=rng.randrange(2), n=rng.choice([large, small, small, 257, 1]), kind=rng.choice(KINDS))))
        elif family == "ntt":
            out.append((family, dict(k=rng.choice([3, 5, 9, 10]), wave=rng.choice([None, 0, 1]), ops=[rng.choice(E.NTT_OPS)])))
        elif family == "fold":
            out.append((family, dict(field=rng.randrange(2), lengths=[rng.choice([1, 257, 1025])])))
        elif family == "lookup":
            out.append((family, dict(field=rng.randrange(2), shapes=[rng.choice(GD.LOOKUP_SHAPES)], hashes=[rng.choice([None, 1])])))
        elif family == "invert":
            out.append((family, dict(field=rng.randrange(2), lengths=[rng.choice([1, 7, 2049])], chunks=[rng.choice([None, 3])])))
        elif family == "deciders":
            out.append((family, dict(field=rng.randrange(2), lengths=[rng.choice([1, 257, 1025])])))
        elif family == "graph":
            out.append((family, dict(field=rng.randrange(2), rows=rng.choice([64, 300]))))
        elif family == "pow_tree":
            out.append((family, dict(field=rng.randrange(2), sizes=[rng.choice([1, 6, 11])])))
        else:
            out.append((family, dict(curve=rng.randrange(2), lengths=[64])))
    assert {f for f, _ in out} == {"msm", "ntt", "fold", "lookup", "invert", "deciders", "graph", "pow_tree", "setup"}
    return out


def check_schedule(lib, large, small, routes, calls=60, bench=None):
    """the randomised soaks made deterministic and small: every result of the list is checked"""
    run = {"ntt": lambda **kw: E.check_ntt(lib, limit=2, roundtrip=False, **kw), "fold": lambda **kw: GD.check_fold(lib, offsets=(1,), **kw),
           "lookup": lambda **kw: GD.check_lookup(lib, offsets=(3,), **kw), "invert": lambda **kw: GD.check_batch_invert(lib, offsets=(1,), **kw),
           "deciders": lambda **kw: GD.check_deciders(lib, offsets=(3,), **kw), "graph": lambda **kw: check_graph_rows(lib, **kw),
           "pow_tree": lambda **kw: GD.check_pow_tree(lib, offsets=(0,), **kw), "setup": lambda **kw: GD.check_generators(lib, offsets=(1,), **kw)}
    with Borrowed(bench or shared_bench(lib, large)) as bench:
        prime_stats(bench, [(kw["name"], kw["curve"], kw["n"], kw["kind"]) for family, kw in schedule(large, small, routes, calls) if family == "msm"])
        for i, (family, kw) in enumerate(schedule(large, small, routes, calls)):
            try:
                if family == "msm":
                    run_route(bench, tag=f"[schedule call {i}] ", **kw)
                else:
                    run[family](**kw)
            except AssertionError as err:
                raise AssertionError(f"schedule call {i} ({family} {kw}): {err}") from err


# ---- after a refusal ------------------------------------------------------------------------------------------------------------
def refused(lib, code, call, what):
    try:
        call()
    except _lib.MiraError as err:
        assert err.code == code, f"{what}: refused with {err.code} ({err}), want {code}"
    else:
        raise AssertionError(f"{what}: not refused")


def check_refusals(lib, n=1025, tmp_dir=None):
    """The error paths that run kernels before they refuse -- a non-canonical element given to count_ne / sum_sub and to the lookup
    vectors, a key file with a point off the curve -- and TooLongInput and an unknown handle: after each, the error code, then the
    next valid call of the same family and one commit against their references."""
    import tempfile
    ref = reference(n)
    with Bench(lib, n) as bench:
        def commit(after, curve):
            run_route(bench, "planned", curve, n, "witness", f"[after {after}] ")
        for field in E.FIELDS:
            cv, reps, p = E._Convert(field), E.representations(field), MODULUS[field]
            curve = 0 if field == E.FIELD_FR else 1
            a = E.cycled(reps, n, 1)
            b = [reps[(i + 2 + (i % 5 == 4)) % len(reps)] for i in range(n)]
            diff = [i for i in range(n) if a[i] != b[i]]
            want_ne = (len(diff), diff[0])
            want_sub = cv.array([sum(cv.values(a)) - sum(cv.values(b))])
            for bad, at in ((p, n - 1), ((1 << 256) - 1, 300)):
                x = list(a)
                x[at] = bad
                with E.Dev(lib) as dev:
                    d_a, d_b, d_x = dev.put(a), dev.put(b), dev.put(x)
                    tag = f"field={field} non-canonical {hex(bad)[:8]}.. at {at}"
                    refused(lib, _lib.MIRA_E_BAD_ARG, lambda: DC.count_ne_device(field, d_x, d_b, n, lib=lib), "count_ne " + tag)
                    assert DC.count_ne_device(field, d_a, d_b, n, lib=lib) == want_ne, "count_ne after a refusal, " + tag
                    commit("count_ne refused", curve)
                    refused(lib, _lib.MIRA_E_BAD_ARG, lambda: DC.sum_sub_device(field, d_a, d_x, n, lib=lib), "sum_sub " + tag)
                    GD.same(DC.sum_sub_device(field, d_a, d_b, n, lib=lib), want_sub, "sum_sub after a refusal, " + tag)
                    assert DC.count_ne_device(field, d_a, d_b, n, lib=lib) == want_ne, "count_ne after a refused sum_sub, " + tag
                    commit("sum_sub refused", curve)
            # the lookup vectors: a non-canonical element in l, then in t; the next call of each kind gives the reference's vectors
            from test_lookup_witness_emu import ref_h_g, ref_m
            n_l, n_t = 257, 255
            l, t = GD.lookup_case(field, n_l, n_t)
            m_ints = ref_m(l, t)
            r = cv.value(reps[9])
            h_ints, g_ints = ref_h_g(cv.values(l), cv.values(t), m_ints, r, p)
            for mode in (None, 1):
                for which, at in (("l", n_l - 1), ("t", 17)):
                    bl, bt = list(l), list(t)
                    (bl if which == "l" else bt)[at] = p + 1
                    tag = f"field={field} hash={mode} non-canonical {which}[{at}]"
                    with E.knobs(lib, LOOKUP_HASH=mode), E.Dev(lib) as dev:
                        d_l, d_t, d_bl, d_bt, d_m, d_h, d_g = dev.put(l), dev.put(t), dev.put(bl), dev.put(bt), dev.empty(n_t), dev.empty(n_l), dev.empty(n_t)
                        refused(lib, _lib.MIRA_E_BAD_ARG, lambda: LU.evaluate_m_device(field, d_m, d_bl, n_l, d_bt, n_t, lib=lib), "lookup_m " + tag)
                        LU.evaluate_m_device(field, d_m, d_l, n_l, d_t, n_t, lib=lib)
                        E.same_bytes(dev.get(d_m, n_t), cv.array(m_ints), "lookup_m after a refusal, " + tag)
                        refused(lib, _lib.MIRA_E_BAD_ARG, lambda: LU.evaluate_h_g_device(field, d_h, d_g, d_bl, n_l, d_bt, d_m, n_t, r, lib=lib), "lookup_h_g " + tag)
                        LU.evaluate_h_g_device(field, d_h, d_g, d_l, n_l, d_t, d_m, n_t, r, lib=lib)
                        E.same_bytes(dev.get(d_h, n_l), cv.array(h_ints), "lookup h after a refusal, " + tag)
                        E.same_bytes(dev.get(d_g, n_t), cv.array(g_ints), "lookup g after a refusal, " + tag)
                        commit("lookup refused", curve)
        # a key file with a point off the curve, loaded with validation
        with tempfile.TemporaryDirectory(dir=tmp_dir) as tmp:
            for curve in CURVES:
                k = 10
                raw = ref.bases[curve][:1 << k].copy()
                good = os.path.join(tmp, f"good{curve}.bin")
                raw.tofile(good)
                raw[777, 4] ^= np.uint64(1)                                 # y of point 777: canonical still, off the curve
                bad = os.path.join(tmp, f"bad{curve}.bin")
                raw.tofile(bad)
                h = ctypes.c_uint64()
                rc = lib.c.mira_msm_register_bases_file(curve, bad.encode(), k, 1, ctypes.byref(h))
                assert rc == _lib.MIRA_E_INVALID_POINT, f"key file with a point off the curve, curve={curve}: rc={rc}"
                commit("a key file refused", curve)
                key = CM.CommitmentKey.load_from_file(curve, good, k, lib=lib, validate=True)
                try:
                    same_point(key.commit_device(bench.vector(curve, "dense"), 1 << k), ref.point(curve, "dense", 1 << k), f"a valid key file after a refused one, curve={curve}")
                finally:
                    key.close()
        # TooLongInput and an unknown handle
        for curve in CURVES:
            key = bench.key(curve)
            out = np.zeros(8, dtype=np.uint64)
            vp = out.ctypes.data_as(ctypes.c_void_p)
            rc = lib.c.mira_msm_device(key.handle, ctypes.c_void_p(bench.vector(curve, "dense")), n + 1, vp)
            assert rc == _lib.MIRA_E_TOO_LONG, f"too long: rc={rc}"
            try:
                key.commit_device(bench.vector(curve, "dense"), n + 1)
            except CM.TooLongInput as err:
                assert (err.input_len, err.limit) == (n + 1, n)
            else:
                raise AssertionError("TooLongInput not raised")
            commit("TooLongInput", curve)
            rc = lib.c.mira_msm_device(0xDEAD0000, ctypes.c_void_p(bench.vector(curve, "dense")), 10, vp)
            assert rc == _lib.MIRA_E_BAD_ARG, f"unknown handle: rc={rc}"
            commit("an unknown handle", curve)
            run_route(bench, "batch_device", curve, n, "dense", "[after an unknown handle] ")


# ---- fresh, poisoned workspaces -------------------------------------------------------------------------------------------------
PLUMBING = ("mira_dev_", "mira_last_", "mira_msm_last_")
PLUMBING_NAMES = ("mira_set_tuning", "mira_msm_set_window_bits", "mira_set_timing", "mira_get_timings", "mira_trim")


class TrimFirst:
    """lib.c behind a proxy that releases every workspace (mira_trim(0, NULL)) before every compute entry point; the pure plumbing --
    mira_dev_*, mira_set_tuning, mira_msm_set_window_bits, mira_last_*, timing and mira_trim itself -- passes through"""

    def __init__(self, c):
        self._c, self.trims = c, 0

    def __getattr__(self, name):
        fn = getattr(self._c, name)
        if name.startswith(PLUMBING) or name in PLUMBING_NAMES:
            return fn

        def call(*args):
            rc = self._c.mira_trim(0, None)
            assert rc == 0, f"mira_trim before {name}: {rc}"
            self.trims += 1
            return fn(*args)
        return call


def fill_byte():
    """the byte glibc fills a new allocation with under MALLOC_PERTURB_ = v: the complement of v's low byte"""
    return ~int(os.environ["MALLOC_PERTURB_"]) & 0xFF


def prove_fill(lib):
    import platform
    if platform.libc_ver()[0] != "glibc":
        print("skip: MALLOC_PERTURB_ is glibc's, this C library is " + repr(platform.libc_ver()), flush=True)
        sys.exit(0)
    want = fill_byte()
    for nbytes in (4096, 1 << 20):
        p = lib.alloc(nbytes)
        got = lib.download(p, nbytes, np.uint8)
        lib.free(p)
        if not (got == want).all():
            sys.exit(f"the fill is not active: a new allocation of {nbytes} bytes holds {sorted(set(got.tolist()))[:8]}, not {want:#x} everywhere "
                     f"(MALLOC_PERTURB_={os.environ.get('MALLOC_PERTURB_')})")
    print(f"fill {want:#04x} active", flush=True)


def check_is_sat_perm(lib, field=E.FIELD_FR):
    pairs, z, bad_z, want = perm_case(field, 67, 1, 0xD7)
    pm = DC.PermutationMatrix(field, pairs, 67, lib=lib)
    try:
        with E.Dev(lib) as dev:
            DC.is_sat_perm_device(pm, E.to_array(z[:1]), dev.put(z[1:]), 66, 1)
            assert pm.check_device(E.to_array(bad_z[:1]), dev.put(bad_z[1:]), 66) == want
    finally:
        pm.close()


CASES = {"edge_" + name: fn for name, fn in E.CASES.items()}
CASES.update({"guarded_deciders": GD.check_deciders, "guarded_lookup": GD.check_lookup, "guarded_pow_tree": GD.check_pow_tree,
              "guarded_generators": GD.check_generators, "guarded_msm_io": GD.check_msm_io, "guarded_ntt_device": GD.check_ntt_device,
              "routes": check_routes, "pairs": check_pairs, "ntt_sequence": check_ntt_sequence, "lookup_sequence": check_lookup_sequence,
              "decider_sequence": check_decider_sequence, "pow_tree_sequence": check_pow_tree_sequence, "fold_sequence": check_fold_sequence,
              "graph_sequence": check_graph_sequence, "setup": check_setup, "is_sat_perm": check_is_sat_perm, "schedule": check_schedule,
              "refusals": check_refusals})


def main(argv):
    lib = _lib.MiraLib(argv[1])
    mode = argv[2]
    if mode == "poison":
        prove_fill(lib)
        lib.c = TrimFirst(lib.c)
    elif mode != "plain":
        sys.exit("mode: plain or poison")
    import time
    import traceback
    failed = 0
    for spec in argv[3:]:
        name, _, kwargs = spec.partition(":")
        print(f"run {spec}", flush=True)
        t0 = time.time()
        try:
            CASES[name](lib, **(json.loads(kwargs) if kwargs else {}))
        except Exception:                                                   # a wrong value: the cases after it still run (a signal ends them all)
            failed += 1
            print(traceback.format_exc()[-3000:], flush=True)
            print(f"failed {spec}", flush=True)
            continue
        print(f"ok {spec}", flush=True)
        print(f"   {time.time() - t0:.1f} s" + (f", {lib.c.trims} trims so far" if mode == "poison" else ""), flush=True)
    close_benches()
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main(sys.argv)
