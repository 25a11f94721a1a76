"""Which route every MSM entry point takes, as far as the C ABI shows it.  `run(lib)` drives one fixed list of calls through
the library object it is given (the host emulation or the device library) and returns one text line per call:

    <label>: rc=<code> err=<mira_last_error(), failures only> plan=<c>,<W> table=<bits> shape=<c>,<W> ok=<0|1>

plan / table are mira_msm_last_plan / mira_msm_last_table_bits after the call (after a refused call: what the call before left),
shape is what a partial call hands back ("-" elsewhere), ok says whether the point -- for a partial: mira_msm_combine of it --
equals the oracle's.  Where a width depends on measured time (a finished trial) the line says only whether it is one of the
trial's candidates.  tests/golden/msm_route_trace.txt is this list as the library answered it BEFORE the routing moved out of
capi.hip into msm_route.hip; test_msm_route_emu.py and test_gpu_msm_route.py hold the library to it line for line.

Labels that start with '@' name rows that tests/emu/test_msm_route.cpp decides too (tests/test_msm_route_host.py compares the
plan, table and shape columns of the two golden files).

Every commit here has at most 2^12 pairs and 2^11 buckets per window: the emulation is slow beyond."""
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # (run as a script: the repository root)
from mira_amd import _lib
from mira_amd import commitment as cm
from oracle import cref as C

N = 1 << 12                      # the smallest key the library builds a GLV copy for, the smallest shape with trials
KNOBS = [_lib.TUNE_TABLE_MIN_N, _lib.TUNE_PLAN_HIST_MIN_N, _lib.TUNE_HOST_CHUNK_MIN_N, _lib.TUNE_TABLE_WIDTH, _lib.TUNE_GLV, _lib.TUNE_SHARED_MIN_N,
         _lib.TUNE_GLV_AUTO_MAX_LOG, _lib.TUNE_WIDTH_TRIALS, _lib.TUNE_WIDE_FRONT_MIN_C]
BATCHES = {1: (600, 600), 3: (300, 350), 9: (100, 100)}         # the matrix (trials off): count -> (n, stride)
TRIAL_BATCH = (1408, 3, 1500)                                   # n, count, stride: n * count >= 2^12, the smallest shape with trials


def _vp(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


class _Trace:
    def __init__(self, lib):
        self.lib, self.c, self.lines = lib, lib.c, []
        self.bases = {cid: C.synth_bases(cid, N, seed=300 + cid) for cid in (0, 1)}
        self.sc = {cid: C.synth_scalars(cid, 3 * N, seed=310 + cid) for cid in (0, 1)}
        self.wit = {cid: C.synth_scalars(cid, N, seed=320 + cid, kind=1) for cid in (0, 1)}
        self.d, self.d_wit, self.want = {}, {}, {}
        for cid in (0, 1):
            self.d[cid] = lib.alloc(3 * N * 32)
            lib.upload(self.d[cid], self.sc[cid])
            self.d_wit[cid] = lib.alloc(N * 32)
            lib.upload(self.d_wit[cid], self.wit[cid])
        self.d_part = lib.alloc(_lib.MIRA_PARTIAL_U64 * 8)
        self.keys = []

    def close(self):
        self.reset()
        for key in self.keys:
            key.close()
        for p in list(self.d.values()) + list(self.d_wit.values()) + [self.d_part]:
            self.lib.free(p)

    def reset(self):
        for k in KNOBS:
            self.lib.tune(k, -1)
        self.lib.check(self.c.mira_msm_set_window_bits(0))

    def key(self, cid):
        k = cm.CommitmentKey(cid, self.bases[cid], lib=self.lib)
        self.keys.append(k)
        return k

    def oracle(self, cid, first, off, n, wit=False):
        """commit of scalars [off, off + n) over the key's points [first, first + n)"""
        k = (cid, first, off, n, wit)
        if k not in self.want:
            self.want[k] = C.commit(cid, self.bases[cid][first:first + n], (self.wit if wit else self.sc)[cid][off:off + n])
        return self.want[k]

    # ---- one line per call
    def last(self):
        c, w, t = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        self.lib.check(self.c.mira_msm_last_plan(ctypes.byref(c), ctypes.byref(w)))
        self.lib.check(self.c.mira_msm_last_table_bits(ctypes.byref(t)))
        return c.value, w.value, t.value

    def line(self, label, rc, shape=None, ok=None, candidates=None):
        c, w, t = self.last()
        err = " err=" + (self.c.mira_last_error() or b"").decode() if rc else ""
        if candidates is not None:                       # a width (or set) that measured time picked: only that it is a candidate
            plan = "in_candidates=%d" % int((t if candidates[0] == "table" else c) in candidates[1])
        else:
            plan = "plan=%d,%d table=%d" % (c, w, t)
        self.lines.append("%s: rc=%d%s %s shape=%s ok=%s" % (label, rc, err, plan, "-" if shape is None or rc else "%d,%d" % shape,
                                                           "-" if ok is None or rc else int(bool(ok))))
        return c, w, t

    # ---- the entry points
    def device(self, label, key, n, d=0, off=0, wit=False, out=True, handle=None, **kw):
        res = np.zeros(8, dtype=np.uint64)
        ptr = None if d is None else (self.d_wit if wit else self.d)[key.curve] + off * 32
        rc = self.c.mira_msm_device(key.handle if handle is None else handle, ptr, n, _vp(res) if out else None)
        return self.line(label, rc, ok=rc == 0 and (res == self.oracle(key.curve, 0, off, min(n, N), wit)).all(), **kw)

    def host(self, label, key, n, null=False, handle=None):
        res = np.zeros(8, dtype=np.uint64)
        rc = self.c.mira_msm(key.handle if handle is None else handle, None if null else _vp(self.sc[key.curve]), n, _vp(res))
        return self.line(label, rc, ok=rc == 0 and (res == self.oracle(key.curve, 0, 0, min(n, N))).all())

    def _batch_ok(self, key, res, n, count, stride):
        return all((res[b] == self.oracle(key.curve, 0, b * stride, min(n, N))).all() for b in range(count))

    def batch_device(self, label, key, n, count, stride, null=False, out=True, **kw):
        res = np.zeros((max(count, 1), 8), dtype=np.uint64)
        rc = self.c.mira_msm_batch_device(key.handle, None if null else self.d[key.curve], n, count, stride, _vp(res) if out else None)
        return self.line(label, rc, ok=rc == 0 and self._batch_ok(key, res, n, count, stride), **kw)

    def batch_host(self, label, key, n, count, stride, null=False, handle=None):
        res = np.zeros((max(count, 1), 8), dtype=np.uint64)
        vs = [np.ascontiguousarray(self.sc[key.curve][b * stride:b * stride + n]) for b in range(count)]
        ptrs = (ctypes.c_void_p * max(count, 1))(*[v.ctypes.data for v in vs])
        rc = self.c.mira_msm_batch(key.handle if handle is None else handle, None if null else ptrs, n, count, _vp(res))
        return self.line(label, rc, ok=rc == 0 and self._batch_ok(key, res, n, count, stride))

    def partial(self, label, key, first, n, width, to_device=False, out=True, handle=None):
        part = np.zeros(_lib.MIRA_PARTIAL_U64, dtype=np.uint64)
        c, w = ctypes.c_int32(width), ctypes.c_int32()
        h = key.handle if handle is None else handle
        if to_device:
            rc = self.c.mira_msm_partial_to_device(h, first, self.d[key.curve], n, self.d_part if out else None, ctypes.byref(c), ctypes.byref(w))
            if rc == 0:
                part = self.lib.download(self.d_part, _lib.MIRA_PARTIAL_U64)
        else:
            rc = self.c.mira_msm_partial_device(h, first, self.d[key.curve], n, _vp(part) if out else None, ctypes.byref(c), ctypes.byref(w))
        ok = False
        if rc == 0:
            ok = (cm.combine_partials(key.curve, part, c.value, w.value, lib=self.lib) == self.oracle(key.curve, first, 0, n)).all()
        return self.line(label, rc, shape=(c.value, w.value), ok=ok)

    # ---- groups of calls
    def matrix(self, mode, key, batches=(3,), wide_partial=False, shared=None, n1=1024):
        """one mode through every entry point (n1: the length of the single commits); shared = "@" marks the rows the host
        program decides too"""
        at = shared or ""
        self.device("%s%s device n=%d" % (at, mode, n1), key, n1)
        self.lib.tune(_lib.TUNE_HOST_CHUNK_MIN_N, 64)
        self.host("%s%s host n=%d" % (at, mode, n1), key, n1)
        for count in batches:
            n, stride = BATCHES[count]
            self.batch_host("%s%s batch host n=%d count=%d" % (at, mode, n, count), key, n, count, stride)
        self.lib.tune(_lib.TUNE_HOST_CHUNK_MIN_N, -1)
        n, stride = BATCHES[3]
        self.batch_device("%s%s batch device n=%d count=3" % (at, mode, n), key, n, 3, stride)
        self.partial("%s%s partial first=100 n=1000 width=9" % (at, mode), key, 100, 1000, 9)
        self.partial("%s%s partial first=50 n=0 width=0" % (at, mode), key, 50, 0, 0)
        if wide_partial:                                 # width 0 on a key with a set: the set's shape (else 16 bits: too slow here)
            self.partial("%s%s partial to device first=0 n=700 width=0" % (at, mode), key, 0, 700, 0, to_device=True)
        else:
            self.partial("%s%s partial to device first=0 n=700 width=10" % (at, mode), key, 0, 700, 10, to_device=True)

    def empties(self, mode, key, shared=None):
        at = shared or ""
        self.device("%s%s empty device" % (at, mode), key, 0, d=None)
        self.host("%s%s empty host" % (at, mode), key, 0, null=True)
        self.batch_device("%s%s empty batch count=2" % (at, mode), key, 0, 2, 0, null=True)
        self.partial("%s%s empty partial first=%d width=0" % (at, mode, N), key, N, 0, 0)
        self.partial("%s%s empty partial first=7 width=9" % (at, mode), key, 7, 0, 9)
        self.partial("%s%s empty partial to device first=%d width=0" % (at, mode, N), key, N, 0, 0, to_device=True)


def run(lib):
    t = _Trace(lib)
    try:
        _run(t, lib)
        return t.lines
    finally:
        t.close()


def _run(t, lib):
    L = _lib
    t.reset()
    # ---- the matrix, trials off: every row is the model's own choice
    lib.tune(L.TUNE_WIDTH_TRIALS, 0)
    k0 = t.key(0)
    lib.tune(L.TUNE_GLV_AUTO_MAX_LOG, 0)                 # no copy is built: the plain path
    t.matrix("glv-auto-off", k0, shared="@")
    t.empties("glv-auto-off", k0, shared="@")
    lib.tune(L.TUNE_GLV_AUTO_MAX_LOG, -1)
    lib.tune(L.TUNE_GLV, 0)
    t.matrix("plain", k0, batches=(1, 3, 9), shared="@")
    lib.tune(L.TUNE_GLV, -1)
    t.matrix("glv-auto", k0, batches=(1, 3, 9), shared="@")   # the first row builds the copy
    t.empties("glv-auto", k0)
    k0.set_window_bits(10)
    t.matrix("handle-width-10", k0, shared="@")
    t.empties("handle-width-10", k0, shared="@")
    k0.set_window_bits(0)
    lib.check(lib.c.mira_msm_set_window_bits(7))
    t.matrix("process-width-7", k0, shared="@")
    lib.check(lib.c.mira_msm_set_window_bits(0))
    k0.set_max_window_bits(20)                           # opted into wide windows; narrow widths take the wide front
    lib.tune(L.TUNE_WIDE_FRONT_MIN_C, 5)
    t.matrix("wide-opt-in", k0, shared="@")
    lib.tune(L.TUNE_GLV, 0)
    t.device("@wide-opt-in plain device n=%d" % N, k0, N)
    lib.tune(L.TUNE_GLV, -1)
    lib.tune(L.TUNE_WIDE_FRONT_MIN_C, -1)
    k0.set_max_window_bits(16)

    k1 = t.key(1)
    k1.precompute(L.TABLE_GLV)
    t.matrix("glv-precomputed", k1, shared="@")
    t.empties("glv-precomputed", k1)

    k2 = t.key(0)
    k2.precompute(11)
    t.matrix("one-set", k2, wide_partial=True, shared="@", n1=N)     # (a set serves single commits from 2^12 pairs)
    t.empties("one-set", k2, shared="@")
    k2.precompute(8)
    lib.tune(L.TUNE_SHARED_MIN_N, 1)
    t.matrix("two-sets", k2, batches=(1, 3, 9), wide_partial=True, shared="@")
    t.empties("two-sets", k2, shared="@")
    lib.tune(L.TUNE_TABLE_WIDTH, 11)
    t.matrix("two-sets-width-11", k2, wide_partial=True, shared="@")
    lib.tune(L.TUNE_TABLE_WIDTH, -1)
    lib.tune(L.TUNE_SHARED_MIN_N, -1)
    lib.tune(L.TUNE_WIDTH_TRIALS, -1)

    # ---- trials: the first ten commits of a shape, then only that the width kept is a candidate
    # (a set trial over two sets is over after four commits -- each set twice -- so from the fifth on only the candidate check)
    kt = t.key(0)
    c0 = None
    for i in range(11):
        c, _, _ = t.device("trial single n=%d commit %d" % (N, i + 1), kt, N, candidates=None if i < 10 else ("c", range(c0 - 2, c0 + 3)))
        c0 = c if i == 0 else c0
    kb = t.key(1)
    n, count, stride = TRIAL_BATCH
    for i in range(11):
        c, _, _ = t.batch_device("trial batch n=%d count=3 commit %d" % (n, i + 1), kb, n, count, stride,
                                 candidates=None if i < 10 else ("c", range(c0 - 2, c0 + 3)))
        c0 = c if i == 0 else c0
    lib.tune(L.TUNE_SHARED_MIN_N, 1)
    for i in range(10):
        t.device("trial two sets n=%d commit %d" % (N, i + 1), k2, N, candidates=None if i < 4 else ("table", (8, 11)))
    lib.tune(L.TUNE_WIDTH_TRIALS, 0)
    for i in range(2):
        t.device("@trials-off two sets n=%d commit %d" % (N, i + 1), k2, N)
    lib.tune(L.TUNE_SHARED_MIN_N, -1)
    ko = t.key(0)
    for i in range(2):
        t.device("@trials-off single n=%d commit %d" % (N, i + 1), ko, N)
    for i in range(2):
        t.batch_device("@trials-off batch n=%d count=3 commit %d" % (n, i + 1), ko, n, count, stride)
    lib.tune(L.TUNE_WIDTH_TRIALS, -1)

    # ---- bit-length statistics: collected by one commit, consumed by the next of its length and kind
    ks = t.key(0)
    lib.tune(L.TUNE_PLAN_HIST_MIN_N, 1)
    lib.tune(L.TUNE_GLV, 0)
    t.device("stats 1 witness-like n=%d" % N, ks, N, wit=True)
    t.device("stats 2 same length n=%d" % N, ks, N)
    t.device("stats 3 another length n=3000", ks, 3000)
    lib.tune(L.TUNE_GLV, -1)
    t.device("stats 4 glv n=3000", ks, 3000)
    t.device("stats 5 glv n=3000 again", ks, 3000)
    lib.tune(L.TUNE_PLAN_HIST_MIN_N, -1)

    # ---- wide tables: only empty requests here (2^19 buckets per window otherwise)
    k1.precompute(20)
    t.empties("tables-20", k1, shared="@")
    lib.tune(L.TUNE_TABLE_MIN_N, 1)
    t.empties("tables-20-min-n-1", k1, shared="@")
    lib.tune(L.TUNE_TABLE_MIN_N, 0)
    t.empties("tables-20-min-n-0", k1, shared="@")
    lib.tune(L.TUNE_TABLE_MIN_N, -1)
    k2.precompute(20)
    t.empties("tables-20-and-sets", k2, shared="@")
    lib.tune(L.TUNE_SHARED_MIN_N, 1)
    t.empties("tables-20-and-sets-shared-min-n-1", k2, shared="@")
    lib.tune(L.TUNE_SHARED_MIN_N, -1)

    # ---- refusals, and which check comes first when two arguments are wrong
    kr = t.key(1)
    bad = 0xDEAD0000
    t.device("refuse unknown handle", kr, 10, handle=bad)
    t.host("refuse unknown handle host", kr, 10, handle=bad)
    t.batch_host("refuse unknown handle batch host", kr, 10, 2, 10, handle=bad)
    t.partial("refuse unknown handle partial", kr, 0, 10, 9, handle=bad)
    t.device("refuse too long", kr, N + 1)
    t.host("refuse too long host", kr, N + 1)
    t.batch_device("refuse too long batch", kr, N + 1, 2, N + 1)
    t.batch_host("refuse too long batch host", kr, N + 1, 2, N + 1)
    t.partial("refuse too long partial first=%d n=2" % (N - 1), kr, N - 1, 2, 9)
    t.partial("refuse too long partial first=%d n=0" % (N + 1), kr, N + 1, 0, 9)
    t.partial("refuse too long partial to device", kr, 1, N, 9, to_device=True)
    t.device("refuse null scalars", kr, 10, d=None)
    t.host("refuse null scalars host", kr, 10, null=True)
    t.batch_device("refuse null scalars batch", kr, 10, 2, 10, null=True)
    t.batch_host("refuse null scalars batch host", kr, 10, 2, 10, null=True)
    t.batch_device("refuse stride < n", kr, 10, 2, 9)
    t.batch_device("accept stride < n for count=1", kr, 10, 1, 0)
    for width in (3, 21):
        t.partial("refuse width %d partial" % width, kr, 0, 10, width)
        t.partial("refuse width %d partial to device" % width, kr, 0, 10, width, to_device=True)
    t.device("order: null output before unknown handle", kr, 10, out=False, handle=bad)
    t.device("order: null output before too long", kr, N + 1, out=False)
    t.device("order: unknown handle before too long and null scalars", kr, N + 1, d=None, handle=bad)
    t.device("order: too long before null scalars", kr, N + 1, d=None)
    t.host("order: null scalars before unknown handle host", kr, 10, null=True, handle=bad)
    t.host("order: unknown handle before too long host", kr, N + 1, handle=bad)
    t.batch_device("order: bad batch arguments before too long", kr, N + 1, 2, 5, out=False)
    t.batch_host("order: null scalars before unknown handle batch host", kr, 10, 2, 10, null=True, handle=bad)
    t.partial("order: null output before bad width", kr, 0, 10, 3, out=False)
    t.partial("order: bad width before unknown handle", kr, 0, 10, 21, handle=bad)
    t.partial("order: null output before bad width to device", kr, 0, 10, 3, to_device=True, out=False)
    t.partial("order: bad width before unknown handle to device", kr, 0, 10, 21, to_device=True, handle=bad)


def run_wide_tables(lib):
    """The rows the emulation cannot run: commits of n = 300 through 20-bit tables (2^19 buckets per window), and the 16-bit
    windows of a sharded partial that names no width."""
    t = _Trace(lib)
    try:
        t.reset()
        key = t.key(0)
        t.partial("plain key sharded partial first=10 n=300 width=0", key, 10, 300, 0)
        key.precompute(20)
        lib.tune(_lib.TUNE_TABLE_MIN_N, 1)
        t.device("tables-20 device n=300", key, 300)
        lib.tune(_lib.TUNE_HOST_CHUNK_MIN_N, 64)
        t.host("tables-20 host n=300", key, 300)
        lib.tune(_lib.TUNE_HOST_CHUNK_MIN_N, -1)
        t.partial("tables-20 partial first=10 n=300 width=0", key, 10, 300, 0)
        t.partial("tables-20 partial to device first=10 n=300 width=0", key, 10, 300, 0, to_device=True)
        return t.lines
    finally:
        t.close()


def golden_lines():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "msm_route_trace.txt")) as f:
        return f.read().splitlines()


def assert_same_lines(got, want):
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"line {i + 1}:\n  got  {g}\n  want {w}"
    assert len(got) == len(want), f"{len(got)} lines, want {len(want)}"


if __name__ == "__main__":                               # python tests/msm_route_trace.py <library>: the trace on stdout
    import time
    t0 = time.time()
    print("\n".join(run(_lib.MiraLib(sys.argv[1]))))
    print("%.1f s" % (time.time() - t0), file=sys.stderr)
