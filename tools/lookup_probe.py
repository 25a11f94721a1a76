"""Probe: device time of the lookup argument's witness rounds -- m (mira_lookup_m_device), h + g (mira_lookup_h_g_device)
and a plain batch inversion of the same length -- at 2^13 .. 2^22 rows, both fields, on two input shapes:

  distinct     t = random distinct values, l = random picks from t
  duplicates   the reference circuit's shape: t = 25 values then zeros, every l the same table value

Stage times come from the library's stage timers (median of --reps calls after a warm-up).
usage: python tools/lookup_probe.py [--min-log 13] [--max-log 22] [--reps 5] [--fields 0,1]"""
import argparse
import os
import random
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mira_amd import _lib  # noqa: E402
from mira_amd import lookup as LU  # noqa: E402
from mira_amd.graph_evaluator import MODULUS  # noqa: E402


def rand_canonical(rng, n, mod):
    a = rng.integers(0, 2 ** 63, size=(n, 4), dtype=np.uint64) * np.uint64(2)
    a[:, 3] = rng.integers(0, mod >> 192, size=n, dtype=np.uint64)
    return a


def inputs(shape, n, mod, rng):
    if shape == "distinct":
        t = rand_canonical(rng, n, mod)
        return t[rng.integers(0, n, size=n)], t
    t = np.zeros((n, 4), dtype=np.uint64)
    t[:25] = rand_canonical(rng, 25, mod)
    return np.repeat(t[3:4], n, axis=0), t


def stage_ms(lib, fn):
    fn()
    return sum(ms for _, ms in lib.timings())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-log", type=int, default=13)
    ap.add_argument("--max-log", type=int, default=22)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fields", default="0,1")
    a = ap.parse_args()
    lib = _lib.load()
    lib.check(lib.c.mira_set_timing(1))
    print("field shape      log_n   m_ms    h_g_ms  m+h+g_ms  inv_ms   (median of %d)" % a.reps, flush=True)
    for field in [int(f) for f in a.fields.split(",")]:
        mod = MODULUS[field]
        r = random.Random(field).randrange(mod)
        for shape in ("distinct", "duplicates"):
            for log_n in range(a.min_log, a.max_log + 1):
                n = 1 << log_n
                l, t = inputs(shape, n, mod, np.random.default_rng(log_n))
                ptrs = [lib.alloc(n * 32) for _ in range(5)]
                d_l, d_t, d_m, d_h, d_g = ptrs
                try:
                    lib.upload(d_l, l)
                    lib.upload(d_t, t)
                    run_m = lambda: LU.evaluate_m_device(field, d_m, d_l, n, d_t, n, lib=lib)
                    run_hg = lambda: LU.evaluate_h_g_device(field, d_h, d_g, d_l, n, d_t, d_m, n, r, lib=lib)
                    run_inv = lambda: LU.batch_invert_device(field, d_h, d_l, n, lib=lib)
                    res = {}
                    for name, fn in (("m", run_m), ("hg", run_hg), ("inv", run_inv)):
                        fn()
                        res[name] = statistics.median(stage_ms(lib, fn) for _ in range(a.reps))
                    print("%-5d %-10s %5d %8.3f %8.3f %9.3f %8.3f" % (field, shape, log_n, res["m"], res["hg"], res["m"] + res["hg"], res["inv"]), flush=True)
                finally:
                    for p in ptrs:
                        lib.free(p)
    lib.check(lib.c.mira_set_timing(0))


if __name__ == "__main__":
    main()
