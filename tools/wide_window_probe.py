"""Wall time of one commit under 15- to 20-bit windows on a plain key (no endomorphism copy), the measurement behind WIDE_WALLS
(mira_amd/csrc/msm_plan.hip).  For every size: one synthetic key and one vector of uniform scalars in device memory, every width
run once to warm up, then --reps rounds that take the widths in turn (so that clock and thermal drift fall on all of them
alike); the median of the rounds per width, from the host clock around commit_device (which returns after the stream is
synchronised).  Every width must give the same point.

    python tools/wide_window_probe.py [--sizes 20,22,24,26,28] [--widths 15-20] [--reps 5] [--out profiles/r05_wide_windows.txt]

With --out '' nothing is written (kernel-trace runs under rocprofv3).
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mira_amd import _lib, commitment as cm  # noqa: E402


def parse_widths(s):
    if "-" in s:
        lo, hi = s.split("-")
        return list(range(int(lo), int(hi) + 1))
    return [int(x) for x in s.split(",")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="20,22,24,26,28", help="log2 of the pairs")
    ap.add_argument("--widths", default="15-20")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--curve", type=int, default=cm.CURVE_BN256)
    ap.add_argument("--out", default=os.path.join("profiles", "r05_wide_windows.txt"))
    args = ap.parse_args()
    lib = _lib.load()
    lib.tune(_lib.TUNE_GLV_AUTO_MAX_LOG, 0)                   # plain keys
    widths = parse_widths(args.widths)
    lines = ["# wall time of one commit in microseconds, uniform scalars in device memory, plain key, curve %d; median of %d rounds"
             % (args.curve, args.reps),
             "# (tools/wide_window_probe.py; widths alternate within each round; rate = pairs / time at the best width)",
             "log_n  " + "  ".join("c=%-6d" % c for c in widths) + "  best  M_pairs/s(best)  M_pairs/s(c=16)"]
    print(lines[-1], flush=True)
    for log_n in (int(x) for x in args.sizes.split(",")):
        n = 1 << log_n
        key = cm.CommitmentKey.synthetic(args.curve, n, seed=0x57494445 + log_n)
        d = cm.synth_scalars_device(args.curve, n, seed=0x53434C52 + log_n)
        times = {c: [] for c in widths}
        ref = None
        for c in widths:                                      # warm-up: allocations of the widest workspaces, code objects
            key.set_window_bits(c)
            pt = key.commit_device(d, n)
            if ref is None:
                ref = pt
            assert (pt == ref).all(), "width %d disagrees at 2^%d" % (c, log_n)
        for _ in range(args.reps):
            for c in widths:
                key.set_window_bits(c)
                t0 = time.perf_counter()
                key.commit_device(d, n)
                times[c].append((time.perf_counter() - t0) * 1e6)
        med = {c: statistics.median(v) for c, v in times.items()}
        best = min(widths, key=lambda c: med[c])
        row = "%5d  " % log_n + "  ".join("%8.0f" % med[c] for c in widths) + "  %4d  %15.0f  %15s" % (
            best, n / med[best], ("%.0f" % (n / med[16])) if 16 in med else "-")
        print(row, flush=True)
        lines.append(row)
        key.close()
        lib.free(d)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
