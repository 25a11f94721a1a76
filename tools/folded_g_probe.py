"""ProtoGalaxy's compute_G at the fold step's own shape, both routes in one process on one device:

    materialised   harness.protogalaxy.compute_G: per evaluation point a folded trace (one mira_lincomb_device per witness
                   vector), every gate over it into a points x gates x rows leaf array, then the tree
    fused          harness.protogalaxy.compute_G_fused: one mira_graph_eval_folded_reduce (the fold in the column fetch, the
                   first eight tree levels inside the workgroup), then the tree's remaining rounds

The circuit is the reference's MainGate<5> gate (harness/main_gate.py), `--gates` configurations of it (2: the primary circuit
of an IVC step, 14 advice and 30 fixed columns), 2^k rows, one incoming trace; the point count is the one compute_G derives
(degree 5, one trace: 8).  Each route is run once to warm up and then timed as the median of `--runs` wall-clock runs; the
spans come from mira_get_timings, summed over the calls of one run.  Prints one JSON object.

    python tools/folded_g_probe.py [--k 17] [--gates 2] [--runs 20]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from harness import graph_evaluator as G                                     # noqa: E402
from harness import main_gate as MG                                          # noqa: E402
from harness import protogalaxy as PG                                        # noqa: E402
from mira_amd import _lib                                                    # noqa: E402
from mira_amd import commitment as cm                                        # noqa: E402

TIMED = ("mira_lincomb_device", "mira_graph_eval_compiled", "mira_pow_tree_reduce_device", "mira_graph_eval_folded_reduce", "mira_ifft_bn256_fr")


class Spans:
    """stands in for lib.c: adds up the spans of every timed call"""

    def __init__(self, lib):
        self.lib, self.real, self.ms, self.calls = lib, lib.c, {}, {}

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        if name not in TIMED:
            return fn

        def call(*args):
            rc = fn(*args)
            self.calls[name] = self.calls.get(name, 0) + 1
            for span, ms in self.lib.timings():
                self.ms[span] = self.ms.get(span, 0.0) + ms
            return rc
        return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=17)
    ap.add_argument("--gates", type=int, default=2)
    ap.add_argument("--runs", type=int, default=20)
    args = ap.parse_args()
    lib = _lib.load()
    k, n = args.k, 1 << args.k
    gates, ctx = MG.circuit_gates(5, args.gates)
    c = cm.CURVE_BN256                                                       # its scalar field is Fr, the field of the pipeline
    d_fix = cm.synth_scalars_device(c, ctx.num_fixed * n, seed=0x5000)
    d_acc = cm.synth_scalars_device(c, ctx.num_advice * n, seed=0x5100)
    d_inc = cm.synth_scalars_device(c, ctx.num_advice * n, seed=0x5200, kind=1)
    S = PG.Structure(k, gates, [], [d_fix + j * n * 32 for j in range(ctx.num_fixed)], ctx.num_advice)
    acc, inc = PG.Trace([], [(d_acc, ctx.num_advice * n)]), PG.Trace([], [(d_inc, ctx.num_advice * n)])
    levels = (args.gates * n - 1).bit_length()
    bs = [(0x9E3779B97F4A7C15 + 1009 * j) ** 5 % PG.R_MOD for j in range(levels)]
    points = 1 << (1 * S.max_degree()).bit_length()
    calcs = sum(G.GraphEvaluator.new(g, PG.FIELD).num_intermediates for g in gates)
    routes = {"materialised": lambda: PG.compute_G(S, bs, acc, [inc], lib=lib), "fused": lambda: PG.compute_G_fused(S, bs, acc, [inc], lib=lib)}
    out = {"k": k, "rows": n, "gates": args.gates, "advice_columns": ctx.num_advice, "fixed_columns": ctx.num_fixed, "traces": 2, "points": points,
           "calculations_per_row": calcs, "runs": args.runs}
    values = {}
    for name, run in routes.items():
        lib.trim(0)
        free0, _ = lib.mem_info()
        values[name] = run()                                                # warm-up
        held = free0 - lib.mem_info()[0]                                    # what the library keeps between calls (the route's own buffers are freed)
        walls = []
        for _ in range(args.runs):
            t0 = time.perf_counter(); run(); walls.append((time.perf_counter() - t0) * 1e3)
        lib.check(lib.c.mira_set_timing(1))
        spans = Spans(lib)
        lib.c = spans
        try:
            run()
        finally:
            lib.c = spans.real
            lib.check(lib.c.mira_set_timing(0))
        eval_ms = spans.ms.get("graph_eval_folded" if name == "fused" else "graph_eval", 0.0)
        out[name] = {"ms_median": round(sorted(walls)[len(walls) // 2], 3), "ms_min": round(min(walls), 3), "ms_max": round(max(walls), 3),
                     "span_ms": {s: round(v, 3) for s, v in spans.ms.items()}, "calls": spans.calls, "library_workspace_bytes_after": held,
                     "G_calculations_per_s_in_gate_kernels": round(points * calcs * n / eval_ms / 1e6, 2) if eval_ms else None}
    witness = ctx.num_advice * n * 32
    out["materialised"]["peak_route_bytes"] = points * (witness + args.gates * n * 32)       # folded witnesses + leaves, all points alive at the tree
    nodes = points * args.gates * (n >> min(8, k)) * 32
    staging = 2 * (ctx.num_fixed + 2 * ctx.num_advice) * 16 + points * args.gates * 48 + points * 2 * 48 + 8 * 32   # column tables, jobs, coefficients, weights
    out["fused"]["peak_route_bytes"] = nodes + staging                                      # the node buffer + the call's staging
    out["same_coefficients"] = values["materialised"] == values["fused"]
    out["fused_speedup"] = round(out["materialised"]["ms_median"] / out["fused"]["ms_median"], 3)
    for p in (d_fix, d_acc, d_inc):
        lib.free(p)
    print(json.dumps(out, indent=1))
    return 0 if out["same_coefficients"] else 1


if __name__ == "__main__":
    sys.exit(main())
