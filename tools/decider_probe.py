"""Measurement: is_sat_relaxed on the device against the download-and-compare route, for the primary circuit of an IVC step
(two MainGate<5>: 14 advice columns, 30 fixed columns, 2^k rows, bn256::Fr, committed on BN256 G1).

device route    mira_amd.decider.is_sat_relaxed_device, itemised: evaluation (mira_graph_eval_compiled), evaluation + compare
                (mira_graph_check_compiled), compare alone (mira_count_ne_device), one log-derivative sum over two 2^k vectors
                (mira_sum_sub_device; the MainGate circuit has no lookup, so the decider itself runs none) and the re-commitments
host route      what a caller had before: mira_graph_eval_compiled, mira_dev_download of the evaluation, E and W, a numpy compare
                (the re-commitments are the same device calls on both routes)

Every item is warmed up and then repeated for at least --seconds of wall time (sustained load); the median is reported.
usage: python tools/decider_probe.py [--k 17] [--seconds 1.0] [--out FILE]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from harness import graph_evaluator as G, main_gate as MG
from mira_amd import _lib, commitment as cm, decider as D


def sustained(fn, seconds, warmup=3):
    for _ in range(warmup):
        fn()
    ts, t_end = [], time.perf_counter() + seconds
    while time.perf_counter() < t_end or len(ts) < 5:
        t0 = time.perf_counter(); fn(); ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return {"median_ms": round(ts[len(ts) // 2], 4), "min_ms": round(ts[0], 4), "runs": len(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=17)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = _lib.load()
    field, cid, n = G.FIELD_FR, 0, 1 << a.k
    cg, ctx = MG.compressed_circuit(5, 2)
    f_ev = G.GraphEvaluator.new(cg.homogeneous, field)
    nw = ctx.num_advice * n
    d_fix = cm.synth_scalars_device(cid, ctx.num_fixed * n, seed=1)
    d_w = cm.synth_scalars_device(cid, nw, seed=2, kind=1)
    chal = [(77 + j) ** 9 % G.MODULUS[field] for j in range(ctx.num_challenges)]             # [y, u]
    cols = G.PlonkEvalDomain(ctx.num_advice, 0, chal, [], [d_fix + j * n * 32 for j in range(ctx.num_fixed)], [(d_w, nw)], [], n).columns()
    specialised = G.GraphEvaluator.specialize([f_ev], cols, len(chal), lib=lib)
    d_e = f_ev.evaluate_device(cols, chal, n, lib=lib)                                       # E := f(W): a satisfied relaxed pair
    d_f = lib.alloc(n * 32)
    key = cm.CommitmentKey.synthetic(cid, nw, lib=lib)
    w_commit, e_commit = key.commit_device(d_w, nw), key.commit_device(d_e, n)
    D.is_sat_relaxed_device(key, f_ev, cols, chal, n, [d_w], [nw], [w_commit], d_e, e_commit, lib=lib)
    assert D.count_ne_device(field, d_e, None, n, lib=lib)[0] > 0                            # E is not the zero vector

    def host_route():
        f_ev.evaluate_device(cols, chal, n, d_out=d_f, lib=lib)
        f, e, w = lib.download(d_f, (n, 4)), lib.download(d_e, (n, 4)), lib.download(d_w, (nw, 4))
        bad = np.flatnonzero((f != e).any(axis=1))
        assert len(bad) == 0 and len(w) == nw

    def commits():
        assert (key.commit_device(d_w, nw) == w_commit).all() and (key.commit_device(d_e, n) == e_commit).all()
    s = a.seconds
    res = {
        "probe": "decider", "k": a.k, "rows": n, "num_advice": ctx.num_advice, "graph_calculations": f_ev.num_intermediates, "specialised": bool(specialised),
        "evaluation": sustained(lambda: f_ev.evaluate_device(cols, chal, n, d_out=d_f, lib=lib), s),
        "evaluation_and_compare": sustained(lambda: f_ev.check_device(cols, chal, n, d_expected=d_e, lib=lib), s),
        "compare": sustained(lambda: D.count_ne_device(field, d_f, d_e, n, lib=lib), s),
        "sum_sub_2_vectors": sustained(lambda: D.sum_sub_device(field, d_f, d_e, n, lib=lib), s),
        "recommit_W_and_E": sustained(commits, s),
        "is_sat_relaxed_device": sustained(lambda: D.is_sat_relaxed_device(key, f_ev, cols, chal, n, [d_w], [nw], [w_commit], d_e, e_commit, lib=lib), s),
        "host_route_without_commits": sustained(host_route, s),
        "host_route_download_bytes": (nw + 2 * n) * 32,
    }
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    for p in (d_fix, d_w, d_e, d_f):
        lib.free(p)
    f_ev.close(); key.close()


if __name__ == "__main__":
    main()
