"""Child process of tests/test_gpu_msm_tuning.py: one fresh process per role, so that nothing a key has learned can reach the
next one except through the file.

    python msm_tuning_child.py <role> <variant> <curve> <blob path>

role "settle": register the synthetic key, commit the variant's fixed vector(s) until the trial of its shape is done (at most
12 commits), commit once more -- that is the settled plan -- and write the blob.  "import": register the same key, load the
blob, commit ONCE, export again.  "fresh": the same first commit without a blob.  Each prints one JSON line: the
(window_bits, num_windows, table_bits) of its last commit, its point(s), and what the role adds."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np

N = 1 << 12
# variant -> key length, commitments per submission, tuning knobs (by name in mira_amd._lib), shared-bucket sets, 32-bit values
VARIANTS = {
    "plain": dict(n=N, count=1, knobs={"TUNE_GLV": 0}),
    "glv": dict(n=N, count=1),
    "batch6": dict(n=N, count=6),
    "two-sets": dict(n=2 * N, count=1, sets=(8, 11)),         # (2^13: clear of MIRA_TUNE_SHARED_MIN_N's 2^12)
    "stats": dict(n=N, count=1, knobs={"TUNE_PLAN_HIST_MIN_N": N}, short=True),
}


def scalars(cid, variant):
    """the variant's vectors, (count * n, 4): uniform scalars, or 32-bit values (half of them zero) in Montgomery form"""
    from oracle import cref as C
    v = VARIANTS[variant]
    total = v["n"] * v["count"]
    if not v.get("short"):
        return C.synth_scalars(cid, total, seed=900 + cid)
    rng = np.random.RandomState(910 + cid)
    plain = np.zeros((total, 4), dtype=np.uint64)
    plain[:, 0] = rng.randint(0, 1 << 32, size=total, dtype=np.uint64) * rng.randint(0, 2, size=total).astype(np.uint64)
    return C.to_mont(1 - cid, plain)                          # (bn256's scalars are Fr, grumpkin's Fq)


def last_plan(lib):
    c, w, t = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    lib.check(lib.c.mira_msm_last_plan(ctypes.byref(c), ctypes.byref(w)))
    lib.check(lib.c.mira_msm_last_table_bits(ctypes.byref(t)))
    return [c.value, w.value, t.value]


def main():
    role, variant, cid, path = sys.argv[1], sys.argv[2], int(sys.argv[3]), sys.argv[4]
    from mira_amd import _lib
    from mira_amd import commitment as cm
    lib = _lib.load()
    v = VARIANTS[variant]
    n, count = v["n"], v["count"]
    for knob, value in v.get("knobs", {}).items():
        lib.tune(getattr(_lib, knob), value)
    key = cm.CommitmentKey.synthetic(cid, n, lib=lib)
    for c in v.get("sets", ()):
        key.precompute(c)
    d = lib.alloc(n * count * 32)
    lib.upload(d, scalars(cid, variant))

    def commit():
        pts = key.commit_device(d, n) if count == 1 else key.commit_batch_device(d, n, count)
        return [[int(x) for x in p] for p in pts.reshape(-1, 8)]

    out = {"role": role}
    if role == "settle":
        for i in range(12):
            commit()
            done = [r for r in key.tuning_records() if r["n"] == n and r["count"] == count]
            if done:
                break
        else:
            print(json.dumps({"role": role, "error": "the trial is not done after 12 commits"}))
            return 1
        out["commits"], out["record"] = i + 1, done[0]
        out["points"], out["plan"] = commit(), last_plan(lib)
        out["stats"] = key.tuning_records().stats is not None
        key.save_tuning(path)
    elif role == "import":
        out["accepted"] = key.load_tuning(path)
        out["points"], out["plan"] = commit(), last_plan(lib)
        with open(path, "rb") as f:
            out["export_equals_file"] = key.export_tuning() == f.read()
    else:
        out["points"], out["plan"] = commit(), last_plan(lib)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
