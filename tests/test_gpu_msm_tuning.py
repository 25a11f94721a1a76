"""A key's MSM tuning from one PROCESS to the next, on the device (mira_msm_tuning_export / mira_msm_tuning_import).

test_second_process_picks_it_up: three fresh python processes (tests/msm_tuning_child.py), one after the other, each under its
own time limit, the parent stopping at the first that fails.  "settle" commits a fixed vector until the trial of its shape is
done and writes the blob; "import" registers the same key, loads the blob, and its FIRST commit must report exactly the
settled (window_bits, num_windows, table_bits) and the settled point, which must be the oracle's; its export must equal the
file.  "fresh" commits without a blob: the same point.

test_every_legal_width_is_the_same_point: blobs built by this file's own writer from the layout in include/mira_gpu.h pin a
2^12 commit to every width a record may hold; the plan shows the width, the point stays the oracle's.  Widths no trial can
produce are refused before anything runs.

Shapes stay at 2^12 pairs (2^13 over the two shared-bucket sets)."""
import ctypes
import json
import os
import struct
import subprocess
import sys

import pytest

import msm_tuning_child as child
from mira_amd import _lib
from mira_amd import commitment as cm
from oracle import cref as C

HERE = os.path.dirname(os.path.abspath(__file__))
N = child.N
_oracle = {}


def oracle_points(cid, variant):
    """the oracle's commitments of the variant's vectors, computed once"""
    if (cid, variant) not in _oracle:
        v = child.VARIANTS[variant]
        bases, sc = C.synth_bases(cid, v["n"]), child.scalars(cid, variant)
        _oracle[cid, variant] = [[int(x) for x in C.commit(cid, bases, sc[b * v["n"]:(b + 1) * v["n"]])] for b in range(v["count"])]
    return _oracle[cid, variant]


def run_child(role, variant, cid, path):
    res = subprocess.run([sys.executable, os.path.join(HERE, "msm_tuning_child.py"), role, variant, str(cid), str(path)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, f"{role}: exit {res.returncode}\n{res.stdout}{res.stderr}"      # (the parent stops here: no later child starts)
    out = json.loads(res.stdout.strip().splitlines()[-1])
    assert "error" not in out, out
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["plain", "glv", "batch6", "two-sets", "stats"])
@pytest.mark.parametrize("cid", [0, 1])
def test_second_process_picks_it_up(gpu_lib, tmp_path, cid, variant):
    path = tmp_path / "key.tuning"
    want = oracle_points(cid, variant)
    a = run_child("settle", variant, cid, path)
    print("settled:", a["commits"], "commits", a["record"], a["plan"])
    assert a["commits"] <= 12 and a["points"] == want and path.exists()
    kind = a["record"]["kind"]
    if variant == "two-sets":
        assert kind & 4 and a["plan"][0] == 0 and a["plan"][2] == a["record"]["best_c"] and a["plan"][2] in (8, 11)
    else:
        assert not kind & 4 and a["plan"][0] == a["record"]["best_c"] and a["plan"][2] == 0
        assert a["plan"][1] == -(-(128 if kind & 1 else 256) // a["plan"][0])
    if variant == "plain":
        assert kind & 1 == 0
    assert a["stats"] == (variant == "stats")                    # the statistics slot takes part only there
    b = run_child("import", variant, cid, path)
    assert b["accepted"] is True
    assert b["plan"] == a["plan"]                                # the FIRST commit of the second process: the settled plan
    assert b["points"] == a["points"] == want
    assert b["export_equals_file"] is True
    c = run_child("fresh", variant, cid, path)
    assert c["points"] == want


# ---- this file's own writer, from the documented layout
def blob_bytes(ident, records, arch=None):
    arch = (arch or ident["arch"]).encode()
    body = b"MIRATUNE" + struct.pack("<II", 1, len(arch)) + arch
    body += struct.pack("<QIQII", ident["model"], ident["curve"], ident["n"], ident["max_c"], len(ident["sets"])) + struct.pack("<%dI" % len(ident["sets"]), *ident["sets"])
    body += struct.pack("<II", ident["table_c"], len(records))
    for r in records:
        body += struct.pack("<QIIIId", r["n"], r["count"], r["kind"], r["c0"], r["best_c"], r["best_us"])
    body += struct.pack("<I", 0)
    return body + struct.pack("<Q", cm.fnv1a64(body))


def pinned(ident, c, glv):
    return blob_bytes(ident, [dict(n=N, count=1, kind=1 if glv else 0, c0=9, best_c=c, best_us=100.0)])


def last_plan(lib):
    c, w, t = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    lib.check(lib.c.mira_msm_last_plan(ctypes.byref(c), ctypes.byref(w)))
    lib.check(lib.c.mira_msm_last_table_bits(ctypes.byref(t)))
    return c.value, w.value, t.value


@pytest.fixture
def one_key(gpu_lib):
    """per curve: a synthetic key of 2^12 points, the fixed vector on the device, the oracle's point"""
    made = {}

    def get(cid):
        if cid not in made:
            sc = child.scalars(cid, "glv")
            d = gpu_lib.alloc(N * 32)
            gpu_lib.upload(d, sc)
            made[cid] = (cm.CommitmentKey.synthetic(cid, N, lib=gpu_lib), d, oracle_points(cid, "glv")[0])
        return made[cid]
    for knob in (_lib.TUNE_GLV, _lib.TUNE_WIDTH_TRIALS, _lib.TUNE_PLAN_HIST_MIN_N, _lib.TUNE_GLV_AUTO_MAX_LOG):
        gpu_lib.tune(knob, -1)
    yield get
    gpu_lib.tune(_lib.TUNE_GLV, -1)
    for key, d, _ in made.values():
        key.close()
        gpu_lib.free(d)


@pytest.mark.gpu
@pytest.mark.parametrize("glv", [False, True])
@pytest.mark.parametrize("cid", [0, 1])
def test_every_legal_width_is_the_same_point(gpu_lib, one_key, cid, glv):
    key, d, want = one_key(cid)
    gpu_lib.tune(_lib.TUNE_GLV, -1 if glv else 0)
    ident = key.tuning_records().identity
    assert ident["arch"].startswith("gfx") and ident["max_c"] == 16
    for c in range(5 if glv else 4, 17):
        blob = pinned(ident, c, glv)
        assert key.import_tuning(blob) is True                  # (replaces the record of the width before)
        got = key.commit_device(d, N)
        assert last_plan(gpu_lib) == (c, -(-(128 if glv else 256) // c), 0), c
        assert [int(x) for x in got] == want, c
        assert key.export_tuning() == blob
    # widths no trial can have produced: refused before anything is launched, and the next commit is unaffected
    settled = key.export_tuning()
    for c in (3, 17):
        with pytest.raises(_lib.MiraError) as e:
            key.import_tuning(pinned(ident, c, glv))
        assert e.value.code == _lib.MIRA_E_BAD_ARG
        assert key.export_tuning() == settled
        got = key.commit_device(d, N)
        assert last_plan(gpu_lib) == (16, -(-(128 if glv else 256) // 16), 0) and [int(x) for x in got] == want


@pytest.mark.gpu
@pytest.mark.parametrize("cid", [0, 1])
def test_other_device_identity(gpu_lib, one_key, cid):
    """A blob whose architecture string names another device -- checksum recomputed, everything else in order -- is not
    accepted, and the first commit runs at the model's width; the same record under this device's name is taken."""
    shared, d, want = one_key(cid)
    fresh = cm.CommitmentKey.synthetic(cid, N, lib=gpu_lib)
    try:
        ident = fresh.tuning_records().identity
        got = fresh.commit_device(d, N)                          # the model's width for this shape, path included
        model = last_plan(gpu_lib)
        assert [int(x) for x in got] == want
    finally:
        fresh.close()
    glv = model[1] != -(-256 // model[0])                       # which path the model's commit took: the record is for that shape
    c = 6 if model[0] != 6 else 7
    record = [dict(n=N, count=1, kind=1 if glv else 0, c0=model[0], best_c=c, best_us=100.0)]
    key = cm.CommitmentKey.synthetic(cid, N, lib=gpu_lib)
    try:
        empty = key.export_tuning()
        assert key.import_tuning(blob_bytes(ident, record, arch="gfx942")) is False
        assert key.import_tuning(blob_bytes(ident, record, arch=ident["arch"] + ":xnack-")) is False
        assert key.export_tuning() == empty
        got = key.commit_device(d, N)
        assert last_plan(gpu_lib) == model and [int(x) for x in got] == want
    finally:
        key.close()
    key = cm.CommitmentKey.synthetic(cid, N, lib=gpu_lib)
    try:
        assert key.import_tuning(blob_bytes(ident, record)) is True
        got = key.commit_device(d, N)
        assert last_plan(gpu_lib) == (c, -(-(128 if glv else 256) // c), 0) and [int(x) for x in got] == want
    finally:
        key.close()
