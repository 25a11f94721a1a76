"""mira_msm_tuning_export / mira_msm_tuning_import through ctypes and mira_amd.commitment, on the test-only host emulation of
the kernel sources: a key of 2^12 synthetic points commits the same 2^12 scalars until the width trial of that shape is done
(n * count = 2^12 is the smallest shape that opens one), its blob goes into the same key registered again under a new handle,
and that key's FIRST commit must report the settled plan and return the oracle's point.  Then the corners of the ABI pair: the
size query, a buffer that is too small, a handle nobody registered, malformed and foreign blobs, and the file helpers."""
import ctypes
import struct

import pytest

from mira_amd import _lib
from mira_amd import commitment as cm
from oracle import cref as C

N = 1 << 12
KNOBS = [_lib.TUNE_PLAN_HIST_MIN_N, _lib.TUNE_TABLE_WIDTH, _lib.TUNE_GLV, _lib.TUNE_SHARED_MIN_N, _lib.TUNE_GLV_AUTO_MAX_LOG, _lib.TUNE_WIDTH_TRIALS]


@pytest.fixture(scope="module")
def case():
    """per curve: bases, scalars and the oracle's commitment, computed once"""
    out = {}
    for cid in (0, 1):
        bases, sc = C.synth_bases(cid, N, seed=700 + cid), C.synth_scalars(cid, N, seed=710 + cid)
        out[cid] = (bases, sc, C.commit(cid, bases, sc))
    return out


@pytest.fixture
def lib(emu_lib):
    for k in KNOBS:
        emu_lib.tune(k, -1)
    emu_lib.check(emu_lib.c.mira_msm_set_window_bits(0))
    return emu_lib


def last_plan(lib):
    c, w, t = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    lib.check(lib.c.mira_msm_last_plan(ctypes.byref(c), ctypes.byref(w)))
    lib.check(lib.c.mira_msm_last_table_bits(ctypes.byref(t)))
    return c.value, w.value, t.value


def settle(lib, key, d_scalars, want):
    """commit until the shape's trial is done: the finished record, and the plan the key then commits under"""
    for _ in range(12):
        assert (key.commit_device(d_scalars, N) == want).all()
        done = [r for r in key.tuning_records() if r["n"] == N and r["count"] == 1]
        if done:
            assert len(done) == 1
            assert (key.commit_device(d_scalars, N) == want).all()
            return done[0], last_plan(lib)
    pytest.fail("the trial of a 2^12 commit is not done after 12 commits")


@pytest.mark.parametrize("cid", [0, 1])
def test_a_key_registered_again_starts_settled(lib, case, cid):
    bases, sc, want = case[cid]
    d = lib.alloc(N * 32)
    a = b = fresh = None
    try:
        lib.upload(d, sc)
        a = cm.CommitmentKey(cid, bases, lib=lib)
        assert list(a.tuning_records()) == [] and a.tuning_records().stats is None
        assert (a.commit_device(d, N) == want).all()
        model = last_plan(lib)
        assert list(a.tuning_records()) == []                      # a running trial is not exported
        rec, settled = settle(lib, a, d, want)
        assert settled[0] == rec["best_c"] and rec["c0"] == model[0] and rec["kind"] & 4 == 0
        blob = a.export_tuning()
        assert a.export_tuning() == blob
        ident = a.tuning_records(blob).identity
        assert (ident["arch"], ident["curve"], ident["n"], ident["max_c"], ident["sets"], ident["table_c"]) == ("emu", cid, N, 16, [], 0)

        b = cm.CommitmentKey(cid, bases, lib=lib)
        assert b.handle != a.handle
        assert b.import_tuning(blob) is True
        assert (b.commit_device(d, N) == want).all()               # the FIRST commit of the new handle
        assert last_plan(lib) == settled
        assert b.export_tuning() == blob
        assert list(b.tuning_records()) == [rec]

        fresh = cm.CommitmentKey(cid, bases, lib=lib)                # a key that never imports starts at the model's width, as ever
        assert (fresh.commit_device(d, N) == want).all()
        assert last_plan(lib) == model
    finally:
        for key in (a, b, fresh):
            if key is not None:
                key.close()
        lib.free(d)


def _reseal(blob):
    return blob[:-8] + struct.pack("<Q", cm.fnv1a64(blob[:-8]))


def _pinned_blob(key, c):
    """the blob of a key that has settled a device commit of 2^12 pairs at c bits on the plain path: this file's own writer"""
    ident = key.tuning_records().identity
    arch = ident["arch"].encode()
    body = b"MIRATUNE" + struct.pack("<II", 1, len(arch)) + arch + struct.pack("<QIQII", ident["model"], ident["curve"], ident["n"], ident["max_c"], 0)
    body += struct.pack("<II", 0, 1) + struct.pack("<QIIIId", N, 1, 0, 9, c, 123.0) + struct.pack("<I", 0)
    return body + struct.pack("<Q", cm.fnv1a64(body))


def test_abi_corners(lib, case, tmp_path):
    bases, sc, want = case[0]
    key = cm.CommitmentKey(0, bases, lib=lib)
    other = cm.CommitmentKey(0, bases[:N // 2], lib=lib)
    try:
        c = lib.c
        # the size query, and a buffer that is too small: the length comes back either way, nothing is written
        n = ctypes.c_size_t(0)
        assert c.mira_msm_tuning_export(key.handle, None, 0, ctypes.byref(n)) == 0
        empty = key.export_tuning()
        assert n.value == len(empty) and len(empty) > 40
        buf = ctypes.create_string_buffer(b"\xAA" * len(empty), len(empty))
        n = ctypes.c_size_t(0)
        assert c.mira_msm_tuning_export(key.handle, buf, len(empty) - 1, ctypes.byref(n)) == _lib.MIRA_E_BAD_ARG
        assert n.value == len(empty) and buf.raw == b"\xAA" * len(empty) and b"too small" in c.mira_last_error()
        assert c.mira_msm_tuning_export(key.handle, buf, len(empty) + 5, ctypes.byref(n)) == 0 and buf.raw == empty
        assert c.mira_msm_tuning_export(key.handle, None, 8, ctypes.byref(n)) == _lib.MIRA_E_BAD_ARG
        assert c.mira_msm_tuning_export(key.handle, buf, len(empty), None) == _lib.MIRA_E_BAD_ARG
        # a handle nobody registered
        ok = ctypes.c_int32(7)
        assert c.mira_msm_tuning_export(0, None, 0, ctypes.byref(n)) == _lib.MIRA_E_BAD_ARG and b"unknown bases handle" in c.mira_last_error()
        assert c.mira_msm_tuning_import(0, empty, len(empty), ctypes.byref(ok)) == _lib.MIRA_E_BAD_ARG and ok.value == 0
        assert c.mira_msm_tuning_import(key.handle, None, 0, ctypes.byref(ok)) == _lib.MIRA_E_BAD_ARG
        assert c.mira_msm_tuning_import(key.handle, empty, len(empty), None) == _lib.MIRA_E_BAD_ARG

        # accepted, foreign, malformed
        pinned = _pinned_blob(key, 6)
        assert other.import_tuning(pinned) is False and other.export_tuning() != pinned      # another key length: not an error, nothing changed
        assert key.import_tuning(_reseal(pinned.replace(b"emu", b"emv", 1))) is False and key.export_tuning() == empty
        for bad in (pinned[:-1], pinned + b"\0", pinned[:50] + bytes([pinned[50] ^ 1]) + pinned[51:], _pinned_blob(key, 3), _pinned_blob(key, 17), b""):
            with pytest.raises(_lib.MiraError) as e:
                key.import_tuning(bad)
            assert e.value.code == _lib.MIRA_E_BAD_ARG and "tuning blob" in str(e.value)
            assert key.export_tuning() == empty
        assert key.import_tuning(pinned) is True and key.export_tuning() == pinned
        lib.tune(_lib.TUNE_GLV, 0)                                  # (the record is the plain path's)
        d = lib.alloc(N * 32)
        try:
            lib.upload(d, sc)
            assert (key.commit_device(d, N) == want).all()
            assert last_plan(lib) == (6, 43, 0)                     # the pinned width, from the first commit on
        finally:
            lib.free(d)

        # the file helpers
        path = tmp_path / "cache" / "bn256"
        path.mkdir(parents=True)
        path = path / "12.tuning"
        assert key.load_tuning(path) is False                       # no file: nothing to load, no error
        blob = key.export_tuning()
        key.save_tuning(path)
        assert path.read_bytes() == blob and [p.name for p in path.parent.iterdir()] == ["12.tuning"]     # no temporary file left
        key.save_tuning(path)                                       # over an existing file
        again = cm.CommitmentKey(0, bases, lib=lib)
        try:
            assert again.load_tuning(path) is True and again.export_tuning() == blob
            assert other.load_tuning(path) is False
            path.write_bytes(blob[:-3])
            with pytest.raises(_lib.MiraError):
                again.load_tuning(path)
        finally:
            again.close()
    finally:
        lib.tune(_lib.TUNE_GLV, -1)
        key.close()
        other.close()
