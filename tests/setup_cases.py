"""Key setup by hash-to-curve (mira_setup_bases_device, mira_hash_to_field_device, mira_map_to_curve_device,
mira_msm_setup_bases) against the plain-Python restatement tests/setup_ref.py: the cases tests/test_setup_emu.py runs on
the CPU emulation at k = 6 and tests/test_gpu_setup.py on the device at k = 10."""
import ctypes
import hashlib
import random

import numpy as np

import setup_ref as R
from mira_amd import _lib

CURVES = (0, 1)
LABELS = (b"", b"mira setup test")


def set_chunk(lib, points):
    lib.tune(_lib.TUNE_SETUP_CHUNK, points)


def setup_bytes(lib, curve, label, first, n):
    """mira_setup_bases_device -> the n * 64 bytes of points [first, first + n)"""
    ptr = lib.alloc(max(n, 1) * 64)
    try:
        lib.check(lib.c.mira_setup_bases_device(curve, label, len(label), first, n, ctypes.c_void_p(ptr)))
        return lib.download(ptr, (n * 64,), np.uint8).tobytes()
    finally:
        lib.free(ptr)


def hash_to_field(lib, curve, msgs):
    """mira_hash_to_field_device -> [(u0, u1)] as plain integers; the library's elements must be canonical"""
    p = R.CURVES[curve][0]
    n = len(msgs)
    d_m, d_u = lib.alloc(n * 32), lib.alloc(n * 64)
    try:
        lib.upload(d_m, np.frombuffer(b"".join(msgs), dtype=np.uint8))
        lib.check(lib.c.mira_hash_to_field_device(curve, ctypes.c_void_p(d_m), n, ctypes.c_void_p(d_u)))
        raw = lib.download(d_u, (n * 64,), np.uint8).tobytes()
    finally:
        lib.free(d_m)
        lib.free(d_u)
    vals = [int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(2 * n)]
    assert all(v < p for v in vals), "an element left hash_to_field unreduced"
    rinv = pow(R.R256, p - 2, p)
    return [(vals[2 * i] * rinv % p, vals[2 * i + 1] * rinv % p) for i in range(n)]


def map_to_curve(lib, curve, pairs, in_place=False):
    """mira_map_to_curve_device on pairs of plain integers -> the n * 64 bytes of points"""
    n = len(pairs)
    d_u = lib.alloc(n * 64)
    d_p = d_u if in_place else lib.alloc(n * 64)
    try:
        lib.upload(d_u, np.frombuffer(b"".join(R.fe_bytes(u0, curve) + R.fe_bytes(u1, curve) for u0, u1 in pairs), dtype=np.uint8))
        lib.check(lib.c.mira_map_to_curve_device(curve, ctypes.c_void_p(d_u), n, ctypes.c_void_p(d_p)))
        return lib.download(d_p, (n * 64,), np.uint8).tobytes()
    finally:
        lib.free(d_u)
        if not in_place:
            lib.free(d_p)


def points_of(raw, curve):
    """reference-layout bytes -> plain affine pairs (None = identity, 64 zero bytes)"""
    p = R.CURVES[curve][0]
    rinv = pow(R.R256, p - 2, p)
    out = []
    for i in range(len(raw) // 64):
        blob = raw[64 * i:64 * i + 64]
        x, y = int.from_bytes(blob[:32], "little"), int.from_bytes(blob[32:], "little")
        assert x < p and y < p
        out.append(None if blob == bytes(64) else (x * rinv % p, y * rinv % p))
    return out


def first_diff(got, want):
    if got == want:
        return None
    i = next(j for j in range(min(len(got), len(want)) // 64 + 1) if got[64 * j:64 * j + 64] != want[64 * j:64 * j + 64])
    return "point %d: got %s want %s" % (i, got[64 * i:64 * i + 64].hex(), want[64 * i:64 * i + 64].hex())


# ---- the cases -----------------------------------------------------------------------------------------------------------------
def check_key(lib, curve, k, label, chunk):
    """item 4 / 5: the whole key equals the restatement, whatever the chunk length"""
    set_chunk(lib, chunk)
    try:
        got = setup_bytes(lib, curve, label, 0, 1 << k)
    finally:
        set_chunk(lib, -1)
    assert first_diff(got, R.key_bytes(curve, k, label)) is None, first_diff(got, R.key_bytes(curve, k, label))
    assert all(R.on_curve(P, curve) for P in points_of(got, curve))


def check_range(lib, curve, k, label, chunk, first=5, n=37):
    """item 6: a range equals the slice of the whole"""
    set_chunk(lib, chunk)
    try:
        got = setup_bytes(lib, curve, label, first, n)
    finally:
        set_chunk(lib, -1)
    want = R.key_bytes(curve, k, label)[64 * first:64 * (first + n)]
    assert first_diff(got, want) is None, first_diff(got, want)


def check_hash_to_field(lib, curve, n):
    """item 7: n messages, the all-zero and the all-ones one among them"""
    rng = random.Random(0x5E70 + curve)
    msgs = [bytes(32), b"\xff" * 32] + [rng.randbytes(32) for _ in range(n - 2)]
    got = hash_to_field(lib, curve, msgs)
    want = [R.hash_to_field(m, curve) for m in msgs]
    assert got == want, next((i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w)


def chosen_pairs(curve):
    """item 8: the map's exceptional inputs, the doubling case, opposite pairs; returns (pairs, indices of the (u, -u) pairs)"""
    p = R.CURVES[curve][0]
    _, c1, _, _, _ = R.svdw_constants(curve)
    specials = [0, 1, p - 1]
    for rhs in (1, p - 1):                                   # c1 u^2 = 1 (tv1 = 0) and c1 u^2 = -1 (tv2 = 0): inv0(0)
        sq = rhs * R.inv0(c1, p) % p
        if R.is_square(sq, p):
            root = R.sqrt_mod(sq, p)
            assert c1 * root * root % p == rhs
            specials += [root, p - root]
    if curve == 0:
        assert (p + 1) // 2 in specials and (p - 1) // 2 in specials          # +-1/2
    rng = random.Random(0xC0FFEE + curve)
    others = [rng.randrange(p) for _ in range(12)]
    pairs = [(s, 7) for s in specials] + [(7, s) for s in specials]
    pairs += [(u, u) for u in specials + others[:4]]
    opposite_at = len(pairs)
    pairs += [(u, (p - u) % p) for u in specials + others]
    return pairs, range(opposite_at, len(pairs))


def check_map_chosen(lib, curve):
    pairs, opposite = chosen_pairs(curve)
    want_pts = [R.map_pair(u0, u1, curve)[0] for u0, u1 in pairs]
    ident = [i for i in opposite if want_pts[i] is None]
    assert ident and len(ident) < len(opposite), "the (u, -u) pairs must hold an identity and a point"
    want = b"".join(R.point_bytes(P, curve) for P in want_pts)
    got = map_to_curve(lib, curve, pairs)
    assert first_diff(got, want) is None, first_diff(got, want)
    assert all(got[64 * i:64 * i + 64] == bytes(64) for i in ident)
    assert map_to_curve(lib, curve, pairs, in_place=True) == want


def check_map_random(lib, curve, n=200):
    p = R.CURVES[curve][0]
    rng = random.Random(0xA11CE + curve)
    pairs = [(rng.randrange(p), rng.randrange(p)) for _ in range(n)]
    mapped = [R.map_pair(u0, u1, curve) for u0, u1 in pairs]
    branches = [b for _, br in mapped for b in br]
    assert {1, 2, 3} == set(branches), "the random pairs must take all three branches"
    want = b"".join(R.point_bytes(P, curve) for P, _ in mapped)
    got = map_to_curve(lib, curve, pairs)
    assert first_diff(got, want) is None, first_diff(got, want)


def check_k32_refused(lib):
    h = ctypes.c_uint64()
    for curve in CURVES:
        assert lib.c.mira_msm_setup_bases(curve, 32, b"x", 1, ctypes.byref(h)) == _lib.MIRA_E_BAD_ARG


def sha256(raw):
    return hashlib.sha256(raw).hexdigest()
