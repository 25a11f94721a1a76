"""Plain-Python restatement of `CommitmentKey::setup(k, label)` (src/commitment.rs:52-76) as this project defines it: the
SHAKE256 stream of the label cut into 32-byte messages, hash_to_field by expand_message_xmd over BLAKE2b-512, the
Shallue-van de Woestijne map of RFC 9380 appendix F.1 for both field elements, and the sum of the two points.  It uses
hashlib and integers only and shares no code with the library; tests compare the library against it byte for byte.

Parity: equal to this restatement and to the checksums below, unpinned against halo2curves (which is in neither tree).
"""
import hashlib

FQ = 0x30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47   # bn256 base field
FR = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001   # bn256 scalar field = Grumpkin base field
R256 = 1 << 256

# curve id -> (base field modulus, A, B, curve_id string)
CURVES = {0: (FQ, 0, 3, b"bn256_g1"), 1: (FR, 0, FR - 17, b"grumpkin_g1")}

# SHA-256 of the raw key bytes (the file save_to_file writes)
CHECKSUMS = {
    (0, 0, b""): "9fa8e2daadd3b88898a2df9f1e361791a81119d7b3cccd65e232c64b3a88a555",
    (0, 3, b"bn256"): "d5807c1f712b1a2a9a5a11e1324fc027227e71f695f4cd503ce92c9f26e9ca76",
    (0, 10, b"mira setup test"): "228aabb167cfba7193a893f5584a0e87aef1d23f145a90a1ba566d6ac1b5a83c",
    (1, 0, b""): "b4318687751ab746804dec493223ba3629b30f673d39c94432cb679737f5149a",
    (1, 3, b"bn256"): "979fa97cec3f6b206fbe9592a810f94b9646aca125b3db409e8f33e4c5638b04",
    (1, 10, b"mira setup test"): "4a665f77a82edc8bae45db838cc62ef13c1c57e955e7a345dd04fdb09c518c7c",
}
FIRST_POINT_BN256_EMPTY = (0x27474c0e125df68b3779a7f0727f9ea49a5756e05ca4b895cdfd26ab9d7934e,
                           0xfc6b2d47cf1d6bf585e1ced3478fe4530de96c3b1c1a53dbaee774474277fa2)


# ---- field helpers ------------------------------------------------------------------------------------------------------
def inv0(v, p):
    return pow(v, p - 2, p)


def is_square(v, p):
    return v % p == 0 or pow(v, (p - 1) // 2, p) == 1


def sgn0(v, p):
    return (v % p) & 1


def sqrt_mod(a, p):
    """A square root of a mod p (a must be a square): the exponent for p = 3 mod 4, Tonelli-Shanks otherwise."""
    a %= p
    if a == 0:
        return 0
    if p % 4 == 3:
        return pow(a, (p + 1) // 4, p)
    q, s = p - 1, 0
    while q % 2 == 0:
        q //= 2
        s += 1
    z = 2
    while is_square(z, p):
        z += 1
    m, c, t, r = s, pow(z, q, p), pow(a, q, p), pow(a, (q + 1) // 2, p)
    while t != 1:
        i, t2 = 0, t
        while t2 != 1:
            t2 = t2 * t2 % p
            i += 1
        b = pow(c, 1 << (m - i - 1), p)
        m, c = i, b * b % p
        t, r = t * c % p, r * b % p
    return r


# ---- SvdW (RFC 9380 F.1) -------------------------------------------------------------------------------------------------
def g_of(x, curve):
    p, a, b, _ = CURVES[curve]
    return (x * x * x + a * x + b) % p


def find_z_svdw(curve):
    p, a, _, _ = CURVES[curve]

    def h(z):
        return (-(3 * z * z + 4 * a) * inv0(4 * g_of(z, curve), p)) % p
    ctr = 1
    while True:
        for z in (ctr % p, (-ctr) % p):
            gz = g_of(z, curve)
            if gz == 0:
                continue
            hz = h(z)
            if hz == 0 or not is_square(hz, p):
                continue
            if is_square(gz, p) or is_square(g_of((-z * inv0(2, p)) % p, curve), p):
                return z
        ctr += 1


def svdw_constants(curve):
    """(Z, c1, c2, c3, c4)"""
    p, a, _, _ = CURVES[curve]
    z = find_z_svdw(curve)
    gz = g_of(z, curve)
    t = (3 * z * z + 4 * a) % p
    c1 = gz
    c2 = (-z * inv0(2, p)) % p
    c3 = sqrt_mod((-gz * t) % p, p)
    if sgn0(c3, p) == 1:
        c3 = p - c3
    c4 = (-4 * gz * inv0(t, p)) % p
    return z, c1, c2, c3, c4


_CONSTS = {}


def map_to_curve(u, curve):
    """SvdW map: ((x, y), branch) with branch 1, 2 or 3 for x1, x2, x3."""
    p = CURVES[curve][0]
    if curve not in _CONSTS:
        _CONSTS[curve] = svdw_constants(curve)
    z, c1, c2, c3, c4 = _CONSTS[curve]
    u %= p
    tv1 = u * u % p * c1 % p
    tv2 = (1 + tv1) % p
    tv1 = (1 - tv1) % p
    tv3 = inv0(tv1 * tv2 % p, p)
    tv4 = u * tv1 % p * tv3 % p * c3 % p
    x1 = (c2 - tv4) % p
    e1 = is_square(g_of(x1, curve), p)
    x2 = (c2 + tv4) % p
    e2 = is_square(g_of(x2, curve), p) and not e1
    x3 = (pow(tv2 * tv2 % p * tv3 % p, 2, p) * c4 + z) % p
    x, branch = (x1, 1) if e1 else (x2, 2) if e2 else (x3, 3)
    y = sqrt_mod(g_of(x, curve), p)
    assert y * y % p == g_of(x, curve)
    if sgn0(y, p) != sgn0(u, p):
        y = (p - y) % p
    return (x, y), branch


# ---- affine group law; None = identity -----------------------------------------------------------------------------------
def point_add(P, Q, curve):
    p, a, _, _ = CURVES[curve]
    if P is None:
        return Q
    if Q is None:
        return P
    (x1, y1), (x2, y2) = P, Q
    if x1 == x2:
        if (y1 + y2) % p == 0:
            return None
        lam = (3 * x1 * x1 + a) * inv0(2 * y1, p) % p
    else:
        lam = (y2 - y1) * inv0(x2 - x1, p) % p
    x3 = (lam * lam - x1 - x2) % p
    return x3, (lam * (x1 - x3) - y1) % p


def on_curve(P, curve):
    p = CURVES[curve][0]
    return P is None or P[1] * P[1] % p == g_of(P[0], curve)


# ---- hash_to_field ---------------------------------------------------------------------------------------------------------
def dst_of(curve):
    body = b"from_uniform_bytes" + b"-" + CURVES[curve][3] + b"_XMD:BLAKE2b_" + b"SVDW" + b"_RO_"
    return body + bytes([len(body)])


def hash_to_field(msg, curve):
    """(u0, u1) of one 32-byte message."""
    p = CURVES[curve][0]
    dst = dst_of(curve)

    def H(data):
        return hashlib.blake2b(data, digest_size=64).digest()
    b0 = H(bytes(128) + msg + b"\x00\x80\x00" + dst)
    b1 = H(b0 + b"\x01" + dst)
    b2 = H(bytes(x ^ y for x, y in zip(b0, b1)) + b"\x02" + dst)
    return int.from_bytes(b1, "big") % p, int.from_bytes(b2, "big") % p


def map_pair(u0, u1, curve):
    """The point of a pair of field elements (None = identity) and the branches its two maps took."""
    q0, br0 = map_to_curve(u0, curve)
    q1, br1 = map_to_curve(u1, curve)
    return point_add(q0, q1, curve), (br0, br1)


# ---- the key -----------------------------------------------------------------------------------------------------------------
def messages(label, first, n):
    stream = hashlib.shake_256(label).digest(32 * (first + n))
    return [stream[32 * i:32 * i + 32] for i in range(first, first + n)]


def setup_points(curve, label, first, n):
    """Points [first, first + n) of the key of `label` as plain affine pairs (None = identity)."""
    return [map_pair(*hash_to_field(m, curve), curve)[0] for m in messages(label, first, n)]


def fe_bytes(v, curve):
    """One field element in the reference layout: 4 x u64 little-endian, Montgomery R = 2^256."""
    return (v * R256 % CURVES[curve][0]).to_bytes(32, "little")


def point_bytes(P, curve):
    return bytes(64) if P is None else fe_bytes(P[0], curve) + fe_bytes(P[1], curve)


def setup_bytes(curve, label, first, n):
    return b"".join(point_bytes(P, curve) for P in setup_points(curve, label, first, n))


_KEYS = {}


def key_bytes(curve, k, label):
    """The whole key of 2^k points (computed once per process and shared)."""
    if (curve, k, label) not in _KEYS:
        _KEYS[(curve, k, label)] = setup_bytes(curve, label, 0, 1 << k)
    return _KEYS[(curve, k, label)]
