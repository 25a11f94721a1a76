// CommitmentKey::setup (src/commitment.rs:52-76): one base per 32 bytes of the label's SHAKE256 stream, by hash-to-curve.
//
//   msg_i  --k_setup_hash-->  (u_0, u_1)  --k_setup_map-->  P_i = map(u_0) + map(u_1)
//
// hash_to_field is expand_message_xmd over BLAKE2b-512 (four compressions per message) with both 512-bit outputs reduced
// mod p; the map is Shallue-van de Woestijne (RFC 9380 appendix F.1) with Z = 1 on both curves.  The derivation is this
// project's own statement of `setup` (tests/setup_ref.py restates it in plain Python); halo2curves, whose hashing the
// reference calls, is in neither tree, so the keys are unpinned against it.
//
// One lane per point in both kernels.  The two stay separate: the hash is 64-bit word shuffling (some 9 000 32-bit
// instructions, no multiplier), the map some 3 000 - 5 000 dependent field multiplications with a dozen live field
// elements; fused, the map's registers would bound the hash's occupancy too.  (u_0, u_1) cross between them in the
// reference's layout (64 B per point, in the very slot the point is written to afterwards).
// The final 1 / ZZZ is a per-lane power (f29_inv, as k_table_step): a tenth of the map's work, and a batch inversion
// would need a second sweep over the points with its own workspace.
#pragma once
#include "table_kernels.cuh"

// ---- BLAKE2b on pairs of 32-bit words ----------------------------------------------------------------------------------
// gfx950 has no 64-bit vector rotate or xor: every 64-bit word is kept as two VGPRs.  The rotations by 32, 24 and 16 are
// then word swaps and v_alignbit_b32 pairs, the one by 63 a funnel shift by one, and only the additions carry.
struct W64 {
    uint32_t lo, hi;
};
HD W64 w64_add(const W64 &a, const W64 &b) {
    const uint64_t s = (((uint64_t)a.hi << 32) | a.lo) + (((uint64_t)b.hi << 32) | b.lo);
    return W64{(uint32_t)s, (uint32_t)(s >> 32)};
}
HD W64 w64_xor(const W64 &a, const W64 &b) { return W64{a.lo ^ b.lo, a.hi ^ b.hi}; }
HD W64 w64_ror32(const W64 &a) { return W64{a.hi, a.lo}; }
HD W64 w64_ror24(const W64 &a) { return W64{(a.lo >> 24) | (a.hi << 8), (a.hi >> 24) | (a.lo << 8)}; }
HD W64 w64_ror16(const W64 &a) { return W64{(a.lo >> 16) | (a.hi << 16), (a.hi >> 16) | (a.lo << 16)}; }
HD W64 w64_ror63(const W64 &a) { return W64{(a.lo << 1) | (a.hi >> 31), (a.hi << 1) | (a.lo >> 31)}; }

struct Blake2b {
    static constexpr uint32_t IV[8][2] = {{0xf3bcc908u, 0x6a09e667u}, {0x84caa73bu, 0xbb67ae85u}, {0xfe94f82bu, 0x3c6ef372u}, {0x5f1d36f1u, 0xa54ff53au},
                                          {0xade682d1u, 0x510e527fu}, {0x2b3e6c1fu, 0x9b05688cu}, {0xfb41bd6bu, 0x1f83d9abu}, {0x137e2179u, 0x5be0cd19u}};
    static constexpr uint8_t SIGMA[10][16] = {
        {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
        {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4}, {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
        {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13}, {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
        {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11}, {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
        {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5}, {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0}};
    static constexpr uint32_t PARAM0 = 0x01010040u;   // digest length 64, no key, fanout 1, depth 1; salt and personalisation zero
};
HD void blake2b_g(W64 &a, W64 &b, W64 &c, W64 &d, const W64 &x, const W64 &y) {
    a = w64_add(w64_add(a, b), x);
    d = w64_ror32(w64_xor(d, a));
    c = w64_add(c, d);
    b = w64_ror24(w64_xor(b, c));
    a = w64_add(w64_add(a, b), y);
    d = w64_ror16(w64_xor(d, a));
    c = w64_add(c, d);
    b = w64_ror63(w64_xor(b, c));
}
HD void blake2b_init(W64 h[8]) {
#pragma unroll
    for (int i = 0; i < 8; i++) h[i] = W64{Blake2b::IV[i][0], Blake2b::IV[i][1]};
    h[0].lo ^= Blake2b::PARAM0;
}
// One compression: `t` bytes hashed so far including this block (every message here is shorter than 2^32 bytes).  The
// rounds are fully unrolled so that the schedule's indices are constants and m stays in registers.
HD void blake2b_compress(W64 h[8], const W64 m[16], uint32_t t, bool last) {
    W64 v[16];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        v[i] = h[i];
        v[8 + i] = W64{Blake2b::IV[i][0], Blake2b::IV[i][1]};
    }
    v[12].lo ^= t;
    if (last) { v[14].lo = ~v[14].lo; v[14].hi = ~v[14].hi; }
#pragma unroll
    for (int r = 0; r < 12; r++) {
        const int s = r % 10;
        blake2b_g(v[0], v[4], v[8], v[12], m[Blake2b::SIGMA[s][0]], m[Blake2b::SIGMA[s][1]]);
        blake2b_g(v[1], v[5], v[9], v[13], m[Blake2b::SIGMA[s][2]], m[Blake2b::SIGMA[s][3]]);
        blake2b_g(v[2], v[6], v[10], v[14], m[Blake2b::SIGMA[s][4]], m[Blake2b::SIGMA[s][5]]);
        blake2b_g(v[3], v[7], v[11], v[15], m[Blake2b::SIGMA[s][6]], m[Blake2b::SIGMA[s][7]]);
        blake2b_g(v[0], v[5], v[10], v[15], m[Blake2b::SIGMA[s][8]], m[Blake2b::SIGMA[s][9]]);
        blake2b_g(v[1], v[6], v[11], v[12], m[Blake2b::SIGMA[s][10]], m[Blake2b::SIGMA[s][11]]);
        blake2b_g(v[2], v[7], v[8], v[13], m[Blake2b::SIGMA[s][12]], m[Blake2b::SIGMA[s][13]]);
        blake2b_g(v[3], v[4], v[9], v[14], m[Blake2b::SIGMA[s][14]], m[Blake2b::SIGMA[s][15]]);
    }
#pragma unroll
    for (int i = 0; i < 8; i++) h[i] = w64_xor(h[i], w64_xor(v[i], v[8 + i]));
}

// ---- per-field constants ---------------------------------------------------------------------------------------------------
// C522, C778: 2^522 and 2^778 mod P (plain integers, 29-bit limbs) -- what the two halves of a 512-bit value are
// Montgomery-multiplied by to land in the resident form x * 2^261.
// B, C1 .. C4: the curve constant and the SvdW constants of RFC 9380 F.1 for Z = 1 (c1 = g(Z), c2 = -Z / 2,
// c3 = sqrt(-g(Z) (3 Z^2 + 4 A)) with sgn0 = 0, c4 = -4 g(Z) / (3 Z^2 + 4 A)), canonical, times 2^261.
// EXP: the exponent of the square root -- (P + 1) / 4 for Fq (P = 3 mod 4); (t - 1) / 2 for Fr, P - 1 = 2^28 t.
// ROOT (Fr): 5^t, a generator of the subgroup of order 2^28, times 2^261.
template <class F> struct SetupConsts;
template <> struct SetupConsts<Fq29> {
    static constexpr uint32_t C522[9] = {0x059bac10u, 0x0d1503a3u, 0x018016b8u, 0x10ab0ca8u, 0x02632639u, 0x02c0169fu, 0x169bfd53u, 0x11869d4cu, 0x002a11a6u};
    static constexpr uint32_t C778[9] = {0x0ff8e86au, 0x07c648f0u, 0x0d256c51u, 0x0e144bb5u, 0x0fe5cb16u, 0x0e4726c0u, 0x07f5c538u, 0x0f6c68ccu, 0x00043c5bu};
    static constexpr uint32_t B[9] = {0x00766463u, 0x1c54760au, 0x08f6927au, 0x03e40c4du, 0x1fea4f2bu, 0x17c6c26au, 0x157fe417u, 0x0f8056f9u, 0x002958a2u};
    static constexpr uint32_t C1[9] = {0x1d76333du, 0x0f6c3cabu, 0x04d61fffu, 0x025aed96u, 0x1507e56cu, 0x122dc278u, 0x06ae4edeu, 0x064ef86eu, 0x0006bc8au};
    static constexpr uint32_t C2[9] = {0x01801893u, 0x16741cafu, 0x1210393du, 0x10c48f5bu, 0x057134dfu, 0x12cc7ff9u, 0x1768ca9cu, 0x0498af45u, 0x00114e0cu};
    static constexpr uint32_t C3[9] = {0x1b4a814fu, 0x1d686287u, 0x16a42cbau, 0x0bac1e79u, 0x013fb16cu, 0x1d850693u, 0x1eba05b6u, 0x0c9dae1eu, 0x001b5818u};
    static constexpr uint32_t C4[9] = {0x068a0e4bu, 0x171eba7cu, 0x0b55234fu, 0x150690b3u, 0x0ed0a792u, 0x1ff392cau, 0x026922c2u, 0x109d85a1u, 0x002768ebu};
    static constexpr uint32_t EXP[9] = {0x161f3f52u, 0x1841182du, 0x071ca8d3u, 0x00b548b4u, 0x0561765eu, 0x08b6d030u, 0x0029b850u, 0x1397098du, 0x000c1913u};
    static constexpr int EXP_BITS = 252;
    static constexpr int TWO_ADICITY = 1;
    static constexpr uint32_t ROOT[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};   // unused: the square root is one power
};
template <> struct SetupConsts<Fr29> {
    static constexpr uint32_t C522[9] = {0x05b69bd4u, 0x06170a5au, 0x020cddceu, 0x1db6310bu, 0x0e54d0ffu, 0x1cf855e3u, 0x1c15e103u, 0x07d09161u, 0x000a054au};
    static constexpr uint32_t C778[9] = {0x1c00feeeu, 0x1c5573e0u, 0x18197feau, 0x08b5c34cu, 0x120f41aeu, 0x1a97f167u, 0x15f6b4bbu, 0x01454f10u, 0x00160937u};
    static constexpr uint32_t B[9] = {0x00000b3eu, 0x1236a921u, 0x0fe04649u, 0x1abd90e5u, 0x16749f78u, 0x1ce1f60fu, 0x141859beu, 0x0ff57cd2u, 0x0007a9efu};
    static constexpr uint32_t C1[9] = {0x10000a95u, 0x10ddb3d5u, 0x150c4cd5u, 0x120de02eu, 0x011ca6d4u, 0x1a2436deu, 0x05eda5c6u, 0x1520447bu, 0x00157225u};
    static constexpr uint32_t C2[9] = {0x10000055u, 0x103450f5u, 0x04980ee2u, 0x184020d5u, 0x056ee593u, 0x12cc7ff9u, 0x1768ca9cu, 0x0498af45u, 0x00114e0cu};
    static constexpr uint32_t C3[9] = {0x038a7f71u, 0x152f5622u, 0x0f680d3eu, 0x0f158a02u, 0x0130a9f9u, 0x082586a4u, 0x155f27dau, 0x0adf3609u, 0x00064be2u};
    static constexpr uint32_t C4[9] = {0x0aaa9c90u, 0x0842a10du, 0x17151f4fu, 0x1d03965bu, 0x1b36e4e8u, 0x0b9eb7d8u, 0x18f6f9f8u, 0x16fa824bu, 0x0023ed8bu};
    static constexpr uint32_t EXP[9] = {0x1f0fac9fu, 0x0e5c2450u, 0x07d090f3u, 0x1585d283u, 0x02db40c0u, 0x00a6e141u, 0x0e5c2634u, 0x0030644eu, 0x00000000u};
    static constexpr int EXP_BITS = 225;
    static constexpr int TWO_ADICITY = 28;
    static constexpr uint32_t ROOT[9] = {0x1a27b370u, 0x1d788b88u, 0x0a3c6e0bu, 0x1fd3f9dau, 0x0f541c23u, 0x1e4ddf15u, 0x093d0e83u, 0x0ae32ca7u, 0x0005d90bu};
};
template <class F> HD Fe29<F> setup_const(const uint32_t (&c)[9]) {
    Fe29<F> r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.l[i] = c[i];
    F29_SET(r, 1.0);
    return r;
}

// ---- 512 bits -> field ---------------------------------------------------------------------------------------------------------
// Any 512-bit integer w (16 little-endian 32-bit words) mod P, in the resident form: w = hi 2^256 + lo, and
// f29_mul2_add(hi, 2^778, lo, 2^522) = (hi 2^517 + lo 2^261) mod P with one reduction.  Both halves are arbitrary 256-bit
// values (either may be >= P): unpacked they are < 6 P with every limb below 2^29, and 6 + 6 <= 168.  Result loose, < 2 P.
template <class F> HD Fe29<F> setup_reduce512(const uint32_t w[16]) {
    using S = typename F::Sat;
    Fe<S> lo, hi;
#pragma unroll
    for (int i = 0; i < 8; i++) { lo.l[i] = w[i]; hi.l[i] = w[8 + i]; }
    return f29_mul2_add(f29_unpack<F>(hi), setup_const<F>(SetupConsts<F>::C778), f29_unpack<F>(lo), setup_const<F>(SetupConsts<F>::C522));
}

// The tails of the message blocks, which depend on the curve's domain-separation tag only (setup.hip builds them):
// b_0's second block is msg || 00 80 00 || DST, b_1's and b_2's block is a digest || counter byte || DST.
struct SetupHashConsts {
    uint32_t tail0[24];   // bytes 32 .. 127 of b_0's second block
    uint32_t tail1[16];   // bytes 64 .. 127 of b_1's block with the counter byte left zero
    uint32_t len0, len1;  // lengths of the two messages: 163 + |DST|, 65 + |DST|
};

// a digest as the big-endian 512-bit integer of its 64 bytes, least significant word first
HD void setup_digest_words(const W64 h[8], uint32_t w[16]) {
#pragma unroll
    for (int j = 0; j < 8; j++) {
        w[15 - 2 * j] = __builtin_bswap32(h[j].lo);
        w[14 - 2 * j] = __builtin_bswap32(h[j].hi);
    }
}

// msgs: n x 32 B (16-byte aligned); u: n x 2 field elements in the reference layout (x * 2^256, canonical)
template <class F>
KERNEL void __launch_bounds__(64) k_setup_hash(const unsigned char *__restrict__ msgs, uint64_t n, SetupHashConsts kc, unsigned char *__restrict__ u) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const U4 *mp = reinterpret_cast<const U4 *>(msgs + i * 32);
    const U4 ma = mp[0], mb = mp[1];
    W64 h[8], m[16], b0[8];
    // b_0 = H(0^128 || msg || 00 80 00 || DST)
    blake2b_init(h);
#pragma unroll
    for (int j = 0; j < 16; j++) m[j] = W64{0, 0};
    blake2b_compress(h, m, 128, false);
    m[0] = W64{ma.x, ma.y}; m[1] = W64{ma.z, ma.w}; m[2] = W64{mb.x, mb.y}; m[3] = W64{mb.z, mb.w};
#pragma unroll
    for (int j = 0; j < 12; j++) m[4 + j] = W64{kc.tail0[2 * j], kc.tail0[2 * j + 1]};
    blake2b_compress(h, m, kc.len0, true);
#pragma unroll
    for (int j = 0; j < 8; j++) b0[j] = h[j];
    // b_1 = H(b_0 || 01 || DST)
#pragma unroll
    for (int j = 0; j < 8; j++) { m[j] = b0[j]; m[8 + j] = W64{kc.tail1[2 * j], kc.tail1[2 * j + 1]}; }
    m[8].lo |= 1u;
    blake2b_init(h);
    blake2b_compress(h, m, kc.len1, true);
    uint32_t w[16];
    setup_digest_words(h, w);
    const Fe29<F> u0 = setup_reduce512<F>(w);
    // b_2 = H((b_0 xor b_1) || 02 || DST)
#pragma unroll
    for (int j = 0; j < 8; j++) m[j] = w64_xor(b0[j], h[j]);
    m[8].lo ^= 3u;
    blake2b_init(h);
    blake2b_compress(h, m, kc.len1, true);
    setup_digest_words(h, w);
    const Fe29<F> u1 = setup_reduce512<F>(w);
    fe_store(u + i * 64, f29_to_r256(u0));
    fe_store(u + i * 64 + 32, f29_to_r256(u1));
}

// ---- the map --------------------------------------------------------------------------------------------------------------------
// sgn0: the parity of the canonical plain value (a * 2^-261, reduced below P)
template <class F> HD uint32_t setup_sgn0(const Fe29<F> &a) { return reduce_once(f29_pack(f29_redc(a))).l[0] & 1u; }

// a^EXP on loose values (any input bound <= 12), least significant bit first as f29_inv
template <class F> HD Fe29<F> setup_pow_exp(const Fe29<F> &a) {
    using K = SetupConsts<F>;
    Fe29<F> acc = f29_one<F>(), base = f29_mul(a, f29_one<F>());
#pragma unroll 1
    for (int i = 0; i < (K::EXP_BITS + 28) / 29; i++) {
        const uint32_t e = K::EXP[i];
        const int bits = K::EXP_BITS - 29 * i < 29 ? K::EXP_BITS - 29 * i : 29;
#pragma unroll 1
        for (int k = 0; k < bits; k++) {
            if ((e >> k) & 1) acc = f29_mul(acc, base);
            base = f29_sqr(base);
        }
    }
    return acc;
}
template <class F> HD bool setup_is_one(const Fe29<F> &b) { return f29_is_zero_mod_p<4>(f29_sub<2>(b, f29_one<F>())); }   // b a product: < 2 P

// is_square and sqrt share their power.  setup_sqrt_begin(g, z, t): is g a square?  For a square, setup_sqrt_finish(z, t)
// is a root of it.  g: bound <= 2.9 (x^3 + B, a product plus a constant), never zero mod P (neither curve has a point
// of order two).
//   Fq (P = 3 mod 4): z = g^((P + 1) / 4) is a root iff g is a square; one squaring tells.
//   Fr (P - 1 = 2^28 t): with w = g^((t - 1) / 2): z = g w = g^((t + 1) / 2), t = z w = g^t, and g is a square iff
//   t^(2^27) = 1.  The finish is the fixed-trip-count Tonelli-Shanks of RFC 9380 appendix I.4: 27 passes, pass i
//   squares t down i - 2 times to read one bit of its discrete logarithm and multiplies the correction in.
template <class F> HD bool setup_sqrt_begin(const Fe29<F> &gx, Fe29<F> &z, Fe29<F> &t) {
    if constexpr (SetupConsts<F>::TWO_ADICITY == 1) {
        z = setup_pow_exp<F>(gx);
        t = z;
        return f29_is_zero_mod_p<5>(f29_sub<3>(f29_sqr(z), gx));
    } else {
    const Fe29<F> w = setup_pow_exp<F>(gx);
    z = f29_mul(w, gx);
    t = f29_mul(z, w);
    Fe29<F> b = t;
#pragma unroll 1
    for (int j = 0; j < SetupConsts<F>::TWO_ADICITY - 1; j++) b = f29_sqr(b);
    return setup_is_one(b);
    }
}
template <class F> HD Fe29<F> setup_sqrt_finish(Fe29<F> z, Fe29<F> t) {
    if (SetupConsts<F>::TWO_ADICITY == 1) return z;
    Fe29<F> c = setup_const<F>(SetupConsts<F>::ROOT);
#pragma unroll 1
    for (int i = SetupConsts<F>::TWO_ADICITY; i >= 2; i--) {
        Fe29<F> b = t;
#pragma unroll 1
        for (int j = 1; j <= i - 2; j++) b = f29_sqr(b);
        const bool e = setup_is_one(b);
        if (!e) z = f29_mul(z, c);                                 // branches, not selects of both products: half the registers
        c = f29_sqr(c);
        if (!e) t = f29_mul(t, c);
    }
    return z;
}

// g(x) = x^3 + B for x with a bound <= 3: < 2.1 P
template <class F> HD Fe29<F> setup_g(const Fe29<F> &x) { return f29_add(f29_mul(f29_sqr(x), x), setup_const<F>(SetupConsts<F>::B)); }

// RFC 9380 F.1 with Z = 1, A = 0.  u: canonical, reference layout.  Returns a point of the curve (never the identity):
// x < 3.1 P, y < 2.1 P.  The three candidates for x cost four multiplications more than the first alone and are taken up
// front; what costs -- the power behind is_square -- runs once per candidate in a loop a lane leaves at its first
// square, so a wave pays for the second and third round only while one of its lanes needs them (half of all inputs
// stop at x1, a quarter at x2; g(x3) is a square whenever the other two are not).  One copy of the power's code serves
// all three rounds and both maps of a point: the kernel's registers are those of one round.
template <class F> HD Aff29<F> setup_map_to_curve(const Fe<typename F::Sat> &u_r256) {
    using K = SetupConsts<F>;
    const Fe29<F> one = f29_one<F>(), c2 = setup_const<F>(K::C2);
    Fe29<F> x1, x2, x3;
    uint32_t sgn_u;
    {
        const Fe29<F> u = f29_from_r256<F>(u_r256);
        sgn_u = setup_sgn0(u);
        Fe29<F> tv1 = f29_mul(f29_sqr(u), setup_const<F>(K::C1));
        const Fe29<F> tv2 = f29_add(one, tv1);                     // < 2.1
        tv1 = f29_sub<2>(one, tv1);                                // < 3
        const Fe29<F> tv3 = f29_inv(f29_mul(tv1, tv2));            // inv0: 0 -> 0
        const Fe29<F> tv4 = f29_mul(f29_mul(f29_mul(u, tv1), tv3), setup_const<F>(K::C3));
        x1 = f29_sub<2>(c2, tv4);                                  // < 3
        x2 = f29_add(c2, tv4);                                     // < 2.1
        x3 = f29_add(f29_mul(f29_sqr(f29_mul(f29_sqr(tv2), tv3)), setup_const<F>(K::C4)), one);   // < 2.1
    }
    Aff29<F> r;
    Fe29<F> z, t;
    r.x = x1;
#pragma unroll 1
    for (int cand = 0; cand < 3; cand++) {
        if (setup_sqrt_begin<F>(setup_g<F>(r.x), z, t)) break;
        r.x = cand == 0 ? x2 : x3;
    }
    r.y = setup_sqrt_finish<F>(z, t);
    if (setup_sgn0(r.y) != sgn_u) r.y = f29_neg<2>(r.y);
    return r;
}

// u: n x 2 field elements (reference layout, canonical); out: n x 64 B, the points map(u_0) + map(u_1) in the reference
// layout (x * 2^256, y * 2^256) or, with resident != 0, in the engine's resident layout (x * 2^261, y * 2^261); the
// identity is 64 zero bytes in both.  out may be u itself: a lane reads its slot before it writes it.
template <class F>
KERNEL void __launch_bounds__(64) k_setup_map(const unsigned char *u, uint64_t n, unsigned char *out, uint32_t resident) {
    using S = typename F::Sat;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Fe<S> u0 = fe_load<S>(u + i * 64), u1 = fe_load<S>(u + i * 64 + 32);
    Aff29<F> q0, q1;
#pragma unroll 1
    for (int j = 0; j < 2; j++) {                                  // one copy of the map's code
        q1 = setup_map_to_curve<F>(j ? u1 : u0);
        if (j == 0) q0 = q1;
    }
    Xyzz29<F> acc;
    acc.x = q0.x; acc.y = q0.y; acc.zz = f29_one<F>(); acc.zzz = f29_one<F>();
    xyzz29_add_affine(acc, q1);                                    // the full law: q1 = q0 doubles, q1 = -q0 gives the identity
    Fe<S> x = fe_zero<S>(), y = fe_zero<S>();
    if (!xyzz29_is_identity(acc)) {
        const Fe29<F> zi = f29_inv(acc.zzz);                       // 1 / ZZZ
        const Fe29<F> zzi = f29_sqr(f29_mul(zi, acc.zz));          // (ZZ / ZZZ)^2 = 1 / ZZ
        const Fe29<F> xa = f29_mul(acc.x, zzi), ya = f29_mul(acc.y, zi);
        if (resident) { x = reduce_once(f29_pack(xa)); y = reduce_once(f29_pack(ya)); }
        else { x = f29_to_r256(xa); y = f29_to_r256(ya); }
    }
    fe_store(out + i * 64, x);
    fe_store(out + i * 64 + 32, y);
}
