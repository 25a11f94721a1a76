// Host side of CommitmentKey::setup (src/commitment.rs:52-76; kernels: setup_kernels.cuh).
//
// The label's SHAKE256 stream is one serial sponge, so it is squeezed on the CPU -- chunk by chunk into two pinned
// buffers, each uploaded on the copy stream while the kernels of the chunk before run on the work stream (the pattern of
// load_bases_file, msm_host.cuh).  Point i takes bytes [32 i, 32 i + 32) of the stream: a range [first, first + n) skips
// 32 first bytes and is the same slice of the whole key.
#include <chrono>

#include "ctx.h"
#include "setup_kernels.cuh"

namespace {

// ---- Keccak-f[1600] / SHAKE256 (FIPS 202) ---------------------------------------------------------------------------------
inline uint64_t rotl64(uint64_t x, int n) { return (x << n) | (x >> (64 - n)); }
void keccak_f1600(uint64_t s[25]) {
    static const uint64_t RC[24] = {0x0000000000000001ULL, 0x0000000000008082ULL, 0x800000000000808aULL, 0x8000000080008000ULL, 0x000000000000808bULL, 0x0000000080000001ULL,
                                    0x8000000080008081ULL, 0x8000000000008009ULL, 0x000000000000008aULL, 0x0000000000000088ULL, 0x0000000080008009ULL, 0x000000008000000aULL,
                                    0x000000008000808bULL, 0x800000000000008bULL, 0x8000000000008089ULL, 0x8000000000008003ULL, 0x8000000000008002ULL, 0x8000000000000080ULL,
                                    0x000000000000800aULL, 0x800000008000000aULL, 0x8000000080008081ULL, 0x8000000000008080ULL, 0x0000000080000001ULL, 0x8000000080008008ULL};
    static const int RHO[24] = {1, 3, 6, 10, 15, 21, 28, 36, 45, 55, 2, 14, 27, 41, 56, 8, 25, 43, 62, 18, 39, 61, 20, 44};
    static const int PI[24] = {10, 7, 11, 17, 18, 3, 5, 16, 8, 21, 24, 4, 15, 23, 19, 13, 12, 2, 20, 14, 22, 9, 6, 1};
    for (int round = 0; round < 24; round++) {
        uint64_t c[5];
        for (int x = 0; x < 5; x++) c[x] = s[x] ^ s[x + 5] ^ s[x + 10] ^ s[x + 15] ^ s[x + 20];
        for (int x = 0; x < 5; x++) {
            const uint64_t d = c[(x + 4) % 5] ^ rotl64(c[(x + 1) % 5], 1);
            for (int y = 0; y < 25; y += 5) s[y + x] ^= d;
        }
        uint64_t cur = s[1];
        for (int i = 0; i < 24; i++) {
            const int j = PI[i];
            const uint64_t next = s[j];
            s[j] = rotl64(cur, RHO[i]);
            cur = next;
        }
        for (int y = 0; y < 25; y += 5) {
            uint64_t row[5];
            for (int x = 0; x < 5; x++) row[x] = s[y + x];
            for (int x = 0; x < 5; x++) s[y + x] = row[x] ^ (~row[(x + 1) % 5] & row[(x + 2) % 5]);
        }
        s[0] ^= RC[round];
    }
}
// The XOF of one label (little-endian host, as everything that reads the reference's buffers here)
struct Shake256 {
    static constexpr size_t RATE = 136;
    uint64_t s[25];
    size_t pos = 0;   // bytes of the current block already handed out
    Shake256(const unsigned char *label, size_t len) {
        memset(s, 0, sizeof s);
        unsigned char *b = reinterpret_cast<unsigned char *>(s);
        size_t at = 0;
        for (size_t i = 0; i < len; i++) {
            b[at++] ^= label[i];
            if (at == RATE) { keccak_f1600(s); at = 0; }
        }
        b[at] ^= 0x1F;
        b[RATE - 1] ^= 0x80;
        keccak_f1600(s);
    }
    void squeeze(unsigned char *out, size_t n) {
        const unsigned char *b = reinterpret_cast<const unsigned char *>(s);
        while (n) {
            if (pos == RATE) { keccak_f1600(s); pos = 0; }
            const size_t take = std::min(n, RATE - pos);
            memcpy(out, b + pos, take);
            out += take; pos += take; n -= take;
        }
    }
    void skip(uint64_t n) {
        while (n) {
            if (pos == RATE) { keccak_f1600(s); pos = 0; }
            const uint64_t take = std::min<uint64_t>(n, RATE - pos);
            pos += (size_t)take; n -= take;
        }
    }
};

// DST = "from_uniform_bytes" || "-" || curve_id || "_XMD:BLAKE2b_" || "SVDW" || "_RO_" || byte(length of all that)
SetupHashConsts hash_consts(int curve) {
    std::string dst = std::string("from_uniform_bytes") + "-" + (curve == MIRA_CURVE_BN256 ? "bn256_g1" : "grumpkin_g1") + "_XMD:BLAKE2b_" + "SVDW" + "_RO_";
    dst.push_back((char)dst.size());
    SetupHashConsts kc;
    unsigned char t0[96] = {0}, t1[64] = {0};
    t0[0] = 0x00; t0[1] = 0x80; t0[2] = 0x00;                     // l_i_b_str: 128 bytes out, then the counter 0
    memcpy(t0 + 3, dst.data(), dst.size());                       // |DST| <= 52: fits both tails
    memcpy(t1 + 1, dst.data(), dst.size());
    memcpy(kc.tail0, t0, sizeof t0);
    memcpy(kc.tail1, t1, sizeof t1);
    kc.len0 = (uint32_t)(128 + 32 + 3 + dst.size());
    kc.len1 = (uint32_t)(64 + 1 + dst.size());
    return kc;
}

constexpr size_t SETUP_CHUNK_DEFAULT = (size_t)1 << 18;           // points per chunk: 8 MiB of stream, some 13 ms of squeeze
constexpr uint32_t SETUP_BLOCK = 64;

template <class F> void launch_hash(int curve, const void *d_msgs, size_t n, void *d_u, hipStream_t st) {
    LAUNCH(k_setup_hash<F>, ceil_div(n, SETUP_BLOCK), SETUP_BLOCK, 0, st, reinterpret_cast<const unsigned char *>(d_msgs), (uint64_t)n, hash_consts(curve),
           reinterpret_cast<unsigned char *>(d_u));
}
template <class F> void launch_map(const void *d_u, size_t n, void *d_points, bool resident, hipStream_t st) {
    LAUNCH(k_setup_map<F>, ceil_div(n, SETUP_BLOCK), SETUP_BLOCK, 0, st, reinterpret_cast<const unsigned char *>(d_u), (uint64_t)n,
           reinterpret_cast<unsigned char *>(d_points), resident ? 1u : 0u);
}

// the per-chunk marks of one run folded into three entries: the host's squeeze, and each kernel over all chunks (a
// chunk's "hash" interval includes its wait for the upload; only the first 63 chunks fit the timers)
void fold_timings(double squeeze_ms) {
    if (!g.tm.enabled) return;
    float hash = 0.f, map = 0.f;
    for (size_t i = 0; i < g.tm.names.size() && i < g.tm.ms.size(); i++) (strcmp(g.tm.names[i], "setup_hash") == 0 ? hash : map) += g.tm.ms[i];
    g.tm.names = {"setup_squeeze_host", "setup_hash", "setup_map"};
    g.tm.ms = {(float)squeeze_ms, hash, map};
}

template <class F> int setup_bases_t(int curve, const unsigned char *label, size_t label_len, uint64_t first, size_t n, void *d_out, bool resident) {
    const size_t chunk = std::min<size_t>(n, std::max<size_t>(1, tuned(MIRA_TUNE_SETUP_CHUNK, SETUP_CHUNK_DEFAULT)));
    int rc;
    if ((rc = g.setup_stage.ensure(2 * chunk * 32))) return rc;
    unsigned char *pinned[2] = {nullptr, nullptr};
    double squeeze_ms = 0;
    auto body = [&]() -> int {
        for (int k = 0; k < 2; k++) RT_CHECK(rt_host_alloc(reinterpret_cast<void **>(&pinned[k]), chunk * 32));
#ifndef MIRA_CPU_EMU
        if (!g.copy_stream) RT_CHECK(hipStreamCreateWithFlags(&g.copy_stream, hipStreamNonBlocking));
        while (g.copy_events.size() < 4) {
            hipEvent_t e;
            RT_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            g.copy_events.push_back(e);
        }
#endif
        hipStream_t st = g.stream, cs = g.copy_stream ? g.copy_stream : st;
        Shake256 xof(label, label_len);
        xof.skip(first * 32);
        unsigned char *dst = reinterpret_cast<unsigned char *>(d_out);
        tm_begin();
        size_t i = 0;
        for (size_t off = 0; off < n; off += chunk, i++) {
            const size_t cnt = std::min(chunk, n - off);
            unsigned char *buf = pinned[i & 1], *stage = reinterpret_cast<unsigned char *>(g.setup_stage.p) + (i & 1) * chunk * 32;
#ifndef MIRA_CPU_EMU
            if (i >= 2) RT_CHECK(rt_event_sync(g.copy_events[i & 1]));                           // the copy out of this pinned buffer two chunks ago is done
#endif
            const auto t0 = std::chrono::steady_clock::now();
            xof.squeeze(buf, cnt * 32);
            squeeze_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
#ifndef MIRA_CPU_EMU
            if (i >= 2 && cs != st) RT_CHECK(hipStreamWaitEvent(cs, g.copy_events[2 + (i & 1)], 0));   // ... and the hash kernel that read this half of the stage
#endif
            RT_CHECK(rt_h2d(stage, buf, cnt * 32, cs));
#ifndef MIRA_CPU_EMU
            if (cs != st) RT_CHECK(rt_stream_wait(st, cs, g.copy_events[i & 1]));
            else RT_CHECK(hipEventRecord(g.copy_events[i & 1], cs));
#endif
            launch_hash<F>(curve, stage, cnt, dst + off * 64, st);
#ifndef MIRA_CPU_EMU
            RT_CHECK(hipEventRecord(g.copy_events[2 + (i & 1)], st));
#endif
            tm_mark("setup_hash");
            launch_map<F>(dst + off * 64, cnt, dst + off * 64, resident, st);                    // in place: u_0, u_1 lie in the point's own slot
            tm_mark("setup_map");
        }
        RT_CHECK(rt_last());
        RT_CHECK(rt_sync(cs));
        RT_CHECK(rt_sync(st));
        tm_end();
        fold_timings(squeeze_ms);
        return MIRA_OK;
    };
    rc = body();
    if (rc != MIRA_OK) { if (g.copy_stream) (void)rt_sync(g.copy_stream); (void)rt_sync(g.stream); }
    for (int k = 0; k < 2; k++) if (pinned[k]) (void)rt_host_free(pinned[k]);
    return rc;
}

template <class F> int run_stage(int curve, const void *d_in, size_t n, void *d_out, bool hash) {
    tm_begin();
    if (hash) launch_hash<F>(curve, d_in, n, d_out, g.stream);
    else launch_map<F>(d_in, n, d_out, false, g.stream);
    tm_mark(hash ? "setup_hash" : "setup_map");
    RT_CHECK(rt_last());
    RT_CHECK(rt_sync(g.stream));
    tm_end();
    return MIRA_OK;
}

}   // namespace

// curve 0 (BN256 G1) has its coordinates in Fq, curve 1 (Grumpkin G1) in bn256's Fr
int setup_hash_device(int curve, const void *d_msgs, size_t n, void *d_u) {
    return curve == MIRA_CURVE_BN256 ? run_stage<Fq29>(curve, d_msgs, n, d_u, true) : run_stage<Fr29>(curve, d_msgs, n, d_u, true);
}
int setup_map_device(int curve, const void *d_u, size_t n, void *d_points) {
    return curve == MIRA_CURVE_BN256 ? run_stage<Fq29>(curve, d_u, n, d_points, false) : run_stage<Fr29>(curve, d_u, n, d_points, false);
}
int setup_bases_device(int curve, const unsigned char *label, size_t label_len, uint64_t first, size_t n, void *d_out, bool resident) {
    return curve == MIRA_CURVE_BN256 ? setup_bases_t<Fq29>(curve, label, label_len, first, n, d_out, resident)
                                     : setup_bases_t<Fr29>(curve, label, label_len, first, n, d_out, resident);
}
