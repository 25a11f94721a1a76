// TEST-ONLY: the 512-bit reduction of hash_to_field (setup_kernels.cuh: setup_reduce512) against schoolbook long
// division, on the host with bound tracking on.  Build/run: see tests/test_setup_emu.py (plain and under the address
// and undefined-behaviour sanitizers).
#define MIRA_CPU_EMU
#define F29_TRACK
#include "../../mira_amd/csrc/setup_kernels.cuh"
thread_local dim3 threadIdx, blockIdx;
dim3 blockDim, gridDim;
pthread_barrier_t *emu_barrier = nullptr;
unsigned char *emu_dyn_shared = nullptr;

static uint64_t st = 0x5E7B0B;
static uint64_t rnd() { st += 0x9E3779B97F4A7C15ull; uint64_t z = st; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }

struct U512 {
    uint32_t w[16];   // least significant first
};
static U512 zero512() { U512 r; for (int i = 0; i < 16; i++) r.w[i] = 0; return r; }

// w mod P one bit at a time: r = 2 r + bit, minus P when that reaches it (r < P < 2^254 throughout: nine words never overflow)
template <class S> static void long_division(const U512 &v, uint32_t rem[8]) {
    uint32_t r[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int bit = 511; bit >= 0; bit--) {
        uint32_t carry = (v.w[bit / 32] >> (bit % 32)) & 1u;
        for (int i = 0; i < 9; i++) { const uint32_t top = r[i] >> 31; r[i] = (r[i] << 1) | carry; carry = top; }
        uint32_t d[9];
        uint64_t br = 0;
        for (int i = 0; i < 9; i++) {
            const uint64_t x = (uint64_t)r[i] - (i < 8 ? S::P[i] : 0u) - br;
            d[i] = (uint32_t)x;
            br = (x >> 32) & 1;
        }
        if (!br) for (int i = 0; i < 9; i++) r[i] = d[i];
    }
    for (int i = 0; i < 8; i++) rem[i] = r[i];
}
// k * P + delta (delta = -1, 0, +1) for k < 2^256 given as 8 words: the product fits 510 bits
template <class S> static U512 multiple_of_p(const uint32_t k[8], int delta) {
    U512 r = zero512();
    for (int i = 0; i < 8; i++) {
        uint64_t carry = 0;
        for (int j = 0; j < 8; j++) {
            const uint64_t x = (uint64_t)k[i] * S::P[j] + r.w[i + j] + carry;
            r.w[i + j] = (uint32_t)x;
            carry = x >> 32;
        }
        r.w[i + 8] = (uint32_t)carry;
    }
    if (delta > 0) { for (int i = 0; i < 16 && ++r.w[i] == 0; i++) {} }
    if (delta < 0) { for (int i = 0; i < 16 && r.w[i]-- == 0; i++) {} }
    return r;
}

template <class F> static int check(const char *name, const char *what, const U512 &v) {
    using S = typename F::Sat;
    uint32_t want[8];
    long_division<S>(v, want);
    const Fe<S> got = fe_from_mont(f29_to_r256(setup_reduce512<F>(v.w)));
    for (int i = 0; i < 8; i++)
        if (got.l[i] != want[i]) { printf("%s: %s differs from long division\n", name, what); return 1; }
    return 0;
}

template <class F> static int run(const char *name) {
    using S = typename F::Sat;
    int bad = 0;
    U512 v = zero512();
    bad += check<F>(name, "0", v);
    for (int i = 0; i < 16; i++) v.w[i] = 0xFFFFFFFFu;
    bad += check<F>(name, "2^512 - 1", v);
    for (int i = 0; i < 8; i++) { v.w[i] = 0; v.w[8 + i] = S::P[i]; }
    bad += check<F>(name, "P 2^256", v);
    for (int i = 0; i < 16 && v.w[i]-- == 0; i++) {}
    bad += check<F>(name, "P 2^256 - 1", v);
    // both halves >= P at once, and the halves P and P - 1
    for (int i = 0; i < 8; i++) { v.w[i] = S::P[i]; v.w[8 + i] = 0xFFFFFFFFu; }
    bad += check<F>(name, "(2^256 - 1) 2^256 + P", v);
    for (int i = 0; i < 8; i++) { v.w[i] = S::P[i]; v.w[8 + i] = S::P[i]; }
    v.w[0] -= 1;
    bad += check<F>(name, "P 2^256 + P - 1", v);
    // k P - 1, k P, k P + 1: small k, k around 2^256 / P (the largest multiples below 2^512 have k < 2^258: reached through
    // the all-ones case), random k
    for (int it = 0; it < 40; it++) {
        uint32_t k[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (it < 8) k[0] = (uint32_t)it + 1;
        else if (it < 12) { for (int i = 0; i < 8; i++) k[i] = 0xFFFFFFFFu; k[0] -= (uint32_t)(it - 8); }
        else if (it < 16) { k[0] = 5 + (uint32_t)(it - 12); k[7] = 0; k[6] = 0; k[5] = 1; }   // k P just above 2^256 ... the low half wraps
        else for (int i = 0; i < 8; i += 2) { const uint64_t x = rnd(); k[i] = (uint32_t)x; k[i + 1] = (uint32_t)(x >> 32); }
        for (int delta = -1; delta <= 1; delta++) bad += check<F>(name, "k P + delta", multiple_of_p<S>(k, delta));
    }
    for (int it = 0; it < 1000; it++) {
        for (int i = 0; i < 16; i += 2) { const uint64_t x = rnd(); v.w[i] = (uint32_t)x; v.w[i + 1] = (uint32_t)(x >> 32); }
        bad += check<F>(name, "random", v);
    }
    printf("%s: %s\n", name, bad ? "FAILED" : "ok");
    return bad;
}

int main() {
    int bad = run<Fq29>("Fq29");
    bad += run<Fr29>("Fr29");
    return bad ? 1 : 0;
}
