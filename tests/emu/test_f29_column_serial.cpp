// TEST-ONLY: the column-serial multipliers of field29.cuh (host form: the same order in plain C++) against the in-place forms
// they replace (f29_inplace_ref.h), on operands at the documented limits (f29_operands.h): both fields, f29_mul, f29_sqr,
// f29_mul2_add and f29_redc, every column as its carry leaves it and every output limb.  Build/run: tests/test_f29_column_serial_emu.py
#define MIRA_CPU_EMU
#include <cstdint>
static uint64_t g_cols[18];
#define F29_COLUMN_HOOK(k, v) (g_cols[k] = (v))
#include "../../mira_amd/csrc/field29.cuh"
#include "f29_inplace_ref.h"
#include "f29_operands.h"
thread_local dim3 threadIdx, blockIdx;
dim3 blockDim, gridDim;
pthread_barrier_t *emu_barrier = nullptr;
unsigned char *emu_dyn_shared = nullptr;

#if !F29_COLUMN_SERIAL
#error "this test compares the column-serial form; build it with F29_COLUMN_SERIAL at its default"
#endif

template <class F> static Fe29<F> load(const uint32_t *l) {
    Fe29<F> r;
    for (int i = 0; i < 9; i++) r.l[i] = l[i];
    return r;
}
template <class F> static int run(const char *name) {
    static const char *const FN[4] = {"mul", "sqr", "mul2_add", "redc"};
    const std::vector<F29Case> cases = f29_cases<F>();
    long bad = 0, count[4] = {0, 0, 0, 0};
    for (const F29Case &k : cases) {
        uint32_t want[9];
        uint64_t want_cols[18];
        Fe29<F> got;
        for (int i = 0; i < 18; i++) g_cols[i] = ~0ull;
        const Fe29<F> a = load<F>(k.op[0]), b = load<F>(k.op[1]), c = load<F>(k.op[2]), d = load<F>(k.op[3]);
        switch (k.fn) {
        case F29_FN_MUL: f29_ref_mul<F>(k.op[0], k.op[1], want, want_cols); got = f29_mul(a, b); break;
        case F29_FN_SQR: f29_ref_sqr<F>(k.op[0], want, want_cols); got = f29_sqr(a); break;
        case F29_FN_MUL2_ADD: f29_ref_mul2_add<F>(k.op[0], k.op[1], k.op[2], k.op[3], want, want_cols); got = f29_mul2_add(a, b, c, d); break;
        default: f29_ref_redc<F>(k.op[0], want, want_cols); got = f29_redc(a); break;
        }
        count[k.fn]++;
        int diff = 0;
        for (int i = 0; i < 9; i++) diff += got.l[i] != want[i];
        for (int i = 0; i < 18; i++) diff += g_cols[i] != want_cols[i];
        if (diff && bad++ < 5) printf("%s %s: %d limbs or columns differ (a[0] = %08x, b[0] = %08x)\n", name, FN[k.fn], diff, k.op[0][0], k.op[1][0]);
    }
    // the list holds what it is meant to hold: the limits are in it and the big cases were not dropped by the budget filter
    const std::vector<F29Operand> ops = f29_operands<F>();
    bool has30 = false, has315 = false, has168 = false;
    for (const F29Operand &o : ops) {
        has30 |= f29_op_max(o) == 0x40000008u;
        has315 |= f29_op_max(o) == 3037000499u;
        has168 |= o.l[8] == 168u * F::P[8] + (uint32_t)((168ull * F::P[7] + ((168ull * F::P[6]) >> 29)) >> 29);
    }
    if (!has30 || !has315 || !has168 || count[0] < 300 || count[1] < 15 || count[2] < 5000 || count[3] < 20) {
        printf("%s: operand list incomplete (%ld mul, %ld sqr, %ld mul2_add, %ld redc)\n", name, count[0], count[1], count[2], count[3]);
        bad++;
    }
    printf("%s: %ld mul, %ld sqr, %ld mul2_add, %ld redc: %s\n", name, count[0], count[1], count[2], count[3], bad ? "FAIL" : "ok");
    return bad != 0;
}
int main() { return (run<Fq29>("Fq29") | run<Fr29>("Fr29")) ? 1 : 0; }
