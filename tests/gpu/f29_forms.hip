// TEST-ONLY: the device forms of f29_mul, f29_sqr, f29_mul2_add and f29_redc (field29.cuh, as libmira_gpu.so compiles them)
// against the in-place reference (tests/emu/f29_inplace_ref.h), limb by limb, on the operand set of tests/emu/f29_operands.h,
// for both fields.  4 096 lanes share the calls; each computes both forms and the kernel counts the limbs that differ; the host
// then compares the device's limbs with its own run of the reference as well.  Prints "<field>: <calls> calls, <n> limbs differ"
// per field and exits 0 only if n is 0 everywhere.  Build/run: tests/test_gpu_f29_column_serial.py
#include "../../mira_amd/csrc/field29.cuh"
#include "../emu/f29_inplace_ref.h"
#include "../emu/f29_operands.h"

static constexpr uint32_t LANES = 4096, BLOCK = 256;

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)

template <class F> __device__ Fe29<F> load_op(const uint32_t *l) {
    Fe29<F> r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.l[i] = l[i];
    return r;
}
// out: 9 limbs per call (the device form); differ: limbs on which the two forms disagree, summed over all calls
template <class F> __global__ void k_forms(const F29Case *cases, uint32_t n_cases, uint32_t *out, uint32_t *differ) {
    const uint32_t lane = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t bad = 0;
    for (uint32_t i = lane; i < n_cases; i += gridDim.x * blockDim.x) {
        const F29Case &k = cases[i];
        const Fe29<F> a = load_op<F>(k.op[0]), b = load_op<F>(k.op[1]), c = load_op<F>(k.op[2]), d = load_op<F>(k.op[3]);
        Fe29<F> got;
        uint32_t want[9];
        switch (k.fn) {
        case F29_FN_MUL: got = f29_mul(a, b); f29_ref_mul<F>(a.l, b.l, want, nullptr); break;
        case F29_FN_SQR: got = f29_sqr(a); f29_ref_sqr<F>(a.l, want, nullptr); break;
        case F29_FN_MUL2_ADD: got = f29_mul2_add(a, b, c, d); f29_ref_mul2_add<F>(a.l, b.l, c.l, d.l, want, nullptr); break;
        default: got = f29_redc(a); f29_ref_redc<F>(a.l, want, nullptr); break;
        }
        for (int q = 0; q < 9; q++) {
            out[(size_t)i * 9 + q] = got.l[q];
            bad += got.l[q] != want[q];
        }
    }
    if (bad) atomicAdd(differ, bad);
}

template <class F> static int run(const char *name) {
    const std::vector<F29Case> cases = f29_cases<F>();
    const uint32_t n = (uint32_t)cases.size();
    F29Case *d_cases = nullptr;
    uint32_t *d_out = nullptr, *d_differ = nullptr;
    CHECK(hipMalloc(&d_cases, n * sizeof(F29Case)));
    CHECK(hipMalloc(&d_out, (size_t)n * 9 * sizeof(uint32_t)));
    CHECK(hipMalloc(&d_differ, sizeof(uint32_t)));
    CHECK(hipMemcpy(d_cases, cases.data(), n * sizeof(F29Case), hipMemcpyHostToDevice));
    CHECK(hipMemset(d_out, 0xFF, (size_t)n * 9 * sizeof(uint32_t)));
    CHECK(hipMemset(d_differ, 0, sizeof(uint32_t)));
    hipLaunchKernelGGL(k_forms<F>, dim3(LANES / BLOCK), dim3(BLOCK), 0, 0, d_cases, n, d_out, d_differ);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    std::vector<uint32_t> out((size_t)n * 9);
    uint32_t differ = 0;
    CHECK(hipMemcpy(out.data(), d_out, out.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(&differ, d_differ, sizeof(uint32_t), hipMemcpyDeviceToHost));
    CHECK(hipFree(d_cases));
    CHECK(hipFree(d_out));
    CHECK(hipFree(d_differ));
    uint32_t host_differ = 0;
    for (uint32_t i = 0; i < n; i++) {
        const F29Case &k = cases[i];
        uint32_t want[9];
        switch (k.fn) {
        case F29_FN_MUL: f29_ref_mul<F>(k.op[0], k.op[1], want, nullptr); break;
        case F29_FN_SQR: f29_ref_sqr<F>(k.op[0], want, nullptr); break;
        case F29_FN_MUL2_ADD: f29_ref_mul2_add<F>(k.op[0], k.op[1], k.op[2], k.op[3], want, nullptr); break;
        default: f29_ref_redc<F>(k.op[0], want, nullptr); break;
        }
        for (int q = 0; q < 9; q++) host_differ += out[(size_t)i * 9 + q] != want[q];
    }
    printf("%s: %u calls, %u limbs differ (device reference), %u limbs differ (host reference), column-serial %d\n", name, n, differ, host_differ, (int)F29_COLUMN_SERIAL);
    return (differ || host_differ) ? 1 : 0;
}
int main() {
    const int q = run<Fq29>("Fq29");
    if (q > 1) return q;
    const int r = run<Fr29>("Fr29");
    return q | r;
}
