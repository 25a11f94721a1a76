// TEST-ONLY: the in-place ("operand scanning") multipliers of field29.cuh as they stood before the column-serial form, kept as
// the reference that form is compared with, column by column (tests/emu/test_f29_column_serial.cpp) and limb by limb on the
// device (tests/gpu/f29_forms.hip).  Plain integers in, plain integers out: limbs[9] and, where asked for, the 18 columns as
// they stand when their carry leaves them (cols[17] is the last carry alone).
#pragma once
#if defined(__HIPCC__)
#define F29_REF_HD __host__ __device__
#else
#define F29_REF_HD
#endif

// the reduction and the output, shared by the four forms: c[0 .. 17] holds the operand terms
template <class F> F29_REF_HD inline void f29_ref_reduce(uint64_t *c, uint32_t *limbs, uint64_t *cols) {
    for (int k = 0; k < 9; k++) {
        uint32_t m = ((uint32_t)c[k] * F::N0) & 0x1FFFFFFFu;
        for (int j = 0; j < 9; j++) c[k + j] += (uint64_t)m * F::P[j];
        c[k + 1] += c[k] >> 29;
    }
    for (int i = 9; i < 17; i++) {
        limbs[i - 9] = (uint32_t)c[i] & 0x1FFFFFFFu;
        c[i + 1] += c[i] >> 29;
    }
    limbs[8] = (uint32_t)c[17];
    if (cols)
        for (int k = 0; k < 18; k++) cols[k] = c[k];
}
template <class F> F29_REF_HD inline void f29_ref_mul(const uint32_t *a, const uint32_t *b, uint32_t *limbs, uint64_t *cols) {
    uint64_t c[18];
    for (int k = 0; k < 18; k++) c[k] = 0;
    for (int i = 0; i < 9; i++)
        for (int j = 0; j < 9; j++) c[i + j] += (uint64_t)a[i] * b[j];
    f29_ref_reduce<F>(c, limbs, cols);
}
template <class F> F29_REF_HD inline void f29_ref_mul2_add(const uint32_t *a, const uint32_t *b, const uint32_t *c2, const uint32_t *d, uint32_t *limbs, uint64_t *cols) {
    uint64_t c[18];
    for (int k = 0; k < 18; k++) c[k] = 0;
    for (int i = 0; i < 9; i++)
        for (int j = 0; j < 9; j++) c[i + j] += (uint64_t)a[i] * b[j];
    for (int i = 0; i < 9; i++)
        for (int j = 0; j < 9; j++) c[i + j] += (uint64_t)c2[i] * d[j];
    f29_ref_reduce<F>(c, limbs, cols);
}
template <class F> F29_REF_HD inline void f29_ref_redc(const uint32_t *a, uint32_t *limbs, uint64_t *cols) {
    uint64_t c[18];
    for (int k = 0; k < 9; k++) { c[k] = a[k]; c[k + 9] = 0; }
    f29_ref_reduce<F>(c, limbs, cols);
}
template <class F> F29_REF_HD inline void f29_ref_sqr(const uint32_t *a, uint32_t *limbs, uint64_t *cols) {
    uint64_t c[18];
    for (int k = 0; k < 18; k++) c[k] = 0;
    uint32_t d[9];
    for (int i = 0; i < 9; i++) d[i] = a[i] << 1;
    for (int i = 0; i < 9; i++) {
        c[2 * i] += (uint64_t)a[i] * a[i];
        for (int j = i + 1; j < 9; j++) c[i + j] += (uint64_t)a[i] * d[j];
    }
    f29_ref_reduce<F>(c, limbs, cols);
}
