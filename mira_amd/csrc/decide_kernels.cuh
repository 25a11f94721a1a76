// The deciders of the reference (PlonkStructure::is_sat, is_sat_relaxed, is_sat_perm, is_sat_log_derivative,
// src/plonk/mod.rs:434-622) on vectors that already live in HBM.  Each of them ends in a count or a sum over a whole vector:
//
//   row sweep        #{row : f(row) != 0} (is_sat) or #{row : f(row) != E[row]} (is_sat_relaxed) -> EvaluationMismatch   k_count_ne
//   log-derivative   sum_i (h_i - g_i) == 0 per lookup                                                                   k_sum_sub
//   permutation      y = P Z (matrix_multiply, src/polynomial/sparse.rs:7-19), #{i : y_i != Z_i} -> PermCheckFail        k_perm_check
//
// Streaming / gather kernels over 32-byte elements, grid-stride over a bounded grid: HBM-bound.  Every lane keeps a count, the
// smallest mismatching index it saw (the reference warn!s the row) and / or a running field sum; the workgroup folds its lanes
// through LDS and writes ONE partial record to a workspace, and one more workgroup (k_decide_finish) folds the records into the
// result the host reads.  No global atomic but the error word: nothing depends on the order the workgroups ran in.
//
// Equality is decided on the 32-byte representation, as PartialEq on the canonical Montgomery limbs does in the reference; an
// input element >= the modulus raises the error word (the lookup kernels' contract) and counts as zero.
#pragma once
#include "fold_kernels.cuh"
#include "lookup_kernels.cuh"

static constexpr uint32_t DECIDE_BLOCK = 256;        // lanes per workgroup (any power of two works: the emulation runs 8)
static constexpr uint64_t DECIDE_NONE = ~0ull;       // `first` of a record without a mismatch

struct DecidePartial {
    uint64_t count, first;
};
// what the host reads back after k_decide_finish
struct DecideResult {
    uint64_t count, first;
    uint64_t sum[4];            // sum a - sum b, canonical Montgomery
    uint32_t err, pad;          // LookupErr bits
};
static_assert(sizeof(DecideResult) == 56, "read back in one copy");

template <class FP> DEV Fe<FP> decide_load(const unsigned char *p, uint32_t *err) {
    Fe<FP> v = fe_load<FP>(p);
    if (!lk_is_canonical(v)) {
        atomicMax(err, (uint32_t)LK_ERR_NONCANONICAL);
        v = fe_zero<FP>();
    }
    return v;
}

// count and minimum of the calling workgroup's lanes -> lane 0's return value; cnt, fst: blockDim.x words of LDS each
DEV DecidePartial decide_wg_count(uint64_t count, uint64_t first, uint64_t *cnt, uint64_t *fst) {
    const uint32_t j = threadIdx.x, L = blockDim.x;
    cnt[j] = count;
    fst[j] = first;
    __syncthreads();
    uint32_t w = 1;
    while (w < L) w <<= 1;
    for (w >>= 1; w >= 1; w >>= 1) {
        if (j < w && j + w < L) {
            cnt[j] += cnt[j + w];
            fst[j] = fst[j] < fst[j + w] ? fst[j] : fst[j + w];
        }
        __syncthreads();
    }
    return DecidePartial{cnt[0], fst[0]};
}
// the same for a field sum; red: blockDim.x elements of LDS
template <class FP> DEV Fe<FP> decide_wg_sum(const Fe<FP> &v, Fe<FP> *red) {
    const uint32_t j = threadIdx.x, L = blockDim.x;
    red[j] = v;
    __syncthreads();
    uint32_t w = 1;
    while (w < L) w <<= 1;
    for (w >>= 1; w >= 1; w >>= 1) {
        if (j < w && j + w < L) red[j] = fe_add(red[j], red[j + w]);
        __syncthreads();
    }
    return red[0];
}

// #{i < n : a[i] != b[i]} (b null: a[i] != 0) and the smallest such i: one record per workgroup
template <class F>
KERNEL void k_count_ne(const unsigned char *__restrict__ a, const unsigned char *__restrict__ b, uint64_t n, DecidePartial *__restrict__ parts, uint32_t *err) {
    using S = typename F::Sat;
    __shared__ uint64_t cnt[DECIDE_BLOCK], fst[DECIDE_BLOCK];
    uint64_t count = 0, first = DECIDE_NONE;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const Fe<S> x = decide_load<S>(a + i * 32, err);
        const bool ne = b ? !fe_eq(x, decide_load<S>(b + i * 32, err)) : !fe_is_zero(x);
        if (ne) {
            count++;
            if (first == DECIDE_NONE) first = i;              // a lane's indices only grow
        }
    }
    const DecidePartial r = decide_wg_count(count, first, cnt, fst);
    if (threadIdx.x == 0) parts[blockIdx.x] = r;
}

// sum a[i] and, when b is given, sum b[i]: one 32-byte partial per vector per workgroup, sums[v * gridDim.x + workgroup]
template <class F>
KERNEL void k_sum_sub(const unsigned char *__restrict__ a, const unsigned char *__restrict__ b, uint64_t n, unsigned char *__restrict__ sums, uint32_t *err) {
    using S = typename F::Sat;
    __shared__ Fe<S> red[DECIDE_BLOCK];
    Fe<S> sa = fe_zero<S>(), sb = fe_zero<S>();
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        sa = fe_add(sa, decide_load<S>(a + i * 32, err));
        if (b) sb = fe_add(sb, decide_load<S>(b + i * 32, err));
    }
    sa = decide_wg_sum(sa, red);
    if (threadIdx.x == 0) fe_store(sums + (size_t)blockIdx.x * 32, sa);
    if (!b) return;                                            // (uniform over the workgroup)
    __syncthreads();
    sb = decide_wg_sum(sb, red);
    if (threadIdx.x == 0) fe_store(sums + ((size_t)gridDim.x + blockIdx.x) * 32, sb);
}

// One workgroup folds G partial records (parts, or null) and G partial sums per vector (sums, or null; two_sums: a second
// vector follows the first) into the result: count, first (DECIDE_NONE if no record has one) and sum a - sum b.  Addition in
// the field is exact and associative (and so are integer addition and the minimum), so ANY reduction tree -- this one, whatever
// the grid was -- gives the value of the reference's sequential loops bit for bit.
template <class F>
KERNEL void k_decide_finish(const DecidePartial *__restrict__ parts, const unsigned char *__restrict__ sums, uint32_t two_sums, uint32_t G, DecideResult *out) {
    using S = typename F::Sat;
    __shared__ uint64_t cnt[DECIDE_BLOCK], fst[DECIDE_BLOCK];
    __shared__ Fe<S> red[DECIDE_BLOCK];
    uint64_t count = 0, first = DECIDE_NONE;
    Fe<S> sa = fe_zero<S>(), sb = fe_zero<S>();
    for (uint32_t k = threadIdx.x; k < G; k += blockDim.x) {
        if (parts) {
            count += parts[k].count;
            first = first < parts[k].first ? first : parts[k].first;
        }
        if (sums) {
            sa = fe_add(sa, fe_load<S>(sums + (size_t)k * 32));
            if (two_sums) sb = fe_add(sb, fe_load<S>(sums + ((size_t)G + k) * 32));
        }
    }
    const DecidePartial r = decide_wg_count(count, first, cnt, fst);
    sa = decide_wg_sum(sa, red);
    __syncthreads();
    sb = decide_wg_sum(sb, red);
    if (threadIdx.x == 0) {
        out->count = r.count;
        out->first = r.first;
        fe_store(out->sum, fe_sub(sa, sb));
    }
}

// ---- is_sat_perm ----------------------------------------------------------------------------------------------------------
// A compiled permutation matrix (mira_perm_compile): N x N in one of two row encodings.
//   fast     every row holds exactly one entry of value ONE -- what construct_permutation_matrix emits for copy constraints
//            plus fill_sparse_matrix's identity rows (src/plonk/util.rs:44-71, 128-174): sigma[i] = the column of row i, and
//            y_i = Z[sigma[i]]
//   general  CSR: row_ptr[N + 1], col[nnz], val[nnz] in the 48-byte multiplier form fold_const_load reads;
//            y_i = sum val * Z[col] over the row's entries (none: 0), as matrix_multiply defines it on arbitrary triples
// Z = instance || W is never materialised: index j < num_io reads the instance buffer, j >= num_io reads w + (j - num_io) * 32.
struct PermMatrix {
    const uint32_t *sigma;          // fast form, or null
    const uint32_t *row_ptr, *col;
    const unsigned char *val;
    uint64_t n;
};
struct PermZ {
    const unsigned char *inst, *w;
    uint64_t num_io;
    DEV const unsigned char *at(uint64_t j) const { return j < num_io ? inst + j * 32 : w + (j - num_io) * 32; }
};
// One lane per row, grid-stride over the bounded grid; every Z element is some row's Z_i, where it is checked to be canonical.
template <class F>
KERNEL void k_perm_check(PermMatrix m, PermZ z, DecidePartial *__restrict__ parts, uint32_t *err) {
    using S = typename F::Sat;
    __shared__ uint64_t cnt[DECIDE_BLOCK], fst[DECIDE_BLOCK];
    uint64_t count = 0, first = DECIDE_NONE;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m.n; i += (uint64_t)gridDim.x * blockDim.x) {
        const Fe<S> zi = decide_load<S>(z.at(i), err);
        Fe<S> y;
        if (m.sigma) {
            y = fe_load<S>(z.at(m.sigma[i]));
        } else {
            y = fe_zero<S>();
            for (uint32_t e = m.row_ptr[i]; e < m.row_ptr[i + 1]; e++) {
                const Fe<S> zc = decide_load<S>(z.at(m.col[e]), err);
                y = fe_add(y, fold_canonical(f29_mul(f29_unpack_canonical<F>(zc), fold_const_load<F>(m.val + (size_t)e * 48))));
            }
        }
        if (!fe_eq(y, zi)) {
            count++;
            if (first == DECIDE_NONE) first = i;
        }
    }
    const DecidePartial r = decide_wg_count(count, first, cnt, fst);
    if (threadIdx.x == 0) parts[blockIdx.x] = r;
}
