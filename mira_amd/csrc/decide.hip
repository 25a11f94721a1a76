// Host side of the decider kernels (decide_kernels.cuh): compare-and-count, field sums, and the permutation check with its
// compiled matrix objects.
#include "ctx.h"
#include "decide_kernels.cuh"
#include "host_field.hpp"
#include <new>

namespace {

constexpr uint32_t DECIDE_MAX_GRID = 2048;   // 8 workgroups per CU, as k_lk_count's

// workgroups of one sweep over n elements; MIRA_TUNE_DECIDE_GRID sets the number (tests: several workgroups at small sizes)
uint32_t decide_grid(uint64_t n) {
    const int64_t knob = g.tune[MIRA_TUNE_DECIDE_GRID];
    if (knob > 0) return (uint32_t)knob;                    // 1 .. DECIDE_MAX_GRID: mira_set_tuning rejects anything else
    return std::max<uint32_t>(1, (uint32_t)std::min<uint64_t>((n + DECIDE_BLOCK - 1) / DECIDE_BLOCK, DECIDE_MAX_GRID));
}

// g.decide_parts: the result record | one partial record per workgroup | one partial sum per vector per workgroup
struct Workspace {
    DecideResult *result;
    DecidePartial *parts;
    unsigned char *sums;
    uint32_t *err;
};
int begin(uint32_t G, Workspace &ws) {
    int rc;
    if ((rc = g.decide_parts.ensure(64 + (size_t)G * (sizeof(DecidePartial) + 2 * 32)))) return rc;
    unsigned char *p = reinterpret_cast<unsigned char *>(g.decide_parts.p);
    ws.result = reinterpret_cast<DecideResult *>(p);
    ws.parts = reinterpret_cast<DecidePartial *>(p + 64);
    ws.sums = p + 64 + (size_t)G * sizeof(DecidePartial);
    ws.err = &ws.result->err;
    RT_CHECK(rt_memset(p, 0, 64, g.stream));
    tm_begin();
    return MIRA_OK;
}
// the result record and the error word the kernels raised, read after the stream has drained
int finish(const char *stage, const Workspace &ws, DecideResult &res) {
    tm_mark(stage);
    RT_CHECK(rt_last());
    RT_CHECK(rt_d2h(&res, ws.result, sizeof res, g.stream));
    RT_CHECK(rt_sync(g.stream));
    tm_end();
    if (res.err & LK_ERR_NONCANONICAL) { set_error(std::string(stage) + ": an input element is not canonical (>= the modulus)"); return MIRA_E_BAD_ARG; }
    return MIRA_OK;
}

template <class F> int count_ne_t(const void *d_a, const void *d_b, size_t n, uint64_t *count_out, uint64_t *first_out) {
    const uint32_t G = decide_grid(n);
    Workspace ws;
    int rc;
    if ((rc = begin(G, ws))) return rc;
    LAUNCH_BARRIER_FLEX(k_count_ne<F>, G, DECIDE_BLOCK, 0, g.stream, reinterpret_cast<const unsigned char *>(d_a), reinterpret_cast<const unsigned char *>(d_b), (uint64_t)n,
                        ws.parts, ws.err);
    LAUNCH_BARRIER_FLEX(k_decide_finish<F>, 1, DECIDE_BLOCK, 0, g.stream, (const DecidePartial *)ws.parts, (const unsigned char *)nullptr, 0u, G, ws.result);
    DecideResult res;
    if ((rc = finish("count_ne", ws, res))) return rc;
    *count_out = res.count;
    if (first_out) *first_out = res.first;
    return MIRA_OK;
}

template <class F> int sum_sub_t(const void *d_a, const void *d_b, size_t n, uint64_t out[4]) {
    const uint32_t G = decide_grid(n);
    Workspace ws;
    int rc;
    if ((rc = begin(G, ws))) return rc;
    LAUNCH_BARRIER_FLEX(k_sum_sub<F>, G, DECIDE_BLOCK, 0, g.stream, reinterpret_cast<const unsigned char *>(d_a), reinterpret_cast<const unsigned char *>(d_b), (uint64_t)n, ws.sums,
                        ws.err);
    LAUNCH_BARRIER_FLEX(k_decide_finish<F>, 1, DECIDE_BLOCK, 0, g.stream, (const DecidePartial *)nullptr, (const unsigned char *)ws.sums, d_b ? 1u : 0u, G, ws.result);
    DecideResult res;
    if ((rc = finish("sum_sub", ws, res))) return rc;
    memcpy(out, res.sum, 32);
    return MIRA_OK;
}

// ---- compiled permutation matrices ------------------------------------------------------------------------------------
struct Perm {
    int field = 0;
    uint64_t n = 0, nnz = 0;
    bool fast = false;
    void *d = nullptr;                         // fast: sigma[n]; general: row_ptr[n + 1] | col[nnz] | val[nnz] (48 B each, 16-byte aligned)
    size_t o_col = 0, o_val = 0;
};
std::map<uint64_t, Perm> g_perms;

template <class FP> bool is_canonical(const uint64_t v[4]) {
    hostf::HFe<FP> s;
    memcpy(s.l, v, 32);
    return !hostf::geq_p(s);
}
template <class FP> bool is_one(const uint64_t v[4]) {
    const hostf::HFe<FP> o = hostf::one<FP>();
    return memcmp(o.l, v, 32) == 0;
}

template <class F> int perm_check_t(const Perm &pm, const uint64_t *instance, size_t num_io, const void *d_w, uint64_t *mismatch_out, uint64_t *first_out) {
    const uint32_t G = decide_grid(pm.n);
    Workspace ws;
    int rc;
    if ((rc = g.decide_inst.ensure(std::max<size_t>(num_io, 1) * 32))) return rc;
    if ((rc = begin(G, ws))) return rc;
    if (num_io) RT_CHECK(rt_h2d(g.decide_inst.p, instance, num_io * 32, g.stream));   // `instance` stays the caller's until finish() has drained the stream
    const unsigned char *base = reinterpret_cast<const unsigned char *>(pm.d);
    PermMatrix m;
    m.sigma = pm.fast ? reinterpret_cast<const uint32_t *>(base) : nullptr;
    m.row_ptr = reinterpret_cast<const uint32_t *>(base);
    m.col = reinterpret_cast<const uint32_t *>(base + pm.o_col);
    m.val = base + pm.o_val;
    m.n = pm.n;
    const PermZ z{reinterpret_cast<const unsigned char *>(g.decide_inst.p), reinterpret_cast<const unsigned char *>(d_w), (uint64_t)num_io};
    LAUNCH_BARRIER_FLEX(k_perm_check<F>, G, DECIDE_BLOCK, 0, g.stream, m, z, ws.parts, ws.err);
    LAUNCH_BARRIER_FLEX(k_decide_finish<F>, 1, DECIDE_BLOCK, 0, g.stream, (const DecidePartial *)ws.parts, (const unsigned char *)nullptr, 0u, G, ws.result);
    DecideResult res;
    if ((rc = finish("perm_check", ws, res))) return rc;
    *mismatch_out = res.count;
    if (first_out) *first_out = res.first;
    return MIRA_OK;
}

}   // namespace

int count_ne_device(int field, const void *d_a, const void *d_b, size_t n, uint64_t *count_out, uint64_t *first_out) {
    return field == MIRA_FIELD_FR ? count_ne_t<Fr29>(d_a, d_b, n, count_out, first_out) : count_ne_t<Fq29>(d_a, d_b, n, count_out, first_out);
}
int sum_sub_device(int field, const void *d_a, const void *d_b, size_t n, uint64_t out[4]) {
    return field == MIRA_FIELD_FR ? sum_sub_t<Fr29>(d_a, d_b, n, out) : sum_sub_t<Fq29>(d_a, d_b, n, out);
}

// COO -> the device form.  Triples in any order; duplicates of (row, col) stay separate entries of their row, which the
// kernel adds -- as the reference's loop does.
static int perm_compile_host(int field, const uint64_t *rows, const uint64_t *cols, const uint64_t *values, size_t nnz, size_t n, uint64_t *handle_out) {
    std::vector<uint32_t> row_ptr(n + 1, 0);
    bool all_one = true;
    for (size_t e = 0; e < nnz; e++) {
        if (rows[e] >= n || cols[e] >= n) { set_error("invalid matrix multiply: triple " + std::to_string(e) + " lies outside the " + std::to_string(n) + " x " + std::to_string(n) + " matrix"); return MIRA_E_BAD_ARG; }
        if (values) {
            const uint64_t *v = values + e * 4;
            if (!(field == MIRA_FIELD_FR ? is_canonical<FrP>(v) : is_canonical<FqP>(v))) { set_error("a matrix value is not canonical (>= the modulus)"); return MIRA_E_BAD_ARG; }
            all_one = all_one && (field == MIRA_FIELD_FR ? is_one<FrP>(v) : is_one<FqP>(v));
        }
        row_ptr[rows[e] + 1]++;
    }
    Perm pm;
    pm.field = field; pm.n = n; pm.nnz = nnz;
    pm.fast = all_one && nnz == n;
    for (size_t i = 0; i < n && pm.fast; i++) pm.fast = row_ptr[i + 1] == 1;
    for (size_t i = 0; i < n; i++) row_ptr[i + 1] += row_ptr[i];
    std::vector<unsigned char> stage;
    if (pm.fast) {
        stage.resize(std::max<size_t>(n, 1) * 4);
        uint32_t *sigma = reinterpret_cast<uint32_t *>(stage.data());
        for (size_t e = 0; e < nnz; e++) sigma[rows[e]] = (uint32_t)cols[e];
    } else {
        pm.o_col = (n + 1) * 4;
        pm.o_val = (pm.o_col + nnz * 4 + 15) & ~(size_t)15;
        stage.assign(pm.o_val + std::max<size_t>(nnz, 1) * 48, 0);
        memcpy(stage.data(), row_ptr.data(), (n + 1) * 4);
        uint32_t *col = reinterpret_cast<uint32_t *>(stage.data() + pm.o_col);
        std::vector<uint32_t> cursor(row_ptr.begin(), row_ptr.end() - 1);
        uint64_t one[4];
        if (field == MIRA_FIELD_FR) { auto o = hostf::one<FrP>(); memcpy(one, o.l, 32); } else { auto o = hostf::one<FqP>(); memcpy(one, o.l, 32); }
        for (size_t e = 0; e < nnz; e++) {
            const uint32_t at = cursor[rows[e]]++;
            col[at] = (uint32_t)cols[e];
            to_mult48(field, values ? values + e * 4 : one, reinterpret_cast<uint32_t *>(stage.data() + pm.o_val + (size_t)at * 48));
        }
    }
    if (rt_malloc(&pm.d, stage.size()) != hipSuccess || !pm.d) { set_error("device allocation for the permutation matrix failed"); return MIRA_E_ALLOC; }
    // (`stage` is pageable host memory about to go out of scope: drained before the return)
    if (rt_h2d(pm.d, stage.data(), stage.size(), g.stream) != hipSuccess || rt_sync(g.stream) != hipSuccess) {
        (void)rt_free(pm.d);
        set_error("uploading the permutation matrix failed");
        return MIRA_E_NO_DEVICE;
    }
    const uint64_t handle = g.next_handle;
    try {
        g_perms[handle] = pm;
    } catch (const std::bad_alloc &) {
        (void)rt_free(pm.d);
        throw;
    }
    *handle_out = g.next_handle++;
    return MIRA_OK;
}
// the host vectors are sized by the caller's n and nnz (up to 2^32 - 1 each): running out of host memory is an error code,
// not an exception through the C boundary
int perm_compile(int field, const uint64_t *rows, const uint64_t *cols, const uint64_t *values, size_t nnz, size_t n, uint64_t *handle_out) {
    try {
        return perm_compile_host(field, rows, cols, values, nnz, n, handle_out);
    } catch (const std::bad_alloc &) {
        set_error("host allocation for a permutation matrix of " + std::to_string(n) + " rows and " + std::to_string(nnz) + " entries failed");
        return MIRA_E_ALLOC;
    }
}

int perm_check_device(uint64_t handle, const uint64_t *instance, size_t num_io, const void *d_w, size_t n_w, uint64_t *mismatch_out, uint64_t *first_out) {
    auto it = g_perms.find(handle);
    if (it == g_perms.end()) { set_error("unknown permutation handle"); return MIRA_E_BAD_ARG; }
    const Perm &pm = it->second;
    if ((uint64_t)num_io + (uint64_t)n_w != pm.n) {
        set_error("the matrix was compiled for Z of " + std::to_string(pm.n) + " elements, got " + std::to_string(num_io) + " + " + std::to_string(n_w));
        return MIRA_E_BAD_ARG;
    }
    if (pm.n == 0) { *mismatch_out = 0; if (first_out) *first_out = DECIDE_NONE; return MIRA_OK; }
    return pm.field == MIRA_FIELD_FR ? perm_check_t<Fr29>(pm, instance, num_io, d_w, mismatch_out, first_out) : perm_check_t<Fq29>(pm, instance, num_io, d_w, mismatch_out, first_out);
}

int perm_free(uint64_t handle) {
    auto it = g_perms.find(handle);
    if (it == g_perms.end()) { set_error("unknown permutation handle"); return MIRA_E_BAD_ARG; }
    if (it->second.d) (void)rt_free(it->second.d);
    g_perms.erase(it);
    return MIRA_OK;
}
