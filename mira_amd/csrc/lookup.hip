// Host side of the lookup-argument kernels (lookup_kernels.cuh): batch inversion, the multiplicities m and the fused h, g.
// The device code of this unit keeps the in-place multiplier (field29.cuh: F29_COLUMN_SERIAL): k_inv_top, whose Fermat chain
// keeps an accumulator and an LDS table across loops, compiles worse around the column-serial form (128 VGPRs with 6 spilled
// against 89, 4 158 VALU instructions against 2 992 for the same 1 321 multiply-adds), and the other kernels here are
// latency-bound tails.  Device code only: a unit's device code is a code object of its own, while the host bodies of the inline
// multipliers are shared by every unit of the library and must be the same everywhere.
// (decide.hip includes lookup_kernels.cuh too and compiles what it uses of it column-serial; k_inv_top is launched from here only.)
#if defined(__HIP_DEVICE_COMPILE__)
#undef F29_COLUMN_SERIAL
#define F29_COLUMN_SERIAL 0
#endif
#include "ctx.h"
#include "lookup_kernels.cuh"

namespace {

constexpr uint32_t INV_TOP_LANES = 256;     // the one workgroup that runs the Fermat chain
constexpr uint32_t INV_CHUNK_DEFAULT = 8;   // elements per lane below it

uint32_t inv_chunk() { return (uint32_t)std::min<size_t>(64, std::max<size_t>(2, tuned(MIRA_TUNE_INV_CHUNK, INV_CHUNK_DEFAULT))); }

// The levels of one batch inversion: level l holds n[l] elements over G[l] = ceil(n[l] / K) lanes; the last level (at most
// INV_TOP_LANES * K elements) is the top workgroup's.
struct InvPlan {
    std::vector<uint64_t> n, G;   // n.size() == G.size() + 1
    uint64_t ws_elems = 0;        // level >= 1 values and prefix products
    InvPlan(uint64_t n0, uint32_t K) {
        n.push_back(n0);
        while (n.back() > (uint64_t)INV_TOP_LANES * K) {
            G.push_back((n.back() + K - 1) / K);
            n.push_back(G.back());
            ws_elems += 2 * G.back();
        }
    }
};

// Level 0 is `lv`; `pre0_ws`: level 0's prefix products go to the workspace (in-place inversion) rather than to the outputs.
template <class F> int run_inversion(InvLevel0 lv, bool pre0_ws, uint32_t *d_err) {
    const InvPlan plan(lv.n, inv_chunk());
    const size_t pre0 = pre0_ws ? lv.n : 0;
    int rc;
    if ((rc = g.inv_ws.ensure((plan.ws_elems + pre0) * 32 + 32))) return rc;
    unsigned char *ws = reinterpret_cast<unsigned char *>(g.inv_ws.p);
    if (pre0_ws) {
        lv.pre[0] = ws;
        lv.pre[1] = ws + lv.n0 * 32;
    }
    std::vector<InvLevelN> up;   // levels 1 .. D
    size_t off = pre0 * 32;
    for (size_t l = 1; l < plan.n.size(); l++) {
        up.push_back(InvLevelN{ws + off, ws + off + plan.n[l] * 32, plan.n[l]});
        off += 2 * plan.n[l] * 32;
    }
    const size_t D = plan.G.size();
    for (size_t l = 0; l < D; l++) {
        const uint32_t grid = ceil_div(plan.G[l], 256);
        if (l == 0) LAUNCH((k_inv_up<F, InvLevel0, InvAcc0>), grid, 256, 0, g.stream, lv, (uint64_t)plan.G[0], up[0].vals, d_err);
        else LAUNCH((k_inv_up<F, InvLevelN, InvAccN>), grid, 256, 0, g.stream, up[l - 1], (uint64_t)plan.G[l], up[l].vals, d_err);
    }
    const size_t shmem = (2 * INV_TOP_LANES + 16) * sizeof(Fe29<F>);
    if (D == 0) LAUNCH_BARRIER_FLEX((k_inv_top<F, InvLevel0, InvAcc0>), 1, INV_TOP_LANES, shmem, g.stream, lv, d_err);
    else LAUNCH_BARRIER_FLEX((k_inv_top<F, InvLevelN, InvAccN>), 1, INV_TOP_LANES, shmem, g.stream, up[D - 1], d_err);
    for (size_t l = D; l-- > 0;) {
        const uint32_t grid = ceil_div(plan.G[l], 256);
        if (l == 0) LAUNCH((k_inv_down<F, InvLevel0, InvAcc0>), grid, 256, 0, g.stream, lv, (uint64_t)plan.G[0], (const unsigned char *)up[0].vals, d_err);
        else LAUNCH((k_inv_down<F, InvLevelN, InvAccN>), grid, 256, 0, g.stream, up[l - 1], (uint64_t)plan.G[l], (const unsigned char *)up[l].vals, d_err);
    }
    return MIRA_OK;
}

// the error word the kernels raise, read after the stream has drained
int finish(const char *stage, uint32_t *d_err) {
    uint32_t err = 0;
    tm_mark(stage);
    RT_CHECK(rt_last());
    RT_CHECK(rt_d2h(&err, d_err, sizeof err, g.stream));
    RT_CHECK(rt_sync(g.stream));
    tm_end();
    if (err & LK_ERR_NONCANONICAL) { set_error(std::string(stage) + ": an input element is not canonical (>= the modulus)"); return MIRA_E_BAD_ARG; }
    if (err & LK_ERR_TABLE_FULL) { set_error(std::string(stage) + ": hash table full (internal error)"); return MIRA_E_NO_DEVICE; }
    return MIRA_OK;
}
int begin(uint32_t **d_err) {
    int rc;
    if ((rc = g.lk_err.ensure(sizeof(uint32_t)))) return rc;
    *d_err = reinterpret_cast<uint32_t *>(g.lk_err.p);
    RT_CHECK(rt_memset(*d_err, 0, sizeof(uint32_t), g.stream));
    tm_begin();
    return MIRA_OK;
}

template <class F> int batch_invert_t(void *d_out, const void *d_in, size_t n) {
    uint32_t *d_err;
    int rc;
    if ((rc = begin(&d_err))) return rc;
    InvLevel0 lv;
    memset(&lv, 0, sizeof lv);
    lv.in[0] = lv.in[1] = reinterpret_cast<const unsigned char *>(d_in);
    lv.out[0] = lv.out[1] = lv.pre[0] = lv.pre[1] = reinterpret_cast<unsigned char *>(d_out);
    lv.n0 = lv.n = n;
    if ((rc = run_inversion<F>(lv, d_out == d_in, d_err))) return rc;
    return finish("batch_invert", d_err);
}

template <class F> int lookup_h_g_t(void *d_h, void *d_g, const void *d_l, size_t n_l, const void *d_t, const void *d_m, size_t n_t, const uint64_t r[4]) {
    uint32_t *d_err;
    int rc;
    if ((rc = begin(&d_err))) return rc;
    InvLevel0 lv;
    memset(&lv, 0, sizeof lv);
    lv.in[0] = reinterpret_cast<const unsigned char *>(d_l);
    lv.in[1] = reinterpret_cast<const unsigned char *>(d_t);
    lv.out[0] = lv.pre[0] = reinterpret_cast<unsigned char *>(d_h);
    lv.out[1] = lv.pre[1] = reinterpret_cast<unsigned char *>(d_g);
    lv.mul1 = reinterpret_cast<const unsigned char *>(d_m);
    lv.n0 = n_l;
    lv.n = n_l + n_t;
    memcpy(lv.r, r, 32);
    lv.add_r = true;
    if ((rc = run_inversion<F>(lv, false, d_err))) return rc;
    return finish("lookup_h_g", d_err);
}

template <class F> int lookup_m_t(void *d_m, const void *d_l, size_t n_l, const void *d_t, size_t n_t) {
    using S = typename F::Sat;
    uint64_t cap = 2;
    while (cap < 2 * (uint64_t)n_t) cap <<= 1;
    int rc;
    if ((rc = g.lk_owner.ensure(cap * 8)) || (rc = g.lk_first.ensure(cap * 4)) || (rc = g.lk_count.ensure(cap * 4)) || (rc = g.lk_slot.ensure((size_t)n_t * 8)))
        return rc;
    LkTable tab;
    tab.owner = reinterpret_cast<uint64_t *>(g.lk_owner.p);
    tab.first = reinterpret_cast<uint32_t *>(g.lk_first.p);
    tab.count = reinterpret_cast<uint32_t *>(g.lk_count.p);
    tab.slot_of_t = reinterpret_cast<uint64_t *>(g.lk_slot.p);
    tab.mask = cap - 1;
    tab.hash_mode = (uint32_t)tuned(MIRA_TUNE_LOOKUP_HASH, 0);
    uint32_t *d_err;
    if ((rc = begin(&d_err))) return rc;
    RT_CHECK(rt_memset(tab.owner, 0, cap * 8, g.stream));
    RT_CHECK(rt_memset(tab.first, 0xFF, cap * 4, g.stream));
    RT_CHECK(rt_memset(tab.count, 0, cap * 4, g.stream));
    const unsigned char *t = reinterpret_cast<const unsigned char *>(d_t), *l = reinterpret_cast<const unsigned char *>(d_l);
    LAUNCH(k_lk_insert<S>, ceil_div(n_t, 256), 256, 0, g.stream, t, (uint64_t)n_t, tab, d_err);
    // a bounded grid (8 workgroups per CU): each workgroup gathers the counts of its share of l in LDS before it adds them to HBM
    if (n_l) LAUNCH_BARRIER_FLEX(k_lk_count<S>, std::min<uint32_t>(ceil_div(n_l, 256), 2048), 256, 0, g.stream, l, (uint64_t)n_l, t, tab, d_err);
    LAUNCH(k_lk_write_m<F>, ceil_div(n_t, 256), 256, 0, g.stream, tab, (uint64_t)n_t, reinterpret_cast<unsigned char *>(d_m));
    return finish("lookup_m", d_err);
}

}   // namespace

int batch_invert_device(int field, void *d_out, const void *d_in, size_t n) {
    return field == MIRA_FIELD_FR ? batch_invert_t<Fr29>(d_out, d_in, n) : batch_invert_t<Fq29>(d_out, d_in, n);
}
int lookup_m_device(int field, void *d_m, const void *d_l, size_t n_l, const void *d_t, size_t n_t) {
    return field == MIRA_FIELD_FR ? lookup_m_t<Fr29>(d_m, d_l, n_l, d_t, n_t) : lookup_m_t<Fq29>(d_m, d_l, n_l, d_t, n_t);
}
int lookup_h_g_device(int field, void *d_h, void *d_g, const void *d_l, size_t n_l, const void *d_t, const void *d_m, size_t n_t, const uint64_t r[4]) {
    return field == MIRA_FIELD_FR ? lookup_h_g_t<Fr29>(d_h, d_g, d_l, n_l, d_t, d_m, n_t, r) : lookup_h_g_t<Fq29>(d_h, d_g, d_l, n_l, d_t, d_m, n_t, r);
}
