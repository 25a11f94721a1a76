// libmira_gpu.so: process-wide context + the C ABI of include/mira_gpu.h.  The host side
// mirrors the reference's compiled-language surface for this path: CommitmentKey::commit
// (src/commitment.rs:78-87) and fft / ifft / coset_fft / coset_ifft / best_fft
// (src/fft.rs:51-196).  Kernels live in the per-curve units and ntt.hip.
#include "ctx.h"
#include "glv_consts.h"
#include "host_curve.hpp"
#include "msm_route.h"
#include "msm_tuning.h"
#include <cerrno>
#include <chrono>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#ifdef MIRA_CPU_EMU
thread_local dim3 threadIdx, blockIdx;
dim3 blockDim, gridDim;
pthread_barrier_t *emu_barrier = nullptr;
unsigned char *emu_dyn_shared = nullptr;
#ifdef F29_TRACK
// The branch census (f29_census.h), for the tests alone: not in include/mira_gpu.h.  One line per (kernel, section, function, exit),
// "kernel|section|function|exit|count\n"; returns the length of the whole text, of which at most cap - 1 bytes and a terminating
// zero are written to buf.
extern "C" size_t mira_emu_census_read(char *buf, size_t cap) {
    std::map<std::string, uint64_t> merged;
    {
        std::lock_guard<std::mutex> lk(emu_census.m);
        for (const auto &kv : emu_census.hits)
            merged[std::string(std::get<0>(kv.first)) + "|" + std::get<1>(kv.first) + "|" + std::get<2>(kv.first) + "|" + std::get<3>(kv.first)] += kv.second;
    }
    std::string text;
    for (const auto &kv : merged) text += kv.first + "|" + std::to_string(kv.second) + "\n";
    if (buf && cap) {
        const size_t len = text.size() < cap - 1 ? text.size() : cap - 1;
        memcpy(buf, text.data(), len);
        buf[len] = 0;
    }
    return text.size();
}
extern "C" void mira_emu_census_reset() {
    std::lock_guard<std::mutex> lk(emu_census.m);
    emu_census.hits.clear();
}
#endif
#endif

static thread_local std::string g_err;
void set_error(const std::string &s) { g_err = s; }
static std::mutex g_lock;
Ctx g;
static std::map<uint64_t, Bases> g_bases;

static int upload_consts();   // the device constants block (ctx.h: DevConsts)

static int ensure_ctx() {
    if (g.ready) return MIRA_OK;
#ifndef MIRA_CPU_EMU
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess || cnt <= 0) {
        set_error("no HIP device visible (libmira_gpu has no CPU fallback)");
        return MIRA_E_NO_DEVICE;
    }
    RT_CHECK(hipSetDevice(g.device));
    if (!g.stream) {
        RT_CHECK(hipStreamCreateWithFlags(&g.stream, hipStreamNonBlocking));
        g.own_stream = true;
    }
#endif
    int rc;
    if ((rc = curve_ops(MIRA_CURVE_BN256).init())) return rc;
    if ((rc = curve_ops(MIRA_CURVE_GRUMPKIN).init())) return rc;
    if ((rc = ntt_init())) return rc;
    g.ready = true;
    rc = upload_consts();
    if (rc != MIRA_OK) g.ready = false;
    return rc;
}

// ------------------------------------------------------------------------------------------
// timing
void tm_begin() {
    g.tm.names.clear(); g.tm.ms.clear();
#ifndef MIRA_CPU_EMU
    if (g.tm.enabled) {
        if (g.tm.ev.empty()) {
            g.tm.ev.resize(128);
            for (auto &e : g.tm.ev) (void)hipEventCreate(&e);
        }
        (void)hipEventRecord(g.tm.ev[0], g.stream);
    }
#endif
}
void tm_mark(const char *name) {
    if (!g.tm.enabled) return;
    g.tm.names.push_back(name);
#ifndef MIRA_CPU_EMU
    if (g.tm.names.size() < g.tm.ev.size()) (void)hipEventRecord(g.tm.ev[g.tm.names.size()], g.stream);
#endif
}
void tm_end() {   // after stream sync
    if (!g.tm.enabled) return;
    g.tm.ms.assign(g.tm.names.size(), 0.f);
#ifndef MIRA_CPU_EMU
    for (size_t i = 0; i < g.tm.names.size() && i + 1 < g.tm.ev.size(); i++)
        (void)hipEventElapsedTime(&g.tm.ms[i], g.tm.ev[i], g.tm.ev[i + 1]);
#endif
}

// ------------------------------------------------------------------------------------------
// curve constants
template <class FP> static hostf::HFe<FP> small_const(long v) {
    hostf::HFe<FP> x = hostf::from_u64<FP>((uint64_t)(v < 0 ? -v : v));
    return v < 0 ? hostf::sub(hostf::zero<FP>(), x) : x;
}
static int upload_consts() {
    DevConsts blk;
    memset(&blk, 0, sizeof blk);
    auto gx = small_const<FqP>(1), gy = small_const<FqP>(2);
    memcpy(blk.gen[MIRA_CURVE_BN256], gx.l, 32); memcpy(blk.gen[MIRA_CURVE_BN256] + 4, gy.l, 32);
    auto hx = small_const<FrP>(1);
    // sqrt(-16) mod r = 17631683881184975370165255887551781615748388533673675138860
    hostf::HFe<FrP> hy_plain = {{0x833fc48d823f272cULL, 0x2d270d45f1181294ULL, 0xcf135e7506a45d63ULL, 0x2ULL}};
    auto hy = hostf::to_mont(hy_plain);
    memcpy(blk.gen[MIRA_CURVE_GRUMPKIN], hx.l, 32); memcpy(blk.gen[MIRA_CURVE_GRUMPKIN] + 4, hy.l, 32);
    // curve constants in the resident R' = 2^261 form: b * 2^261 = (32 b) * 2^256
    auto b0 = small_const<FqP>(3 * 32);
    auto b1 = small_const<FrP>(-17 * 32);
    memcpy(blk.b_r261[MIRA_CURVE_BN256], b0.l, 32); memcpy(blk.b_r261[MIRA_CURVE_GRUMPKIN], b1.l, 32);
    // beta * 2^261 of each curve's endomorphism (glv.cuh): (32 beta) * 2^256, beta < 2^192
    auto beta_r261 = [](const uint64_t b[4], auto tag) {
        using FP = decltype(tag);
        hostf::HFe<FP> v = {{b[0] << 5, (b[1] << 5) | (b[0] >> 59), (b[2] << 5) | (b[1] >> 59), (b[3] << 5) | (b[2] >> 59)}};
        return hostf::to_mont(v);
    };
    auto be0 = beta_r261(Glv<FrP>::BETA, FqP{});
    auto be1 = beta_r261(Glv<FqP>::BETA, FrP{});
    memcpy(blk.beta_r261[MIRA_CURVE_BN256], be0.l, 32); memcpy(blk.beta_r261[MIRA_CURVE_GRUMPKIN], be1.l, 32);
    int rc = g.consts.ensure(sizeof blk);
    if (rc) return rc;
    RT_CHECK(rt_h2d(g.consts.p, &blk, sizeof blk, g.stream));
    RT_CHECK(rt_sync(g.stream));
    return MIRA_OK;
}

// ------------------------------------------------------------------------------------------
// argument checks every entry point shares
static bool curve_ok(int curve) { return curve == MIRA_CURVE_BN256 || curve == MIRA_CURVE_GRUMPKIN; }
static bool field_ok(int field) { return field == MIRA_FIELD_FQ || field == MIRA_FIELD_FR; }
static Bases *find_bases(uint64_t handle) {                  // null (and the error text) for a handle nobody registered
    auto it = g_bases.find(handle);
    if (it == g_bases.end()) { set_error("unknown bases handle"); return nullptr; }
    return &it->second;
}
// Error::TooLongInput (src/commitment.rs:21-24), the reference's text
static int too_long(size_t len, size_t limit) {
    set_error("Can't commit too long input: input len: " + std::to_string(len) + ", but limit is " + std::to_string(limit));
    return MIRA_E_TOO_LONG;
}

// ------------------------------------------------------------------------------------------
// MSM: the route is decided in msm_route.hip (on the planner, msm_plan.hip); here it is run

static double us_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count(); }
// One launch sequence through the per-window path (a shared-bucket set included), timed for the width or set trial it belongs
// to, and the bit-length statistics it collected (p.stats) kept as the planning input of the next commit of its shape
// (msm_launch ends with a stream synchronisation).
static int launch_and_report(const Bases &bs, size_t first, const void *d_scalars, const void *h_scalars, size_t n, const MsmPlan &p, uint64_t *out,
                             Bases::WidthTrial *trial) {
    const auto t_launch = std::chrono::steady_clock::now();
    const int rc = curve_ops(bs.curve).msm_launch(bs, first, d_scalars, h_scalars, n, p, out);
    if (rc != MIRA_OK) return rc;
    if (trial) trial_report(*trial, us_since(t_launch), bs);
    if (p.stats) {
        memcpy(bs.stat_hist, g.hist_host, sizeof bs.stat_hist);
        bs.stat_n = n; bs.stat_kind = p.glv ? 1 : 0;
    }
    return MIRA_OK;
}
// The endomorphism copy of a key, built the first time a commit takes the GLV split (msm_route.h: GlvCopyFn).  A failed allocation
// leaves the key as it is.
static bool glv_ready(const Bases &bs) {                     // the copy is there now
    if (bs.glv) return true;
    if (curve_ops(bs.curve).build_glv(const_cast<Bases &>(bs)) != MIRA_OK) { bs.glv_auto_failed = true; (void)rt_last(); return false; }
    return bs.glv != nullptr;
}
// what mira_msm_last_plan / mira_msm_last_table_bits answer
static void record_route(const MsmRoute &r) { g.last_c = r.last_c; g.last_w = r.last_w; g.last_table_c = r.last_table_c; }

// A single commit or a partial: the points of its route into out_partial (or rq.windows_dst), their shape into *shape.  h_scalars:
// the scalars are still in host memory, d_scalars is their staging buffer.
static int msm_partial_locked(uint64_t handle, MsmRequest rq, const void *d_scalars, const void *h_scalars, uint64_t *out_partial, PartialShape *shape) {
    int rc = ensure_ctx();
    if (rc) return rc;
    const Bases *found = find_bases(handle);
    if (!found) return MIRA_E_BAD_ARG;
    const Bases &bs = *found;
    if (rq.first > bs.n || rq.n > bs.n - rq.first) return too_long(rq.first + rq.n, bs.n);
    rq.have_scalars = d_scalars != nullptr; rq.host_scalars = h_scalars != nullptr;
    const MsmRoute r = route_commit(bs, rq, glv_ready);
    if (r.recorded) {
        *shape = r.shape;
        record_route(r);
        memset(out_partial, 0, MIRA_PARTIAL_U64 * 8);
    }
    if (r.rc) { set_error(r.err); return r.rc; }
    if (r.empty) return MIRA_OK;
    if (r.mode == MSM_WIDE_TABLE) {
        if (h_scalars) RT_CHECK(rt_h2d(const_cast<void *>(d_scalars), h_scalars, rq.n * 32, g.stream));
        return curve_ops(bs.curve).msm_launch_table(bs, rq.first, d_scalars, rq.n, out_partial, rq.windows_dst);
    }
    return launch_and_report(bs, rq.first, d_scalars, h_scalars, rq.n, r.plan, out_partial, r.trial);
}

static int combine_locked(int curve, const uint64_t *partials, size_t nparts, uint32_t c, uint32_t W, uint64_t out[8]) {
    if (!curve_ok(curve)) { set_error("unknown curve"); return MIRA_E_BAD_ARG; }
    if (!partials || !out || nparts == 0 || c > MSM_MAX_C || W < 1 || W > MIRA_MAX_WINDOWS) { set_error("bad combine arguments"); return MIRA_E_BAD_ARG; }
    std::vector<uint64_t> win((size_t)W * 16);
    const PartialShape sh{c, W, c ? c - 1 : 0, 1};           // (a caller's own description of its partials, not a route's)
    on_curve(curve, [&](auto fb, auto) {
        sum_partials<decltype(fb)>(partials, nparts, W, win.data());
        horner_pieces<decltype(fb)>(win.data(), sh, out);
    });
    return MIRA_OK;
}

// count MSMs over the prefix of one key in a single pass of the pipeline (a batch is count * W windows), in the launches its route
// cuts it into.  h_batch: the vectors are still in host memory, d_scalars is their staging buffer.
static int msm_batch_device_locked(uint64_t handle, const void *d_scalars, size_t n, size_t count, size_t stride, uint64_t *out_affine,
                                   const uint64_t *const *h_batch = nullptr) {
    int rc = ensure_ctx();
    if (rc) return rc;
    const Bases *found = find_bases(handle);
    if (!found) return MIRA_E_BAD_ARG;
    const Bases &bs = *found;
    if (!out_affine || (count && n && !d_scalars) || (count > 1 && stride < n)) { set_error("bad batch arguments"); return MIRA_E_BAD_ARG; }
    if (n > bs.n) return too_long(n, bs.n);
    MsmRequest rq;
    rq.n = n; rq.count = count; rq.stride = stride; rq.have_scalars = d_scalars != nullptr; rq.h_batch = h_batch;
    const BatchRoute b = route_batch(bs, rq, glv_ready);
    if (b.rc) { set_error(b.err); return b.rc; }
    if (b.empty) { memset(out_affine, 0, count * 64); return MIRA_OK; }
    const auto t_batch = std::chrono::steady_clock::now();
    std::vector<uint64_t> pts;
    for (size_t done = 0; done < count; done += b.per) {
        const MsmRoute r = route_batch_launch(bs, rq, b, done);
        const MsmPlan &p = r.plan;
        record_route(r);
        pts.assign((size_t)p.nsets * p.pieces * 16, 0);
        const unsigned char *sc = reinterpret_cast<const unsigned char *>(d_scalars) + done * stride * 32;
        rc = launch_and_report(bs, 0, sc, nullptr, n, p, pts.data(), r.trial);
        if (rc) return rc;
        if (r.trial_to_end) r.trial_to_end->done = true;
        const size_t per_commit = (size_t)r.shape.W * r.shape.P * 16;
        on_curve(bs.curve, [&](auto fb, auto) {
            auto finish = [&](size_t i) { horner_pieces<decltype(fb)>(pts.data() + i * per_commit, r.shape, out_affine + (done + i) * 8); };
            // the per-window epilogues of a batch are independent chains of ~250 doublings (60 us each): one host thread per
            // commitment; the sums of a shared-bucket set are just added
            if (r.mode == MSM_PER_WINDOW) host_parallel_for(p.count, finish);
            else for (size_t i = 0; i < p.count; i++) finish(i);
        });
    }
    if (b.set_trial) trial_report(*b.set_trial, us_since(t_batch), bs);   // (the whole batch: its launches and their epilogues)
    return MIRA_OK;
}

static int ntt_kind_device_ctx(void *d_a, uint32_t log_n, NttKind kind, const uint64_t *omega_in) {
    int rc = ensure_ctx();
    if (rc) return rc;
    return ntt_kind_device(d_a, log_n, kind, omega_in);
}
static int ntt_kind_host_locked(uint64_t *a, uint32_t log_n, NttKind kind, const uint64_t *omega_in) {
    int rc = ensure_ctx();
    if (rc) return rc;
    if (!a) { set_error("null argument"); return MIRA_E_BAD_ARG; }
    if (log_n > 28) { set_error("k=" + std::to_string(log_n) + " should no larger than F::S=28"); return MIRA_E_BAD_ARG; }
    const size_t bytes = (size_t)32 << log_n;
    if ((rc = g.ntt_stage.ensure(bytes))) return rc;
    RT_CHECK(rt_h2d(g.ntt_stage.p, a, bytes, g.stream));
    if ((rc = ntt_kind_device(g.ntt_stage.p, log_n, kind, omega_in))) return rc;
    RT_CHECK(rt_d2h(a, g.ntt_stage.p, bytes, g.stream));
    RT_CHECK(rt_sync(g.stream));
    return MIRA_OK;
}

// ------------------------------------------------------------------------------------------
// C ABI
extern "C" {

int mira_device_count(void) {
#ifndef MIRA_CPU_EMU
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess) return 0;
    return cnt;
#else
    return 1;
#endif
}
int mira_init(int device) {
    std::lock_guard<std::mutex> lk(g_lock);
    if (g.ready && device != g.device) { set_error("library already bound to device " + std::to_string(g.device)); return MIRA_E_BAD_ARG; }
    g.device = device;
    return ensure_ctx();
}
int mira_set_stream(void *hip_stream) {
    std::lock_guard<std::mutex> lk(g_lock);
    int rc = ensure_ctx();
    if (rc) return rc;
#ifndef MIRA_CPU_EMU
    if (hip_stream) {
        if (g.own_stream && g.stream) { (void)hipStreamSynchronize(g.stream); (void)hipStreamDestroy(g.stream); }
        g.stream = reinterpret_cast<hipStream_t>(hip_stream); g.own_stream = false;
    } else if (!g.own_stream) {
        RT_CHECK(hipStreamCreateWithFlags(&g.stream, hipStreamNonBlocking)); g.own_stream = true;
    }
#else
    (void)hip_stream;
#endif
    return MIRA_OK;
}
const char *mira_last_error(void) { return g_err.c_str(); }

// Both register calls leave a library-owned resident copy of the key in the engine's layout
// (canonical x * 2^261, y * 2^261; k_convert_bases), so the caller's buffer -- host or device --
// is free again when the call returns.
static int register_common(int curve, const void *src, bool src_on_device, size_t n, uint64_t *handle_out) {
    int rc = ensure_ctx();
    if (rc) return rc;
    if (!curve_ok(curve) || !handle_out || (n && !src)) { set_error("bad register arguments"); return MIRA_E_BAD_ARG; }
    Bases b; b.curve = curve; b.n = n; b.owned = true;
    if (rt_malloc(&b.d, std::max<size_t>(64, n * 64)) != hipSuccess || !b.d) { set_error("device allocation for bases failed"); return MIRA_E_ALLOC; }
    if (n) {
        const void *conv_src = src;
        if (!src_on_device) {
            RT_CHECK(rt_h2d(b.d, src, n * 64, g.stream));
            conv_src = b.d;   // convert in place
        }
        rc = curve_ops(curve).convert_bases(conv_src, b.d, n);
        if (rc) { (void)rt_free(b.d); return rc; }
    }
    *handle_out = g.next_handle++;
    g_bases[*handle_out] = b;
    return MIRA_OK;
}
int mira_msm_register_bases(int curve, const uint64_t *bases, size_t n, uint64_t *handle_out) {
    std::lock_guard<std::mutex> lk(g_lock);
    return register_common(curve, bases, false, n, handle_out);
}
int mira_msm_register_bases_device(int curve, const void *d_bases, size_t n, uint64_t *handle_out) {
    std::lock_guard<std::mutex> lk(g_lock);
    return register_common(curve, d_bases, true, n, handle_out);
}
int mira_msm_unregister(uint64_t handle) {
    std::lock_guard<std::mutex> lk(g_lock);
    const Bases *bs = find_bases(handle);
    if (!bs) return MIRA_E_BAD_ARG;
    if (bs->owned && bs->d) (void)rt_free(bs->d);
    if (bs->tables) (void)rt_free(bs->tables);
    for (auto &set : bs->shared) (void)rt_free(set.p);
    if (bs->glv) (void)rt_free(bs->glv);
    g_bases.erase(g_bases.find(handle));
    return MIRA_OK;
}
static int precompute_locked(uint64_t handle, int32_t window_bits) {
    int rc = ensure_ctx();
    if (rc) return rc;
    Bases *found = find_bases(handle);
    if (!found) return MIRA_E_BAD_ARG;
    Bases &bs = *found;
    if (window_bits >= 8 && window_bits <= 16) {             // a shared-bucket set: any number of widths beside each other
        for (const auto &set : bs.shared) if (set.c == (uint32_t)window_bits) return MIRA_OK;
        const uint32_t W = (256 + (uint32_t)window_bits - 1) / (uint32_t)window_bits;
        if ((uint64_t)bs.n * W >= (1ull << 31)) { set_error("key too long for 31-bit table indices"); return MIRA_E_UNSUPPORTED; }
        Bases tmp = bs;                                      // build_tables fills tables / table_c / table_w of what it is given
        tmp.tables = nullptr; tmp.table_c = tmp.table_w = 0;
        rc = curve_ops(bs.curve).build_tables(tmp, (uint32_t)window_bits, W);
        if (rc) return rc;
        if (tmp.tables) { bs.shared.push_back({tmp.tables, (uint32_t)window_bits, W}); bs.trials.clear(); }   // the trials among the sets start again
        return MIRA_OK;
    }
    if (window_bits == MIRA_TABLE_GLV) {                       // the interleaved key [P_i, phi(P_i)] of the GLV split
        if (bs.glv || bs.n == 0) return MIRA_OK;
        return curve_ops(bs.curve).build_glv(bs);
    }
    if (window_bits != 20 && window_bits != 22) { set_error("window tables are built for 8- to 16-bit (shared buckets), 20- or 22-bit windows"); return MIRA_E_BAD_ARG; }
    if (bs.tables && bs.table_c != (uint32_t)window_bits) { set_error("this key already has wide tables of another width"); return MIRA_E_BAD_ARG; }
    const uint32_t W = window_bits == 22 ? 12 : 13;          // ceil(256 / c); 12 x 22 = 264 covers a signed 254-bit scalar
    if ((uint64_t)bs.n * W >= (1ull << 31)) { set_error("key too long for 31-bit table indices"); return MIRA_E_UNSUPPORTED; }
    return curve_ops(bs.curve).build_tables(bs, (uint32_t)window_bits, W);
}
int mira_msm_precompute(uint64_t handle) {
    std::lock_guard<std::mutex> lk(g_lock);
    return precompute_locked(handle, 20);
}
int mira_msm_precompute_ex(uint64_t handle, int32_t window_bits) {
    std::lock_guard<std::mutex> lk(g_lock);
    return precompute_locked(handle, window_bits);
}
int mira_msm_check_bases(uint64_t handle) {
    std::lock_guard<std::mutex> lk(g_lock);
    int rc = ensure_ctx();
    if (rc) return rc;
    const Bases *found = find_bases(handle);
    if (!found) return MIRA_E_BAD_ARG;
    const Bases &bs = *found;
    if (bs.n == 0) return MIRA_OK;
    if ((rc = g.heavy.ensure(64))) return rc;
    uint32_t *bad = reinterpret_cast<uint32_t *>(g.heavy.p);
    RT_CHECK(rt_memset(bad, 0, 4, g.stream));
    if ((rc = curve_ops(bs.curve).check_bases(bs, bad))) return rc;
    uint32_t h = 0;
    RT_CHECK(rt_d2h(&h, bad, 4, g.stream));
    RT_CHECK(rt_sync(g.stream));
    if (h) { set_error("Wrong key, " + std::to_string(h) + " points out of curve"); return MIRA_E_INVALID_POINT; }
    return MIRA_OK;
}

static int msm_device_locked(uint64_t handle, const void *d_scalars, size_t n, uint64_t out_affine[8], const void *h_scalars = nullptr) {
    if (!out_affine) { set_error("null output"); return MIRA_E_BAD_ARG; }
    uint64_t part[MIRA_PARTIAL_U64];
    PartialShape sh;
    MsmRequest rq;
    rq.n = n; rq.caller_combines = true;
    int rc = msm_partial_locked(handle, rq, d_scalars, h_scalars, part, &sh);
    if (rc) return rc;
    on_curve(g_bases[handle].curve, [&](auto fb, auto) { horner_pieces<decltype(fb)>(part, sh, out_affine); });
    return MIRA_OK;
}
int mira_msm_device(uint64_t handle, const void *d_scalars, size_t n, uint64_t out_affine[8]) {
    std::lock_guard<std::mutex> lk(g_lock);
    return msm_device_locked(handle, d_scalars, n, out_affine);
}
int mira_msm(uint64_t handle, const uint64_t *scalars, size_t n, uint64_t out_affine[8]) {
    std::lock_guard<std::mutex> lk(g_lock);
    int rc = ensure_ctx();
    if (rc) return rc;
    if (n && !scalars) { set_error("null scalars"); return MIRA_E_BAD_ARG; }
    const Bases *bs = find_bases(handle);
    if (!bs) return MIRA_E_BAD_ARG;
    if (n > bs->n) return too_long(n, bs->n);   // length check before any copy, as commit does (src/commitment.rs:79)
    // the scalars cross PCIe inside the launch sequence, chunk by chunk beside the kernels (msm_host.cuh)
    if (n && (rc = g.scalars_stage.ensure(n * 32))) return rc;
    return msm_device_locked(handle, g.scalars_stage.p, n, out_affine, n ? scalars : nullptr);
}
int mira_msm_batch_device(uint64_t handle, const void *d_scalars, size_t n, size_t count, size_t stride_elems, uint64_t *out_affine) {
    std::lock_guard<std::mutex> lk(g_lock);
    return msm_batch_device_locked(handle, d_scalars, n, count, stride_elems, out_affine);
}
int mira_msm_batch(uint64_t handle, const uint64_t *const *scalars, size_t n, size_t count, uint64_t *out_affine) {
    std::lock_guard<std::mutex> lk(g_lock);
    int rc = ensure_ctx();
    if (rc) return rc;
    if (count && n && !scalars) { set_error("null scalars"); return MIRA_E_BAD_ARG; }
    const Bases *bs = find_bases(handle);
    if (!bs) return MIRA_E_BAD_ARG;
    if (n > bs->n) return too_long(n, bs->n);
    if (n && count) {
        if ((rc = g.scalars_stage.ensure(n * count * 32))) return rc;
        for (size_t b = 0; b < count; b++)
            if (!scalars[b]) { set_error("null scalars"); return MIRA_E_BAD_ARG; }
    }
    // the vectors cross PCIe inside the launch sequence, in point chunks beside the kernels (msm_host.cuh)
    return msm_batch_device_locked(handle, g.scalars_stage.p, n, count, n, out_affine, (n && count) ? scalars : nullptr);
}
int mira_msm_partial_device(uint64_t handle, size_t first, const void *d_scalars, size_t n, uint64_t out_partial[MIRA_PARTIAL_U64],
                            int32_t *window_bits, int32_t *num_windows) {
    std::lock_guard<std::mutex> lk(g_lock);
    if (!out_partial || !window_bits || !num_windows) { set_error("null output"); return MIRA_E_BAD_ARG; }
    if (*window_bits != 0 && (*window_bits < 4 || *window_bits > (int32_t)MSM_MAX_C)) { set_error("window_bits must be 0 or 4..20"); return MIRA_E_BAD_ARG; }
    PartialShape sh;
    MsmRequest rq;
    rq.first = first; rq.n = n; rq.sharded = true; rq.requested_c = *window_bits;
    int rc = msm_partial_locked(handle, rq, d_scalars, nullptr, out_partial, &sh);
    if (rc) return rc;
    *window_bits = (int32_t)sh.c; *num_windows = (int32_t)sh.W;
    return MIRA_OK;
}
int mira_msm_combine(int curve, const uint64_t *partials, size_t nparts, int32_t window_bits, int32_t num_windows, uint64_t out_affine[8]) {
    return combine_locked(curve, partials, nparts, (uint32_t)window_bits, (uint32_t)num_windows, out_affine);
}
int mira_set_tuning(int knob, int64_t value) {
    std::lock_guard<std::mutex> lk(g_lock);
    if (knob < 0 || knob > MIRA_TUNE_FOLDED_GRID || (knob == MIRA_TUNE_PASS_ENTRIES_LOG && value > 32)) { set_error("unknown tuning knob"); return MIRA_E_BAD_ARG; }
    if (knob == MIRA_TUNE_DECIDE_GRID && (value == 0 || value > 2048)) { set_error("MIRA_TUNE_DECIDE_GRID takes 1 .. 2048 workgroups (negative: the default)"); return MIRA_E_BAD_ARG; }
    if (knob == MIRA_TUNE_SETUP_CHUNK && value >= 0 && (value < 16 || value > (1 << 24))) { set_error("MIRA_TUNE_SETUP_CHUNK takes 16 .. 2^24 points (negative: the default)"); return MIRA_E_BAD_ARG; }
    if (knob == MIRA_TUNE_MIN_SEGMENT && (value == 0 || value > (1 << 20))) { set_error("MIRA_TUNE_MIN_SEGMENT takes 1 .. 2^20 entries (negative: the default)"); return MIRA_E_BAD_ARG; }
    g.tune[knob] = value;
    return MIRA_OK;
}
int mira_msm_plan_window_bits(size_t n, int32_t *window_bits) {
    std::lock_guard<std::mutex> lk(g_lock);                  // make_plan reads the tuning knobs mira_set_tuning writes under this lock
    if (!window_bits) { set_error("null output"); return MIRA_E_BAD_ARG; }
    *window_bits = (int32_t)make_plan(std::max<size_t>(n, 1), 0).c;
    return MIRA_OK;
}
int mira_msm_last_plan(int32_t *window_bits, int32_t *num_windows) {
    std::lock_guard<std::mutex> lk(g_lock);
    if (!window_bits || !num_windows) { set_error("null output"); return MIRA_E_BAD_ARG; }
    *window_bits = g.last_c; *num_windows = g.last_w;
    return MIRA_OK;
}
int mira_msm_last_table_bits(int32_t *table_bits) {
    std::lock_guard<std::mutex> lk(g_lock);
    if (!table_bits) { set_error("null output"); return MIRA_E_BAD_ARG; }
    *table_bits = g.last_table_c;
    return MIRA_OK;
}
int mira_msm_set_window_bits(int32_t c) {
    std::lock_guard<std::mutex> lk(g_lock);
    if (c != 0 && (c < 4 || c > 16)) { set_error("window bits must be 0 or in [4,16]"); return MIRA_E_BAD_ARG; }
    g.forced_c = c;
    return MIRA_OK;
}

int mira_msm_set_handle_window_bits(uint64_t handle, int32_t c) {
    std::lock_guard<std::mutex> lk(g_lock);
    if (c != 0 && (c < 4 || c > (int32_t)MSM_MAX_C)) { set_error("window bits must be 0 or in [4,20]"); return MIRA_E_BAD_ARG; }
    Bases *bs = find_bases(handle);
    if (!bs) return MIRA_E_BAD_ARG;
    bs->forced_c = c;
    return MIRA_OK;
}
int mira_msm_set_handle_max_window_bits(uint64_t handle, int32_t cmax) {
    std::lock_guard<std::mutex> lk(g_lock);
    if (cmax < (int32_t)MSM_MAX_NARROW_C || cmax > (int32_t)MSM_MAX_C) { set_error("max window bits must be in [16,20]"); return MIRA_E_BAD_ARG; }
    Bases *bs = find_bases(handle);
    if (!bs) return MIRA_E_BAD_ARG;
    if (bs->max_c != (uint32_t)cmax) { bs->max_c = (uint32_t)cmax; bs->trials.clear(); }   // the width trials start again
    return MIRA_OK;
}
// ---- a key's tuning as bytes (msm_tuning.hip): nothing is launched, no device memory is touched
// the architecture a blob was tuned on: the device's gcn arch name up to the first ':' (gfx950:sramecc+:xnack- -> gfx950)
static int tuning_arch(std::string *arch) {
#ifndef MIRA_CPU_EMU
    static std::string name;                                 // (under the library lock; the bound device does not change once a key exists)
    if (name.empty()) {
        hipDeviceProp_t prop;
        RT_CHECK(hipGetDeviceProperties(&prop, g.device));
        name = prop.gcnArchName;
        name = name.substr(0, name.find(':'));
        if (name.empty()) name = "unknown";
    }
    *arch = name;
#else
    *arch = "emu";
#endif
    return MIRA_OK;
}
int mira_msm_tuning_export(uint64_t handle, void *buf, size_t cap, size_t *len_out) {
    std::lock_guard<std::mutex> lk(g_lock);
    if (!len_out || (cap && !buf)) { set_error("null output"); return MIRA_E_BAD_ARG; }
    const Bases *bs = find_bases(handle);
    if (!bs) return MIRA_E_BAD_ARG;
    std::string arch;
    int rc = tuning_arch(&arch);
    if (rc) return rc;
    std::vector<unsigned char> bytes;
    tuning_export(*bs, arch.c_str(), &bytes);
    *len_out = bytes.size();
    if (cap == 0) return MIRA_OK;                            // the size query
    if (cap < bytes.size()) { set_error("tuning buffer too small: " + std::to_string(cap) + " bytes, the blob has " + std::to_string(bytes.size())); return MIRA_E_BAD_ARG; }
    memcpy(buf, bytes.data(), bytes.size());
    return MIRA_OK;
}
int mira_msm_tuning_import(uint64_t handle, const void *buf, size_t len, int32_t *accepted_out) {
    std::lock_guard<std::mutex> lk(g_lock);
    if (!accepted_out) { set_error("null output"); return MIRA_E_BAD_ARG; }
    *accepted_out = 0;
    if (!buf) { set_error("null tuning blob"); return MIRA_E_BAD_ARG; }
    const Bases *bs = find_bases(handle);
    if (!bs) return MIRA_E_BAD_ARG;
    std::string arch, err;
    int rc = tuning_arch(&arch);
    if (rc) return rc;
    rc = tuning_import(*bs, arch.c_str(), buf, len, accepted_out, &err);
    if (rc) set_error(err);
    return rc;
}

int mira_msm_partial_to_device(uint64_t handle, size_t first, const void *d_scalars, size_t n, void *d_out_partial,
                               int32_t *window_bits, int32_t *num_windows) {
    std::lock_guard<std::mutex> lk(g_lock);
    if (!d_out_partial || !window_bits || !num_windows) { set_error("null output"); return MIRA_E_BAD_ARG; }
    if (*window_bits != 0 && (*window_bits < 4 || *window_bits > (int32_t)MSM_MAX_C)) { set_error("window_bits must be 0 or 4..20"); return MIRA_E_BAD_ARG; }
    int rc = ensure_ctx();
    if (rc) return rc;
    RT_CHECK(rt_memset(d_out_partial, 0, MIRA_PARTIAL_U64 * 8, g.stream));     // words beyond the partial's windows (and an empty chunk) read as the identity
    RT_CHECK(rt_sync(g.stream));
    uint64_t unused[MIRA_PARTIAL_U64];
    PartialShape sh;
    MsmRequest rq;
    rq.first = first; rq.n = n; rq.sharded = true; rq.requested_c = *window_bits; rq.windows_dst = d_out_partial;
    if ((rc = msm_partial_locked(handle, rq, d_scalars, nullptr, unused, &sh))) return rc;
    *window_bits = (int32_t)sh.c; *num_windows = (int32_t)sh.W;
    return MIRA_OK;
}

// CommitmentKey::load_from_file + the is_on_curve pass of load_or_setup_cache (src/commitment.rs:110-127, 145-154)
int mira_msm_register_bases_file(int curve, const char *path, uint32_t k, int validate, uint64_t *handle_out) {
    std::lock_guard<std::mutex> lk(g_lock);
    int rc = ensure_ctx();
    if (rc) return rc;
    if (!curve_ok(curve) || !path || !handle_out || k > 31) { set_error("bad register arguments"); return MIRA_E_BAD_ARG; }
    const size_t n = (size_t)1 << k;
    const int fd = open(path, O_RDONLY);
    if (fd < 0) { set_error(std::string(path) + ": " + strerror(errno)); return MIRA_E_IO; }
    struct stat sb;
    if (fstat(fd, &sb) != 0 || (size_t)sb.st_size < n * 64) {                  // read_exact of vec_len * size_of::<C>() bytes
        set_error("failed to fill whole buffer");
        close(fd);
        return MIRA_E_IO;
    }
    Bases b; b.curve = curve; b.n = n; b.owned = true;
    if (rt_malloc(&b.d, n * 64) != hipSuccess || !b.d) { close(fd); set_error("device allocation for bases failed"); return MIRA_E_ALLOC; }
    uint32_t *bad = nullptr;
    if ((rc = g.heavy.ensure(64)) == MIRA_OK) {
        bad = reinterpret_cast<uint32_t *>(g.heavy.p);
        rc = curve_ops(curve).load_bases_file(b, fd, validate != 0, bad);
    }
    close(fd);
    if (rc == MIRA_OK && validate) {
        uint32_t h = 0;
        if (rt_d2h(&h, bad, 4, g.stream) != hipSuccess || rt_sync(g.stream) != hipSuccess) { set_error("device to host copy failed"); rc = MIRA_E_NO_DEVICE; }
        else if (h) { set_error("Wrong file in cache, some ptr out of curve"); rc = MIRA_E_INVALID_POINT; }
    }
    if (rc != MIRA_OK) { (void)rt_free(b.d); return rc; }
    *handle_out = g.next_handle++;
    g_bases[*handle_out] = b;
    return MIRA_OK;
}
// save_to_file (src/commitment.rs:96-101): the key as the raw slice of reference-layout points
int mira_msm_save_bases_file(uint64_t handle, const char *path) {
    std::lock_guard<std::mutex> lk(g_lock);
    int rc = ensure_ctx();
    if (rc) return rc;
    const Bases *bs = find_bases(handle);
    if (!bs || !path) { set_error("unknown bases handle"); return MIRA_E_BAD_ARG; }
    const int fd = open(path, O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (fd < 0) { set_error(std::string(path) + ": " + strerror(errno)); return MIRA_E_IO; }
    rc = curve_ops(bs->curve).save_bases_file(*bs, fd);
    if (close(fd) != 0 && rc == MIRA_OK) { set_error(std::string("close failed: ") + strerror(errno)); rc = MIRA_E_IO; }
    return rc;
}

// Release grow-only workspaces, largest first, until at most keep_bytes remain.
int mira_trim(size_t keep_bytes, size_t *released_out) {
    std::lock_guard<std::mutex> lk(g_lock);
    if (released_out) *released_out = 0;
    if (!g.ready) return MIRA_OK;
    RT_CHECK(rt_sync(g.stream));
    if (g.copy_stream) RT_CHECK(rt_sync(g.copy_stream));
    // `consts`, `ntt_consts` and `fold_consts` hold uploaded constants (a few hundred bytes): never released
    std::vector<DevBuf *> bufs = {&g.digits, &g.counts, &g.offsets, &g.cursor, &g.block_sums, &g.sorted_idx, &g.bucket_sums, &g.part, &g.coarse_offsets,
                                  &g.fine_counts, &g.fine_cursor, &g.head_part, &g.tail_part, &g.tail_key, &g.heavy, &g.heavy_out, &g.chunks, &g.window_sums,
                                  &g.scalars_stage, &g.ntt_tmp, &g.ntt_stage, &g.graph_ws, &g.fold_nodes, &g.tree_a, &g.tree_b, &g.hist_dev,
                                  &g.inv_ws, &g.lk_owner, &g.lk_first, &g.lk_count, &g.lk_slot, &g.decide_parts, &g.decide_eval, &g.decide_inst, &g.setup_stage};
    for (int i = 0; i < Ctx::NTT_SETS; i++) bufs.push_back(&g.ntt_set[i]);
    size_t total = 0;
    for (DevBuf *b : bufs) total += b->cap;
    std::sort(bufs.begin(), bufs.end(), [](const DevBuf *a, const DevBuf *b) { return a->cap > b->cap; });
    size_t released = 0;
    for (DevBuf *b : bufs) {
        if (total - released <= keep_bytes || b->cap == 0) break;
        for (int i = 0; i < Ctx::NTT_SETS; i++)
            if (b == &g.ntt_set[i]) { g.ntt_set_key[i].clear(); g.ntt_set_stamp[i] = 0; }
        if (b == &g.hist_dev) g.hist_sel = 0;
        released += b->cap;
        b->release();
    }
    if (released_out) *released_out = released;
    return MIRA_OK;
}
int mira_dev_mem_info(size_t *free_bytes, size_t *total_bytes) {
    std::lock_guard<std::mutex> lk(g_lock);
    int rc = ensure_ctx();
    if (rc) return rc;
    size_t f = 0, t = 0;
#ifndef MIRA_CPU_EMU
    RT_CHECK(hipMemGetInfo(&f, &t));
#endif
    if (free_bytes) *free_bytes = f;
    if (total_bytes) *total_bytes = t;
    return MIRA_OK;
}

int mira_ntt_bn256_fr(uint64_t *a, uint32_t log_n, const uint64_t omega[4]) {
    std::lock_guard<std::mutex> lk(g_lock);
    if (!omega) { set_error("null omega"); return MIRA_E_BAD_ARG; }
    return ntt_kind_host_locked(a, log_n, NTT_BEST, omega);
}
int mira_ntt_bn256_fr_device(void *d_a, uint32_t log_n, const uint64_t omega[4]) {
    std::lock_guard<std::mutex> lk(g_lock);
    if (!omega) { set_error("null omega"); return MIRA_E_BAD_ARG; }
    return ntt_kind_device_ctx(d_a, log_n, NTT_BEST, omega);
}
int mira_fft_bn256_fr(uint64_t *a, uint32_t log_n) { std::lock_guard<std::mutex> lk(g_lock); return ntt_kind_host_locked(a, log_n, NTT_FFT, nullptr); }
int mira_ifft_bn256_fr(uint64_t *a, uint32_t log_n) { std::lock_guard<std::mutex> lk(g_lock); return ntt_kind_host_locked(a, log_n, NTT_IFFT, nullptr); }
int mira_fft_bn256_fr_device(void *d_a, uint32_t log_n) { std::lock_guard<std::mutex> lk(g_lock); return ntt_kind_device_ctx(d_a, log_n, NTT_FFT, nullptr); }
int mira_ifft_bn256_fr_device(void *d_a, uint32_t log_n) { std::lock_guard<std::mutex> lk(g_lock); return ntt_kind_device_ctx(d_a, log_n, NTT_IFFT, nullptr); }
int mira_coset_fft_bn256_fr(uint64_t *a, uint32_t log_n) { std::lock_guard<std::mutex> lk(g_lock); return ntt_kind_host_locked(a, log_n, NTT_COSET_FFT, nullptr); }
int mira_coset_ifft_bn256_fr(uint64_t *a, uint32_t log_n) { std::lock_guard<std::mutex> lk(g_lock); return ntt_kind_host_locked(a, log_n, NTT_COSET_IFFT, nullptr); }
int mira_get_omega_or_inv(uint32_t k, int is_inverse, uint64_t out[4]) {
    if (!out || k > 28) { set_error("k=" + std::to_string(k) + " should no larger than F::S=28"); return MIRA_E_BAD_ARG; }
    return ntt_get_omega_or_inv(k, is_inverse != 0, out);
}

int mira_fold_witness_device(int field, void *d_out, const void *d_w1, const void *d_w2, const uint64_t r[4], size_t n) {
    std::lock_guard<std::mutex> lk(g_lock);
    int rc = ensure_ctx();
    if (rc) return rc;
    if (!field_ok(field) || !r || (n && (!d_out || !d_w1 || !d_w2))) { set_error("bad fold arguments"); return MIRA_E_BAD_ARG; }
    if (!n) return MIRA_OK;
    return fold_witness_device(field, d_out, d_w1, d_w2, r, n);
}
// every cross-term vector of a fold over n elements is there
static int check_cross_terms(const void *const *d_cross_terms, size_t num_terms, size_t n) {
    for (size_t k = 0; k < num_terms; k++)
        if (n && !d_cross_terms[k]) { set_error("null cross term"); return MIRA_E_BAD_ARG; }
    return MIRA_OK;
}
int mira_fold_error_device(int field, void *d_e, const void *const *d_cross_terms, size_t num_terms, const uint64_t r[4], size_t n) {
    std::lock_guard<std::mutex> lk(g_lock);
    int rc = ensure_ctx();
    if (rc) return rc;
    if (!field_ok(field) || !r || num_terms > 16 || (num_terms && !d_cross_terms) || (n && !d_e)) { set_error("bad fold arguments"); return MIRA_E_BAD_ARG; }
    if ((rc = check_cross_terms(d_cross_terms, num_terms, n))) return rc;
    if (!n || !num_terms) return MIRA_OK;
    return fold_error_device(field, d_e, d_cross_terms, num_terms, r, n);
}
int mira_fold_relaxed_witness_device(int field, void *d_w_out, const void *d_w1, const void *d_w2, size_t n_w, void *d_e_out, const void *d_e,
                                     const void *const *d_cross_terms, size_t num_terms, const uint64_t r[4], size_t n) {
    std::lock_guard<std::mutex> lk(g_lock);
    int rc = ensure_ctx();
    if (rc) return rc;
    if (!field_ok(field) || !r || num_terms > 16 || (num_terms && !d_cross_terms) || (n_w && (!d_w_out || !d_w1 || !d_w2)) || (n && (!d_e_out || !d_e))) {
        set_error("bad fold arguments");
        return MIRA_E_BAD_ARG;
    }
    if ((rc = check_cross_terms(d_cross_terms, num_terms, n))) return rc;
    if (!n_w && !n) return MIRA_OK;
    return fold_relaxed_device(field, d_w_out, d_w1, d_w2, n_w, d_e_out, d_e, d_cross_terms, num_terms, r, n);
}
// ---- lookup argument (lookup.hip)
// [a, a + 32 na) and [b, b + 32 nb) share a byte
static bool lk_overlap(const void *a, size_t na, const void *b, size_t nb) {
    if (!na || !nb) return false;
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + 32 * nb && y < x + 32 * na;
}
static int lk_check_len(size_t n) {
    if ((uint64_t)n >= (1ull << 32)) { set_error("lookup vectors of 2^32 elements or more are not supported"); return MIRA_E_UNSUPPORTED; }
    return MIRA_OK;
}
int mira_batch_invert_device(int field, void *d_out, const void *d_in, size_t n) {
    std::lock_guard<std::mutex> lk(g_lock);
    int rc = ensure_ctx();
    if (rc) return rc;
    if (!field_ok(field) || (n && (!d_out || !d_in))) { set_error("bad batch-inversion arguments"); return MIRA_E_BAD_ARG; }
    if (!n) return MIRA_OK;
    if ((rc = lk_check_len(n))) return rc;
    if (d_out != d_in && lk_overlap(d_out, n, d_in, n)) { set_error("the output overlaps the input (only d_out == d_in is allowed)"); return MIRA_E_BAD_ARG; }
    return batch_invert_device(field, d_out, d_in, n);
}
int mira_lookup_m_device(int field, void *d_m, const void *d_l, size_t n_l, const void *d_t, size_t n_t) {
    std::lock_guard<std::mutex> lk(g_lock);
    int rc = ensure_ctx();
    if (rc) return rc;
    if (!field_ok(field) || (n_t && (!d_m || !d_t)) || (n_l && n_t && !d_l)) { set_error("bad lookup_m arguments"); return MIRA_E_BAD_ARG; }
    if (!n_t) return MIRA_OK;
    if ((rc = lk_check_len(n_l)) || (rc = lk_check_len(n_t))) return rc;
    if (lk_overlap(d_m, n_t, d_t, n_t) || lk_overlap(d_m, n_t, d_l, n_l)) { set_error("m overlaps an input"); return MIRA_E_BAD_ARG; }
    return lookup_m_device(field, d_m, d_l, n_l, d_t, n_t);
}
int mira_lookup_h_g_device(int field, void *d_h, void *d_g, const void *d_l, size_t n_l, const void *d_t, const void *d_m, size_t n_t, const uint64_t r[4]) {
    std::lock_guard<std::mutex> lk(g_lock);
    int rc = ensure_ctx();
    if (rc) return rc;
    if (!field_ok(field) || !r || (n_l && (!d_h || !d_l)) || (n_t && (!d_g || !d_t || !d_m))) { set_error("bad lookup_h_g arguments"); return MIRA_E_BAD_ARG; }
    if (!n_l && !n_t) return MIRA_OK;
    if ((rc = lk_check_len(n_l)) || (rc = lk_check_len(n_t))) return rc;
    const void *ins[3] = {d_l, d_t, d_m};
    const size_t in_n[3] = {n_l, n_t, n_t};
    for (int k = 0; k < 3; k++)
        if (lk_overlap(d_h, n_l, ins[k], in_n[k]) || lk_overlap(d_g, n_t, ins[k], in_n[k])) { set_error("an output of lookup_h_g overlaps an input"); return MIRA_E_BAD_ARG; }
    if (lk_overlap(d_h, n_l, d_g, n_t)) { set_error("h and g overlap"); return MIRA_E_BAD_ARG; }
    // r is compared on its representation like the vectors: it must be below the modulus
    uint32_t rw[8];
    memcpy(rw, r, 32);
    const uint32_t *P = field == MIRA_FIELD_FR ? FrP::P : FqP::P;
    bool below = false;
    for (int k = 7; k >= 0; k--)
        if (rw[k] != P[k]) { below = rw[k] < P[k]; break; }
    if (!below) { set_error("r is not canonical (>= the modulus)"); return MIRA_E_BAD_ARG; }
    return lookup_h_g_device(field, d_h, d_g, d_l, n_l, d_t, d_m, n_t, r);
}
// ---- deciders (decide.hip)
int mira_count_ne_device(int field, const void *d_a, const void *d_b, size_t n, uint64_t *count_out, uint64_t *first_out) {
    std::lock_guard<std::mutex> lk(g_lock);
    int rc = ensure_ctx();
    if (rc) return rc;
    if (!field_ok(field) || !count_out || (n && !d_a)) { set_error("bad count_ne arguments"); return MIRA_E_BAD_ARG; }
    if (!n) { *count_out = 0; if (first_out) *first_out = UINT64_MAX; return MIRA_OK; }
    return count_ne_device(field, d_a, d_b, n, count_out, first_out);
}
int mira_sum_sub_device(int field, const void *d_a, const void *d_b, size_t n, uint64_t out[4]) {
    std::lock_guard<std::mutex> lk(g_lock);
    int rc = ensure_ctx();
    if (rc) return rc;
    if (!field_ok(field) || !out || (n && !d_a)) { set_error("bad sum_sub arguments"); return MIRA_E_BAD_ARG; }
    if (!n) { memset(out, 0, 32); return MIRA_OK; }
    return sum_sub_device(field, d_a, d_b, n, out);
}
int mira_graph_check_compiled(uint64_t handle, const mira_eval_column *columns, uint32_t num_columns, const uint64_t *challenges, uint32_t num_challenges,
                              size_t num_rows, const void *d_expected, uint64_t *mismatch_out, uint64_t *first_row_out) {
    std::lock_guard<std::mutex> lk(g_lock);
    int rc = ensure_ctx();
    if (rc) return rc;
    if ((num_columns && !columns) || (num_challenges && !challenges) || !mismatch_out) { set_error("bad graph check arguments"); return MIRA_E_BAD_ARG; }
    int field = 0;
    if ((rc = graph_field(handle, &field))) return rc;
    if ((rc = g.decide_eval.ensure(std::max<size_t>(num_rows, 1) * 32))) return rc;
    // the evaluation itself is mira_graph_eval_compiled's, specialised kernel included; the compare re-reads it (64 B per row)
    if ((rc = graph_eval_compiled(handle, columns, num_columns, challenges, num_challenges, num_rows, g.decide_eval.p))) return rc;
    if (!num_rows) { *mismatch_out = 0; if (first_row_out) *first_row_out = UINT64_MAX; return MIRA_OK; }
    return count_ne_device(field, g.decide_eval.p, d_expected, num_rows, mismatch_out, first_row_out);
}
int mira_perm_compile(int field, const uint64_t *rows, const uint64_t *cols, const uint64_t *values, size_t nnz, size_t n, uint64_t *handle_out) {
    std::lock_guard<std::mutex> lk(g_lock);
    int rc = ensure_ctx();
    if (rc) return rc;
    if (!field_ok(field) || !handle_out || (nnz && (!rows || !cols))) { set_error("bad permutation matrix arguments"); return MIRA_E_BAD_ARG; }
    if ((uint64_t)n >= (1ull << 32) || (uint64_t)nnz >= (1ull << 32)) { set_error("permutation matrices of 2^32 rows or entries or more are not supported"); return MIRA_E_UNSUPPORTED; }
    return perm_compile(field, rows, cols, values, nnz, n, handle_out);
}
int mira_perm_check_device(uint64_t handle, const uint64_t *instance, size_t num_io, const void *d_w, size_t n_w, uint64_t *mismatch_out, uint64_t *first_out) {
    std::lock_guard<std::mutex> lk(g_lock);
    int rc = ensure_ctx();
    if (rc) return rc;
    if (!mismatch_out || (num_io && !instance) || (n_w && !d_w)) { set_error("bad permutation check arguments"); return MIRA_E_BAD_ARG; }
    return perm_check_device(handle, instance, num_io, d_w, n_w, mismatch_out, first_out);
}
int mira_perm_free(uint64_t handle) {
    std::lock_guard<std::mutex> lk(g_lock);
    int rc = ensure_ctx();
    if (rc) return rc;
    return perm_free(handle);
}
int mira_lincomb_device(int field, void *d_out, const void *const *d_vecs, const uint64_t *coeffs, size_t num_vecs, size_t n) {
    std::lock_guard<std::mutex> lk(g_lock);
    int rc = ensure_ctx();
    if (rc) return rc;
    if (!field_ok(field) || num_vecs == 0 || num_vecs > 16 || !d_vecs || !coeffs || (n && !d_out)) { set_error("bad linear-combination arguments"); return MIRA_E_BAD_ARG; }
    for (size_t k = 0; k < num_vecs; k++)
        if (n && !d_vecs[k]) { set_error("null vector"); return MIRA_E_BAD_ARG; }
    if (!n) return MIRA_OK;
    return lincomb_device(field, d_out, d_vecs, coeffs, num_vecs, n);
}
int mira_lincomb_multi_device(int field, void *const *d_outs, size_t num_outs, const void *const *d_vecs, size_t num_vecs, const uint64_t *coeffs, size_t n) {
    std::lock_guard<std::mutex> lk(g_lock);
    int rc = ensure_ctx();
    if (rc) return rc;
    if (!field_ok(field) || num_outs == 0 || num_outs > 8 || num_vecs == 0 || num_vecs > 16 || !d_outs || !d_vecs || !coeffs) {
        set_error("bad linear-combination arguments");
        return MIRA_E_BAD_ARG;
    }
    for (size_t k = 0; k < num_vecs; k++)
        if (n && !d_vecs[k]) { set_error("null vector"); return MIRA_E_BAD_ARG; }
    for (size_t m = 0; m < num_outs; m++) {
        if (n && !d_outs[m]) { set_error("null output"); return MIRA_E_BAD_ARG; }
        for (size_t q = 0; q < m; q++)
            if (n && d_outs[m] == d_outs[q]) { set_error("two outputs share one buffer"); return MIRA_E_BAD_ARG; }
        for (size_t k = 0; k < num_vecs; k++)
            if (n && d_outs[m] == d_vecs[k]) { set_error("an output aliases an input vector"); return MIRA_E_BAD_ARG; }
    }
    if (!n) return MIRA_OK;
    return lincomb_multi_device(field, d_outs, num_outs, d_vecs, num_vecs, coeffs, n);
}
int mira_pow_tree_reduce_device(int field, const void *d_leaves, size_t n_leaves, size_t leaf_point_stride, const uint64_t *weights, uint32_t num_points, uint64_t *out) {
    std::lock_guard<std::mutex> lk(g_lock);
    int rc = ensure_ctx();
    if (rc) return rc;
    if (!field_ok(field) || !d_leaves || !out || num_points == 0 || num_points > 65535 || n_leaves == 0) { set_error("bad tree-reduction arguments"); return MIRA_E_BAD_ARG; }
    if (n_leaves & (n_leaves - 1)) {
        // itertools::tree_reduce would pair nodes of different heights: `unreachable!` in the reference
        set_error("tree reduction needs a power-of-two number of leaves, got " + std::to_string(n_leaves));
        return MIRA_E_UNSUPPORTED;
    }
    uint32_t levels = 0;
    while (((size_t)1 << levels) < n_leaves) levels++;
    if (levels && !weights) { set_error("null weights"); return MIRA_E_BAD_ARG; }
    if (leaf_point_stride != 0 && leaf_point_stride < n_leaves) { set_error("leaf_point_stride shorter than the leaves"); return MIRA_E_BAD_ARG; }
    return pow_tree_reduce_device(field, d_leaves, levels, leaf_point_stride, weights, num_points, out);
}
// a cross-term graph as an entry point may be handed it: its arrays are there where it counts some, and the counts are in range
static bool graph_args_ok(int field, const mira_graph *graph, uint32_t num_columns) {
    return field_ok(field) && graph && !(graph->code_words && !graph->code) && !(graph->num_constants && !graph->constants) &&
           !(graph->num_rotations && !graph->rotations) && num_columns <= 0xFFFFFu && graph->num_rotations <= 512u;
}
int mira_graph_eval_device(int field, const mira_graph *graph, const mira_eval_column *columns, uint32_t num_columns, const uint64_t *challenges,
                           uint32_t num_challenges, size_t num_rows, void *d_out) {
    std::lock_guard<std::mutex> lk(g_lock);
    int rc = ensure_ctx();
    if (rc) return rc;
    if (!graph_args_ok(field, graph, num_columns) || (num_columns && !columns) || (num_challenges && !challenges) || (num_rows && !d_out)) {
        set_error("bad graph evaluation arguments");
        return MIRA_E_BAD_ARG;
    }
    return graph_eval_device(field, graph, columns, num_columns, challenges, num_challenges, num_rows, d_out);
}
int mira_graph_compile(int field, const mira_graph *graph, uint32_t num_challenges, uint32_t num_columns, uint64_t *handle_out) {
    std::lock_guard<std::mutex> lk(g_lock);
    int rc = ensure_ctx();
    if (rc) return rc;
    if (!graph_args_ok(field, graph, num_columns) || !handle_out) {
        set_error("bad graph compilation arguments");
        return MIRA_E_BAD_ARG;
    }
    return graph_compile(field, graph, num_challenges, num_columns, handle_out);
}
int mira_graph_eval_compiled(uint64_t handle, const mira_eval_column *columns, uint32_t num_columns, const uint64_t *challenges, uint32_t num_challenges,
                             size_t num_rows, void *d_out) {
    std::lock_guard<std::mutex> lk(g_lock);
    int rc = ensure_ctx();
    if (rc) return rc;
    if ((num_columns && !columns) || (num_challenges && !challenges) || (num_rows && !d_out)) { set_error("bad graph evaluation arguments"); return MIRA_E_BAD_ARG; }
    return graph_eval_compiled(handle, columns, num_columns, challenges, num_challenges, num_rows, d_out);
}
int mira_graph_eval_batch(const uint64_t *handles, uint32_t count, const mira_eval_column *columns, uint32_t num_columns, const uint64_t *challenges,
                          uint32_t num_challenges, size_t num_rows, void *const *d_outs) {
    std::lock_guard<std::mutex> lk(g_lock);
    int rc = ensure_ctx();
    if (rc) return rc;
    if ((count && (!handles || !d_outs)) || (num_columns && !columns) || (num_challenges && !challenges)) { set_error("bad graph evaluation arguments"); return MIRA_E_BAD_ARG; }
    return graph_eval_batch(handles, count, columns, num_columns, challenges, num_challenges, num_rows, d_outs);
}
static bool folded_args_ok(const uint64_t *handles, uint32_t num_gates, const mira_eval_column *columns, uint32_t num_columns, uint32_t num_traces,
                           const uint8_t *column_folded, const uint64_t *coeffs, const uint64_t *challenges, uint32_t num_challenges, uint32_t num_points) {
    if (num_traces < 1 || num_traces > 16) { set_error("num_traces must be 1 .. 16"); return false; }
    if (num_points < 1 || num_points > 256) { set_error("num_points must be 1 .. 256"); return false; }
    if ((num_gates && !handles) || (num_columns && (!columns || !column_folded)) || !coeffs || (num_challenges && !challenges)) {
        set_error("bad folded graph evaluation arguments");
        return false;
    }
    return true;
}
int mira_graph_eval_folded_device(const uint64_t *handles, uint32_t num_gates, const mira_eval_column *columns, uint32_t num_columns, uint32_t num_traces,
                                  const uint8_t *column_folded, const uint64_t *coeffs, const uint64_t *challenges, uint32_t num_challenges, uint32_t num_points,
                                  size_t num_rows, void *d_out) {
    std::lock_guard<std::mutex> lk(g_lock);
    int rc = ensure_ctx();
    if (rc) return rc;
    if (!folded_args_ok(handles, num_gates, columns, num_columns, num_traces, column_folded, coeffs, challenges, num_challenges, num_points)) return MIRA_E_BAD_ARG;
    if (num_rows && num_gates && !d_out) { set_error("null output"); return MIRA_E_BAD_ARG; }
    return graph_eval_folded(handles, num_gates, columns, num_columns, num_traces, column_folded, coeffs, challenges, num_challenges, num_points, num_rows, d_out, nullptr, nullptr);
}
int mira_graph_eval_folded_reduce(const uint64_t *handles, uint32_t num_gates, const mira_eval_column *columns, uint32_t num_columns, uint32_t num_traces,
                                  const uint8_t *column_folded, const uint64_t *coeffs, const uint64_t *challenges, uint32_t num_challenges, uint32_t num_points,
                                  size_t num_rows, const uint64_t *weights, uint64_t *out) {
    std::lock_guard<std::mutex> lk(g_lock);
    int rc = ensure_ctx();
    if (rc) return rc;
    if (!folded_args_ok(handles, num_gates, columns, num_columns, num_traces, column_folded, coeffs, challenges, num_challenges, num_points)) return MIRA_E_BAD_ARG;
    if (!out) { set_error("null output"); return MIRA_E_BAD_ARG; }
    static const uint64_t no_weights[4] = {0, 0, 0, 0};         // a tree of one leaf has no levels: `weights` may be null there
    const size_t leaves = (size_t)num_gates * num_rows;
    if (leaves > 1 && !weights) { set_error("null weights"); return MIRA_E_BAD_ARG; }
    return graph_eval_folded(handles, num_gates, columns, num_columns, num_traces, column_folded, coeffs, challenges, num_challenges, num_points, num_rows, nullptr,
                             weights ? weights : no_weights, out);
}
int mira_graph_free(uint64_t handle) {
    std::lock_guard<std::mutex> lk(g_lock);
    return graph_free(handle);
}
int mira_graph_specialize(const uint64_t *handles, uint32_t count, const mira_eval_column *columns, uint32_t num_columns) {
    std::unique_lock<std::mutex> lk(g_lock);
    int rc = ensure_ctx();
    if (rc) return rc;
    if ((count && !handles) || (num_columns && !columns)) { set_error("null argument"); return MIRA_E_BAD_ARG; }
    return graph_specialize(handles, count, columns, num_columns, &lk);
}
int mira_graph_is_specialized(uint64_t handle, int32_t *out) {
    std::lock_guard<std::mutex> lk(g_lock);
    return graph_is_specialized(handle, out);
}
int mira_graph_set_cache_dir(const char *dir) {
    std::lock_guard<std::mutex> lk(g_lock);
    return graph_set_cache_dir(dir);
}
int mira_graph_jit_compile_check(const char *source, size_t *code_size_out) {
    return graph_jit_compile_check(source, code_size_out);       // touches neither the device nor the library's state (rtc() is loaded once)
}
int mira_graph_jit_stats(uint32_t *compiled_out, uint32_t *from_disk_out) {
    std::lock_guard<std::mutex> lk(g_lock);
    return graph_jit_stats(compiled_out, from_disk_out);
}
int mira_graph_jit_source(uint64_t handle, const mira_eval_column *columns, uint32_t num_columns, char *buf, size_t cap, size_t *len_out) {
    std::lock_guard<std::mutex> lk(g_lock);
    if (num_columns && !columns) { set_error("null argument"); return MIRA_E_BAD_ARG; }
    return graph_jit_source(handle, columns, num_columns, buf, cap, len_out);
}
int mira_g1_mul_add(int curve, const uint64_t acc[8], const uint64_t scalar[4], const uint64_t point[8], uint64_t out[8]) {
    if (!curve_ok(curve) || !acc || !scalar || !point || !out) { set_error("bad arguments"); return MIRA_E_BAD_ARG; }
    on_curve(curve, [&](auto fb, auto fs) { g1_mul_add_t<decltype(fb), decltype(fs)>(acc, scalar, point, out); });
    return MIRA_OK;
}
int mira_g1_lincomb(int curve, const uint64_t acc[8], const uint64_t *scalars, const uint64_t *points, size_t count, uint64_t out[8]) {
    if (!curve_ok(curve) || !acc || !out || (count && (!scalars || !points)) || count > 64) { set_error("bad arguments"); return MIRA_E_BAD_ARG; }
    on_curve(curve, [&](auto fb, auto fs) { g1_lincomb_t<decltype(fb), decltype(fs)>(acc, scalars, points, count, out); });
    return MIRA_OK;
}
int mira_g1_fold_commitments(int curve, const uint64_t r[4], const uint64_t *w1, const uint64_t *w2, size_t nw, const uint64_t e[8], const uint64_t *t_commits,
                             size_t count, uint64_t *w_out, uint64_t e_out[8]) {
    if (!curve_ok(curve) || !r || !e || !e_out || (nw && (!w1 || !w2 || !w_out)) || (count && !t_commits) || nw > 64 || count > 64) {
        set_error("bad arguments");
        return MIRA_E_BAD_ARG;
    }
    on_curve(curve, [&](auto fb, auto fs) { g1_fold_commitments_t<decltype(fb), decltype(fs)>(r, w1, w2, nw, e, t_commits, count, w_out, e_out); });
    return MIRA_OK;
}
int mira_msm_download_bases(uint64_t handle, size_t first, size_t n, uint64_t *bases_out) {
    std::lock_guard<std::mutex> lk(g_lock);
    int rc = ensure_ctx();
    if (rc) return rc;
    const Bases *found = find_bases(handle);
    if (!found) return MIRA_E_BAD_ARG;
    const Bases &bs = *found;
    if (first > bs.n || n > bs.n - first || (n && !bases_out)) { set_error("range outside the registered key"); return MIRA_E_BAD_ARG; }
    if (!n) return MIRA_OK;
    if ((rc = g.scalars_stage.ensure(n * 64))) return rc;
    if ((rc = curve_ops(bs.curve).export_bases(bs, first, n, g.scalars_stage.p))) return rc;
    RT_CHECK(rt_d2h(bases_out, g.scalars_stage.p, n * 64, g.stream));
    RT_CHECK(rt_sync(g.stream));
    return MIRA_OK;
}

int mira_synth_scalars_device(int curve, size_t n, uint64_t index0, uint64_t seed, int kind, void *d_out) {
    std::lock_guard<std::mutex> lk(g_lock);
    int rc = ensure_ctx();
    if (rc) return rc;
    if (!curve_ok(curve) || (n && !d_out)) { set_error("bad synth arguments"); return MIRA_E_BAD_ARG; }
    if (!n) return MIRA_OK;
    return curve_ops(curve).synth_scalars(n, index0, seed, kind, d_out);
}
int mira_synth_bases_device(int curve, size_t n, uint64_t index0, uint64_t seed, void *d_out) {
    std::lock_guard<std::mutex> lk(g_lock);
    int rc = ensure_ctx();
    if (rc) return rc;
    if (!curve_ok(curve) || (n && !d_out)) { set_error("bad synth arguments"); return MIRA_E_BAD_ARG; }
    if (!n) return MIRA_OK;
    return curve_ops(curve).synth_bases(n, index0, seed, d_out);
}

// CommitmentKey::setup (src/commitment.rs:52-76): the derivation is stated in include/mira_gpu.h, its host side is setup.hip
static bool setup_range_ok(const void *label, size_t label_len, uint64_t first, size_t n) {
    return (label || !label_len) && first <= ((uint64_t)1 << 32) && n <= ((uint64_t)1 << 32) - first;
}
int mira_setup_bases_device(int curve, const void *label, size_t label_len, uint64_t first, size_t n, void *d_out) {
    std::lock_guard<std::mutex> lk(g_lock);
    if (!curve_ok(curve) || !setup_range_ok(label, label_len, first, n) || (n && !d_out)) { set_error("bad setup arguments"); return MIRA_E_BAD_ARG; }
    int rc = ensure_ctx();
    if (rc) return rc;
    if (!n) return MIRA_OK;
    return setup_bases_device(curve, reinterpret_cast<const unsigned char *>(label), label_len, first, n, d_out, false);
}
int mira_msm_setup_bases(int curve, uint32_t k, const void *label, size_t label_len, uint64_t *handle_out) {
    std::lock_guard<std::mutex> lk(g_lock);
    if (k >= 32) { set_error("setup: k = " + std::to_string(k) + " is not below 32"); return MIRA_E_BAD_ARG; }   // assert!(k < 32), src/commitment.rs:53
    if (!curve_ok(curve) || !handle_out || (!label && label_len)) { set_error("bad setup arguments"); return MIRA_E_BAD_ARG; }
    int rc = ensure_ctx();
    if (rc) return rc;
    Bases b; b.curve = curve; b.n = (size_t)1 << k; b.owned = true;
    if (rt_malloc(&b.d, b.n * 64) != hipSuccess || !b.d) { set_error("device allocation for bases failed"); return MIRA_E_ALLOC; }
    // straight into the resident layout: no second sweep to convert the key
    if ((rc = setup_bases_device(curve, reinterpret_cast<const unsigned char *>(label), label_len, 0, b.n, b.d, true))) { (void)rt_free(b.d); return rc; }
    *handle_out = g.next_handle++;
    g_bases[*handle_out] = b;
    return MIRA_OK;
}
int mira_hash_to_field_device(int curve, const void *d_msgs, size_t n, void *d_u) {
    std::lock_guard<std::mutex> lk(g_lock);
    if (!curve_ok(curve) || (n && (!d_msgs || !d_u)) || n > ((uint64_t)1 << 32)) { set_error("bad hash_to_field arguments"); return MIRA_E_BAD_ARG; }
    int rc = ensure_ctx();
    if (rc) return rc;
    if (!n) return MIRA_OK;
    return setup_hash_device(curve, d_msgs, n, d_u);
}
int mira_map_to_curve_device(int curve, const void *d_u, size_t n, void *d_points) {
    std::lock_guard<std::mutex> lk(g_lock);
    if (!curve_ok(curve) || (n && (!d_u || !d_points)) || n > ((uint64_t)1 << 32)) { set_error("bad map_to_curve arguments"); return MIRA_E_BAD_ARG; }
    int rc = ensure_ctx();
    if (rc) return rc;
    if (!n) return MIRA_OK;
    return setup_map_device(curve, d_u, n, d_points);
}

int mira_dev_alloc(size_t bytes, void **d_out) {
    std::lock_guard<std::mutex> lk(g_lock);
    int rc = ensure_ctx();
    if (rc) return rc;
    if (!d_out) { set_error("null output"); return MIRA_E_BAD_ARG; }
    if (rt_malloc(d_out, std::max<size_t>(bytes, 64)) != hipSuccess || !*d_out) { set_error("device allocation failed"); return MIRA_E_ALLOC; }
    return MIRA_OK;
}
int mira_dev_free(void *d) { std::lock_guard<std::mutex> lk(g_lock); if (d) (void)rt_free(d); return MIRA_OK; }
int mira_dev_upload(void *d_dst, const void *h_src, size_t bytes) {
    std::lock_guard<std::mutex> lk(g_lock);
    int rc = ensure_ctx();
    if (rc) return rc;
    RT_CHECK(rt_h2d(d_dst, h_src, bytes, g.stream));
    RT_CHECK(rt_sync(g.stream));
    return MIRA_OK;
}
int mira_dev_download(void *h_dst, const void *d_src, size_t bytes) {
    std::lock_guard<std::mutex> lk(g_lock);
    int rc = ensure_ctx();
    if (rc) return rc;
    RT_CHECK(rt_d2h(h_dst, d_src, bytes, g.stream));
    RT_CHECK(rt_sync(g.stream));
    return MIRA_OK;
}
int mira_dev_copy(void *d_dst, const void *d_src, size_t bytes) {
    std::lock_guard<std::mutex> lk(g_lock);
    int rc = ensure_ctx();
    if (rc) return rc;
    if (bytes && (!d_dst || !d_src)) { set_error("null argument"); return MIRA_E_BAD_ARG; }
    RT_CHECK(rt_d2d(d_dst, d_src, bytes, g.stream));
    RT_CHECK(rt_sync(g.stream));
    return MIRA_OK;
}
int mira_dev_sync(void) {
    std::lock_guard<std::mutex> lk(g_lock);
    int rc = ensure_ctx();
    if (rc) return rc;
    RT_CHECK(rt_sync(g.stream));
    return MIRA_OK;
}

int mira_set_timing(int enabled) { std::lock_guard<std::mutex> lk(g_lock); g.tm.enabled = enabled != 0; return MIRA_OK; }
int mira_get_timings(const char **names, float *ms, int capacity) {
    std::lock_guard<std::mutex> lk(g_lock);
    int cnt = (int)std::min(g.tm.names.size(), g.tm.ms.size());
    for (int i = 0; i < cnt && i < capacity; i++) {
        if (names) names[i] = g.tm.names[i];
        if (ms) ms[i] = g.tm.ms[i];
    }
    return cnt;
}

}   // extern "C"
