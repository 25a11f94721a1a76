// The route of an MSM (msm_route.h).  The rules that single commits and batches share are written once, up front; where the two
// genuinely differ the difference is kept and named at the place.  Host code only; it runs on every commit.
#include "msm_route.h"
#include "glv_consts.h"

static constexpr size_t PLAN_HIST_MIN_N = (size_t)1 << 15;  // below this the pre-pass (one extra sync) costs more than it can save
static constexpr size_t TABLE_MIN_N = (size_t)1 << 18;   // below this an MSM is latency-bound and the per-window path is as fast
static constexpr size_t TABLE16_MIN_N = (size_t)1 << 12;

// ---- the shared rules ----------------------------------------------------------------------------------------------------------
// window width: this key's (mira_msm_set_handle_window_bits), else the process default
static int32_t forced_width(const Bases &bs) { return bs.forced_c ? bs.forced_c : g.forced_c; }
// The model's shared-bucket set.  20- / 22-bit tables pay from 2^18 pairs (2^19 buckets to reduce whatever n is); the shared-bucket
// sets have the bucket count of ONE window of the per-window path, so they win from a few thousand pairs.  A key with both uses
// the wide tables where they pay and a shared set below.  widths_free: no width is forced or asked for.
static const Bases::SharedSet *model_set(const Bases &bs, bool widths_free, size_t n, uint32_t count, bool sharded, const uint32_t *bitlen_hist) {
    return (widths_free && (sharded || n >= tuned(MIRA_TUNE_SHARED_MIN_N, TABLE16_MIN_N))) ? pick_shared(bs, n, count, sharded, bitlen_hist) : nullptr;
}
// the shape a trial record belongs to (msm_plan.h: trial_for)
static uint32_t trial_kind(bool glv, bool host_scalars, bool among_sets = false) { return (glv ? 1u : 0u) | (host_scalars ? 2u : 0u) | (among_sets ? 4u : 0u); }
// Which of the key's shared-bucket sets a submission goes through: the model's, or -- while the shape's set trial runs (msm_plan.hip:
// trial_set) -- the set it measures now.  *trial: that trial, or null.
static const Bases::SharedSet *set_under_trial(const Bases &bs, const Bases::SharedSet *model, size_t n, uint32_t count, bool host_scalars, bool may_trial,
                                               Bases::WidthTrial **trial) {
    *trial = (may_trial && bs.shared.size() > 1 && tuned(MIRA_TUNE_TABLE_WIDTH, 0) == 0) ? trial_for(bs, n, count, trial_kind(false, host_scalars, true), model->c) : nullptr;
    return *trial ? trial_set(bs, **trial, model) : model;
}
// The GLV split (glv.cuh): 2 n half-length scalars over the interleaved key, half the windows.  Windows wider than 16 bits are for
// the plain path: a key forced to one, or whose planner picked one, never splits.
static bool may_split(const Bases &bs, size_t n, int32_t forced_c) {
    return n != 0 && n < (1ull << 30) && (forced_c == 0 || forced_c <= (int32_t)MSM_MAX_NARROW_C) && glv_possible(bs);
}
// ... and the planners' estimates for the two paths decide; then the copy has to be there
static bool takes_split(const Bases &bs, const MsmPlan &plain, const MsmPlan &split, size_t pairs, GlvCopyFn copy_ready) {
    return plain.c <= MSM_MAX_NARROW_C && choose_glv(bs, plain, split, pairs) && copy_ready(bs);
}
// the plan of a launch under the width its trial measures now (statistics are not consulted: the width is given)
static MsmPlan plan_at_width(bool glv, size_t n, uint32_t c, uint32_t count, uint64_t stride) {
    return glv ? make_plan(2 * n, (int32_t)c, count, stride, nullptr, GLV_BITS) : make_plan(n, (int32_t)c, count, stride, nullptr);
}
// What comes back and what mira_msm_last_plan / mira_msm_last_table_bits report, from the plan of the mode: the only place either
// is put together.
static void settle(MsmRoute &r, MsmMode mode, uint32_t table_c) {
    const MsmPlan &p = r.plan;
    r.mode = mode; r.recorded = true; r.last_table_c = (int32_t)table_c;
    switch (mode) {
    case MSM_PER_WINDOW: r.shape = PartialShape{p.c, p.W, p.cb, p.pieces}; r.last_c = (int32_t)p.c; r.last_w = (int32_t)p.W; break;
    case MSM_SHARED_SET: r.shape = PartialShape{0, 1, p.cb, p.pieces}; r.last_c = 0; r.last_w = (int32_t)p.pieces; break;   // the pieces of ONE bucket set (P = 1: its sum)
    case MSM_WIDE_TABLE: r.shape = PartialShape{0, 64, 0, 1}; r.last_c = 0; r.last_w = 64; break;                            // 64 partial sums, combined by a plain sum
    }
}
static MsmRoute &refuse(MsmRoute &r, int rc, const char *err) { r.rc = rc; r.err = err; return r; }

// ---- a single commit, a partial ------------------------------------------------------------------------------------------------
MsmRoute route_commit(const Bases &bs, const MsmRequest &rq, GlvCopyFn copy_ready) {
    MsmRoute r;
    const size_t n = rq.n;
    const bool sharded = rq.sharded;
    const int32_t forced_c = forced_width(bs);
    const bool tables_ok = forced_c == 0 && rq.requested_c == 0;
    // fixed-base mode: window tables present, MSM large enough to be throughput-bound, no forced width
    const bool table_mode = bs.tables && tables_ok && (sharded || n >= tuned(MIRA_TUNE_TABLE_MIN_N, TABLE_MIN_N));
    // Data-dependent planning for single (unsharded) commits (ranks of a sharded MSM must agree on
    // the window width, so they keep the dense estimate).  The statistics are those of the previous
    // commit of the same length over this key -- successive fold steps commit witnesses of one
    // shape -- so no call waits for a pre-pass: this call's histogram is enqueued ahead of its MSM
    // kernels and read after the synchronisation that ends it.
    const size_t hist_min_n = tuned(MIRA_TUNE_PLAN_HIST_MIN_N, PLAN_HIST_MIN_N);
    const bool can_hist = !table_mode && !sharded && forced_c == 0 && rq.requested_c == 0 && n >= hist_min_n && rq.have_scalars;
    // statistics are consumed only by the kind of path that collected them: the halves of the GLV split have other lengths than
    // the scalars they come from
    const uint32_t *stat_any = (can_hist && bs.stat_n == n) ? bs.stat_hist : nullptr;
    const uint32_t *stat_full = bs.stat_kind == 0 ? stat_any : nullptr;
    const Bases::SharedSet *model = model_set(bs, tables_ok && !table_mode, n, 1, sharded, stat_full);
    const bool use_hist = can_hist && !model;
    // a rank of a sharded MSM that was not given a width takes 16, whatever its chunk length: partials
    // of different widths cannot be combined, and chunk lengths differ between ranks
    const int32_t width = rq.requested_c ? rq.requested_c : (sharded && forced_c == 0) ? 16 : forced_c;
    // the split: not for ranks of a sharded MSM (their partials must have one shape whatever each rank's key holds) nor beside a
    // table set
    const MsmPlan p_plain = make_plan(n, width, 1, 0, (use_hist && bs.stat_kind == 0) ? stat_any : nullptr, 256, bs.max_c);
    const bool glv_ok = !model && !table_mode && !sharded && p_plain.c <= MSM_MAX_NARROW_C && may_split(bs, n, width);
    const MsmPlan p_split = glv_ok ? make_plan(2 * n, width, 1, 0, (use_hist && bs.stat_kind == 1) ? stat_any : nullptr, GLV_BITS) : p_plain;
    const bool glv = glv_ok && takes_split(bs, p_plain, p_split, n, copy_ready);
    MsmPlan &p = r.plan;
    p = glv ? p_split : p_plain;
    // the planner's width for this shape, checked against its neighbours on the first commits of the shape (trial_*)
    // (not before the scalar statistics of the shape exist where they are collected: the model's width for a witness vector
    // without them is the dense vector's, too far from the best one for its neighbourhood to hold it)
    const bool stats_pending = use_hist && !stat_any;
    r.trial = (width == 0 && !sharded && !model && !table_mode && n && !stats_pending) ? trial_for(bs, n, 1, trial_kind(glv, rq.host_scalars), p.c) : nullptr;
    if (r.trial && trial_width(*r.trial) != p.c) p = plan_at_width(glv, n, trial_width(*r.trial), 1, 0);
    p.glv = glv; p.glv_bases = glv ? bs.glv : nullptr;
    p.stats = use_hist;
    p.windows_dst = rq.windows_dst;
    // (a commit of n W >= 2^32 entries is cut into point chunks inside the launch sequence, msm_host.cuh; the 31-bit limit is the
    // point index of a sorted entry, the sign in bit 31)
    if (n >= (1ull << 31)) return refuse(r, MIRA_E_UNSUPPORTED, "n too large for 31-bit point indices");
    if (p.W > MIRA_MAX_WINDOWS) return refuse(r, MIRA_E_UNSUPPORTED, "window configuration exceeds MIRA_MAX_WINDOWS");
    const bool own_pieces = rq.caller_combines && !rq.windows_dst;
    if (own_pieces) plan_reduction(p, default_pieces(p, MIRA_MAX_WINDOWS));
    settle(r, MSM_PER_WINDOW, 0);
    // an empty chunk (a rank beyond the prefix being committed) answers with the identity in the SHAPE its mode has for any
    // length, settled below like any other: the ranks of a sharded MSM exchange and combine partials of one shape (mira_amd/dist.py
    // checks it)
    r.empty = n == 0;
    // (refused with the per-window route on record, whatever the mode: the mode is looked at after the arguments)
    if (!r.empty && !rq.have_scalars) return refuse(r, MIRA_E_BAD_ARG, "null scalars");
    if (model) {                                             // shared buckets through the per-window launch sequence
        r.set = set_under_trial(bs, model, n, 1, rq.host_scalars, !sharded && !(can_hist && !stat_any), &r.trial);
        p = make_plan_shared(n, *r.set, bs.n);
        if (own_pieces && !r.empty) plan_reduction(p, default_pieces(p, MIRA_MAX_WINDOWS));   // (an empty answer is one identity)
        p.stats = can_hist;
        p.windows_dst = rq.windows_dst;
        settle(r, MSM_SHARED_SET, r.set->c);
    } else if (table_mode) settle(r, MSM_WIDE_TABLE, bs.table_c);
    return r;
}

// ---- a batch ---------------------------------------------------------------------------------------------------------------------
// What a batch does differently from count single commits, on purpose:
//   - it collects and consumes no bit-length statistics;
//   - it never takes the wide tables, and a forced width alone (no requested one exists) keeps it off the sets;
//   - the set pick sees min(count, 64) commitments, choose_glv the estimates of a batch of min(count, 8) and all their pairs;
//   - a trial width must fit one scan (SCAN_MAX_COUNTERS); the trial ends where it is when a candidate does not;
//   - a set trial is reported once for the whole batch, a width trial per launch.
BatchRoute route_batch(const Bases &bs, const MsmRequest &rq, GlvCopyFn copy_ready) {
    BatchRoute b;
    const size_t n = rq.n, count = rq.count;
    if (n == 0) { b.empty = true; return b; }
    if (n >= (1ull << 31)) { b.rc = MIRA_E_UNSUPPORTED; b.err = "n too large for 32-bit entry offsets"; return b; }
    // shared-bucket tables: every commitment of the batch gets ONE bucket set for its W windows
    // (ceil(256 / c) additions per pair, 2^(c-1) buckets per commitment instead of W 2^(c-1)),
    // and its partial sums come back to be added -- no chain of doublings
    b.forced_c = forced_width(bs);
    const Bases::SharedSet *model = model_set(bs, b.forced_c == 0, n, (uint32_t)std::min<size_t>(count, 64), false, nullptr);
    if (model) {
        // which of the key's sets: the model's choice, checked against the others on the first batches of the shape (trial_report_sets)
        b.set = set_under_trial(bs, model, n, (uint32_t)count, rq.h_batch != nullptr, count <= 64, &b.set_trial);
        const uint32_t Ws = (256 + b.set->c - 1) / b.set->c;
        b.per = std::max<size_t>(1, std::min<size_t>(64, (size_t)(((1ull << 32) - 1) / ((uint64_t)n * Ws))));
        return b;
    }
    if (may_split(bs, n, b.forced_c)) {                      // the planners' estimates for a batch of this shape decide (choose_glv)
        const uint32_t shape = (uint32_t)std::min<size_t>(count, 8);
        b.glv = takes_split(bs, make_batch_plan(n, b.forced_c, shape, rq.stride, 256, bs.max_c), make_plan(2 * n, b.forced_c, shape, rq.stride, nullptr, GLV_BITS), n * shape,
                            copy_ready);
    }
    b.per = b.glv ? batch_per_launch(2 * n, b.forced_c, GLV_BITS, MSM_MAX_NARROW_C) : batch_per_launch(n, b.forced_c, 256, bs.max_c);
    return b;
}
MsmRoute route_batch_launch(const Bases &bs, const MsmRequest &rq, const BatchRoute &b, size_t done) {
    MsmRoute r;
    MsmPlan &p = r.plan;
    const size_t n = rq.n;
    const uint32_t cnt = (uint32_t)std::min(b.per, rq.count - done);
    if (b.set) {
        r.set = b.set;
        p = make_plan_shared(n, *b.set, bs.n, cnt, rq.stride);
        plan_reduction(p, default_pieces(p, MIRA_MAX_WINDOWS));
        p.h_batch = rq.h_batch ? rq.h_batch + done : nullptr;
        settle(r, MSM_SHARED_SET, b.set->c);
        return r;
    }
    const uint32_t bits = b.glv ? GLV_BITS : 256;
    p = make_batch_plan(b.glv ? 2 * n : n, b.forced_c, cnt, rq.stride, bits, b.glv ? MSM_MAX_NARROW_C : bs.max_c);
    Bases::WidthTrial *trial = b.forced_c == 0 ? trial_for(bs, n, cnt, trial_kind(b.glv, rq.h_batch != nullptr), p.c) : nullptr;
    if (trial && trial_width(*trial) != p.c) {
        const uint32_t c = trial_width(*trial);
        if ((uint64_t)((bits + c - 1) / c) * cnt * (1ull << (c - 1)) <= SCAN_MAX_COUNTERS) p = plan_at_width(b.glv, n, c, cnt, rq.stride);   // (a width whose counters one scan takes)
        else r.trial_to_end = trial;                         // the candidate does not fit one scan: the walk ends where it is
    }
    if (!r.trial_to_end) r.trial = trial;
    p.glv = b.glv; p.glv_bases = b.glv ? bs.glv : nullptr;
    p.h_batch = rq.h_batch ? rq.h_batch + done : nullptr;
    plan_reduction(p, default_pieces(p, 1u << 20));
    settle(r, MSM_PER_WINDOW, 0);
    return r;
}
