// The MSM route (mira_amd/csrc/msm_route.hip) on the host, on its own: no kernels, no emulation library.  Prints what
// route_commit / route_batch / route_batch_launch decide -- mode, plan, set, trial, shape, the numbers behind mira_msm_last_plan
// and mira_msm_last_table_bits, refusals -- over a grid of keys, lengths, counts and request flags, through the protocol around a
// GLV copy that cannot be built, and through trials under scripted timings.  tests/test_msm_route_host.py compares the output
// with tests/golden/msm_route_decisions.txt.
//
// The lines that start with '@' replay the calls of the same name in tests/msm_route_trace.py, with the key in the state the
// trace has left it in: their plan / table / shape columns must equal those of tests/golden/msm_route_trace.txt, which is how
// this file is tied to what the library did before the route had a file of its own.
#include <cstdio>

#include "../../mira_amd/csrc/msm_route.h"

Ctx g;
void set_error(const std::string &) {}

// ---- what capi.hip does around a route: the copy, the record, the trial report ----------------------------------------------------
static bool copy_builds = true;
static int copy_asked = 0;
static bool copy_ready(const Bases &bs) {
    copy_asked++;
    if (bs.glv) return true;
    if (!copy_builds) { bs.glv_auto_failed = true; return false; }
    bs.glv = const_cast<Bases *>(&bs);
    return true;
}
static struct { int32_t c = 0, w = 0, table = 0; } last;
static void record(const MsmRoute &r) { last.c = r.last_c; last.w = r.last_w; last.table = r.last_table_c; }
static const char *mode_name(MsmMode m) { return m == MSM_PER_WINDOW ? "windows" : m == MSM_SHARED_SET ? "set" : "table"; }

static void print_trial(const char *name, const Bases::WidthTrial *t) {
    if (!t) { printf(" %s=-", name); return; }
    printf(" %s=%zu/%u/%u/%u@%u%s", name, t->n, t->count, t->kind, t->c0, trial_width(*t), t->done ? "!" : "");
}
// one route: mode, the plan's c/W/count/pieces, flags (g = GLV split, s = collects statistics, h = host batch, d = sums stay on the
// device, e = empty), set, trial, shape c.W.cb.P, last c.W.table
static void print_route(const MsmRoute &r, const char *end = "\n") {
    printf(" rc=%d", r.rc);
    if (r.rc) printf(" \"%s\"", r.err);
    if (r.recorded) {
        const MsmPlan &p = r.plan;
        printf(" %s %u/%u/%u/%u %s%s%s%s%s- set=%u", mode_name(r.mode), p.c, p.W, p.count, p.pieces, p.glv ? "g" : "", p.stats ? "s" : "", p.h_batch ? "h" : "",
               p.windows_dst ? "d" : "", r.empty ? "e" : "", r.set ? r.set->c : 0);
        print_trial("trial", r.trial);
        if (r.trial_to_end) print_trial("ends", r.trial_to_end);
        printf(" shape=%u.%u.%u.%u last=%d.%d.%d", r.shape.c, r.shape.W, r.shape.cb, r.shape.P, r.last_c, r.last_w, r.last_table_c);
    }
    printf("%s", end);
}
static MsmRoute commit(const Bases &bs, const MsmRequest &rq) {
    const MsmRoute r = route_commit(bs, rq, copy_ready);
    if (r.recorded) record(r);
    return r;
}
// a batch as capi.hip runs it; us: the scripted wall time of a launch (or of the whole batch, for a set trial), by width
static const uint64_t *const H_BATCH[1] = {nullptr};
static void batch(const Bases &bs, const MsmRequest &rq, bool print, double (*us)(uint32_t) = nullptr, const char *end = "\n", bool all_launches = true) {
    const BatchRoute b = route_batch(bs, rq, copy_ready);
    if (print) {
        printf(" rc=%d", b.rc);
        if (b.rc) printf(" \"%s\"", b.err);
        printf(" %s%s- set=%u per=%zu", b.empty ? "e" : "", b.glv ? "g" : "", b.set ? b.set->c : 0, b.per);
        print_trial("set_trial", b.set_trial);
    }
    if (b.rc || b.empty) { if (print) printf("%s", end); return; }
    for (size_t done = 0; done < rq.count; done += b.per) {
        const MsmRoute r = route_batch_launch(bs, rq, b, done);
        record(r);
        if (print && (done == 0 || (all_launches && done + b.per >= rq.count))) { printf(" @%zu:", done); print_route(r, ""); }
        if (r.trial && us) trial_report(*r.trial, us(r.plan.c), bs);
        if (r.trial_to_end) r.trial_to_end->done = true;
    }
    if (b.set_trial && us) trial_report(*b.set_trial, us(b.set->c), bs);
    if (print) printf("%s", end);
}

// ---- the rows shared with the ABI trace -----------------------------------------------------------------------------------------
static const size_t N = (size_t)1 << 12;
static void shared_columns(const char *mode, const char *call, const PartialShape *shape) {
    printf("@%s %s: plan=%d,%d table=%d shape=", mode, call, last.c, last.w, last.table);
    if (shape) printf("%u,%u\n", shape->c, shape->W); else printf("-\n");
}
static void at_device(const char *mode, const char *call, const Bases &bs, size_t n, bool host) {
    MsmRequest rq;
    rq.n = n; rq.caller_combines = true; rq.have_scalars = n != 0; rq.host_scalars = host && n != 0;
    commit(bs, rq);
    shared_columns(mode, call, nullptr);
}
static void at_batch(const char *mode, const char *call, const Bases &bs, size_t n, size_t count, size_t stride, bool host) {
    MsmRequest rq;
    rq.n = n; rq.count = count; rq.stride = stride; rq.have_scalars = n != 0; rq.h_batch = host && n ? H_BATCH : nullptr;
    batch(bs, rq, false);
    shared_columns(mode, call, nullptr);
}
static void at_partial(const char *mode, const char *call, const Bases &bs, size_t first, size_t n, int32_t width, bool to_device) {
    MsmRequest rq;
    rq.first = first; rq.n = n; rq.sharded = true; rq.requested_c = width; rq.have_scalars = true; rq.windows_dst = to_device ? &g : nullptr;
    const MsmRoute r = commit(bs, rq);
    shared_columns(mode, call, &r.shape);
}
static void at_matrix(const char *mode, const Bases &bs, bool all_batches, bool set_partial, size_t n1 = 1024) {
    at_device(mode, n1 == N ? "device n=4096" : "device n=1024", bs, n1, false);
    at_device(mode, n1 == N ? "host n=4096" : "host n=1024", bs, n1, true);
    if (all_batches) at_batch(mode, "batch host n=600 count=1", bs, 600, 1, 600, true);
    at_batch(mode, "batch host n=300 count=3", bs, 300, 3, 300, true);
    if (all_batches) at_batch(mode, "batch host n=100 count=9", bs, 100, 9, 100, true);
    at_batch(mode, "batch device n=300 count=3", bs, 300, 3, 350, false);
    at_partial(mode, "partial first=100 n=1000 width=9", bs, 100, 1000, 9, false);
    at_partial(mode, "partial first=50 n=0 width=0", bs, 50, 0, 0, false);
    if (set_partial) at_partial(mode, "partial to device first=0 n=700 width=0", bs, 0, 700, 0, true);
    else at_partial(mode, "partial to device first=0 n=700 width=10", bs, 0, 700, 10, true);
}
static void at_empties(const char *mode, const Bases &bs) {
    at_device(mode, "empty device", bs, 0, false);
    at_device(mode, "empty host", bs, 0, true);
    at_batch(mode, "empty batch count=2", bs, 0, 2, 0, false);
    at_partial(mode, "empty partial first=4096 width=0", bs, N, 0, 0, false);
    at_partial(mode, "empty partial first=7 width=9", bs, 7, 0, 9, false);
    at_partial(mode, "empty partial to device first=4096 width=0", bs, N, 0, 0, true);
}
static void add_set(Bases &bs, uint32_t c) { bs.shared.push_back({nullptr, c, (256 + c - 1) / c}); bs.trials.clear(); }
static void shared_rows() {
    g.tune[MIRA_TUNE_WIDTH_TRIALS] = 0;
    Bases k0; k0.curve = MIRA_CURVE_BN256; k0.n = N;
    g.tune[MIRA_TUNE_GLV_AUTO_MAX_LOG] = 0;
    at_matrix("glv-auto-off", k0, false, false);
    at_empties("glv-auto-off", k0);
    g.tune[MIRA_TUNE_GLV_AUTO_MAX_LOG] = -1;
    g.tune[MIRA_TUNE_GLV] = 0;
    at_matrix("plain", k0, true, false);
    g.tune[MIRA_TUNE_GLV] = -1;
    at_matrix("glv-auto", k0, true, false);
    k0.forced_c = 10;
    at_matrix("handle-width-10", k0, false, false);
    at_empties("handle-width-10", k0);
    k0.forced_c = 0;
    g.forced_c = 7;
    at_matrix("process-width-7", k0, false, false);
    g.forced_c = 0;
    k0.max_c = 20;
    at_matrix("wide-opt-in", k0, false, false);
    g.tune[MIRA_TUNE_GLV] = 0;
    at_device("wide-opt-in", "plain device n=4096", k0, N, false);
    g.tune[MIRA_TUNE_GLV] = -1;
    k0.max_c = 16;

    Bases k1; k1.curve = MIRA_CURVE_GRUMPKIN; k1.n = N; k1.glv = &k1;
    at_matrix("glv-precomputed", k1, false, false);

    Bases k2; k2.curve = MIRA_CURVE_BN256; k2.n = N;
    add_set(k2, 11);
    at_matrix("one-set", k2, false, true, N);
    at_empties("one-set", k2);
    add_set(k2, 8);
    g.tune[MIRA_TUNE_SHARED_MIN_N] = 1;
    at_matrix("two-sets", k2, true, true);
    at_empties("two-sets", k2);
    g.tune[MIRA_TUNE_TABLE_WIDTH] = 11;
    at_matrix("two-sets-width-11", k2, false, true);
    g.tune[MIRA_TUNE_TABLE_WIDTH] = -1;
    at_device("trials-off", "two sets n=4096 commit 1", k2, N, false);
    at_device("trials-off", "two sets n=4096 commit 2", k2, N, false);
    g.tune[MIRA_TUNE_SHARED_MIN_N] = -1;
    Bases ko; ko.curve = MIRA_CURVE_BN256; ko.n = N;
    at_device("trials-off", "single n=4096 commit 1", ko, N, false);
    at_device("trials-off", "single n=4096 commit 2", ko, N, false);
    at_batch("trials-off", "batch n=1408 count=3 commit 1", ko, 1408, 3, 1500, false);
    at_batch("trials-off", "batch n=1408 count=3 commit 2", ko, 1408, 3, 1500, false);
    g.tune[MIRA_TUNE_WIDTH_TRIALS] = -1;

    k1.tables = &k1; k1.table_c = 20; k1.table_w = 13;
    at_empties("tables-20", k1);
    g.tune[MIRA_TUNE_TABLE_MIN_N] = 1;
    at_empties("tables-20-min-n-1", k1);
    g.tune[MIRA_TUNE_TABLE_MIN_N] = 0;
    at_empties("tables-20-min-n-0", k1);
    g.tune[MIRA_TUNE_TABLE_MIN_N] = -1;
    k2.tables = &k2; k2.table_c = 20; k2.table_w = 13;
    at_empties("tables-20-and-sets", k2);
    g.tune[MIRA_TUNE_SHARED_MIN_N] = 1;
    at_empties("tables-20-and-sets-shared-min-n-1", k2);
    g.tune[MIRA_TUNE_SHARED_MIN_N] = -1;
}

// ---- the grid ----------------------------------------------------------------------------------------------------------------------
struct KeyKind { const char *name; Bases bs; };
static std::vector<KeyKind> key_kinds() {
    std::vector<KeyKind> ks;
    auto add = [&](const char *name) -> Bases & { ks.push_back({name, Bases()}); Bases &b = ks.back().bs; b.curve = MIRA_CURVE_BN256; b.n = (size_t)1 << 28; return b; };
    add("plain").n = (size_t)1 << 24;                        // gets its copy where the split wins
    { Bases &b = add("copy"); b.glv = &b; }
    add("failed").glv_auto_failed = true;
    { Bases &b = add("sets-8-16"); add_set(b, 8); add_set(b, 16); }
    { Bases &b = add("tables-20"); b.tables = &b; b.table_c = 20; b.table_w = 13; }
    { Bases &b = add("tables-22-set-13"); b.tables = &b; b.table_c = 22; b.table_w = 12; add_set(b, 13); }
    add("width-10").forced_c = 10;
    add("wide-opt-in").max_c = 20;
    return ks;
}
static const size_t GRID_N[] = {0, 300, (size_t)1 << 12, (size_t)1 << 18, (size_t)1 << 24, (size_t)1 << 28};

// One line per (key, n) and kind of call; every call meets the key as it was registered.
static void grid() {
    for (const KeyKind &kk : key_kinds())
        for (size_t n : GRID_N) {
            if (n > kk.bs.n) continue;
            // a commit of this process: no scalars at all (refused unless empty), in device memory, in host memory
            printf("commit %s n=%zu none/device/host:", kk.name, n);
            for (int sc = 0; sc < 3; sc++) {
                Bases bs = kk.bs;
                MsmRequest rq;
                rq.n = n; rq.caller_combines = true; rq.have_scalars = sc > 0; rq.host_scalars = sc == 2;
                print_route(commit(bs, rq), sc == 2 ? "\n" : " |");
            }
            // a rank's partial: width 0 or 9, to the host or left on the device; then without scalars
            printf("partial %s n=%zu width 0,9 x dst 0,1; no scalars:", kk.name, n);
            for (int k = 0; k < 5; k++) {
                Bases bs = kk.bs;
                MsmRequest rq;
                rq.first = 5; rq.n = n > 5 ? n - 5 : n; rq.sharded = true; rq.requested_c = (k & 2) ? 9 : 0; rq.have_scalars = k < 4; rq.windows_dst = (k & 1) ? &g : nullptr;
                print_route(commit(bs, rq), k == 4 ? "\n" : " |");
            }
            if (n == 0 || n == ((size_t)1 << 28)) continue;
            printf("batch %s n=%zu count 1,2,8,14,64:", kk.name, n);
            for (size_t count : {1, 2, 8, 14, 64}) {
                Bases bs = kk.bs;
                MsmRequest rq;
                rq.n = n; rq.count = count; rq.stride = n + 3; rq.have_scalars = true; rq.h_batch = count == 8 ? H_BATCH : nullptr;   // (the batch of 8: from host memory)
                batch(bs, rq, true, nullptr, count == 64 ? "\n" : " |", false);
            }
        }
    // an empty batch; lengths nothing can run
    Bases huge; huge.curve = MIRA_CURVE_BN256; huge.n = (size_t)1 << 32;
    for (size_t n : {(size_t)0, (size_t)1 << 30, ((size_t)1 << 31) - 1, (size_t)1 << 31}) {
        MsmRequest rq;
        rq.n = n; rq.caller_combines = true; rq.have_scalars = true;
        printf("huge key n=%zu commit:", n);
        print_route(commit(huge, rq), " | batch of 2:");
        rq.count = 2; rq.stride = n;
        batch(huge, rq, true);
    }
}

// ---- the wide tables with n > 0 (the emulation cannot run them: 2^19 buckets per window) -------------------------------------------
static void wide_tables() {
    Bases bs; bs.curve = MIRA_CURVE_BN256; bs.n = N; bs.tables = &bs; bs.table_c = 20; bs.table_w = 13;
    g.tune[MIRA_TUNE_TABLE_MIN_N] = 1;
    for (int kind = 0; kind < 4; kind++) {
        MsmRequest rq;
        rq.n = 300; rq.have_scalars = true;
        if (kind < 2) { rq.caller_combines = true; rq.host_scalars = kind == 1; }
        else { rq.first = 10; rq.sharded = true; rq.windows_dst = kind == 3 ? &g : nullptr; }
        printf("tables-20 min_n=1 n=300 %s:", kind == 0 ? "device" : kind == 1 ? "host" : kind == 2 ? "partial" : "partial to device");
        print_route(commit(bs, rq));
    }
    g.tune[MIRA_TUNE_TABLE_MIN_N] = -1;
    Bases plain; plain.curve = MIRA_CURVE_BN256; plain.n = N;
    MsmRequest rq;
    rq.first = 10; rq.n = 300; rq.sharded = true; rq.have_scalars = true;
    printf("plain key sharded partial n=300 width=0:");
    print_route(commit(plain, rq));
}

// ---- statistics: collected by one commit, consumed by the next of its length and kind ----------------------------------------------
static void statistics() {
    g.tune[MIRA_TUNE_PLAN_HIST_MIN_N] = 1;
    for (int has_set = 0; has_set < 2; has_set++)
        for (int stat_kind = 0; stat_kind < 2; stat_kind++)
            for (size_t stat_n : {(size_t)0, (size_t)1 << 16, (size_t)1 << 17}) {
                Bases bs; bs.curve = MIRA_CURVE_BN256; bs.n = (size_t)1 << 20;
                if (has_set) { add_set(bs, 9); add_set(bs, 15); }
                bs.stat_n = stat_n; bs.stat_kind = stat_kind;
                for (int len = 1; len <= 32; len++) bs.stat_hist[len] = (uint32_t)(((stat_kind ? 2 : 1) * stat_n) >> (33 - len));   // 32-bit witness values
                for (int have = 0; have < 2; have++) {
                    MsmRequest rq;
                    rq.n = (size_t)1 << 16; rq.caller_combines = true; rq.have_scalars = have;
                    printf("stats sets=%d kept: n=%zu kind=%d scalars=%d:", has_set * 2, stat_n, stat_kind, have);
                    print_route(commit(bs, rq));
                }
            }
    g.tune[MIRA_TUNE_PLAN_HIST_MIN_N] = -1;
}

// ---- a copy that cannot be built -------------------------------------------------------------------------------------------------
static void failed_copy() {
    Bases bs; bs.curve = MIRA_CURVE_BN256; bs.n = (size_t)1 << 20;
    MsmRequest rq;
    rq.n = (size_t)1 << 14; rq.caller_combines = true; rq.have_scalars = true;
    copy_builds = false;
    for (int i = 0; i < 2; i++) {
        const int asked = copy_asked;
        printf("copy cannot be built, commit %d:", i + 1);
        const MsmRoute r = commit(bs, rq);
        print_route(r);
        printf("    asked for the copy %d time(s), glv_auto_failed=%d, trial records:", copy_asked - asked, (int)bs.glv_auto_failed);
        for (const auto &t : bs.trials) printf(" %zu/%u/%u", t.n, t.count, t.kind);
        printf("\n");
    }
    rq.count = 3; rq.stride = rq.n;
    Bases b2; b2.curve = MIRA_CURVE_BN256; b2.n = (size_t)1 << 20;
    for (int i = 0; i < 2; i++) {
        const int asked = copy_asked;
        printf("copy cannot be built, batch %d:", i + 1);
        batch(b2, rq, true);
        printf("    asked for the copy %d time(s), glv_auto_failed=%d, trial records:", copy_asked - asked, (int)b2.glv_auto_failed);
        for (const auto &t : b2.trials) printf(" %zu/%u/%u", t.n, t.count, t.kind);
        printf("\n");
    }
    copy_builds = true;
}

// ---- trials under scripted timings -----------------------------------------------------------------------------------------------
static double scripted_us(uint32_t c) { return 1000.0 + 41.0 * ((c * 7) % 5) - 13.0 * (c % 3); }
static void trials() {
    {
        Bases bs; bs.curve = MIRA_CURVE_BN256; bs.n = (size_t)1 << 20;
        MsmRequest rq;
        rq.n = (size_t)1 << 14; rq.caller_combines = true; rq.have_scalars = true;   // (below 2^15: no statistics to wait for)
        for (int i = 0; i < 12; i++) {
            printf("trial single commit %d:", i + 1);
            const MsmRoute r = commit(bs, rq);
            print_route(r);
            if (r.trial) trial_report(*r.trial, scripted_us(r.plan.c), bs);
        }
    }
    for (int sets = 0; sets < 2; sets++) {
        Bases bs; bs.curve = MIRA_CURVE_GRUMPKIN; bs.n = (size_t)1 << 20;
        if (sets) { add_set(bs, 8); add_set(bs, 11); add_set(bs, 15); }
        MsmRequest rq;
        rq.n = (size_t)1 << 15; rq.count = 70; rq.stride = rq.n; rq.have_scalars = true;    // (more than 64: no set trial, two launches)
        if (!sets) rq.count = 3;
        for (int i = 0; i < (sets ? 2 : 12); i++) {
            printf("trial batch sets=%d count=%zu submission %d:", sets * 3, rq.count, i + 1);
            batch(bs, rq, true, scripted_us);
        }
        if (sets) {
            rq.count = 3;
            for (int i = 0; i < 8; i++) {
                printf("trial batch sets=3 count=3 submission %d:", i + 1);
                batch(bs, rq, true, scripted_us);
            }
            MsmRequest one;
            one.n = (size_t)1 << 14; one.caller_combines = true; one.have_scalars = true; one.host_scalars = true;
            for (int i = 0; i < 8; i++) {
                printf("trial single sets=3 commit %d:", i + 1);
                const MsmRoute r = commit(bs, one);
                print_route(r);
                if (r.trial) trial_report(*r.trial, scripted_us(r.set->c), bs);
            }
        }
    }
    {   // a key that opted into wide windows: a candidate width whose counters one scan does not take ends the trial
        Bases bs; bs.curve = MIRA_CURVE_BN256; bs.n = (size_t)1 << 24; bs.max_c = 20;
        g.tune[MIRA_TUNE_GLV] = 0;
        MsmRequest rq;
        rq.n = (size_t)1 << 20; rq.count = 24; rq.stride = rq.n; rq.have_scalars = true;
        for (int i = 0; i < 6; i++) {
            printf("trial batch wide-opt-in submission %d:", i + 1);
            batch(bs, rq, true, scripted_us);
        }
        g.tune[MIRA_TUNE_GLV] = -1;
    }
}

int main() {
    shared_rows();
    grid();
    wide_tables();
    statistics();
    failed_copy();
    trials();
    return 0;
}
