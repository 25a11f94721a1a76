// A key's MSM tuning as bytes (mira_amd/csrc/msm_tuning.hip) on the host, on its own: no kernels, no emulation library.  Trials are
// finished under scripted timings as in test_msm_route.cpp, exported, imported into fresh keys and looked at through the route
// (msm_route.hip), which this feature leaves as it is.  The blobs the cases tamper with are built by a writer of this file's own,
// from the layout include/mira_gpu.h documents; tests/test_msm_tuning_host.py builds and runs the program, once more under
// -fsanitize=address,undefined: the reader takes bytes from disk.  Prints one "ok" line per case; exit status 1 and a FAILED line
// per failed check otherwise.
#include <cstdio>
#include <cstring>

#include "../../mira_amd/csrc/msm_route.h"
#include "../../mira_amd/csrc/msm_tuning.h"

Ctx g;
void set_error(const std::string &) {}

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

static bool copy_ready(const Bases &bs) { if (!bs.glv) bs.glv = const_cast<Bases *>(&bs); return true; }
static double scripted_us(uint32_t c) { return 1000.0 + 41.0 * ((c * 7) % 5) - 13.0 * (c % 3); }
static const char *ARCH = "emu";
static const size_t KEY_N = (size_t)1 << 20;

static Bases key(size_t n = KEY_N, int curve = MIRA_CURVE_BN256) { Bases bs; bs.curve = curve; bs.n = n; return bs; }
static void add_set(Bases &bs, uint32_t c) { bs.shared.push_back({nullptr, c, (256 + c - 1) / c}); }
static MsmRequest single(size_t n) { MsmRequest rq; rq.n = n; rq.caller_combines = true; rq.have_scalars = true; return rq; }

// ---- this file's own writer, from the documented layout -----------------------------------------------------------------------------
struct Rec { uint64_t n; uint32_t count, kind, c0, best_c; double best_us; };
struct TBlob {
    std::string magic = "MIRATUNE", arch = ARCH;
    uint32_t version = 1;
    uint64_t model = plan_model_fingerprint(), n = KEY_N;
    uint32_t curve = MIRA_CURVE_BN256, max_c = 16, table_c = 0;
    std::vector<uint32_t> sets;
    std::vector<Rec> recs;
    uint32_t stats_flag = 0, stat_kind = 0;
    uint64_t stat_n = 0;
    uint32_t hist[256] = {0};
    std::vector<unsigned char> extra;                        // bytes put in front of the checksum
};
static uint64_t t_fnv(const std::vector<unsigned char> &b, size_t len) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < len; i++) h = (h ^ b[i]) * 0x100000001b3ull;
    return h;
}
static void put(std::vector<unsigned char> &b, uint64_t v, int bytes) { for (int i = 0; i < bytes; i++) b.push_back((unsigned char)(v >> (8 * i))); }
static void reseal(std::vector<unsigned char> &b) {           // the checksum over what is in front of it now
    const uint64_t h = t_fnv(b, b.size() - 8);
    for (int i = 0; i < 8; i++) b[b.size() - 8 + i] = (unsigned char)(h >> (8 * i));
}
static std::vector<unsigned char> bytes_of(const TBlob &t) {
    std::vector<unsigned char> b(t.magic.begin(), t.magic.end());
    put(b, t.version, 4);
    put(b, t.arch.size(), 4); b.insert(b.end(), t.arch.begin(), t.arch.end());
    put(b, t.model, 8); put(b, t.curve, 4); put(b, t.n, 8); put(b, t.max_c, 4);
    put(b, t.sets.size(), 4);
    for (uint32_t c : t.sets) put(b, c, 4);
    put(b, t.table_c, 4);
    put(b, t.recs.size(), 4);
    for (const Rec &r : t.recs) {
        uint64_t us; memcpy(&us, &r.best_us, 8);
        put(b, r.n, 8); put(b, r.count, 4); put(b, r.kind, 4); put(b, r.c0, 4); put(b, r.best_c, 4); put(b, us, 8);
    }
    put(b, t.stats_flag, 4);
    if (t.stats_flag) {
        put(b, t.stat_n, 8); put(b, t.stat_kind, 4);
        for (uint32_t v : t.hist) put(b, v, 4);
    }
    b.insert(b.end(), t.extra.begin(), t.extra.end());
    put(b, 0, 8);
    reseal(b);
    return b;
}
// the blob of this key, in this file's words
static TBlob blob_for(const Bases &bs) {
    TBlob t;
    t.curve = (uint32_t)bs.curve; t.n = bs.n; t.max_c = bs.max_c; t.table_c = bs.tables ? bs.table_c : 0;
    for (const auto &s : bs.shared) t.sets.push_back(s.c);
    return t;
}
static void witness_hist(uint32_t *hist, size_t n) {         // 32-bit witness values, half of them zero
    memset(hist, 0, 1024);
    hist[0] = (uint32_t)(n / 2);
    for (int len = 2; len <= 32; len++) hist[len] = (uint32_t)((n / 2) >> (33 - len));
}

// ---- the key's state, to compare before and after --------------------------------------------------------------------------------
static bool same_trial(const Bases::WidthTrial &a, const Bases::WidthTrial &b) {
    return a.n == b.n && a.count == b.count && a.kind == b.kind && a.c0 == b.c0 && a.best_c == b.best_c && a.cur_c == b.cur_c && a.best_us == b.best_us &&
           a.cur_us == b.cur_us && a.cur_runs == b.cur_runs && a.steps == b.steps && a.done == b.done && a.stamp == b.stamp;
}
static bool same_state(const Bases &a, const Bases &b) {
    if (a.trials.size() != b.trials.size() || a.trial_stamp != b.trial_stamp || a.stat_n != b.stat_n || a.stat_kind != b.stat_kind) return false;
    for (size_t i = 0; i < a.trials.size(); i++) if (!same_trial(a.trials[i], b.trials[i])) return false;
    return memcmp(a.stat_hist, b.stat_hist, sizeof a.stat_hist) == 0;
}
static int import(const Bases &bs, const std::vector<unsigned char> &b, int32_t *accepted, std::string *err = nullptr, const char *arch = ARCH) {
    std::string e;
    *accepted = -1;
    const int rc = tuning_import(bs, arch, b.data(), b.size(), accepted, &e);
    if (err) *err = e;
    return rc;
}
static std::vector<unsigned char> exported(const Bases &bs) { std::vector<unsigned char> b; tuning_export(bs, ARCH, &b); return b; }
// a key with a running trial, a finished one and statistics: what the refusing cases must leave alone
static Bases busy_key() {
    Bases bs = key();
    const MsmRequest rq = single((size_t)1 << 14);
    for (int i = 0; i < 3; i++) { const MsmRoute r = route_commit(bs, rq, copy_ready); trial_report(*r.trial, scripted_us(r.plan.c), bs); }
    Bases::WidthTrial d;
    d.n = 5000; d.count = 2; d.kind = 0; d.c0 = d.best_c = d.cur_c = 9; d.best_us = 321.5; d.done = true; d.stamp = ++bs.trial_stamp;
    bs.trials.push_back(d);
    bs.stat_n = 3000; bs.stat_kind = 1; witness_hist(bs.stat_hist, 3000);
    return bs;
}
static void expect_refused(const char *what, const std::vector<unsigned char> &b) {
    const Bases before = busy_key();
    Bases bs = before;
    int32_t acc;
    std::string err;
    const int rc = import(bs, b, &acc, &err);
    if (rc != MIRA_E_BAD_ARG || acc != 0 || err.empty() || !same_state(bs, before)) { printf("FAILED malformed \"%s\": rc=%d accepted=%d err=\"%s\"\n", what, rc, acc, err.c_str()); failures++; }
}
static void expect_other_identity(const char *what, const std::vector<unsigned char> &b, const Bases &target, const char *arch = ARCH) {
    const Bases before = target;
    Bases bs = before;
    int32_t acc;
    const int rc = import(bs, b, &acc, nullptr, arch);
    if (rc != MIRA_OK || acc != 0 || !same_state(bs, before)) { printf("FAILED identity \"%s\": rc=%d accepted=%d\n", what, rc, acc); failures++; }
}
// drive one shape's trial to its end; returns the commits it took
static int settle(Bases &bs, const MsmRequest &rq, Bases::WidthTrial *out) {
    for (int i = 1; i <= 12; i++) {
        const MsmRoute r = route_commit(bs, rq, copy_ready);
        if (!r.trial) return -1;
        trial_report(*r.trial, scripted_us(r.plan.c), bs);
        if (r.trial->done) { *out = *r.trial; return i; }
    }
    return -1;
}

// ---- the cases ---------------------------------------------------------------------------------------------------------------------
static void finish_export_import() {
    Bases a = key();
    const MsmRequest rq = single((size_t)1 << 14);
    Bases::WidthTrial done;
    const int commits = settle(a, rq, &done);
    CHECK(commits > 1 && commits <= 12);
    const std::vector<unsigned char> blob = exported(a);
    Bases b = key();
    int32_t acc;
    CHECK(import(b, blob, &acc) == MIRA_OK && acc == 1);
    const MsmRoute r = route_commit(b, rq, copy_ready);      // the FIRST request of the fresh key
    CHECK(r.trial && r.trial->done && trial_width(*r.trial) == done.best_c && r.plan.c == done.best_c);
    CHECK(r.trial && r.trial->kind == done.kind && r.trial->c0 == done.c0 && r.trial->best_us == done.best_us && r.trial->cur_c == done.best_c);
    if (r.trial) {
        const Bases::WidthTrial before = *r.trial;
        trial_report(*r.trial, 1.0, b);                      // a finished record takes no more reports
        CHECK(same_trial(*r.trial, before));
    }
    // a key that never imported starts where the first one started
    Bases c = key();
    const MsmRoute rc = route_commit(c, rq, copy_ready);
    CHECK(rc.trial && !rc.trial->done && rc.plan.c == done.c0);
    printf("ok finish, export, import: settled at c=%u after %d commits (model %u)\n", done.best_c, commits, done.c0);
}

static void stats_slot() {
    g.tune[MIRA_TUNE_PLAN_HIST_MIN_N] = (int64_t)1 << 12;
    g.tune[MIRA_TUNE_GLV] = 0;
    const size_t n = (size_t)1 << 14;
    Bases a = key();
    a.stat_n = n; a.stat_kind = 0; witness_hist(a.stat_hist, n);
    const MsmRoute want = route_commit(a, single(n), copy_ready);          // what a key that collected them plans
    Bases fresh = key();
    const MsmRoute pending = route_commit(fresh, single(n), copy_ready);   // and one that has none
    CHECK(want.trial && want.plan.stats && !pending.trial && pending.plan.stats);
    CHECK(want.plan.c != pending.plan.c);                    // (the histogram is worth a width here: the case can tell them apart)
    Bases b = key();
    int32_t acc;
    CHECK(import(b, exported(a), &acc) == MIRA_OK && acc == 1);
    CHECK(b.stat_n == n && b.stat_kind == 0 && memcmp(b.stat_hist, a.stat_hist, 1024) == 0);
    const MsmRoute got = route_commit(b, single(n), copy_ready);
    CHECK(got.trial && got.plan.stats && got.plan.c == want.plan.c);       // not stats_pending: planned from the imported histogram
    Bases b2 = key();
    CHECK(import(b2, exported(a), &acc) == MIRA_OK && acc == 1);
    Bases fresh2 = key();
    const MsmRoute other = route_commit(b2, single((size_t)1 << 13), copy_ready), other_fresh = route_commit(fresh2, single((size_t)1 << 13), copy_ready);
    CHECK(!other.trial && other.plan.c == other_fresh.plan.c && other.plan.stats);   // another length ignores it
    g.tune[MIRA_TUNE_PLAN_HIST_MIN_N] = -1;
    g.tune[MIRA_TUNE_GLV] = -1;
    printf("ok statistics slot: c=%u with the histogram, %u without\n", want.plan.c, pending.plan.c);
}

static void round_trip() {
    Bases a = busy_key();                                    // one running trial, one finished, statistics
    const std::vector<unsigned char> first = exported(a);
    CHECK(first == exported(a));                             // deterministic
    TBlob t = blob_for(a);
    t.recs.push_back({5000, 2, 0, 9, 9, 321.5});             // the finished one alone
    t.stats_flag = 1; t.stat_n = 3000; t.stat_kind = 1; witness_hist(t.hist, 3000);
    CHECK(first == bytes_of(t));                             // the documented layout, byte for byte
    Bases b = key();
    int32_t acc;
    CHECK(import(b, first, &acc) == MIRA_OK && acc == 1 && b.trials.size() == 1);
    CHECK(exported(b) == first);
    // records come out sorted by (n, count, kind) whatever order they were learned in
    Bases c = key();
    for (const Rec &r : {Rec{9000, 1, 1, 8, 7, 10.0}, Rec{4096, 3, 0, 9, 9, 11.0}, Rec{4096, 1, 2, 9, 10, 12.0}, Rec{4096, 1, 0, 9, 8, 13.0}}) {
        Bases::WidthTrial w;
        w.n = r.n; w.count = r.count; w.kind = r.kind; w.c0 = r.c0; w.best_c = w.cur_c = r.best_c; w.best_us = r.best_us; w.done = true; w.stamp = ++c.trial_stamp;
        c.trials.push_back(w);
    }
    TBlob sorted = blob_for(c);
    sorted.recs = {{4096, 1, 0, 9, 8, 13.0}, {4096, 1, 2, 9, 10, 12.0}, {4096, 3, 0, 9, 9, 11.0}, {9000, 1, 1, 8, 7, 10.0}};
    CHECK(exported(c) == bytes_of(sorted));
    printf("ok round trip: %zu bytes\n", first.size());
}

static void batch() {
    MsmRequest rq;
    rq.n = (size_t)1 << 15; rq.count = 3; rq.stride = rq.n; rq.have_scalars = true;
    for (int glv = 0; glv < 2; glv++) {
        g.tune[MIRA_TUNE_GLV] = glv ? -1 : 0;
        Bases fresh = key();
        const BatchRoute fb = route_batch(fresh, rq, copy_ready);
        const MsmRoute fr = route_batch_launch(fresh, rq, fb, 0);
        CHECK(fb.glv == (glv == 1) && fb.per >= 3 && fr.trial && !fr.trial->done);
        const uint32_t pinned = fr.plan.c == 7 ? 8 : 7;      // a legal width the model did not pick
        TBlob t = blob_for(fresh);
        t.recs.push_back({rq.n, 3, (uint32_t)glv, fr.plan.c, pinned, 500.0});
        Bases b = key();
        int32_t acc;
        CHECK(import(b, bytes_of(t), &acc) == MIRA_OK && acc == 1);
        const BatchRoute bb = route_batch(b, rq, copy_ready);
        const MsmRoute r = route_batch_launch(b, rq, bb, 0);
        CHECK(bb.glv == fb.glv && r.trial && r.trial->done && r.plan.c == pinned && r.plan.glv == (glv == 1) && !r.trial_to_end);
    }
    // a width whose counters one scan does not take is not used: the same branch as a local trial's candidate
    g.tune[MIRA_TUNE_GLV] = 0;
    Bases wide = key((size_t)1 << 24); wide.max_c = 20;
    MsmRequest big;
    big.n = (size_t)1 << 20; big.count = 24; big.stride = big.n; big.have_scalars = true;
    Bases fresh = wide;
    const BatchRoute fb = route_batch(fresh, big, copy_ready);
    const MsmRoute fr = route_batch_launch(fresh, big, fb, 0);
    const uint32_t cnt = (uint32_t)std::min<size_t>(fb.per, big.count);
    CHECK((uint64_t)13 * cnt * (1ull << 19) > SCAN_MAX_COUNTERS && fr.plan.c != 20);
    TBlob t = blob_for(wide);
    t.recs.push_back({big.n, cnt, 0, fr.plan.c, 20, 500.0});
    int32_t acc;
    CHECK(import(wide, bytes_of(t), &acc) == MIRA_OK && acc == 1);
    const BatchRoute wb = route_batch(wide, big, copy_ready);
    const MsmRoute r = route_batch_launch(wide, big, wb, 0);
    CHECK(r.trial_to_end && r.trial_to_end->done && !r.trial && r.plan.c == fr.plan.c);
    g.tune[MIRA_TUNE_GLV] = -1;
    printf("ok batch: plain and GLV records reach the launch; 20 bits x %u commitments stay unused (c=%u)\n", cnt, r.plan.c);
}

static void set_trial() {
    Bases two = key(); add_set(two, 8); add_set(two, 11);
    const MsmRequest rq = single((size_t)1 << 14);
    Bases fresh = two;
    const MsmRoute fr = route_commit(fresh, rq, copy_ready);
    CHECK(fr.mode == MSM_SHARED_SET && fr.set && fr.trial && (fr.trial->kind & 4));
    const uint32_t model = fr.set ? fr.set->c : 8, other = model == 8 ? 11 : 8;
    TBlob t = blob_for(two);
    t.recs.push_back({rq.n, 1, 4, model, other, 400.0});
    const std::vector<unsigned char> blob = bytes_of(t);
    Bases b = two;
    int32_t acc;
    CHECK(import(b, blob, &acc) == MIRA_OK && acc == 1);
    const MsmRoute r = route_commit(b, rq, copy_ready);
    CHECK(r.mode == MSM_SHARED_SET && r.set && r.set->c == other && r.trial && r.trial->done && r.last_table_c == (int32_t)other);
    Bases one = key(); add_set(one, model);                  // lacks the set the record names
    expect_other_identity("a key lacking the set", blob, one);
    printf("ok set trial: the %u-bit set over the model's %u\n", other, model);
}

static void identity() {
    Bases target = busy_key();
    add_set(target, 9); target.tables = &target; target.table_c = 20;
    TBlob good = blob_for(target);
    good.recs.push_back({(size_t)1 << 14, 1, 0, 9, 10, 100.0});
    {   // (the unaltered blob IS accepted: every refusal below is the altered field's)
        Bases bs = target;
        int32_t acc;
        CHECK(import(bs, bytes_of(good), &acc) == MIRA_OK && acc == 1);
    }
    TBlob t = good; t.arch = "gfx942"; expect_other_identity("architecture", bytes_of(t), target);
    expect_other_identity("architecture of the importing device", bytes_of(good), target, "gfx950");
    t = good; t.model ^= (uint64_t)1 << 40; expect_other_identity("model fingerprint, one byte", bytes_of(t), target);
    t = good; t.curve = MIRA_CURVE_GRUMPKIN; expect_other_identity("curve", bytes_of(t), target);
    t = good; t.n = KEY_N * 2; expect_other_identity("key length", bytes_of(t), target);
    t = good; t.max_c = 17; expect_other_identity("max_c", bytes_of(t), target);
    t = good; t.sets = {10}; expect_other_identity("set width", bytes_of(t), target);
    t = good; t.sets = {9, 12}; expect_other_identity("one set more", bytes_of(t), target);
    t = good; t.sets.clear(); expect_other_identity("no sets", bytes_of(t), target);
    t = good; t.table_c = 22; expect_other_identity("table_c", bytes_of(t), target);
    t = good; t.table_c = 0; expect_other_identity("no tables", bytes_of(t), target);
    printf("ok identity\n");
}

static void malformed() {
    TBlob good = blob_for(key());
    good.recs = {{(size_t)1 << 14, 1, 0, 9, 10, 100.0}, {(size_t)1 << 14, 1, 1, 8, 7, 90.0}};
    good.stats_flag = 1; good.stat_n = 4096; witness_hist(good.hist, 4096);
    const std::vector<unsigned char> ok = bytes_of(good);
    {
        Bases bs = busy_key();
        int32_t acc;
        CHECK(import(bs, ok, &acc) == MIRA_OK && acc == 1);  // the blob every case below spoils
    }
    TBlob t;
    std::vector<unsigned char> b;
    t = good; t.magic = "MIRATUNX"; expect_refused("magic", bytes_of(t));
    t = good; t.version = 2; expect_refused("version", bytes_of(t));
    t = good; t.version = 0; expect_refused("version 0", bytes_of(t));
    expect_refused("empty", {});
    b = ok; b.resize(19); expect_refused("19 bytes", b);
    b = ok; b.pop_back(); expect_refused("one byte short", b);
    b = ok; b.resize(b.size() - 8); expect_refused("no checksum", b);
    b = ok; b[b.size() - 1] ^= 1; expect_refused("checksum", b);
    b = ok; b[40] ^= 4; expect_refused("a changed byte under the old checksum", b);
    b = ok; b.push_back(0); expect_refused("a byte behind the checksum", b);
    t = good; t.extra = {0, 0, 0, 0}; expect_refused("trailing bytes in front of the checksum", bytes_of(t));
    t = good; t.recs.clear(); for (uint32_t k = 0; k < 13; k++) t.recs.push_back({4096 + k, 1, 0, 9, 9, 1.0}); expect_refused("13 records", bytes_of(t));
    t = good; t.recs.push_back(t.recs[0]); expect_refused("duplicate shape", bytes_of(t));
    t = good; t.recs[0].n = 0; expect_refused("n = 0", bytes_of(t));
    t = good; t.recs[0].n = KEY_N + 1; expect_refused("n beyond the key", bytes_of(t));
    t = good; t.recs[0].count = 0; expect_refused("count = 0", bytes_of(t));
    t = good; t.recs[0].kind = 8; expect_refused("kind bit 3", bytes_of(t));
    t = good; t.recs[0].kind = 0x80000000u; expect_refused("kind bit 31", bytes_of(t));
    t = good; t.recs[0].best_c = 3; expect_refused("plain width 3", bytes_of(t));
    t = good; t.recs[0].best_c = 17; expect_refused("plain width 17 over max_c 16", bytes_of(t));
    t = good; t.recs[0].best_c = 0; expect_refused("plain width 0", bytes_of(t));
    t = good; t.recs[1].best_c = 4; expect_refused("GLV width 4", bytes_of(t));
    t = good; t.recs[1].best_c = 17; expect_refused("GLV width 17", bytes_of(t));
    t = good; t.max_c = 20; t.recs[1].best_c = 17; expect_refused("GLV width 17 under max_c 20", bytes_of(t));
    t = good; t.recs[0].kind = 4; expect_refused("set trial over a key without sets", bytes_of(t));
    t = good; t.sets = {8, 11}; t.recs[0].kind = 6; t.recs[0].best_c = 10; expect_refused("set trial width that is no set", bytes_of(t));
    t = good; t.recs[0].best_us = -1.0; expect_refused("negative wall time", bytes_of(t));
    t = good; t.recs[0].best_us = std::nan(""); expect_refused("wall time not a number", bytes_of(t));
    t = good; t.stat_kind = 2; expect_refused("stat_kind 2", bytes_of(t));
    t = good; t.stats_flag = 2; expect_refused("statistics flag 2", bytes_of(t));
    t = good; t.stat_n = 0; expect_refused("statistics of length 0", bytes_of(t));
    t = good; t.stat_n = KEY_N + 1; expect_refused("statistics beyond the key", bytes_of(t));
    t = good; t.hist[7] += 2 * 4096; expect_refused("counters beyond twice the scalars", bytes_of(t));
    t = good; t.stat_kind = 1; t.hist[7] = 4 * 4096; expect_refused("counters beyond twice the halves", bytes_of(t));
    t = good; t.hist[255] = 0xFFFFFFFFu; t.hist[254] = 0xFFFFFFFFu; expect_refused("counters that overflow 32 bits", bytes_of(t));
    t = good; t.arch.clear(); expect_refused("no architecture", bytes_of(t));
    t = good; t.arch.assign(65, 'x'); expect_refused("architecture of 65 bytes", bytes_of(t));
    b = ok; b[12] = 0xFF; b[13] = 0xFF; b[14] = 0xFF; b[15] = 0xFF; reseal(b); expect_refused("architecture length 2^32 - 1", b);
    t = good; t.sets.assign(33, 9); expect_refused("33 sets", bytes_of(t));
    {   // the widest legal sample IS taken: 2 (stat_kind + 1) stat_n
        t = good; memset(t.hist, 0, 1024); t.hist[32] = 2 * 4096;
        Bases bs = key();
        int32_t acc;
        CHECK(import(bs, bytes_of(t), &acc) == MIRA_OK && acc == 1);
        // and so is a wide width on a key that opted in, and a null blob is refused
        t = good; t.max_c = 20; t.recs[0].best_c = 20;
        Bases w = key(); w.max_c = 20;
        CHECK(import(w, bytes_of(t), &acc) == MIRA_OK && acc == 1);
        std::string err;
        CHECK(tuning_import(bs, ARCH, nullptr, 0, &acc, &err) == MIRA_E_BAD_ARG && acc == 0);
    }
    printf("ok malformed\n");
}

static bool record_valid(const Bases &bs, const Bases::WidthTrial &t) {
    std::vector<uint32_t> sets;
    for (const auto &s : bs.shared) sets.push_back(s.c);
    return t.done && t.n != 0 && t.n <= bs.n && t.count != 0 && t.kind <= 7 && t.cur_c == t.best_c && t.best_us >= 0 &&
           trial_width_possible(t.kind, t.best_c, bs.max_c, sets.data(), sets.size());
}
static void robustness() {
    Bases target = key(); add_set(target, 8); add_set(target, 11);
    TBlob good = blob_for(target);
    good.recs = {{(size_t)1 << 14, 1, 0, 9, 10, 100.0}, {(size_t)1 << 14, 1, 1, 8, 7, 90.0}, {(size_t)1 << 14, 1, 4, 8, 11, 80.0}};
    good.stats_flag = 1; good.stat_n = 4096; witness_hist(good.hist, 4096);
    const std::vector<unsigned char> ok = bytes_of(good);
    int outcome[3] = {0, 0, 0};                              // refused, not accepted, accepted
    auto offer = [&](const unsigned char *p, size_t len) {
        // (a heap copy of exactly len bytes: the sanitizer build sees a read one byte beyond it)
        std::vector<unsigned char> exact(p, p + len);
        Bases bs = target;
        int32_t acc = -1;
        std::string err;
        const int rc = tuning_import(bs, ARCH, exact.data(), exact.size(), &acc, &err);
        if (rc == MIRA_E_BAD_ARG) { CHECK(acc == 0 && same_state(bs, target)); outcome[0]++; }
        else if (rc == MIRA_OK && acc == 0) { CHECK(same_state(bs, target)); outcome[1]++; }
        else {
            CHECK(rc == MIRA_OK && acc == 1 && bs.trials.size() <= TUNING_MAX_RECORDS);
            for (const auto &t : bs.trials) CHECK(record_valid(bs, t));
            CHECK(bs.stat_n <= bs.n && (bs.stat_kind == 0 || bs.stat_kind == 1));
            outcome[2]++;
        }
    };
    for (size_t len = 0; len < ok.size(); len++) offer(ok.data(), len);                      // every truncation
    for (size_t len = 20; len < ok.size(); len++) { std::vector<unsigned char> b(ok.begin(), ok.begin() + (long)len); reseal(b); offer(b.data(), len); }   // ... resealed
    for (size_t i = 0; i < ok.size(); i++) {
        for (unsigned char mask : {(unsigned char)0xFF, (unsigned char)0x01, (unsigned char)0x80}) {
            std::vector<unsigned char> b = ok;
            b[i] ^= mask;
            offer(b.data(), b.size());                       // every single byte, under the old checksum
            if (i + 8 < ok.size()) { reseal(b); offer(b.data(), b.size()); }   // ... and under a checksum that matches: the validation itself
        }
    }
    CHECK(outcome[0] > 0 && outcome[1] > 0 && outcome[2] > 0);
    printf("ok robustness: %zu bytes; %d refused, %d of another identity, %d accepted and valid\n", ok.size(), outcome[0], outcome[1], outcome[2]);
}

static void lru() {
    Bases bs = key();
    for (uint32_t k = 0; k < 12; k++) {
        Bases::WidthTrial w;
        w.n = 10000 + k; w.count = 1; w.kind = 0; w.c0 = w.best_c = w.cur_c = 9; w.done = k % 2 == 0; w.stamp = ++bs.trial_stamp;
        bs.trials.push_back(w);
    }
    TBlob t = blob_for(bs);
    for (uint32_t k = 0; k < 12; k++) t.recs.push_back({20000 + k, 2, 1, 8, 7, 50.0 + k});
    int32_t acc;
    CHECK(import(bs, bytes_of(t), &acc) == MIRA_OK && acc == 1);
    CHECK(bs.trials.size() == 12);
    for (const auto &w : bs.trials) CHECK(w.n >= 20000 && w.done && w.best_c == 7);
    // a record of a shape the key is still measuring replaces it, and nothing else moves
    Bases run = key();
    const MsmRequest rq = single((size_t)1 << 14);
    const MsmRoute r0 = route_commit(run, rq, copy_ready);
    CHECK(r0.trial && !r0.trial->done && run.trials.size() == 1);
    TBlob one = blob_for(run);
    one.recs.push_back({rq.n, 1, r0.trial->kind, r0.trial->c0, r0.trial->c0 + 1, 77.0});
    CHECK(import(run, bytes_of(one), &acc) == MIRA_OK && acc == 1 && run.trials.size() == 1);
    const MsmRoute r1 = route_commit(run, rq, copy_ready);
    CHECK(r1.trial && r1.trial->done && r1.plan.c == one.recs[0].best_c);
    printf("ok lru\n");
}

int main() {
    finish_export_import();
    stats_slot();
    round_trip();
    batch();
    set_trial();
    identity();
    malformed();
    robustness();
    lru();
    if (failures) { printf("%d check(s) FAILED\n", failures); return 1; }
    printf("all ok\n");
    return 0;
}
