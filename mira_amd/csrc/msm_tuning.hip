// A key's MSM tuning as bytes (msm_tuning.h; the layout: include/mira_gpu.h, mira_msm_tuning_export).  Host code only.  The
// reader takes bytes from a file somebody else may have written: every read is bounds-checked, the whole blob is parsed and
// validated into a value of its own, and only a valid blob of the key's identity is then installed.
#include "msm_tuning.h"

#include <cstring>

namespace {
const char MAGIC[8] = {'M', 'I', 'R', 'A', 'T', 'U', 'N', 'E'};

struct Record { uint64_t n; uint32_t count, kind, c0, best_c; double best_us; };
struct Blob {
    std::string arch;
    uint64_t model = 0, n = 0;
    uint32_t curve = 0, max_c = 0, table_c = 0;
    std::vector<uint32_t> sets;
    std::vector<Record> records;
    bool has_stats = false;
    uint64_t stat_n = 0;
    uint32_t stat_kind = 0, hist[256] = {0};
};

// ---- little-endian writer / bounds-checked reader
struct Writer {
    std::vector<unsigned char> &b;
    void bytes(const void *p, size_t len) { const unsigned char *c = static_cast<const unsigned char *>(p); b.insert(b.end(), c, c + len); }
    void u32(uint32_t v) { for (int i = 0; i < 4; i++) b.push_back((unsigned char)(v >> (8 * i))); }
    void u64(uint64_t v) { for (int i = 0; i < 8; i++) b.push_back((unsigned char)(v >> (8 * i))); }
    void f64(double v) { uint64_t bits; memcpy(&bits, &v, 8); u64(bits); }
};
struct Reader {
    const unsigned char *p;
    size_t len, at = 0;
    bool ok = true;
    bool take(size_t k) { if (!ok || k > len - at) { ok = false; return false; } return true; }
    uint32_t u32() { if (!take(4)) return 0; uint32_t v = 0; for (int i = 0; i < 4; i++) v |= (uint32_t)p[at + i] << (8 * i); at += 4; return v; }
    uint64_t u64() { if (!take(8)) return 0; uint64_t v = 0; for (int i = 0; i < 8; i++) v |= (uint64_t)p[at + i] << (8 * i); at += 8; return v; }
    double f64() { const uint64_t bits = u64(); double v; memcpy(&v, &bits, 8); return v; }
};

// The counters are a SAMPLE (msm_kernels.cuh: k_digits counts every eighth block, eight-fold; the emulation's lanes flush early and
// count fewer; the halves of the GLV split are two values per scalar), so they do not add up to the length exactly.  What no
// sample reaches is twice the values histogrammed: a ninth block of one lane makes 8 (B + 1) of 8 B + 1 scalars.
bool stat_total_possible(uint64_t total, uint64_t stat_n, uint32_t stat_kind) {
    const uint64_t per = 2 * (stat_kind + 1);
    return (total + per - 1) / per <= stat_n;
}
bool shape_less(const Record &a, const Record &b) {
    if (a.n != b.n) return a.n < b.n;
    if (a.count != b.count) return a.count < b.count;
    return a.kind < b.kind;
}

Blob blob_of(const Bases &bs, const char *arch) {
    Blob bl;
    bl.arch = arch; bl.model = plan_model_fingerprint();
    bl.curve = (uint32_t)bs.curve; bl.n = bs.n; bl.max_c = bs.max_c; bl.table_c = bs.tables ? bs.table_c : 0;
    for (const auto &set : bs.shared) bl.sets.push_back(set.c);
    for (const auto &t : bs.trials)
        if (t.done) bl.records.push_back({(uint64_t)t.n, t.count, t.kind, t.c0, t.best_c, t.best_us});
    std::sort(bl.records.begin(), bl.records.end(), shape_less);
    bl.has_stats = bs.stat_n != 0;
    if (bl.has_stats) { bl.stat_n = bs.stat_n; bl.stat_kind = (uint32_t)bs.stat_kind; memcpy(bl.hist, bs.stat_hist, sizeof bl.hist); }
    return bl;
}

void write_blob(const Blob &bl, std::vector<unsigned char> &out) {
    out.clear();
    Writer w{out};
    w.bytes(MAGIC, 8); w.u32(TUNING_VERSION);
    w.u32((uint32_t)bl.arch.size()); w.bytes(bl.arch.data(), bl.arch.size());
    w.u64(bl.model); w.u32(bl.curve); w.u64(bl.n); w.u32(bl.max_c);
    w.u32((uint32_t)bl.sets.size());
    for (uint32_t c : bl.sets) w.u32(c);
    w.u32(bl.table_c);
    w.u32((uint32_t)bl.records.size());
    for (const Record &r : bl.records) { w.u64(r.n); w.u32(r.count); w.u32(r.kind); w.u32(r.c0); w.u32(r.best_c); w.f64(r.best_us); }
    w.u32(bl.has_stats ? 1 : 0);
    if (bl.has_stats) {
        w.u64(bl.stat_n); w.u32(bl.stat_kind);
        for (uint32_t v : bl.hist) w.u32(v);
    }
    w.u64(fnv1a64(out.data(), out.size()));
}

// null: the blob is well-formed (in *bl); else what is wrong with it.  A blob is judged against the identity IT states -- the
// key length, max_c and set widths of its own header -- so the answer does not depend on the key it is offered to.
const char *parse_blob(const unsigned char *bytes, size_t len, Blob *bl) {
    if (len < 8 + 4 + 8) return "tuning blob: too short";
    if (memcmp(bytes, MAGIC, 8) != 0) return "tuning blob: bad magic";
    Reader r{bytes, len - 8};                                // (the checksum is read on its own)
    r.at = 8;
    if (r.u32() != TUNING_VERSION) return "tuning blob: unknown format version";
    Reader sum{bytes, len};
    sum.at = len - 8;
    if (sum.u64() != fnv1a64(bytes, len - 8)) return "tuning blob: checksum mismatch";
    const uint32_t arch_len = r.u32();
    if (!r.ok || arch_len == 0 || arch_len > TUNING_MAX_ARCH || !r.take(arch_len)) return "tuning blob: bad architecture string";
    bl->arch.assign(reinterpret_cast<const char *>(bytes + r.at), arch_len);
    r.at += arch_len;
    bl->model = r.u64(); bl->curve = r.u32(); bl->n = r.u64(); bl->max_c = r.u32();
    const uint32_t nsets = r.u32();
    if (!r.ok || nsets > TUNING_MAX_SETS) return "tuning blob: bad table set list";
    for (uint32_t k = 0; k < nsets; k++) bl->sets.push_back(r.u32());
    bl->table_c = r.u32();
    const uint32_t nrec = r.u32();
    if (!r.ok) return "tuning blob: truncated header";
    if (nrec > TUNING_MAX_RECORDS) return "tuning blob: more than 12 records";
    for (uint32_t k = 0; k < nrec; k++) {
        Record rec;
        rec.n = r.u64(); rec.count = r.u32(); rec.kind = r.u32(); rec.c0 = r.u32(); rec.best_c = r.u32(); rec.best_us = r.f64();
        if (!r.ok) return "tuning blob: truncated records";
        if (rec.n == 0 || rec.n > bl->n) return "tuning blob: record length outside the key";
        if (rec.count == 0) return "tuning blob: record of zero commitments";
        if (rec.kind > 7) return "tuning blob: unknown record kind";
        if (!trial_width_possible(rec.kind, rec.best_c, bl->max_c, bl->sets.data(), bl->sets.size())) return "tuning blob: width no trial of this kind can produce";
        if (!(rec.best_us >= 0.0 && rec.best_us < 1e300)) return "tuning blob: bad wall time";   // (NaN fails both)
        for (const Record &o : bl->records)
            if (o.n == rec.n && o.count == rec.count && o.kind == rec.kind) return "tuning blob: duplicate shape";
        bl->records.push_back(rec);
    }
    const uint32_t has_stats = r.u32();
    if (!r.ok || has_stats > 1) return "tuning blob: bad statistics flag";
    bl->has_stats = has_stats == 1;
    if (bl->has_stats) {
        bl->stat_n = r.u64(); bl->stat_kind = r.u32();
        uint64_t total = 0;
        for (uint32_t &v : bl->hist) { v = r.u32(); total += v; }
        if (!r.ok) return "tuning blob: truncated statistics";
        if (bl->stat_n == 0 || bl->stat_n > bl->n) return "tuning blob: statistics length outside the key";
        if (bl->stat_kind > 1) return "tuning blob: unknown statistics kind";
        if (!stat_total_possible(total, bl->stat_n, bl->stat_kind)) return "tuning blob: statistics counters sum beyond their length";
    }
    if (r.at != r.len) return "tuning blob: trailing bytes";
    return nullptr;
}
}   // namespace

void tuning_export(const Bases &bs, const char *arch, std::vector<unsigned char> *out_bytes) {
    write_blob(blob_of(bs, arch), *out_bytes);
}

int tuning_import(const Bases &bs, const char *arch, const void *bytes, size_t len, int32_t *accepted, std::string *err) {
    *accepted = 0;
    Blob bl;
    if (const char *why = bytes ? parse_blob(static_cast<const unsigned char *>(bytes), len, &bl) : "tuning blob: null") { *err = why; return MIRA_E_BAD_ARG; }
    // another device, another model, another key: a stale file costs nothing and is no error
    Blob mine = blob_of(bs, arch);
    if (bl.arch != mine.arch || bl.model != mine.model || bl.curve != mine.curve || bl.n != mine.n || bl.max_c != mine.max_c || bl.sets != mine.sets ||
        bl.table_c != mine.table_c)
        return MIRA_OK;
    for (const Record &rec : bl.records) {
        Bases::WidthTrial t;
        t.n = (size_t)rec.n; t.count = rec.count; t.kind = rec.kind; t.c0 = rec.c0; t.best_c = t.cur_c = rec.best_c; t.best_us = rec.best_us;
        t.done = true; t.stamp = ++bs.trial_stamp;
        bool replaced = false;
        for (auto &old : bs.trials)
            if (old.n == t.n && old.count == t.count && old.kind == t.kind) { old = t; replaced = true; }   // (a running one included)
        if (replaced) continue;
        if (bs.trials.size() >= TUNING_MAX_RECORDS) {         // as trial_for: the least recently used one goes
            size_t lru = 0;
            for (size_t i = 1; i < bs.trials.size(); i++) if (bs.trials[i].stamp < bs.trials[lru].stamp) lru = i;
            bs.trials.erase(bs.trials.begin() + (long)lru);
        }
        bs.trials.push_back(t);
    }
    if (bl.has_stats) {
        memcpy(bs.stat_hist, bl.hist, sizeof bs.stat_hist);
        bs.stat_n = (size_t)bl.stat_n; bs.stat_kind = (int)bl.stat_kind;
    }
    *accepted = 1;
    return MIRA_OK;
}
