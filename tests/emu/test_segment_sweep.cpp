// The sanitizers' view of the MSM workspaces under every minimum segment length of the sweep (tests/segment_geometry.py: SWEEP).
// A program of its own: it is compiled together with the emulation build of the library sources (-DMIRA_CPU_EMU) under
// -fsanitize=address,undefined by tests/test_segment_geometry_emu.py and speaks to them through the public C ABI only.  Synthetic
// keys and vectors (mira_synth_*) are committed at the default length first, then at every L: each point must equal the default's
// -- the values themselves are the business of the Python modules -- and every read or write beyond a workspace, the head and tail
// partials, the tail keys and the heavy-run lists sized from the upper bound of segments among them, stops the program.
// Prints one "ok L=.." line per length, then "all ok"; exit status 1 and a FAILED line otherwise.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/mira_gpu.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED %s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, mira_last_error()); failures++; } } while (0)

static const int SWEEP[] = {1, 2, 3, 5, 10, 13, 15, 16, 17, 19, 31, 32, 33, 47, 48, 49, 65};
struct Shape { int curve; size_t n; int kind, width; bool glv; int64_t pass_log; };
// dense, witness-like (kind 1: zeros and short values, heavy buckets) vectors; 5-bit windows make every bucket heavy at small L;
// the last two: the GLV split, and a commit cut into passes (the ADD instantiation of k_accumulate)
static const Shape SHAPES[] = {{0, 700, 0, 8, false, -1}, {1, 1037, 1, 8, false, -1}, {0, 900, 1, 5, false, -1}, {1, 600, 0, 9, true, -1}, {1, 1100, 1, 8, false, 14}};
static const size_t NMAX = 1100;

int main() {
    uint64_t keys[2][2] = {{0, 0}, {0, 0}};                 // [curve][glv]
    void *d_bases = nullptr, *d_sc[sizeof(SHAPES) / sizeof(SHAPES[0])] = {nullptr};
    CHECK(mira_dev_alloc(NMAX * 64, &d_bases) == MIRA_OK);
    for (int curve = 0; curve < 2; curve++) {
        CHECK(mira_synth_bases_device(curve, NMAX, 0, 0x42415345, d_bases) == MIRA_OK);
        for (int glv = 0; glv < 2; glv++) {
            CHECK(mira_msm_register_bases_device(curve, d_bases, NMAX, &keys[curve][glv]) == MIRA_OK);
            if (glv) CHECK(mira_msm_precompute_ex(keys[curve][glv], MIRA_TABLE_GLV) == MIRA_OK);
        }
    }
    const size_t ns = sizeof(SHAPES) / sizeof(SHAPES[0]);
    for (size_t s = 0; s < ns; s++) {
        CHECK(mira_dev_alloc(SHAPES[s].n * 32, &d_sc[s]) == MIRA_OK);
        CHECK(mira_synth_scalars_device(SHAPES[s].curve, SHAPES[s].n, 0, 0x5E60 + s, SHAPES[s].kind, d_sc[s]) == MIRA_OK);
    }
    if (failures) return 1;
    auto commit = [&](size_t s, int64_t L, uint64_t out[8]) {
        const Shape &sh = SHAPES[s];
        CHECK(mira_set_tuning(MIRA_TUNE_MIN_SEGMENT, L) == MIRA_OK);
        CHECK(mira_set_tuning(MIRA_TUNE_GLV, sh.glv ? -1 : 0) == MIRA_OK);
        CHECK(mira_set_tuning(MIRA_TUNE_PASS_ENTRIES_LOG, sh.pass_log) == MIRA_OK);
        CHECK(mira_msm_set_window_bits(sh.width) == MIRA_OK);
        CHECK(mira_trim(0, nullptr) == MIRA_OK);            // every workspace exactly as large as this commit asks for
        CHECK(mira_msm_device(keys[sh.curve][sh.glv ? 1 : 0], d_sc[s], sh.n, out) == MIRA_OK);
        int32_t c = 0, w = 0;
        CHECK(mira_msm_last_plan(&c, &w) == MIRA_OK && c == sh.width && (sh.glv ? c * w < 200 : c * w >= 256));
    };
    uint64_t want[sizeof(SHAPES) / sizeof(SHAPES[0])][8];
    for (size_t s = 0; s < ns; s++) commit(s, -1, want[s]);
    CHECK(mira_set_tuning(MIRA_TUNE_MIN_SEGMENT, 0) == MIRA_E_BAD_ARG);
    for (int L : SWEEP) {
        const int before = failures;
        for (size_t s = 0; s < ns; s++) {
            uint64_t got[8];
            commit(s, L, got);
            if (memcmp(got, want[s], sizeof(got)) != 0) { printf("FAILED L=%d shape %zu: the point differs from the default length's\n", L, s); failures++; }
        }
        if (failures == before) printf("ok L=%d (%zu commits)\n", L, ns);
        fflush(stdout);
    }
    mira_set_tuning(MIRA_TUNE_MIN_SEGMENT, -1); mira_set_tuning(MIRA_TUNE_GLV, -1); mira_set_tuning(MIRA_TUNE_PASS_ENTRIES_LOG, -1);
    mira_msm_set_window_bits(0);
    for (size_t s = 0; s < ns; s++) mira_dev_free(d_sc[s]);
    for (int curve = 0; curve < 2; curve++) for (int glv = 0; glv < 2; glv++) mira_msm_unregister(keys[curve][glv]);
    mira_dev_free(d_bases);
    if (failures) { printf("%d FAILED\n", failures); return 1; }
    printf("all ok\n");
    return 0;
}
