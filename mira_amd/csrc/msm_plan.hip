// The MSM planner (msm_plan.h): the measured cost models of the three paths -- per-window buckets, the GLV split, a key's
// shared-bucket table sets -- and the trials that check the model's choice on the first commits of a shape.  Host code
// only; it runs on every commit, so the cost loops stay free of allocations and indirect calls.
#include "msm_plan.h"
#include "glv_consts.h"

// Wall time in microseconds of one commit of 2^log_n[r] uniform scalars under width c (wall_us[r][c]).  Between rows: linear in
// log2 n; beyond the last row: proportional to n.
struct MeasuredWalls {
    int rows;
    int log_n[11];
    double wall_us[11][21];
    double interpolate(uint32_t c, double n) const {
        const double x = std::log2(std::max(n, 1.0));
        if (x <= log_n[0]) return wall_us[0][c];
        for (int r = 1; r < rows; r++)
            if (x <= log_n[r]) {
                const double t = (x - log_n[r - 1]) / (log_n[r] - log_n[r - 1]);
                return wall_us[r - 1][c] * (1.0 - t) + wall_us[r][c] * t;
            }
        return wall_us[rows - 1][c] * n / std::exp2((double)log_n[rows - 1]);
    }
};

// Estimated time of one submission in microseconds for window width c.
//
// Dense vectors: measured.  PLAN_WALLS is the wall time of one commit of uniform scalars under width c on MI355X
// (tools/plan_calibrate.py, one box, one run, profiles/r03_d_plan_calibrate.txt; boxes differ by 5 - 10 %, the ORDER of the widths
// within a row is what is used).
//
// Other vectors (witnesses: mostly zeros and short values, src/util.rs:189-193) are looked up as the
// dense vector with the same number of bucket additions: n_eff = additions(c) / W(c), from the bit
// lengths of the actual scalars (bitlen_hist, summed over the batch; null = uniform field elements).
// On top, the one effect the dense table cannot know: a bucket made heavy by the length
// distribution -- the scalars of length len share the 2^((len - 1) mod c) values their top digit can
// take, and a length that is a multiple of c always carries a 1 into the next window -- costs two
// LDS trees of general additions (5 us per level here).  A batch is count * W windows of one launch
// sequence: the additions scale, the latency does not; its W * (count - 1) * B extra counters are
// scanned at 5 800 per microsecond.
static const MeasuredWalls PLAN_WALLS = {
    10, {6, 10, 13, 15, 16, 17, 18, 19, 20, 21},   // (all rows re-measured at the END of round 4, per-window path alone -- PLAIN=1 tools/plan_calibrate.py, one box: profiles/r04_o_plan_calibrate.txt; the table of the middle of the round still had c = 8 level with 13 at 2^17, where the later tail work had moved 12 and 13 by 8 %: planned plain commits of 2^17 pairs took c = 8, 0.58 ms against 0.49)
    {
    //            c = 4     5     6     7     8     9    10    11    12    13    14    15    16
    {0, 0, 0, 0,   193,   194,   229,   233,   265,   253,   294,   317,   281,   308,   466,   396,   413},
    {0, 0, 0, 0,   276,   235,   234,   241,   222,   259,   280,   287,   336,   363,   549,   475,   495},
    {0, 0, 0, 0,   300,   298,   305,   298,   275,   265,   271,   289,   298,   340,   468,   450,   483},
    {0, 0, 0, 0,   373,   389,   420,   362,   362,   387,   352,   337,   354,   352,   493,   461,   514},
    {0, 0, 0, 0,   496,   479,   499,   551,   418,   466,   485,   424,   406,   385,   488,   483,   547},
    {0, 0, 0, 0,   780,   699,   688,   718,   569,   599,   619,   565,   493,   495,   602,   579,   609},
    {0, 0, 0, 0,  1333,  1170,  1075,  1045,   854,   865,   862,   773,   720,   698,   802,   757,   775},
    {0, 0, 0, 0,  2484,  2089,  1895,  1758,  1442,  1535,  1416,  1232,  1146,  1061,  1152,  1081,  1055},
    {0, 0, 0, 0,  4911,  4127,  3654,  3255,  2757,  2781,  2492,  2218,  1987,  1860,  1927,  1747,  1743},
    {0, 0, 0, 0,  9931,  8222,  7233,  6390,  5410,  5416,  4749,  4231,  3851,  3523,  3506,  3160,  3013},
    }};

// The GLV split (glv.cuh) has a table of its own: wall time in microseconds of one commit of 2^log_n[r] uniform pairs -- twice
// as many half-length scalars -- under width c (tools/glv_probe.py --calibrate; re-measured at the end of round 4, profiles/r04_o_plan_calibrate.txt).  The widths that cut
// 128 bits evenly stand out (9 at 2^17, 13 at 2^18 - 2^19, 16 beyond): a last window that holds only a few bits of every half is a
// handful of very heavy buckets.
static const MeasuredWalls GLV_WALLS = {
    11, {10, 12, 14, 15, 16, 17, 18, 19, 20, 21, 22},
    {
    //                c = 5      6      7      8      9     10     11     12     13     14     15     16
    {    0,     0,     0,     0,     0,   258,   231,   209,   201,   229,   222,   256,   258,   287,   383,   497,   484},
    {    0,     0,     0,     0,     0,   247,   245,   250,   225,   243,   226,   247,   273,   261,   351,   487,   491},
    {    0,     0,     0,     0,     0,   297,   312,   301,   285,   342,   305,   295,   299,   290,   364,   450,   431},
    {    0,     0,     0,     0,     0,   360,   364,   349,   319,   339,   365,   330,   306,   309,   387,   470,   487},
    {    0,     0,     0,     0,     0,   483,   451,   428,   437,   397,   473,   470,   384,   332,   403,   479,   537},
    {    0,     0,     0,     0,     0,   731,   640,   601,   589,   533,   594,   599,   496,   441,   509,   571,   623},
    {    0,     0,     0,     0,     0,  1169,  1025,   939,   877,   862,   868,   835,   693,   627,   703,   745,   759},
    {    0,     0,     0,     0,     0,  2116,  1857,  1663,  1467,  1465,  1387,  1308,  1117,  1017,  1078,  1108,  1079},
    {    0,     0,     0,     0,     0,  4043,  3548,  3177,  2803,  2799,  2505,  2297,  1998,  1807,  1829,  1841,  1741},   // (c < 9: not measured, scaled from the 2^19 row)
    {    0,     0,     0,     0,     0,  8188,  7186,  6435,  5677,  5669,  5023,  4617,  4092,  3643,  3666,  3548,  3264},   // (c < 9: not measured, scaled from the 2^19 row)
    {    0,     0,     0,     0,     0, 16300, 14305, 12810, 11300, 11285,  9870,  8977,  8082,  7357,  7152,  6959,  6222},   // (c < 9: not measured, scaled from the 2^19 row)
    }};

// Which of a key's shared-bucket sets serves a commit of n pairs (count of them in one submission).  Measured
// (tools/shared_width_probe.py, profiles/r03_d_shared_widths.txt): wall time of one commit in microseconds under width c at
// 2^12 .. 2^21 pairs, interpolated in log2 n like the per-window planner's table; beyond the last row proportional to
// n.  MIRA_TUNE_TABLE_WIDTH names a width outright (calibration, tests).
static const MeasuredWalls SHARED_WALLS = {
    6, {12, 14, 16, 17, 19, 21},
    {
    //                          c = 8     9    10    11    12    13    14    15    16      (re-measured at the end of round 4: profiles/r04_o_plan_calibrate.txt)
    {0, 0, 0, 0, 0, 0, 0, 0,   199,   216,   208,   233,   223,   212,   239,   244,   296},
    {0, 0, 0, 0, 0, 0, 0, 0,   261,   270,   283,   294,   315,   308,   278,   269,   293},
    {0, 0, 0, 0, 0, 0, 0, 0,   355,   337,   348,   381,   448,   472,   434,   368,   423},
    {0, 0, 0, 0, 0, 0, 0, 0,   520,   501,   491,   498,   564,   534,   557,   468,   497},
    {0, 0, 0, 0, 0, 0, 0, 0,  1522,  1544,  1404,  1318,  1306,  1196,  1189,  1026,  1021},
    {0, 0, 0, 0, 0, 0, 0, 0,  5978,  5853,  5072,  4661,  4298,  3998,  3751,  3341,  3243},
    }};

// additions per MSM and the heaviest bucket load of a length distribution (h[len] scalars of bit length
// len).  Integer arithmetic only: this runs 13 times per commit on the host (with exp2 / ceil on
// doubles it cost 40 us, more than the choice of width gains at 2^16 pairs).
static void plan_len_stats(uint32_t c, const double *h, double *adds_out, double *load_out) {
    double adds = 0, load = 0;
    for (uint32_t len = 1; len < 256; len++) {
        if (h[len] == 0) continue;
        adds += h[len] * (double)((len + c - 1) / c);
        load = std::max(load, h[len] / (double)(1u << ((len - 1) % c)));
        if (len % c == 0) load = std::max(load, h[len]);
    }
    *adds_out = adds; *load_out = load;
}
// lengths of UNIFORM field elements as fractions: r = 0.756 * 2^254 -> 254: 0.339, 253: 0.331, 252: 0.165, ...
static const double *plan_uniform_fractions() {
    static double f[256];
    if (f[254] == 0)
        for (int len = 0; len < 256; len++) f[len] = len > 254 ? 0.0 : len == 254 ? 0.3386 : len < 200 ? 0.0 : 0.6614 * std::exp2((double)len - 253.0);
    return f;
}
// bit lengths of a magnitude uniform below 2^126 (what the GLV table was measured on)
static const double *glv_uniform_fractions() {
    static double f[256];
    if (f[126] == 0)
        for (int len = 1; len <= 126; len++) f[len] = std::exp2((double)len - 127.0);
    return f;
}
static double plan_heavy_us(double adds, double load, uint32_t count) {
    const double seg = std::max(16.0, adds * count / (256.0 * 4 * 3 * 64));
    const double partials = load / seg;
    return partials > 6.0 ? 5.0 * (std::ceil(std::log2(partials)) + 3.0) : 0.0;
}
// The scalars of length distribution h looked up as the dense vector with as many bucket additions: returns its length n_eff,
// and in *heavy what the heavy buckets of h cost beyond those of a vector of `uniform` lengths with as many additions (the
// measured table holds the latter).  The three models call this differently; each difference changes widths, so they stay as
// they were calibrated:
//   uniform      -- the length distribution the model's table was measured on
//   W            -- 0: divide the additions by the uniform vector's additions per scalar; else by W, the windows per scalar
//   clamp        -- n_eff at least 1
//   heavy_count  -- the commits per submission the heavy-bucket estimate assumes
static double dense_equivalent(uint32_t c, const double *h, const double *uniform, uint32_t W, bool clamp, uint32_t heavy_count, double *heavy) {
    double adds, load, u_adds, u_load;
    plan_len_stats(c, h, &adds, &load);
    plan_len_stats(c, uniform, &u_adds, &u_load);
    double n_eff = W ? adds / W : adds / u_adds;
    if (clamp) n_eff = std::max(1.0, n_eff);
    *heavy = std::max(0.0, plan_heavy_us(adds, load, heavy_count) - plan_heavy_us(u_adds * n_eff, u_load * n_eff, heavy_count));
    return n_eff;
}
static double plan_cost_us(uint32_t c, double n, uint32_t count, const double *bitlen_hist /* per MSM, or null = uniform */) {
    const double W = std::ceil(256.0 / c), B = (double)(1u << (c - 1));
    double heavy = 0, n_eff = n;
    // the dense vector with as many additions: the table was measured on UNIFORM field elements, which have u_adds non-zero
    // digits each -- not W (254 bits under 15-bit windows: 17 digits in 18 windows; dividing by W made a uniform 2^22-pair
    // vector look 6 % shorter under c = 15 than the vector the table was measured on, and 15 won over the faster 16).
    // Not clamped; the heavy buckets of the whole batch.
    if (bitlen_hist) n_eff = dense_equivalent(c, bitlen_hist, plan_uniform_fractions(), 0, false, count, &heavy);
    return PLAN_WALLS.interpolate(c, n_eff * count) + heavy + W * (count - 1) * B / 5800.0;
}
// The wide windows of the plain path (17 .. 20 bits: int32 digits, the two-level front of msm_host.cuh) have a table of their own,
// measured with 15 and 16 bits beside them in one process (tools/wide_window_probe.py, uniform scalars, one box:
// profiles/r05_wide_windows.txt).  Only its RATIOS are used: make_plan scales the 16-bit wall of PLAN_WALLS by
// WIDE(c) / WIDE(16), and takes a wide width where that puts it 2 % ahead of the narrow model's best -- as choose_glv does.
static const MeasuredWalls WIDE_WALLS = {
    5, {20, 22, 24, 26, 28},
    {
    //                                                    c = 15      16      17      18      19      20
    {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,     1866,   1816,   1933,   2267,   2751,   4000},
    {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,     6374,   6023,   6011,   6453,   6672,   7180},
    {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,    23700,  22393,  22055,  22352,  21948,  21462},
    {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,    92656,  86971,  85485,  85616,  82857,  78441},
    {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,   376924, 354433, 344830, 343482, 327019, 305107},
    }};
static double wide_cost_us(uint32_t c, double n, uint32_t count, const double *bitlen_hist) {
    double heavy = 0, n_eff = n;
    if (bitlen_hist) n_eff = dense_equivalent(c, bitlen_hist, plan_uniform_fractions(), 0, false, count, &heavy);
    return WIDE_WALLS.interpolate(c, n_eff * count) + heavy + std::ceil(256.0 / c) * (count - 1) * (double)(1u << (c - 1)) / 5800.0;
}
// n halves (2 x the pairs); with the bit lengths of the previous commit's halves: the dense commit with as many bucket additions,
// plus what its heavy buckets cost beyond a uniform vector's
static double glv_cost_us(uint32_t c, double n_halves, const double *hist, uint32_t count = 1) {
    const uint32_t W = (GLV_BITS + c - 1) / c;
    double pairs = n_halves / 2, heavy = 0;
    // additions per window, at least one half; the heavy buckets of one commit
    if (hist) pairs = dense_equivalent(c, hist, glv_uniform_fractions(), W, true, 1, &heavy) / 2;
    // a batch: the commits' additions in one launch, and W 2^(c-1) more buckets to reduce per further commit (as plan_cost_us)
    return GLV_WALLS.interpolate(c, pairs * count) + heavy + (double)W * (count - 1) * (double)(1u << (c - 1)) / 5800.0;
}

MsmPlan make_plan(size_t n, int32_t forced_c, uint32_t count, uint64_t stride, const uint32_t *bitlen_hist, uint32_t bits, uint32_t cmax) {
    MsmPlan p;
    uint32_t best_c = 13;
    double best = 1e300;
    double per_msm[256];
    if (bitlen_hist)
        for (int len = 0; len < 256; len++) per_msm[len] = (double)bitlen_hist[len] / count;
    for (uint32_t c = (bits == 256 ? 4 : 5); c <= std::min<uint32_t>(cmax, MSM_MAX_NARROW_C) && !forced_c; c++) {
        const double cost = bits == 256 ? plan_cost_us(c, (double)n, count, bitlen_hist ? per_msm : nullptr)
                                        : glv_cost_us(c, (double)n, bitlen_hist ? per_msm : nullptr, count);   // the halves of the GLV split: their own table
        if (cost < best * 0.99) { best = cost; best_c = c; }    // ties go to the narrower window (fewer buckets: less that skewed data can upset)
    }
    if (!forced_c && bits == 256 && cmax > MSM_MAX_NARROW_C) {     // a key that opted into wide windows: 17 .. cmax bits from their own table
        const double *h = bitlen_hist ? per_msm : nullptr;
        const double narrow16 = plan_cost_us(MSM_MAX_NARROW_C, (double)n, count, h), wide16 = wide_cost_us(MSM_MAX_NARROW_C, (double)n, count, h);
        for (uint32_t c = MSM_MAX_NARROW_C + 1; c <= std::min<uint32_t>(cmax, MSM_MAX_C); c++) {
            const double cost = narrow16 * wide_cost_us(c, (double)n, count, h) / wide16;
            if (cost < best * 0.98) { best = cost; best_c = c; }
        }
    }
    p.c = forced_c ? (uint32_t)forced_c : best_c;
    p.est_us = forced_c ? 0.0 : best;
    p.W = (bits + p.c - 1) / p.c;
    p.B = 1u << (p.c - 1);
    p.count = count; p.stride = stride; p.Wt = p.W * count;
    p.NB = p.Wt * p.B;
    // histogram / scatter tiling: about one workgroup per CU, at least 1024 points per tile (msm_host.cuh tiles each point chunk the same way)
    uint32_t want_tiles = std::max<uint32_t>(1, MSM_HIST_WGS / p.Wt);
    p.tile = std::max<uint32_t>(1024, ceil_div(n, want_tiles));
    p.tile = (p.tile + 1023) / 1024 * 1024;
    p.ntiles = ceil_div(n, p.tile);
    // accumulate: one segment of consecutive sorted entries per resident lane (k_plan fixes the
    // segment length on the device from the number of non-zero digits); 142 VGPRs -> 3 waves/SIMD
    uint64_t entries = (uint64_t)n * p.Wt;
    p.lanes = 256u * 4u * 3u * 64u;
    p.L = (uint32_t)tuned(MIRA_TUNE_MIN_SEGMENT, 10);   // minimum segment length: more, shorter segments keep the lanes of a small commit busy (16 -> 10: 2^15 pairs 0.40 -> 0.35 ms), below 10 the cut runs cost the fix-up more than the additions gain (tools/min_segment_probe.py)
    p.T = (uint32_t)std::min<uint64_t>(p.lanes, ceil_div(entries, p.L));   // upper bound of segments
    plan_reduction(p, 1);                                    // callers that can take several pieces per window ask again
    return p;
}
// Batches (msm_route.hip: route_batch, route_batch_launch).  The number of commitments per launch comes from the plan of ONE commitment; the
// plan of a launch of cnt commitments is then made for cnt of them, and it may pick another width -- the model of a batch is the
// commit of n cnt pairs, whose rows favour wider windows.  So that its counters still fit one scan, that plan's widths are capped at
// the widest c with ceil(bits / c) cnt 2^(c-1) <= SCAN_MAX_COUNTERS (without the cap, a key that opted into wide windows planned
// 3 x 2^23 pairs at 20 bits: 20.4 M counters, a launch the scan refuses).  A forced width is not capped: per_launch is sized by it.
uint32_t scan_width_cap(uint32_t count, uint32_t bits, uint32_t cmax) {
    uint32_t c = cmax;
    while (c > 4 && (uint64_t)((bits + c - 1) / c) * count * (1ull << (c - 1)) > SCAN_MAX_COUNTERS) c--;
    return c;
}
size_t batch_per_launch(size_t n, int32_t forced_c, uint32_t bits, uint32_t cmax) {
    const MsmPlan p1 = make_plan(n, forced_c, 1, 0, nullptr, bits, cmax);
    // W_total * B counters within the scan's capacity and n * W_total entries < 2^32 (a configuration beyond the capacity, one
    // commitment per launch, is refused by the launch sequence)
    return std::max<size_t>(1, std::min<size_t>((size_t)(SCAN_MAX_COUNTERS / ((uint64_t)p1.W * p1.B)),
                                                 (size_t)(((1ull << 32) - 1) / ((uint64_t)std::max<size_t>(n, 1) * p1.W))));
}
MsmPlan make_batch_plan(size_t n, int32_t forced_c, uint32_t cnt, uint64_t stride, uint32_t bits, uint32_t cmax) {
    return make_plan(n, forced_c, cnt, stride, nullptr, bits, forced_c ? cmax : scan_width_cap(cnt, bits, cmax));
}

// Pieces per bucket set for a commit whose points the library's own epilogue combines (host_curve.hpp: horner_pieces): the device's
// Horner chain over the bits of a bucket index is cut into P parts and the host's chain of doublings, which passes every bit
// position anyway, adds P points per window instead of one (0.25 us each).
uint32_t default_pieces(const MsmPlan &p, uint32_t max_points) {
    uint32_t P = (uint32_t)tuned(MIRA_TUNE_REDUCE_PIECES, 3);
    const uint32_t sets_per_result = p.shared ? 1u : p.W;
    while (P > 1 && sets_per_result * P > max_points) P--;
    return std::max(1u, P);
}

// Shared-bucket fixed-base tables (mira_msm_precompute_ex(handle, c), c = 8 .. 16): W = ceil(256 / c) signed c-bit
// digits per scalar against the tables 2^(c w) P_i, ONE set of 2^(c-1) buckets for all windows, `sums` partial
// sums back (no chain of doublings on the host).  A commit then pays ceil(256 / c) additions per pair and the
// fix-up / bucket reduction of ONE window of 2^(c-1) buckets: narrow widths for the small commits of a fold
// step (few buckets: a short tail), 16 bits for the large ones (fewest additions).
MsmPlan make_plan_shared(size_t n, const Bases::SharedSet &set, uint64_t table_n, uint32_t count, uint64_t stride) {
    MsmPlan p = make_plan(n, (int32_t)set.c, count, stride);
    p.shared = true; p.shared_tables = set.p; p.table_n = table_n;
    p.NB = count * p.B;                                      // one bucket set per MSM
    plan_reduction(p, 1);
    return p;
}
// sharded: every rank must pick the same set whatever its chunk length -> the widest.  bitlen_hist (or null): the bit
// lengths of the scalars of the previous commit of this shape -- a witness vector (mostly zeros and short values) is looked
// up as the dense vector with as many bucket additions, as the per-window planner does (1.8 M witness scalars are 0.23 M
// dense ones under 16-bit windows: a narrow set serves them, not the 16-bit one their length suggests).
const Bases::SharedSet *pick_shared(const Bases &bs, size_t n, uint32_t count, bool sharded, const uint32_t *bitlen_hist) {
    if (bs.shared.empty()) return nullptr;
    const size_t forced = tuned(MIRA_TUNE_TABLE_WIDTH, 0);
    const Bases::SharedSet *best = nullptr;
    double best_us = 1e300, h[256];
    if (bitlen_hist)
        for (int len = 0; len < 256; len++) h[len] = (double)bitlen_hist[len];
    for (const auto &set : bs.shared) {
        if (forced) { if (set.c == forced) return &set; continue; }
        double n_eff = (double)n * count, heavy = 0;
        // the dense vector with as many additions: the table was measured on UNIFORM field elements, which have u_adds non-zero
        // digits each, not W (a 15-bit set has 18 tables for the 17 digits of a uniform scalar) -- as plan_cost_us counts -- plus what
        // the length distribution makes heavy beyond it: 32-bit witness values under 15-bit windows share TWO top-digit values, under
        // 16-bit windows all carry a one into the third window, under 13-bit windows they spread over 32.  Clamped at one scalar;
        // the heavy buckets of one commit (h is the whole batch's)
        if (bitlen_hist) n_eff = dense_equivalent(set.c, h, plan_uniform_fractions(), 0, true, 1, &heavy);
        // a batch is count bucket sets to reduce: ~1 ns per bucket of every further set (6 x 2^15 buckets: 0.19 ms of k_reduce_chunks
        // against 0.03 for one set; profiles/r03_d_batch_tables.txt)
        const double us = sharded ? -(double)set.c : SHARED_WALLS.interpolate(set.c, n_eff) + heavy + (count - 1) * (double)(1u << (set.c - 1)) / 1000.0;
        if (us < best_us) { best_us = us; best = &set; }
    }
    return best;
}

// The endomorphism copy of a key, built the first time a commit takes the GLV split (MIRA_TUNE_GLV_AUTO_MAX_LOG): the split
// halves the windows -- half the bucket reduction, half the host's chain of doublings -- for 2 x the key's memory and one
// streaming kernel.  Keys shorter than 2^12 points are not worth a copy.  A failed allocation leaves the key as it is.
static constexpr size_t GLV_AUTO_MIN_KEY = (size_t)1 << 12;
bool glv_possible(const Bases &bs) {
    if (tuned(MIRA_TUNE_GLV, 1) == 0) return false;
    if (bs.glv) return true;
    const size_t max_log = tuned(MIRA_TUNE_GLV_AUTO_MAX_LOG, 26);
    return !bs.glv_auto_failed && max_log != 0 && bs.n >= GLV_AUTO_MIN_KEY && bs.n <= ((size_t)1 << std::min<size_t>(max_log, 30));
}
// Plain path or GLV split for this commit?  With a forced width: the split wherever the key has (or may get) its copy, as
// before.  Planned: both planners are asked -- their tables are measured walls of the two paths (tools/plan_calibrate.py,
// tools/glv_probe.py --calibrate) -- and the split must be ahead by 2 %: it wins up to ~2^19 pairs (2^17: 0.49 against 0.53 ms)
// and for the batches of a fold step, and loses from 2^20 on, where the decomposition in k_digits and the doubled point
// stream cost more than the halved bucket reduction saves (profiles/r04_c_glv.txt).
bool choose_glv(const Bases &bs, const MsmPlan &plain, const MsmPlan &split, size_t pairs) {
    if (!glv_possible(bs)) return false;
    if (plain.est_us > 0 && split.est_us > 0) {
        if (split.est_us >= 0.98 * plain.est_us) return false;
    } else if (!bs.glv && pairs > ((size_t)1 << 19)) return false;     // forced width, no estimates: a copy the caller asked for is used; none is built for sizes the split loses at
    return true;
}
// ---- width trials (ctx.h: Bases::WidthTrial) ------------------------------------------------------------------------------------
static constexpr size_t TRIAL_MIN_N = (size_t)1 << 12;
static constexpr int TRIAL_RUNS = 2;
static constexpr int TRIAL_OFFSETS[5] = {0, +1, -1, +2, -2};    // the model's width, then its neighbours: the landscape has bumps (a width that leaves a two-bit top window), so all five are measured rather than walked
Bases::WidthTrial *trial_for(const Bases &bs, size_t n, uint32_t count, uint32_t kind, uint32_t c_model) {
    if (tuned(MIRA_TUNE_WIDTH_TRIALS, 1) == 0 || n * count < TRIAL_MIN_N) return nullptr;
    for (auto &t : bs.trials)
        if (t.n == n && t.count == count && t.kind == kind) { t.stamp = ++bs.trial_stamp; return &t; }
    if (bs.trials.size() >= 12) {                            // a key sees a handful of shapes; the least recently used one goes
        size_t lru = 0;
        for (size_t i = 1; i < bs.trials.size(); i++) if (bs.trials[i].stamp < bs.trials[lru].stamp) lru = i;
        bs.trials.erase(bs.trials.begin() + (long)lru);
    }
    Bases::WidthTrial t;
    t.n = n; t.count = count; t.kind = kind; t.c0 = t.best_c = t.cur_c = c_model; t.stamp = ++bs.trial_stamp;
    bs.trials.push_back(t);
    return &bs.trials.back();
}
// ... and the same among a key's shared-bucket table sets: the model (pick_shared) ranks them for dense vectors; for the witness
// vectors of a fold step it was 12 % off (14 x 2^17 scalars: the 11-bit set, 0.82 ms, where the 15-bit one takes 0.73).  A shape's first
// commits go through every set the key has, twice each, and the fastest is kept (kind bit 2 marks these records).
const Bases::SharedSet *trial_set(const Bases &bs, const Bases::WidthTrial &t, const Bases::SharedSet *model) {
    const uint32_t c = trial_width(t);
    for (const auto &set : bs.shared) if (set.c == c) return &set;
    return model;
}
// candidate k after the model's choice, 0 where there is none: a neighbour width (TRIAL_OFFSETS) within 4 .. 16 -- up to the key's
// mira_msm_set_handle_max_window_bits on the plain path -- (the halves of the GLV split from 5), or the key's k-th set unless it is the model's (that one went first)
static uint32_t trial_candidate(const Bases::WidthTrial &t, const Bases &bs, size_t k) {
    if (t.kind & 4) return bs.shared[k].c != t.c0 ? bs.shared[k].c : 0;
    const int c = (int)t.c0 + TRIAL_OFFSETS[k + 1];
    return c >= ((t.kind & 1) ? 5 : 4) && c <= (int)((t.kind & 1) ? MSM_MAX_NARROW_C : bs.max_c) ? (uint32_t)c : 0;   // (wide widths: keys that opted in, plain path)
}
void trial_report(Bases::WidthTrial &t, double us, const Bases &bs) {
    if (t.done) return;
    t.cur_us = t.cur_runs == 0 ? us : std::min(t.cur_us, us);
    if (++t.cur_runs < TRIAL_RUNS) return;
    if (t.best_us == 0 || t.cur_us < 0.98 * t.best_us) { t.best_us = t.cur_us; t.best_c = t.cur_c; }   // a candidate must be ahead by more than the noise
    const size_t candidates = (t.kind & 4) ? bs.shared.size() : 4;
    while ((size_t)t.steps < candidates)                     // steps: the candidates looked at so far
        if (const uint32_t c = trial_candidate(t, bs, (size_t)t.steps++)) { t.cur_c = c; t.cur_runs = 0; return; }
    t.done = true;
}
// ---- what a persisted record may hold (msm_tuning.hip) ---------------------------------------------------------------------------
// a width trial_candidate's rules (or the model, which plans within the same ranges) could have left in a record of this kind,
// over a key with this max_c and these shared-bucket sets
bool trial_width_possible(uint32_t kind, uint32_t c, uint32_t max_c, const uint32_t *set_widths, size_t nsets) {
    if (kind & 4) {
        for (size_t k = 0; k < nsets; k++) if (set_widths[k] == c) return true;
        return false;
    }
    return c >= ((kind & 1) ? 5u : 4u) && c <= ((kind & 1) ? MSM_MAX_NARROW_C : max_c);
}
// FNV-1a 64 over the bytes of the measured tables and the trial schedule themselves: a re-measured table or another schedule is
// another model, and what was tuned under the old one is not carried over (msm_tuning.hip keeps it in a blob's identity)
uint64_t plan_model_fingerprint() {
    uint64_t h = fnv1a64(nullptr, 0);
    auto add = [&h](const void *data, size_t len) { h = fnv1a64(data, len, h); };
    for (const MeasuredWalls *w : {&PLAN_WALLS, &GLV_WALLS, &SHARED_WALLS, &WIDE_WALLS}) {
        add(&w->rows, sizeof w->rows); add(w->log_n, sizeof w->log_n); add(w->wall_us, sizeof w->wall_us);
    }
    add(&TRIAL_RUNS, sizeof TRIAL_RUNS); add(TRIAL_OFFSETS, sizeof TRIAL_OFFSETS);
    return h;
}
