// The MSM planner (mira_amd/csrc/msm_plan.hip) on the host, on its own: prints its DECISIONS over a grid of commit shapes --
// window width and windows of the plain path and of the GLV split, pieces per bucket set, plain or split, which shared-bucket
// set -- and the sequences of widths and sets the two trial machines walk under scripted timings.  tests/test_msm_plan_host.py
// compares the output with tests/golden/msm_plan_decisions.txt.  The estimates themselves are not printed: a recalibration of
// the measured tables changes that file, not this program.
#include <cmath>
#include <cstdio>

#include "../../mira_amd/csrc/msm_plan.h"
#include "../../mira_amd/csrc/glv_consts.h"

Ctx g;
void set_error(const std::string &) {}

// bit lengths of count * n scalars: 0 none (the dense model), 1 uniform (254-bit field elements, or 126-bit halves), 2 32-bit
// witness values, 3 all one bit, 4 90 % zeros
static const uint32_t *make_hist(int kind, uint32_t bits, uint64_t total, uint32_t *h) {
    memset(h, 0, 256 * 4);
    if (total > (1ull << 31)) total = 1ull << 31;
    switch (kind) {
    case 0: return nullptr;
    case 1:
        if (bits == 256) { for (int len = 200; len <= 254; len++) h[len] = (uint32_t)(total * (len == 254 ? 0.3386 : 0.6614 * std::exp2((double)len - 253.0))); }
        else { for (int len = 1; len <= 126; len++) h[len] = (uint32_t)(total * std::exp2((double)len - 127.0)); }
        break;
    case 2: for (int len = 1; len <= 32; len++) h[len] = (uint32_t)(total >> (33 - len)); break;
    case 3: h[1] = (uint32_t)total; break;
    case 4: h[0] = (uint32_t)(total - total / 10); h[bits == 256 ? 254 : 126] = (uint32_t)(total / 10); break;
    }
    return h;
}

int main() {
    std::vector<size_t> ns;
    for (int k = 0; k <= 28; k++) ns.push_back((size_t)1 << k);
    for (int k : {6, 12, 16, 18, 20, 24}) ns.push_back((size_t)3 << k);
    const uint32_t counts[] = {1, 2, 6, 8, 14, 64};
    uint32_t h[256];
    // keys: with the endomorphism copy, without one but allowed to get one, without one and not allowed (a failed build)
    Bases k_has; k_has.curve = MIRA_CURVE_BN256; k_has.n = (size_t)1 << 20; k_has.glv = &k_has;
    Bases k_may; k_may.curve = MIRA_CURVE_GRUMPKIN; k_may.n = (size_t)1 << 20;
    Bases k_fail; k_fail.curve = MIRA_CURVE_BN256; k_fail.n = (size_t)1 << 20; k_fail.glv_auto_failed = true;
    for (size_t n : ns)
        if (choose_glv(k_fail, make_plan(n, 0), make_plan(2 * n, 0, 1, 0, nullptr, GLV_BITS), n)) printf("split without a copy at n=%zu\n", n);
    // per line: n, count, width forced or not; per histogram kind (a forced width reads none): plain c/W/pieces, split
    // c/W/pieces, then choose_glv for the first two keys at n and at n * count pairs
    for (int32_t fc : {0, 12})
        for (size_t n : ns)
            for (uint32_t count : counts) {
                printf("plan n=%zu cnt=%u fc=%d", n, count, fc);
                for (int hk = 0; hk < (fc ? 1 : 5); hk++) {
                    const MsmPlan a = make_plan(n, fc, count, n, make_hist(hk, 256, (uint64_t)n * count, h));
                    const MsmPlan b = make_plan(2 * n, fc, count, n, make_hist(hk, GLV_BITS, (uint64_t)2 * n * count, h), GLV_BITS);
                    printf(" | %u/%u/%u %u/%u/%u ", a.c, a.W, default_pieces(a, MIRA_MAX_WINDOWS), b.c, b.W, default_pieces(b, MIRA_MAX_WINDOWS));
                    for (size_t pairs : {n, n * count})
                        printf("%d%d", (int)choose_glv(k_has, a, b, pairs), (int)choose_glv(k_may, a, b, pairs));
                }
                printf("\n");
            }
    // the set pick_shared takes (0 = none), per histogram kind, unsharded / sharded
    const std::vector<std::vector<uint32_t>> lists = {{}, {16}, {8, 11, 13, 15, 16}};
    for (const auto &l : lists) {
        Bases bs; bs.curve = MIRA_CURVE_BN256; bs.n = (size_t)1 << 22;
        for (uint32_t c : l) bs.shared.push_back({nullptr, c, (256 + c - 1) / c});
        for (int forced : {-1, 13, 11}) {                    // MIRA_TUNE_TABLE_WIDTH names the set (or none): one length shows it
            g.tune[MIRA_TUNE_TABLE_WIDTH] = forced;
            for (size_t n : ns) {
                if ((forced >= 0 || l.empty()) && n != ((size_t)1 << 16)) continue;
                printf("shared sets=%zu forced=%d n=%zu:", l.size(), forced, n);
                for (uint32_t count : counts) {
                    printf(" ");
                    for (int hk = 0; hk < 5; hk++)
                        for (int sharded = 0; sharded < 2; sharded++) {
                            const Bases::SharedSet *s = pick_shared(bs, n, count, sharded, make_hist(hk, 256, (uint64_t)n * count, h));
                            printf("%s%u", hk || sharded ? "," : "", s ? s->c : 0);
                        }
                }
                printf("\n");
            }
        }
    }
    g.tune[MIRA_TUNE_TABLE_WIDTH] = -1;
    // width trials: the widths a shape's first commits run under, and the width kept
    for (uint32_t kind : {0u, 1u})
        for (uint32_t c0 : {4u, 5u, 6u, 12u, 13u, 15u, 16u}) {
            Bases bs; bs.curve = MIRA_CURVE_BN256; bs.n = (size_t)1 << 20;
            Bases::WidthTrial *t = trial_for(bs, 1 << 16, 1, kind, c0);
            printf("width trial kind=%u model=%u:", kind, c0);
            for (int i = 0; i < 16 && !t->done; i++) {
                const uint32_t c = trial_width(*t);
                printf(" %u", c);
                trial_report(*t, 1000.0 + 37.0 * ((c * 7 + i * 3) % 5) - 9.0 * (c == c0 + 2) + (i % 3) * 4.5, bs);
            }
            printf(" -> %u\n", trial_width(*t));
        }
    // set trials: the sets a shape's first commits go through, and the set kept
    for (const auto &l : lists)
        for (size_t first = 0; first < l.size(); first++) {
            Bases bs; bs.curve = MIRA_CURVE_BN256; bs.n = (size_t)1 << 20;
            for (uint32_t c : l) bs.shared.push_back({nullptr, c, (256 + c - 1) / c});
            const Bases::SharedSet *model = &bs.shared[first];
            Bases::WidthTrial *t = trial_for(bs, 1 << 15, 3, 4u, model->c);
            printf("set trial sets=%zu model=%u:", l.size(), model->c);
            for (int i = 0; i < 16 && t && !t->done; i++) {
                const Bases::SharedSet *s = trial_set(bs, *t, model);
                printf(" %u", s->c);
                trial_report(*t, 500.0 + 23.0 * ((s->c * 5 + i) % 7) - 3.0 * i, bs);
            }
            printf(" -> %u\n", t ? trial_set(bs, *t, model)->c : model->c);
        }
    // trial records: a key keeps the 12 most recently used shapes; no trials below 2^12 scalars or with the knob at 0
    {
        Bases bs; bs.curve = MIRA_CURVE_BN256; bs.n = (size_t)1 << 20;
        for (int i = 0; i < 20; i++) trial_for(bs, (size_t)1 << (12 + i % 14), 1, 0, 10 + i % 5);
        trial_for(bs, (size_t)1 << 13, 1, 0, 13);
        printf("trial records:");
        for (const auto &t : bs.trials) printf(" %zu/%u", t.n, t.c0);
        printf("\n");
        g.tune[MIRA_TUNE_WIDTH_TRIALS] = 0;
        const bool off = trial_for(bs, 1 << 20, 1, 0, 13) == nullptr;
        g.tune[MIRA_TUNE_WIDTH_TRIALS] = -1;
        printf("no trial: knob off %d, 2 x 2^10 scalars %d\n", (int)off, (int)(trial_for(bs, 1 << 10, 2, 0, 13) == nullptr));
    }
    return 0;
}
