// The launches of a batch (msm_plan.hip: batch_per_launch, make_batch_plan, as msm_route.hip's route_batch forms them) for keys
// that opted into wide windows and keys that did not: one line per (pairs, commitments, cmax, path) with the widest launch's
// width and bucket counters.  tests/test_wide_windows_host.py checks that no launch holds more counters than one scan takes.
#include <cstdio>

#include "../../mira_amd/csrc/msm_plan.h"
#include "../../mira_amd/csrc/glv_consts.h"

Ctx g;
void set_error(const std::string &) {}

int main() {
    std::vector<size_t> ns;
    for (int k = 10; k <= 28; k++) ns.push_back((size_t)1 << k);
    for (int m = 3; m <= 15; m++) ns.push_back((size_t)m << 20);
    for (size_t n : ns)
        for (uint32_t count : {2u, 3u, 5u, 8u, 11u, 14u, 15u, 31u, 64u})
            for (uint32_t cmax = MSM_MAX_NARROW_C; cmax <= MSM_MAX_C; cmax++)
                for (int glv = 0; glv < 2; glv++) {
                    const size_t nv = glv ? 2 * n : n;
                    const uint32_t bits = glv ? GLV_BITS : 256, cm = glv ? MSM_MAX_NARROW_C : cmax;
                    const size_t per = batch_per_launch(nv, 0, bits, cm);
                    uint64_t worst_nb = 0;
                    uint32_t worst_c = 0;
                    for (size_t done = 0; done < count; done += per) {
                        const size_t cnt = std::min<size_t>(per, count - done);
                        const MsmPlan p = make_batch_plan(nv, 0, (uint32_t)cnt, 0, bits, cm);
                        if (p.NB > worst_nb) { worst_nb = p.NB; worst_c = p.c; }
                    }
                    printf("n=%zu count=%u cmax=%u glv=%d per=%zu c=%u counters=%llu\n", n, count, cmax, glv, per, worst_c, (unsigned long long)worst_nb);
                }
    return 0;
}
