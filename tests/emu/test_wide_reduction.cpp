// The device shapes of the bucket reduction (ctx.h: plan_reduction<false>) for every width, single commits and batches: prints
// one line per shape with the LDS bytes of k_set_finish (its (kappa + 2) 2^gamma node points) and of k_bucket_tree.
// tests/test_wide_windows_host.py checks them against the 160 KiB of a CU.
#include <cstdio>

#include "../../mira_amd/csrc/msm_plan.h"

Ctx g;
void set_error(const std::string &) {}

int main() {
    const size_t XYZZ = 144;
    for (uint32_t c = 4; c <= MSM_MAX_C; c++)
        for (uint32_t count : {1u, 2u, 3u, 8u, 14u}) {
            MsmPlan p = make_plan((size_t)1 << 20, (int32_t)c, count);
            if ((uint64_t)p.NB > SCAN_MAX_COUNTERS) continue;              // (a launch the batch path never forms)
            plan_reduction<false>(p, 3);
            const size_t finish = ((size_t)(p.kappa + 2) << p.gamma) * XYZZ, tree = ((size_t)2 << p.kappa) * XYZZ;
            printf("c=%u count=%u quad=%d lambda=%u kappa=%u gamma=%u set_finish=%zu bucket_tree=%zu\n", c, count, p.rquad ? 1 : 0, p.lambda, p.kappa, p.gamma,
                   finish, tree);
        }
    return 0;
}
