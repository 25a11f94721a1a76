// bn256: instantiates the MSM pipeline for this curve (coordinates Fq29 / FqP, scalars FrP).
#include "msm_host.cuh"

const CurveOps CURVE_OPS_BN256 = make_curve_ops<Fq29, FqP, FrP, MIRA_CURVE_BN256>();

#ifdef MSM_PROBE_STAMPS
// timing probe only (msm_kernels.cuh): the stamps of the LAST bn256 k_accumulate launch
extern "C" int mira_debug_acc_stamps(uint64_t *out, size_t n_words) {
    if (n_words > 4096 * 3) n_words = 4096 * 3;
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_acc_stamps), n_words * 8, 0, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
#endif
