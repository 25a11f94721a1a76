// grumpkin: instantiates the MSM pipeline for this curve (coordinates Fr29 / FrP, scalars FqP).
#include "msm_host.cuh"

const CurveOps CURVE_OPS_GRUMPKIN = make_curve_ops<Fr29, FrP, FqP, MIRA_CURVE_GRUMPKIN>();
