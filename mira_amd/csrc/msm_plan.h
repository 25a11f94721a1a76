// The MSM planner (msm_plan.hip): window width, GLV split or not, which shared-bucket set, and the width / set trials.  Host
// code only: it reads the tuning knobs and the key's records, allocates nothing on the device and launches nothing.  What a
// commit, a partial or a batch does with these answers -- its route -- is decided one level up, in msm_route.h.
#pragma once
#include "ctx.h"

// the plan of one launch sequence over n scalars of `bits` bits (256, or GLV_BITS for the halves of the GLV split); forced_c != 0
// names the width, else the measured cost model picks it -- from bitlen_hist (the bit lengths of the count * n scalars of the
// previous commit of this shape) when given
// cmax (17 .. 20, plain path only): the key opted into wide windows (mira_msm_set_handle_max_window_bits); the model then takes
// one where its measured table puts it at least 2 % ahead
MsmPlan make_plan(size_t n, int32_t forced_c, uint32_t count = 1, uint64_t stride = 0, const uint32_t *bitlen_hist = nullptr, uint32_t bits = 256,
                  uint32_t cmax = MSM_MAX_NARROW_C);
// ... over one of a key's shared-bucket table sets
MsmPlan make_plan_shared(size_t n, const Bases::SharedSet &set, uint64_t table_n, uint32_t count = 1, uint64_t stride = 0);
// a batch of MSMs over n `bits`-bit scalars (n: the columns of one commitment's digit matrix): commitments per launch, and the plan of a
// launch of cnt of them -- a planned width never puts more than SCAN_MAX_COUNTERS bucket counters into one launch (scan_width_cap)
uint32_t scan_width_cap(uint32_t count, uint32_t bits, uint32_t cmax);
size_t batch_per_launch(size_t n, int32_t forced_c, uint32_t bits, uint32_t cmax);
MsmPlan make_batch_plan(size_t n, int32_t forced_c, uint32_t cnt, uint64_t stride, uint32_t bits, uint32_t cmax);
// pieces per bucket set when at most max_points points may come back per commitment
uint32_t default_pieces(const MsmPlan &p, uint32_t max_points);
// the key's shared-bucket set for a commit of n pairs (count of them in one submission), or null when the key has none
const Bases::SharedSet *pick_shared(const Bases &bs, size_t n, uint32_t count, bool sharded, const uint32_t *bitlen_hist = nullptr);

// the key has the endomorphism copy of the GLV split, or the library may build one for it
bool glv_possible(const Bases &bs);
// the split is to be preferred to the plain path for this commit (pairs: the pairs of the submission); the caller still has to
// have the copy (msm_route.h: GlvCopyFn; capi.hip: glv_ready)
bool choose_glv(const Bases &bs, const MsmPlan &plain, const MsmPlan &split, size_t pairs);

// Width trials (ctx.h: Bases::WidthTrial).  kind: bit 0 = GLV split, bit 1 = host scalars, bit 2 = a trial among the key's
// shared-bucket sets instead of neighbour widths.  Null where no trial runs for this shape.
Bases::WidthTrial *trial_for(const Bases &bs, size_t n, uint32_t count, uint32_t kind, uint32_t c_model);
static inline uint32_t trial_width(const Bases::WidthTrial &t) { return t.done ? t.best_c : t.cur_c; }
// the set a set trial measures now (model: the planner's set, where the trial's width names none of the key's)
const Bases::SharedSet *trial_set(const Bases &bs, const Bases::WidthTrial &t, const Bases::SharedSet *model);
// the wall time of the commit that ran under trial_width(t)
void trial_report(Bases::WidthTrial &t, double us, const Bases &bs);

// What a record that outlives the process may hold (msm_tuning.h): a width trial_candidate's rules could have produced for this
// kind -- plain 4 .. max_c, the halves of the GLV split 5 .. 16, a set trial one of set_widths -- and the fingerprint of the model
// the trials checked: FNV-1a 64 over the bytes of the measured tables, TRIAL_RUNS and TRIAL_OFFSETS.
static inline uint64_t fnv1a64(const void *data, size_t len, uint64_t h = 0xcbf29ce484222325ull) {   // (h: the hash so far, to go on from)
    const unsigned char *p = static_cast<const unsigned char *>(data);
    for (size_t i = 0; i < len; i++) { h ^= p[i]; h *= 0x100000001b3ull; }
    return h;
}
bool trial_width_possible(uint32_t kind, uint32_t c, uint32_t max_c, const uint32_t *set_widths, size_t nsets);
uint64_t plan_model_fingerprint();
