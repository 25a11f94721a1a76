// The route of an MSM (msm_route.hip): which mode a commit, a partial or a batch takes -- per-window buckets, one of the key's
// shared-bucket sets, or its 20 / 22-bit wide tables --, whether it takes the GLV split, under which width or set trial, whether
// it collects or consumes bit-length statistics, and the shape of what comes back.  Decided here, executed in capi.hip.  Host
// code only, like the planner it calls (msm_plan.h): no HIP call, no allocation, no launch; tests/emu/test_msm_route.cpp runs it
// without kernels.  The one device action a decision depends on -- building a key's endomorphism copy -- is the caller's: the
// route asks for it through a function it is given, at the point where the answer is needed (GlvCopyFn).
#pragma once
#include "msm_plan.h"

enum MsmMode { MSM_PER_WINDOW, MSM_SHARED_SET, MSM_WIDE_TABLE };

struct MsmRequest {
    size_t first = 0, n = 0;                   // the key's points [first, first + n)
    size_t count = 1, stride = 0;              // batches: commitments, and the elements between the starts of their vectors
    bool sharded = false;                      // the caller is one rank of a point-chunk sharded MSM: all ranks must produce the same kind of
                                               // partial, so the mode depends on what the handle has and on the widths asked for, never on n
    int32_t requested_c = 0;                   // the call's own window width (sharded partials), 0 = none
    bool have_scalars = false;                 // a device buffer of scalars was given at all
    bool host_scalars = false;                 // a single commit whose scalars are still in host memory (the device buffer is their staging area)
    const uint64_t *const *h_batch = nullptr;  // a batch whose vectors are still in host memory
    bool caller_combines = false;              // the points come back to a commit of this process, which combines any number of pieces itself
                                               // (horner_pieces); else the public partial format, one point per window
    void *windows_dst = nullptr;               // mira_msm_partial_to_device: the sums stay in device memory, here
};

struct MsmRoute {
    int rc = MIRA_OK;                          // the request is refused: code and text
    const char *err = nullptr;
    bool recorded = false;                     // shape and last_* are settled: the executor records them, for a request refused after this point too
    bool empty = false;                        // n == 0: nothing to launch, the answer is the identity in `shape`
    MsmMode mode = MSM_PER_WINDOW;
    MsmPlan plan;                              // glv, stats, pieces, h_batch and windows_dst settled (wide tables: only windows_dst is read)
    const Bases::SharedSet *set = nullptr;     // MSM_SHARED_SET: which
    Bases::WidthTrial *trial = nullptr;        // the width or set trial this launch reports its time to, or null
    Bases::WidthTrial *trial_to_end = nullptr; // batches: the trial whose candidate does not fit one scan ends once this launch has run
    PartialShape shape;
    int32_t last_c = 0, last_w = 0, last_table_c = 0;   // mira_msm_last_plan, mira_msm_last_table_bits
};

// The key's endomorphism copy is there now (capi.hip: glv_ready builds it on first use).  Called only once the split is otherwise
// decided, and before any trial record of the commit is looked up: a split whose copy could not be built touches no trial, leaves
// glv_auto_failed set on the key, and the commit goes down the plain path under the plain plan's trial.
typedef bool (*GlvCopyFn)(const Bases &bs);

// (the route is the library's own business: its functions stay out of the dynamic symbol table)
#define MSM_ROUTE_LOCAL __attribute__((visibility("hidden")))
// a single commit or a partial (first + n within the key: the caller has checked)
MSM_ROUTE_LOCAL MsmRoute route_commit(const Bases &bs, const MsmRequest &rq, GlvCopyFn copy_ready);

// A batch of rq.count commitments over the key's prefix is cut into launches of `per` commitments (the window-counter scan and the
// 32-bit entry offsets stay in range): route_batch decides what the whole batch shares, route_batch_launch the launch that starts
// at commitment `done`.
struct BatchRoute {
    int rc = MIRA_OK;
    const char *err = nullptr;
    bool empty = false;                        // n == 0: count identities
    int32_t forced_c = 0;
    const Bases::SharedSet *set = nullptr;     // every commitment gets one bucket set of this table set; null: per-window buckets
    Bases::WidthTrial *set_trial = nullptr;    // the set trial the WHOLE batch (its launches and their epilogues) reports to, or null
    bool glv = false;
    size_t per = 1;
};
MSM_ROUTE_LOCAL BatchRoute route_batch(const Bases &bs, const MsmRequest &rq, GlvCopyFn copy_ready);
MSM_ROUTE_LOCAL MsmRoute route_batch_launch(const Bases &bs, const MsmRequest &rq, const BatchRoute &b, size_t done);
