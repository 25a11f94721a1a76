// What a key has learned about its own commits, as bytes (msm_tuning.hip): the finished width and set trials of its shapes
// (ctx.h: Bases::WidthTrial) and the bit-length statistics of its last commit, written out by one process and read back by the
// next, so that the first commits of a fresh process run at the widths the last one settled on.  The layout is documented byte
// by byte in include/mira_gpu.h (mira_msm_tuning_export).  Host code only, like the planner and the route (msm_plan.h,
// msm_route.h): no HIP call, no allocation on the device, no launch; tests/emu/test_msm_tuning.cpp runs it without kernels.
// A blob never changes a result, only which width a commit runs at.
#pragma once
#include "msm_plan.h"

static constexpr uint32_t TUNING_VERSION = 1;
static constexpr size_t TUNING_MAX_RECORDS = 12;             // trial_for keeps as many shapes per key
static constexpr size_t TUNING_MAX_ARCH = 64, TUNING_MAX_SETS = 32;

// (the library's own business, like the route: out of the dynamic symbol table)
#define MSM_TUNING_LOCAL __attribute__((visibility("hidden")))
// The key's finished trials and its statistics slot under the identity (arch, planner model, curve, length, max_c, set widths,
// table_c).  arch: the device's architecture name, from the caller.  Deterministic: the same state gives the same bytes.
MSM_TUNING_LOCAL void tuning_export(const Bases &bs, const char *arch, std::vector<unsigned char> *out_bytes);
// MIRA_E_BAD_ARG (*err says why) for a malformed blob; MIRA_OK with *accepted = 0 for a well-formed blob of another identity;
// MIRA_OK with *accepted = 1 once its records and statistics are the key's.  Only the last changes bs, and the whole blob is
// validated before anything is touched.
MSM_TUNING_LOCAL int tuning_import(const Bases &bs, const char *arch, const void *bytes, size_t len, int32_t *accepted, std::string *err);
