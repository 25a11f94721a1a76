// Host side of the cross-term evaluator (graph_kernels.cuh).  A flattened GraphEvaluator (include/mira_gpu.h) is COMPILED
// once per circuit (graph_compile.hip) and its instruction stream and constants uploaded; the handle is then evaluated for
// any number of (columns, challenges) pairs, alone or with the other graphs of a fold step, with one small upload and one
// launch -- or by a kernel of its own (mira_graph_specialize: graph_jit.hpp, graph_jit.hip).
#include "ctx.h"
#include "graph_compile.h"
#include "graph_kernels.cuh"
#include "graph_jit.hpp"
#include "host_field.hpp"
#ifndef MIRA_CPU_EMU
#include <thread>
#endif

namespace {

// reference form (x * 2^256, 4 x u64) -> x * 2^(261 - 5 form) (graph_compile.h: forms) as 9 x 29-bit limbs, canonical
template <class FP> void to_limbs29(const uint64_t in[4], int form, uint32_t out[9]) {
    hostf::HFe<FP> s;
    memcpy(s.l, in, 32);
    static hostf::HFe<FP> p32 = hostf::from_u64<FP>(32), i32 = hostf::inv(hostf::from_u64<FP>(32));
    for (int k = form; k < 1; k++) s = hostf::mul(s, p32);       // 2^256 -> 2^(256 + 5 (1 - form))
    for (int k = 1; k < form; k++) s = hostf::mul(s, i32);
    for (int i = 0; i < 9; i++) {
        const int bit = 29 * i, w = bit / 64, sh = bit % 64;
        uint64_t v = s.l[w] >> sh;
        if (sh > 35 && w + 1 < 4) v |= s.l[w + 1] << (64 - sh);
        out[i] = (uint32_t)(v & M29);
    }
}
void to_limbs29(int field, const uint64_t in[4], int form, uint32_t out[9]) {
    if (field == MIRA_FIELD_FQ) to_limbs29<FqP>(in, form, out); else to_limbs29<FrP>(in, form, out);
}
void one_raw(int field, uint64_t out[4]) {                      // 1 in the reference form
    if (field == MIRA_FIELD_FQ) { auto o = hostf::one<FqP>(); memcpy(out, o.l, 32); } else { auto o = hostf::one<FrP>(); memcpy(out, o.l, 32); }
}

struct Program {
    int field = 0;
    uint32_t num_challenges = 0, num_columns = 0, num_rotations = 0, num_calculations = 0;
    CompiledGraph cg;                          // its stream stays on the host too: what graph_jit.hpp writes out as a kernel
    void *d_static = nullptr;                  // code | constants | rotations
    size_t o_code = 0, o_const = 0, o_rot = 0;
    std::vector<int32_t> h_rot;                // the rotations again on the host (graph_jit.hpp)
#ifndef MIRA_CPU_EMU
    hipModule_t jit_mod = nullptr;             // the specialised kernel of this program (mira_graph_specialize), or null: interpreted
    hipFunction_t jit_fn = nullptr;
#endif
    std::vector<uint32_t> jit_kinds;           // the column kinds that kernel was built for (an evaluation with others is interpreted)
    DevBuf dyn;                                // challenges | column table of the current evaluation
    unsigned char *h_dyn = nullptr;            // pinned staging of the same
    size_t o_chal = 0, o_cols = 0, o_jobs = 0, dyn_bytes = 0;   // | job table of the batch this program leads
};
std::map<uint64_t, Program> g_programs;
uint32_t g_jit_last_compiled = 0, g_jit_last_from_disk = 0;   // of the last mira_graph_specialize: kernels compiled / read from the cache directory
constexpr uint32_t GRAPH_MAX_BATCH = 16;           // graphs per launch
// Intermediates kept in LDS per workgroup (9 KiB each at 256 lanes).  Measured at k = 17: with a batch
// that fills the wave slots two slots are best (eleven graphs 1.98 -> 1.87 ms; eight cost occupancy, 2.14),
// a lone graph of two workgroups per CU takes eight (0.280 -> 0.247 ms).
constexpr uint32_t GRAPH_LDS_SLOTS_BATCH = 2, GRAPH_LDS_SLOTS_LONE = 8;

size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }
int ensure_dyn(Program &pg, size_t bytes) {
    if (bytes <= pg.dyn_bytes && pg.h_dyn) return MIRA_OK;
    if (pg.h_dyn) (void)rt_host_free(pg.h_dyn);
    pg.h_dyn = nullptr; pg.dyn_bytes = 0;
    int rc = pg.dyn.ensure(bytes);
    if (rc) return rc;
    if (rt_host_alloc(reinterpret_cast<void **>(&pg.h_dyn), bytes) != hipSuccess) { pg.h_dyn = nullptr; set_error("pinned allocation for the compiled graph failed"); return MIRA_E_ALLOC; }
    pg.dyn_bytes = bytes;
    return MIRA_OK;
}

}   // namespace

int graph_compile(int field, const mira_graph *gr, uint32_t num_challenges, uint32_t num_columns, uint64_t *handle_out) {
    Program pg;
    if (int rc = compile_graph(*gr, num_challenges, num_columns, pg.cg)) return rc;
    const CompiledGraph &cg = pg.cg;
    pg.field = field; pg.num_challenges = num_challenges; pg.num_columns = num_columns;
    pg.num_rotations = gr->num_rotations; pg.num_calculations = gr->num_calculations;
    // static part on the device: code | constants (9 x 29-bit limbs, multiplier form) | rotations
    pg.o_code = 0;
    pg.o_const = align16(cg.stream.size() * 4);
    pg.o_rot = align16(pg.o_const + cg.pool.size() * 36);
    pg.h_rot.assign(gr->rotations, gr->rotations + gr->num_rotations);
    const size_t total = align16(pg.o_rot + (size_t)gr->num_rotations * 4) + 16;
    std::vector<unsigned char> stage(total, 0);
    memcpy(stage.data() + pg.o_code, cg.stream.data(), cg.stream.size() * 4);
    uint64_t one_r[4];
    one_raw(field, one_r);
    for (size_t k = 0; k < cg.pool.size(); k++)
        to_limbs29(field, cg.pool[k].first < 0 ? one_r : gr->constants + (size_t)cg.pool[k].first * 4, cg.pool[k].second,
                   reinterpret_cast<uint32_t *>(stage.data() + pg.o_const) + k * 9);
    if (gr->num_rotations) memcpy(stage.data() + pg.o_rot, gr->rotations, (size_t)gr->num_rotations * 4);
    if (rt_malloc(&pg.d_static, total) != hipSuccess || !pg.d_static) { set_error("device allocation for the compiled graph failed"); return MIRA_E_ALLOC; }
    RT_CHECK(rt_h2d(pg.d_static, stage.data(), total, g.stream));
    RT_CHECK(rt_sync(g.stream));                             // `stage` is pageable host memory about to go out of scope
    // dynamic part of an evaluation: column table | job table | the challenges of every program of the batch in the forms
    // it reads them, staged in pinned host memory (grown by the evaluation that needs more)
    pg.o_cols = 0;
    pg.o_jobs = align16((size_t)num_columns * sizeof(GraphCol));
    pg.o_chal = align16(pg.o_jobs + (size_t)GRAPH_MAX_BATCH * sizeof(GraphJob));
    int rc = ensure_dyn(pg, pg.o_chal + (cg.chal_vars.size() + 8) * 36 * 4);
    if (rc) { (void)rt_free(pg.d_static); return rc; }
    *handle_out = g.next_handle++;
    g_programs[*handle_out] = pg;
    return MIRA_OK;
}

int graph_free(uint64_t handle) {
    auto it = g_programs.find(handle);
    if (it == g_programs.end()) { set_error("unknown graph handle"); return MIRA_E_BAD_ARG; }
    Program &pg = it->second;
#ifndef MIRA_CPU_EMU
    if (pg.jit_mod) (void)hipModuleUnload(pg.jit_mod);
#endif
    if (pg.d_static) (void)rt_free(pg.d_static);
    if (pg.dyn.p) (void)rt_free(pg.dyn.p);
    if (pg.h_dyn) (void)rt_host_free(pg.h_dyn);
    g_programs.erase(it);
    return MIRA_OK;
}

int graph_field(uint64_t handle, int *field_out) {
    auto it = g_programs.find(handle);
    if (it == g_programs.end()) { set_error("unknown graph handle"); return MIRA_E_BAD_ARG; }
    *field_out = it->second.field;
    return MIRA_OK;
}

// count compiled graphs over the same columns and challenges, results to d_outs[k]; one launch per
// GRAPH_MAX_BATCH graphs
int graph_eval_batch(const uint64_t *handles, uint32_t count, const mira_eval_column *columns, uint32_t num_columns, const uint64_t *challenges,
                     uint32_t num_challenges, size_t num_rows, void *const *d_outs) {
    int rc;
    if (count == 0) return MIRA_OK;
    std::vector<Program *> pgs(count);
    for (uint32_t k = 0; k < count; k++) {
        auto it = g_programs.find(handles[k]);
        if (it == g_programs.end()) { set_error("unknown graph handle"); return MIRA_E_BAD_ARG; }
        Program &pg = *(pgs[k] = &it->second);
        if (num_challenges != pg.num_challenges || num_columns != pg.num_columns) {
            set_error("the graph was compiled for " + std::to_string(pg.num_challenges) + " challenges and " + std::to_string(pg.num_columns) + " columns");
            return MIRA_E_BAD_ARG;
        }
        if (pg.field != pgs[0]->field) { set_error("the graphs of a batch must be over one field"); return MIRA_E_BAD_ARG; }
        for (uint32_t col : pg.cg.used_columns) {
            if (!columns[col].d_data) {
                set_error("column variable index out of boundary: " + std::to_string(col));   // EvalError::ColumnVariableIndexOutOfBoundary / InvalidWitnessIndex
                return MIRA_E_BAD_ARG;
            }
            if (columns[col].kind != MIRA_COL_FIELD && columns[col].kind != MIRA_COL_BOOL) { set_error("unknown column kind"); return MIRA_E_BAD_ARG; }
        }
        if (num_rows && !d_outs[k]) { set_error("null output"); return MIRA_E_BAD_ARG; }
    }
    if (num_rows == 0) return MIRA_OK;
    if (num_rows > ((size_t)1 << 31)) { set_error("num_rows > 2^31"); return MIRA_E_UNSUPPORTED; }
    const uint32_t block = 256;
    const uint32_t grid = (uint32_t)std::min<size_t>((num_rows + block - 1) / block, 256 * 4);
    const size_t T = (size_t)grid * block;
    Program &p0 = *pgs[0];                                   // its staging carries the batch's column table, job table and challenges
    {
        size_t worst = 0;                                    // challenge entries of the largest launch
        for (uint32_t done = 0; done < count; done += GRAPH_MAX_BATCH) {
            size_t w = 0;
            for (uint32_t k = done; k < std::min<uint32_t>(count, done + GRAPH_MAX_BATCH); k++) w += pgs[k]->cg.chal_vars.size();
            worst = std::max(worst, w);
        }
        if ((rc = ensure_dyn(p0, p0.o_chal + (worst + 1) * 36))) return rc;
    }
    // the call's column pointers and challenges (each in the forms its program reads it): one small copy from pinned memory
    for (uint32_t c = 0; c < num_columns; c++) {
        GraphCol gc{reinterpret_cast<const unsigned char *>(columns[c].d_data), columns[c].kind, 0};
        memcpy(p0.h_dyn + p0.o_cols + (size_t)c * sizeof(GraphCol), &gc, sizeof gc);
    }
#ifndef MIRA_CPU_EMU
    static bool lds_ready = false;                           // eight LDS slots are 72 KiB, above the 64 KiB default
    if (!lds_ready) {
        RT_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_graph_eval<Fq29>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(GRAPH_LDS_SLOTS_LONE * 9 * block * 4)));
        RT_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_graph_eval<Fr29>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(GRAPH_LDS_SLOTS_LONE * 9 * block * 4)));
        lds_ready = true;
    }
#endif
    tm_begin();
#ifndef MIRA_CPU_EMU
    std::vector<std::pair<hipFunction_t, GraphJob>> jit_jobs;
#endif
    for (uint32_t done = 0; done < count; done += GRAPH_MAX_BATCH) {
        const uint32_t cnt = std::min<uint32_t>(GRAPH_MAX_BATCH, count - done);
        if (done) RT_CHECK(rt_sync(g.stream));               // the previous launch's copy still reads the pinned staging
        uint32_t live = 0, max_slots = 1, live_guess = 0;
        size_t chal_at = 0;
        for (uint32_t k = 0; k < cnt; k++) live_guess += pgs[done + k]->num_calculations != 0;
        const uint32_t lds_slots = (uint64_t)grid * live_guess <= 512 ? GRAPH_LDS_SLOTS_LONE : GRAPH_LDS_SLOTS_BATCH;
        for (uint32_t k = 0; k < cnt; k++) {
            Program &pg = *pgs[done + k];
            if (pg.num_calculations == 0) {                  // Ok(F::ZERO), graph_evaluator.rs:386-389
                RT_CHECK(rt_memset(d_outs[done + k], 0, num_rows * 32, g.stream));
                continue;
            }
            const unsigned char *st = reinterpret_cast<const unsigned char *>(pg.d_static);
            for (size_t v = 0; v < pg.cg.chal_vars.size(); v++)
                to_limbs29(p0.field, challenges + (size_t)pg.cg.chal_vars[v].first * 4, pg.cg.chal_vars[v].second, reinterpret_cast<uint32_t *>(p0.h_dyn + p0.o_chal) + (chal_at + v) * 9);
            GraphJob job{reinterpret_cast<const uint32_t *>(st + pg.o_code), reinterpret_cast<const uint32_t *>(st + pg.o_const),
                         reinterpret_cast<const uint32_t *>(reinterpret_cast<const unsigned char *>(p0.dyn.p) + p0.o_chal) + chal_at * 9,
                         reinterpret_cast<const int32_t *>(st + pg.o_rot), reinterpret_cast<unsigned char *>(d_outs[done + k]), pg.cg.ninstr,
                         std::min<uint32_t>(pg.cg.nslots, lds_slots)};
            chal_at += pg.cg.chal_vars.size();
#ifndef MIRA_CPU_EMU
            if (pg.jit_fn) {
                bool same = true;
                for (uint32_t col : pg.cg.used_columns) same &= columns[col].kind == pg.jit_kinds[col];
                if (same) { jit_jobs.push_back({pg.jit_fn, job}); continue; }
            }
#endif
            memcpy(p0.h_dyn + p0.o_jobs + (size_t)live * sizeof(GraphJob), &job, sizeof job);
            max_slots = std::max(max_slots, pg.cg.nslots);
            live++;
        }
#ifdef MIRA_CPU_EMU
        if (live) RT_CHECK(rt_h2d(p0.dyn.p, p0.h_dyn, p0.dyn_bytes, g.stream));
#else
        if (live || !jit_jobs.empty()) RT_CHECK(rt_h2d(p0.dyn.p, p0.h_dyn, p0.dyn_bytes, g.stream));
        // specialised programs: one launch each (a launch of 2^17 rows is two waves per SIMD, what their 256 VGPRs allow)
        for (auto &jj : jit_jobs) {
            struct { const uint32_t *consts29, *chal29; const GraphCol *cols; unsigned char *out; uint64_t nrows; } args{
                jj.second.consts29, jj.second.challenges29, reinterpret_cast<const GraphCol *>(reinterpret_cast<const unsigned char *>(p0.dyn.p) + p0.o_cols), jj.second.out, (uint64_t)num_rows};
            size_t arg_bytes = sizeof args;
            void *cfg[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &args, HIP_LAUNCH_PARAM_BUFFER_SIZE, &arg_bytes, HIP_LAUNCH_PARAM_END};
            const uint32_t jgrid = (uint32_t)std::min<size_t>((num_rows + graphjit::BLOCK - 1) / graphjit::BLOCK, 256 * 4 * 2 * 4);
            RT_CHECK(hipModuleLaunchKernel(jj.first, jgrid, 1, 1, graphjit::BLOCK, 1, 1, 0, g.stream, nullptr, cfg));
        }
        jit_jobs.clear();
#endif
        if (live) {
            const size_t ws_stride = (size_t)max_slots * 9 * T;
            if ((rc = g.graph_ws.ensure(ws_stride * live * 4))) return rc;
            const unsigned char *dy = reinterpret_cast<const unsigned char *>(p0.dyn.p);
            if (p0.field == MIRA_FIELD_FQ)
                LAUNCH(k_graph_eval<Fq29>, dim3(grid, live), block, (size_t)lds_slots * 9 * block * 4, g.stream, reinterpret_cast<const GraphJob *>(dy + p0.o_jobs),
                       reinterpret_cast<const GraphCol *>(dy + p0.o_cols), (uint64_t)num_rows, reinterpret_cast<uint32_t *>(g.graph_ws.p), (uint64_t)ws_stride);
            else
                LAUNCH(k_graph_eval<Fr29>, dim3(grid, live), block, (size_t)lds_slots * 9 * block * 4, g.stream, reinterpret_cast<const GraphJob *>(dy + p0.o_jobs),
                       reinterpret_cast<const GraphCol *>(dy + p0.o_cols), (uint64_t)num_rows, reinterpret_cast<uint32_t *>(g.graph_ws.p), (uint64_t)ws_stride);
        }
    }
    tm_mark("graph_eval");
    RT_CHECK(rt_last());
    RT_CHECK(rt_sync(g.stream));
    tm_end();
    return MIRA_OK;
}

// ---- the gates of a circuit over a Lagrange combination of traces (k_graph_eval_folded) ----------------------------------
// Lanes of a workgroup: the emulation's are OS threads that meet at every barrier of the in-workgroup tree, so it takes small
// workgroups (as REDUCE_SMALL_WG does); the kernel is written for any power of two up to 256.
#ifdef MIRA_CPU_EMU
static constexpr uint32_t FOLDED_BLOCK = 32, FOLDED_BLOCK_LOG = 5;
#else
static constexpr uint32_t FOLDED_BLOCK = 256, FOLDED_BLOCK_LOG = 8;
#endif
static constexpr uint32_t FOLDED_WORKGROUPS = 2048;   // default grid over all (point, gate, row block): a few turns of the two 80 KiB workgroups a CU's LDS holds

template <class F, bool REDUCE>
static void launch_folded(dim3 grid, size_t lds_bytes, const GraphJob *jobs, const GraphCol *cols, uint32_t ncols, uint32_t ntraces, const unsigned char *coeffs,
                          uint64_t nrows, uint32_t *ws, uint64_t ws_stride, const unsigned char *w, uint32_t tree_levels) {
    if (REDUCE) LAUNCH_BARRIER((k_graph_eval_folded<F, REDUCE>), grid, FOLDED_BLOCK, lds_bytes, g.stream, jobs, cols, ncols, ntraces, coeffs, nrows, ws, ws_stride, w, tree_levels);
    else LAUNCH((k_graph_eval_folded<F, REDUCE>), grid, FOLDED_BLOCK, lds_bytes, g.stream, jobs, cols, ncols, ntraces, coeffs, nrows, ws, ws_stride, w, tree_levels);
}

// weights == null: the leaves go to d_out[(p * num_gates + g) * num_rows + row].  Else: the roots of compute_G's tree to out[p]
// (host); the first min(log2 FOLDED_BLOCK, log2 num_rows) levels are folded inside the workgroups, the nodes lie in g.fold_nodes
// as k_pow_tree expects its leaves (node index = leaf index >> levels, point stride num_gates * num_rows >> levels).
// A specialised handle (mira_graph_specialize) is interpreted here: the generated kernels know plain columns only.
int graph_eval_folded(const uint64_t *handles, uint32_t num_gates, const mira_eval_column *columns, uint32_t num_columns, uint32_t num_traces,
                      const uint8_t *column_folded, const uint64_t *coeffs, const uint64_t *challenges, uint32_t num_challenges, uint32_t num_points, size_t num_rows,
                      void *d_out, const uint64_t *weights, uint64_t *out) {
    int rc;
    const bool reduce = weights != nullptr;
    std::vector<Program *> pgs(num_gates);
    for (uint32_t k = 0; k < num_gates; k++) {
        auto it = g_programs.find(handles[k]);
        if (it == g_programs.end()) { set_error("unknown graph handle"); return MIRA_E_BAD_ARG; }
        Program &pg = *(pgs[k] = &it->second);
        if (num_challenges != pg.num_challenges || num_columns != pg.num_columns) {
            set_error("the graph was compiled for " + std::to_string(pg.num_challenges) + " challenges and " + std::to_string(pg.num_columns) + " columns");
            return MIRA_E_BAD_ARG;
        }
        if (pg.field != pgs[0]->field) { set_error("the graphs of a batch must be over one field"); return MIRA_E_BAD_ARG; }
        for (uint32_t col : pg.cg.used_columns) {
            for (uint32_t j = 0; j < (column_folded[col] ? num_traces : 1u); j++) {
                const mira_eval_column &c = columns[(size_t)j * num_columns + col];
                if (!c.d_data) {
                    set_error("column variable index out of boundary: " + std::to_string(col) + (j ? " of trace " + std::to_string(j) : std::string()));
                    return MIRA_E_BAD_ARG;
                }
                if (c.kind != MIRA_COL_FIELD && c.kind != MIRA_COL_BOOL) { set_error("unknown column kind"); return MIRA_E_BAD_ARG; }
                if (column_folded[col] && c.kind != MIRA_COL_FIELD) { set_error("folded column " + std::to_string(col) + " is not of kind MIRA_COL_FIELD"); return MIRA_E_BAD_ARG; }
            }
        }
    }
    if (num_rows > ((size_t)1 << 31)) { set_error("num_rows > 2^31"); return MIRA_E_UNSUPPORTED; }
    const size_t leaves = (size_t)num_gates * num_rows;
    if (reduce && leaves == 0) { memset(out, 0, (size_t)num_points * 32); return MIRA_OK; }
    if (leaves == 0) return MIRA_OK;
    uint32_t levels_total = 0, rows_log = 0;
    if (reduce) {
        if (leaves & (leaves - 1)) {
            set_error("tree reduction needs a power-of-two number of leaves, got " + std::to_string(num_gates) + " gates x " + std::to_string(num_rows) + " rows");
            return MIRA_E_UNSUPPORTED;
        }
        while (((size_t)1 << levels_total) < leaves) levels_total++;
        while (((size_t)1 << rows_log) < num_rows) rows_log++;
    }
    const uint32_t block = FOLDED_BLOCK, tree_levels = reduce ? std::min(FOLDED_BLOCK_LOG, rows_log) : 0, tail_levels = levels_total - tree_levels;
    const size_t nblocks = (num_rows + block - 1) / block;
    const size_t nodes_per_point = leaves >> tree_levels;                 // reduce: node index = leaf index >> tree_levels
    Program &p0 = *pgs[0];                                   // its staging carries the call's tables
    const int field = p0.field;
    // the largest launch: gates per launch, challenge entries per point
    size_t worst_chal = 0;
    for (uint32_t done = 0; done < num_gates; done += GRAPH_MAX_BATCH) {
        size_t wv = 0;
        for (uint32_t k = done; k < std::min<uint32_t>(num_gates, done + GRAPH_MAX_BATCH); k++) wv += pgs[k]->cg.chal_vars.size();
        worst_chal = std::max(worst_chal, wv);
    }
    const uint32_t max_cnt = std::min<uint32_t>(num_gates, GRAPH_MAX_BATCH);
    // staging of one launch: column tables of every trace (the folded flag in trace 0's) | job per (point, gate) | coefficients
    // per (point, trace), multiplier form | the tree's first weights | challenges per (point, gate) in the forms the program reads
    const size_t o_cols = 0;
    const size_t o_jobs = align16((size_t)num_traces * num_columns * sizeof(GraphCol));
    const size_t o_coef = align16(o_jobs + (size_t)num_points * max_cnt * sizeof(GraphJob));
    const size_t o_w = o_coef + (size_t)num_points * num_traces * 48;
    const size_t o_chal = o_w + (size_t)FOLDED_BLOCK_LOG * 32;
    const size_t total = o_chal + ((size_t)num_points * worst_chal + 1) * 36;
    if ((rc = ensure_dyn(p0, total))) return rc;
    if (reduce && (rc = g.fold_nodes.ensure((size_t)num_points * nodes_per_point * 32))) return rc;
    std::vector<uint64_t> tail_w;
    if (reduce && tail_levels) {                             // k_pow_tree takes weights per point
        tail_w.resize((size_t)num_points * tail_levels * 4);
        for (uint32_t p = 0; p < num_points; p++) memcpy(tail_w.data() + (size_t)p * tail_levels * 4, weights + (size_t)tree_levels * 4, (size_t)tail_levels * 32);
        if ((rc = pow_tree_stage(tail_levels, tail_w.data(), num_points))) return rc;
    }
    for (uint32_t j = 0; j < num_traces; j++)
        for (uint32_t c = 0; c < num_columns; c++) {
            const mira_eval_column &col = columns[(size_t)j * num_columns + c];
            GraphCol gc{reinterpret_cast<const unsigned char *>(col.d_data), col.kind, j == 0 && column_folded[c] ? 1u : 0u};
            memcpy(p0.h_dyn + o_cols + ((size_t)j * num_columns + c) * sizeof(GraphCol), &gc, sizeof gc);
        }
    for (size_t q = 0; q < (size_t)num_points * num_traces; q++) to_mult48(field, coeffs + q * 4, reinterpret_cast<uint32_t *>(p0.h_dyn + o_coef + q * 48));
    if (tree_levels) memcpy(p0.h_dyn + o_w, weights, (size_t)tree_levels * 32);
    size_t want_grid = tuned(MIRA_TUNE_FOLDED_GRID, 0);
    if (want_grid == 0) want_grid = std::max<size_t>(1, FOLDED_WORKGROUPS / ((size_t)num_points * max_cnt));
    const uint32_t gx = (uint32_t)std::min<size_t>(nblocks, want_grid);
    const size_t T = (size_t)gx * block;
#ifndef MIRA_CPU_EMU
    static bool lds_ready = false;                           // eight LDS slots and the tree's nodes are 80 KiB, above the 64 KiB default
    if (!lds_ready) {
        const int most = (int)(GRAPH_LDS_SLOTS_LONE * 9 * block * 4 + FOLDED_TREE_BYTES);
        RT_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_graph_eval_folded<Fq29, false>), hipFuncAttributeMaxDynamicSharedMemorySize, most));
        RT_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_graph_eval_folded<Fr29, false>), hipFuncAttributeMaxDynamicSharedMemorySize, most));
        RT_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_graph_eval_folded<Fq29, true>), hipFuncAttributeMaxDynamicSharedMemorySize, most));
        RT_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_graph_eval_folded<Fr29, true>), hipFuncAttributeMaxDynamicSharedMemorySize, most));
        lds_ready = true;
    }
#endif
    unsigned char *dst = reinterpret_cast<unsigned char *>(reduce ? g.fold_nodes.p : d_out);
    const size_t per_gate = reduce ? num_rows >> tree_levels : num_rows;   // elements one (point, gate) writes
    tm_begin();
    for (uint32_t done = 0; done < num_gates; done += GRAPH_MAX_BATCH) {
        const uint32_t cnt = std::min<uint32_t>(GRAPH_MAX_BATCH, num_gates - done);
        if (done) RT_CHECK(rt_sync(g.stream));               // the previous launch's copy still reads the pinned staging
        std::vector<uint32_t> live;                          // gates of this launch that have calculations
        uint32_t max_slots = 1, max_nlds = 0;
        for (uint32_t k = 0; k < cnt; k++) {
            Program &pg = *pgs[done + k];
            if (pg.num_calculations == 0) {                  // Ok(F::ZERO), graph_evaluator.rs:386-389: zero leaves, zero nodes
                for (uint32_t p = 0; p < num_points; p++)
                    RT_CHECK(rt_memset(dst + ((size_t)p * num_gates + done + k) * per_gate * 32, 0, per_gate * 32, g.stream));
                continue;
            }
            live.push_back(done + k);
            max_slots = std::max(max_slots, pg.cg.nslots);
            max_nlds = std::max(max_nlds, std::min<uint32_t>(pg.cg.nslots, GRAPH_LDS_SLOTS_LONE));
        }
        if (live.empty()) continue;
        const uint32_t nlive = (uint32_t)live.size();
        size_t chal_at = 0;
        const unsigned char *dy = reinterpret_cast<const unsigned char *>(p0.dyn.p);
        for (uint32_t p = 0; p < num_points; p++)
            for (uint32_t q = 0; q < nlive; q++) {
                Program &pg = *pgs[live[q]];
                const unsigned char *st = reinterpret_cast<const unsigned char *>(pg.d_static);
                for (size_t v = 0; v < pg.cg.chal_vars.size(); v++)
                    to_limbs29(field, challenges + ((size_t)p * num_challenges + pg.cg.chal_vars[v].first) * 4, pg.cg.chal_vars[v].second,
                               reinterpret_cast<uint32_t *>(p0.h_dyn + o_chal) + (chal_at + v) * 9);
                GraphJob job{reinterpret_cast<const uint32_t *>(st + pg.o_code), reinterpret_cast<const uint32_t *>(st + pg.o_const),
                             reinterpret_cast<const uint32_t *>(dy + o_chal) + chal_at * 9, reinterpret_cast<const int32_t *>(st + pg.o_rot),
                             dst + ((size_t)p * num_gates + live[q]) * per_gate * 32, pg.cg.ninstr, std::min<uint32_t>(pg.cg.nslots, GRAPH_LDS_SLOTS_LONE)};
                memcpy(p0.h_dyn + o_jobs + ((size_t)p * nlive + q) * sizeof(GraphJob), &job, sizeof job);
                chal_at += pg.cg.chal_vars.size();
            }
        RT_CHECK(rt_h2d(p0.dyn.p, p0.h_dyn, total, g.stream));
        // slots past the LDS planes live in the workspace, indexed by slot like k_graph_eval's: none when every program fits LDS
        const size_t ws_stride = max_slots > GRAPH_LDS_SLOTS_LONE ? (size_t)max_slots * 9 * T : 0;
        if ((rc = g.graph_ws.ensure(std::max<size_t>(16, ws_stride * nlive * num_points * 4)))) return rc;
        const dim3 grid(gx, nlive, num_points);
        const size_t lds_bytes = (size_t)FOLDED_TREE_BYTES + (size_t)max_nlds * 9 * block * 4;
        const GraphJob *jobs = reinterpret_cast<const GraphJob *>(dy + o_jobs);
        const GraphCol *cols = reinterpret_cast<const GraphCol *>(dy + o_cols);
        uint32_t *ws = reinterpret_cast<uint32_t *>(g.graph_ws.p);
        if (field == MIRA_FIELD_FQ) {
            if (reduce) launch_folded<Fq29, true>(grid, lds_bytes, jobs, cols, num_columns, num_traces, dy + o_coef, (uint64_t)num_rows, ws, (uint64_t)ws_stride, dy + o_w, tree_levels);
            else launch_folded<Fq29, false>(grid, lds_bytes, jobs, cols, num_columns, num_traces, dy + o_coef, (uint64_t)num_rows, ws, (uint64_t)ws_stride, dy + o_w, tree_levels);
        } else {
            if (reduce) launch_folded<Fr29, true>(grid, lds_bytes, jobs, cols, num_columns, num_traces, dy + o_coef, (uint64_t)num_rows, ws, (uint64_t)ws_stride, dy + o_w, tree_levels);
            else launch_folded<Fr29, false>(grid, lds_bytes, jobs, cols, num_columns, num_traces, dy + o_coef, (uint64_t)num_rows, ws, (uint64_t)ws_stride, dy + o_w, tree_levels);
        }
    }
    tm_mark("graph_eval_folded");
    if (reduce) {
        const void *roots = g.fold_nodes.p;                  // no level left: the nodes are the roots, one per point
        if (tail_levels && (rc = pow_tree_launch(field, g.fold_nodes.p, tail_levels, nodes_per_point, num_points, &roots))) return rc;
        tm_mark("pow_tree");
        RT_CHECK(rt_last());
        RT_CHECK(rt_d2h(out, roots, (size_t)num_points * 32, g.stream));
    } else {
        RT_CHECK(rt_last());
    }
    RT_CHECK(rt_sync(g.stream));
    tm_end();
    return MIRA_OK;
}

int graph_eval_compiled(uint64_t handle, const mira_eval_column *columns, uint32_t num_columns, const uint64_t *challenges, uint32_t num_challenges,
                        size_t num_rows, void *d_out) {
    return graph_eval_batch(&handle, 1, columns, num_columns, challenges, num_challenges, num_rows, &d_out);
}

// one-shot form: compile, evaluate, free
int graph_eval_device(int field, const mira_graph *gr, const mira_eval_column *columns, uint32_t num_columns, const uint64_t *challenges,
                      uint32_t num_challenges, size_t num_rows, void *d_out) {
    uint64_t h = 0;
    int rc = graph_compile(field, gr, num_challenges, num_columns, &h);
    if (rc) return rc;
    rc = graph_eval_compiled(h, columns, num_columns, challenges, num_challenges, num_rows, d_out);
    const std::string err = rc ? std::string(mira_last_error()) : std::string();
    graph_free(h);
    if (rc) set_error(err);
    return rc;
}

// ---- specialised kernels (graph_jit.hpp) ----------------------------------------------------------------------------
static std::vector<uint32_t> kinds_of(const mira_eval_column *columns, uint32_t num_columns) {
    std::vector<uint32_t> k(num_columns, MIRA_COL_FIELD);
    for (uint32_t c = 0; c < num_columns; c++) if (columns) k[c] = columns[c].kind;
    return k;
}
int graph_jit_source(uint64_t handle, const mira_eval_column *columns, uint32_t num_columns, char *buf, size_t cap, size_t *len_out) {
    auto it = g_programs.find(handle);
    if (it == g_programs.end()) { set_error("unknown graph handle"); return MIRA_E_BAD_ARG; }
    const Program &pg = it->second;
    if (!len_out) { set_error("null output"); return MIRA_E_BAD_ARG; }
    if (pg.num_calculations == 0 || pg.cg.ninstr == 0) { *len_out = 0; return MIRA_OK; }
    if (num_columns != pg.num_columns) { set_error("the graph was compiled for " + std::to_string(pg.num_columns) + " columns"); return MIRA_E_BAD_ARG; }
    const std::string src = graphjit::source(pg.field, pg.cg.stream, pg.h_rot, kinds_of(columns, num_columns), tuned(MIRA_TUNE_JIT_LOADS_AHEAD, graphjit::LOADS_AHEAD_DEFAULT));
    *len_out = src.size();
    if (buf && cap) {
        const size_t ncopy = std::min(cap - 1, src.size());
        memcpy(buf, src.data(), ncopy);
        buf[ncopy] = 0;
    }
    return MIRA_OK;
}

// Every handle gets its own kernel; the compilations run on one host thread each (a MainGate<5> evaluation point takes
// ~5 s).  A handle that is specialised already, or has no calculations, is left as it is.  On failure nothing changes:
// the graphs stay interpreted.
int graph_specialize(const uint64_t *handles, uint32_t count, const mira_eval_column *columns, uint32_t num_columns, std::unique_lock<std::mutex> *library_lock) {
#ifdef MIRA_CPU_EMU
    (void)handles; (void)count; (void)columns; (void)num_columns; (void)library_lock;
    set_error("the host emulation has no run-time compiler: graphs stay interpreted");
    return MIRA_E_JIT_UNAVAILABLE;
#else
    std::vector<uint64_t> todo;                              // handles, not pointers: the lock is released while the compiler runs
    for (uint32_t k = 0; k < count; k++) {
        auto it = g_programs.find(handles[k]);
        if (it == g_programs.end()) { set_error("unknown graph handle"); return MIRA_E_BAD_ARG; }
        const Program &pg = it->second;
        if (num_columns != pg.num_columns) { set_error("the graph was compiled for " + std::to_string(pg.num_columns) + " columns"); return MIRA_E_BAD_ARG; }
        if (pg.jit_fn || pg.num_calculations == 0 || pg.cg.ninstr == 0) continue;
        if (pg.cg.ninstr > graphjit::MAX_INSTR) { set_error("graph of " + std::to_string(pg.cg.ninstr) + " instructions is too long to specialise"); return MIRA_E_UNSUPPORTED; }
        if (std::find(todo.begin(), todo.end(), handles[k]) == todo.end()) todo.push_back(handles[k]);
    }
    g_jit_last_compiled = g_jit_last_from_disk = 0;
    if (todo.empty()) return MIRA_OK;
    if (!graphjit::rtc().error.empty()) { set_error(graphjit::rtc().error); return MIRA_E_JIT_UNAVAILABLE; }
    std::vector<std::vector<char>> code(todo.size());
    std::vector<std::string> errs(todo.size());
    std::vector<std::thread> workers;
    const std::vector<uint32_t> kinds = kinds_of(columns, num_columns);
    const size_t ahead = tuned(MIRA_TUNE_JIT_LOADS_AHEAD, graphjit::LOADS_AHEAD_DEFAULT);
    // code objects of this process by source text: a second evaluator of the same graph (another PlonkStructure of the same
    // circuit, the other leg of a benchmark) costs a module load, not a compilation
    static std::map<std::string, std::vector<char>> compiled;
    std::vector<std::string> src(todo.size());
    std::vector<size_t> fresh;
    size_t from_disk = 0;
    for (size_t k = 0; k < todo.size(); k++) {
        const Program &pg = g_programs.find(todo[k])->second;
        src[k] = graphjit::source(pg.field, pg.cg.stream, pg.h_rot, kinds, ahead);
        auto hit = compiled.find(src[k]);
        if (hit != compiled.end()) { code[k] = hit->second; continue; }
        code[k] = graphjit::cache_load(src[k]);              // a file of an earlier process (mira_graph_set_cache_dir)
        if (code[k].empty()) fresh.push_back(k); else { compiled[src[k]] = code[k]; from_disk++; }
    }
    // The compiler runs for seconds and touches nothing of the library's: other threads may commit, transform and evaluate
    // (interpreted) meanwhile.  They may also free one of these handles -- looked up again below.
    if (library_lock && !fresh.empty()) library_lock->unlock();
    auto work = [&](size_t k) { code[k] = graphjit::compile(src[k], errs[k]); };
    for (size_t q = 1; q < fresh.size(); q++) workers.emplace_back(work, fresh[q]);
    if (!fresh.empty()) work(fresh[0]);
    for (auto &t : workers) t.join();
    if (library_lock && !fresh.empty()) library_lock->lock();
    for (size_t k = 0; k < todo.size(); k++)
        if (code[k].empty()) { set_error(errs[k]); return MIRA_E_JIT_FAILED; }
    if (compiled.size() + fresh.size() > 256) compiled.clear();   // a bound on what a long-lived process keeps (a code object is ~200 KiB)
    for (size_t k : fresh) { compiled[src[k]] = code[k]; graphjit::cache_store(src[k], code[k]); }
    g_jit_last_compiled = (uint32_t)fresh.size(); g_jit_last_from_disk = (uint32_t)from_disk;
    std::vector<Program *> live(todo.size(), nullptr);       // freed meanwhile, or specialised by another thread: nothing to do
    for (size_t k = 0; k < todo.size(); k++) {
        auto it = g_programs.find(todo[k]);
        if (it != g_programs.end() && !it->second.jit_fn) live[k] = &it->second;
    }
    std::vector<hipModule_t> mods(todo.size(), nullptr);
    std::vector<hipFunction_t> fns(todo.size(), nullptr);
    for (size_t k = 0; k < todo.size(); k++) {
        if (!live[k]) continue;
        hipError_t e = hipModuleLoadData(&mods[k], code[k].data());
        if (e == hipSuccess) e = hipModuleGetFunction(&fns[k], mods[k], "mira_jit_eval");
        if (e != hipSuccess) {
            for (size_t q = 0; q <= k; q++) if (mods[q]) (void)hipModuleUnload(mods[q]);
            set_error(std::string("loading a specialised kernel failed: ") + hipGetErrorString(e));
            return MIRA_E_JIT_FAILED;
        }
    }
    for (size_t k = 0; k < todo.size(); k++)
        if (live[k]) { live[k]->jit_mod = mods[k]; live[k]->jit_fn = fns[k]; live[k]->jit_kinds = kinds; }
    return MIRA_OK;
#endif
}
int graph_jit_stats(uint32_t *compiled_out, uint32_t *from_disk_out) {
    if (compiled_out) *compiled_out = g_jit_last_compiled;
    if (from_disk_out) *from_disk_out = g_jit_last_from_disk;
    return MIRA_OK;
}
int graph_is_specialized(uint64_t handle, int32_t *out) {
    auto it = g_programs.find(handle);
    if (it == g_programs.end() || !out) { set_error("unknown graph handle"); return MIRA_E_BAD_ARG; }
#ifdef MIRA_CPU_EMU
    *out = 0;
#else
    *out = it->second.jit_fn ? 1 : 0;
#endif
    return MIRA_OK;
}
