// Cross-term evaluation on the GPU: the calculation list of a GraphEvaluator (reference
// src/polynomial/graph_evaluator.rs:70-162, 361-390) run for every row at once.
//
// The reference walks the list once per row, rows in parallel over rayon threads
// (src/nifs/vanilla/mod.rs:104-113).  Here a lane owns a row and the whole wave walks the list in
// lockstep: instruction words, constants and challenges are wave-uniform (scalar loads), column
// reads are 32-byte loads at consecutive rows (rotations shift the whole wave), and the
// intermediates live in a slot-major workspace ws[slot][limb][lane] so that every intermediate
// access is nine fully coalesced dword bursts per wave.  Slots are the host's register allocation of
// the intermediates (graph_compile.hip): a handful, reused, so the workspace stays cache resident.
//
// Arithmetic: 9 x 29-bit limbs (field29.cuh: half the instructions of the 8 x 32-bit CIOS per
// multiplication).  Values are "loose" between calculations; the host COMPILES the program
// (graph_compile.hip, the stream format in graph_stream.h) with a proven bound for every value -- invariant: whatever is stored or forwarded is
// < 12 P, so any two values may be multiplied (144 <= 168) -- and inserts a normalising
// multiplication by one where a chain of additions would leave the budget.  Columns are read as they lie
// in memory (x * 2^256, no lifting product): the compiler tracks for every value the power of two it
// carries (its "form", graph_compile.h), hands constants and challenges over in the form each use wants,
// and converts where forms cannot be made to agree; the program's last instruction leaves the result
// as x * 2^256 below 2 P and the kernel stores it canonical.  Field results are exact, so every value
// equals the reference's bit for bit whatever the order of rows.
#pragma once
#include "field29.cuh"
#include "graph_stream.h"
#include "fold_kernels.cuh"

struct GraphCol {
    const unsigned char *p;
    uint32_t kind, pad;                                  // pad: read by the folded fetch alone (GraphFold), != 0 = a witness column
};

template <class F> DEV Fe29<F> graph_sub(const Fe29<F> &a, const Fe29<F> &b, uint32_t K) {
    switch (K) {                                         // smallest multiple of P above the subtrahend (chosen by the host)
        case 2: return f29_sub<2>(a, b);
        case 4: return f29_sub<4>(a, b);
        case 8: return f29_sub<8>(a, b);
        default: return f29_sub<16>(a, b);
    }
}

// one compiled graph of a batch: the graphs of a batch (the d - 1 cross-term expressions of a fold
// step, src/nifs/vanilla/mod.rs:100-121) read the same columns and challenges
struct GraphJob {
    const uint32_t *code, *consts29, *challenges29;      // constants and this evaluation's challenges, each in the forms the program reads them
    const int32_t *rotations;
    unsigned char *out;
    uint32_t ninstr, nlds;                               // slots below nlds live in LDS (the compiler numbers the most used ones lowest)
};

// The folded fetch (k_graph_eval_folded below): the column table holds `ntraces` tables of `ncols` entries one after the other
// (trace 0 = the accumulator), `coeffs` the evaluation point's ntraces Lagrange coefficients in multiplier form (48 B each, value *
// 2^261, as fold_const_load reads them).  A column whose entry in trace 0 is marked `pad != 0` is a witness column: the program
// reads sum_j coeffs[j] * trace_j[column][row] there (FoldedTrace, reference src/nifs/protogalaxy/poly/folded_trace.rs:53-131).
struct GraphFold {
    const unsigned char *coeffs;
    uint32_t ntraces, ncols;
};

// One row through one compiled program: the walk of the instruction stream shared by every kernel of this file.  Returns the
// program's last value, x * 2^256 below 2 P.  FOLDED: witness columns are folded on the fly (GraphFold); the folded value meets
// the stream's contract for a column -- canonical, form 1, as a column lies in memory: every term is made canonical and the sum
// is taken canonically, exactly as k_lincomb does, so it equals the materialised folded trace bit for bit.  The rotation is
// applied to the row before the traces are read (the fold is linear).
template <class F, bool FOLDED>
DEV Fe29<F> graph_eval_row(const uint32_t *__restrict__ code, const uint32_t ninstr, const uint32_t *__restrict__ consts29,
                           const uint32_t *__restrict__ challenges29, const int32_t *__restrict__ rotations, const GraphCol *__restrict__ cols,
                           const uint64_t nrows, const uint64_t row, uint32_t *__restrict__ lds, const uint32_t nlds, uint32_t *__restrict__ ws,
                           const uint64_t T, const uint64_t lane, const GraphFold fold) {
    using S = typename F::Sat;
    Fe29<F> v = f29_zero<F>(), prev;
    auto fetch = [&](uint32_t s, uint32_t bound) -> Fe29<F> {
        const uint32_t kind = s >> 29, payload = s & 0x1FFFFFFFu;     // graph_stream.h spelled out: its helpers here change the code object
        Fe29<F> r;
        if (kind == GRAPH_SRC_PREV) {
            r = prev;
        } else if (kind == MIRA_SRC_CONSTANT || kind == MIRA_SRC_CHALLENGE) {
            const uint32_t *p = (kind == MIRA_SRC_CONSTANT ? consts29 : challenges29) + (size_t)payload * 9;
#pragma unroll
            for (int k = 0; k < 9; k++) r.l[k] = p[k];
        } else if (kind == MIRA_SRC_INTERMEDIATE) {
            if (payload < nlds) {                        // wave-uniform
#pragma unroll
                for (int k = 0; k < 9; k++) r.l[k] = lds[(payload * 9 + k) * blockDim.x + threadIdx.x];
            } else {
#pragma unroll
                for (int k = 0; k < 9; k++) r.l[k] = ws[((size_t)payload * 9 + k) * T + lane];
            }
        } else {
            const GraphCol c = cols[payload & 0xFFFFFu];
            int64_t rr = ((int64_t)row + rotations[payload >> 20]) % (int64_t)nrows;   // rem_euclid, graph_evaluator.rs:51-53
            if (rr < 0) rr += (int64_t)nrows;
            // a column enters as it lies in memory -- x * 2^256, "form 1" of the compiler (graph_compile.h), no lifting
            // product -- and a selector as the number one in that form (src/plonk/eval.rs:62)
            if (FOLDED && c.pad) {                       // wave-uniform: a property of the column
                Fe<S> acc = fe_zero<S>();
                for (uint32_t j = 0; j < fold.ntraces; j++) {
                    const Fe<S> t = fe_load<S>(cols[(size_t)j * fold.ncols + (payload & 0xFFFFFu)].p + (size_t)rr * 32);
                    acc = fe_add(acc, fold_canonical(f29_mul(f29_unpack_canonical<F>(t), fold_const_load<F>(fold.coeffs + (size_t)j * 48))));
                }
                r = f29_unpack_canonical<F>(acc);
            } else if (c.kind == MIRA_COL_BOOL) {
                Fe<S> one_r;
#pragma unroll
                for (int k = 0; k < 8; k++) one_r.l[k] = c.p[rr] ? S::R1[k] : 0u;
                r = f29_unpack_canonical<F>(one_r);
            } else {
                r = f29_unpack_canonical<F>(fe_load<S>(c.p + (size_t)rr * 32));
            }
        }
        F29_SET(r, (double)bound / 256.0);
        (void)bound;
        return r;
    };
    const uint32_t *pc = code;
    for (uint32_t i = 0; i < ninstr; i++) {
        const uint32_t head = pc[0], dst = pc[1], bounds = pc[2];
        prev = v;
        const uint32_t op = gop_op(head), K = gop_bias(head);
        const Fe29<F> a = fetch(pc[3], bounds & 0xFFFFu);
        if (op == GOP_ADD) { v = f29_add(a, fetch(pc[4], bounds >> 16)); pc += 5; }
        else if (op == GOP_SUB) { v = graph_sub(a, fetch(pc[4], bounds >> 16), K); pc += 5; }
        else if (op == GOP_MUL) { v = f29_mul(a, fetch(pc[4], bounds >> 16)); pc += 5; }
        else if (op == GOP_MAC) { const Fe29<F> b = fetch(pc[4], bounds >> 16), c = fetch(pc[5], pc[6]); v = f29_add(f29_mul(a, b), c); pc += 7; }
        else {
            if (op == GOP_SQR) v = f29_sqr(a);
            else if (op == GOP_DBL) v = f29_dbl(a);
            else if (op == GOP_NEG) v = graph_sub(f29_zero<F>(), a, K);
            else if (op == GOP_NORM) v = f29_mul(a, f29_one<F>());
            else v = a;                                  // GOP_COPY
            pc += 4;
        }
        if (dst != GRAPH_NO_SLOT) {                      // no slot: nobody reads it again
            if (dst < nlds) {
#pragma unroll
                for (int k = 0; k < 9; k++) lds[(dst * 9 + k) * blockDim.x + threadIdx.x] = v.l[k];
            } else {
#pragma unroll
                for (int k = 0; k < 9; k++) ws[((size_t)dst * 9 + k) * T + lane] = v.l[k];
            }
        }
    }
    return v;
}

// grid = (row blocks, graphs of the batch): a fold step's handful of graphs over 2^17 rows are two waves
// per SIMD each -- launched together they fill the wave slots (82 VGPRs: six per SIMD)
template <class F>
KERNEL void __launch_bounds__(256) k_graph_eval(const GraphJob *__restrict__ jobs,
                         const GraphCol *__restrict__ cols, uint64_t nrows, uint32_t *__restrict__ ws_all, uint64_t ws_stride) {
    DYN_SHARED(uint32_t, lds);                           // lds[slot][limb][lane of the workgroup]
    const GraphJob job = jobs[blockIdx.y];
    const uint32_t nlds = job.nlds;
    const uint32_t *__restrict__ code = job.code, *__restrict__ consts29 = job.consts29, *__restrict__ challenges29 = job.challenges29;
    const int32_t *__restrict__ rotations = job.rotations;
    unsigned char *__restrict__ out = job.out;
    const uint32_t ninstr = job.ninstr;
    uint32_t *__restrict__ ws = ws_all + (size_t)blockIdx.y * ws_stride;
    const uint64_t T = (uint64_t)gridDim.x * blockDim.x, lane = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (uint64_t row = lane; row < nrows; row += T) {
        const Fe29<F> v = graph_eval_row<F, false>(code, ninstr, consts29, challenges29, rotations, cols, nrows, row, lds, nlds, ws, T, lane, GraphFold{nullptr, 0, 0});
        fe_store(out + row * 32, reduce_once(f29_pack(v)));     // the program's last instruction left x * 2^256 below 2 P
    }
}

// The gates of a circuit over a Lagrange combination of traces (ProtoGalaxy's compute_G, reference
// src/nifs/protogalaxy/poly/mod.rs:218-303): the same walk with the folded fetch, for every evaluation point at once.
//   grid = (row-block workgroups per (point, gate), gates of this launch, points), 256 lanes; jobs[point * gridDim.y + gate]
//   carries the program and that point's challenges in the forms the program reads them; coeffs[point][trace], 48 B each.
// A workgroup owns 256 consecutive rows at a time and walks the row blocks blockIdx.x, blockIdx.x + gridDim.x, ...: the trip count
// of that loop depends on blockIdx alone, so every lane of the workgroup takes part in every barrier below -- lanes past nrows
// with a zero leaf.
// REDUCE = false: the leaves are written to job.out[row].
// REDUCE = true:  the leaves are not written.  They go to LDS and tree_levels = min(8, log2 nrows) levels of compute_G's tree
//   (:263-290), node = left + right * w[level], are folded there (nrows is a power of two); one node per row block goes to
//   job.out[block] -- k_pow_tree finishes from there with the remaining weights.
//   w: tree_levels canonical Montgomery elements, the same for every point.
// LDS: 8 KiB of tree nodes in front of the slot planes lds[slot][limb][lane].
static constexpr uint32_t FOLDED_TREE_BYTES = 256 * 32;
template <class F, bool REDUCE>
KERNEL void __launch_bounds__(256) k_graph_eval_folded(const GraphJob *__restrict__ jobs, const GraphCol *__restrict__ cols, uint32_t ncols, uint32_t ntraces,
                         const unsigned char *__restrict__ coeffs, uint64_t nrows, uint32_t *__restrict__ ws_all, uint64_t ws_stride,
                         const unsigned char *__restrict__ w, uint32_t tree_levels) {
    using S = typename F::Sat;
    DYN_SHARED(unsigned char, smem);
    unsigned char *red = smem;                           // the tree's nodes, one element per lane
    uint32_t *lds = reinterpret_cast<uint32_t *>(smem + FOLDED_TREE_BYTES);
    const uint32_t jidx = blockIdx.z * gridDim.y + blockIdx.y;
    const GraphJob job = jobs[jidx];
    const GraphFold fold{coeffs + (size_t)blockIdx.z * ntraces * 48, ntraces, ncols};
    uint32_t *__restrict__ ws = ws_all + (size_t)jidx * ws_stride;
    const uint64_t T = (uint64_t)gridDim.x * blockDim.x, lane = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t nblocks = (nrows + blockDim.x - 1) / blockDim.x;
    for (uint64_t blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {       // uniform over the workgroup
        const uint64_t row = blk * blockDim.x + threadIdx.x;
        Fe<S> leaf = fe_zero<S>();
        if (row < nrows)
            leaf = reduce_once(f29_pack(graph_eval_row<F, true>(job.code, job.ninstr, job.consts29, job.challenges29, job.rotations, cols, nrows, row, lds, job.nlds,
                                                                ws, T, lane, fold)));
        if (!REDUCE) {
            if (row < nrows) fe_store(job.out + row * 32, leaf);
            continue;
        }
        fe_store(red + (size_t)threadIdx.x * 32, leaf);
        __syncthreads();
        Fe<S> acc = leaf;
        for (uint32_t j = 0, width = 1u << tree_levels; j < tree_levels; j++, width >>= 1) {   // as k_pow_tree's levels through LDS
            const bool active = threadIdx.x < (width >> 1);
            if (active) acc = fe_add(fe_load<S>(red + (size_t)(2 * threadIdx.x) * 32), fe_mul(fe_load<S>(red + (size_t)(2 * threadIdx.x + 1) * 32), fe_load<S>(w + (size_t)j * 32)));
            __syncthreads();
            if (active) fe_store(red + (size_t)threadIdx.x * 32, acc);
            __syncthreads();
        }
        if (threadIdx.x == 0) fe_store(job.out + blk * 32, acc);
    }
}
