// The compiled instruction stream of a cross-term graph: what graph_compile.hip writes, k_graph_eval (graph_kernels.cuh)
// interprets and graph_jit.hpp writes out as a kernel of its own.  Per instruction
//   [op | K << 8]  [dst slot]  [bounds of a and b in 1/256 P: lo 16 | hi 16 bits]  [source a]  ([source b])
// and for GOP_MAC (a * b + c: an addition that absorbed the product feeding it, graph_compile.hip) two more: [source c] [bound of c]
// A source is kind << 29 | payload, the kinds of include/mira_gpu.h (MIRA_SRC_*) and GRAPH_SRC_PREV = the value of the
// instruction just before (still in registers -- most results of a post-order expression walk are consumed by the very next
// instruction and never touch the workspace).  INTERMEDIATE payloads are slots; a COLUMN payload is column | rotation << 20.
// K = the multiple of P a subtraction adds.  The bounds word only feeds the test build's bound bookkeeping (F29_TRACK).
#pragma once
#include "platform.h"
#include "../../include/mira_gpu.h"

static constexpr uint32_t GRAPH_SRC_PREV = 4u;
static constexpr uint32_t GRAPH_NO_SLOT = 0xFFFFFFFFu;
static constexpr uint32_t GOP_ADD = 0, GOP_SUB = 1, GOP_MUL = 2, GOP_SQR = 3, GOP_DBL = 4, GOP_NEG = 5, GOP_COPY = 6, GOP_NORM = 7, GOP_MAC = 8;
static constexpr double GRAPH_MAX_BOUND = 12.0;          // of every stored or forwarded value, in multiples of P

HD constexpr uint32_t src_word(uint32_t kind, uint32_t payload) { return kind << 29 | payload; }
HD constexpr uint32_t src_kind(uint32_t w) { return w >> 29; }
HD constexpr uint32_t src_payload(uint32_t w) { return w & 0x1FFFFFFFu; }
HD constexpr uint32_t col_index(uint32_t payload) { return payload & 0xFFFFFu; }
HD constexpr uint32_t col_rotation(uint32_t payload) { return payload >> 20; }

HD constexpr uint32_t gop_head(uint32_t op, uint32_t K) { return op | K << 8; }
HD constexpr uint32_t gop_op(uint32_t head) { return head & 0xFFu; }
HD constexpr uint32_t gop_bias(uint32_t head) { return head >> 8; }
HD constexpr uint32_t gop_operands(uint32_t op) { return op == GOP_MAC ? 3u : (op == GOP_ADD || op == GOP_SUB || op == GOP_MUL) ? 2u : 1u; }
HD constexpr uint32_t gop_words(uint32_t op) { return 3u + gop_operands(op) + (op == GOP_MAC ? 1u : 0u); }

// f(words of the instruction) for every instruction of a stream of n words, in order
template <class W, class F> inline void for_each_instruction(W *stream, size_t n, F f) {
    for (size_t pos = 0; pos < n; pos += gop_words(gop_op(stream[pos]))) f(stream + pos);
}
