// The cross-term graph compiler (graph_compile.hip): a flattened GraphEvaluator (include/mira_gpu.h) in, the instruction
// stream of graph_stream.h out.  Host code only: it allocates nothing on the device and launches nothing; graph.hip uploads
// what it decides.
//
// Forms.  The kernel's multiplier divides by 2^261, so a value x is carried as x * 2^(261 - 5 f) for some integer f, its FORM:
// f = 0 is the multiplier's own Montgomery form (closed under multiplication), f = 1 is the reference's memory layout
// x * 2^256 -- a column as it is read, no lifting product -- and the product of forms f1 and f2 has form f1 + f2; sums need
// equal forms.  Constants and challenges are converted on the host to whatever form their use wants (graph.hip: to_limbs29).
#pragma once
#include <string>
#include <utility>
#include <vector>

#include "graph_stream.h"

void set_error(const std::string &s);

struct CompiledGraph {
    std::vector<uint32_t> stream;                        // ninstr instructions (graph_stream.h)
    uint32_t ninstr = 0, nslots = 0;
    std::vector<std::pair<int, int>> pool;               // CONSTANT payloads: (constant index, or -1 for the number one; form)
    std::vector<std::pair<uint32_t, int>> chal_vars;     // CHALLENGE payloads: (challenge, form), converted per evaluation
    std::vector<uint32_t> used_columns;                  // column indices the code reads, ascending
};

// MIRA_OK, or MIRA_E_BAD_ARG (message through set_error) for malformed code or an index out of bounds
int compile_graph(const mira_graph &gr, uint32_t num_challenges, uint32_t num_columns, CompiledGraph &out);
