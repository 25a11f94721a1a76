// The cross-term graph compiler (mira_amd/csrc/graph_compile.hip) on the host, on its own: compiles every graph of the case
// file tests/test_graph_compile_host.py writes (one per line: name field calculations constants challenges columns, the
// rotations and the code words, each list preceded by its length) and prints what came out.  The test compares the output
// with tests/golden/graph_compile.txt.
#include <cstdio>
#include <fstream>
#include <sstream>

#include "../../mira_amd/csrc/graph_compile.h"
#include "../../mira_amd/csrc/graph_jit.hpp"

static std::string g_error;
void set_error(const std::string &s) { g_error = s; }

static uint64_t fnv1a(const void *p, size_t n) {
    const unsigned char *b = static_cast<const unsigned char *>(p);
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 0x100000001b3ull; }
    return h;
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s <case file>\n", argv[0]); return 2; }
    std::ifstream in(argv[1]);
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        std::string name;
        int field;
        uint32_t ncalc, nconst, nchal, ncols, nrot;
        size_t ncode;
        ss >> name >> field >> ncalc >> nconst >> nchal >> ncols >> nrot;
        std::vector<int32_t> rots(nrot);
        for (auto &r : rots) ss >> r;
        ss >> ncode;
        std::vector<uint32_t> code(ncode);
        for (auto &w : code) ss >> w;
        if (!ss) { fprintf(stderr, "malformed case: %s\n", line.c_str()); return 2; }
        const mira_graph gr{code.data(), code.size(), ncalc, nconst, nullptr, rots.data(), nrot, 0};
        printf("graph %s\n", name.c_str());
        CompiledGraph cg;
        const int rc = compile_graph(gr, nchal, ncols, cg);
        if (rc) { printf("error %d %s\n", rc, g_error.c_str()); continue; }
        printf("ninstr %u nslots %u\nused_columns", cg.ninstr, cg.nslots);
        for (uint32_t c : cg.used_columns) printf(" %u", c);
        printf("\npool");
        for (auto &p : cg.pool) printf(" %d:%d", p.first, p.second);
        printf("\nchal_vars");
        for (auto &cv : cg.chal_vars) printf(" %u:%d", cv.first, cv.second);
        printf("\n");
        if (cg.ninstr <= 64) {
            uint32_t i = 0;
            for_each_instruction(cg.stream.data(), cg.stream.size(), [&](const uint32_t *ins) {
                printf("i%u", i++);
                for (uint32_t k = 0; k < gop_words(gop_op(ins[0])); k++) printf(" %08x", ins[k]);
                printf("\n");
            });
        } else {
            printf("stream %zu words fnv1a64 %016llx\n", cg.stream.size(), (unsigned long long)fnv1a(cg.stream.data(), cg.stream.size() * 4));
        }
        if (cg.ninstr) {                                     // the kernel source, all columns field elements / the first two selectors
            std::vector<uint32_t> kinds(ncols, MIRA_COL_FIELD);
            const std::string a = graphjit::source(field, cg.stream, rots, kinds);
            for (uint32_t c = 0; c < ncols && c < 2; c++) kinds[c] = MIRA_COL_BOOL;
            const std::string b = graphjit::source(field, cg.stream, rots, kinds);
            printf("jit fields %016llx selectors %016llx\n", (unsigned long long)fnv1a(a.data(), a.size()), (unsigned long long)fnv1a(b.data(), b.size()));
        }
    }
    return 0;
}
