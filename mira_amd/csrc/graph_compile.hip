// The cross-term graph compiler (graph_compile.h): passes over calculations on a flat list of source words, in the order
// compile_graph at the end runs them.
#include "graph_compile.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr uint32_t NONE = 0xFFFFFFFFu;
// compiler-internal calculation: addend + p * q (an ADD that absorbed the single-use MUL feeding it); never accepted from a caller
constexpr uint32_t OP_MAC_INTERNAL = 0xFEu;

struct Calc {
    uint32_t op, nparts;
    size_t first_src, nsrc;   // into the flat source list
};
struct Ir {
    std::vector<Calc> calcs;
    std::vector<uint32_t> srcs;
    uint32_t size() const { return (uint32_t)calcs.size(); }
    const uint32_t *src(uint32_t i) const { return srcs.data() + calcs[i].first_src; }
    void add(uint32_t op, uint32_t nparts, size_t nsrc) { calcs.push_back(Calc{op, nparts, srcs.size(), nsrc}); }
    template <class Remap> void copy_calc(const Ir &from, uint32_t i, Remap remap) {
        const Calc &c = from.calcs[i];
        add(c.op, c.nparts, c.nsrc);
        for (size_t k = 0; k < c.nsrc; k++) srcs.push_back(remap(from.src(i)[k]));
    }
};

bool is_intermediate(uint32_t w) { return src_kind(w) == MIRA_SRC_INTERMEDIATE; }
int bad(const std::string &msg) { set_error(msg); return MIRA_E_BAD_ARG; }

// number of operand words of a calculation, or -1 for an unknown opcode
int operand_count(uint32_t op, uint32_t nparts) {
    switch (op) {
        case MIRA_OP_ADD: case MIRA_OP_SUB: case MIRA_OP_MUL: return 2;
        case MIRA_OP_SQUARE: case MIRA_OP_DOUBLE: case MIRA_OP_NEGATE: case MIRA_OP_STORE: return 1;
        case MIRA_OP_HORNER: return 2 + (int)nparts;
        default: return -1;
    }
}

// the caller's code (include/mira_gpu.h) as calculations, every source checked against what it indexes
int parse(const mira_graph &gr, uint32_t num_challenges, uint32_t num_columns, Ir &ir, std::vector<uint32_t> &used_columns) {
    std::vector<bool> col_used(num_columns, false);
    ir.calcs.reserve(gr.num_calculations);
    size_t pos = 0;
    for (uint32_t i = 0; i < gr.num_calculations; i++) {
        if (pos >= gr.code_words) return bad("graph code ends inside calculation " + std::to_string(i));
        const uint32_t head = gr.code[pos++];
        const uint32_t op = head & 0xFFu, nparts = head >> 8;
        const int cnt = operand_count(op, nparts);
        if (cnt < 0 || (op != MIRA_OP_HORNER && nparts != 0)) return bad("unknown calculation " + std::to_string(head) + " at index " + std::to_string(i));
        if (pos + (size_t)cnt > gr.code_words) return bad("graph code ends inside calculation " + std::to_string(i));
        ir.add(op, nparts, (size_t)cnt);
        for (int k = 0; k < cnt; k++) {
            const uint32_t s = gr.code[pos++];
            const uint32_t kind = src_kind(s), payload = src_payload(s);
            if (kind > MIRA_SRC_CHALLENGE) return bad("unknown value source kind " + std::to_string(kind));
            if (kind == MIRA_SRC_CONSTANT && payload >= gr.num_constants) return bad("constant index out of boundary: " + std::to_string(payload));
            if (kind == MIRA_SRC_INTERMEDIATE && payload >= i) return bad("calculation " + std::to_string(i) + " reads intermediate " + std::to_string(payload) + " before it is written");
            if (kind == MIRA_SRC_CHALLENGE && payload >= num_challenges) return bad("challenge index out of boundary: " + std::to_string(payload));   // EvalError::ChallengeIndexOutOfBoundary
            if (kind == MIRA_SRC_COLUMN) {
                if (col_index(payload) >= num_columns) return bad("column variable index out of boundary: " + std::to_string(col_index(payload)));   // EvalError::ColumnVariableIndexOutOfBoundary
                if (col_rotation(payload) >= gr.num_rotations) return bad("rotation index out of boundary: " + std::to_string(col_rotation(payload)));
                col_used[col_index(payload)] = true;
            }
            ir.srcs.push_back(s);
        }
    }
    if (pos != gr.code_words) return bad("graph code has trailing words");
    for (uint32_t c = 0; c < num_columns; c++)
        if (col_used[c]) used_columns.push_back(c);
    return MIRA_OK;
}

// The skeleton of both rewrite passes: the calculations `gone` marks are dropped, the others keep their order and are
// renumbered.  copy(i, remap, out) appends calculation i, its sources through remap: a read of a kept intermediate gets
// the new number, a read of a dropped one t becomes alias[t].
template <class Copy> Ir rewrite(const Ir &ir, const std::vector<bool> &gone, const std::vector<uint32_t> &alias, Copy copy) {
    Ir out;
    std::vector<uint32_t> new_index(ir.size(), 0);
    auto remap = [&](uint32_t w) {
        if (!is_intermediate(w)) return w;
        const uint32_t t = src_payload(w);
        return gone[t] ? alias[t] : src_word(MIRA_SRC_INTERMEDIATE, new_index[t]);
    };
    for (uint32_t i = 0; i < ir.size(); i++) {
        if (gone[i]) continue;
        new_index[i] = out.size();
        copy(i, remap, out);
    }
    return out;
}

// Constants and challenges that the reference copies into intermediates (Store, graph_evaluator.rs:261-279) are read at
// their uses instead: as direct operands the host can hand each use the form it wants.
Ir inline_stores(const Ir &ir) {
    std::vector<bool> gone(ir.size(), false);
    std::vector<uint32_t> alias(ir.size(), NONE);
    for (uint32_t i = 0; i + 1 < ir.size(); i++) {           // the last calculation is the result: it stays
        const uint32_t w = ir.src(i)[0];
        if (ir.calcs[i].op == MIRA_OP_STORE && (src_kind(w) == MIRA_SRC_CONSTANT || src_kind(w) == MIRA_SRC_CHALLENGE)) { gone[i] = true; alias[i] = w; }
    }
    return rewrite(ir, gone, alias, [&](uint32_t i, auto remap, Ir &out) { out.copy_calc(ir, i, remap); });
}

// Multiply-accumulate fusion.  Gates are sums of products: `acc = acc + c_i * x_i` flattens to MUL, ADD pairs whose product
// is read once, by the ADD.  Folding the MUL into the ADD (one instruction addend + p * q) halves the instruction count of
// such chains, and the running sum then stays in the forwarding register from link to link instead of going through a
// workspace slot while the product is computed.  Not when an operand of the MUL is itself a forwarded value (it would need
// a slot instead); values are exact field elements, so regrouping changes no result.
Ir fuse_mac(const Ir &ir) {
    const uint32_t n = ir.size();
    std::vector<uint32_t> nuses(n, 0);
    for (uint32_t i = 0; i < n; i++)
        for (size_t k = 0; k < ir.calcs[i].nsrc; k++)
            if (is_intermediate(ir.src(i)[k])) nuses[src_payload(ir.src(i)[k])]++;
    std::vector<bool> absorbed(n, false);                    // MUL j is taken by an ADD (its only reader: never remapped)
    std::vector<int> takes(n, -1);                           // ADD i -> which of its operands is the absorbed MUL
    for (uint32_t i = 0; i < n; i++) {
        if (ir.calcs[i].op != MIRA_OP_ADD) continue;
        int best = -1;
        uint32_t best_j = 0;
        for (int k = 0; k < 2; k++) {
            const uint32_t w = ir.src(i)[k];
            if (!is_intermediate(w)) continue;
            const uint32_t j = src_payload(w);
            if (ir.calcs[j].op != MIRA_OP_MUL || nuses[j] != 1 || absorbed[j]) continue;
            bool ok = true;
            for (size_t q = 0; q < 2; q++) {
                const uint32_t o = ir.src(j)[q];
                if (is_intermediate(o) && src_payload(o) + 1 == j && nuses[src_payload(o)] == 1) ok = false;
            }
            if (ok && (best < 0 || j > best_j)) { best = k; best_j = j; }
        }
        if (best >= 0) { takes[i] = best; absorbed[best_j] = true; }
    }
    return rewrite(ir, absorbed, {}, [&](uint32_t i, auto remap, Ir &out) {
        if (takes[i] < 0) { out.copy_calc(ir, i, remap); return; }
        const uint32_t *sum = ir.src(i), *product = ir.src(src_payload(sum[takes[i]]));
        out.add(OP_MAC_INTERNAL, 0, 3);
        out.srcs.insert(out.srcs.end(), {remap(sum[1 - takes[i]]), remap(product[0]), remap(product[1])});
    });
}

// Which form (graph_compile.h) should every calculation's value have, so that as few conversions (one multiplication each)
// as possible are needed?  Columns are form 1, constants and challenges are free, a product's form is the sum of its
// factors' forms, a sum's operands must agree, and the result may leave in any form (the last instruction converts and
// reduces it anyway).  Values whose form can still slide -- products with a free factor, and sums of such -- are elements of
// a union-find with potentials: form = value(element) + offset; meeting a fixed form pins a whole group.  What cannot be
// reconciled (a shared subexpression wanted in two forms, ...) is converted where it is used.
struct FormSolver {
    enum Kind { FREE, FIXED, SLIDING };                      // a constant or challenge; form f; form = val(e) + f
    struct Desc { Kind kind; int f; uint32_t e; };
    static Desc fixed(int f) { return Desc{FIXED, f, 0}; }
    Desc sliding() {                                         // a new group of its own
        parent.push_back((uint32_t)parent.size()); pot.push_back(0); var.push_back(0); res.push_back(0);
        return Desc{SLIDING, 0, (uint32_t)parent.size() - 1};
    }
    int final_form(const Desc &x) { if (x.kind == FIXED) return x.f; int v; pinned(x.e, v); return v + x.f; }   // unpinned groups sit at var 0
    void as_fixed(Desc &x, int want) {                       // pin a sliding value so that its form is `want` (if still possible)
        if (x.kind == SLIDING) { pin(x.e, want - x.f); x = fixed(final_form(x)); }
    }
    Desc add(Desc x, Desc y) {
        if (x.kind == FREE && y.kind == FREE) return sliding();
        if (x.kind == FREE) return y;
        if (y.kind == FREE) return x;
        settle(x); settle(y);
        if (x.kind == FIXED && y.kind == FIXED) return x;
        if (x.kind == FIXED) { as_fixed(y, x.f); return x; }
        if (y.kind == FIXED) { as_fixed(x, y.f); return y; }
        unite(x.e, y.e, x.f - y.f);                          // val(y.e) + y.f = val(x.e) + x.f
        return x;
    }
    Desc mul(Desc x, Desc y) {
        if (x.kind == FREE || y.kind == FREE) return sliding();   // a free factor: the product can have any form
        settle(x); settle(y);
        if (x.kind == SLIDING && y.kind == SLIDING) as_fixed(y, 0);
        if (x.kind == FIXED && y.kind == FIXED) return fixed(x.f + y.f);
        if (x.kind == FIXED) return Desc{SLIDING, y.f + x.f, y.e};
        return Desc{SLIDING, x.f + y.f, x.e};
    }
    std::vector<uint32_t> parent;
    std::vector<int> pot, var;                               // pot = val(x) - val(parent); var of a resolved root
    std::vector<char> res;
    uint32_t find(uint32_t x, int &p) {                      // root of x, p = val(x) - val(root)
        p = 0;
        uint32_t r = x;
        while (parent[r] != r) { p += pot[r]; r = parent[r]; }
        uint32_t y = x; int acc = p;                         // path compression
        while (parent[y] != y) { const uint32_t nx = parent[y]; const int py = pot[y]; parent[y] = r; pot[y] = acc; acc -= py; y = nx; }
        return r;
    }
    void pin(uint32_t e, int value) {                        // val(e) := value unless the group is pinned already
        int p; const uint32_t r = find(e, p);
        if (!res[r]) { res[r] = 1; var[r] = value - p; }
    }
    bool pinned(uint32_t e, int &value) { int p; const uint32_t r = find(e, p); value = var[r] + p; return (bool)res[r]; }
    void settle(Desc &x) { int v; if (x.kind == SLIDING && pinned(x.e, v)) x = fixed(v + x.f); }   // a pinned group is a fixed form
    void unite(uint32_t a, uint32_t b, int d) {              // val(b) = val(a) + d, if both groups can still move
        int pa, pb; const uint32_t ra = find(a, pa), rb = find(b, pb);
        if (ra == rb) return;
        if (res[ra] && res[rb]) return;
        if (res[rb]) { parent[ra] = rb; pot[ra] = pb - d - pa; }   // val(ra) = val(rb) + pb - d - pa
        else { parent[rb] = ra; pot[rb] = pa + d - pb; }
    }
};

std::vector<int> infer_forms(const Ir &ir) {
    using Desc = FormSolver::Desc;
    FormSolver fs;
    std::vector<Desc> desc(ir.size());
    auto operand = [&](uint32_t w) -> Desc {
        if (is_intermediate(w)) return desc[src_payload(w)];
        if (src_kind(w) == MIRA_SRC_COLUMN) return FormSolver::fixed(1);
        return Desc{FormSolver::FREE, 0, 0};
    };
    for (uint32_t i = 0; i < ir.size(); i++) {
        const uint32_t *w = ir.src(i);
        Desc r;
        switch (ir.calcs[i].op) {
            case MIRA_OP_ADD: case MIRA_OP_SUB: r = fs.add(operand(w[0]), operand(w[1])); break;
            case MIRA_OP_MUL: r = fs.mul(operand(w[0]), operand(w[1])); break;
            case MIRA_OP_SQUARE: { Desc x = operand(w[0]); if (x.kind == FormSolver::FREE) r = fs.sliding(); else { fs.as_fixed(x, 0); r = FormSolver::fixed(2 * fs.final_form(x)); } break; }
            case MIRA_OP_DOUBLE: case MIRA_OP_NEGATE: case MIRA_OP_STORE: { Desc x = operand(w[0]); r = x.kind == FormSolver::FREE ? fs.sliding() : x; break; }
            case OP_MAC_INTERNAL: r = fs.add(operand(w[0]), fs.mul(operand(w[1]), operand(w[2]))); break;
            default:                                         // HORNER: value = value * factor + part
                r = operand(w[0]);
                if (r.kind == FormSolver::FREE) r = fs.sliding();
                for (uint32_t k = 0; k < ir.calcs[i].nparts; k++) r = fs.add(fs.mul(r, operand(w[1])), operand(w[2 + k]));
                break;
        }
        desc[i] = r;
    }
    std::vector<int> form_of(ir.size());
    for (uint32_t i = 0; i < ir.size(); i++) form_of[i] = fs.final_form(desc[i]);
    return form_of;
}

// an operand as the emitter sees it: the word the kernel fetches, a proven bound, and its form (free: any)
struct Opnd { uint32_t w; double b; int f; bool free, prev; };
constexpr uint32_t PREV = src_word(GRAPH_SRC_PREV, 0);

// The instruction stream, with a proven bound (in multiples of P) for every value, and the constants and challenges in the
// forms their uses want.  What an instruction computes is the forwarded value of the next one; the emitting calls return
// its bound.
struct Emitter {
    std::vector<uint32_t> stream;
    std::vector<std::pair<int, int>> pool;
    std::vector<std::pair<uint32_t, int>> chal_vars;
    uint32_t ninstr = 0;
    size_t last_head = 0;                                    // stream index of the most recent instruction

    static uint32_t bcode(double b) { return (uint32_t)std::min(65535.0, std::ceil(b * 256.0)); }
    // one instruction on resolved sources sa, sb with proven bounds ba, bb
    double emit(uint32_t op, uint32_t sa, double ba, uint32_t sb, double bb) {
        uint32_t K = 0;
        double rb = 0;
        const bool binary = gop_operands(op) == 2;
        auto bias = [](double b2) { return b2 < 1.99 ? 2u : b2 < 3.99 ? 4u : b2 < 7.99 ? 8u : 16u; };   // f29_sub<K> needs the subtrahend below K P
        switch (op) {
            case GOP_ADD: rb = ba + bb; break;
            case GOP_SUB: K = bias(bb); rb = ba + K; break;
            case GOP_NEG: K = bias(ba); rb = K; break;
            case GOP_MUL: rb = ba * bb / 168.9 + 1.0; break;
            case GOP_SQR: rb = ba * ba / 168.9 + 1.0; break;
            case GOP_DBL: rb = 2 * ba; break;
            case GOP_NORM: rb = ba / 168.9 + 1.0; break;
            default: rb = ba; break;
        }
        last_head = stream.size();
        stream.insert(stream.end(), {gop_head(op, K), GRAPH_NO_SLOT, bcode(ba) | bcode(binary ? bb : 0.0) << 16, sa});
        if (binary) stream.push_back(sb);
        ninstr++;
        return rb;
    }
    // addend + p * q
    double emit_mac(uint32_t sc, double bc, uint32_t sp, double bp, uint32_t sq, double bq) {
        last_head = stream.size();
        stream.insert(stream.end(), {GOP_MAC, GRAPH_NO_SLOT, bcode(bp) | bcode(bq) << 16, sp, sq, sc, bcode(bc)});
        ninstr++;
        return bp * bq / 168.9 + 1.0 + bc;
    }
    // constant ci (-1: the number one) in the given form
    uint32_t pool_word(int ci, int form) { return src_word(MIRA_SRC_CONSTANT, entry(pool, std::make_pair(ci, form))); }
    uint32_t chal_word(uint32_t ch, int form) { return src_word(MIRA_SRC_CHALLENGE, entry(chal_vars, std::make_pair(ch, form))); }
    template <class T> static uint32_t entry(std::vector<T> &v, const T &x) {
        for (size_t k = 0; k < v.size(); k++)
            if (v[k] == x) return (uint32_t)k;
        v.push_back(x);
        return (uint32_t)(v.size() - 1);
    }
    void materialise(Opnd &x, int form) {                    // a free operand in the given form
        if (!x.free) return;
        x.w = src_kind(x.w) == MIRA_SRC_CONSTANT ? pool_word((int)src_payload(x.w), form) : chal_word(src_payload(x.w), form);
        x.f = form; x.free = false;
    }
    double convert_prev(double b, int from, int to) {       // the forwarded value into another form: times the number one in form to - from
        return from == to ? b : emit(GOP_MUL, PREV, b, pool_word(-1, to - from), 1.0);
    }
    void convert(Opnd &x, int to) {                          // any fixed operand into form `to`: the result is the forwarded value
        x.b = emit(GOP_MUL, x.w, x.b, pool_word(-1, to - x.f), 1.0);
        x.w = PREV; x.prev = true; x.f = to;
    }
    // x (+ / -) y in form `target`
    double addsub(uint32_t op, Opnd x, Opnd y, int target) {
        int F;
        if (x.free && y.free) F = target;
        else if (x.free) F = y.f;
        else if (y.free) F = x.f;
        else if (x.f == y.f) F = x.f;
        else if (x.prev) { convert(x, y.f); F = y.f; }        // never convert the OTHER operand while one sits in the forwarding register
        else if (y.prev) { convert(y, x.f); F = x.f; }
        else { convert(y, x.f); F = x.f; }
        materialise(x, F); materialise(y, F);
        return convert_prev(emit(op, x.w, x.b, y.w, y.b), F, target);
    }
    void fit_product(Opnd &x, Opnd &y, int target) {         // free factors of x * y in the forms that make it form `target`
        if (x.free && y.free) { materialise(x, target); materialise(y, 0); }
        else if (x.free) materialise(x, target - y.f);
        else if (y.free) materialise(y, target - x.f);
    }
    double mul(Opnd x, Opnd y, int target) {
        fit_product(x, y, target);
        return convert_prev(emit(GOP_MUL, x.w, x.b, y.w, y.b), x.f + y.f, target);
    }
    // c + pq * q in form T
    double mac(Opnd c, Opnd pq, Opnd q, int T) {
        const bool free_factor = pq.free || q.free;
        const int fp = free_factor ? 0 : pq.f + q.f;         // the product's form, if it is not ours to choose
        if (c.free || free_factor) {                         // a constant addend takes the product's form, a free factor makes the product meet the addend
            const int F = !c.free ? c.f : free_factor ? T : fp;
            fit_product(pq, q, F);
            materialise(c, F);
            return convert_prev(emit_mac(c.w, c.b, pq.w, pq.b, q.w, q.b), F, T);
        }
        if (fp == c.f || c.prev) {                           // a forwarded addend is brought to the product's form: IT is in the register
            if (c.f != fp) convert(c, fp);
            return convert_prev(emit_mac(c.w, c.b, pq.w, pq.b, q.w, q.b), fp, T);
        }
        const double bp = emit(GOP_MUL, pq.w, pq.b, q.w, q.b);   // product first (a factor may be the forwarded value), then the sum
        return addsub(GOP_ADD, Opnd{PREV, bp, fp, false, true}, c, T);
    }
    // start, factor, parts[] (graph_evaluator.rs:148-155): value = value * factor + part, in form T
    double horner(std::vector<Opnd> &o, uint32_t nparts, int T) {
        materialise(o[0], T);
        double rb = emit(GOP_COPY, o[0].w, o[0].b, 0, 0);
        int fv = o[0].f;
        for (uint32_t k = 0; k < nparts; k++) {
            Opnd part = o[2 + k];
            const int want = part.free ? T : part.f;         // the product in the form of the part it meets
            rb = mul(Opnd{PREV, rb, fv, false, true}, o[1], o[1].free ? want : fv + o[1].f);
            fv = o[1].free ? want : fv + o[1].f;
            rb = addsub(GOP_ADD, Opnd{PREV, rb, fv, false, true}, part, part.free ? fv : part.f);
            fv = part.free ? fv : part.f;
            if (rb > GRAPH_MAX_BOUND) rb = emit(GOP_NORM, PREV, rb, 0, 0);
        }
        return convert_prev(rb, fv, T);
    }
};

// The reference keeps one intermediate per calculation (graph_evaluator.rs:354-359).  Most die young: slots are handed out
// by last use, so a 300-calculation gate needs ~10-20 of them.  Returns the number of slots.
uint32_t lower(const Ir &ir, const std::vector<int> &form_of, Emitter &em) {
    const uint32_t n = ir.size();
    // readers of every intermediate; the final calculation's value leaves through `out`
    std::vector<uint32_t> last_use(n, 0), first_use(n, NONE);
    for (uint32_t i = 0; i < n; i++)
        for (size_t k = 0; k < ir.calcs[i].nsrc; k++) {
            const uint32_t w = ir.src(i)[k];
            if (is_intermediate(w)) { last_use[src_payload(w)] = i; first_use[src_payload(w)] = std::min(first_use[src_payload(w)], i); }
        }
    // a value read only by the next calculation is forwarded in registers; the rest get a slot from their definition to
    // their last reader.  (HORNER expands to several instructions, each of which moves the forwarding register on: its
    // operands always come from slots.)
    auto used = [&](uint32_t t) { return first_use[t] != NONE; };
    auto reads_of = [&](uint32_t i, uint32_t t) {            // how often calculation i reads intermediate t
        uint32_t c = 0;
        for (size_t k = 0; k < ir.calcs[i].nsrc; k++) c += ir.src(i)[k] == src_word(MIRA_SRC_INTERMEDIATE, t);
        return c;
    };
    // (read ONCE: a form conversion of one operand moves the forwarding register on, a second read would see the converted value)
    auto forwarded = [&](uint32_t t) {
        return used(t) && first_use[t] == t + 1 && last_use[t] == t + 1 && ir.calcs[t + 1].op != MIRA_OP_HORNER && reads_of(t + 1, t) == 1;
    };
    std::vector<uint32_t> slot_of(n, GRAPH_NO_SLOT), free_slots;
    std::vector<double> bound_of(n, 0.0);                    // proven bound of every calculation's value
    std::vector<std::vector<uint32_t>> dying(n);
    for (uint32_t t = 0; t < n; t++)
        if (used(t) && !forwarded(t)) dying[last_use[t]].push_back(t);
    auto resolve = [&](uint32_t w) -> Opnd {                 // intermediates become slots or the forwarded register
        if (is_intermediate(w)) {
            const uint32_t t = src_payload(w);
            return Opnd{forwarded(t) ? PREV : src_word(MIRA_SRC_INTERMEDIATE, slot_of[t]), bound_of[t], form_of[t], false, forwarded(t)};
        }
        if (src_kind(w) == MIRA_SRC_COLUMN) return Opnd{w, 1.0, 1, false, false};   // canonical, in the reference's form
        return Opnd{w, 1.0, 0, true, false};                 // constants and challenges are canonical in whatever form they are asked for
    };
    uint32_t nslots = 0;
    for (uint32_t i = 0; i < n; i++) {
        std::vector<Opnd> o(ir.calcs[i].nsrc);
        for (size_t k = 0; k < o.size(); k++) o[k] = resolve(ir.src(i)[k]);
        const int T = form_of[i];
        double rb;
        switch (ir.calcs[i].op) {
            case MIRA_OP_ADD: rb = em.addsub(GOP_ADD, o[0], o[1], T); break;
            case MIRA_OP_SUB: rb = em.addsub(GOP_SUB, o[0], o[1], T); break;
            case MIRA_OP_MUL: rb = em.mul(o[0], o[1], T); break;
            case MIRA_OP_SQUARE:
                if (o[0].free) em.materialise(o[0], T % 2 == 0 ? T / 2 : 0);
                rb = em.convert_prev(em.emit(GOP_SQR, o[0].w, o[0].b, 0, 0), 2 * o[0].f, T);
                break;
            case MIRA_OP_DOUBLE: case MIRA_OP_NEGATE: case MIRA_OP_STORE: {
                em.materialise(o[0], T);
                const uint32_t gop = ir.calcs[i].op == MIRA_OP_DOUBLE ? GOP_DBL : ir.calcs[i].op == MIRA_OP_NEGATE ? GOP_NEG : GOP_COPY;
                rb = em.convert_prev(em.emit(gop, o[0].w, o[0].b, 0, 0), o[0].f, T);
                break;
            }
            case OP_MAC_INTERNAL: rb = em.mac(o[0], o[1], o[2], T); break;
            default: rb = em.horner(o, ir.calcs[i].nparts, T); break;
        }
        if (rb > GRAPH_MAX_BOUND) rb = em.emit(GOP_NORM, PREV, rb, 0, 0);   // keep the invariant: stored and forwarded values < 12 P
        if (i + 1 == n) rb = em.emit(GOP_MUL, PREV, rb, em.pool_word(-1, 1 - T), 1.0);   // the result: into the reference's form, below 2 P (the kernel stores it canonical)
        bound_of[i] = rb;
        // operands are in registers before the result is written: a slot that dies here can take it
        for (uint32_t t : dying[i]) free_slots.push_back(slot_of[t]);
        if (used(i) && !forwarded(i)) {
            if (free_slots.empty()) free_slots.push_back(nslots++);
            slot_of[i] = free_slots.back();
            free_slots.pop_back();
            em.stream[em.last_head + 1] = slot_of[i];            // the calculation's last instruction writes the slot
        }
    }
    return nslots;
}

// Renumber the slots by how often the program touches them, most used first: the kernel keeps the lowest-numbered ones in
// LDS (graph.hip: GRAPH_LDS_SLOTS_*) and the rest in the global workspace.
void renumber_slots(std::vector<uint32_t> &stream, uint32_t nslots) {
    std::vector<uint64_t> uses(nslots, 0);
    for_each_instruction(stream.data(), stream.size(), [&](const uint32_t *ins) {
        if (ins[1] != GRAPH_NO_SLOT) uses[ins[1]]++;
        for (uint32_t k = 0; k < gop_operands(gop_op(ins[0])); k++)
            if (is_intermediate(ins[3 + k])) uses[src_payload(ins[3 + k])]++;
    });
    std::vector<uint32_t> order(nslots), rank(nslots);
    for (uint32_t i = 0; i < nslots; i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return uses[a] > uses[b]; });
    for (uint32_t i = 0; i < nslots; i++) rank[order[i]] = i;
    for_each_instruction(stream.data(), stream.size(), [&](uint32_t *ins) {
        if (ins[1] != GRAPH_NO_SLOT) ins[1] = rank[ins[1]];
        for (uint32_t k = 0; k < gop_operands(gop_op(ins[0])); k++)
            if (is_intermediate(ins[3 + k])) ins[3 + k] = src_word(MIRA_SRC_INTERMEDIATE, rank[src_payload(ins[3 + k])]);
    });
}

}   // namespace

int compile_graph(const mira_graph &gr, uint32_t num_challenges, uint32_t num_columns, CompiledGraph &out) {
    Ir ir;
    if (int rc = parse(gr, num_challenges, num_columns, ir, out.used_columns)) return rc;
    ir = fuse_mac(inline_stores(ir));
    Emitter em;
    out.nslots = lower(ir, infer_forms(ir), em);
    renumber_slots(em.stream, out.nslots);
    out.stream = std::move(em.stream);
    out.ninstr = em.ninstr;
    out.pool = std::move(em.pool);
    out.chal_vars = std::move(em.chal_vars);
    return MIRA_OK;
}
