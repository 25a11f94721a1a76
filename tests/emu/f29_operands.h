// TEST-ONLY (host code): the operands that the column-serial multipliers are compared on, at the limits field29.cuh documents,
// and the calls made with them.  Include field29.cuh first.  Shared by tests/emu/test_f29_column_serial.cpp and tests/gpu/f29_forms.hip.
#pragma once
#include <cstring>
#include <vector>

struct F29Operand {
    uint32_t l[9];
    bool carried;          // limbs 0..7 < 2^29 + 8: what every carrying f29 function returns
    const char *what;
};
enum { F29_FN_MUL = 0, F29_FN_SQR = 1, F29_FN_MUL2_ADD = 2, F29_FN_REDC = 3 };
struct F29Case {
    uint32_t fn;
    uint32_t op[4][9];     // mul: a, b; sqr: a; mul2_add: a, b, c, d; redc: a
};

// k * P with carried limbs
template <class F> inline F29Operand f29_op_kp(uint32_t k, const char *what) {
    F29Operand o{{}, true, what};
    uint64_t carry = 0;
    for (int i = 0; i < 9; i++) {
        uint64_t v = (uint64_t)k * F::P[i] + carry;
        o.l[i] = i < 8 ? (uint32_t)(v & 0x1FFFFFFFu) : (uint32_t)v;
        carry = v >> 29;
    }
    return o;
}
inline F29Operand f29_op_fill(uint32_t limb, bool carried, const char *what) {
    F29Operand o{{}, carried, what};
    for (int i = 0; i < 9; i++) o.l[i] = limb;
    return o;
}
template <class F> inline std::vector<F29Operand> f29_operands() {
    std::vector<F29Operand> v;
    v.push_back(f29_op_fill(0, true, "0"));
    F29Operand one = f29_op_fill(0, true, "1");
    one.l[0] = 1;
    v.push_back(one);
    F29Operand mont = f29_op_fill(0, true, "2^261 mod P");
    for (int i = 0; i < 9; i++) mont.l[i] = F::ONE[i];
    v.push_back(mont);
    v.push_back(f29_op_kp<F>(1, "P"));
    v.push_back(f29_op_kp<F>(2, "2 P"));
    // bound products up to 168: 12 * 14 = 168, 11 * 15 = 165, 13 * 12 = 156, 1 * 168
    v.push_back(f29_op_kp<F>(11, "11 P"));
    v.push_back(f29_op_kp<F>(12, "12 P"));
    v.push_back(f29_op_kp<F>(13, "13 P"));
    v.push_back(f29_op_kp<F>(14, "14 P"));
    v.push_back(f29_op_kp<F>(15, "15 P"));
    v.push_back(f29_op_kp<F>(168, "168 P"));
    v.push_back(f29_op_fill(0x1FFFFFFFu, true, "all limbs 2^29 - 1"));
    v.push_back(f29_op_fill(0x20000007u, true, "all limbs 2^29 + 7"));
    v.push_back(f29_op_fill(0x40000008u, false, "all limbs 2^30 + 8"));
    // f29_sub_nc<7> of a zero minuend, as xyzz29_add_affine negates a coordinate: limbs up to 2^30 + 8
    {
        Fe29<F> p;
        for (int i = 0; i < 9; i++) p.l[i] = F::P[i];
        F29_SET(p, 1.0);
        const Fe29<F> n = f29_sub_nc<7>(f29_zero<F>(), p);
        F29Operand o{{}, false, "f29_sub_nc<7>(0, P)"};
        for (int i = 0; i < 9; i++) o.l[i] = n.l[i];
        v.push_back(o);
    }
    v.push_back(f29_op_fill(3037000499u, false, "all limbs 2^31.5"));       // the NTT budget, against a carried operand only
    uint64_t st = 0x29C0FFEEull + F::P[0];
    static const char *const RANDOM[4] = {"random loose 0", "random loose 1", "random loose 2", "random loose 3"};
    for (int n = 0; n < 4; n++) {
        F29Operand o{{}, true, RANDOM[n]};
        for (int i = 0; i < 9; i++) {
            st = st * 6364136223846793005ull + 1442695040888963407ull;
            o.l[i] = (uint32_t)(st >> 35);                                     // 29 bits
        }
        o.l[8] &= 0x00FFFFFFu;
        v.push_back(o);
    }
    return v;
}
inline uint32_t f29_op_max(const F29Operand &o) {
    uint32_t m = 0;
    for (int i = 0; i < 9; i++) m = o.l[i] > m ? o.l[i] : m;
    return m;
}
// the column budget of field29.cuh (f29_check_columns, f29_check_columns2): products, nine reduction products and a carry
inline bool f29_columns_fit(long double products) {
    return 9.0L * products + 9.0L * 536870912.0L * 536870912.0L + 68719476736.0L < 18446744073709551616.0L;
}
// every call whose columns fit: all pairs for mul, every operand for sqr and redc (redc takes any limbs < 2^32, so it also
// gets all-ones limbs), and for mul2_add every pair of pairs from a shorter list (it documents carried operands and ONE with limbs < 2^30)
template <class F> inline std::vector<F29Case> f29_cases() {
    const std::vector<F29Operand> ops = f29_operands<F>();
    std::vector<F29Case> out;
    auto put = [&](uint32_t fn, const F29Operand *a, const F29Operand *b, const F29Operand *c, const F29Operand *d) {
        F29Case k{};
        k.fn = fn;
        const F29Operand *p[4] = {a, b, c, d};
        for (int n = 0; n < 4; n++)
            for (int i = 0; i < 9; i++) k.op[n][i] = p[n] ? p[n]->l[i] : 0u;
        out.push_back(k);
    };
    for (const F29Operand &a : ops)
        for (const F29Operand &b : ops)
            if (f29_columns_fit((long double)f29_op_max(a) * f29_op_max(b))) put(F29_FN_MUL, &a, &b, nullptr, nullptr);
    for (const F29Operand &a : ops) {
        if (f29_columns_fit((long double)f29_op_max(a) * f29_op_max(a))) put(F29_FN_SQR, &a, nullptr, nullptr, nullptr);
        put(F29_FN_REDC, &a, nullptr, nullptr, nullptr);
    }
    const F29Operand ones = f29_op_fill(0xFFFFFFFFu, false, "all limbs 2^32 - 1");
    put(F29_FN_REDC, &ones, nullptr, nullptr, nullptr);
    // f29_mul2_add: the operands named here, in every combination of four that its contract allows
    static const char *const FEW[] = {"0", "1", "P", "2 P", "12 P", "14 P", "all limbs 2^29 - 1", "all limbs 2^29 + 7", "all limbs 2^30 + 8",
                                      "f29_sub_nc<7>(0, P)", "random loose 0"};
    std::vector<const F29Operand *> few;
    for (const char *name : FEW) {
        const F29Operand *hit = nullptr;
        for (const F29Operand &o : ops)
            if (!strcmp(o.what, name)) hit = &o;
        if (!hit) return {};                                   // a renamed operand: no cases at all, which the tests report
        few.push_back(hit);
    }
    for (const F29Operand *a : few)
        for (const F29Operand *b : few)
            for (const F29Operand *c : few)
                for (const F29Operand *d : few) {
                    const int loose = !a->carried + !b->carried + !c->carried + !d->carried;
                    if (loose <= 1 && f29_columns_fit((long double)f29_op_max(*a) * f29_op_max(*b) + (long double)f29_op_max(*c) * f29_op_max(*d)))
                        put(F29_FN_MUL2_ADD, a, b, c, d);
                }
    return out;
}
