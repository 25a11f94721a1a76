// The two rounds of the lookup argument that the reference computes on the host between two commits of one fold step
// (src/plonk/lookup.rs:278-321, called from run_sps_protocol_2 / _3, src/plonk/mod.rs:745-800, 846-905):
//
//   evaluate_m    m_i = #{j : l_j = t_i} at the first occurrence of t_i's value in t, else 0      (a HashMap there)
//   evaluate_h_g  h_i = 1 / (l_i + r),  g_i = m_i / (t_i + r),  0 where the denominator is 0    (one inversion per element)
//
// Batch inversion (Montgomery's trick, applied as a tree of launches).  Level 0 holds the n denominators; lane j of G lanes
// takes elements j, j + G, j + 2G, ... (K of them, coalesced), stores the exclusive prefix products of its non-zero ones and
// hands its lane total up as one element of level 1, and so on until one workgroup holds the rest (k_inv_top): it multiplies
// its lanes' totals up a tree in LDS, lane 0 raises the root to p - 2 -- the ONE Fermat chain of the call -- and the inverse
// walks back down the tree and then down every level: out_i = (inverse of the lane's running product) * prefix_i.  3 products
// per element plus that chain; zeros are skipped on the way up and written as 0 on the way down.
//
// Arithmetic: the Fe29 multiplier (R' = 2^261).  A reference element x * 2^256 is read as the Fe29 integer it is, i.e. as the
// value x / 32 in R' form; the root's inverse is scaled once by 2^-10 (R' form: the integer 2^251), which makes every inverse
// that comes out x^-1 * 2^256 -- the reference layout, with no conversion per element.  Level >= 1 values and the prefix
// products are stored as the 256-bit integers of loose Fe29 values (< 2 P).
//
// Multiplicities: an open-addressing table of capacity C = 2^c >= 2 n_t, slot = (owner, first, count).  owner = index + 1 of
// a t element that holds the slot's value (0 = empty; claimed by compare-and-swap and never changed again), first = lowest
// index with that value (atomic minimum), count = occurrences in l (atomic addition).  The keys are the immutable inputs
// themselves (t[owner - 1]), so nothing but the owner word is ever published.  Every result is a minimum or a sum of
// integers, so it does not depend on the order the lanes ran in.
#pragma once
#include "field29.cuh"

enum LookupErr : uint32_t { LK_ERR_NONCANONICAL = 1, LK_ERR_TABLE_FULL = 2 };

template <class FP> DEV bool lk_is_canonical(const Fe<FP> &a) {
    Fe<FP> t;
    return sub_p(t, a) != 0;   // a - P borrows
}
// a loose Fe29 straight out of the multiplier (limbs 0 .. 7 masked, value < 2 P < 2^255) as a 256-bit integer, and back
template <class F> DEV void inv_store(unsigned char *p, const Fe29<F> &v) { fe_store(p, f29_pack_product(v)); }
template <class F> DEV Fe29<F> inv_load(const unsigned char *p) {
    Fe29<F> r = f29_unpack<F>(fe_load<typename F::Sat>(p));
    F29_SET(r, 2.0);
    return r;
}
template <class F> DEV Fe<typename F::Sat> lk_canonical(const Fe29<F> &v) { return reduce_once(f29_pack(v)); }

// ---- level 0: the denominators of one call ------------------------------------------------------------------------------
// element i < n0: in[0][i] + r -> out[0][i];  n0 <= i < n: in[1][i - n0] + r -> out[1][i - n0], times mul1[i - n0] when set
struct InvLevel0 {
    const unsigned char *in[2];
    unsigned char *out[2];
    unsigned char *pre[2];          // exclusive prefix products (may be out: each element is read there before it is written)
    const unsigned char *mul1;      // g = m / (t + r); null for a plain inversion
    uint64_t n0, n;
    uint32_t r[8];                  // added to every input element (canonical; zero for a plain inversion)
    bool add_r;
};
template <class F> struct InvAcc0 {
    using S = typename F::Sat;
    const InvLevel0 d;
    DEV uint64_t n() const { return d.n; }
    // false: the denominator is zero
    DEV bool load(uint64_t i, Fe29<F> &x, uint32_t *err) const {
        Fe<S> v = fe_load<S>(i < d.n0 ? d.in[0] + i * 32 : d.in[1] + (i - d.n0) * 32);
        if (!lk_is_canonical(v)) {
            if (err) atomicMax(err, (uint32_t)LK_ERR_NONCANONICAL);
            v = fe_zero<S>();
        }
        if (d.add_r) {
            Fe<S> r;
#pragma unroll
            for (int k = 0; k < 8; k++) r.l[k] = d.r[k];
            v = fe_add(v, r);
        }
        if (fe_is_zero(v)) return false;
        x = f29_unpack_canonical<F>(v);
        return true;
    }
    DEV unsigned char *pre_at(uint64_t i) const { return i < d.n0 ? d.pre[0] + i * 32 : d.pre[1] + (i - d.n0) * 32; }
    DEV void store_pre(uint64_t i, const Fe29<F> &e) const { inv_store(pre_at(i), e); }
    DEV Fe29<F> load_pre(uint64_t i) const { return inv_load<F>(pre_at(i)); }
    DEV void store_out(uint64_t i, const Fe29<F> *v, uint32_t *err) const {
        if (i < d.n0) {
            fe_store(d.out[0] + i * 32, v ? lk_canonical(*v) : fe_zero<S>());
            return;
        }
        const uint64_t j = i - d.n0;
        if (!v) {
            fe_store(d.out[1] + j * 32, fe_zero<S>());
            return;
        }
        Fe29<F> w = *v;
        if (d.mul1) {
            const Fe<S> m = fe_load<S>(d.mul1 + j * 32);
            if (!lk_is_canonical(m)) atomicMax(err, (uint32_t)LK_ERR_NONCANONICAL);
            w = f29_mul(w, f29_from_r256<F>(m));           // (x^-1 2^256) (m 2^261) 2^-261 = m x^-1 2^256
        }
        fe_store(d.out[1] + j * 32, lk_canonical(w));
    }
};
// ---- level >= 1: the lane totals of the level below, inverted in place -------------------------------------------------
struct InvLevelN {
    unsigned char *vals;
    unsigned char *pre;
    uint64_t n;
};
template <class F> struct InvAccN {
    const InvLevelN d;
    DEV uint64_t n() const { return d.n; }
    DEV bool load(uint64_t i, Fe29<F> &x, uint32_t *) const {   // products of non-zero elements (or 1): never zero
        x = inv_load<F>(d.vals + i * 32);
        return true;
    }
    DEV void store_pre(uint64_t i, const Fe29<F> &e) const { inv_store(d.pre + i * 32, e); }
    DEV Fe29<F> load_pre(uint64_t i) const { return inv_load<F>(d.pre + i * 32); }
    DEV void store_out(uint64_t i, const Fe29<F> *v, uint32_t *) const { inv_store(d.vals + i * 32, *v); }
};

// lane j of G: the product of its non-zero elements (1 if none), exclusive prefix products stored on the way
template <class F, class A> DEV Fe29<F> inv_up(const A &a, uint64_t j, uint64_t G, uint32_t *err) {
    Fe29<F> acc = f29_one<F>();
    for (uint64_t i = j; i < a.n(); i += G) {
        Fe29<F> x;
        if (!a.load(i, x, err)) continue;
        a.store_pre(i, acc);
        acc = f29_mul(acc, x);
    }
    return acc;
}
// ... and back: inv = (scaled) inverse of that product
template <class F, class A> DEV void inv_down(const A &a, uint64_t j, uint64_t G, Fe29<F> inv, uint32_t *err) {
    if (j >= a.n()) return;
    for (uint64_t i = j + (a.n() - 1 - j) / G * G;; i -= G) {
        Fe29<F> x;
        if (a.load(i, x, nullptr)) {
            const Fe29<F> v = f29_mul(inv, a.load_pre(i));
            a.store_out(i, &v, err);
            inv = f29_mul(inv, x);
        } else {
            a.store_out(i, nullptr, err);
        }
        if (i == j) break;
    }
}

template <class F, class Lv, template <class> class Acc>
KERNEL void k_inv_up(Lv lv, uint64_t G, unsigned char *__restrict__ totals, uint32_t *err) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= G) return;
    const Acc<F> a{lv};
    inv_store(totals + j * 32, inv_up<F>(a, j, G, err));
}
template <class F, class Lv, template <class> class Acc>
KERNEL void k_inv_down(Lv lv, uint64_t G, const unsigned char *__restrict__ inv_totals, uint32_t *err) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= G) return;
    const Acc<F> a{lv};
    inv_down<F>(a, j, G, inv_load<F>(inv_totals + j * 32), err);
}

// bit k of P - 2 (P[0] >= 2: no borrow).  The words are compile-time constants: a select chain, no memory access inside the chain
template <class F> DEV uint32_t inv_exp_bit(int k) {
    uint32_t w = F::Sat::P[0] - 2u;
#pragma unroll
    for (int q = 1; q < 8; q++)
        if ((k >> 5) == q) w = F::Sat::P[q];
    return (w >> (k & 31)) & 1u;
}
// x^(P - 2) by 5-bit sliding windows over the odd powers x, x^3, .., x^31 (tab: 16 entries): 253 squarings and 53 (Fq) / 56 (Fr)
// multiplications, table included, against 109 / 126 for plain square-and-multiply.  One lane.
template <class F> DEV Fe29<F> inv_fermat(const Fe29<F> &x, Fe29<F> *tab) {
    tab[0] = x;
    const Fe29<F> x2 = f29_sqr(x);
    for (int k = 1; k < 16; k++) tab[k] = f29_mul(tab[k - 1], x2);
    Fe29<F> acc = f29_one<F>();
    bool started = false;
    int i = 253;                                          // both moduli are < 2^254 with bit 253 set
    while (i >= 0) {
        if (!inv_exp_bit<F>(i)) {
            if (started) acc = f29_sqr(acc);
            i--;
            continue;
        }
        int lo = i - 4 < 0 ? 0 : i - 4;
        while (!inv_exp_bit<F>(lo)) lo++;
        uint32_t w = 0;
        for (int k = i; k >= lo; k--) {
            w = (w << 1) | inv_exp_bit<F>(k);
            if (started) acc = f29_sqr(acc);
        }
        acc = started ? f29_mul(acc, tab[w >> 1]) : tab[w >> 1];
        started = true;
        i = lo - 1;
    }
    return acc;
}

// One workgroup (blockDim.x a power of two, L lanes) finishes the call: lane totals up a product tree in LDS (nodes 1 .. 2L - 1,
// leaves at L + lane), the Fermat chain on the root, inverses down the tree (node k's inverse times its sibling's value), then the
// lanes walk back over their elements.  LDS: (2 L + 16) Fe29.
template <class F, class Lv, template <class> class Acc>
KERNEL void k_inv_top(Lv lv, uint32_t *err) {
    DYN_SHARED(Fe29<F>, nodes);
    Fe29<F> *tab = nodes + 2 * blockDim.x;
    const uint32_t L = blockDim.x, j = threadIdx.x;
    const Acc<F> a{lv};
    nodes[L + j] = inv_up<F>(a, j, L, err);
    __syncthreads();
    for (uint32_t w = L >> 1; w >= 1; w >>= 1) {
        if (j < w) nodes[w + j] = f29_mul(nodes[2 * (w + j)], nodes[2 * (w + j) + 1]);
        __syncthreads();
    }
    if (j == 0) {
        Fe29<F> scale = f29_zero<F>();                    // 2^-10 in R' form: the integer 2^251 (< P for both fields)
        scale.l[8] = 1u << 19;
        F29_SET(scale, 1.0);
        nodes[1] = f29_mul(inv_fermat(nodes[1], tab), scale);
    }
    __syncthreads();
    for (uint32_t w = 1; w < L; w <<= 1) {
        if (j < w) {
            const uint32_t k = w + j;
            const Fe29<F> iv = nodes[k], x0 = nodes[2 * k], x1 = nodes[2 * k + 1];
            nodes[2 * k] = f29_mul(iv, x1);
            nodes[2 * k + 1] = f29_mul(iv, x0);
        }
        __syncthreads();
    }
    inv_down<F>(a, j, L, nodes[L + j], err);
}

// ---- multiplicities ----------------------------------------------------------------------------------------------------
struct LkTable {
    uint64_t *owner;                // index + 1 of a t element with the slot's value, 0 = empty
    uint32_t *first;                // lowest such index (starts at 0xFFFFFFFF)
    uint32_t *count;                // occurrences of the value in l
    uint64_t *slot_of_t;            // slot of every t element, ~0 if it has none (non-canonical input)
    uint64_t mask;                  // capacity - 1
    uint32_t hash_mode;             // 1: every key starts probing at slot 0 (tests: long probe chains at small sizes)
};
template <class FP> DEV uint64_t lk_hash(const Fe<FP> &k) {
    uint64_t h = 0x9E3779B97F4A7C15ull;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        h = (h ^ k.l[i]) * 0xFF51AFD7ED558CCDull;
        h ^= h >> 31;
    }
    return h;
}
template <class FP> DEV uint64_t lk_start(const Fe<FP> &k, const LkTable &tab) { return tab.hash_mode == 1 ? 0 : lk_hash(k) & tab.mask; }
// the slot of t_i's value, claimed for index i if the value has none yet; ~0 if every slot was tried (cannot happen below half load)
template <class FP> DEV uint64_t lk_claim(const unsigned char *__restrict__ t, const Fe<FP> &key, uint64_t i, const LkTable &tab) {
    uint64_t s = lk_start(key, tab);
    for (uint64_t step = 0; step <= tab.mask; step++, s = (s + 1) & tab.mask) {
        uint64_t o = tab.owner[s];                        // owners only ever change from 0: a stale 0 is caught by the CAS below
        if (o == 0) {
            o = atomic_cas_u64(tab.owner + s, 0, i + 1);
            if (o == 0) return s;
        }
        if (fe_eq(fe_load<FP>(t + (o - 1) * 32), key)) return s;
    }
    return ~0ull;
}

// pass 1: every t_i claims or finds the slot of its value; the lowest index of each value is kept.  Lanes of a wave that hold
// one value (grouped by a 64-bit hash of all eight words) probe once: the group's lowest lane probes, the others take its slot
// after comparing their key with its element (a hash collision probes for itself) -- a table column of 2^k - 25 zeros would
// otherwise send every lane's compare-and-swap to one address.
template <class FP>
KERNEL void k_lk_insert(const unsigned char *__restrict__ t, uint64_t n_t, LkTable tab, uint32_t *err) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_t) return;
    const Fe<FP> key = fe_load<FP>(t + i * 32);
    if (!lk_is_canonical(key)) {
        atomicMax(err, (uint32_t)LK_ERR_NONCANONICAL);
        tab.slot_of_t[i] = ~0ull;
        return;
    }
    uint32_t cnt, lead_lane;
    const bool lead = wave_group_leader(lk_hash(key), &cnt, &lead_lane);
    uint64_t found = lead ? lk_claim(t, key, i, tab) : ~0ull;
    const uint64_t lead_found = wave_shfl_u64(found, lead_lane), i_lead = wave_shfl_u64(i, lead_lane);
    if (!lead) {
        found = fe_eq(fe_load<FP>(t + i_lead * 32), key) ? lead_found : lk_claim(t, key, i, tab);
    }
    tab.slot_of_t[i] = found;
    if (found == ~0ull) {
        atomicMax(err, (uint32_t)LK_ERR_TABLE_FULL);
        return;
    }
    // the group's lowest lane holds its lowest index; `first` only ever decreases, so a value read at or below it already
    // makes the atomic redundant (a stale read is only ever too high)
    if (wave_group_leader(found, &cnt) && tab.first[found] > (uint32_t)i) atomic_min_u32(tab.first + found, (uint32_t)i);
}
// pass 2: every l_i found in the table adds 1 to its slot's count (a value absent from t contributes nothing).  Grid-stride
// over a bounded grid; a wave's group count goes to a small LDS table of the workgroup first (LK_WG_SLOTS entries keyed by
// slot, claimed by compare-and-swap; an entry taken by another slot sends the count straight to HBM) and every workgroup
// adds its entries to HBM once at the end -- a value most of l holds costs one global atomic per workgroup, not per wave.
static constexpr uint32_t LK_WG_SLOTS = 64;
template <class FP>
KERNEL void k_lk_count(const unsigned char *__restrict__ l, uint64_t n_l, const unsigned char *__restrict__ t, LkTable tab, uint32_t *err) {
    __shared__ uint64_t wkey[LK_WG_SLOTS];
    __shared__ uint32_t wcnt[LK_WG_SLOTS];
    for (uint32_t h = threadIdx.x; h < LK_WG_SLOTS; h += blockDim.x) {
        wkey[h] = ~0ull;
        wcnt[h] = 0;
    }
    __syncthreads();
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_l; i += (uint64_t)gridDim.x * blockDim.x) {
        const Fe<FP> key = fe_load<FP>(l + i * 32);
        if (!lk_is_canonical(key)) {
            atomicMax(err, (uint32_t)LK_ERR_NONCANONICAL);
            continue;
        }
        uint64_t s = lk_start(key, tab), found = ~0ull;
        for (uint64_t step = 0; step <= tab.mask; step++, s = (s + 1) & tab.mask) {
            const uint64_t o = tab.owner[s];
            if (o == 0) break;
            if (fe_eq(fe_load<FP>(t + (o - 1) * 32), key)) { found = s; break; }
        }
        if (found == ~0ull) continue;
        uint32_t cnt;
        if (!wave_group_leader(found, &cnt)) continue;
        const uint32_t h = (uint32_t)(found & (LK_WG_SLOTS - 1));
        uint64_t k = wkey[h];
        if (k == ~0ull) {
            k = atomic_cas_u64(wkey + h, ~0ull, found);
            if (k == ~0ull) k = found;
        }
        if (k == found) atomicAdd(wcnt + h, cnt);
        else atomicAdd(tab.count + found, cnt);
    }
    __syncthreads();
    for (uint32_t h = threadIdx.x; h < LK_WG_SLOTS; h += blockDim.x)
        if (wcnt[h]) atomicAdd(tab.count + wkey[h], wcnt[h]);
}
// pass 3: m_i = count at the first occurrence, else 0, as a field element: F::from_u128(count) = count * 2^256 mod P
template <class F>
KERNEL void k_lk_write_m(LkTable tab, uint64_t n_t, unsigned char *__restrict__ m) {
    using S = typename F::Sat;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_t) return;
    const uint64_t s = tab.slot_of_t[i];
    const uint32_t c = (s <= tab.mask && tab.first[s] == (uint32_t)i) ? tab.count[s] : 0u;
    if (c == 0) {
        fe_store(m + i * 32, fe_zero<S>());
        return;
    }
    Fe<S> ci = fe_zero<S>(), r2;
    ci.l[0] = c;
#pragma unroll
    for (int k = 0; k < 8; k++) r2.l[k] = S::R2[k];
    Fe29<F> k266;
#pragma unroll
    for (int k = 0; k < 9; k++) k266.l[k] = F::R256_TO_R261[k];
    F29_SET(k266, 1.0);
    // c * 2^512 * 2^-261 = c 2^251, then * 2^266 * 2^-261 = c 2^256
    const Fe29<F> v = f29_mul(f29_mul(f29_unpack_canonical<F>(ci), f29_unpack_canonical<F>(r2)), k266);
    fe_store(m + i * 32, lk_canonical(v));
}
