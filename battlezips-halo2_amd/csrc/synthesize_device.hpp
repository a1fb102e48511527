// Witness synthesis of the Shot and Board circuits on the device (bzh_synthesize_{shot,board}_with, BZH_SYNTH_DEVICE): the
// per-lane bodies of csrc/synthesize_device.hip's three kernels as host/device functions, so that a host program can run them
// lane by lane against the Layouter path (tests/helpers/synth_device_check.hip).
//
// csrc/circuit/chips.hpp and ecc.hpp stay the specification and the HOST path.  What is restated here is where a region's cells
// lie relative to its first row, and what integer each holds; the region rows, the column indices and the stride come from the
// circuit object (SynLayout, filled by csrc/circuits.hip from region_starts and the configs).
//   syn_cells_row           every cell that is an integer built from the proof's input words: one lane per (proof, row)
//   syn_mulfixed_gather     lane = window of one fixed-base multiplication: table look-up, window point and u cells
//   syn_mulfixed_finish     the lane's running sum to affine (its own fe_inv_ct: in a wave the lanes invert in lockstep, so one
//                           inversion per lane lasts as long as one per wave and needs no product scan), the x_qr / y_qr cells
//   syn_incomplete_exceptional   add_incomplete_assign_region's refusal, on the normalised operands
//   syn_ecc_tail            one lane per proof: the three complete additions, Shot's native commitment cells, the instance words
#pragma once
#include <string>
#include <vector>

#include "curve.cuh"
#include "normalize.hpp"

namespace bzh {

using SynP = FpParams;
using SynFe = Fe<SynP>;
using SynAff = Affine<SynP>;
using SynXyzz = Xyzz<SynP>;

constexpr int SYN_NW = 85;            // ECC_NUM_WINDOWS
constexpr int SYN_H = 8;              // ECC_H
constexpr int SYN_BOARD = 100;        // BOARD_SIZE
constexpr int SYN_MAX_REGIONS = 40;   // Board has 35
constexpr int SYN_TBL_WORDS = 24;     // a table entry: x, y, u (Montgomery)
constexpr size_t SYN_TBL_ENTRIES = (size_t)2 * SYN_NW * SYN_H;

// status word of a proof: the host path's throw sites that depend on more than the trapdoor's range
constexpr uint32_t SYN_ST_EXCEPTIONAL = 1;   // "incomplete addition: exceptional case"
constexpr uint32_t SYN_ST_WINDOW_X0 = 2;     // "fixed-base mul: window point with x = 0"
constexpr uint32_t SYN_ST_MESSAGE = 4;       // "pedersen_commit: message repr is not a canonical scalar"

enum SynRegionType : uint32_t {
    SYN_R_SKIP = 0,      // cells written by the ECC kernels
    SYN_R_SHOT_LOAD,     // "load private ShotChip advice values" (rows 1-2: syn_ecc_tail)
    SYN_R_BOARD_LOAD,    // "load ship placements"
    SYN_R_BITIFY,        // num2bits / bits2num; arg = source word | first column slot << 8
    SYN_R_PLACE_A,       // "permute and collapse bit decompositions"; arg = ship
    SYN_R_PLACE_B,       // "placement running sum trace"
    SYN_R_PLACE_C,       // "constrain running sum output"
    SYN_R_TRANSPOSE,     // "Transpose ship commitments"
    SYN_R_SHOT_SUM,      // "shot running sum"
    SYN_R_SHOT_OUT,      // "shot running sum output checks"
    SYN_R_BF_Z,          // running sum z_i = alpha >> 3 i of the base-field multiplication
    SYN_R_FW_WIN,        // the 3-bit windows of the full-width multiplication
    SYN_R_WITNESS,       // "Witness element": alpha_0' >> 10 i
    SYN_R_CANON,         // "Canonicity checks"
};
struct SynRegion {
    uint32_t type, start, rows, arg;
};
struct SynLayout {
    uint32_t kind;                 // BZH_CIRCUIT_SHOT / BZH_CIRCUIT_BOARD
    uint32_t n, rows_used, num_advice, nregions, in_words;
    uint32_t col[11];              // column index of the config's advice[i]
    uint32_t load, inc[2], add[2], final_add;   // first rows: the load region, (incomplete, complete) of V and R, the last addition
    uint32_t src_board, src_trapdoor;           // input words (units of 4 x u64)
    uint64_t place_mask[5][2];     // ship i: the offsets j with j % 10 + S <= 10, below 100
    uint32_t place_len[5];
    SynRegion reg[SYN_MAX_REGIONS];
};

// ---- 256-bit integers in four words, no indexing by a lane's data (that would put them in scratch memory) ------------------
struct SynU256 {
    uint64_t a, b, c, d;   // little-endian
};
BZH_HD SynU256 syn_zero() { return SynU256{0, 0, 0, 0}; }
BZH_HD SynU256 syn_small(uint64_t v) { return SynU256{v, 0, 0, 0}; }
BZH_HD SynU256 syn_load(const uint64_t* p) { return SynU256{p[0], p[1], p[2], p[3]}; }
BZH_HD SynU256 syn_shr(SynU256 v, unsigned s) {
    const unsigned ws = s >> 6, bs = s & 63;
    if (ws & 1) v = SynU256{v.b, v.c, v.d, 0};
    if (ws & 2) v = SynU256{v.c, v.d, 0, 0};
    if (ws >= 4) v = syn_zero();
    if (bs) {
        v.a = (v.a >> bs) | (v.b << (64 - bs));
        v.b = (v.b >> bs) | (v.c << (64 - bs));
        v.c = (v.c >> bs) | (v.d << (64 - bs));
        v.d >>= bs;
    }
    return v;
}
BZH_HD uint64_t syn_low_mask(unsigned bits, unsigned word) {   // the part of 2^bits - 1 in `word`
    const unsigned lo = 64 * word;
    return bits >= lo + 64 ? ~(uint64_t)0 : (bits <= lo ? 0 : (((uint64_t)1 << (bits - lo)) - 1));
}
BZH_HD SynU256 syn_low(SynU256 v, unsigned bits) {   // v mod 2^bits
    return SynU256{v.a & syn_low_mask(bits, 0), v.b & syn_low_mask(bits, 1), v.c & syn_low_mask(bits, 2), v.d & syn_low_mask(bits, 3)};
}
BZH_HD SynU256 syn_and(SynU256 x, SynU256 y) { return SynU256{x.a & y.a, x.b & y.b, x.c & y.c, x.d & y.d}; }
BZH_HD SynU256 syn_or(SynU256 x, SynU256 y) { return SynU256{x.a | y.a, x.b | y.b, x.c | y.c, x.d | y.d}; }
BZH_HD uint64_t syn_bit(SynU256 v, unsigned i) { return syn_shr(v, i).a & 1; }
BZH_HD SynU256 syn_pow2(unsigned i) {
    const uint64_t o = (uint64_t)1 << (i & 63);
    const unsigned w = i >> 6;
    return SynU256{w == 0 ? o : 0, w == 1 ? o : 0, w == 2 ? o : 0, w == 3 ? o : 0};
}
BZH_HD unsigned syn_pop64(uint64_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (unsigned)__popcll(x);
#else
    return (unsigned)__builtin_popcountll(x);
#endif
}
BZH_HD uint64_t syn_pop(SynU256 v) { return syn_pop64(v.a) + syn_pop64(v.b) + syn_pop64(v.c) + syn_pop64(v.d); }
BZH_HD SynU256 syn_add(SynU256 x, SynU256 y) {
    SynU256 r;
    uint64_t c;
    r.a = x.a + y.a, c = r.a < x.a;
    r.b = x.b + c, c = r.b < c, r.b += y.b, c += r.b < y.b;
    r.c = x.c + c, c = r.c < c, r.c += y.c, c += r.c < y.c;
    r.d = x.d + c + y.d;
    return r;
}
BZH_HD SynU256 syn_not(SynU256 x) { return SynU256{~x.a, ~x.b, ~x.c, ~x.d}; }
BZH_HD SynU256 syn_sub(SynU256 x, SynU256 y) { return syn_add(syn_add(x, syn_not(y)), syn_small(1)); }
// an integer below p as a field element: one product by R^2
BZH_HD SynFe syn_fe(SynU256 v) {
    SynFe r;
    r.l[0] = (uint32_t)v.a, r.l[1] = (uint32_t)(v.a >> 32), r.l[2] = (uint32_t)v.b, r.l[3] = (uint32_t)(v.b >> 32);
    r.l[4] = (uint32_t)v.c, r.l[5] = (uint32_t)(v.c >> 32), r.l[6] = (uint32_t)v.d, r.l[7] = (uint32_t)(v.d >> 32);
    return fe_to_mont(r);
}

// ---- cells --------------------------------------------------------------------------------------------------------------------
// `adv`: the proof's (num_advice, n) block of 8-word elements
BZH_HD uint32_t* syn_cell(const SynLayout* L, uint32_t* adv, unsigned slot, size_t row) { return adv + ((size_t)L->col[slot] * L->n + row) * 8; }
BZH_HD void syn_put_fe(const SynLayout* L, uint32_t* adv, unsigned slot, size_t row, const SynFe& v) { norm_store<SynP>(syn_cell(L, adv, slot, row), v); }
BZH_HD void syn_put(const SynLayout* L, uint32_t* adv, unsigned slot, size_t row, SynU256 v) { syn_put_fe(L, adv, slot, row, syn_fe(v)); }
BZH_HD SynFe syn_get_fe(const SynLayout* L, const uint32_t* adv, unsigned slot, size_t row) {
    return norm_load<SynP>(adv + ((size_t)L->col[slot] * L->n + row) * 8);
}

// the scalar of the base-field multiplication: the board state as the circuit recomposes it (Shot: the low 128 bits of the
// board word, src/chips/shot.rs:316; Board: the 100 transposed bits, bits2num)
BZH_HD SynU256 syn_alpha(const SynLayout* L, const uint64_t* in) {
    return syn_low(syn_load(in + 4 * L->src_board), L->kind == BZH_CIRCUIT_SHOT ? 128 : SYN_BOARD);
}
// alpha_0' = alpha_0 + 2^130 - t_p with alpha_0 = alpha mod 2^252 (mul_fixed_base_field_elem); positive and below p as an integer
BZH_HD SynU256 syn_alpha_0_prime(SynU256 alpha) {
    const SynU256 t_p{0x992d30ed00000001ull, 0x224698fc094cf91bull, 0, 0};   // p - 2^254
    return syn_sub(syn_add(syn_low(alpha, 252), syn_pow2(130)), t_p);
}
// window w of a fixed-base scalar (decompose_word_3bit): base 0 = V with alpha, base 1 = R with the trapdoor
BZH_HD unsigned syn_window(const SynLayout* L, const uint64_t* in, int base, unsigned w) {
    const SynU256 s = base ? syn_load(in + 4 * L->src_trapdoor) : syn_alpha(L, in);
    return (unsigned)(syn_shr(s, 3 * w).a & 7);
}
// ship i of a Board proof (zip of its two commitments) and its full-window offsets (compute_placement_trace's `increment`,
// restricted to the offsets of the i % 10 + S <= 10 rule)
BZH_HD SynU256 syn_ship(const uint64_t* in, unsigned i) { return syn_low(syn_or(syn_load(in + 8 * i), syn_load(in + 8 * i + 4)), SYN_BOARD); }
BZH_HD SynU256 syn_full_windows(const SynLayout* L, const uint64_t* in, unsigned i) {
    const SynU256 ship = syn_ship(in, i);
    SynU256 f = ship;
    for (unsigned s = 1; s < L->place_len[i]; s++) f = syn_and(f, syn_shr(ship, s));
    return syn_and(f, SynU256{L->place_mask[i][0], L->place_mask[i][1], 0, 0});
}

BZH_HD void syn_region_row(const SynLayout* L, const uint64_t* in, const SynRegion reg, unsigned off, size_t row, uint32_t* adv) {
    switch (reg.type) {
        case SYN_R_SHOT_LOAD: {
            if (off == 0) syn_put(L, adv, 4, row, syn_low(syn_load(in), 128));
            if (off == 3) syn_put(L, adv, 4, row, syn_low(syn_load(in + 8), 128));
            if (off == 4) syn_put(L, adv, 4, row, syn_low(syn_load(in + 12), 128));
            break;
        }
        case SYN_R_BOARD_LOAD: {
            for (unsigned c = 0; c < 10; c++) syn_put(L, adv, c, row, syn_low(syn_load(in + 4 * c), 128));
            break;
        }
        case SYN_R_BITIFY: {
            const SynU256 v = syn_load(in + 4 * (reg.arg & 0xff));
            const unsigned cb = reg.arg >> 8;
            if (off < (unsigned)SYN_BOARD) syn_put(L, adv, cb, row, syn_small(syn_bit(v, off)));
            syn_put(L, adv, cb + 1, row, syn_low(v, off));
            syn_put(L, adv, cb + 2, row, syn_pow2(off));
            break;
        }
        case SYN_R_PLACE_A: {
            const SynU256 h = syn_load(in + 8 * reg.arg), v = syn_load(in + 8 * reg.arg + 4);
            syn_put(L, adv, 1, row, syn_small(syn_bit(h, off)));
            syn_put(L, adv, 2, row, syn_small(syn_bit(v, off)));
            syn_put(L, adv, 0, row, syn_small(syn_bit(h, off) | syn_bit(v, off)));
            break;
        }
        case SYN_R_PLACE_B: {
            if (off == 0) break;   // the two constants 0
            const SynU256 ship = syn_ship(in, reg.arg);
            syn_put(L, adv, 0, row, syn_small(syn_bit(ship, off - 1)));
            syn_put(L, adv, 1, row, syn_small(syn_pop(syn_low(ship, off))));
            syn_put(L, adv, 2, row, syn_small(syn_pop(syn_low(syn_full_windows(L, in, reg.arg), off))));
            break;
        }
        case SYN_R_PLACE_C: {
            syn_put(L, adv, 1, row, syn_small(syn_pop(syn_ship(in, reg.arg))));
            syn_put(L, adv, 2, row, syn_small(syn_pop(syn_full_windows(L, in, reg.arg))));
            break;
        }
        case SYN_R_TRANSPOSE: {
            for (unsigned c = 0; c < 10; c++) {
                const unsigned idx = (c & 1) ? off % 10 * 10 + off / 10 : off;
                syn_put(L, adv, c, row, syn_small(syn_bit(syn_load(in + 4 * c), idx)));
            }
            syn_put(L, adv, 10, row, syn_small(syn_bit(syn_load(in + 4 * L->src_board), off)));
            break;
        }
        case SYN_R_SHOT_SUM: {
            if (off == 0) break;
            const SynU256 board = syn_load(in), shot = syn_load(in + 8);
            syn_put(L, adv, 5, row, syn_small(syn_bit(board, off - 1)));
            syn_put(L, adv, 6, row, syn_small(syn_bit(shot, off - 1)));
            syn_put(L, adv, 7, row, syn_small(syn_pop(syn_low(shot, off))));
            syn_put(L, adv, 8, row, syn_small(syn_pop(syn_low(syn_and(board, shot), off))));
            break;
        }
        case SYN_R_SHOT_OUT: {
            const SynU256 board = syn_load(in), shot = syn_load(in + 8);
            syn_put(L, adv, 5, row, syn_low(syn_load(in + 12), 128));
            syn_put(L, adv, 6, row, syn_small(syn_pop(syn_low(shot, SYN_BOARD))));
            syn_put(L, adv, 7, row, syn_small(syn_pop(syn_low(syn_and(board, shot), SYN_BOARD))));
            break;
        }
        case SYN_R_BF_Z: syn_put(L, adv, 4, row, syn_shr(syn_alpha(L, in), 3 * off)); break;
        case SYN_R_FW_WIN: syn_put(L, adv, 4, row, syn_small(syn_window(L, in, 1, off))); break;
        case SYN_R_WITNESS: syn_put(L, adv, 9, row, syn_shr(syn_alpha_0_prime(syn_alpha(L, in)), 10 * off)); break;
        case SYN_R_CANON: {
            const SynU256 alpha = syn_alpha(L, in), a0p = syn_alpha_0_prime(alpha);
            if (off == 0) {
                syn_put(L, adv, 6, row, alpha);
                syn_put(L, adv, 8, row, syn_shr(alpha, 252));                    // z_84
            } else if (off == 1) {
                syn_put(L, adv, 6, row, a0p);
                syn_put(L, adv, 7, row, syn_low(syn_shr(alpha, 252), 2));        // alpha_1
                syn_put(L, adv, 8, row, syn_small(syn_bit(alpha, 254)));         // alpha_2
            } else {
                syn_put(L, adv, 6, row, syn_shr(a0p, 130));                      // z_13 of alpha_0'
                syn_put(L, adv, 7, row, syn_shr(alpha, 132));                    // z_44
                syn_put(L, adv, 8, row, syn_shr(alpha, 129));                    // z_43
            }
            break;
        }
        default: break;
    }
}
// lane (proof, row): a row lies in as many regions as use disjoint columns there
BZH_HD void syn_cells_row(const SynLayout* L, const uint64_t* in, size_t row, uint32_t* adv) {
    for (uint32_t r = 0; r < L->nregions; r++) {
        const SynRegion reg = L->reg[r];
        if (reg.type != SYN_R_SKIP && row >= reg.start && row - reg.start < reg.rows) syn_region_row(L, in, reg, (unsigned)(row - reg.start), row, adv);
    }
}

// ---- fixed-base multiplications -----------------------------------------------------------------------------------------------
// complete XYZZ addition with everything inlined (curve.cuh's xyzz_add keeps its doubling branch out of line)
BZH_HD SynXyzz syn_xyzz_add(const SynXyzz& a, const SynXyzz& b) {
    if (xyzz_is_id(b)) return a;
    if (xyzz_is_id(a)) return b;
    const SynFe u1 = fe_mul(a.x, b.zz), u2 = fe_mul(b.x, a.zz), s1 = fe_mul(a.y, b.zzz), s2 = fe_mul(b.y, a.zzz);
    const SynFe pp_ = fe_sub(u2, u1), r = fe_sub(s2, s1);
    if (fe_is_zero(pp_)) return fe_is_zero(r) ? xyzz_dbl_inl(a) : xyzz_identity<SynP>();
    const SynFe pp = fe_sqr(pp_), ppp = fe_mul(pp_, pp), qq = fe_mul(u1, pp);
    SynXyzz o;
    o.x = fe_sub(fe_sub(fe_sqr(r), ppp), fe_dbl(qq));
    o.y = fe_sub(fe_mul(r, fe_sub(qq, o.x)), fe_mul(s1, ppp));
    o.zz = fe_mul(fe_mul(a.zz, b.zz), pp);
    o.zzz = fe_mul(fe_mul(a.zzz, b.zzz), ppp);
    return o;
}
// the running sums of `n` window points, in place: what the device does in 7 levels over an LDS tile, as a plain loop
inline void syn_scan_host(SynXyzz* v, int n) {
    for (int i = 1; i < n; i++) v[i] = syn_xyzz_add(v[i - 1], v[i]);
}
// lane w < 85 of base `base`: m_w = points[w][k_w]; writes x_p, y_p and u at offset w
BZH_HD SynAff syn_mulfixed_gather(const SynLayout* L, const uint32_t* tbl, const uint64_t* in, int base, unsigned w, uint32_t* adv, uint32_t* flag) {
    const unsigned k = syn_window(L, in, base, w);
    const uint32_t* e = tbl + (((size_t)base * SYN_NW + w) * SYN_H + k) * SYN_TBL_WORDS;
    SynAff m;
    m.x = norm_load<SynP>(e);
    m.y = norm_load<SynP>(e + 8);
    const size_t row = (size_t)L->inc[base] + w;
    syn_put_fe(L, adv, 0, row, m.x);
    syn_put_fe(L, adv, 1, row, m.y);
    syn_put_fe(L, adv, 5, row, norm_load<SynP>(e + 16));
    if (fe_is_zero(m.x)) *flag |= SYN_ST_WINDOW_X0;
    return m;
}
BZH_HD SynAff syn_xyzz_to_affine_ct(const SynXyzz& p) {   // the identity (ZZ = 0) comes out as (0, 0): 0^-1 = 0
    const SynFe i = fe_inv_ct(fe_mul(p.zz, p.zzz));
    SynAff r;
    r.x = fe_mul(p.x, fe_mul(i, p.zzz));
    r.y = fe_mul(p.y, fe_mul(i, p.zz));
    return r;
}
// lane w < 84: acc_w = sum_{j <= w} m_j to affine, into x_qr / y_qr at offset w + 1
BZH_HD SynAff syn_mulfixed_finish(const SynLayout* L, int base, unsigned w, const SynXyzz& acc, uint32_t* adv) {
    const SynAff a = syn_xyzz_to_affine_ct(acc);
    const size_t row = (size_t)L->inc[base] + w + 1;
    syn_put_fe(L, adv, 2, row, a.x);
    syn_put_fe(L, adv, 3, row, a.y);
    return a;
}
// add_incomplete_assign_region(p = m_w, q = acc_{w-1}) refuses an identity operand and equal x
BZH_HD uint32_t syn_incomplete_exceptional(const SynAff& acc_prev, const SynAff& m) {
    return (aff_is_id(acc_prev) || aff_is_id(m) || fe_eq(acc_prev.x, m.x)) ? SYN_ST_EXCEPTIONAL : 0u;
}

// ---- tail ---------------------------------------------------------------------------------------------------------------------
// add_assign_region: P + Q with its inv0 cells and lambda, every branch a select.  The five inverses (x_q - x_p, x_p, x_q,
// y_q + y_p and the tangent's 2 y_p) share one fe_inv_ct; a zero counts as one in the products and comes out as zero.
struct SynAdd {
    SynFe alpha, beta, gamma, delta, lambda, xr, yr;
};
BZH_HD SynAdd syn_complete_add(const SynFe& xp, const SynFe& yp, const SynFe& xq, const SynFe& yq) {
    const SynFe one = fe_one<SynP>(), zero = fe_zero<SynP>();
    const SynFe d0 = fe_sub(xq, xp), d3 = fe_add(yq, yp), d4 = fe_dbl(yp);
    const bool z0 = fe_is_zero(d0), z1 = fe_is_zero(xp), z2 = fe_is_zero(xq), z3 = fe_is_zero(d3), z4 = fe_is_zero(d4);
    const SynFe s0 = fe_csel(z0, one, d0), s1 = fe_csel(z1, one, xp), s2 = fe_csel(z2, one, xq), s3 = fe_csel(z3, one, d3), s4 = fe_csel(z4, one, d4);
    const SynFe p1 = fe_mul(s0, s1), p2 = fe_mul(p1, s2), p3 = fe_mul(p2, s3);
    SynFe inv = fe_inv_ct(fe_mul(p3, s4));
    const SynFe i4 = fe_csel(z4, zero, fe_mul(inv, p3));
    inv = fe_mul(inv, s4);
    const SynFe i3 = fe_csel(z3, zero, fe_mul(inv, p2));
    inv = fe_mul(inv, s3);
    const SynFe i2 = fe_csel(z2, zero, fe_mul(inv, p1));
    inv = fe_mul(inv, s2);
    const SynFe i1 = fe_csel(z1, zero, fe_mul(inv, s0));
    const SynFe i0 = fe_csel(z0, zero, fe_mul(inv, s1));
    SynAdd r;
    r.alpha = i0, r.beta = i1, r.gamma = i2;
    r.delta = fe_csel(z0, i3, zero);
    const SynFe xx = fe_sqr(xp);
    r.lambda = fe_csel(z0, fe_mul(fe_add(fe_dbl(xx), xx), i4), fe_mul(fe_sub(yq, yp), i0));   // y_p = 0 on the tangent branch: i4 = 0
    const SynFe xs = fe_sub(fe_sub(fe_sqr(r.lambda), xp), xq), ys = fe_sub(fe_mul(r.lambda, fe_sub(xp, xs)), yp);
    const bool neg = z0 && z3;   // x_q = x_p and y_q = -y_p
    r.xr = fe_csel(z1, xq, fe_csel(z2, xp, fe_csel(neg, zero, xs)));
    r.yr = fe_csel(z1, yq, fe_csel(z2, yp, fe_csel(neg, zero, ys)));
    return r;
}
// the rows of one add_assign_region at `row`; returns the sum
BZH_HD SynAff syn_add_region(const SynLayout* L, uint32_t* adv, size_t row, const SynAff& p, const SynAff& q) {
    const SynAdd a = syn_complete_add(p.x, p.y, q.x, q.y);
    syn_put_fe(L, adv, 0, row, p.x);
    syn_put_fe(L, adv, 1, row, p.y);
    syn_put_fe(L, adv, 2, row, q.x);
    syn_put_fe(L, adv, 3, row, q.y);
    syn_put_fe(L, adv, 4, row, a.lambda);
    syn_put_fe(L, adv, 5, row, a.alpha);
    syn_put_fe(L, adv, 6, row, a.beta);
    syn_put_fe(L, adv, 7, row, a.gamma);
    syn_put_fe(L, adv, 8, row, a.delta);
    syn_put_fe(L, adv, 2, row + 1, a.xr);
    syn_put_fe(L, adv, 3, row + 1, a.yr);
    return SynAff{a.xr, a.yr};
}
// the complete addition that ends multiplication `b`: m_84 in (x_p, y_p) and acc_83 in (x_qr, y_qr) of the last incomplete row
BZH_HD SynAff syn_tail_sum(const SynLayout* L, uint32_t* adv, int b) {
    const size_t last = (size_t)L->inc[b] + SYN_NW - 1;
    const SynAff p{syn_get_fe(L, adv, 0, last), syn_get_fe(L, adv, 1, last)}, q{syn_get_fe(L, adv, 2, last), syn_get_fe(L, adv, 3, last)};
    return syn_add_region(L, adv, L->add[b], p, q);
}
// one lane per proof, after the multiplications' cells are in place.  inst_xy: 16 words, the commitment's canonical x || y.
// Returns the status bits of this stage.
BZH_HD uint32_t syn_ecc_tail(const SynLayout* L, const uint64_t* in, uint32_t* adv, uint32_t* inst_xy) {
    const SynAff v = syn_tail_sum(L, adv, 0), r = syn_tail_sum(L, adv, 1);
    const SynAff cm = syn_add_region(L, adv, L->final_add, v, r);
    uint32_t st = 0;
    if (L->kind == BZH_CIRCUIT_SHOT) {   // the native commitment ShotChip loads: the same group element
        syn_put_fe(L, adv, 4, (size_t)L->load + 1, cm.x);
        syn_put_fe(L, adv, 4, (size_t)L->load + 2, cm.y);
        const SynU256 m = syn_alpha(L, in);   // Fq::from_repr(message.to_repr()).unwrap()
        Fe<FqParams> mq;
        mq.l[0] = (uint32_t)m.a, mq.l[1] = (uint32_t)(m.a >> 32), mq.l[2] = (uint32_t)m.b, mq.l[3] = (uint32_t)(m.b >> 32);
        mq.l[4] = (uint32_t)m.c, mq.l[5] = (uint32_t)(m.c >> 32), mq.l[6] = (uint32_t)m.d, mq.l[7] = (uint32_t)(m.d >> 32);
        if (!fe_lt_p(mq)) st |= SYN_ST_MESSAGE;
    }
    norm_store<SynP>(inst_xy, fe_from_mont(cm.x));
    norm_store<SynP>(inst_xy + 8, fe_from_mont(cm.y));
    return st;
}

// ---- the launch (csrc/synthesize_device.hip); the caller holds ctx->mu ---------------------------------------------------------
struct SynRun {
    const SynLayout* layout = nullptr;
    size_t batch = 0;
    const uint64_t* inputs = nullptr;      // batch x layout->in_words, packed
    const uint32_t* table = nullptr;       // SYN_TBL_ENTRIES x SYN_TBL_WORDS words, uploaded on the ctx's first call
    uint32_t* d_advice = nullptr;
    uint64_t* commitments = nullptr;       // batch x 8 canonical words (x || y), or null
    uint32_t* status = nullptr;            // batch words
};
// enqueue, then read back: one staged upload, the zero fill, the three kernels, one read-back (the call's only stream wait)
int synth_device_run(bzh_ctx* ctx, const SynRun& run);
// the enqueue-only form: the same upload, fill and kernels, the status words (batch) and the commitments (batch x 16 canonical
// words, x || y) to DEVICE pointers of the caller's (16-byte aligned), no read-back and no stream wait.  run.status and
// run.commitments are not read.  *d_inputs: where the packed inputs lie in WS_STAGE -- valid for kernels the caller enqueues before
// anything else takes that slot.  ev: null, or five events recorded around the fill and the kernels (synth_device_run's trace).
int synth_device_enqueue(bzh_ctx* ctx, const SynRun& run, uint32_t* d_status, uint32_t* d_commitments, const uint64_t** d_inputs,
                         hipEvent_t* ev = nullptr);
// the host path's text for a status word (the first of its throw sites that the word names)
inline const char* syn_status_text(uint32_t st) {
    return (st & SYN_ST_MESSAGE)     ? "pedersen_commit: message repr is not a canonical scalar"
           : (st & SYN_ST_WINDOW_X0) ? "fixed-base mul: window point with x = 0"
                                     : "incomplete addition: exceptional case";
}
// csrc/circuits.hip: the layout and the table of a circuit, for the launch and for the host twin's test program
int synth_layout(const bzh_circuit* c, SynLayout* out);
const uint32_t* synth_table_host();
// csrc/circuits.hip: what a caller outside that file may know of a circuit object
struct SynShape {
    int kind;                                   // bzh_circuit_kind
    size_t n, num_advice, num_instance, inst_rows;   // rows, advice columns, instance columns, public inputs per proof
};
int synth_shape(const bzh_circuit* c, SynShape* out);
// csrc/circuits.hip: step one of a device synthesis, "check and pack the inputs" (no device use).  a .. d: the input arrays of
// bzh_synthesize_shot (boards, trapdoors, shots, hits) or bzh_synthesize_board (ship_commitments, boards, trapdoors, null).
// Fills the layout and `in` (batch x layout->in_words words) for SynRun.  BZH_E_RANGE with the host path's text in *err (and in
// bzh_circuit_last_error) for what the host path refuses on the inputs alone: a non-canonical trapdoor, H and V sharing a bit.
int synth_pack_inputs(const bzh_circuit* c, size_t batch, const uint64_t* a, const uint64_t* b, const uint64_t* c_in, const uint64_t* d,
                      SynLayout* layout, std::vector<uint64_t>* in, std::string* err);

}  // namespace bzh
