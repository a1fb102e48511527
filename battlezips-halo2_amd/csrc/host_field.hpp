// Host-side field and curve helpers of the library (portable Fe<P> arithmetic, csrc/field.cuh's host product) and the
// dispatch from a runtime field / curve id (include/bzh2.h) to the parameter pack: the one home of the per-field constants,
// limb marshalling, roots of unity, the square root, the Jacobi symbol, batch inversion, interpolation, Jacobian / XYZZ -> affine
// and point (de)compression.  The circuit front end's value types (csrc/circuit/hostfield.hpp) forward to it.
// Host only; Montgomery form unless noted.
#pragma once
#include <cstring>
#include <utility>
#include <vector>

#include "../../include/bzh2.h"
#include "curve.cuh"

namespace bzh {

// ---------------------------------------------------------------------------
// constants: C-ABI id, two-adicity S (2^S | p - 1) and multiplicative generator per field; base / scalar field per curve
// ---------------------------------------------------------------------------
template <class P>
struct FieldInfo;
template <int ID, unsigned TWO_ADICITY, uint32_t GEN>
struct FieldInfoOf {
    static constexpr int id = ID;
    static constexpr unsigned S = TWO_ADICITY;
    static constexpr uint32_t gen = GEN;
};
template <>
struct FieldInfo<FpParams> : FieldInfoOf<BZH_FIELD_FP, 32, 5> {};
template <>
struct FieldInfo<FqParams> : FieldInfoOf<BZH_FIELD_FQ, 32, 5> {};
template <>
struct FieldInfo<BnFrParams> : FieldInfoOf<BZH_FIELD_BN254_FR, 28, 7> {};
template <>
struct FieldInfo<BnFqParams> : FieldInfoOf<BZH_FIELD_BN254_FQ, 1, 3> {};

template <class C>
struct CurveInfo;
template <class C, class Scalar>
struct CurveInfoOf {
    using Base = typename C::Base;
    using SF = Scalar;  // the scalar field: the curve's group order
    static constexpr int id = C::id;
    static constexpr uint32_t b = C::b;
    static constexpr int scalar_field = FieldInfo<Scalar>::id;
};
template <>
struct CurveInfo<VestaCurve> : CurveInfoOf<VestaCurve, FpParams> {};
template <>
struct CurveInfo<PallasCurve> : CurveInfoOf<PallasCurve, FqParams> {};
template <>
struct CurveInfo<Bn254Curve> : CurveInfoOf<Bn254Curve, BnFrParams> {};

// ---------------------------------------------------------------------------
// runtime id -> parameter pack: f(FpParams{}) / f(VestaCurve{}) ..., f returns a status; unknown id: BZH_E_ARG
// ---------------------------------------------------------------------------
template <class F>
inline int with_field(int id, F&& f) {
    switch (id) {
        case BZH_FIELD_FP: return f(FpParams{});
        case BZH_FIELD_FQ: return f(FqParams{});
        case BZH_FIELD_BN254_FR: return f(BnFrParams{});
        case BZH_FIELD_BN254_FQ: return f(BnFqParams{});
    }
    return BZH_E_ARG;
}
template <class F>
inline int with_pasta_field(int id, F&& f) {
    switch (id) {
        case BZH_FIELD_FP: return f(FpParams{});
        case BZH_FIELD_FQ: return f(FqParams{});
    }
    return BZH_E_ARG;
}
template <class F>
inline int with_pasta_curve(int id, F&& f) {
    switch (id) {
        case BZH_CURVE_VESTA: return f(VestaCurve{});
        case BZH_CURVE_PALLAS: return f(PallasCurve{});
    }
    return BZH_E_ARG;
}
template <class F>
inline int with_curve(int id, F&& f) {
    switch (id) {
        case BZH_CURVE_VESTA: return f(VestaCurve{});
        case BZH_CURVE_PALLAS: return f(PallasCurve{});
        case BZH_CURVE_BN254: return f(Bn254Curve{});
    }
    return BZH_E_ARG;
}

// ---------------------------------------------------------------------------
// limb marshalling: 4 x u64 little-endian <-> Fe<P>.  `form` names the form of the limbs in memory; the Fe<P> is in
// Montgomery form when it is given, and simply the limbs when it is left out.
// ---------------------------------------------------------------------------
template <class P>
inline Fe<P> fe_from_u64(const uint64_t* p, int form = BZH_FORM_MONTGOMERY) {
    Fe<P> v;
    for (int i = 0; i < 4; i++) {
        v.l[2 * i] = (uint32_t)p[i];
        v.l[2 * i + 1] = (uint32_t)(p[i] >> 32);
    }
    return form == BZH_FORM_CANONICAL ? fe_to_mont(v) : v;
}
template <class P>
inline void fe_to_u64(uint64_t* p, Fe<P> v, int form = BZH_FORM_MONTGOMERY) {
    if (form == BZH_FORM_CANONICAL) v = fe_from_mont(v);
    for (int i = 0; i < 4; i++) p[i] = (uint64_t)v.l[2 * i] | ((uint64_t)v.l[2 * i + 1] << 32);
}
template <class P>
inline Fe<P> h_from_bytes(const uint8_t* b) {  // canonical little-endian -> Montgomery
    uint64_t l[4];
    memcpy(l, b, 32);
    return fe_from_u64<P>(l, BZH_FORM_CANONICAL);
}
// Field::random / a challenge: 64 bytes little-endian mod p.  lo + hi * 2^256 has the Montgomery image lo R + hi R R
template <class P>
inline Fe<P> h_from_u512(const uint8_t* b) {
    uint64_t lo[4], hi[4];
    memcpy(lo, b, 32);
    memcpy(hi, b + 32, 32);
    const Fe<P> r2 = fe_r2<P>();
    return fe_add(fe_mul(fe_from_u64<P>(lo), r2), fe_mul(fe_mul(fe_from_u64<P>(hi), r2), r2));
}
// the limbs are a canonical encoding: v < p
template <class P>
inline bool is_canonical(const Fe<P>& v) {
    for (int i = 7; i >= 0; i--)
        if (v.l[i] != P::mod(i)) return v.l[i] < P::mod(i);
    return false;
}

// ---------------------------------------------------------------------------
// powers and roots
// ---------------------------------------------------------------------------
template <class P>
inline Fe<P> h_pow_u64(Fe<P> base, uint64_t e) {
    Fe<P> acc = fe_one<P>();
    for (; e; e >>= 1) {
        if (e & 1) acc = fe_mul(acc, base);
        base = fe_sqr(base);
    }
    return acc;
}
inline void h_shr256(const uint32_t in[8], unsigned s, uint32_t out[8]) {
    for (int i = 0; i < 8; i++) {
        const unsigned src = i + s / 32;
        const uint64_t lo = src < 8 ? in[src] : 0, hi = src + 1 < 8 ? in[src + 1] : 0;
        out[i] = (s % 32) ? (uint32_t)((lo | (hi << 32)) >> (s % 32)) : (uint32_t)lo;
    }
}
// (p - 1) >> s, an exponent for fe_pow
template <class P>
inline void h_pm1_shr(unsigned s, uint32_t out[8]) {
    uint32_t pm1[8];
    for (int i = 0; i < 8; i++) pm1[i] = P::mod(i);
    pm1[0] -= 1;  // p is odd
    h_shr256(pm1, s, out);
}
// ROOT_OF_UNITY = gen^((p - 1) >> S): generates the 2-Sylow subgroup (order 2^S)
template <class P>
inline Fe<P> h_root_of_unity() {
    uint32_t e[8];
    h_pm1_shr<P>(FieldInfo<P>::S, e);
    return fe_pow(fe_from_u32<P>(FieldInfo<P>::gen), e);
}
// the 2^log_n-th root of unity ROOT^(2^(S - log_n)) out of ROOT (EvaluationDomain::new); log_n <= S
template <class P>
inline Fe<P> h_omega(Fe<P> root, unsigned log_n) {
    for (unsigned i = log_n; i < FieldInfo<P>::S; i++) root = fe_sqr(root);
    return root;
}
template <class P>
inline Fe<P> h_omega(unsigned log_n) {
    return h_omega(h_root_of_unity<P>(), log_n);
}
// ---------------------------------------------------------------------------
// square root, host and device (csrc/sqrt_decompress.hip runs the same function, one lane per element)
//
// The root is the one pasta_curves 0.4.1's table-based `sqrt` (Sarkar) returns: with p - 1 = 2^S T, g = gen^T and t in [0, 2^S)
// such that u^T g^t = 1 -- t is even exactly when u is a square -- it is u^((T+1)/2) g^(t/2).  This fixes WHICH of the two roots
// the circuit's fixed-base `u` tables hold; the sampled U rows of tests/golden/fixed_bases.json pin it.
//   * v = u^((T-1)/2) by 3-bit fixed windows over the compile-time exponent p >> (S + 1); then w = v u = u^((T+1)/2) and
//     x = w v = u^T, so no inversion is needed.
//   * t bit by bit from the bottom, in two halves (Pohlig-Hellman): x^(2^HI) has order dividing 2^LO and gives the low LO bits
//     with chains of at most LO - 1 squarings; x g^(t_lo) then has order dividing 2^HI and gives the rest.  S = 32 costs
//     16 + 2 * 120 squarings instead of 496.
//   * every loop bound is a constant of the field; a set bit multiplies by g^(2^i) through a select.  No trip count and no
//     branch depends on u, so a wave runs it in lockstep.
// gpow: g^(2^i) for i <= S, 8 Montgomery limbs each (h_sqrt_table on the host; the ctx owns the device copy).
// ---------------------------------------------------------------------------
template <class P>
BZH_HD Fe<P> fe_csel(bool c, const Fe<P>& a, const Fe<P>& b) {  // c ? a : b
    Fe<P> r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.l[i] = c ? a.l[i] : b.l[i];
    return r;
}
template <class P>
struct SqrtExp {
    static constexpr unsigned S = FieldInfo<P>::S;
    // bit i of (T - 1) / 2 = (p - 1) >> (S + 1) = p >> (S + 1)
    BZH_HD static constexpr unsigned bit(unsigned i) {
        const unsigned j = i + S + 1;
        return j < 256 ? (P::mod((int)(j >> 5)) >> (j & 31)) & 1u : 0u;
    }
    BZH_HD static constexpr unsigned digit(int w) { return bit(3 * w) | (bit(3 * w + 1) << 1) | (bit(3 * w + 2) << 2); }
    static constexpr int top_window() {
        int w = 85;
        while (w > 0 && digit(w) == 0) w--;
        return w;
    }
    static constexpr int top = top_window();
};
template <class P>
BZH_HD Fe<P> fe_sqrt_window(const Fe<P> (&tb)[7], unsigned d) {  // tb[d - 1], d in 1..7, as selects (d is uniform)
    Fe<P> r = tb[0];
#pragma unroll
    for (int j = 1; j < 7; j++) r = fe_csel(d == (unsigned)(j + 1), tb[j], r);
    return r;
}
template <class P>
BZH_HD Fe<P> fe_sqrt_gpow(const uint32_t* gpow, unsigned i) {
    Fe<P> r;
#pragma unroll
    for (int k = 0; k < 8; k++) r.l[k] = gpow[8 * i + k];
    return r;
}
// false: u is not a square; root then holds r with r^2 = u / g (g = gpow[0]), which csrc/hash_to_curve.hpp's map uses.
// Zero maps to zero.
template <class P>
BZH_HD bool fe_sqrt_ct(const Fe<P>& u, const uint32_t* gpow, Fe<P>& root) {
    constexpr unsigned S = FieldInfo<P>::S, LO = S / 2, HI = S - LO;
    Fe<P> tb[7];  // u^1 .. u^7
    tb[0] = u;
    tb[1] = fe_sqr(u);
    tb[2] = fe_mul(tb[1], u);
    tb[3] = fe_sqr(tb[1]);
    tb[4] = fe_mul(tb[3], u);
    tb[5] = fe_sqr(tb[2]);
    tb[6] = fe_mul(tb[5], u);
    Fe<P> v = fe_sqrt_window(tb, SqrtExp<P>::digit(SqrtExp<P>::top));
#pragma unroll 1
    for (int w = SqrtExp<P>::top - 1; w >= 0; w--) {
        v = fe_sqr(fe_sqr(fe_sqr(v)));
        const unsigned d = SqrtExp<P>::digit(w);
        if (d) v = fe_mul(v, fe_sqrt_window(tb, d));
    }
    const Fe<P> one = fe_one<P>();
    Fe<P> res = fe_mul(v, u);    // u^((T+1)/2)
    Fe<P> cur = fe_mul(res, v);  // u^T, in the 2-Sylow subgroup; from here on cur = u^T g^(bits of t found so far)
    bool odd = false;            // bit 0 of t
    if constexpr (LO > 0) {
        Fe<P> c0 = cur;  // cur^(2^HI)
#pragma unroll 1
        for (unsigned j = 0; j < HI; j++) c0 = fe_sqr(c0);
#pragma unroll 1
        for (unsigned i = 0; i < LO; i++) {
            Fe<P> y = c0;
#pragma unroll 1
            for (unsigned j = i + 1; j < LO; j++) y = fe_sqr(y);
            const bool bit = !fe_eq(y, one);  // y is 1 or -1
            c0 = fe_csel(bit, fe_mul(c0, fe_sqrt_gpow<P>(gpow, HI + i)), c0);
            cur = fe_csel(bit, fe_mul(cur, fe_sqrt_gpow<P>(gpow, i)), cur);
            if (i == 0)
                odd = bit;
            else
                res = fe_csel(bit, fe_mul(res, fe_sqrt_gpow<P>(gpow, i - 1)), res);
        }
    }
#pragma unroll 1
    for (unsigned i = 0; i < HI; i++) {
        Fe<P> y = cur;
#pragma unroll 1
        for (unsigned j = i + 1; j < HI; j++) y = fe_sqr(y);
        const bool bit = !fe_eq(y, one);
        cur = fe_csel(bit, fe_mul(cur, fe_sqrt_gpow<P>(gpow, LO + i)), cur);
        if (LO + i == 0)
            odd = bit;
        else
            res = fe_csel(bit, fe_mul(res, fe_sqrt_gpow<P>(gpow, LO + i - 1)), res);
    }
    root = res;
    return !odd || fe_is_zero(u);
}
// g^(2^i), i <= S, 8 Montgomery limbs each: made once per field
template <class P>
inline const uint32_t* h_sqrt_table() {
    static const std::vector<uint32_t> tbl = [] {
        std::vector<uint32_t> t((FieldInfo<P>::S + 1) * 8);
        Fe<P> g = h_root_of_unity<P>();
        for (unsigned i = 0; i <= FieldInfo<P>::S; i++) {
            memcpy(&t[8 * i], g.l, 32);
            g = fe_sqr(g);
        }
        return t;
    }();
    return tbl.data();
}
// square root with the root choice above; false if a is a non-residue
template <class P>
inline bool h_sqrt(const Fe<P>& a, Fe<P>& out) {
    Fe<P> r;
    if (!fe_sqrt_ct(a, h_sqrt_table<P>(), r)) return false;
    out = r;
    return true;
}
// Jacobi symbol (a / p) of a CANONICAL a (plain limbs below p, not Montgomery) by the binary algorithm: +1 a non-zero square,
// -1 a non-square, 0 zero.  Shifts and subtractions only, where a square root costs ~600 products: the circuit's fixed-base
// tables ask it per table entry (the search for z, and the check of a cached table).
template <class P>
inline int h_jacobi(const Fe<P>& canonical) {
    uint64_t a[4], n[4];
    Fe<P> p;
    for (int i = 0; i < 8; i++) p.l[i] = P::mod(i);
    fe_to_u64<P>(a, canonical);
    fe_to_u64<P>(n, p);
    auto is_zero = [](const uint64_t* x) { return (x[0] | x[1] | x[2] | x[3]) == 0; };
    auto shr = [](uint64_t* x, unsigned s) {
        for (; s >= 64; s -= 64) x[0] = x[1], x[1] = x[2], x[2] = x[3], x[3] = 0;
        if (s) {
            for (int i = 0; i < 3; i++) x[i] = (x[i] >> s) | (x[i + 1] << (64 - s));
            x[3] >>= s;
        }
    };
    auto ctz = [](const uint64_t* x) {
        unsigned s = 0;
        for (int i = 0; i < 4 && !x[i]; i++) s += 64;
        return s < 256 ? s + (unsigned)__builtin_ctzll(x[s / 64]) : s;
    };
    auto less = [](const uint64_t* x, const uint64_t* y) {
        for (int i = 3; i >= 0; i--)
            if (x[i] != y[i]) return x[i] < y[i];
        return false;
    };
    int t = 1;
    while (!is_zero(a)) {
        const unsigned z = ctz(a);   // (2 / n) = -1 exactly for n = 3, 5 mod 8
        shr(a, z);
        if ((z & 1) && ((n[0] & 7) == 3 || (n[0] & 7) == 5)) t = -t;
        if (less(a, n)) {            // reciprocity: the sign flips when both are 3 mod 4
            for (int i = 0; i < 4; i++) std::swap(a[i], n[i]);
            if ((a[0] & 3) == 3 && (n[0] & 3) == 3) t = -t;
        }
        uint64_t br = 0;             // a -= n (both odd: a becomes even)
        for (int i = 0; i < 4; i++) {
            const uint64_t d = a[i] - n[i] - br;
            br = a[i] < n[i] || (a[i] == n[i] && br);
            a[i] = d;
        }
    }
    return (n[0] == 1 && !(n[1] | n[2] | n[3])) ? t : 0;
}

// ---------------------------------------------------------------------------
// v[i] <- 1 / v[i], i < n, with ONE field inversion (Montgomery's trick; an inversion is ~12 us on the host).  A zero has no
// inverse: with skip_zeros it stays zero and the others are inverted, without it the call returns false and writes nothing.
// ---------------------------------------------------------------------------
template <class P>
inline bool h_batch_invert(Fe<P>* v, size_t n, bool skip_zeros = false) {
    std::vector<Fe<P>> pre(n + 1);
    pre[0] = fe_one<P>();
    for (size_t i = 0; i < n; i++) {
        const bool zero = fe_is_zero(v[i]);
        if (zero && !skip_zeros) return false;
        pre[i + 1] = zero ? pre[i] : fe_mul(pre[i], v[i]);
    }
    Fe<P> inv = fe_inv(pre[n]);
    for (size_t i = n; i-- > 0;) {
        if (fe_is_zero(v[i])) continue;
        const Fe<P> d = v[i];
        v[i] = fe_mul(inv, pre[i]);
        inv = fe_mul(inv, d);
    }
    return true;
}

// ---------------------------------------------------------------------------
// out[0 .. np) <- the coefficients, lowest first, of the polynomial of degree < np through (points[j], evals[j]), j < np, by
// Lagrange's formula.  inv_den[j] = 1 / prod_(m != j) (points[j] - points[m]): the caller inverts them (h_batch_invert, for many
// interpolations at once).
// ---------------------------------------------------------------------------
template <class P>
inline void h_interpolate(const Fe<P>* points, const Fe<P>* evals, const Fe<P>* inv_den, size_t np, Fe<P>* out) {
    for (size_t i = 0; i < np; i++) out[i] = fe_zero<P>();
    for (size_t j = 0; j < np; j++) {
        std::vector<Fe<P>> num{fe_one<P>()};   // prod_(m != j) (X - points[m])
        for (size_t m = 0; m < np; m++) {
            if (m == j) continue;
            std::vector<Fe<P>> nx(num.size() + 1);
            nx[0] = fe_neg(fe_mul(points[m], num[0]));
            for (size_t i = 1; i < num.size(); i++) nx[i] = fe_sub(num[i - 1], fe_mul(points[m], num[i]));
            nx[num.size()] = num.back();
            num.swap(nx);
        }
        const Fe<P> cf = fe_mul(evals[j], inv_den[j]);
        for (size_t i = 0; i < np; i++) out[i] = fe_add(out[i], fe_mul(cf, num[i]));
    }
}

// ---------------------------------------------------------------------------
// points
// ---------------------------------------------------------------------------
// n Jacobian points (X, Y, Z: 12 limbs each, in in_form) -> affine x || y (8 limbs each, in out_form) with one inversion;
// the identity (Z = 0) maps to (0, 0)
template <class P>
inline void h_jac_to_affine(const uint64_t* xyz, size_t n, int in_form, int out_form, uint64_t* xy) {
    std::vector<Fe<P>> zi(n);
    for (size_t i = 0; i < n; i++) zi[i] = fe_from_u64<P>(xyz + 12 * i + 8, in_form);
    h_batch_invert(zi.data(), n, true);
    for (size_t i = 0; i < n; i++) {
        if (fe_is_zero(zi[i])) {
            memset(xy + 8 * i, 0, 64);
            continue;
        }
        const Fe<P> zi2 = fe_sqr(zi[i]), zi3 = fe_mul(zi2, zi[i]);
        fe_to_u64<P>(xy + 8 * i, fe_mul(fe_from_u64<P>(xyz + 12 * i, in_form), zi2), out_form);
        fe_to_u64<P>(xy + 8 * i + 4, fe_mul(fe_from_u64<P>(xyz + 12 * i + 4, in_form), zi3), out_form);
    }
}
// n XYZZ points -> affine with one inversion: i = 1 / (ZZ ZZZ) gives 1 / ZZ = i ZZZ and 1 / ZZZ = i ZZ; the identity (ZZ = 0)
// maps to (0, 0)
template <class P>
inline void h_xyzz_to_affine(const Xyzz<P>* v, size_t n, Affine<P>* out) {
    std::vector<Fe<P>> zi(n);
    for (size_t i = 0; i < n; i++) zi[i] = fe_mul(v[i].zz, v[i].zzz);
    h_batch_invert(zi.data(), n, true);
    for (size_t i = 0; i < n; i++) {
        out[i].x = fe_mul(v[i].x, fe_mul(zi[i], v[i].zzz));
        out[i].y = fe_mul(v[i].y, fe_mul(zi[i], v[i].zz));
    }
}
// pasta_curves to_bytes: x little-endian, bit 255 = parity of y; the identity (0, 0) = zeros
template <class C>
inline void h_compress(const uint64_t* xy, int form, uint8_t out[32]) {
    using PB = typename C::Base;
    uint64_t x[4], y[4];
    fe_to_u64<PB>(x, fe_from_u64<PB>(xy, form), BZH_FORM_CANONICAL);
    fe_to_u64<PB>(y, fe_from_u64<PB>(xy + 4, form), BZH_FORM_CANONICAL);
    memcpy(out, x, 32);
    out[31] |= (uint8_t)((y[0] & 1) << 7);
}
// pasta_curves from_bytes -> affine canonical x || y; false: x >= p, not on the curve, or a sign bit on the identity
template <class C>
inline bool h_decompress(const uint8_t* in, uint64_t* xy_canonical) {
    using PB = typename C::Base;
    uint8_t raw[32];
    memcpy(raw, in, 32);
    const unsigned ysign = raw[31] >> 7;
    raw[31] &= 0x7f;
    uint64_t xl[4];
    memcpy(xl, raw, 32);
    if (!(xl[0] | xl[1] | xl[2] | xl[3])) {
        if (ysign) return false;
        memset(xy_canonical, 0, 64);
        return true;
    }
    const Fe<PB> x = fe_from_u64<PB>(xl);
    if (!is_canonical(x)) return false;
    const Fe<PB> xm = fe_to_mont(x);
    Fe<PB> y;
    if (!h_sqrt(fe_add(fe_mul(fe_sqr(xm), xm), fe_from_u32<PB>(C::b)), y)) return false;
    Fe<PB> yc = fe_from_mont(y);
    if ((yc.l[0] & 1u) != ysign) yc = fe_from_mont(fe_neg(y));
    fe_to_u64<PB>(xy_canonical, x);
    fe_to_u64<PB>(xy_canonical + 4, yc);
    return true;
}

}  // namespace bzh
