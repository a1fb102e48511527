// Host-side field and curve helpers of the library (portable Fe<P> arithmetic, csrc/field.cuh's host product) and the
// dispatch from a runtime field / curve id (include/bzh2.h) to the parameter pack: the one home of the per-field constants,
// limb marshalling, roots of unity, the square root, batch inversion, Jacobian -> affine and point (de)compression.
// Host only; Montgomery form unless noted.
#pragma once
#include <cstring>
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
// square root (Tonelli-Shanks); false if a is a non-residue
template <class P>
inline bool h_sqrt(const Fe<P>& a, Fe<P>& out) {
    if (fe_is_zero(a)) {
        out = a;
        return true;
    }
    constexpr unsigned S = FieldInfo<P>::S;
    uint32_t t[8], t1h[8];
    h_pm1_shr<P>(S, t);          // t = (p - 1) / 2^S, odd
    h_pm1_shr<P>(S + 1, t1h);    // (t + 1) / 2 = (t >> 1) + 1
    for (int i = 0; i < 8 && ++t1h[i] == 0; i++) {
    }
    Fe<P> zgen = fe_pow(fe_from_u32<P>(FieldInfo<P>::gen), t);
    Fe<P> x = fe_pow(a, t1h), b = fe_pow(a, t);
    const Fe<P> one = fe_one<P>();
    unsigned m = S;
    while (!fe_eq(b, one)) {
        unsigned i = 0;
        Fe<P> b2 = b;
        while (!fe_eq(b2, one)) {
            b2 = fe_sqr(b2);
            i++;
            if (i >= m) return false;  // not a square
        }
        Fe<P> w = zgen;
        for (unsigned k = 0; k + i + 1 < m; k++) w = fe_sqr(w);
        zgen = fe_sqr(w);
        x = fe_mul(x, w);
        b = fe_mul(b, zgen);
        m = i;
    }
    out = x;
    return fe_eq(fe_sqr(x), a);
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
