// The circuit front end's field and curve types (witness synthesis, keygen constants): value types with operators over the
// library's one host field library, bzh::Fe<P> (csrc/field.cuh, csrc/host_field.hpp, csrc/curve.cuh).  No arithmetic lives
// here.  A value is 8 x 32-bit Montgomery limbs with R = 2^256: the memory image of the device's field elements and of
// pasta_curves' in-memory Fp / Fq (4 x 64-bit limbs, little-endian), so synthesised advice columns are uploaded without
// conversion.
//
// Stands where the reference reaches pasta_curves 0.4.1 (Cargo.lock:567-570, un-vendored) from its chips:
// src/chips/bitify.rs:117-123 (field adds / muls), src/chips/placement.rs:196 (lagrange_interpolate), and, through
// halo2_gadgets' ECC chip, the affine Pallas arithmetic of src/chips/pedersen.rs:104-134.
#pragma once
#include <stdint.h>
#include <string.h>

#include <array>
#include <type_traits>
#include <vector>

#include "../host_field.hpp"

namespace bzc {

template <class P>
struct F {
    bzh::Fe<P> fe;

    F() = default;
    F(const bzh::Fe<P>& v) : fe(v) {}
    operator const bzh::Fe<P>&() const { return fe; }

    static F zero() { return bzh::fe_zero<P>(); }
    static F one() { return bzh::fe_one<P>(); }
    // any 256-bit integer (little-endian limbs) mod p -> Montgomery
    static F from_raw_reduce(std::array<uint64_t, 4> c) { return bzh::fe_from_u64<P>(c.data(), BZH_FORM_CANONICAL); }
    static F from_u64(uint64_t v) { return from_raw_reduce({v, 0, 0, 0}); }
    static F from_u128(const std::array<uint64_t, 2>& v) { return from_raw_reduce({v[0], v[1], 0, 0}); }
    static bool is_canonical(const uint64_t* c) { return bzh::is_canonical(bzh::fe_from_u64<P>(c)); }
    // 32 canonical little-endian bytes; false if >= p (from_repr(..) is None upstream)
    static bool from_repr(const uint8_t* b, F* out) {
        uint64_t c[4];
        memcpy(c, b, 32);
        return from_limbs(c, out);
    }
    static bool from_limbs(const uint64_t* c, F* out) {
        if (!is_canonical(c)) return false;
        *out = bzh::fe_from_u64<P>(c, BZH_FORM_CANONICAL);
        return true;
    }
    void to_limbs(uint64_t* out) const { bzh::fe_to_u64<P>(out, fe, BZH_FORM_CANONICAL); }  // canonical
    void to_repr(uint8_t* out) const {
        const std::array<uint64_t, 4> c = canon();
        memcpy(out, c.data(), 32);
    }
    std::array<uint64_t, 4> canon() const {
        std::array<uint64_t, 4> c;
        to_limbs(c.data());
        return c;
    }

    bool is_zero() const { return bzh::fe_is_zero(fe); }
    bool is_odd() const { return canon()[0] & 1; }
    friend bool operator==(const F& a, const F& b) { return bzh::fe_eq(a.fe, b.fe); }
    friend bool operator!=(const F& a, const F& b) { return !(a == b); }
    friend F operator+(const F& a, const F& b) { return bzh::fe_add(a.fe, b.fe); }
    friend F operator-(const F& a, const F& b) { return bzh::fe_sub(a.fe, b.fe); }
    friend F operator*(const F& a, const F& b) { return bzh::fe_mul(a.fe, b.fe); }
    F operator-() const { return bzh::fe_neg(fe); }
    F dbl() const { return bzh::fe_dbl(fe); }
    F sqr() const { return bzh::fe_sqr(fe); }
    // 0 -> 0, like ff's invert().unwrap_or(0) call sites in the ECC witness code
    F inv() const { return bzh::fe_inv(fe); }
    // +1 square, -1 non-square, 0 zero
    int jacobi() const { return bzh::h_jacobi(bzh::fe_from_mont(fe)); }
    // the root pasta_curves' `sqrt` returns (csrc/host_field.hpp states the choice); false for a non-square
    bool sqrt(F* out) const { return bzh::h_sqrt(fe, out->fe); }
};
typedef F<bzh::FpParams> Fp;  // Pallas base field = Vesta scalar field = the circuit field (modulus literal: src/chips/bitify.rs:461)
typedef F<bzh::FqParams> Fq;  // Pallas scalar field
// a vector of values is a vector of bzh::Fe<P> to the helpers below, and pinned staging memory is written as Fp
static_assert(sizeof(Fp) == 32 && sizeof(Fq) == 32, "a value is its eight limbs");
static_assert(sizeof(Fp) == sizeof(bzh::Fe<bzh::FpParams>) && sizeof(Fq) == sizeof(bzh::Fe<bzh::FqParams>) &&
                  std::is_standard_layout<Fp>::value && std::is_standard_layout<Fq>::value,
              "fe_ptr reads an array of values as an array of bzh::Fe<P>");
static_assert(alignof(Fp) == alignof(bzh::Fe<bzh::FpParams>) && alignof(Fp) <= alignof(uint64_t), "no stricter than the limb buffers cast to it");

template <class P>
inline bzh::Fe<P>* fe_ptr(F<P>* v) {
    return reinterpret_cast<bzh::Fe<P>*>(v);
}
template <class P>
inline const bzh::Fe<P>* fe_ptr(const F<P>* v) {
    return reinterpret_cast<const bzh::Fe<P>*>(v);
}

template <class P>
inline void batch_invert(std::vector<F<P>>& v) {  // zeros stay zero
    bzh::h_batch_invert(fe_ptr(v.data()), v.size(), true);
}

// arithmetic::lagrange_interpolate (UPSTREAM halo2_proofs 0.2.0; call site src/chips/placement.rs:196): coefficients,
// low to high, of the polynomial of degree < n through (points[i], evals[i]).
template <class P>
inline std::vector<F<P>> lagrange_interpolate(const std::vector<F<P>>& points, const std::vector<F<P>>& evals) {
    const size_t n = points.size();
    std::vector<F<P>> den(n, F<P>::one()), res(n);
    for (size_t j = 0; j < n; j++) {
        for (size_t m = 0; m < n; m++) {
            if (m != j) den[j] = den[j] * (points[j] - points[m]);
        }
    }
    batch_invert(den);
    bzh::h_interpolate(fe_ptr(points.data()), fe_ptr(evals.data()), fe_ptr(den.data()), n, fe_ptr(res.data()));
    return res;
}

// Pallas: y^2 = x^3 + 5 over Fp.  Affine points, (0, 0) the identity (halo2_gadgets' convention in the circuit); sums are
// accumulated in XYZZ (csrc/curve.cuh) and normalised with bzh::h_xyzz_to_affine.
typedef bzh::Affine<bzh::FpParams> Aff;
typedef bzh::Xyzz<bzh::FpParams> Xyzz;

}  // namespace bzc
