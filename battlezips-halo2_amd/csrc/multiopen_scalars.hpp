// The small per-proof scalar work of the multiopen argument on device-resident transcripts (bzh_multiopen_batch_device), one lane
// per (proof, point set) or per proof, as host/device functions: what csrc/multiopen.hip's lane kernels run is what
// tests/helpers/multiopen_scalars_check.hip runs on the host against h_interpolate / h_batch_invert and fe_mul / fe_add
// (csrc/host_field.hpp).  Everything is in Montgomery form unless a `canonical` flag says otherwise.
//   mo_point_lane        one opening point of a proof, from the caller's array (in `form`) to its place in the division's order
//   mo_blind_lane        q_blind = Horner in x1 over the blinds of a set's polynomials, in group order
//   mo_interpolate_lane  r(X) through (point_j, q(point_j)), j < np <= 8: the denominators prod_(m != j) (x_j - x_m), one
//                        fe_inv_ct each, the 8 coefficients of r (zero from np on), and a flag: some denominator was zero
//   mo_final_blind_lane  p_blind = Horner in x4 over (f_blind, q_blind_0, ..)
//   mo_status_lane       status[b] = bit 0: a flag of proof b is set | bit 1: the opening reported a zero round challenge
// No branch and no trip count depends on a lane's data (they depend on the set, which is the same for every proof): two equal
// points give a zero denominator, fe_inv_ct gives 0 for it, that term of r vanishes and the flag says so.
#pragma once
#include "ipa_scalars.hpp"

namespace bzh {

static constexpr size_t kMoMaxPoints = 8;   // BZH_MULTIOPEN_MAX_POINTS

// out[at] = points[b][id] in Montgomery form
template <class P>
BZH_HD void mo_point_lane(size_t b, const void* points, size_t npoints, uint32_t id, bool canonical, void* out, size_t at) {
    const Fe<P> x = ipa_at<P>(points, b * npoints + id);
    ipa_put<P>(out, at, canonical ? fe_to_mont(x) : x);
}

// ids[0 .. count): the set's polynomials in group order; an id below npolys_own is proof b's own polynomial, the rest are shared
template <class P>
BZH_HD void mo_blind_lane(size_t b, const void* x1s, const void* blinds, size_t npolys_own, const void* shared_blinds, const uint32_t* ids,
                          size_t count, bool canonical, void* out, size_t at) {
    const Fe<P> x1 = ipa_at<P>(x1s, b);
    Fe<P> acc = fe_zero<P>();
    for (size_t c = 0; c < count; c++) {
        const uint32_t id = ids[c];
        const Fe<P> bl = id < npolys_own ? ipa_at<P>(blinds, b * npolys_own + id) : ipa_at<P>(shared_blinds, id - npolys_own);
        acc = fe_add(fe_mul(acc, x1), canonical ? fe_to_mont(bl) : bl);
    }
    ipa_put<P>(out, at, acc);
}

// point j and q(point j) of this lane at xs / evs [first + at[j] * step], j < np; r: kMoMaxPoints coefficients, lowest first
template <class P>
BZH_HD void mo_interpolate_lane(const void* xs, const void* evs, size_t first, const uint32_t* at, size_t step, size_t np, void* r,
                                uint8_t* flag) {
    Fe<P> x[kMoMaxPoints], out[kMoMaxPoints], num[kMoMaxPoints];
    for (size_t j = 0; j < kMoMaxPoints; j++) out[j] = fe_zero<P>();
    for (size_t j = 0; j < np; j++) x[j] = ipa_at<P>(xs, first + at[j] * step);
    bool zero = false;
    for (size_t j = 0; j < np; j++) {
        // num = prod_(m != j) (X - x_m), len coefficients; den = prod_(m != j) (x_j - x_m)
        Fe<P> den = fe_one<P>();
        size_t len = 1;
        num[0] = fe_one<P>();
        for (size_t m = 0; m < np; m++) {
            if (m == j) continue;
            den = fe_mul(den, fe_sub(x[j], x[m]));
            num[len] = num[len - 1];
            for (size_t i = len - 1; i >= 1; i--) num[i] = fe_sub(num[i - 1], fe_mul(x[m], num[i]));
            num[0] = fe_neg(fe_mul(x[m], num[0]));
            len++;
        }
        zero |= fe_is_zero(den);
        const Fe<P> cf = fe_mul(ipa_at<P>(evs, first + at[j] * step), fe_inv_ct(den));
        for (size_t i = 0; i < np; i++) out[i] = fe_add(out[i], fe_mul(cf, num[i]));
    }
    for (size_t i = 0; i < kMoMaxPoints; i++) ipa_put<P>(r, i, out[i]);
    *flag = (uint8_t)(zero ? 1 : 0);
}

// q_blinds: nsets x batch, set s of proof b at [s * batch + b]
template <class P>
BZH_HD void mo_final_blind_lane(size_t b, size_t batch, const void* x4s, const void* f_blinds, const void* q_blinds, size_t nsets,
                                void* out) {
    const Fe<P> x4 = ipa_at<P>(x4s, b);
    Fe<P> acc = ipa_at<P>(f_blinds, b);
    for (size_t s = 0; s < nsets; s++) acc = fe_add(fe_mul(acc, x4), ipa_at<P>(q_blinds, s * batch + b));
    ipa_put<P>(out, b, acc);
}

// flags: nsets x batch bytes from mo_interpolate_lane; ipa_status: the opening's byte per proof
BZH_HD void mo_status_lane(size_t b, size_t batch, const uint8_t* flags, size_t nsets, const uint8_t* ipa_status, uint8_t* status) {
    uint8_t any = 0;
    for (size_t s = 0; s < nsets; s++) any |= flags[s * batch + b];
    status[b] = (uint8_t)((any ? 1 : 0) | (ipa_status[b] ? 2 : 0));
}

}  // namespace bzh
