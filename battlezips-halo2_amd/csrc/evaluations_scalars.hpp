// The small per-proof scalar work of the evaluation phase on device-resident transcripts (bzh_evaluations_batch_device), one lane
// per proof or per (proof, query), as host/device functions: what csrc/evaluations.hip's lane kernels run is what
// tests/helpers/evaluations_scalars_check.hip runs on the host against fe_mul / fe_sqr / fe_add (csrc/host_field.hpp).  x and
// x^n are in Montgomery form; a caller's array is in Montgomery form unless the `canonical` flag says otherwise.
//   ev_points_lane   out_points[b][j] = x_b * omega^rotation_j for the nrot distinct rotations, from the table of omega^rotation_j
//   ev_xn_lane       xn[b] = x_b^(2^k) by k squarings
//   ev_hblind_lane   out[b] = sum_i xn_b^i * h_blinds[b][i], Horner from the top piece down
//   ev_export_lane   one evaluation from the slot the transcript absorbed it from to the caller's array
// No branch and no trip count depends on a lane's data.
#pragma once
#include "ipa_scalars.hpp"

namespace bzh {

static constexpr size_t kEvMaxRotations = 8;   // BZH_EVAL_MAX_ROTATIONS

// omegas: nrot elements, Montgomery, the same for every proof
template <class P>
BZH_HD void ev_points_lane(size_t b, const void* xs, const void* omegas, size_t nrot, bool canonical, void* out_points) {
    const Fe<P> x = ipa_at<P>(xs, b);
    for (size_t j = 0; j < nrot; j++) {
        const Fe<P> pt = fe_mul(x, ipa_at<P>(omegas, j));
        ipa_put<P>(out_points, b * nrot + j, canonical ? fe_from_mont(pt) : pt);
    }
}

template <class P>
BZH_HD void ev_xn_lane(size_t b, const void* xs, unsigned k, void* xn) {
    Fe<P> acc = ipa_at<P>(xs, b);
    for (unsigned i = 0; i < k; i++) acc = fe_sqr(acc);
    ipa_put<P>(xn, b, acc);
}

// h_blinds: batch x npieces in the caller's form; out[b] in the same form
template <class P>
BZH_HD void ev_hblind_lane(size_t b, const void* xn, const void* h_blinds, size_t npieces, bool canonical, void* out) {
    const Fe<P> y = ipa_at<P>(xn, b);
    Fe<P> acc = fe_zero<P>();
    for (size_t i = npieces; i-- > 0;) {
        const Fe<P> bl = ipa_at<P>(h_blinds, b * npieces + i);
        acc = fe_add(fe_mul(acc, y), canonical ? fe_to_mont(bl) : bl);
    }
    ipa_put<P>(out, b, canonical ? fe_from_mont(acc) : acc);
}

// evals: batch x nqueries, Montgomery
template <class P>
BZH_HD void ev_export_lane(size_t g, const void* evals, bool canonical, void* out) {
    const Fe<P> v = ipa_at<P>(evals, g);
    ipa_put<P>(out, g, canonical ? fe_from_mont(v) : v);
}

}  // namespace bzh
