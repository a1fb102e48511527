// The scalar arithmetic between the rounds of the inner-product-argument opening, one lane per proof, as host/device functions:
// what csrc/ipa.hip's k_ipa_head_scalars and k_ipa_round_scalars run for bzh_ipa_open_batch_device is what
// tests/helpers/ipa_scalars_check.hip runs on the host against the arithmetic the host-transcript opening does between its rounds
// (fe_mul, fe_add, h_batch_invert).  Everything is in Montgomery form unless a `canonical` flag says otherwise.
//   ipa_x3_lane     hc[b][0] = x3_b (given in `form`), status[b] = 0: the start of a call
//   ipa_head_lane   after S: xi, z (the two squeezes) -> hc[b][1], hc[b][2];  f_b = s_blind_b * xi + blind_b
//   ipa_round_lane  after (L_j, R_j): u_j (the squeeze) -> hc[b][3] = u_j, hc[b][4] = u_j^-1 (fe_inv_ct: 0 for 0);
//                   f_b += l_j * u_j^-1 + r_j * u_j;  status[b] |= (u_j == 0)
//   ipa_tail_lane   cf[b] = (c_b, f_b) for the transcript's write_scalars, out_v[b] = v_b in `form`
// No branch and no trip count depends on a lane's data: a zero challenge has no inverse, fe_inv_ct gives 0 for it, the l_j term
// then adds nothing and the status byte says so.
#pragma once
#include "normalize.hpp"

namespace bzh {

// per-proof constants the round kernels read (d_hc): [0] x3, [1] xi, [2] z, [3] u, [4] u_inv   (stride kHc elements)
static constexpr size_t kHc = 8;

// element i of a vector of 32-byte field elements
template <class P>
BZH_HD Fe<P> ipa_at(const void* base, size_t i) {
    return norm_load<P>((const char*)base + i * 32);
}
template <class P>
BZH_HD void ipa_put(void* base, size_t i, const Fe<P>& v) {
    norm_store<P>((char*)base + i * 32, v);
}

template <class P>
BZH_HD void ipa_x3_lane(size_t b, const void* x3s, bool canonical, void* hc, uint8_t* status) {
    const Fe<P> x = ipa_at<P>(x3s, b);
    ipa_put<P>(hc, b * kHc, canonical ? fe_to_mont(x) : x);
    if (status) status[b] = 0;
}

// ch: the two squeezes after S, batch elements each (xi at ch[b], z at ch[batch + b]); rands: batch x nrand drawn scalars, the
// blind of S at [n]
template <class P>
BZH_HD void ipa_head_lane(size_t b, size_t batch, const void* ch, const void* rands, size_t nrand, size_t n, const void* blinds,
                          bool canonical, void* hc, void* f) {
    const Fe<P> xi = ipa_at<P>(ch, b), z = ipa_at<P>(ch, batch + b);
    const Fe<P> bl = ipa_at<P>(blinds, b);
    ipa_put<P>(hc, b * kHc + 1, xi);
    ipa_put<P>(hc, b * kHc + 2, z);
    ipa_put<P>(f, b, fe_add(fe_mul(ipa_at<P>(rands, b * nrand + n), xi), canonical ? fe_to_mont(bl) : bl));
}

// ch: the squeeze after (L_j, R_j), u_j of proof b at ch[b]; the round's blinds l_j, r_j at rands[b][n + 1 + 2 j], [n + 2 + 2 j]
template <class P>
BZH_HD void ipa_round_lane(size_t b, const void* ch, const void* rands, size_t nrand, size_t n, unsigned round, void* hc, void* f,
                           uint8_t* status) {
    const Fe<P> u = ipa_at<P>(ch, b);
    const Fe<P> ui = fe_inv_ct(u);
    ipa_put<P>(hc, b * kHc + 3, u);
    ipa_put<P>(hc, b * kHc + 4, ui);
    const size_t at = b * nrand + n + 1 + 2 * (size_t)round;
    const Fe<P> acc = ipa_at<P>(f, b);
    ipa_put<P>(f, b, fe_add(acc, fe_add(fe_mul(ipa_at<P>(rands, at), ui), fe_mul(ipa_at<P>(rands, at + 1), u))));
    if (status) status[b] |= (uint8_t)(fe_is_zero(u) ? 1 : 0);
}

// p: the folded polynomial, one element per proof by now; v: p_b(x3_b)
template <class P>
BZH_HD void ipa_tail_lane(size_t b, const void* p, const void* f, const void* v, bool canonical, void* cf, void* out_v) {
    ipa_put<P>(cf, 2 * b, ipa_at<P>(p, b));
    ipa_put<P>(cf, 2 * b + 1, ipa_at<P>(f, b));
    const Fe<P> vm = ipa_at<P>(v, b);
    ipa_put<P>(out_v, b, canonical ? fe_from_mont(vm) : vm);
}

}  // namespace bzh
