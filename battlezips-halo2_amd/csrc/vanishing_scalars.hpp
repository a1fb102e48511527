// The constant table of the quotient program for the vanishing argument on device-resident transcripts
// (bzh_vanishing_batch_device), one lane per (proof, constant), as a host/device function: what csrc/vanishing.hip's k_vn_consts
// runs is what tests/helpers/vanishing_scalars_check.hip runs on the host against fe_mul / h_pow_u64 (csrc/host_field.hpp).
//   vn_const_lane   table[b][i] = value_i * challenge_b^exponent_i for a symbol, value_i for a literal, from the descriptors of
//                   bzh_vanishing_plan and the four challenges theta, beta, gamma, y of proof b; written as 8 saturated words, or
//                   as the 12-word slot with 9 fe29 limbs the unsaturated quotient kernel reads (fe29_from_sat_reduced)
// The power is seven square-and-multiply steps (exponents are at most 64) whatever the exponent is: the challenge, the bit and
// the literal / symbol choice are selects, so no branch and no trip count depends on a lane's data or on the table.
#pragma once
#include "fe29.cuh"
#include "ipa_scalars.hpp"

namespace bzh {

// one entry of the plan: the layout of bzh_vanishing_const (include/bzh2.h)
struct VnConst {
    int32_t challenge;    // -1 literal, 0 theta, 1 beta, 2 gamma, 3 y
    uint32_t exponent;    // <= kVnMaxExponent
    uint32_t value[8];    // Montgomery
};
static constexpr uint32_t kVnMaxExponent = 64;
static constexpr int kVnPowSteps = 7;   // bits of kVnMaxExponent
static constexpr size_t kVnSlot29 = 12;   // words of one constant in the unsaturated kernel's table

// lane g = b * nconsts + i.  theta, beta, gamma: batch elements each, in the caller's form; y: batch elements, Montgomery.
// table: batch x nconsts slots of 8 words (planes29 false) or kVnSlot29 words (true).
template <class P>
BZH_HD void vn_const_lane(size_t g, const VnConst* descs, size_t nconsts, const void* theta, const void* beta, const void* gamma,
                          const void* y, bool canonical, bool planes29, uint32_t* table) {
    const size_t b = g / nconsts, i = g - b * nconsts;
    const VnConst d = descs[i];
    Fe<P> th = ipa_at<P>(theta, b), be = ipa_at<P>(beta, b), ga = ipa_at<P>(gamma, b);
    if (canonical) th = fe_to_mont(th), be = fe_to_mont(be), ga = fe_to_mont(ga);   // (uniform over the launch)
    const Fe<P> c = fe_csel(d.challenge == 0, th, fe_csel(d.challenge == 1, be, fe_csel(d.challenge == 2, ga, ipa_at<P>(y, b))));
    Fe<P> pw = fe_one<P>();
#pragma unroll
    for (int bit = kVnPowSteps - 1; bit >= 0; bit--) {
        pw = fe_sqr(pw);
        pw = fe_csel(((d.exponent >> bit) & 1u) != 0, fe_mul(pw, c), pw);
    }
    Fe<P> val;
#pragma unroll
    for (int w = 0; w < 8; w++) val.l[w] = d.value[w];
    const Fe<P> v = fe_csel(d.challenge < 0, val, fe_mul(val, pw));
    if (planes29) {
        if constexpr (fe29_supported<P>()) {
            const Fe29<P> w29 = fe29_from_sat_reduced(v);
            uint32_t* out = table + g * kVnSlot29;
#pragma unroll
            for (int w = 0; w < 9; w++) out[w] = w29.l[w];
            out[9] = out[10] = out[11] = 0;
        }
    } else {
        uint32_t* out = table + g * 8;
#pragma unroll
        for (int w = 0; w < 8; w++) out[w] = v.l[w];
    }
}

}  // namespace bzh
