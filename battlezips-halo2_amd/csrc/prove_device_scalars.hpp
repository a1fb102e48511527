// The two lane bodies of the device-resident batch prover (bzh_prove_batch_device), as host/device functions: what
// csrc/prove_device.hip's k_pd_blinds and k_pd_status run is what tests/helpers/prove_device_scalars_check.hip runs on the host
// against a plain loop.
//   pd_blind_lane    the blind of opened polynomial j of proof b into the [batch][nown] row the multiopen reads.  The opened
//                    polynomials are runs of the leaves' outputs -- instance columns (blind one), advice, the random polynomial,
//                    the grand products, the permuted lookup columns, h(X) -- and each run is one PdBlindSrc: a pointer, the
//                    elements between proofs, the run's length and its first index.  A null pointer stands for Montgomery 1; a run
//                    of length 0 (ni = 0, nl = 0) matches no lane; a stride of 0 gives every proof the same elements.
//   pd_status_lane   the four leaves' status bytes of proof b folded into one byte -- bit 0 a lookup input is not in its table, bit 1
//                    a grand product does not close, bit 2 the quotient's degree check failed, bit 3 the multiopen or the opening
//                    flagged the proof -- and written with the proof's length into the call's read-back slot.
// The run of a lane is chosen by selects over the table, whose length is the launch's; nothing depends on a lane's data.
#pragma once
#include "ipa_scalars.hpp"

namespace bzh {

struct PdBlindSrc {
    const uint32_t* p;   // null: Montgomery 1
    uint64_t stride;     // elements between proofs
    uint32_t first;      // index of the run's first polynomial among the opened ones
    uint32_t count;
};

// lane g = b * nown + j (the polynomial index is fastest: a wave's stores are contiguous)
template <class P>
BZH_HD void pd_blind_lane(size_t g, const PdBlindSrc* srcs, size_t nsrc, size_t nown, void* out) {
    const size_t b = g / nown, j = g - b * nown;
    const uint32_t* at = nullptr;
    for (size_t s = 0; s < nsrc; s++) {
        const PdBlindSrc r = srcs[s];
        const bool in = r.p && j >= r.first && j - r.first < r.count;
        at = in ? r.p + (b * r.stride + (j - r.first)) * 8 : at;
    }
    const Fe<P> v = at ? ipa_at<P>(at, 0) : fe_one<P>();
    ipa_put<P>(out, g, v);
}

// leaf: four rows of status bytes, leaf_stride apart, in chain order; slot: two words per proof (status, proof length)
BZH_HD void pd_status_lane(size_t b, const uint8_t* leaf, size_t leaf_stride, uint32_t proof_len, uint32_t* slot) {
    uint32_t st = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) st |= (leaf[(size_t)i * leaf_stride + b] ? 1u : 0u) << i;
    slot[2 * b] = st;
    slot[2 * b + 1] = proof_len;
}

}  // namespace bzh
