// The two scalar lane bodies of the witness commitments on device-resident transcripts (bzh_commitments_batch_device), as
// host/device functions: what csrc/commitments.hip's k_cm_consts and k_cm_lookup_finish run is what
// tests/helpers/commitments_scalars_check.hip runs on the host against values the test computes.
//   cm_const_lane    one entry of a lookup compress program's constant table (VM v1: 8 saturated Montgomery words per constant,
//                    table[b][i] for a program that names theta, table[i] for one that does not): a literal is copied, the symbol
//                    theta is read from where it was squeezed, in the caller's form, and stored in Montgomery form.  One
//                    descriptor list covers every compress program of the call; each entry names its program's table.
//   cm_status_lane   bit 0 of a proof's status: one of its nl lookups has an input that is not in its table -- lookup_permute's
//                    status word of that pair is not zero
// The literal / symbol choice and the form are selects; the status lane's trip count is the key's nl.
#pragma once
#include "ipa_scalars.hpp"

namespace bzh {

// one constant of one compress program, built on the host from the key's cached programs and the call's workspace
struct CmConst {
    uint32_t* table;      // the program's constant table in device memory
    int32_t sym;          // -1 literal, 0 theta
    uint32_t nconsts;     // constants of that program
    uint32_t index;       // this constant's place among them
    uint32_t per_proof;   // 1: the table has one row per proof, 0: one row
    uint32_t value[8];    // the literal, Montgomery
};

// lane g = b * ndescs + e.  theta: batch elements in the caller's form.
template <class P>
BZH_HD void cm_const_lane(size_t g, const CmConst* descs, size_t ndescs, const void* theta, bool canonical) {
    const size_t b = g / ndescs, e = g - b * ndescs;
    const CmConst d = descs[e];
    if (!d.per_proof && b) return;   // (uniform over an entry's lanes of one proof: the table has a single row)
    Fe<P> th = ipa_at<P>(theta, b);
    if (canonical) th = fe_to_mont(th);   // (uniform over the launch)
    Fe<P> val;
#pragma unroll
    for (int w = 0; w < 8; w++) val.l[w] = d.value[w];
    const Fe<P> v = fe_csel(d.sym < 0, val, th);
    uint32_t* out = d.table + (b * d.nconsts + d.index) * 8;
#pragma unroll
    for (int w = 0; w < 8; w++) out[w] = v.l[w];
}

// words: lookup_permute's status, one per pair, pair = b * nl + lookup
BZH_HD inline uint8_t cm_status_lane(const int32_t* words, size_t nl, size_t b) {
    int32_t any = 0;
    for (size_t l = 0; l < nl; l++) any |= words[b * nl + l];
    return any ? 1 : 0;
}

}  // namespace bzh
