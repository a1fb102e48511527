// The lane bodies of bzh_verify_records_device (verify_board / verify_shot over a batch of binary records), as host/device
// functions: what csrc/verify_records.hip's kernels run is what tests/helpers/verify_records_check.hip runs on the host against
// bzh_record_decode (csrc/record.hip).
//   vr_parse_lane    lane (record b, input i): the header and the record's n_inputs public inputs are read by every lane of the
//                    record -- the loop bound is the launch's, the same for all lanes --, each input is compared limb by limb with
//                    the record format's modulus (Fp, BinaryValue::from_repr(..).to_fp()) and with the key's scalar field, and the
//                    lane knows its record's refusal without talking to its neighbours.  It writes input i in Montgomery form into
//                    the instance column (zero for a refused record), copies the 16-byte units i, i + n_inputs, .. of the proof
//                    into the row the device pass reads (zeros for a refused record and past the proof), and lane 0 writes the
//                    record's pre-reject byte.  Refused: proof_len != the key's, n_inputs != the call's, a non-zero reserved
//                    field, an input that is not canonical.  `kind` and `index` are the caller's tags and are not looked at.
//   vr_srs_lane      lane i < 3: G_0, U, W from row 0 of the SRS window table (affine Montgomery) in canonical form, where the
//                    pass reads them, and one byte that says whether they differ from the three points the caller named
//   vr_add_w_lane    lane b: the prefix MSM's Jacobian sum (Montgomery) plus W, Params::commit_lagrange with blind 1, left in place
//                    as a canonical Jacobian point for the batch normalisation.  A sum that is the identity (an all-zero column,
//                    Z = 0) gives W itself; sum = W doubles and sum = -W gives the identity, through xyzz_madd.
//   vr_result_lane   lane b: the two sums of the opening check compared projectively -- X1 Z2^2 = X2 Z1^2 and Y1 Z2^3 = Y2 Z1^3, or
//                    both Z zero --, folded with the pass's reject byte into results[b], and the pre-reject byte into status[b]
// No lane reads another lane's output; no LDS, no atomics.
#pragma once
#include "ctx.hpp"
#include "curve.cuh"
#include "host_field.hpp"
#include "normalize.hpp"   // norm_load / norm_store; with it hash_to_curve.hpp: fe_lt_p

namespace bzh {

// 16 bytes from src to dst, or zeros: one dwordx4 move on the device (both 16-byte aligned there), bytes on the host
BZH_HD void vr_move16(uint8_t* dst, const uint8_t* src, bool live) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint4 v = *(const uint4*)src;
    *(uint4*)dst = live ? v : make_uint4(0, 0, 0, 0);
#else
    if (live)
        memcpy(dst, src, 16);
    else
        memset(dst, 0, 16);
#endif
}
BZH_HD uint32_t vr_word(const uint8_t* p, int i) {
#if defined(__HIP_DEVICE_COMPILE__)
    return ((const uint32_t*)p)[i];
#else
    uint32_t v;
    memcpy(&v, p + 4 * i, 4);
    return v;
#endif
}
// the limbs of x as an element of another field: below that field's modulus?
template <class Q, class P>
BZH_HD bool vr_below(const Fe<P>& x) {
    Fe<Q> t;
#pragma unroll
    for (int k = 0; k < 8; k++) t.l[k] = x.l[k];
    return fe_lt_p(t);
}

// what refuses a record before verification, in two pieces: the header against what the call expects, and one public input
// against the record format's modulus and the key's scalar field
BZH_HD bool vr_header_refused(const uint8_t* rec, uint32_t proof_len, uint32_t n_inputs) {
    const uint32_t w0 = vr_word(rec, 0), w1 = vr_word(rec, 1), w3 = vr_word(rec, 3);
    return w0 != proof_len || (w1 & 0xffu) != n_inputs || (w1 >> 16) != 0 || w3 != 0;
}
template <class SF>
BZH_HD bool vr_input_refused(const Fe<SF>& v) {
    return !vr_below<FpParams>(v) || !fe_lt_p(v);
}
// the same decision for a whole record on the host (the accumulated call: a batch refused to the last record launches no MSM)
template <class SF>
inline bool vr_record_refused_host(const uint8_t* rec, uint32_t proof_len, uint32_t n_inputs) {
    bool refuse = vr_header_refused(rec, proof_len, n_inputs);
    for (uint32_t j = 0; j < n_inputs; j++) refuse = refuse || vr_input_refused<SF>(norm_load<SF>(rec + 16 + 32 * (size_t)j));
    return refuse;
}

// a: VerifyRecordsArgs (csrc/ctx.hpp); SF: the key's scalar field
template <class SF, class A>
BZH_HD void vr_parse_lane(const A& a, size_t b, uint32_t i) {
    const uint8_t* rec = a.d_records + b * a.rstride;
    bool refuse = vr_header_refused(rec, a.proof_len, a.n_inputs);
    Fe<SF> mine = fe_zero<SF>();
#pragma unroll 1
    for (uint32_t j = 0; j < a.n_inputs; j++) {
        const Fe<SF> v = norm_load<SF>(rec + 16 + 32 * (size_t)j);
        refuse = refuse || vr_input_refused<SF>(v);
        mine = fe_csel(j == i, v, mine);
    }
    norm_store<SF>(a.d_inst + (b * a.n_inputs + i) * 8, fe_to_mont(fe_csel(!refuse, mine, fe_zero<SF>())));
    if (i == 0) a.d_pre[b] = refuse ? 1 : 0;
    const uint8_t* proof = rec + BZH_RECORD_HEADER_BYTES;
    uint8_t* row = a.d_rows + b * a.pstride;
#pragma unroll 1
    for (size_t u = i; u < a.pstride / 16; u += a.n_inputs) {
        const bool inside = 16 * u + 16 <= a.proof_len;   // (proof_len is a multiple of 16: checked by the call)
        vr_move16(row + 16 * u, inside ? proof + 16 * u : proof, inside && !refuse);
    }
}

// table: row 0 of the SRS window table, n_srs = n + 2 affine Montgomery points; given: 3 x 16 canonical words or null
template <class C>
BZH_HD void vr_srs_lane(const uint32_t* table, size_t n_srs, const uint32_t* given, uint32_t i, uint32_t* out_xy, uint8_t* mismatch) {
    using PB = typename C::Base;
    const size_t idx = i == 0 ? 0 : n_srs - 3 + i;   // G_0, U, W
    const Fe<PB> x = fe_from_mont(norm_load<PB>(table + idx * 16)), y = fe_from_mont(norm_load<PB>(table + idx * 16 + 8));
    norm_store<PB>(out_xy + i * 16, x);
    norm_store<PB>(out_xy + i * 16 + 8, y);
    bool differs = false;
    if (given) differs = !fe_eq(x, norm_load<PB>(given + i * 16)) || !fe_eq(y, norm_load<PB>(given + i * 16 + 8));
    mismatch[i] = differs ? 1 : 0;
}

// jac: batch x 24 words X || Y || Z (Montgomery in, canonical out); w_xy: W, affine Montgomery
template <class C>
BZH_HD void vr_add_w_lane(uint32_t* jac, const uint32_t* w_xy, size_t b) {
    using PB = typename C::Base;
    uint32_t* p = jac + b * 24;
    const Fe<PB> X = norm_load<PB>(p), Y = norm_load<PB>(p + 8), Z = norm_load<PB>(p + 16);
    Xyzz<PB> acc = xyzz_identity<PB>();
    if (!fe_is_zero(Z)) {
        acc.x = X, acc.y = Y;
        acc.zz = fe_sqr(Z);
        acc.zzz = fe_mul(acc.zz, Z);
    }
    Affine<PB> w;
    w.x = norm_load<PB>(w_xy), w.y = norm_load<PB>(w_xy + 8);
    xyzz_madd(acc, w);
    Fe<PB> X3, Y3, Z3;
    xyzz_to_jacobian(acc, X3, Y3, Z3);
    norm_store<PB>(p, fe_from_mont(X3));
    norm_store<PB>(p + 8, fe_from_mont(Y3));
    norm_store<PB>(p + 16, fe_from_mont(Z3));
}

// sums: the right sides' Jacobian points (batch x 24 words), then the left sides'; either form, the same for both.
// out: results at out[b], status at out[pitch + b]
template <class C>
BZH_HD void vr_result_lane(const uint32_t* sums, size_t batch, size_t b, const uint8_t* pre, const uint8_t* reject, uint8_t* out, size_t pitch) {
    using PB = typename C::Base;
    const uint32_t *r = sums + b * 24, *l = sums + (batch + b) * 24;
    const Fe<PB> X1 = norm_load<PB>(r), Y1 = norm_load<PB>(r + 8), Z1 = norm_load<PB>(r + 16);
    const Fe<PB> X2 = norm_load<PB>(l), Y2 = norm_load<PB>(l + 8), Z2 = norm_load<PB>(l + 16);
    const bool id1 = fe_is_zero(Z1), id2 = fe_is_zero(Z2);
    const Fe<PB> z1s = fe_sqr(Z1), z2s = fe_sqr(Z2);
    const bool ex = fe_eq(fe_mul(X1, z2s), fe_mul(X2, z1s));
    const bool ey = fe_eq(fe_mul(Y1, fe_mul(z2s, Z2)), fe_mul(Y2, fe_mul(z1s, Z1)));
    const bool equal = (id1 && id2) || (!id1 && !id2 && ex && ey);
    const bool refused = pre[b] != 0;
    out[b] = (equal && !refused && reject[b] == 0) ? 1 : 0;
    out[pitch + b] = refused ? 1 : 0;
}

}  // namespace bzh
