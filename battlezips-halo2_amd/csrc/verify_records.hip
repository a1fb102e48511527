// The four lane kernels of bzh_verify_records_device on gfx950: verify_board / verify_shot (src/wasm/circuit_wasm.rs:86-116,
// 180-194) for a batch of binary records, between one upload of the record bytes and one read-back of a result and a status byte
// per record.
//
// The call itself reads the verifying key and lives with the verifier (csrc/verifier.hpp, part of csrc/prove.hip).  What it adds
// around the device pass (csrc/verify_pass.hip) is small, bodies in verify_records.hpp:
//   k_vr_parse    one lane per (record, input): header and canonical-input check, the instance column in Montgomery form, the
//                 proof rows where the pass reads them, the pre-reject byte per record
//   k_vr_srs      three lanes: G_0 U W of the SRS table in canonical form, compared with the caller's three points
//   k_vr_add_w    one lane per record: the prefix MSM's sum plus W, left for the batch normalisation
//   k_vr_result   one lane per record: the two sums of the opening check compared by cross-multiplication, with the reject bytes
// 64-thread blocks, no LDS, no atomics, plain vector stores: a lane owns what it writes.  A launch for 64 records is one wave (four
// for k_vr_parse on Shot records); its time is the lane's few products or, for k_vr_parse, the row copy.
#include "verify_records.hpp"

namespace bzh {

static constexpr unsigned kVrLanes = 64;

template <class C>
__global__ void __launch_bounds__(kVrLanes) k_vr_parse(const VerifyRecordsArgs a) {
    const size_t g = blockIdx.x * (size_t)kVrLanes + threadIdx.x;   // (record, input)
    if (g >= a.batch * a.n_inputs) return;
    vr_parse_lane<typename CurveInfo<C>::SF>(a, g / a.n_inputs, (uint32_t)(g % a.n_inputs));
}

template <class C>
__global__ void __launch_bounds__(kVrLanes) k_vr_srs(const uint32_t* __restrict__ table, size_t n_srs, const uint32_t* __restrict__ given,
                                                      uint32_t* __restrict__ out_xy, uint8_t* __restrict__ mismatch) {
    if (threadIdx.x >= 3) return;
    vr_srs_lane<C>(table, n_srs, given, threadIdx.x, out_xy, mismatch);
}

template <class C>
__global__ void __launch_bounds__(kVrLanes) k_vr_add_w(uint32_t* __restrict__ jac, const uint32_t* __restrict__ w_xy, size_t batch) {
    const size_t b = blockIdx.x * (size_t)kVrLanes + threadIdx.x;
    if (b >= batch) return;
    vr_add_w_lane<C>(jac, w_xy, b);
}

template <class C>
__global__ void __launch_bounds__(kVrLanes) k_vr_result(const uint32_t* __restrict__ sums, size_t batch, const uint8_t* __restrict__ pre,
                                                         const uint8_t* __restrict__ reject, uint8_t* __restrict__ out, size_t pitch) {
    const size_t b = blockIdx.x * (size_t)kVrLanes + threadIdx.x;
    if (b >= batch) return;
    vr_result_lane<C>(sums, batch, b, pre, reject, out, pitch);
}

static dim3 vr_grid(size_t lanes) { return dim3((unsigned)((lanes + kVrLanes - 1) / kVrLanes)); }

int verify_records_parse(bzh_ctx* ctx, int curve, const VerifyRecordsArgs& a) {
    if (!a.batch) return BZH_OK;
    // what keeps every lane inside its record and its row
    if (!a.n_inputs || a.n_inputs > BZH_RECORD_MAX_INPUTS || (a.rstride & 15) || (a.pstride & 15) || (a.proof_len & 15) ||
        a.proof_len > a.pstride || BZH_RECORD_HEADER_BYTES + (size_t)a.proof_len > a.rstride || a.rstride < BZH_RECORD_HEADER_BYTES + 16)
        return BZH_E_ARG;
    return with_pasta_curve(curve, [&](auto c) -> int {
        hipLaunchKernelGGL((k_vr_parse<decltype(c)>), vr_grid(a.batch * a.n_inputs), dim3(kVrLanes), 0, ctx->stream, a);
        BZH_HIP_TRY(ctx, hipGetLastError());
        return BZH_OK;
    });
}

int verify_records_srs(bzh_ctx* ctx, int curve, const uint32_t* d_table, size_t n_srs, const uint32_t* d_given, uint32_t* d_out_xy,
                       uint8_t* d_mismatch) {
    if (n_srs < 3) return BZH_E_ARG;
    return with_pasta_curve(curve, [&](auto c) -> int {
        hipLaunchKernelGGL((k_vr_srs<decltype(c)>), dim3(1), dim3(kVrLanes), 0, ctx->stream, d_table, n_srs, d_given, d_out_xy, d_mismatch);
        BZH_HIP_TRY(ctx, hipGetLastError());
        return BZH_OK;
    });
}

int verify_records_add_w(bzh_ctx* ctx, int curve, uint32_t* d_jac, const uint32_t* d_w_xy, size_t batch) {
    if (!batch) return BZH_OK;
    return with_pasta_curve(curve, [&](auto c) -> int {
        hipLaunchKernelGGL((k_vr_add_w<decltype(c)>), vr_grid(batch), dim3(kVrLanes), 0, ctx->stream, d_jac, d_w_xy, batch);
        BZH_HIP_TRY(ctx, hipGetLastError());
        return BZH_OK;
    });
}

int verify_records_result(bzh_ctx* ctx, int curve, const uint32_t* d_sums, size_t batch, const uint8_t* d_pre, const uint8_t* d_reject,
                          uint8_t* d_out, size_t pitch) {
    if (!batch) return BZH_OK;
    if (pitch < batch) return BZH_E_ARG;
    return with_pasta_curve(curve, [&](auto c) -> int {
        hipLaunchKernelGGL((k_vr_result<decltype(c)>), vr_grid(batch), dim3(kVrLanes), 0, ctx->stream, d_sums, batch, d_pre, d_reject, d_out,
                           pitch);
        BZH_HIP_TRY(ctx, hipGetLastError());
        return BZH_OK;
    });
}

}  // namespace bzh
