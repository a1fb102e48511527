// The verifier's per-proof host pass on gfx950 (BZH_VERIFY_PASS_DEVICE): the kernels around the key's scalar program
// (csrc/verify_program.hpp).  csrc/verifier.hpp's verify_batch_device_t enqueues them between the proof upload and the IPA check.
//
//   k_vp_gather_points  the 32-byte strings of every point of every proof, by the key's offset list, side by side for k_decompress
//   k_vp_scalars<C>     one lane per proof: the challenges (from the transcript batch's squeezes) and the evaluation scalars
//                       (straight from the uploaded proof bytes, checked against the modulus and taken to Montgomery form) go
//                       into the slot file, the tape runs, the left side's scalars leave in canonical form and (c, u_j) in
//                       Montgomery form, with one reject word per proof.  The slot file is in HBM as [slot][limb][proof]: the
//                       lanes of a wave touch neighbouring words.  The tape index, the offsets and every branch are the same for
//                       all lanes (the tape and the tables are read through uniform addresses); the only data-dependent branch is
//                       the tail guard.  No LDS.  A launch for 64 proofs is ONE wave: its time is the tape's dependent chain.
//   k_vp_points         the left side's points, gathered by the key's table from the decompressed proof points, the key's
//                       commitments, the instance commitments and G_0 U W
//   k_vp_reject         one byte per proof: the lane's flag, the transcript's status, any point that did not decode, a wrong length
// Rejected lanes run to the end like the others.
#include "ctx.hpp"
#include "curve.cuh"
#include "host_field.hpp"
#include "normalize.hpp"

namespace bzh {
namespace {
#include "verify_program.hpp"

__global__ void __launch_bounds__(256) k_vp_gather_points(const uint32_t* __restrict__ proofs, size_t pstride_w, const uint32_t* __restrict__ offs,
                                                          size_t np, size_t total, uint32_t* __restrict__ out) {
    const size_t g = blockIdx.x * (size_t)256 + threadIdx.x;   // (proof, point, word)
    if (g >= total) return;
    const size_t w = g & 7, i = (g >> 3) % np, b = (g >> 3) / np;
    out[g] = proofs[b * pstride_w + (offs[i] >> 2) + w];
}

template <class C>
__global__ void __launch_bounds__(256) k_vp_scalars(const VerifyPassArgs a) {
    const size_t b = blockIdx.x * (size_t)256 + threadIdx.x;
    if (b >= a.batch) return;
    vp_lane<typename CurveInfo<C>::SF>(a, b);
}

__global__ void __launch_bounds__(256) k_vp_points(const VerifyPassArgs a) {
    const size_t g = blockIdx.x * (size_t)256 + threadIdx.x;   // (proof, term)
    if (g >= a.batch * a.nl_cap) return;
    const size_t b = g / a.nl_cap, t = g % a.nl_cap;
    const uint32_t src = a.d_pt_src[t], kind = src >> 28, idx = src & 0x0fffffffu;
    const uint4* p = nullptr;
    switch (kind) {
        case VP_PT_PROOF: p = (const uint4*)(a.d_proof_xy + (b * a.np + idx) * 16); break;
        case VP_PT_FIXED: p = (const uint4*)(a.d_key_xy + (size_t)idx * 16); break;
        case VP_PT_SIGMA: p = (const uint4*)(a.d_key_xy + ((size_t)a.nfixed + idx) * 16); break;
        case VP_PT_INST: p = (const uint4*)(a.d_inst_xy + (b * a.ni + idx) * 16); break;
        case VP_PT_SRS: p = (const uint4*)(a.d_srs_xy + (size_t)idx * 16); break;
        default: break;
    }
    uint4* o = (uint4*)(a.d_lc_pts + g * 16);
    const uint4 z = make_uint4(0, 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 4; i++) o[i] = p ? p[i] : z;
}

__global__ void __launch_bounds__(256) k_vp_reject(const VerifyPassArgs a) {
    const size_t b = blockIdx.x * (size_t)256 + threadIdx.x;
    if (b >= a.batch) return;
    uint32_t r = a.d_flags[b] | a.d_pre_reject[b] | (a.d_tb_status[b] != BZH_POINT_OK ? 1u : 0u);
    for (uint32_t i = 0; i < a.np; i++) r |= a.d_point_status[b * a.np + i] != BZH_POINT_OK ? 1u : 0u;
    a.d_reject[b] = r ? 1 : 0;
}

}  // namespace

int vp_gather_points(bzh_ctx* ctx, const VerifyPassArgs& a, uint32_t* d_out32) {
    const size_t total = a.batch * a.np * 8;
    if (!total) return BZH_OK;
    hipLaunchKernelGGL(k_vp_gather_points, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, (const uint32_t*)a.d_proofs,
                       a.pstride / 4, a.d_vp_offsets, (size_t)a.np, total, d_out32);
    BZH_HIP_TRY(ctx, hipGetLastError());
    return BZH_OK;
}

int vp_scalars_run(bzh_ctx* ctx, int curve, const VerifyPassArgs& a) {
    return with_pasta_curve(curve, [&](auto c) -> int {
        {
            ScopedTimer tm(ctx, BZH_T_POLY);
            hipLaunchKernelGGL((k_vp_scalars<decltype(c)>), dim3((unsigned)((a.batch + 255) / 256)), dim3(256), 0, ctx->stream, a);
        }
        BZH_HIP_TRY(ctx, hipGetLastError());
        return BZH_OK;
    });
}

int vp_assemble_run(bzh_ctx* ctx, const VerifyPassArgs& a) {
    const size_t terms = a.batch * a.nl_cap;
    hipLaunchKernelGGL(k_vp_points, dim3((unsigned)((terms + 255) / 256)), dim3(256), 0, ctx->stream, a);
    BZH_HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_vp_reject, dim3((unsigned)((a.batch + 255) / 256)), dim3(256), 0, ctx->stream, a);
    BZH_HIP_TRY(ctx, hipGetLastError());
    return BZH_OK;
}

}  // namespace bzh
