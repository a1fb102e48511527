// The two lane kernels of the device-resident batch prover (bzh_prove_batch_device) on gfx950.
//
// The call itself -- halo2_proofs 0.2.0 `plonk::create_proof` (UPSTREAM, un-vendored) as the chain of the five leaves on ONE
// device transcript batch -- reads the proving key and therefore lives with it (csrc/prove_device.hpp, part of csrc/prove.hip).
// The leaves hand their polynomials to the evaluations and the multiopen where they lie, through a source table; what is left to
// arrange between them is small:
//   k_pd_blinds   one lane per (proof, opened polynomial), body in prove_device_scalars.hpp: the [batch][nown] blind row the
//                 multiopen reads, gathered from the leaves' blind arrays through a table of (pointer, per-proof stride, first,
//                 count); the polynomial index is fastest, so a wave stores 64 consecutive elements (two dwordx4 a lane).  A
//                 streaming copy of 64 bytes per element.
//   k_pd_status   one lane per proof: the four leaves' status bytes folded into bits 0 .. 3, and the proof's length, into the
//                 two-word slot the call reads back.  Plain vector stores, no atomics: a lane owns its slot.
#include "ctx.hpp"
#include "curve.cuh"
#include "host_field.hpp"
#include "prove_device_scalars.hpp"

static_assert(sizeof(bzh::PdBlindSrc) == 24, "the source table is uploaded as it lies");

namespace bzh {

static constexpr unsigned kPdLanes = 64;

template <class P>
__global__ void __launch_bounds__(kPdLanes) k_pd_blinds(const PdBlindSrc* __restrict__ srcs, size_t nsrc, size_t nown, size_t batch,
                                                        uint32_t* __restrict__ out) {
    const size_t g = blockIdx.x * (size_t)kPdLanes + threadIdx.x;
    if (g >= nown * batch) return;
    pd_blind_lane<P>(g, srcs, nsrc, nown, out);
}

__global__ void __launch_bounds__(kPdLanes) k_pd_status(const uint8_t* __restrict__ leaf, size_t leaf_stride, size_t batch, uint32_t proof_len,
                                                        uint32_t* __restrict__ slot) {
    const size_t b = blockIdx.x * (size_t)kPdLanes + threadIdx.x;
    if (b >= batch) return;
    pd_status_lane(b, leaf, leaf_stride, proof_len, slot);
}

int prove_device_blinds(bzh_ctx* ctx, int field, const void* d_srcs, size_t nsrc, size_t nown, size_t batch, uint32_t* d_out) {
    if (!nown || !batch) return BZH_OK;
    const size_t lanes = nown * batch;
    if ((lanes + kPdLanes - 1) / kPdLanes > 0x7fffffffu) return BZH_E_ARG;
    BZH_TRY(with_pasta_field(field, [&](auto p) {
        using P = decltype(p);
        hipLaunchKernelGGL((k_pd_blinds<P>), dim3((unsigned)((lanes + kPdLanes - 1) / kPdLanes)), dim3(kPdLanes), 0, ctx->stream,
                           (const PdBlindSrc*)d_srcs, nsrc, nown, batch, d_out);
        return (int)BZH_OK;
    }));
    BZH_HIP_TRY(ctx, hipGetLastError());
    return BZH_OK;
}

int prove_device_status(bzh_ctx* ctx, const uint8_t* d_leaf, size_t leaf_stride, size_t batch, uint32_t proof_len, uint32_t* d_slot) {
    if (!batch) return BZH_OK;
    if (leaf_stride < batch) return BZH_E_ARG;
    hipLaunchKernelGGL(k_pd_status, dim3((unsigned)((batch + kPdLanes - 1) / kPdLanes)), dim3(kPdLanes), 0, ctx->stream, d_leaf, leaf_stride,
                       batch, proof_len, d_slot);
    BZH_HIP_TRY(ctx, hipGetLastError());
    return BZH_OK;
}

}  // namespace bzh
