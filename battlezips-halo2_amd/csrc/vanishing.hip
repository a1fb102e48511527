// The two kernels of the vanishing argument on device-resident transcripts (bzh_vanishing_batch_device) on gfx950.
//
// The call itself -- phase 5 of halo2_proofs 0.2.0 `plonk::create_proof` (UPSTREAM, un-vendored) between the grand products and
// the evaluations: commit the random polynomial, squeeze y, evaluate the quotient on the extended coset, transform it back,
// check its degree, commit its pieces -- reads the proving key and therefore lives with it (csrc/vanishing_device.hpp, part of
// csrc/prove.hip).  bzh_prove_batch's vanishing() phase (csrc/prover.hpp) does the same around host transcripts: y comes down,
// the quotient program's constant table (theta, beta, gamma, y, y^m, beta * delta^j) is computed on the host and uploaded, and
// the degree check is one word for the whole batch, read back.  Here:
//   k_vn_consts   one lane per (proof, constant), body in vanishing_scalars.hpp: the table straight from the challenges in HBM,
//                 in the format of the quotient flavour that will run.  The constant index is the fastest one, so a wave covers
//                 consecutive constants of one proof (of two, at a proof's end) and its stores are contiguous.  For a batch of
//                 64 this is a handful of waves whose time is that of fifteen dependent 256-bit products (seven square-and-
//                 multiply steps -- 7 squarings, 7 selected multiplications -- and the multiplication by the value); it has not
//                 been measured.
//   k_vn_degree   one workgroup per proof ORs the words of h[b][npieces * n .. en); one lane sets bit 0 of that proof's status
//                 byte and of its transcript's sticky byte.  Plain byte stores: they take any alignment.
#include "ctx.hpp"
#include "curve.cuh"
#include "host_field.hpp"
#include "vanishing_scalars.hpp"

static_assert(sizeof(bzh::VnConst) == sizeof(bzh_vanishing_const) && sizeof(bzh_vanishing_const) == 40, "lane bodies and header disagree");

namespace bzh {

static constexpr unsigned kVnLanes = 64;
static constexpr unsigned kVnDegreeThreads = 256;

template <class P>
__global__ void __launch_bounds__(kVnLanes) k_vn_consts(const VnConst* __restrict__ descs, size_t nconsts, size_t batch,
                                                        const uint32_t* __restrict__ theta, const uint32_t* __restrict__ beta,
                                                        const uint32_t* __restrict__ gamma, const uint32_t* __restrict__ y, int canonical,
                                                        int planes29, uint32_t* __restrict__ table) {
    const size_t g = blockIdx.x * (size_t)kVnLanes + threadIdx.x;
    if (g >= nconsts * batch) return;
    vn_const_lane<P>(g, descs, nconsts, theta, beta, gamma, y, canonical != 0, planes29 != 0, table);
}

// h: batch rows of `pitch` elements; the tail of row b is its elements [first, pitch).  first < pitch.
__global__ void __launch_bounds__(kVnDegreeThreads) k_vn_degree(const uint32_t* __restrict__ h, size_t first, size_t pitch,
                                                                uint8_t* __restrict__ status, uint8_t* __restrict__ sticky) {
    const size_t b = blockIdx.x;
    const uint4* __restrict__ row = (const uint4*)(h + (b * pitch + first) * 8);
    const size_t n16 = (pitch - first) * 2;
    uint32_t acc = 0;
    for (size_t i = threadIdx.x; i < n16; i += kVnDegreeThreads) {
        const uint4 v = row[i];
        acc |= v.x | v.y | v.z | v.w;
    }
    const int any = __syncthreads_or(acc != 0);
    if (threadIdx.x == 0 && any) {
        if (status) status[b] = (uint8_t)(status[b] | 1u);
        sticky[b] = (uint8_t)(sticky[b] | 1u);
    }
}

int vanishing_consts(bzh_ctx* ctx, int field, const void* d_descs, size_t nconsts, size_t batch, const uint32_t* d_theta,
                     const uint32_t* d_beta, const uint32_t* d_gamma, const uint32_t* d_y, int form, bool planes29, uint32_t* d_table) {
    if (!nconsts || !batch) return BZH_OK;
    const int canonical = form == BZH_FORM_CANONICAL ? 1 : 0;
    BZH_TRY(with_pasta_field(field, [&](auto p) {
        using P = decltype(p);
        if (planes29 && !fe29_supported<P>()) return (int)BZH_E_ARG;
        hipLaunchKernelGGL((k_vn_consts<P>), dim3((unsigned)((nconsts * batch + kVnLanes - 1) / kVnLanes)), dim3(kVnLanes), 0, ctx->stream,
                           (const VnConst*)d_descs, nconsts, batch, d_theta, d_beta, d_gamma, d_y, canonical, planes29 ? 1 : 0, d_table);
        return (int)BZH_OK;
    }));
    BZH_HIP_TRY(ctx, hipGetLastError());
    return BZH_OK;
}

int vanishing_degree(bzh_ctx* ctx, const uint32_t* d_h, size_t first, size_t pitch, size_t batch, uint8_t* d_status, uint8_t* d_sticky) {
    if (first >= pitch || !batch) return BZH_OK;
    hipLaunchKernelGGL(k_vn_degree, dim3((unsigned)batch), dim3(kVnDegreeThreads), 0, ctx->stream, d_h, first, pitch, d_status, d_sticky);
    BZH_HIP_TRY(ctx, hipGetLastError());
    return BZH_OK;
}

}  // namespace bzh
