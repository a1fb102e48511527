// The two kernels of the grand products on device-resident transcripts (bzh_grand_products_batch_device) on gfx950.
//
// The call itself -- phase 4 of halo2_proofs 0.2.0 `plonk::create_proof` (UPSTREAM, un-vendored): the permutation argument's and
// the lookups' running products between the squeeze of beta, gamma and the vanishing argument -- reads the proving key and
// therefore lives with it (csrc/products_device.hpp, part of csrc/prove.hip).  bzh_prove_batch's grand_products() phase
// (csrc/prover.hpp) builds every numerator and denominator through the VM v1 interpreter, whose constant table is filled on the
// host from beta and gamma, and finishes each product with a scale, a blind and a copy of its own.  Here:
//   k_gp_factors  one thread per (row, product, proof): the numerator and the denominator of that row's factor, from beta_b and
//                 gamma_b in HBM and the columns read in place through the call's column table (GpCol, products_scalars.hpp).
//                 A workgroup has one product and one proof, so the two challenges and the table entries are uniform over it:
//                 two lanes load and convert the challenges into LDS, the entries come through the scalar unit.  Per column and
//                 row a permutation set does four field products (beta * sigma, ident * beta, two accumulations; two for its
//                 first column) for 96 bytes read -- value, sigma, ident, each two dwordx4 per lane, consecutive lanes on
//                 consecutive rows -- and a lookup two products for 128 bytes; each thread stores 64 bytes.  Whether HBM or the
//                 multiplier bounds it has not been measured.
//   k_gp_finish   one thread per (row, product, proof), after the batch inversion, the product and the exclusive scan of
//                 polyops.hip: lane 0 of a workgroup forms the carry of its permutation set (gp_carry_lane), every thread writes
//                 raw * carry, or the drawn blinding value in the last bf rows, straight into z[b][product][row]; in the first
//                 workgroup of a (product, proof) lane 0 copies the blind, and for product 0 sets the proof's status
//                 (gp_status_lane) and ORs it into the transcript's sticky byte.  Plain byte stores: they take any alignment.
#include "ctx.hpp"
#include "curve.cuh"
#include "host_field.hpp"
#include "products_scalars.hpp"

static_assert(sizeof(bzh::GpCol) == 32 && sizeof(bzh::GpProd) == 8, "the column table is uploaded as it lies");

namespace bzh {

static constexpr unsigned kGpThreads = 256;

template <class P>
__global__ void __launch_bounds__(kGpThreads) k_gp_factors(const GpCol* __restrict__ cols, const GpProd* __restrict__ prods, size_t nsets,
                                                           size_t n, size_t batch, const uint32_t* __restrict__ beta,
                                                           const uint32_t* __restrict__ gamma, int canonical, uint32_t* __restrict__ num,
                                                           uint32_t* __restrict__ den) {
    __shared__ __attribute__((aligned(16))) uint32_t ch[2][8];
    const size_t p = blockIdx.y, b = blockIdx.z;
    if (threadIdx.x < 2) {
        Fe<P> c = fe_load<P>((threadIdx.x ? gamma : beta) + b * 8);
        if (canonical) c = fe_to_mont(c);   // (uniform over the launch)
        fe_store(ch[threadIdx.x], c);
    }
    __syncthreads();
    const size_t row = blockIdx.x * (size_t)kGpThreads + threadIdx.x;
    if (row >= n) return;
    const Fe<P> be = fe_load<P>(ch[0]), ga = fe_load<P>(ch[1]);
    const GpProd pr = prods[p];
    const GpCol* __restrict__ c = cols + pr.first;
    Fe<P> fn, fd;
    if (p < nsets) {
        auto factors = [&](uint32_t j, Fe<P>& u, Fe<P>& d) {
            const GpCol col = c[j];
            const Fe<P> gv = fe_add(ga, fe_load<P>(col.v + (b * col.stride + row) * 8));
            d = fe_add(fe_mul(be, fe_load<P>(col.sigma + row * 8)), gv);
            u = fe_add(fe_mul(fe_load<P>(col.ident + row * 8), be), gv);
        };
        factors(0, fn, fd);   // (a set has at least one column)
        for (uint32_t j = 1; j < pr.count; j++) {
            Fe<P> u, d;
            factors(j, u, d);
            fn = fe_mul(fn, u);
            fd = fe_mul(fd, d);
        }
    } else {
        auto at = [&](int j) { return fe_load<P>(c[j].v + (b * c[j].stride + row) * 8); };
        fn = fe_mul(fe_add(at(0), be), fe_add(at(1), ga));
        fd = fe_mul(fe_add(at(2), be), fe_add(at(3), ga));
    }
    const size_t o = ((p * batch + b) * n + row) * 8;
    fe_store(num + o, fn);
    fe_store(den + o, fd);
}

template <class P>
__global__ void __launch_bounds__(kGpThreads) k_gp_finish(const uint32_t* __restrict__ raw, const uint32_t* __restrict__ drawn, size_t n,
                                                          size_t usable, size_t bf, size_t nsets, size_t nl, size_t batch,
                                                          uint32_t* __restrict__ z, uint32_t* __restrict__ blinds,
                                                          uint8_t* __restrict__ status, uint8_t* __restrict__ sticky) {
    __shared__ __attribute__((aligned(16))) uint32_t carry[8];
    const size_t p = blockIdx.y, b = blockIdx.z, nz = nsets + nl;
    if (threadIdx.x == 0) fe_store(carry, gp_carry_lane<P>(raw, batch, n, usable, p, b, nsets));
    __syncthreads();
    const uint32_t* __restrict__ dr = drawn + (b * nz + p) * (bf + 1) * 8;   // this product's draws: bf rows, then the blind
    const size_t row = blockIdx.x * (size_t)kGpThreads + threadIdx.x;
    if (row < n) {
        Fe<P> v;
        if (row < n - bf) v = fe_mul(fe_load<P>(raw + ((p * batch + b) * n + row) * 8), fe_load<P>(carry));
        else v = fe_load<P>(dr + (row - (n - bf)) * 8);
        fe_store(z + ((b * nz + p) * n + row) * 8, v);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        fe_store(blinds + (b * nz + p) * 8, fe_load<P>(dr + bf * 8));
        if (p == 0) {
            const uint8_t bit = gp_status_lane<P>(raw, batch, n, usable, b, nsets, nl);
            if (status) status[b] = bit;
            if (bit) sticky[b] = (uint8_t)(sticky[b] | 1u);
        }
    }
}

int products_factors(bzh_ctx* ctx, int field, const void* d_cols, const void* d_prods, size_t nsets, size_t nl, size_t n, size_t batch,
                     const uint32_t* d_beta, const uint32_t* d_gamma, int form, uint32_t* d_num, uint32_t* d_den) {
    const size_t nz = nsets + nl;
    if (!nz || !batch || !n) return BZH_OK;
    if (nz > 65535 || batch > 65535) return BZH_E_ARG;
    const int canonical = form == BZH_FORM_CANONICAL ? 1 : 0;
    BZH_TRY(with_pasta_field(field, [&](auto p) {
        using P = decltype(p);
        hipLaunchKernelGGL((k_gp_factors<P>), dim3((unsigned)((n + kGpThreads - 1) / kGpThreads), (unsigned)nz, (unsigned)batch), dim3(kGpThreads), 0,
                           ctx->stream, (const GpCol*)d_cols, (const GpProd*)d_prods, nsets, n, batch, d_beta, d_gamma, canonical, d_num, d_den);
        return (int)BZH_OK;
    }));
    BZH_HIP_TRY(ctx, hipGetLastError());
    return BZH_OK;
}

int products_finish(bzh_ctx* ctx, int field, const uint32_t* d_raw, const uint32_t* d_drawn, size_t n, size_t usable, size_t bf, size_t nsets,
                    size_t nl, size_t batch, uint32_t* d_z, uint32_t* d_blinds, uint8_t* d_status, uint8_t* d_sticky) {
    const size_t nz = nsets + nl;
    if (!nz || !batch || !n) return BZH_OK;
    if (nz > 65535 || batch > 65535 || usable >= n || bf >= n) return BZH_E_ARG;
    BZH_TRY(with_pasta_field(field, [&](auto p) {
        using P = decltype(p);
        hipLaunchKernelGGL((k_gp_finish<P>), dim3((unsigned)((n + kGpThreads - 1) / kGpThreads), (unsigned)nz, (unsigned)batch), dim3(kGpThreads), 0,
                           ctx->stream, d_raw, d_drawn, n, usable, bf, nsets, nl, batch, d_z, d_blinds, d_status, d_sticky);
        return (int)BZH_OK;
    }));
    BZH_HIP_TRY(ctx, hipGetLastError());
    return BZH_OK;
}

}  // namespace bzh
