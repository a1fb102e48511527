// The four kernels of the witness commitments on device-resident transcripts (bzh_commitments_batch_device) on gfx950.
//
// The call itself -- phases 1 to 3 of halo2_proofs 0.2.0 `plonk::create_proof` (UPSTREAM, un-vendored): the instance and advice
// commitments, theta, the lookups' compressed and permuted columns and their commitments, beta and gamma -- reads the proving key
// and therefore lives with it (csrc/commitments_device.hpp, part of csrc/prove.hip).  bzh_prove_batch's commit_instances(),
// commit_advice() and lookups() phases (csrc/prover.hpp) do the same around host transcripts: the instance goes up converted on
// the host, the columns are assembled with a device copy, a fill and strided copies, theta comes down and goes back up inside the
// compress programs' constant tables, and every blind is drawn on the host and uploaded with its commitment.  Here:
//   k_cm_place          one thread per (row, column, proof) of the advice and instance columns: a row below `usable` of an advice
//                       column is the caller's value, taken to Montgomery form in the same pass when it is canonical, a row from
//                       `usable` on is that column's drawn blinding value; an instance column is the caller's instance_rows values
//                       and zeros.  Each thread moves one element as two dwordx4, consecutive lanes on consecutive rows; the
//                       kernel is a streaming copy of 64 bytes per element.  Lane 0 of a column's first workgroup copies the
//                       column's blind.
//   k_cm_consts         one lane per (proof, constant) over the constants of every compress program of the call, body in
//                       commitments_scalars.hpp: the constant tables straight from theta in HBM.
//   k_cm_lookup_finish  one workgroup per (lookup, proof): the 2 (bf + 1) drawn rows of the permuted pair, its two blinds, and for
//                       lookup 0 the proof's status from lookup_permute's words (cm_status_lane), also ORed into the transcript's
//                       sticky byte.  Plain byte stores: they take any alignment.
//   k_cm_scalar_rows    one thread per (entry, column): the scalar row (evaluations | 0 | blind [| 0]) of a commitment in the
//                       Lagrange basis, the blind from device memory, for a table of n + 2 or n + 3 points.
#include "ctx.hpp"
#include "curve.cuh"
#include "host_field.hpp"
#include "commitments_scalars.hpp"

static_assert(sizeof(bzh::CmConst) == 56, "the descriptor list is uploaded as it lies");

namespace bzh {

static constexpr unsigned kCmThreads = 256;
static constexpr unsigned kCmLanes = 64;

template <class P>
__global__ void __launch_bounds__(kCmThreads) k_cm_place(const uint32_t* __restrict__ advice, const uint32_t* __restrict__ instances,
                                                         size_t inst_rows, const uint32_t* __restrict__ drawn, size_t nd, size_t n,
                                                         size_t usable, size_t na, size_t ni, int canonical,
                                                         uint32_t* __restrict__ out_adv, uint32_t* __restrict__ out_inst,
                                                         uint32_t* __restrict__ out_blinds) {
    const size_t c = blockIdx.y, b = blockIdx.z, bf1 = n - usable;
    const size_t row = blockIdx.x * (size_t)kCmThreads + threadIdx.x;
    if (c < na) {
        const uint32_t* __restrict__ dr = drawn + b * nd * 8;   // this proof's draws: na x bf1 blinding rows, then the na blinds
        if (row < n) {
            Fe<P> v;
            if (row < usable) {
                v = fe_load<P>(advice + ((b * na + c) * n + row) * 8);
                if (canonical) v = fe_to_mont(v);   // (uniform over the launch)
            } else {
                v = fe_load<P>(dr + (c * bf1 + (row - usable)) * 8);
            }
            fe_store(out_adv + ((b * na + c) * n + row) * 8, v);
        }
        if (blockIdx.x == 0 && threadIdx.x == 0) fe_store(out_blinds + (b * na + c) * 8, fe_load<P>(dr + (na * bf1 + c) * 8));
    } else if (row < n) {
        const size_t i = c - na;
        Fe<P> v = fe_zero<P>();
        if (row < inst_rows) {
            v = fe_load<P>(instances + ((b * ni + i) * inst_rows + row) * 8);
            if (canonical) v = fe_to_mont(v);
        }
        fe_store(out_inst + ((b * ni + i) * n + row) * 8, v);
    }
}

template <class P>
__global__ void __launch_bounds__(kCmLanes) k_cm_consts(const CmConst* __restrict__ descs, size_t ndescs, size_t batch,
                                                        const uint32_t* __restrict__ theta, int canonical) {
    const size_t g = blockIdx.x * (size_t)kCmLanes + threadIdx.x;
    if (g >= ndescs * batch) return;
    cm_const_lane<P>(g, descs, ndescs, theta, canonical != 0);
}

// drawn: proof b's draws of lookup l at drawn[b * nd + first + l * (2 bf1 + 2)]: bf1 rows of the input, bf1 of the table, two blinds
template <class P>
__global__ void __launch_bounds__(kCmLanes) k_cm_lookup_finish(const uint32_t* __restrict__ drawn, size_t nd, size_t first, size_t n,
                                                               size_t usable, size_t nl, const int32_t* __restrict__ words,
                                                               uint32_t* __restrict__ permuted, uint32_t* __restrict__ blinds,
                                                               uint8_t* __restrict__ status, uint8_t* __restrict__ sticky) {
    const size_t l = blockIdx.x, b = blockIdx.y, bf1 = n - usable, pair = b * nl + l;
    const uint32_t* __restrict__ dr = drawn + (b * nd + first + l * (2 * bf1 + 2)) * 8;
    for (size_t i = threadIdx.x; i < 2 * bf1 + 2; i += kCmLanes) {
        const Fe<P> v = fe_load<P>(dr + i * 8);
        if (i < 2 * bf1) {
            const size_t side = i / bf1, r = i - side * bf1;
            fe_store(permuted + ((pair * 2 + side) * n + usable + r) * 8, v);
        } else {
            fe_store(blinds + (pair * 2 + (i - 2 * bf1)) * 8, v);
        }
    }
    if (l == 0 && threadIdx.x == 0) {
        const uint8_t bit = cm_status_lane(words, nl, b);
        if (status) status[b] = bit;
        if (bit) sticky[b] = (uint8_t)(sticky[b] | 1u);
    }
}

template <class P>
__global__ void __launch_bounds__(kCmThreads) k_cm_scalar_rows(const uint32_t* __restrict__ evals, const uint32_t* __restrict__ blinds,
                                                               size_t n, size_t cols, uint32_t* __restrict__ sc) {
    const size_t i = blockIdx.x * (size_t)kCmThreads + threadIdx.x, v = blockIdx.y;
    if (i >= cols) return;
    Fe<P> o = fe_zero<P>();
    if (i < n) o = fe_load<P>(evals + (v * n + i) * 8);
    else if (i == n + 1) o = fe_load<P>(blinds + v * 8);
    fe_store(sc + (v * cols + i) * 8, o);
}

int commitments_place(bzh_ctx* ctx, int field, const uint32_t* d_advice, const uint32_t* d_instances, size_t inst_rows,
                      const uint32_t* d_drawn, size_t nd, size_t n, size_t usable, size_t na, size_t ni, size_t batch, int form,
                      uint32_t* d_out_adv, uint32_t* d_out_inst, uint32_t* d_out_blinds) {
    if (!(na + ni) || !batch || !n) return BZH_OK;
    if (na + ni > 65535 || batch > 65535 || usable >= n || inst_rows > n || nd < na * (n - usable + 1)) return BZH_E_ARG;
    const int canonical = form == BZH_FORM_CANONICAL ? 1 : 0;
    BZH_TRY(with_pasta_field(field, [&](auto p) {
        using P = decltype(p);
        hipLaunchKernelGGL((k_cm_place<P>), dim3((unsigned)((n + kCmThreads - 1) / kCmThreads), (unsigned)(na + ni), (unsigned)batch),
                           dim3(kCmThreads), 0, ctx->stream, d_advice, d_instances, inst_rows, d_drawn, nd, n, usable, na, ni, canonical,
                           d_out_adv, d_out_inst, d_out_blinds);
        return (int)BZH_OK;
    }));
    BZH_HIP_TRY(ctx, hipGetLastError());
    return BZH_OK;
}

int commitments_consts(bzh_ctx* ctx, int field, const void* d_descs, size_t ndescs, size_t batch, const uint32_t* d_theta, int form) {
    if (!ndescs || !batch) return BZH_OK;
    const int canonical = form == BZH_FORM_CANONICAL ? 1 : 0;
    BZH_TRY(with_pasta_field(field, [&](auto p) {
        using P = decltype(p);
        hipLaunchKernelGGL((k_cm_consts<P>), dim3((unsigned)((ndescs * batch + kCmLanes - 1) / kCmLanes)), dim3(kCmLanes), 0, ctx->stream,
                           (const CmConst*)d_descs, ndescs, batch, d_theta, canonical);
        return (int)BZH_OK;
    }));
    BZH_HIP_TRY(ctx, hipGetLastError());
    return BZH_OK;
}

int commitments_lookup_finish(bzh_ctx* ctx, int field, const uint32_t* d_drawn, size_t nd, size_t first, size_t n, size_t usable, size_t nl,
                              size_t batch, const int32_t* d_words, uint32_t* d_permuted, uint32_t* d_blinds, uint8_t* d_status,
                              uint8_t* d_sticky) {
    if (!nl || !batch) return BZH_OK;
    if (nl > 65535 || batch > 65535 || usable >= n || nd < first + nl * (2 * (n - usable) + 2)) return BZH_E_ARG;
    BZH_TRY(with_pasta_field(field, [&](auto p) {
        using P = decltype(p);
        hipLaunchKernelGGL((k_cm_lookup_finish<P>), dim3((unsigned)nl, (unsigned)batch), dim3(kCmLanes), 0, ctx->stream, d_drawn, nd, first, n,
                           usable, nl, d_words, d_permuted, d_blinds, d_status, d_sticky);
        return (int)BZH_OK;
    }));
    BZH_HIP_TRY(ctx, hipGetLastError());
    return BZH_OK;
}

int commitments_scalar_rows(bzh_ctx* ctx, int field, const uint32_t* d_evals, const uint32_t* d_blinds, size_t n, size_t cols, size_t count,
                            uint32_t* d_scalars) {
    if (!count) return BZH_OK;
    if (count > 65535 || (cols != n + 2 && cols != n + 3)) return BZH_E_ARG;
    BZH_TRY(with_pasta_field(field, [&](auto p) {
        using P = decltype(p);
        hipLaunchKernelGGL((k_cm_scalar_rows<P>), dim3((unsigned)((cols + kCmThreads - 1) / kCmThreads), (unsigned)count), dim3(kCmThreads), 0,
                           ctx->stream, d_evals, d_blinds, n, cols, d_scalars);
        return (int)BZH_OK;
    }));
    BZH_HIP_TRY(ctx, hipGetLastError());
    return BZH_OK;
}

}  // namespace bzh
