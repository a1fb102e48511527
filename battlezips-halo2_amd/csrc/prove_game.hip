// The two lane kernels of the game-input prover (bzh_prove_shots_device / bzh_prove_boards_device) on gfx950.
//
// The call itself -- the three synthesis kernels of csrc/synthesize_device.hip in front of the device-resident batch prover's chain
// -- reads the proving key and lives with it (csrc/prove_game.hpp and csrc/prove_device.hpp, parts of csrc/prove.hip).  What joins
// the two halves on the device is small, one lane per proof in 64-thread blocks, bodies in prove_game_scalars.hpp:
//   k_pg_instances   the commitment k_syn_ecc_tail left (and Shot's shot and hit words) into the Montgomery instance rows the
//                    commitments leaf reads and the canonical rows the call reads back: two or four elements a lane, dwordx4 stores
//   k_pg_status      the synthesis status word into bits 4 .. 6 of the slot k_pd_status filled
// No LDS, no atomics, plain vector stores: a lane owns its rows and its slot.
#include "ctx.hpp"
#include "prove_game_scalars.hpp"

namespace bzh {

static constexpr unsigned kPgLanes = 64;

__global__ void __launch_bounds__(kPgLanes) k_pg_instances(bool shot, const uint32_t* __restrict__ cm, const uint64_t* __restrict__ in, size_t in_words,
                                                           size_t batch, uint32_t* __restrict__ mont, uint32_t* __restrict__ canon) {
    const size_t b = blockIdx.x * (size_t)kPgLanes + threadIdx.x;
    if (b >= batch) return;
    pg_instance_lane(b, shot, cm, in, in_words, mont, canon);
}

__global__ void __launch_bounds__(kPgLanes) k_pg_status(const uint32_t* __restrict__ syn_status, size_t batch, uint32_t* __restrict__ slot) {
    const size_t b = blockIdx.x * (size_t)kPgLanes + threadIdx.x;
    if (b >= batch) return;
    pg_status_lane(b, syn_status, slot);
}

int prove_game_instances(bzh_ctx* ctx, bool shot, const uint32_t* d_cm, const uint64_t* d_in, size_t in_words, size_t batch, uint32_t* d_mont,
                         uint32_t* d_canon) {
    if (!batch) return BZH_OK;
    if (shot && in_words < 16) return BZH_E_ARG;   // the lane reads words 8 .. 9 and 12 .. 13 of its proof
    hipLaunchKernelGGL(k_pg_instances, dim3((unsigned)((batch + kPgLanes - 1) / kPgLanes)), dim3(kPgLanes), 0, ctx->stream, shot, d_cm, d_in,
                       in_words, batch, d_mont, d_canon);
    BZH_HIP_TRY(ctx, hipGetLastError());
    return BZH_OK;
}

int prove_game_status(bzh_ctx* ctx, const uint32_t* d_syn_status, size_t batch, uint32_t* d_slot) {
    if (!batch) return BZH_OK;
    hipLaunchKernelGGL(k_pg_status, dim3((unsigned)((batch + kPgLanes - 1) / kPgLanes)), dim3(kPgLanes), 0, ctx->stream, d_syn_status, batch,
                       d_slot);
    BZH_HIP_TRY(ctx, hipGetLastError());
    return BZH_OK;
}

}  // namespace bzh
