// Params files in halo2_proofs 0.2.0's byte format (Params::write / Params::read; layout: csrc/params_file.hpp): the two
// host-only entry points, and the one kernel bzh_params_read (csrc/params.hip) adds to the library's existing ones.
//
//   k_pf_verdict   one lane per string of the file (2 n + 2 of them), 256-thread blocks.  A lane decides two things about its
//                  point: did it decode (the status byte decompress_run left), and -- when Params::new's generators are checked --
//                  is it, limb for limb, the point Params::new has in that place (g against h2c_generators_run's output where it
//                  lies, w and u against the two points the host hashed; g_lagrange is not looked at here).  Each wave folds
//                  its 64 answers with a ballot: a count, and the lowest offending lane (the lanes of a wave are consecutive, so
//                  that is the ballot's lowest bit).  The four waves of a workgroup meet in 64 bytes of LDS and thread 0 sends ONE
//                  atomicAdd and ONE atomicMax (on the complement of the lane: the words start at zero) per kind, and only for a
//                  kind that has an offender -- a good file makes no atomic but the ticket.  Thread 0 then waits for its atomics
//                  (release fence, s_waitcnt vmcnt(0)) and draws a ticket with a returning atomicAdd; the workgroup that draws
//                  the last one reads the four words back with returning atomics -- every access to a shared word is a
//                  device-scope atomic, nothing is polled, no workgroup waits for another --, compares the two Jacobian sums of
//                  the Lagrange check by cross-multiplication (X1 Z2^2 = X2 Z1^2 and Y1 Z2^3 = Y2 Z1^3; both Z zero: equal, one:
//                  not) and writes the 16-byte verdict record with plain vector stores.
// A launch is ceil((2 n + 2) / 256) workgroups; a lane reads 1 byte, or 1 + 128 with the generator check.  No loop bound depends
// on data.  Registers, scratch and occupancy of the gfx950 build: DESIGN.md section 7.
#include <cstring>

#include "ctx.hpp"
#include "curve.cuh"
#include "host_field.hpp"
#include "params_file.hpp"

namespace bzh {
namespace {

constexpr unsigned kPfLanes = 256, kPfWaves = kPfLanes / 64;
// d_acc: how many strings did not decode, ~(the lowest such lane), the same two for points that are not Params::new's, the ticket
enum { ACC_DEC_N = 0, ACC_DEC_FIRST = 1, ACC_GEN_N = 2, ACC_GEN_FIRST = 3, ACC_TICKET = 4 };

__device__ __forceinline__ bool pf_same_point(const uint32_t* a, const uint32_t* b) {
    uint32_t diff = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const uint4 u = reinterpret_cast<const uint4*>(a)[q], v = reinterpret_cast<const uint4*>(b)[q];
        diff |= (u.x ^ v.x) | (u.y ^ v.y) | (u.z ^ v.z) | (u.w ^ v.w);
    }
    return diff == 0;
}

__device__ bool pf_sums_equal(const uint32_t* sums) {
    using PB = VestaCurve::Base;
    const Fe<PB> X1 = fe_load<PB>(sums), Y1 = fe_load<PB>(sums + 8), Z1 = fe_load<PB>(sums + 16);
    const Fe<PB> X2 = fe_load<PB>(sums + 24), Y2 = fe_load<PB>(sums + 32), Z2 = fe_load<PB>(sums + 40);
    const bool id1 = fe_is_zero(Z1), id2 = fe_is_zero(Z2);
    const Fe<PB> z1s = fe_sqr(Z1), z2s = fe_sqr(Z2);
    const bool ex = fe_eq(fe_mul(X1, z2s), fe_mul(X2, z1s));
    const bool ey = fe_eq(fe_mul(Y1, fe_mul(z2s, Z2)), fe_mul(Y2, fe_mul(z1s, Z1)));
    return (id1 && id2) || (!id1 && !id2 && ex && ey);
}

__global__ void __launch_bounds__(kPfLanes) k_pf_verdict(const PfVerdictArgs a) {
    __shared__ uint32_t s_count[2][kPfWaves], s_first[2][kPfWaves];
    const size_t n = a.n, lanes = pf_points(n);
    const size_t i = blockIdx.x * (size_t)kPfLanes + threadIdx.x;
    const unsigned wave = threadIdx.x >> 6;
    bool bad[2] = {false, false};
    if (i < lanes) {
        bad[0] = a.d_status[i] != BZH_POINT_OK;
        if (a.d_gen) {
            uint32_t section, index;
            pf_lane_section(i, n, &section, &index);
            if (section == PF_G) bad[1] = a.d_gen_status[index] != BZH_POINT_OK || !pf_same_point(a.d_points + i * 16, a.d_gen + (size_t)index * 16);
            else if (section != PF_G_LAGRANGE) bad[1] = !pf_same_point(a.d_points + i * 16, a.d_wu + (section == PF_W ? 0 : 16));
        }
    }
#pragma unroll
    for (int kind = 0; kind < 2; kind++) {
        const unsigned long long m = __ballot(bad[kind]);
        if ((threadIdx.x & 63) == 0) {
            s_count[kind][wave] = (uint32_t)__popcll(m);
            // the wave's first lane is i here; an empty ballot leaves the complement's neutral element
            s_first[kind][wave] = m ? (uint32_t)i + (uint32_t)(__ffsll((long long)m) - 1) : 0xffffffffu;
        }
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
#pragma unroll
    for (int kind = 0; kind < 2; kind++) {
        uint32_t count = 0, first = 0xffffffffu;
        for (unsigned w = 0; w < kPfWaves; w++) {
            count += s_count[kind][w];
            first = s_first[kind][w] < first ? s_first[kind][w] : first;
        }
        if (count) {
            atomicAdd(a.d_acc + (kind ? ACC_GEN_N : ACC_DEC_N), count);
            atomicMax(a.d_acc + (kind ? ACC_GEN_FIRST : ACC_DEC_FIRST), ~first);
        }
    }
    // the atomics above have been performed before the ticket is drawn
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (atomicAdd(a.d_acc + ACC_TICKET, 1u) != gridDim.x - 1) return;
    // the last workgroup: every other one has added its words
    const uint32_t dec_n = atomicAdd(a.d_acc + ACC_DEC_N, 0u), dec_first = ~atomicAdd(a.d_acc + ACC_DEC_FIRST, 0u);
    const uint32_t gen_n = atomicAdd(a.d_acc + ACC_GEN_N, 0u), gen_first = ~atomicAdd(a.d_acc + ACC_GEN_FIRST, 0u);
    uint32_t bits = 0, section = 0, first_bad = 0, n_bad = 0;
    if (dec_n) {   // nothing else can be said about a file with a string that is no point
        bits = BZH_PARAMS_BAD_DECODE;
        pf_lane_section(dec_first, n, &section, &first_bad);
        n_bad = dec_n;
    } else {
        if (a.d_sums && !pf_sums_equal(a.d_sums)) {   // the sums say that g_lagrange is wrong, not where
            bits |= BZH_PARAMS_BAD_LAGRANGE;
            section = PF_G_LAGRANGE;
        }
        if (gen_n) {
            bits |= BZH_PARAMS_BAD_GENERATORS;
            pf_lane_section(gen_first, n, &section, &first_bad);
            n_bad = gen_n;
        }
    }
    *reinterpret_cast<uint4*>(a.d_verdict) = make_uint4(bits, section, first_bad, n_bad);
}

}  // namespace

int params_file_verdict_run(bzh_ctx* ctx, const PfVerdictArgs& a) {
    if (!a.d_status || !a.d_points || !a.d_acc || !a.d_verdict || !a.n || a.n > ((size_t)1 << kPfMaxK)) return BZH_E_ARG;
    if ((a.d_gen != nullptr) != (a.d_gen_status != nullptr) || (a.d_gen != nullptr) != (a.d_wu != nullptr)) return BZH_E_ARG;
    BZH_HIP_TRY(ctx, hipMemsetAsync(a.d_acc, 0, 32, ctx->stream));
    const unsigned blocks = (unsigned)((pf_points(a.n) + kPfLanes - 1) / kPfLanes);
    hipLaunchKernelGGL(k_pf_verdict, dim3(blocks), dim3(kPfLanes), 0, ctx->stream, a);
    BZH_HIP_TRY(ctx, hipGetLastError());
    return BZH_OK;
}

}  // namespace bzh

using namespace bzh;

extern "C" int bzh_params_file_info(const uint8_t* bytes, size_t len, unsigned* k, size_t* n_points) {
    if (!bytes || len < kPfHeaderBytes) return BZH_E_ARG;
    const uint32_t kk = (uint32_t)bytes[0] | ((uint32_t)bytes[1] << 8) | ((uint32_t)bytes[2] << 16) | ((uint32_t)bytes[3] << 24);
    if (kk > kPfMaxK) return BZH_E_ARG;
    const size_t n = (size_t)1 << kk;
    if (len != pf_file_bytes(n)) return BZH_E_ARG;
    if (k) *k = kk;
    if (n_points) *n_points = n;
    return BZH_OK;
}

extern "C" int bzh_params_encode(unsigned k, const uint64_t* g_xy, const uint64_t* g_lagrange_xy, const uint64_t* w_xy, const uint64_t* u_xy,
                                 uint8_t* out, size_t cap, size_t* len) {
    if (k > kPfMaxK || !len) return BZH_E_ARG;
    const size_t n = (size_t)1 << k, need = pf_file_bytes(n);
    *len = need;
    if (!out) return BZH_OK;   // the size query
    if (cap < need || !g_xy || !g_lagrange_xy || !w_xy || !u_xy) return BZH_E_ARG;
    for (int b = 0; b < 4; b++) out[b] = (uint8_t)(k >> (8 * b));
    const uint64_t* src[kPfSections] = {g_xy, g_lagrange_xy, w_xy, u_xy};   // by section code
    for (int s = 0; s < kPfSections; s++)
        for (size_t i = 0; i < pf_section_len(s, n); i++) h_compress<VestaCurve>(src[s] + 8 * i, BZH_FORM_CANONICAL, out + pf_offset(s, i, n));
    return BZH_OK;
}
