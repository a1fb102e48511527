// Inner-product-argument opening on gfx950.
//
// Replaces halo2_proofs 0.2.0 `poly::commitment::{create_proof, verify_proof}` (UPSTREAM,
// un-vendored: Cargo.lock:382-385), step 9 of plonk::create_proof as called from
// benches/shot.rs:68, benches/board.rs:61-68, src/circuits/shot.rs:921-928,
// src/circuits/board.rs:913-920, and the verifier half used by benches/board.rs:80-86.
//
// MI355X-first restructuring: upstream halves the generator vector every round
// ("parallel_generator_collapse": n/2 variable-base 255-bit scalar multiplications, then MSMs on
// the folded, non-fixed bases).  Here the generators are NEVER folded.  After j rounds
//     g^(j)_i = sum_t s^(j)_t * G_(i + t*m),  m = n / 2^j,  s^(j+1)_(2t+beta) = s^(j)_t * u_j^beta,
// so L_j = <p_hi, g_lo> and R_j = <p_lo, g_hi> are MSMs over the ORIGINAL SRS with the scalar
// vectors  p_hi[i] * s_t  /  p_lo[i] * s_t  scattered to index i + t*m -- i.e. two more batched
// MSMs against the fixed window table already resident in HBM (bzh_bases_precompute), plus
// O(n) field multiplications for the scalars.  The [value*z]U and [rand]W terms ride in the same
// MSM (U and W are the last two entries of the table).  Output bytes are identical to the
// collapsing formulation (tests/test_gpu_ipa.py pins them against the oracle's restatement of
// upstream under a shared randomness stream).
//
// Round 3: ONE collapse instead of k.  Every round over the original table costs nwin * n bucket additions whatever the
// round, 14 x 24 n at k = 14 -- a third of a proof's additions.  At round j* the folded generators
//     G'[i] = sum_{t < 2^j*} s_t G_(i + t m),  m = n / 2^j*
// are materialised ONCE per proof through the same window table (msm_collapse_table, csrc/msm.hip: the scalars are shared by
// all i, so the bucket method runs with the level as the outer loop and one output per lane: (2^j* nwin + 2 levels) additions
// per output instead of a 255-bit double-and-add per term) and given their own small window table; the remaining rounds are
// the same paired MSMs on m points.  Additions per opening: 24 n j* + ~48 n + 150 m + 26 m (k - j*) instead of 24 n k
// (k = 14, j* = 4: 168 n against 336 n).  The group elements L_j, R_j are the same, hence the proof bytes.  Used when the
// batch is large enough to be throughput-bound (the collapse is two long per-lane chains: it would lengthen a single
// proof); BZH_IPA_COLLAPSE = 0 disables it, = j forces round j at any batch size; BZH_IPA_TAIL_C sets the tail window.
#include <cstdio>
#include <cstring>
#include <vector>

#include "block.cuh"
#include "ctx.hpp"
#include "curve.cuh"
#include "host_field.hpp"
#include "ipa_scalars.hpp"

namespace bzh {

// ---------------------------------------------------------------------------
// kernels (all Montgomery form)
// ---------------------------------------------------------------------------
// 64-byte RNG outputs -> field elements: 512-bit little-endian integer mod p (Field::random)
template <class P>
__global__ void __launch_bounds__(256) k_reduce_wide(const uint32_t* __restrict__ in, size_t count, uint32_t* __restrict__ out) {
    const size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (g >= count) return;
    Fe<P> lo = fe_load<P>(in + g * 16), hi = fe_load<P>(in + g * 16 + 8);
    // value = lo + hi * 2^256; Montgomery image = lo*R + hi*R*R = mul(lo, R2) + mul(mul(hi, R2), R2)
    Fe<P> r2 = fe_r2<P>();
    fe_store(out + g * 8, fe_add(fe_mul(lo, r2), fe_mul(fe_mul(hi, r2), r2)));
}

// s_new[2t + beta] = s[t] * u^beta
template <class P>
__global__ void __launch_bounds__(256) k_ipa_s_update(const uint32_t* __restrict__ s, size_t count, const uint32_t* __restrict__ u,
                                                        uint32_t* __restrict__ s_new) {
    const size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (g >= count) return;
    const Fe<P> v = fe_load<P>(s + g * 8);
    fe_store(s_new + (2 * g) * 8, v);
    fe_store(s_new + (2 * g + 1) * 8, fe_mul(v, fe_load<P>(u)));
}

struct DevBuf {
    void* p = nullptr;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
};

// ---------------------------------------------------------------------------
// prover, batched: `batch` independent openings advance in lockstep so that every round is ONE
// MSM launch of 2*batch vectors, one device->host copy and one host<-device challenge upload.
// Per-proof vectors are compact: p, b are (batch, m) and s is (batch, n/m) in round j (m = n >> j).
// ---------------------------------------------------------------------------
// constants per proof (d_hc, csrc/ipa_scalars.hpp): [0] x3, [1] xi, [2] z, [3] u, [4] u_inv   (stride kHc); written by the host, or by
// the scalar kernels of the device-transcript opening

template <class P>
__global__ void k_sub_at0_batch(uint32_t* __restrict__ v, size_t stride, const uint32_t* __restrict__ s, size_t batch) {
    const size_t b = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (b >= batch) return;
    uint32_t* e = v + b * stride * 8;
    fe_store(e, fe_sub(fe_load<P>(e), fe_load<P>(s + b * 8)));
}

// commit scalars of S: out[b] = [s_poly_b (n) | 0 | s_blind_b]
template <class P>
__global__ void __launch_bounds__(256) k_ipa_commit_scalars(const uint32_t* __restrict__ spoly, const uint32_t* __restrict__ blinds,
                                                              size_t n, size_t blind_stride, uint32_t* __restrict__ out) {
    const size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x, b = blockIdx.y;
    if (g >= n + 2) return;
    Fe<P> v = fe_zero<P>();
    if (g < n) v = fe_load<P>(spoly + (b * n + g) * 8);
    else if (g == n + 1) v = fe_load<P>(blinds + b * blind_stride * 8);
    fe_store(out + (b * (n + 2) + g) * 8, v);
}

// p'[b][i] = poly[b][i] + xi_b * s[b][i]
template <class P>
__global__ void __launch_bounds__(256) k_ipa_axpy(const uint32_t* __restrict__ poly, const uint32_t* __restrict__ spoly,
                                                    const uint32_t* __restrict__ hc, size_t n, uint32_t* __restrict__ out) {
    const size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x, b = blockIdx.y;
    if (g >= n) return;
    const Fe<P> xi = fe_load<P>(hc + (b * kHc + 1) * 8);
    const size_t o = (b * n + g) * 8;
    fe_store(out + o, fe_add(fe_load<P>(poly + o), fe_mul(xi, fe_load<P>(spoly + o))));
}

// bvec[b][i] = x3_b^i, s[b][0] = 1
template <class P>
__global__ void __launch_bounds__(256) k_ipa_init_b_s(const uint32_t* __restrict__ hc, size_t n, uint32_t* __restrict__ bvec,
                                                        uint32_t* __restrict__ s) {
    const size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x, b = blockIdx.y;
    if (g >= n) return;
    Fe<P> acc = fe_one<P>(), pw = fe_load<P>(hc + b * kHc * 8);
    if (g == 0) fe_store(s + b * 8, acc);
    for (size_t e = g; e; e >>= 1) {
        if (e & 1) acc = fe_mul(acc, pw);
        pw = fe_sqr(pw);
    }
    fe_store(bvec + (b * n + g) * 8, acc);
}

// out[b][0] = <p_hi, b_lo>, out[b][1] = <p_lo, b_hi>; grid (batch, 2)
template <class P>
__global__ void __launch_bounds__(256) k_ipa_inner2(const uint32_t* __restrict__ p, const uint32_t* __restrict__ bv, size_t half,
                                                      uint32_t* __restrict__ out) {
    __shared__ __align__(16) uint4 sh[2 * 256];
    const size_t b = blockIdx.x, side = blockIdx.y, m = 2 * half;
    const uint32_t* pa = p + (b * m + (side ? 0 : half)) * 8;
    const uint32_t* ba = bv + (b * m + (side ? half : 0)) * 8;
    Fe<P> acc = fe_zero<P>();
    for (size_t i = threadIdx.x; i < half; i += 256) acc = fe_add(acc, fe_mul(fe_load<P>(pa + i * 8), fe_load<P>(ba + i * 8)));
    acc = block_sum(acc, sh, 256);
    if (threadIdx.x == 0) fe_store(out + (b * 2 + side) * 8, acc);
}

// Round scalars of proof b: for idx < n with r = idx mod m, t = idx div m:
//   L[idx] = r <  m/2 ? p[r + m/2] * s[t] : 0        R[idx] = r >= m/2 ? p[r - m/2] * s[t] : 0
//   L[n] = vl * z, L[n+1] = l_rand                   R[n] = vr * z, R[n+1] = r_rand
template <class P>
__global__ void __launch_bounds__(256) k_ipa_round_vectors(const uint32_t* __restrict__ p, const uint32_t* __restrict__ s, size_t n,
                                                             unsigned log_m, const uint32_t* __restrict__ vlr,
                                                             const uint32_t* __restrict__ hc, const uint32_t* __restrict__ rands,
                                                             size_t nrand, size_t rand_n, unsigned round, uint32_t* __restrict__ lr) {
    const size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x, b = blockIdx.y;
    const size_t m = (size_t)1 << log_m, half = m >> 1;
    const uint32_t* pb = p + b * m * 8;
    const uint32_t* sb = s + b * (n >> log_m) * 8;
    uint32_t* L = lr + b * 2 * (n + 2) * 8;
    uint32_t* R = L + (n + 2) * 8;
    if (g < n) {
        const size_t r = g & (m - 1), t = g >> log_m;
        const Fe<P> st = fe_load<P>(sb + t * 8);
        const Fe<P> zero = fe_zero<P>();
        if (r < half) {
            fe_store(L + g * 8, fe_mul(fe_load<P>(pb + (r + half) * 8), st));
            fe_store(R + g * 8, zero);
        } else {
            fe_store(L + g * 8, zero);
            fe_store(R + g * 8, fe_mul(fe_load<P>(pb + (r - half) * 8), st));
        }
    } else if (g == n) {
        const Fe<P> zz = fe_load<P>(hc + (b * kHc + 2) * 8);
        const uint32_t* rd = rands + (b * nrand + rand_n + 1 + 2 * (size_t)round) * 8;   // rand_n: the opening's full length
        fe_store(L + n * 8, fe_mul(fe_load<P>(vlr + b * 16), zz));
        fe_store(R + n * 8, fe_mul(fe_load<P>(vlr + b * 16 + 8), zz));
        fe_store(L + (n + 1) * 8, fe_load<P>(rd));
        fe_store(R + (n + 1) * 8, fe_load<P>(rd + 8));
    }
}

// The same scalars as ONE dense vector per proof for msm_run_paired (L and R have disjoint supports):
//   LR[idx] = p[(r + m/2) mod m] * s[t]  (class = r >= m/2),  LR[n..n+1] = (vl z, l_rand),  LR[n+2..n+3] = (vr z, r_rand)
template <class P>
__global__ void __launch_bounds__(256) k_ipa_round_vectors_paired(const uint32_t* __restrict__ p, const uint32_t* __restrict__ s,
                                                                    size_t n, unsigned log_m, const uint32_t* __restrict__ vlr,
                                                                    const uint32_t* __restrict__ hc,
                                                                    const uint32_t* __restrict__ rands, size_t nrand, size_t rand_n,
                                                                    unsigned round, uint32_t* __restrict__ lr) {
    const size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x, b = blockIdx.y;
    const size_t m = (size_t)1 << log_m, half = m >> 1;
    uint32_t* V = lr + b * (n + 4) * 8;
    if (g < n) {
        const size_t r = g & (m - 1), t = g >> log_m;
        const size_t src = r < half ? r + half : r - half;
        fe_store(V + g * 8, fe_mul(fe_load<P>(p + (b * m + src) * 8), fe_load<P>(s + (b * (n >> log_m) + t) * 8)));
    } else if (g == n) {
        const Fe<P> zz = fe_load<P>(hc + (b * kHc + 2) * 8);
        const uint32_t* rd = rands + (b * nrand + rand_n + 1 + 2 * (size_t)round) * 8;
        fe_store(V + n * 8, fe_mul(fe_load<P>(vlr + b * 16), zz));
        fe_store(V + (n + 1) * 8, fe_load<P>(rd));
        fe_store(V + (n + 2) * 8, fe_mul(fe_load<P>(vlr + b * 16 + 8), zz));
        fe_store(V + (n + 3) * 8, fe_load<P>(rd + 8));
    }
}

// one launch per round: p' = p_lo + u^-1 p_hi, b' = b_lo + u b_hi (i < half), s'[2t + beta] = s[t] u^beta (t < cnt)
template <class P>
__global__ void __launch_bounds__(256) k_ipa_round_fold(const uint32_t* __restrict__ p, const uint32_t* __restrict__ bv,
                                                          const uint32_t* __restrict__ s, size_t half, size_t cnt,
                                                          const uint32_t* __restrict__ hc, uint32_t* __restrict__ p_out,
                                                          uint32_t* __restrict__ b_out, uint32_t* __restrict__ s_out) {
    const size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x, b = blockIdx.y;
    const Fe<P> u = fe_load<P>(hc + (b * kHc + 3) * 8);
    if (g < half) {
        const Fe<P> ui = fe_load<P>(hc + (b * kHc + 4) * 8);
        const uint32_t* pb = p + b * 2 * half * 8;
        const uint32_t* bb = bv + b * 2 * half * 8;
        fe_store(p_out + (b * half + g) * 8, fe_add(fe_load<P>(pb + g * 8), fe_mul(ui, fe_load<P>(pb + (half + g) * 8))));
        fe_store(b_out + (b * half + g) * 8, fe_add(fe_load<P>(bb + g * 8), fe_mul(u, fe_load<P>(bb + (half + g) * 8))));
    }
    if (g < cnt) {
        const Fe<P> v = fe_load<P>(s + (b * cnt + g) * 8);
        fe_store(s_out + (b * 2 * cnt + 2 * g) * 8, v);
        fe_store(s_out + (b * 2 * cnt + 2 * g + 1) * 8, fe_mul(v, u));
    }
}

// ---------------------------------------------------------------------------
// The opening has one round loop (ipa_open_t) and two transcript drivers.  Everything that is on the device anyway -- the arena,
// k_reduce_wide, the commit scalars, the axpy and the evaluation, the round vectors, the two MSM flavours, the fold, the collapse
// at jstar -- is the loop's; a driver supplies what happens between those launches:
//   draws   the 64-byte draws into d_raw           begin   x3 -> hc[0] (and what the driver keeps of the drawn scalars)
//   head    S -> transcript, xi, z -> hc[1..2], f  keep_v  v = p'(x3) is in d_dv now
//   round   (L_j, R_j) -> transcript, u_j, u_j^-1 -> hc[3..4], f += l_j u_j^-1 + r_j u_j
//   ones    s <- (1) at the collapse               tail    c, f -> transcript, v -> the caller
// IpaHostDriver is bzh_ipa_open(_batch) and the prover: host bzh_transcript objects, one read-back and one upload per step.
// IpaDeviceDriver is bzh_ipa_open_batch_device: a device-resident bzh_transcript_batch, every step a launch.
// ---------------------------------------------------------------------------
struct IpaArena {
    size_t B, n, nrand;
    unsigned k;
    uint32_t *d_raw, *d_rand, *d_hc, *d_dv, *d_extra;   // d_extra: Driver::kExtraWords words per proof
    uint32_t* d_out;                                    // 2 B Jacobian points: S in [0, B), then (L_j, R_j) of proof b at [2b, 2b + 1]
};

template <class C>
struct IpaHostDriver {
    using SF = typename CurveInfo<C>::SF;
    using PB = typename C::Base;
    static constexpr size_t kExtraWords = 0;
    const uint64_t *blinds, *x3s;
    const uint8_t* rng_bytes;
    size_t rng_stride;
    bzh_transcript* const* trs;
    uint64_t* out_v;
    const uint32_t* d_raw_in;
    size_t ntail = 0;
    std::vector<Fe<SF>> tail, hc, f, vm, us, us_inv;
    std::vector<uint64_t> jac, xy;

    int push_hc(bzh_ctx* ctx, const IpaArena& A) { return h2d_small(ctx, A.d_hc, hc.data(), A.B * kHc * 32); }
    int draws(bzh_ctx* ctx, const IpaArena& A) {
        if (d_raw_in) {  // the 64-byte draws are already on the device (batch x nrand, proof-major)
            BZH_HIP_TRY(ctx, hipMemcpyAsync(A.d_raw, d_raw_in, A.B * A.nrand * 64, hipMemcpyDeviceToDevice, ctx->stream));
        } else {
            for (size_t b = 0; b < A.B; b++)
                BZH_TRY(h2d_small(ctx, A.d_raw + b * A.nrand * 16, rng_bytes + b * rng_stride, A.nrand * 64));
        }
        return BZH_OK;
    }
    int begin(bzh_ctx* ctx, const IpaArena& A) {
        const size_t B = A.B;
        ntail = 1 + 2 * (size_t)A.k;
        // the scalars the host needs (s_blind and the round blinds) come back in one strided copy
        tail.resize(B * ntail);
        for (size_t b = 0; b < B; b++) BZH_TRY(d2h_async(ctx, &tail[b * ntail], A.d_rand + (b * A.nrand + A.n) * 8, ntail * 32));
        hc.assign(B * kHc, fe_zero<SF>());
        for (size_t b = 0; b < B; b++) hc[b * kHc] = fe_to_mont(fe_from_u64<SF>(x3s + 4 * b));
        jac.resize(2 * B * 12), xy.resize(2 * B * 8);
        f.resize(B), vm.resize(B), us.resize(B);
        return push_hc(ctx, A);
    }
    int head(bzh_ctx* ctx, const IpaArena& A) {
        const size_t B = A.B;
        BZH_TRY(d2h_async(ctx, jac.data(), A.d_out, B * 96));
        BZH_TRY(d2h_finish(ctx));
        h_jac_to_affine<PB>(jac.data(), B, BZH_FORM_MONTGOMERY, BZH_FORM_CANONICAL, xy.data());
        uint64_t ch[4];
        for (size_t b = 0; b < B; b++) {
            BZH_TRY(bzh_transcript_write_point(trs[b], C::id, xy.data() + b * 8));
            BZH_TRY(bzh_transcript_squeeze_challenge(trs[b], ch));
            const Fe<SF> xi = fe_to_mont(fe_from_u64<SF>(ch));
            BZH_TRY(bzh_transcript_squeeze_challenge(trs[b], ch));
            hc[b * kHc + 1] = xi;
            hc[b * kHc + 2] = fe_to_mont(fe_from_u64<SF>(ch));
            f[b] = fe_add(fe_mul(tail[b * ntail], xi), fe_to_mont(fe_from_u64<SF>(blinds + 4 * b)));
        }
        return push_hc(ctx, A);
    }
    int keep_v(bzh_ctx* ctx, const IpaArena& A) { return d2h_async(ctx, vm.data(), A.d_dv, A.B * 32); }  // lands at the next d2h_finish
    int round(bzh_ctx* ctx, const IpaArena& A, unsigned j) {
        const size_t B = A.B;
        BZH_TRY(d2h_async(ctx, jac.data(), A.d_out, 2 * B * 96));
        BZH_TRY(d2h_finish(ctx));
        h_jac_to_affine<PB>(jac.data(), 2 * B, BZH_FORM_MONTGOMERY, BZH_FORM_CANONICAL, xy.data());
        uint64_t ch[4];
        for (size_t b = 0; b < B; b++) {
            BZH_TRY(bzh_transcript_write_point(trs[b], C::id, xy.data() + (2 * b) * 8));
            BZH_TRY(bzh_transcript_write_point(trs[b], C::id, xy.data() + (2 * b + 1) * 8));
            BZH_TRY(bzh_transcript_squeeze_challenge(trs[b], ch));
            us[b] = fe_to_mont(fe_from_u64<SF>(ch));
        }
        us_inv = us;
        if (!h_batch_invert(us_inv.data(), B)) return BZH_E_ARG;  // a zero challenge has no inverse (probability 2^-255)
        for (size_t b = 0; b < B; b++) {
            hc[b * kHc + 3] = us[b];
            hc[b * kHc + 4] = us_inv[b];
            f[b] = fe_add(f[b], fe_add(fe_mul(tail[b * ntail + 1 + 2 * j], us_inv[b]), fe_mul(tail[b * ntail + 2 + 2 * j], us[b])));
        }
        return push_hc(ctx, A);
    }
    int ones(bzh_ctx* ctx, const IpaArena& A, uint32_t* s_cur) {
        std::vector<Fe<SF>> one(A.B, fe_one<SF>());
        return h2d_small(ctx, s_cur, one.data(), A.B * 32);
    }
    int tail_out(bzh_ctx* ctx, const IpaArena& A, const uint32_t* p_cur) {
        const size_t B = A.B;
        std::vector<Fe<SF>> c(B);
        BZH_TRY(d2h_async(ctx, c.data(), p_cur, B * 32));
        BZH_TRY(d2h_finish(ctx));
        for (size_t b = 0; b < B; b++) {
            fe_to_u64<SF>(out_v + 4 * b, fe_from_mont(vm[b]));
            uint64_t sc[4];
            fe_to_u64<SF>(sc, fe_from_mont(c[b]));
            BZH_TRY(bzh_transcript_write_scalar(trs[b], sc));
            fe_to_u64<SF>(sc, fe_from_mont(f[b]));
            BZH_TRY(bzh_transcript_write_scalar(trs[b], sc));
        }
        return BZH_OK;
    }
    void msm_begin(bzh_ctx*) {}
    void msm_end(bzh_ctx*) {}
};

// One lane per proof, 1-D grid over B in blocks of 64 (B = 65: a second, partial wave).  For B <= 64 each of these launches, like
// the normalise and the transcript launches around them, is ONE wave: its time is the length of its dependent chain, not
// throughput.  A round has two inversion chains of about 330 products each (fe_inv_ct), one after the other -- the normalise's (L_j and R_j
// share it) and u_j's in k_ipa_round_scalars -- and nothing here tries to hide that.
static constexpr unsigned kLaneBlock = 64;
template <class P>
__global__ void __launch_bounds__(kLaneBlock) k_ipa_x3(const uint32_t* __restrict__ x3s, int canonical, size_t batch,
                                                       uint32_t* __restrict__ hc, uint8_t* __restrict__ status) {
    const size_t b = blockIdx.x * (size_t)kLaneBlock + threadIdx.x;
    if (b >= batch) return;
    ipa_x3_lane<P>(b, x3s, canonical != 0, hc, status);
}
template <class P>
__global__ void __launch_bounds__(kLaneBlock) k_ipa_head_scalars(const uint32_t* __restrict__ ch, const uint32_t* __restrict__ rands,
                                                                 size_t nrand, size_t n, const uint32_t* __restrict__ blinds,
                                                                 int canonical, size_t batch, uint32_t* __restrict__ hc,
                                                                 uint32_t* __restrict__ f) {
    const size_t b = blockIdx.x * (size_t)kLaneBlock + threadIdx.x;
    if (b >= batch) return;
    ipa_head_lane<P>(b, batch, ch, rands, nrand, n, blinds, canonical != 0, hc, f);
}
template <class P>
__global__ void __launch_bounds__(kLaneBlock) k_ipa_round_scalars(const uint32_t* __restrict__ ch, const uint32_t* __restrict__ rands,
                                                                  size_t nrand, size_t n, unsigned round, size_t batch,
                                                                  uint32_t* __restrict__ hc, uint32_t* __restrict__ f,
                                                                  uint8_t* __restrict__ status) {
    const size_t b = blockIdx.x * (size_t)kLaneBlock + threadIdx.x;
    if (b >= batch) return;
    ipa_round_lane<P>(b, ch, rands, nrand, n, round, hc, f, status);
}
template <class P>
__global__ void __launch_bounds__(kLaneBlock) k_ipa_tail_scalars(const uint32_t* __restrict__ p, const uint32_t* __restrict__ f,
                                                                 const uint32_t* __restrict__ v, int canonical, size_t batch,
                                                                 uint32_t* __restrict__ cf, uint32_t* __restrict__ out_v) {
    const size_t b = blockIdx.x * (size_t)kLaneBlock + threadIdx.x;
    if (b >= batch) return;
    ipa_tail_lane<P>(b, p, f, v, canonical != 0, cf, out_v);
}
template <class P>
__global__ void __launch_bounds__(kLaneBlock) k_ipa_fill_one(uint32_t* __restrict__ s, size_t batch) {
    const size_t b = blockIdx.x * (size_t)kLaneBlock + threadIdx.x;
    if (b >= batch) return;
    fe_store(s + b * 8, fe_one<P>());
}

template <class C>
struct IpaDeviceDriver {
    using SF = typename CurveInfo<C>::SF;
    static constexpr size_t kExtraWords = 2 * 8 + 8 + 2 * 8;   // per proof: two challenges | f | (c, f)
    bzh_transcript_batch* tb;
    const uint32_t *d_blinds, *d_x3s;
    const uint8_t* d_rng;
    size_t rng_stride;
    uint32_t* d_out_v;
    uint8_t* d_status;   // may be null
    int form;
    // BZH_PROVE_TRACE=1: the steps' times by events, on stderr (tools/ubench_ipa_open.py reads the line); one wait at the end
    enum { kNormAbsorb = 0, kSqueeze, kScalars, kMsm, kClasses };
    bool trace = false;
    struct Mark {
        int cls;
        hipEvent_t a, b;
    };
    std::vector<Mark> marks;
    hipEvent_t msm_a = nullptr;

    dim3 lanes(const IpaArena& A) const { return dim3((unsigned)((A.B + kLaneBlock - 1) / kLaneBlock)); }
    uint32_t* ch(const IpaArena& A) const { return A.d_extra; }
    uint32_t* fv(const IpaArena& A) const { return A.d_extra + A.B * 16; }
    uint32_t* cf(const IpaArena& A) const { return A.d_extra + A.B * 24; }
    hipEvent_t mark_begin(bzh_ctx* ctx) {
        hipEvent_t e = nullptr;
        if (trace && hipEventCreate(&e) == hipSuccess) (void)hipEventRecord(e, ctx->stream);
        return e;
    }
    void mark_end(bzh_ctx* ctx, int cls, hipEvent_t a) {
        hipEvent_t e = nullptr;
        if (!trace || !a || hipEventCreate(&e) != hipSuccess) return;
        (void)hipEventRecord(e, ctx->stream);
        marks.push_back({cls, a, e});
    }
    void msm_begin(bzh_ctx* ctx) { msm_a = mark_begin(ctx); }
    void msm_end(bzh_ctx* ctx) { mark_end(ctx, kMsm, msm_a); }
    int absorb_points(bzh_ctx* ctx, const IpaArena& A, size_t count) {
        hipEvent_t a = mark_begin(ctx);
        BZH_TRY(tb_write_jacobian_locked(tb, A.d_out, count, count, BZH_FORM_MONTGOMERY));
        mark_end(ctx, kNormAbsorb, a);
        return BZH_OK;
    }
    int squeeze(bzh_ctx* ctx, uint32_t* d_to) {
        hipEvent_t a = mark_begin(ctx);
        BZH_TRY(tb_squeeze_locked(tb, BZH_FORM_MONTGOMERY, d_to));
        mark_end(ctx, kSqueeze, a);
        return BZH_OK;
    }

    int draws(bzh_ctx* ctx, const IpaArena& A) {
        trace = getenv("BZH_PROVE_TRACE") != nullptr;
        BZH_HIP_TRY(ctx, hipMemcpy2DAsync(A.d_raw, A.nrand * 64, d_rng, rng_stride, A.nrand * 64, A.B, hipMemcpyDeviceToDevice, ctx->stream));
        return BZH_OK;
    }
    int begin(bzh_ctx* ctx, const IpaArena& A) {
        hipLaunchKernelGGL((k_ipa_x3<SF>), lanes(A), dim3(kLaneBlock), 0, ctx->stream, d_x3s, form == BZH_FORM_CANONICAL ? 1 : 0, A.B, A.d_hc,
                           d_status);
        BZH_HIP_TRY(ctx, hipGetLastError());
        return BZH_OK;
    }
    int head(bzh_ctx* ctx, const IpaArena& A) {
        BZH_TRY(absorb_points(ctx, A, 1));
        BZH_TRY(squeeze(ctx, ch(A)));
        BZH_TRY(squeeze(ctx, ch(A) + A.B * 8));
        hipEvent_t a = mark_begin(ctx);
        hipLaunchKernelGGL((k_ipa_head_scalars<SF>), lanes(A), dim3(kLaneBlock), 0, ctx->stream, ch(A), A.d_rand, A.nrand, A.n, d_blinds,
                           form == BZH_FORM_CANONICAL ? 1 : 0, A.B, A.d_hc, fv(A));
        mark_end(ctx, kScalars, a);
        BZH_HIP_TRY(ctx, hipGetLastError());
        return BZH_OK;
    }
    int keep_v(bzh_ctx*, const IpaArena&) { return BZH_OK; }   // d_dv is not written again: the tail reads it
    int round(bzh_ctx* ctx, const IpaArena& A, unsigned j) {
        BZH_TRY(absorb_points(ctx, A, 2));
        BZH_TRY(squeeze(ctx, ch(A)));
        hipEvent_t a = mark_begin(ctx);
        hipLaunchKernelGGL((k_ipa_round_scalars<SF>), lanes(A), dim3(kLaneBlock), 0, ctx->stream, ch(A), A.d_rand, A.nrand, A.n, j, A.B, A.d_hc,
                           fv(A), d_status);
        mark_end(ctx, kScalars, a);
        BZH_HIP_TRY(ctx, hipGetLastError());
        return BZH_OK;
    }
    int ones(bzh_ctx* ctx, const IpaArena& A, uint32_t* s_cur) {
        hipLaunchKernelGGL((k_ipa_fill_one<SF>), lanes(A), dim3(kLaneBlock), 0, ctx->stream, s_cur, A.B);
        BZH_HIP_TRY(ctx, hipGetLastError());
        return BZH_OK;
    }
    int tail_out(bzh_ctx* ctx, const IpaArena& A, const uint32_t* p_cur) {
        hipLaunchKernelGGL((k_ipa_tail_scalars<SF>), lanes(A), dim3(kLaneBlock), 0, ctx->stream, p_cur, fv(A), A.d_dv,
                           form == BZH_FORM_CANONICAL ? 1 : 0, A.B, cf(A), d_out_v);
        BZH_HIP_TRY(ctx, hipGetLastError());
        BZH_TRY(tb_absorb_locked(tb, 3, cf(A), 2, 2, BZH_FORM_MONTGOMERY, nullptr));
        if (trace) {
            double ms[kClasses] = {0, 0, 0, 0};
            BZH_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            for (auto& m : marks) {
                float t = 0;
                (void)hipEventElapsedTime(&t, m.a, m.b);
                ms[m.cls] += t;
                (void)hipEventDestroy(m.a), (void)hipEventDestroy(m.b);
            }
            marks.clear();
            fprintf(stderr, "[bzh_ipa_open_batch_device] batch=%zu k=%u io:normalize_absorb_ms=%.4f io:squeeze_ms=%.4f io:round_scalars_ms=%.4f io:msm_ms=%.4f\n",
                    A.B, A.k, ms[kNormAbsorb], ms[kSqueeze], ms[kScalars], ms[kMsm]);
        }
        return BZH_OK;
    }
};

template <class C, class D>
static int ipa_open_t(bzh_ctx* ctx, const bzh_bases* bases, const uint32_t* d_polys, size_t batch, D& drv) {
    using SF = typename CurveInfo<C>::SF;
    const int field = CurveInfo<C>::scalar_field;
    const size_t n = bases->n - 2, B = batch;
    unsigned k = 0;
    while (((size_t)1 << k) < n) k++;
    if (((size_t)1 << k) != n || !B) return BZH_E_ARG;
    const size_t nrand = n + 1 + 2 * (size_t)k;
    hipStream_t st = ctx->stream;

    // The generator collapse: at round jstar the folded generators get their own tables and the rounds continue on m points
    // (header).  jstar minimises  24 n j + 48 n + 150 m + 26 m (k - j)  over the rounds that leave m >= 64.
    unsigned jstar = 0;
    int tail_c = 9;
    {
        static const int env_j = [] {
            const char* e = getenv("BZH_IPA_COLLAPSE");
            return e ? atoi(e) : -1;
        }();
        static const int env_c = [] {
            const char* e = getenv("BZH_IPA_TAIL_C");
            return e ? atoi(e) : 0;
        }();
        if (env_c >= 4 && env_c <= 13) tail_c = env_c;
        if (bases->pre_c != 0 && !bases->vec_col_stride && env_j != 0) {
            if (env_j > 0) {
                if ((unsigned)env_j + 1 < k) jstar = (unsigned)env_j;   // forced (tests): any batch size, m >= 2
            } else if (B >= 8 && k >= 9) {
                double best = 24.0 * (double)n * k * 0.9;               // at least 10 % fewer additions than no collapse
                for (unsigned j = 1; j + 6 <= k; j++) {
                    const double m = (double)(n >> j);
                    const double cost = 24.0 * n * j + 48.0 * n + 150.0 * m + 26.0 * m * (k - j);
                    if (cost < best) {
                        best = cost;
                        jstar = j;
                    }
                }
            }
            if (jstar && (size_t)(2 * ((size_t)1 << jstar) * bases->pre_nwin) * 4 > 48 * 1024) jstar = 0;   // item lists must fit LDS
        }
    }
    const size_t tail_m = jstar ? n >> jstar : 0;
    const int tail_nwin = (256 + tail_c - 1) / tail_c;
    const size_t tail_scratch = jstar ? msm_collapse_scratch_bytes(bases, (size_t)1 << jstar, B, tail_c) : 0;
    // device arena (WS_IPA; the MSMs, the collapse and the poly_* calls of the rounds take WS_SCRATCH_* only), per proof:
    // raw rng | rand scalars | s_poly | p x2 | b x2 | s x2 | LR | S scalars | small | the driver's own
    const size_t per = nrand * 16 + nrand * 8 + n * 8 + 2 * n * 8 + 2 * n * 8 + 2 * n * 8 + 2 * (n + 4) * 8 + (n + 2) * 8 +
                       (kHc + 4) * 8 + D::kExtraWords;
    const size_t tail_words = jstar ? B * (tail_m + 2) * (size_t)tail_nwin * (16 + 20) + (tail_scratch + 3) / 4 + 64 : 0;   // table + its fe29 copy
    void* arena = nullptr;
    BZH_TRY(ws_ensure(ctx, WS_IPA, (B * per + tail_words) * 4 + 256 + 16 * 16, &arena));   // (+ the roundings of take())
    uint32_t* cur = (uint32_t*)arena;
    auto take = [&](size_t w) {   // every piece starts 16-byte aligned (uint4 loads / stores): word counts rounded up to 4
        uint32_t* r = cur;
        cur += (w + 3) & ~(size_t)3;
        return r;
    };
    uint32_t* d_raw = take(B * nrand * 16);
    uint32_t* d_rand = take(B * nrand * 8);
    uint32_t* d_spoly = take(B * n * 8);
    uint32_t* p_cur = take(B * n * 8);
    uint32_t* p_nxt = take(B * n * 8);
    uint32_t* b_cur = take(B * n * 8);
    uint32_t* b_nxt = take(B * n * 8);
    uint32_t* s_cur = take(B * n * 8);
    uint32_t* s_nxt = take(B * n * 8);
    uint32_t* d_lr = take(B * 2 * (n + 4) * 8);
    // window table: L_j and R_j of a proof share one dense vector (msm_run_paired).  Its 16-bit digits hold bucket + class * M below
    // 2^15, so a table of width c = 15 (M = 2^14; bzh_bases_precompute accepts it) takes the two-vector rounds instead.  A tail
    // table has c <= 13: once collapsed, the rounds always pair.
    auto pairs = [](const bzh_bases* t) { return t->pre_c != 0 && t->pre_c <= 14; };
    uint32_t* d_commit = take(B * (n + 2) * 8);
    uint32_t* d_tail_table = jstar ? take(B * (tail_m + 2) * (size_t)tail_nwin * 16) : nullptr;
    uint32_t* d_tail_table29 = jstar ? take(B * (tail_m + 2) * (size_t)tail_nwin * 20) : nullptr;
    void* d_tail_scratch = jstar ? (void*)take((tail_scratch + 3) / 4) : nullptr;
    uint32_t* d_hc = take(B * kHc * 8);
    uint32_t* d_dv = take(B * 8);       // s(x3) / v per proof
    uint32_t* d_vlr = take(B * 2 * 8);  // value_l, value_r per proof
    uint32_t* d_extra = D::kExtraWords ? take(B * D::kExtraWords) : nullptr;
    void* d_out = nullptr;
    BZH_TRY(ws_ensure(ctx, WS_IPA_OUT, 2 * B * 96, &d_out));   // each round's MSM writes here: msm_run* take WS_SCRATCH_* only
    const IpaArena A{B, n, nrand, k, d_raw, d_rand, d_hc, d_dv, d_extra, (uint32_t*)d_out};

    const unsigned g256 = 256;
    auto grid2 = [&](size_t c) { return dim3((unsigned)((c + g256 - 1) / g256), (unsigned)B); };
    if (B > 65535) return BZH_E_ARG;

    // randomness: upstream draw order = n coefficients of s(X), s_blind, then (l_j, r_j) per round
    BZH_TRY(drv.draws(ctx, A));
    hipLaunchKernelGGL((k_reduce_wide<SF>), dim3((unsigned)((B * nrand + g256 - 1) / g256)), dim3(g256), 0, st, d_raw, B * nrand,
                       d_rand);
    BZH_HIP_TRY(ctx, hipMemcpy2DAsync(d_spoly, n * 32, d_rand, nrand * 32, n * 32, B, hipMemcpyDeviceToDevice, st));
    BZH_TRY(drv.begin(ctx, A));
    // s(X) -= s(x3)
    BZH_TRY(poly_eval(ctx, field, d_spoly, n, B, d_hc, kHc, d_dv));
    hipLaunchKernelGGL((k_sub_at0_batch<SF>), dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, d_spoly, n, d_dv, B);
    // S = commit(s, s_blind): scalars [s..., 0, s_blind]
    hipLaunchKernelGGL((k_ipa_commit_scalars<SF>), grid2(n + 2), dim3(g256), 0, st, d_spoly, d_rand + n * 8, n, nrand, d_commit);
    BZH_HIP_TRY(ctx, hipGetLastError());
    drv.msm_begin(ctx);
    BZH_TRY(msm_run(ctx, bases, d_commit, n + 2, B, BZH_FORM_MONTGOMERY, (uint32_t*)d_out));
    drv.msm_end(ctx);
    BZH_TRY(drv.head(ctx, A));
    // p' = poly + xi * s_poly, then p'[0] -= v with v = p'(x3)
    hipLaunchKernelGGL((k_ipa_axpy<SF>), grid2(n), dim3(g256), 0, st, d_polys, d_spoly, d_hc, n, p_cur);
    BZH_TRY(poly_eval(ctx, field, p_cur, n, B, d_hc, kHc, d_dv));
    hipLaunchKernelGGL((k_sub_at0_batch<SF>), dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, p_cur, n, d_dv, B);
    BZH_TRY(drv.keep_v(ctx, A));
    hipLaunchKernelGGL((k_ipa_init_b_s<SF>), grid2(n), dim3(g256), 0, st, d_hc, n, b_cur, s_cur);
    BZH_HIP_TRY(ctx, hipGetLastError());

    // the instance the rounds run on: the SRS and n points, or (from round jstar on) the per-proof tables and tail_m points
    const bzh_bases* rb = bases;
    bzh_bases tail_bases;
    size_t rn = n;          // points of the current instance
    unsigned j0 = 0;        // the round its s vector restarted at
    for (unsigned j = 0; j < k; j++) {
        if (jstar && j == jstar) {
            BZH_TRY(msm_collapse_table(ctx, bases, s_cur, (size_t)1 << j, B, tail_c, d_tail_table29, d_tail_table, d_tail_scratch, &tail_bases));
            rb = &tail_bases;
            rn = tail_m;
            j0 = j;
            // s restarts at (1): the folded generators ARE the instance now
            BZH_TRY(drv.ones(ctx, A, s_cur));
        }
        const size_t m = n >> j, half = m >> 1, cnt = (size_t)1 << (j - j0);
        hipLaunchKernelGGL((k_ipa_inner2<SF>), dim3((unsigned)B, 2), dim3(256), 0, st, p_cur, b_cur, half, d_vlr);
        if (pairs(rb)) {
            hipLaunchKernelGGL((k_ipa_round_vectors_paired<SF>), grid2(rn + 1), dim3(g256), 0, st, p_cur, s_cur, rn, k - j, d_vlr, d_hc,
                               d_rand, nrand, n, j, d_lr);
            BZH_HIP_TRY(ctx, hipGetLastError());
            drv.msm_begin(ctx);
            BZH_TRY(msm_run_paired(ctx, rb, d_lr, rn, k - j, B, BZH_FORM_MONTGOMERY, (uint32_t*)d_out));
        } else {   // (rb is the SRS here)
            hipLaunchKernelGGL((k_ipa_round_vectors<SF>), grid2(n + 1), dim3(g256), 0, st, p_cur, s_cur, n, k - j, d_vlr, d_hc,
                               d_rand, nrand, n, j, d_lr);
            BZH_HIP_TRY(ctx, hipGetLastError());
            drv.msm_begin(ctx);
            BZH_TRY(msm_run(ctx, bases, d_lr, n + 2, 2 * B, BZH_FORM_MONTGOMERY, (uint32_t*)d_out));
        }
        drv.msm_end(ctx);
        BZH_TRY(drv.round(ctx, A, j));
        // p' <- p_lo + u^-1 p_hi ; b <- b_lo + u b_hi ; s <- s (x) (1, u)
        hipLaunchKernelGGL((k_ipa_round_fold<SF>), grid2(half > cnt ? half : cnt), dim3(g256), 0, st, p_cur, b_cur, s_cur, half, cnt,
                           d_hc, p_nxt, b_nxt, s_nxt);
        BZH_HIP_TRY(ctx, hipGetLastError());
        std::swap(p_cur, p_nxt);
        std::swap(b_cur, b_nxt);
        std::swap(s_cur, s_nxt);
    }
    return drv.tail_out(ctx, A, p_cur);
}

// ---------------------------------------------------------------------------
// verifier:  sum_j (u_j^-1 L_j + u_j R_j) + P - [v]G_0 + [xi]S  ==  [c]G'_0 + [c b_0 z]U + [f]W
// The n-term G'_0 = <s, G> runs on the GPU against the SRS table with s started at c; the
// (2k+5)-term left side is a second, small MSM on an ad-hoc table.
// ---------------------------------------------------------------------------
template <class C>
static int ipa_verify_t(bzh_ctx* ctx, const bzh_bases* bases, const uint64_t* commitment_xy, const uint64_t* x3, const uint64_t* v,
                        const uint8_t* proof, size_t proof_len, bzh_transcript* tr, const uint64_t* g0_u_w_xy) {
    using SF = typename CurveInfo<C>::SF;
    const size_t n = bases->n - 2;
    unsigned k = 0;
    while (((size_t)1 << k) < n) k++;
    if (((size_t)1 << k) != n) return BZH_E_ARG;
    if (proof_len != 32 * (1 + 2 * (size_t)k + 2)) return BZH_E_VERIFY;
    hipStream_t st = ctx->stream;
    const size_t nl = 2 * (size_t)k + 5;
    std::vector<uint64_t> pts(nl * 8), scal(nl * 4);
    uint64_t ch[4];
    // S
    uint64_t S[8];
    // identity points cannot enter the transcript upstream (Blake2bRead::common_point errors): reject them
    auto is_identity = [](const uint64_t* p) {
        uint64_t any = 0;
        for (int i = 0; i < 8; i++) any |= p[i];
        return any == 0;
    };
    if (!h_decompress<C>(proof, S) || is_identity(S)) return BZH_E_VERIFY;
    BZH_TRY(bzh_transcript_common_point(tr, S));
    BZH_TRY(bzh_transcript_squeeze_challenge(tr, ch));
    const Fe<SF> xi = fe_to_mont(fe_from_u64<SF>(ch));
    BZH_TRY(bzh_transcript_squeeze_challenge(tr, ch));
    const Fe<SF> z = fe_to_mont(fe_from_u64<SF>(ch));
    std::vector<Fe<SF>> us(k);
    for (unsigned j = 0; j < k; j++) {
        uint64_t* L = &pts[(2 * j) * 8];
        uint64_t* R = &pts[(2 * j + 1) * 8];
        if (!h_decompress<C>(proof + 32 + 64 * j, L) || !h_decompress<C>(proof + 64 + 64 * j, R)) return BZH_E_VERIFY;
        if (is_identity(L) || is_identity(R)) return BZH_E_VERIFY;
        BZH_TRY(bzh_transcript_common_point(tr, L));
        BZH_TRY(bzh_transcript_common_point(tr, R));
        BZH_TRY(bzh_transcript_squeeze_challenge(tr, ch));
        us[j] = fe_to_mont(fe_from_u64<SF>(ch));
        if (fe_is_zero(us[j])) return BZH_E_VERIFY;
        fe_to_u64<SF>(&scal[(2 * j) * 4], fe_from_mont(fe_inv(us[j])));
        fe_to_u64<SF>(&scal[(2 * j + 1) * 4], fe_from_mont(us[j]));
    }
    uint64_t cl[4], fl[4];
    memcpy(cl, proof + 32 + 64 * k, 32);
    memcpy(fl, proof + 64 + 64 * k, 32);
    Fe<SF> c = fe_from_u64<SF>(cl), f = fe_from_u64<SF>(fl);
    if (!is_canonical(c) || !is_canonical(f)) return BZH_E_VERIFY;
    const Fe<SF> cm = fe_to_mont(c), fm = fe_to_mont(f), x3m = fe_to_mont(fe_from_u64<SF>(x3)), vm = fe_to_mont(fe_from_u64<SF>(v));
    // b_0 = prod_j (1 + u_j x3^(2^(k-1-j)))
    std::vector<Fe<SF>> xp(k ? k : 1);
    if (k) {
        xp[0] = x3m;
        for (unsigned i = 1; i < k; i++) xp[i] = fe_sqr(xp[i - 1]);
    }
    Fe<SF> b0 = fe_one<SF>();
    for (unsigned j = 0; j < k; j++) b0 = fe_mul(b0, fe_add(fe_one<SF>(), fe_mul(us[j], xp[k - 1 - j])));
    // left-side table tail: P (1), G_0 (-v), S (xi), U (-c b0 z), W (-f)
    size_t o = 2 * (size_t)k;
    memcpy(&pts[o * 8], commitment_xy, 64);
    fe_to_u64<SF>(&scal[o * 4], fe_from_mont(fe_one<SF>()));
    o++;
    memcpy(&pts[o * 8], g0_u_w_xy, 64);
    fe_to_u64<SF>(&scal[o * 4], fe_from_mont(fe_neg(vm)));
    o++;
    memcpy(&pts[o * 8], S, 64);
    fe_to_u64<SF>(&scal[o * 4], fe_from_mont(xi));
    o++;
    memcpy(&pts[o * 8], g0_u_w_xy + 8, 64);
    fe_to_u64<SF>(&scal[o * 4], fe_from_mont(fe_neg(fe_mul(fe_mul(cm, b0), z))));
    o++;
    memcpy(&pts[o * 8], g0_u_w_xy + 16, 64);
    fe_to_u64<SF>(&scal[o * 4], fe_from_mont(fe_neg(fm)));

    // device: s vector (started at c) and the two MSMs
    DevBuf arena;
    const size_t words = 2 * (n + 2) * 8 + nl * 16 + nl * 8 + 64;
    BZH_HIP_TRY(ctx, hipMalloc(&arena.p, words * 4));
    uint32_t* d_s0 = (uint32_t*)arena.p;
    uint32_t* d_s1 = d_s0 + (n + 2) * 8;
    uint32_t* d_pts = d_s1 + (n + 2) * 8;
    uint32_t* d_scal = d_pts + nl * 16;
    uint32_t* d_u = d_scal + nl * 8;
    BZH_HIP_TRY(ctx, hipMemcpyAsync(d_s0, cm.l, 32, hipMemcpyHostToDevice, st));
    BZH_HIP_TRY(ctx, hipStreamSynchronize(st));
    uint32_t* s_cur = d_s0;
    uint32_t* s_nxt = d_s1;
    for (unsigned j = 0; j < k; j++) {
        BZH_HIP_TRY(ctx, hipMemcpyAsync(d_u, us[j].l, 32, hipMemcpyHostToDevice, st));
        const size_t cnt = (size_t)1 << j;
        hipLaunchKernelGGL((k_ipa_s_update<SF>), dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, s_cur, cnt, d_u, s_nxt);
        BZH_HIP_TRY(ctx, hipGetLastError());
        BZH_HIP_TRY(ctx, hipStreamSynchronize(st));
        std::swap(s_cur, s_nxt);
    }
    BZH_HIP_TRY(ctx, hipMemsetAsync(s_cur + n * 8, 0, 64, st));  // no U / W contribution on the right
    void* d_out = nullptr;
    BZH_TRY(ws_ensure(ctx, WS_STAGE, 4 * 96, &d_out));   // the MSMs' result points: msm_run takes WS_SCRATCH_* only (bzh_ipa_verify stages nothing else)
    BZH_TRY(msm_run(ctx, bases, s_cur, n + 2, 1, BZH_FORM_MONTGOMERY, (uint32_t*)d_out));
    uint64_t jac[24];
    BZH_HIP_TRY(ctx, hipMemcpyAsync(jac, d_out, 96, hipMemcpyDeviceToHost, st));
    // left side on an ad-hoc table (canonical in)
    BZH_HIP_TRY(ctx, hipMemcpyAsync(d_pts, pts.data(), nl * 64, hipMemcpyHostToDevice, st));
    BZH_HIP_TRY(ctx, hipMemcpyAsync(d_scal, scal.data(), nl * 32, hipMemcpyHostToDevice, st));
    BZH_TRY(bases_to_montgomery(ctx, C::id, d_pts, nl));
    bzh_bases tmp;
    tmp.curve = C::id;
    tmp.n = nl;
    tmp.d_xy = d_pts;
    tmp.device = ctx->device;
    BZH_TRY(msm_run(ctx, &tmp, d_scal, nl, 1, BZH_FORM_CANONICAL, (uint32_t*)d_out + 24));
    BZH_HIP_TRY(ctx, hipMemcpyAsync(jac + 12, (uint32_t*)d_out + 24, 96, hipMemcpyDeviceToHost, st));
    BZH_HIP_TRY(ctx, hipStreamSynchronize(st));
    uint64_t rhs[8], lhs[8];
    h_jac_to_affine<typename C::Base>(jac, 1, BZH_FORM_MONTGOMERY, BZH_FORM_CANONICAL, rhs);
    h_jac_to_affine<typename C::Base>(jac + 12, 1, BZH_FORM_CANONICAL, BZH_FORM_CANONICAL, lhs);  // the second MSM ran with canonical form
    return memcmp(lhs, rhs, 64) == 0 ? BZH_OK : BZH_E_VERIFY;
}

// s[b][i] = c_b * prod_{j : bit (k-1-j) of i} u_(b,j)  for i < n;  s[b][n], s[b][n+1] = 0   (the verifier's G'_0 scalars)
template <class P>
__global__ void __launch_bounds__(256) k_ipa_verify_s(const uint32_t* __restrict__ cu, size_t n, unsigned k, uint32_t* __restrict__ s) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x, b = blockIdx.y;
    if (i >= n + 2) return;
    Fe<P> acc = fe_zero<P>();
    if (i < n) {
        const uint32_t* row = cu + b * (size_t)(k + 1) * 8;  // [c, u_0 .. u_(k-1)]
        acc = fe_load<P>(row);
        for (unsigned j = 0; j < k; j++)
            if ((i >> (k - 1 - j)) & 1) acc = fe_mul(acc, fe_load<P>(row + (size_t)(j + 1) * 8));
    }
    fe_store(s + (b * (n + 2) + i) * 8, acc);
}

// One workgroup per opening: sum_i scal[b][i] * pts[b][i] over nl (~100) ad-hoc points, one term per lane by
// double-and-add (scalars canonical, points affine Montgomery, (0,0) = identity padding), then an LDS tree over the
// lanes.  The 255 dependent doublings of a fresh point (~5 us each on a SIMD of its own) are the floor of any schedule
// for this sum, ~1.5 ms; work and workspace are linear in the batch (a shared Pippenger table over batch * nl points
// was quadratic in it).
static constexpr int kSmallMsmThreads = 128;
template <class C>
__global__ void __launch_bounds__(kSmallMsmThreads) k_ipa_small_msm(const uint32_t* __restrict__ pts, const uint32_t* __restrict__ scal,
                                                                     size_t nl, uint32_t* __restrict__ out_xyz) {
    using P = typename C::Base;
    constexpr int T = kSmallMsmThreads;
    __shared__ Xyzz<P> sh[T];
    const int lane = threadIdx.x;
    const size_t b = blockIdx.x;
    Xyzz<P> sum = xyzz_identity<P>();
    for (size_t i = lane; i < nl; i += T) {
        Affine<P> q;
        q.x = fe_load<P>(pts + (b * nl + i) * 16);
        q.y = fe_load<P>(pts + (b * nl + i) * 16 + 8);
        if (aff_is_id(q)) continue;
        const uint32_t* sc = scal + (b * nl + i) * 8;
        int top = 255;
        while (top >= 0 && !((sc[top >> 5] >> (top & 31)) & 1)) top--;
        if (top < 0) continue;
        Xyzz<P> acc = xyzz_from_affine(q);
        for (int bit = top - 1; bit >= 0; bit--) {
            acc = xyzz_dbl_inl(acc);
            if ((sc[bit >> 5] >> (bit & 31)) & 1) xyzz_madd(acc, q);
        }
        xyzz_add(sum, acc);
    }
    sh[lane] = sum;
    __syncthreads();
    for (int d = T >> 1; d >= 1; d >>= 1) {
        if (lane < d) {
            Xyzz<P> o = sh[lane + d];
            xyzz_add(sum, o);
            sh[lane] = sum;
        }
        __syncthreads();
    }
    if (lane == 0) {
        Fe<P> X, Y, Z;
        xyzz_to_jacobian(sum, X, Y, Z);
        uint32_t* o = out_xyz + b * 24;
        fe_store(o, X);
        fe_store(o + 8, Y);
        fe_store(o + 16, Z);
    }
}

// The launches, operands in device memory: d_s batch x (n + 2) scratch, d_cu Montgomery, d_pts canonical (taken to Montgomery form
// in place; pts_montgomery: they already are, by the accumulated check that ran before on the same operands, and stay as they
// are), d_scal canonical, d_out 2 x batch Jacobian sums (Montgomery): the right sides, then the left sides.
template <class C>
static int ipa_check_enqueue_t(bzh_ctx* ctx, const bzh_bases* bases, size_t batch, size_t nl, uint32_t* d_s, const uint32_t* d_cu, uint32_t* d_pts,
                               const uint32_t* d_scal, uint32_t* d_out, bool pts_montgomery = false) {
    using SF = typename CurveInfo<C>::SF;
    const size_t n = bases->n - 2, B = batch;
    unsigned k = 0;
    while (((size_t)1 << k) < n) k++;
    hipStream_t st = ctx->stream;
    // right side
    hipLaunchKernelGGL((k_ipa_verify_s<SF>), dim3((unsigned)((n + 2 + 255) / 256), (unsigned)B), dim3(256), 0, st, d_cu, n, k, d_s);
    BZH_HIP_TRY(ctx, hipGetLastError());
    BZH_TRY(msm_run(ctx, bases, d_s, n + 2, B, BZH_FORM_MONTGOMERY, d_out));
    // left side: B independent nl-term sums
    if (!pts_montgomery) BZH_TRY(bases_to_montgomery(ctx, C::id, d_pts, B * nl));
    hipLaunchKernelGGL((k_ipa_small_msm<C>), dim3((unsigned)B), dim3(kSmallMsmThreads), 0, st, d_pts, d_scal, nl, d_out + B * 24);
    BZH_HIP_TRY(ctx, hipGetLastError());
    return BZH_OK;
}
// ... and the comparison on the host: the sums come back and are normalised there
template <class C>
static int ipa_check_run_t(bzh_ctx* ctx, const bzh_bases* bases, size_t batch, size_t nl, uint32_t* d_s, const uint32_t* d_cu, uint32_t* d_pts,
                           const uint32_t* d_scal, uint32_t* d_out, int* ok, bool pts_montgomery = false) {
    using PB = typename C::Base;
    const size_t B = batch;
    BZH_TRY(ipa_check_enqueue_t<C>(ctx, bases, batch, nl, d_s, d_cu, d_pts, d_scal, d_out, pts_montgomery));
    std::vector<uint64_t> jac(2 * B * 12), lhs(B * 8), rhs(B * 8);
    BZH_TRY(d2h_async(ctx, jac.data(), d_out, 2 * B * 96));
    BZH_TRY(d2h_finish(ctx));
    h_jac_to_affine<PB>(jac.data(), B, BZH_FORM_MONTGOMERY, BZH_FORM_CANONICAL, rhs.data());
    h_jac_to_affine<PB>(jac.data() + B * 12, B, BZH_FORM_MONTGOMERY, BZH_FORM_CANONICAL, lhs.data());
    for (size_t b = 0; b < B; b++) ok[b] = memcmp(&lhs[b * 8], &rhs[b * 8], 64) == 0;
    return BZH_OK;
}

// For every opening b:  sum_i lc_scal[b][i] * lc_pts[b][i]  ==  <c_b * s(u_b), G>  ?   (the IPA verification equation with
// everything but the n-term G'_0 moved to the left: L_j, R_j, S, the opened commitment expanded into the proof's own
// commitments, G_0, U, W).  lc_pts: batch x nl affine canonical points ((0,0) = identity padding), lc_scal: canonical.
// Upload, then ipa_check_run_t.
template <class C>
static int ipa_check_batch_t(bzh_ctx* ctx, const bzh_bases* bases, size_t batch, size_t nl, const uint64_t* lc_pts,
                             const uint64_t* lc_scal, const uint64_t* cu /* batch x (k+1) canonical: c, u_j */, int* ok) {
    using SF = typename CurveInfo<C>::SF;
    const size_t n = bases->n - 2, B = batch;
    unsigned k = 0;
    while (((size_t)1 << k) < n) k++;
    if (((size_t)1 << k) != n || !B || !nl) return BZH_E_ARG;
    const size_t na = B * nl;  // every opening's own nl points and scalars, side by side
    const size_t words = B * (n + 2) * 8 + B * (k + 1) * 8 + na * 16 + na * 8 + 2 * B * 24 + 256;
    void* arena = nullptr;
    BZH_TRY(ws_ensure(ctx, WS_IPA, words * 4, &arena));   // held across ipa_check_run_t's MSMs, which take WS_SCRATCH_* only
    uint32_t* d_s = (uint32_t*)arena;
    uint32_t* d_cu = d_s + B * (n + 2) * 8;
    uint32_t* d_pts = d_cu + B * (k + 1) * 8;
    uint32_t* d_scal = d_pts + na * 16;
    uint32_t* d_out = d_scal + na * 8;
    std::vector<Fe<SF>> cum(B * (k + 1));
    for (size_t i = 0; i < cum.size(); i++) cum[i] = fe_to_mont(fe_from_u64<SF>(cu + 4 * i));
    BZH_TRY(h2d_small(ctx, d_cu, cum.data(), cum.size() * 32));
    BZH_TRY(h2d_small(ctx, d_pts, lc_pts, na * 64));
    BZH_TRY(h2d_small(ctx, d_scal, lc_scal, na * 32));
    return ipa_check_run_t<C>(ctx, bases, B, nl, d_s, d_cu, d_pts, d_scal, d_out, ok);
}

int ipa_check_batch(bzh_ctx* ctx, const bzh_bases* bases, size_t batch, size_t nl, const uint64_t* lc_pts, const uint64_t* lc_scal,
                    const uint64_t* cu, int* ok) {
    return with_curve(bases->curve, [&](auto c) { return ipa_check_batch_t<decltype(c)>(ctx, bases, batch, nl, lc_pts, lc_scal, cu, ok); });
}

int ipa_check_batch_device(bzh_ctx* ctx, const bzh_bases* bases, size_t batch, size_t nl, uint32_t* d_pts, const uint32_t* d_scal,
                           const uint32_t* d_cu, int* ok, bool pts_montgomery) {
    const size_t n = bases->n - 2, B = batch;
    unsigned k = 0;
    while (((size_t)1 << k) < n) k++;
    if (((size_t)1 << k) != n || !B || !nl) return BZH_E_ARG;
    void* arena = nullptr;   // WS_IPA: the G'_0 scalars and the two sums per opening, held across MSMs (WS_SCRATCH_* only)
    BZH_TRY(ws_ensure(ctx, WS_IPA, (B * (n + 2) * 8 + 2 * B * 24 + 256) * 4, &arena));
    uint32_t* d_s = (uint32_t*)arena;
    uint32_t* d_out = d_s + B * (n + 2) * 8;
    return with_curve(bases->curve, [&](auto c) {
        return ipa_check_run_t<decltype(c)>(ctx, bases, B, nl, d_s, d_cu, d_pts, d_scal, d_out, ok, pts_montgomery);
    });
}

int ipa_check_sums_device(bzh_ctx* ctx, const bzh_bases* bases, size_t batch, size_t nl, uint32_t* d_pts, const uint32_t* d_scal,
                          const uint32_t* d_cu, const uint32_t** d_sums, bool pts_montgomery) {
    const size_t n = bases->n - 2, B = batch;
    unsigned k = 0;
    while (((size_t)1 << k) < n) k++;
    if (((size_t)1 << k) != n || !B || !nl || !d_sums) return BZH_E_ARG;
    void* arena = nullptr;   // WS_IPA as in ipa_check_batch_device
    BZH_TRY(ws_ensure(ctx, WS_IPA, (B * (n + 2) * 8 + 2 * B * 24 + 256) * 4, &arena));
    uint32_t* d_s = (uint32_t*)arena;
    uint32_t* d_out = d_s + B * (n + 2) * 8;
    *d_sums = d_out;
    return with_curve(bases->curve, [&](auto c) {
        return ipa_check_enqueue_t<decltype(c)>(ctx, bases, B, nl, d_s, d_cu, d_pts, d_scal, d_out, pts_montgomery);
    });
}

// ---------------------------------------------------------------------------
// The accumulated opening check: a random linear combination of the batch's B equations is ONE equation,
//     sum_b w_b * ( sum_i lc_scal[b][i] * lc_pts[b][i] )  ==  < sum_b w_b * c_b * s(u_b) , G >
// so the right side is one n-term MSM against the SRS on a vector a field kernel accumulates, and the left side one Pippenger MSM
// over the B * nl ad-hoc points: no B x n buffer, no per-opening chain of doublings.  An excluded opening (weight 0) contributes
// to neither side.  Workspace (WS_IPA): (n + 2) + B + B * nl scalars and two sums.
// ---------------------------------------------------------------------------
// w'_b = exclude[b] ? 0 : w_b   (Montgomery)
template <class P>
__global__ void __launch_bounds__(256) k_ipa_acc_weights(const uint32_t* __restrict__ w, const uint8_t* __restrict__ exclude, size_t batch,
                                                           uint32_t* __restrict__ wp) {
    const size_t b = blockIdx.x * (size_t)256 + threadIdx.x;
    if (b >= batch) return;
    const bool out = exclude != nullptr && exclude[b] != 0;
    fe_store(wp + b * 8, out ? fe_zero<P>() : fe_load<P>(w + b * 8));
}

// s_acc[i] = sum_b w'_b * c_b * prod_{j : bit (k-1-j) of i} u_(b,j)  for i < n;  s_acc[n] = s_acc[n+1] = 0.
// A workgroup owns 2^ke consecutive i (ke = min(k, 8): 256 of them, or all n below that), one per lane, and walks the batch in
// groups of kAccSGroup proofs.  Bit p of i selects u_(k-1-p); the low ke bits are split into kl = ke / 2 low and km = ke - kl
// middle bits, the bits above ke are the workgroup's own.  Per group, lane (g, x) writes two LDS table entries of proof g:
//   tl[g][x] = the product over the set bits of x among the kl low ones                          (at most kl products)
//   tm[g][x] = w'_b c_b * the workgroup's bits * the set bits of x among the km middle ones     (at most 1 + (k - ke) + km)
// and after a barrier every live lane adds tl[g][lo] * tm[g][mid] for the group's proofs: ONE product per (b, i), plus the
// tables' at most kl + 1 + (k - ke) + km = k + 1 products per lane and group of 16, issued by all 256 lanes whatever ke is.
// Per (b, i) that is 1 + (k + 1) / 16 for k >= 8 (kl = km = 4; 1.9 at k = 14), where walking all k bits per (b, i) costs k / 2.
// For k < 8 the workgroup is the whole vector, kl = k / 2 (2 at k = 5, 3 at k = 6), and only 2^k of the 256 lanes are live in the
// accumulate phase (32 at k = 5): the tables' k + 1 issues per group are then spread over 2^k elements, 1 + (k + 1) * 256 /
// (16 * 2^k) per (b, i) -- 4 at k = 5 -- which at n <= 128 is a one-workgroup kernel of microseconds either way.
// A proof of weight 0 leaves zero tables and its (c, u_j) row is not read; lanes past the batch in the last group likewise.
// Reads d_cu in place, writes (n + 2) * 32 bytes, nothing proportional to B * n.
// gfx950 (Pasta fields): 68 VGPRs, no scratch, 16 KB of LDS; k_ipa_acc_scale 57 VGPRs, k_ipa_acc_result 94, no scratch either.
static constexpr unsigned kAccSGroup = 16, kAccSSlots = 16;
template <class P>
__global__ void __launch_bounds__(256) k_ipa_acc_s(const uint32_t* __restrict__ cu, const uint32_t* __restrict__ wp, size_t batch, size_t n,
                                                     unsigned k, uint32_t* __restrict__ s_acc) {
    __shared__ Fe<P> tl[kAccSGroup][kAccSSlots], tm[kAccSGroup][kAccSSlots];
    const unsigned t = threadIdx.x, ke = k < 8 ? k : 8, kl = ke / 2, km = ke - kl;
    const size_t base = (size_t)blockIdx.x << ke, i = base + t;
    const bool live = t < (1u << ke);   // (the grid is n >> ke workgroups: base + t < n)
    const unsigned lo = t & ((1u << kl) - 1u), mid = (t >> kl) & ((1u << km) - 1u);
    const unsigned g = t / kAccSSlots, x = t % kAccSSlots;
    Fe<P> acc = fe_zero<P>();
    for (size_t b0 = 0; b0 < batch; b0 += kAccSGroup) {
        const size_t b = b0 + g;
        Fe<P> el = fe_zero<P>(), em = fe_zero<P>();
        if (b < batch) {
            const Fe<P> w = fe_load<P>(wp + b * 8);
            if (!fe_is_zero(w)) {
                const uint32_t* row = cu + b * (size_t)(k + 1) * 8;   // [c, u_0 .. u_(k-1)]: bit p of i takes row[k - p]
                if (x < (1u << kl)) {
                    el = fe_one<P>();
                    for (unsigned p = 0; p < kl; p++)
                        if ((x >> p) & 1) el = fe_mul(el, fe_load<P>(row + (size_t)(k - p) * 8));
                }
                if (x < (1u << km)) {
                    em = fe_mul(w, fe_load<P>(row));
                    for (unsigned p = ke; p < k; p++)   // the workgroup's bits: uniform
                        if ((base >> p) & 1) em = fe_mul(em, fe_load<P>(row + (size_t)(k - p) * 8));
                    for (unsigned p = 0; p < km; p++)
                        if ((x >> p) & 1) em = fe_mul(em, fe_load<P>(row + (size_t)(k - kl - p) * 8));
                }
            }
        }
        __syncthreads();   // the previous group's tables have been read
        tl[g][x] = el;
        tm[g][x] = em;
        __syncthreads();
        const unsigned cnt = batch - b0 < kAccSGroup ? (unsigned)(batch - b0) : kAccSGroup;
        if (live)
            for (unsigned q = 0; q < cnt; q++) acc = fe_add(acc, fe_mul(tl[q][lo], tm[q][mid]));
    }
    if (live) fe_store(s_acc + i * 8, acc);
    if (blockIdx.x == 0 && t < 2) fe_store(s_acc + (n + t) * 8, fe_zero<P>());   // no U / W contribution on the right
}

// scal'[b][i] = w'_b * lc_scal[b][i], canonical in and canonical out (a Montgomery factor times a canonical one), the form the
// left side's msm_run is given.  The (0,0) padding of an opening's last slots is kept out of the sum HERE, by a zero scalar -- a
// zero scalar has all-zero digits and k_msm_accumulate files it in no bucket, so the point is never loaded (its own aff_is_id
// test in the saturated loop is a second guard, not what this path relies on); an opening of weight 0 gets zeros without its
// rows being read.
template <class C>
__global__ void __launch_bounds__(256) k_ipa_acc_scale(const uint32_t* __restrict__ pts, const uint32_t* __restrict__ scal,
                                                         const uint32_t* __restrict__ wp, size_t total, size_t nl, uint32_t* __restrict__ out) {
    using P = typename C::Base;
    using SF = typename CurveInfo<C>::SF;
    const size_t e = blockIdx.x * (size_t)256 + threadIdx.x;
    if (e >= total) return;
    const Fe<SF> w = fe_load<SF>(wp + (e / nl) * 8);
    Fe<SF> r = fe_zero<SF>();
    if (!fe_is_zero(w)) {
        Affine<P> q;
        q.x = fe_load<P>(pts + e * 16);
        q.y = fe_load<P>(pts + e * 16 + 8);
        if (!aff_is_id(q)) r = fe_mul(w, fe_load<SF>(scal + e * 8));
    }
    fe_store(out + e * 8, r);
}

// one lane: the right sum (Jacobian, Montgomery) against the left sum (Jacobian, canonical: its MSM ran on canonical scalars), by
// cross-multiplication as k_vr_result compares -- X1 Z2^2 = X2 Z1^2 and Y1 Z2^3 = Y2 Z1^3, or both the identity -- into one byte
template <class C>
__global__ void __launch_bounds__(64) k_ipa_acc_result(const uint32_t* __restrict__ sums, uint8_t* __restrict__ ok) {
    using P = typename C::Base;
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const Fe<P> X1 = fe_load<P>(sums), Y1 = fe_load<P>(sums + 8), Z1 = fe_load<P>(sums + 16);
    const Fe<P> X2 = fe_to_mont(fe_load<P>(sums + 24)), Y2 = fe_to_mont(fe_load<P>(sums + 32)), Z2 = fe_to_mont(fe_load<P>(sums + 40));
    const bool id1 = fe_is_zero(Z1), id2 = fe_is_zero(Z2);
    const Fe<P> z1s = fe_sqr(Z1), z2s = fe_sqr(Z2);
    const bool ex = fe_eq(fe_mul(X1, z2s), fe_mul(X2, z1s));
    const bool ey = fe_eq(fe_mul(Y1, fe_mul(z2s, Z2)), fe_mul(Y2, fe_mul(z1s, Z1)));
    ok[0] = ((id1 && id2) || (!id1 && !id2 && ex && ey)) ? 1 : 0;
}

int ipa_check_accumulated_device(bzh_ctx* ctx, const bzh_bases* bases, size_t batch, size_t nl, uint32_t* d_pts, const uint32_t* d_scal,
                                 const uint32_t* d_cu, const uint32_t* d_weights, const uint8_t* d_exclude, uint8_t* d_ok) {
    const size_t n = bases->n - 2, B = batch, na = B * nl;
    unsigned k = 0;
    while (((size_t)1 << k) < n) k++;
    if (((size_t)1 << k) != n || !B || !nl || !d_weights || !d_ok) return BZH_E_ARG;
    void* arena = nullptr;   // WS_IPA, held across the two MSMs (which take WS_SCRATCH_* only): O(n + B * nl)
    BZH_TRY(ws_ensure(ctx, WS_IPA, ((n + 2) * 8 + B * 8 + na * 8 + 2 * 24 + 64) * 4, &arena));
    uint32_t* d_s = (uint32_t*)arena;
    uint32_t* d_wp = d_s + (n + 2) * 8;
    uint32_t* d_sc = d_wp + B * 8;
    uint32_t* d_sums = d_sc + na * 8;
    return with_curve(bases->curve, [&](auto c) -> int {
        using C = decltype(c);
        using SF = typename CurveInfo<C>::SF;
        hipStream_t st = ctx->stream;
        const unsigned ke = k < 8 ? k : 8;
        hipLaunchKernelGGL((k_ipa_acc_weights<SF>), dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, d_weights, d_exclude, B, d_wp);
        hipLaunchKernelGGL((k_ipa_acc_s<SF>), dim3((unsigned)(n >> ke)), dim3(256), 0, st, d_cu, d_wp, B, n, k, d_s);
        BZH_HIP_TRY(ctx, hipGetLastError());
        BZH_TRY(msm_run(ctx, bases, d_s, n + 2, 1, BZH_FORM_MONTGOMERY, d_sums));
        // left side: one sum over every opening's points, on an ad-hoc table (no window rows, no fe29 copy: the saturated loop,
        // whose xyzz_madd takes P + P and P + (-P) -- points repeat across openings, so both occur)
        BZH_TRY(bases_to_montgomery(ctx, C::id, d_pts, na));
        hipLaunchKernelGGL((k_ipa_acc_scale<C>), dim3((unsigned)((na + 255) / 256)), dim3(256), 0, st, d_pts, d_scal, d_wp, na, nl, d_sc);
        BZH_HIP_TRY(ctx, hipGetLastError());
        bzh_bases tmp;
        tmp.curve = C::id;
        tmp.n = na;
        tmp.d_xy = d_pts;
        tmp.device = ctx->device;
        BZH_TRY(msm_run(ctx, &tmp, d_sc, na, 1, BZH_FORM_CANONICAL, d_sums + 24));
        hipLaunchKernelGGL((k_ipa_acc_result<C>), dim3(1), dim3(64), 0, st, d_sums, d_ok);
        BZH_HIP_TRY(ctx, hipGetLastError());
        return BZH_OK;
    });
}

// the same with its operands in host memory (bzh_ipa_check_accumulated): uploaded as ipa_check_batch_t uploads, weights canonical
int ipa_check_accumulated(bzh_ctx* ctx, const bzh_bases* bases, size_t batch, size_t nl, const uint64_t* lc_pts, const uint64_t* lc_scal,
                          const uint64_t* cu, const uint64_t* weights, const uint8_t* exclude, int* ok) {
    const size_t n = bases->n - 2, B = batch, na = B * nl, Bpad = (B + 15) & ~(size_t)15;
    unsigned k = 0;
    while (((size_t)1 << k) < n) k++;
    if (((size_t)1 << k) != n || !B || !nl) return BZH_E_ARG;
    void* arena = nullptr;   // WS_STAGE: the operands (the leaf holds WS_IPA)
    BZH_TRY(ws_ensure(ctx, WS_STAGE, (B * (k + 1) * 8 + na * 16 + na * 8 + B * 8) * 4 + Bpad + 64, &arena));
    uint32_t* d_cu = (uint32_t*)arena;
    uint32_t* d_pts = d_cu + B * (k + 1) * 8;
    uint32_t* d_scal = d_pts + na * 16;
    uint32_t* d_w = d_scal + na * 8;
    uint8_t* d_ex = (uint8_t*)(d_w + B * 8);
    uint8_t* d_ok = d_ex + Bpad;
    return with_curve(bases->curve, [&](auto c) -> int {
        using SF = typename CurveInfo<decltype(c)>::SF;
        std::vector<Fe<SF>> cum(B * (k + 1)), wm(B);
        for (size_t i = 0; i < cum.size(); i++) cum[i] = fe_to_mont(fe_from_u64<SF>(cu + 4 * i));
        for (size_t b = 0; b < B; b++) wm[b] = fe_to_mont(fe_from_u64<SF>(weights + 4 * b));
        std::vector<uint8_t> ex(Bpad, 0);
        if (exclude) memcpy(ex.data(), exclude, B);
        BZH_TRY(h2d_small(ctx, d_cu, cum.data(), cum.size() * 32));
        BZH_TRY(h2d_small(ctx, d_pts, lc_pts, na * 64));
        BZH_TRY(h2d_small(ctx, d_scal, lc_scal, na * 32));
        BZH_TRY(h2d_small(ctx, d_w, wm.data(), B * 32));
        BZH_TRY(h2d_small(ctx, d_ex, ex.data(), Bpad));
        BZH_TRY(ipa_check_accumulated_device(ctx, bases, B, nl, d_pts, d_scal, d_cu, d_w, exclude ? d_ex : nullptr, d_ok));
        uint8_t out[16] = {0};
        BZH_TRY(d2h_async(ctx, out, d_ok, 16));
        BZH_TRY(d2h_finish(ctx));
        *ok = out[0] ? 1 : 0;
        return BZH_OK;
    });
}


// pasta_curves from_bytes for one compressed point (host): false = not on the curve / non-canonical
bool point_decompress(int curve, const uint8_t* in, uint64_t* xy_canonical) {
    bool ok = false;
    with_curve(curve, [&](auto c) {
        ok = h_decompress<decltype(c)>(in, xy_canonical);
        return BZH_OK;
    });
    return ok;
}

int random_field(bzh_ctx* ctx, int field, const uint32_t* d_raw, size_t count, uint32_t* d_out) {
    if (!count) return BZH_OK;
    const dim3 grid((unsigned)((count + 255) / 256)), block(256);
    BZH_TRY(with_field(field, [&](auto p) {
        hipLaunchKernelGGL((k_reduce_wide<decltype(p)>), grid, block, 0, ctx->stream, d_raw, count, d_out);
        return BZH_OK;
    }));
    BZH_HIP_TRY(ctx, hipGetLastError());
    return BZH_OK;
}

int ipa_open(bzh_ctx* ctx, const bzh_bases* bases, const uint32_t* d_polys, size_t batch, const uint64_t* blinds,
             const uint64_t* x3s, const uint8_t* rng_bytes, size_t rng_stride, bzh_transcript* const* trs, uint64_t* out_v,
             const uint32_t* d_raw_in) {
    return with_curve(bases->curve, [&](auto c) {
        using C = decltype(c);
        IpaHostDriver<C> drv{blinds, x3s, rng_bytes, rng_stride, trs, out_v, d_raw_in};
        return ipa_open_t<C>(ctx, bases, d_polys, batch, drv);
    });
}
int ipa_open_device(bzh_ctx* ctx, const bzh_bases* bases, const uint32_t* d_polys, size_t batch, const uint32_t* d_blinds,
                    const uint32_t* d_x3s, int form, const uint8_t* d_rng, size_t rng_stride, bzh_transcript_batch* tb,
                    uint32_t* d_out_v, uint8_t* d_status) {
    return with_curve(bases->curve, [&](auto c) {
        using C = decltype(c);
        IpaDeviceDriver<C> drv{tb, d_blinds, d_x3s, d_rng, rng_stride, d_out_v, d_status, form};
        return ipa_open_t<C>(ctx, bases, d_polys, batch, drv);
    });
}
int ipa_commit_blinded(bzh_ctx* ctx, const bzh_bases* bases, const uint32_t* d_polys, size_t batch, const uint32_t* d_blinds,
                       uint32_t* d_scalars, uint32_t* d_out_xyz) {
    const size_t n = bases->n - 2;
    BZH_TRY(with_curve(bases->curve, [&](auto c) {
        using SF = typename CurveInfo<decltype(c)>::SF;
        hipLaunchKernelGGL((k_ipa_commit_scalars<SF>), dim3((unsigned)((n + 2 + 255) / 256), (unsigned)batch), dim3(256), 0, ctx->stream, d_polys,
                           d_blinds, n, (size_t)1, d_scalars);
        return BZH_OK;
    }));
    BZH_HIP_TRY(ctx, hipGetLastError());
    return msm_run(ctx, bases, d_scalars, n + 2, batch, BZH_FORM_MONTGOMERY, d_out_xyz);
}
int ipa_verify(bzh_ctx* ctx, const bzh_bases* bases, const uint64_t* commitment_xy, const uint64_t* x3, const uint64_t* v,
               const uint8_t* proof, size_t proof_len, bzh_transcript* tr, const uint64_t* g0_u_w_xy) {
    return with_curve(bases->curve, [&](auto c) {
        return ipa_verify_t<decltype(c)>(ctx, bases, commitment_xy, x3, v, proof, proof_len, tr, g0_u_w_xy);
    });
}

}  // namespace bzh
