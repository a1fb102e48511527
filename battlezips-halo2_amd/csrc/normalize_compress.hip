// Batch normalisation and compression of group elements on the device: pasta_curves' Curve::batch_normalize / to_affine and
// GroupEncoding::to_bytes for the Jacobian points bzh_msm leaves in HBM (bzh_batch_normalize, bzh_affine_compress_batch) -- the
// outbound twin of csrc/sqrt_decompress.hip's from_bytes.
//
// Two kernels around csrc/normalize.hpp -- the functions the host path (ctx == NULL) runs:
//   k_batch_normalize  lane t owns the points t, t + lanes, ... (coalesced, 16-byte moves): the running product of their Z's
//                      forward, ONE fe_inv_ct, and backward zi = 1 / Z, x = X zi^2, y = Y zi^3, the affine point, the 32-byte
//                      encoding and a status byte, each optional.  The running products wait in the output being produced, so a
//                      call needs no buffer besides its outputs.  The shape is normalize_plan's: one point per lane up to
//                      16 384 points, then chains of up to 32.  A launch is at most a few hundred waves on 1 024 SIMDs, so its
//                      time is the length of one lane's chain -- the inversion (330 / 327 products for Fp / Fq, 362 for BN254's
//                      Fq) plus 7 to 9 per chained point -- not throughput.
//   k_affine_compress  one lane per affine point: to canonical form, the parity bit, one 32-byte store.
// 256-thread blocks, no LDS, no scratch; VGPRs from the gfx950 compile are in DESIGN.md section 4.  No loop bound and no branch
// depends on a lane's data but the tail guard.
#include <cstring>
#include <vector>

#include "ctx.hpp"
#include "curve.cuh"
#include "normalize.hpp"

namespace bzh {
namespace {

template <class C>
static __global__ void __launch_bounds__(256) k_batch_normalize(const NormIo io) {
    const size_t t = blockIdx.x * (size_t)256 + threadIdx.x;
    if (t >= io.lanes) return;
    normalize_chain<C>(io, t);
}

// in: n x 16 words x || y in `form`; out: n x 8 words
template <class C>
static __global__ void __launch_bounds__(256) k_affine_compress(const uint32_t* __restrict__ in, size_t n, int canonical,
                                                                uint32_t* __restrict__ out) {
    using PB = typename C::Base;
    const size_t i = blockIdx.x * (size_t)256 + threadIdx.x;
    if (i >= n) return;
    fe_store<PB>(out + i * 8, affine_encode(fe_load<PB>(in + i * 16), fe_load<PB>(in + i * 16 + 8), canonical != 0));
}

static bool valid_form(int f) { return f == BZH_FORM_CANONICAL || f == BZH_FORM_MONTGOMERY; }
static bool valid_mem(int m) { return m == BZH_MEM_HOST || m == BZH_MEM_DEVICE; }
static bool valid_curve(int c) { return c >= BZH_CURVE_VESTA && c <= BZH_CURVE_BN254; }
constexpr size_t kMaxCount = (size_t)1 << 28;   // the byte offsets and the grid stay far inside their types

}  // namespace

// device pointers, 16-byte aligned; enqueues only (declared in ctx.hpp: csrc/transcript_batch.hip's write_jacobian runs it too)
int normalize_run(bzh_ctx* ctx, int curve, const void* d_xyz, size_t n, int form, void* d_out_xy, void* d_out32, uint8_t* d_status) {
    NormIo io{d_xyz, d_out_xy, d_out32, d_status, n, 0, 0, form == BZH_FORM_CANONICAL ? 1 : 0};
    normalize_plan(n, &io.lanes, &io.chain);
    return with_curve(curve, [&](auto c) -> int {
        {
            ScopedTimer t(ctx, BZH_T_POLY);
            hipLaunchKernelGGL(k_batch_normalize<decltype(c)>, dim3((unsigned)((io.lanes + 255) / 256)), dim3(256), 0, ctx->stream, io);
        }
        BZH_HIP_TRY(ctx, hipGetLastError());
        return BZH_OK;
    });
}
namespace {

static int compress_run(bzh_ctx* ctx, int curve, const uint32_t* d_xy, size_t n, int form, uint32_t* d_out32) {
    return with_curve(curve, [&](auto c) -> int {
        {
            ScopedTimer t(ctx, BZH_T_POLY);
            hipLaunchKernelGGL(k_affine_compress<decltype(c)>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_xy, n,
                               form == BZH_FORM_CANONICAL ? 1 : 0, d_out32);
        }
        BZH_HIP_TRY(ctx, hipGetLastError());
        return BZH_OK;
    });
}

}  // namespace
}  // namespace bzh

using namespace bzh;

extern "C" int bzh_batch_normalize_plan(size_t n, size_t* lanes, size_t* chain) {
    if (!lanes || !chain) return BZH_E_ARG;
    normalize_plan(n, lanes, chain);
    return BZH_OK;
}

extern "C" int bzh_batch_normalize(bzh_ctx* ctx, int curve, const uint64_t* xyz, size_t n, int form, int mem, uint64_t* out_xy,
                                   uint8_t* out32, uint8_t* status) {
    if (!valid_curve(curve) || !valid_form(form) || !valid_mem(mem) || n > kMaxCount || (n && (!xyz || (!out_xy && !out32)))) return BZH_E_ARG;
    if (!ctx && mem != BZH_MEM_HOST) return BZH_E_ARG;
    if (mem == BZH_MEM_DEVICE && (((uintptr_t)xyz | (uintptr_t)out_xy | (uintptr_t)out32) & 15)) return BZH_E_ARG;   // the kernel moves 16 bytes at a time
    if (!n) return BZH_OK;
    if (mem == BZH_MEM_HOST && form == BZH_FORM_CANONICAL) {
        // host operands are checked before anything is written; device operands by the kernel, per lane
        const int rc = with_curve(curve, [&](auto c) -> int {
            for (size_t i = 0; i < 3 * n; i++)
                if (!is_canonical(fe_from_u64<typename decltype(c)::Base>(xyz + 4 * i))) return BZH_E_RANGE;
            return BZH_OK;
        });
        if (rc) return rc;
    }
    if (!ctx) {
        NormIo io{xyz, out_xy, out32, status, n, 0, 0, form == BZH_FORM_CANONICAL ? 1 : 0};
        normalize_plan(n, &io.lanes, &io.chain);
        return with_curve(curve, [&](auto c) -> int {
            for (size_t t = 0; t < io.lanes; t++) normalize_chain<decltype(c)>(io, t);
            return BZH_OK;
        });
    }
    std::lock_guard<std::mutex> lk(ctx->mu);
    BZH_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (mem == BZH_MEM_DEVICE && status) return normalize_run(ctx, curve, xyz, n, form, out_xy, out32, status);
    // staged in WS_STAGE: Jacobian points | affine points | encodings | status bytes (the first three only for host buffers);
    // normalize_run takes no workspace slot
    const bool host = mem == BZH_MEM_HOST;
    const size_t ibytes = host ? n * 96 : 0, xbytes = host && out_xy ? n * 64 : 0, ebytes = host && out32 ? n * 32 : 0;
    void* ws = nullptr;
    BZH_TRY(ws_ensure(ctx, WS_STAGE, ibytes + xbytes + ebytes + n + 256, &ws));
    char* const w = (char*)ws;
    const void* d_in = host ? ws : (const void*)xyz;
    void* d_xy = host ? (out_xy ? w + ibytes : nullptr) : (void*)out_xy;
    void* d_e = host ? (out32 ? w + ibytes + xbytes : nullptr) : (void*)out32;
    uint8_t* d_st = (uint8_t*)w + ibytes + xbytes + ebytes;
    if (host) BZH_TRY(h2d_small(ctx, ws, xyz, n * 96));
    BZH_TRY(normalize_run(ctx, curve, d_in, n, form, d_xy, d_e, d_st));
    std::vector<uint8_t> st(n);
    BZH_TRY(d2h_async(ctx, st.data(), d_st, n));
    if (host && out_xy) BZH_TRY(d2h_async(ctx, out_xy, d_xy, n * 64));
    if (host && out32) BZH_TRY(d2h_async(ctx, out32, d_e, n * 32));
    BZH_TRY(d2h_finish(ctx));
    bool any_invalid = false;
    for (size_t i = 0; i < n; i++) any_invalid = any_invalid || st[i] == BZH_POINT_INVALID;
    if (status) memcpy(status, st.data(), n);
    return (status || !any_invalid) ? BZH_OK : BZH_E_RANGE;
}

extern "C" int bzh_affine_compress_batch(bzh_ctx* ctx, int curve, const uint64_t* xy, size_t n, int form, int mem, uint8_t* out32) {
    if (!valid_curve(curve) || !valid_form(form) || !valid_mem(mem) || n > kMaxCount || (n && (!xy || !out32))) return BZH_E_ARG;
    if (!ctx && mem != BZH_MEM_HOST) return BZH_E_ARG;
    if (mem == BZH_MEM_DEVICE && (((uintptr_t)xy | (uintptr_t)out32) & 15)) return BZH_E_ARG;
    if (!n) return BZH_OK;
    if (!ctx) {
        return with_curve(curve, [&](auto c) -> int {
            using P = typename decltype(c)::Base;
            for (size_t i = 0; i < n; i++)
                norm_store<P>(out32 + 32 * i, affine_encode(norm_load<P>(xy + 8 * i), norm_load<P>(xy + 8 * i + 4), form == BZH_FORM_CANONICAL));
            return BZH_OK;
        });
    }
    std::lock_guard<std::mutex> lk(ctx->mu);
    BZH_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (mem == BZH_MEM_DEVICE) return compress_run(ctx, curve, (const uint32_t*)xy, n, form, (uint32_t*)out32);
    void* ws = nullptr;   // WS_STAGE: affine points | encodings (compress_run takes no workspace slot)
    BZH_TRY(ws_ensure(ctx, WS_STAGE, n * 96, &ws));
    uint32_t* d_out = (uint32_t*)((char*)ws + n * 64);
    BZH_TRY(h2d_small(ctx, ws, xy, n * 64));
    BZH_TRY(compress_run(ctx, curve, (const uint32_t*)ws, n, form, d_out));
    BZH_TRY(d2h_async(ctx, out32, d_out, n * 32));
    return d2h_finish(ctx);
}
