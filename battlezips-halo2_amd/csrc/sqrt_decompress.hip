// Batched field square roots and point decompression: ff::Field::sqrt (bzh_batch_sqrt) and pasta_curves' from_bytes
// (bzh_affine_decompress; Blake2bRead::read_point reads every commitment of a proof through it), one lane per element.
//
// Both kernels run fe_sqrt_ct (csrc/host_field.hpp) -- the function the host path runs -- on field.cuh's saturated product.
// Products per root: Fp 591, Fq 588 (6 for the window table, 219 squarings + 29 / 26 window products for u^((T-1)/2), 2, then
// 16 + 2 * 120 squarings and 79 selected products for the 32-bit logarithm and g^(t/2)); BN254 Fr 555, BN254 Fq 326 (S = 1:
// the exponentiation and one comparison).  A launch is a few dozen waves on 1 024 SIMDs, so its time is the length of that
// chain, not throughput.  Control flow is uniform: no loop bound and no branch but the tail guard depends on a lane's data.
// 256-thread blocks, no LDS, no scratch (k_batch_sqrt 118-122 VGPRs, k_decompress 148-152).
#include <cstring>
#include <vector>

#include "ctx.hpp"
#include "curve.cuh"
#include "host_field.hpp"

namespace bzh {
namespace {

template <class P>
static __global__ void __launch_bounds__(256) k_batch_sqrt(uint32_t* __restrict__ data, size_t n, int canonical,
                                                           const uint32_t* __restrict__ gpow, uint8_t* __restrict__ status) {
    const size_t i = blockIdx.x * (size_t)256 + threadIdx.x;
    if (i >= n) return;
    Fe<P> u = fe_load<P>(data + i * 8);
    if (canonical) u = fe_to_mont(u);
    Fe<P> r;
    const bool ok = fe_sqrt_ct(u, gpow, r);
    if (canonical) r = fe_from_mont(r);
    if (ok) fe_store<P>(data + i * 8, r);   // a non-square is left as it was
    status[i] = ok ? 1 : 0;
}

// in: n x 8 words (x little-endian, bit 255 = parity of y); out: n x 16 words x || y, zeros unless the status is BZH_POINT_OK
template <class C>
static __global__ void __launch_bounds__(256) k_decompress(const uint32_t* __restrict__ in, size_t n, int canonical,
                                                           const uint32_t* __restrict__ gpow, uint32_t* __restrict__ out,
                                                           uint8_t* __restrict__ status) {
    using PB = typename C::Base;
    const size_t i = blockIdx.x * (size_t)256 + threadIdx.x;
    if (i >= n) return;
    Fe<PB> x = fe_load<PB>(in + i * 8);
    const uint32_t ysign = x.l[7] >> 31;
    x.l[7] &= 0x7fffffffu;
    const bool zero = fe_is_zero(x);
    bool below = false;   // x < p, limb by limb from the top
    {
        bool decided = false;
#pragma unroll
        for (int k = 7; k >= 0; k--) {
            const bool ne = x.l[k] != PB::mod(k);
            below = (!decided && ne) ? x.l[k] < PB::mod(k) : below;
            decided = decided || ne;
        }
    }
    // every lane takes the root, whatever its x: the product reduces any 255-bit x times R^2 mod p to a value below p
    const Fe<PB> xm = fe_to_mont(x);
    Fe<PB> y;
    const bool square = fe_sqrt_ct(fe_add(fe_mul(fe_sqr(xm), xm), fe_from_u32<PB>(C::b)), gpow, y);
    const Fe<PB> yneg = fe_neg(y);
    const bool flip = (fe_from_mont(y).l[0] & 1u) != ysign;
    y = fe_csel(flip, yneg, y);
    const bool ok = !zero && below && square;
    const uint8_t st = ok ? BZH_POINT_OK : ((zero && !ysign) ? BZH_POINT_IDENTITY : BZH_POINT_INVALID);
    const Fe<PB> z = fe_zero<PB>();
    fe_store<PB>(out + i * 16, fe_csel(ok, canonical ? x : xm, z));
    fe_store<PB>(out + i * 16 + 8, fe_csel(ok, canonical ? fe_from_mont(y) : y, z));
    status[i] = st;
}

// the ctx's device copy of g^(2^i), i <= S, of one field (h_sqrt_table), uploaded at the first call that needs it
template <class P>
static int sqrt_table(bzh_ctx* ctx, const uint32_t** out) {
    uint32_t*& slot = ctx->sqrt_tbl[FieldInfo<P>::id];
    if (!slot) {
        const size_t bytes = (FieldInfo<P>::S + 1) * 32;
        uint32_t* d = nullptr;
        BZH_HIP_TRY(ctx, hipMalloc((void**)&d, bytes));
        const int rc = h2d_small(ctx, d, h_sqrt_table<P>(), bytes);
        if (rc) {
            (void)hipFree(d);
            return rc;
        }
        slot = d;
    }
    *out = slot;
    return BZH_OK;
}

static bool valid_form(int f) { return f == BZH_FORM_CANONICAL || f == BZH_FORM_MONTGOMERY; }
static bool valid_mem(int m) { return m == BZH_MEM_HOST || m == BZH_MEM_DEVICE; }
constexpr size_t kMaxCount = (size_t)1 << 28;   // 2^28 blocks of 256 lanes stay inside a 32-bit grid

}  // namespace

int batch_sqrt_run(bzh_ctx* ctx, int field, uint32_t* d_data, size_t count, int form, uint8_t* d_status) {
    if (!count) return BZH_OK;
    return with_field(field, [&](auto p) -> int {
        using P = decltype(p);
        const uint32_t* gpow = nullptr;
        BZH_TRY(sqrt_table<P>(ctx, &gpow));
        {
            ScopedTimer t(ctx, BZH_T_POLY);
            hipLaunchKernelGGL(k_batch_sqrt<P>, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, ctx->stream, d_data, count,
                               form == BZH_FORM_CANONICAL ? 1 : 0, gpow, d_status);
        }
        BZH_HIP_TRY(ctx, hipGetLastError());
        return BZH_OK;
    });
}

int decompress_run(bzh_ctx* ctx, int curve, const uint32_t* d_in, size_t n, int form, uint32_t* d_out_xy, uint8_t* d_status) {
    if (!n) return BZH_OK;
    return with_curve(curve, [&](auto c) -> int {
        using C = decltype(c);
        const uint32_t* gpow = nullptr;
        BZH_TRY(sqrt_table<typename C::Base>(ctx, &gpow));
        {
            ScopedTimer t(ctx, BZH_T_POLY);
            hipLaunchKernelGGL(k_decompress<C>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_in, n,
                               form == BZH_FORM_CANONICAL ? 1 : 0, gpow, d_out_xy, d_status);
        }
        BZH_HIP_TRY(ctx, hipGetLastError());
        return BZH_OK;
    });
}

// pasta_curves from_bytes on the host: h_decompress, with the three outcomes told apart
template <class C>
static uint8_t decompress_host(const uint8_t* in, int form, uint64_t* out_xy) {
    using PB = typename C::Base;
    uint64_t xy[8];
    if (!h_decompress<C>(in, xy)) {
        memset(out_xy, 0, 64);
        return BZH_POINT_INVALID;
    }
    uint64_t any = 0;
    for (int i = 0; i < 8; i++) any |= xy[i];
    if (!any) {
        memset(out_xy, 0, 64);
        return BZH_POINT_IDENTITY;
    }
    fe_to_u64<PB>(out_xy, fe_from_u64<PB>(xy, BZH_FORM_CANONICAL), form);
    fe_to_u64<PB>(out_xy + 4, fe_from_u64<PB>(xy + 4, BZH_FORM_CANONICAL), form);
    return BZH_POINT_OK;
}

}  // namespace bzh

using namespace bzh;

extern "C" int bzh_batch_sqrt(bzh_ctx* ctx, int field, uint64_t* data, size_t count, int form, int mem, uint8_t* status) {
    if (field < BZH_FIELD_FP || field > BZH_FIELD_BN254_FQ || !valid_form(form) || !valid_mem(mem) || (!data && count) || count > kMaxCount)
        return BZH_E_ARG;
    if (!ctx && mem != BZH_MEM_HOST) return BZH_E_ARG;
    if (mem == BZH_MEM_DEVICE && ((uintptr_t)data & 15)) return BZH_E_ARG;   // the kernel moves 16 bytes at a time
    if (!count) return BZH_OK;
    bool all_squares = true;
    if (!ctx) {
        return with_field(field, [&](auto p) -> int {
            using P = decltype(p);
            for (size_t i = 0; i < count; i++) {
                Fe<P> r;
                const bool ok = h_sqrt(fe_from_u64<P>(data + 4 * i, form), r);
                if (ok) fe_to_u64<P>(data + 4 * i, r, form);
                if (status) status[i] = ok ? 1 : 0;
                all_squares = all_squares && ok;
            }
            return (status || all_squares) ? BZH_OK : BZH_E_RANGE;
        });
    }
    std::lock_guard<std::mutex> lk(ctx->mu);
    BZH_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (mem == BZH_MEM_DEVICE && status) return batch_sqrt_run(ctx, field, (uint32_t*)data, count, form, status);
    // the statuses come back to the host: staged in WS_STAGE, elements | status bytes (batch_sqrt_run takes no workspace slot)
    const size_t ebytes = mem == BZH_MEM_HOST ? count * 32 : 0;
    void* ws = nullptr;
    BZH_TRY(ws_ensure(ctx, WS_STAGE, ebytes + count + 256, &ws));
    uint32_t* d = mem == BZH_MEM_HOST ? (uint32_t*)ws : (uint32_t*)data;
    uint8_t* d_st = (uint8_t*)ws + ebytes;
    if (mem == BZH_MEM_HOST) BZH_TRY(h2d_small(ctx, d, data, count * 32));
    BZH_TRY(batch_sqrt_run(ctx, field, d, count, form, d_st));
    std::vector<uint8_t> st(count);
    BZH_TRY(d2h_async(ctx, st.data(), d_st, count));
    if (mem == BZH_MEM_HOST) BZH_TRY(d2h_async(ctx, data, d, count * 32));
    BZH_TRY(d2h_finish(ctx));
    for (size_t i = 0; i < count; i++) all_squares = all_squares && st[i];
    if (status) memcpy(status, st.data(), count);
    return (status || all_squares) ? BZH_OK : BZH_E_RANGE;
}

extern "C" int bzh_affine_decompress(bzh_ctx* ctx, int curve, const uint8_t* in32, size_t n, int form, int mem, uint64_t* out_xy,
                                     uint8_t* status) {
    if (curve < BZH_CURVE_VESTA || curve > BZH_CURVE_BN254 || !valid_form(form) || !valid_mem(mem) || ((!in32 || !out_xy) && n) || n > kMaxCount)
        return BZH_E_ARG;
    if (!ctx && mem != BZH_MEM_HOST) return BZH_E_ARG;
    if (mem == BZH_MEM_DEVICE && (((uintptr_t)in32 | (uintptr_t)out_xy) & 15)) return BZH_E_ARG;   // the kernel moves 16 bytes at a time
    if (!n) return BZH_OK;
    bool all_points = true;
    if (!ctx) {
        return with_curve(curve, [&](auto c) -> int {
            for (size_t i = 0; i < n; i++) {
                const uint8_t st = decompress_host<decltype(c)>(in32 + 32 * i, form, out_xy + 8 * i);
                if (status) status[i] = st;
                all_points = all_points && st != BZH_POINT_INVALID;
            }
            return (status || all_points) ? BZH_OK : BZH_E_RANGE;
        });
    }
    std::lock_guard<std::mutex> lk(ctx->mu);
    BZH_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (mem == BZH_MEM_DEVICE && status) return decompress_run(ctx, curve, (const uint32_t*)in32, n, form, (uint32_t*)out_xy, status);
    // staged in WS_STAGE: compressed points | affine points | status bytes (the first two only for host buffers); decompress_run
    // takes no workspace slot
    const size_t ibytes = mem == BZH_MEM_HOST ? n * 32 : 0, obytes = mem == BZH_MEM_HOST ? n * 64 : 0;
    void* ws = nullptr;
    BZH_TRY(ws_ensure(ctx, WS_STAGE, ibytes + obytes + n + 256, &ws));
    const uint32_t* d_in = mem == BZH_MEM_HOST ? (const uint32_t*)ws : (const uint32_t*)in32;
    uint32_t* d_out = mem == BZH_MEM_HOST ? (uint32_t*)((char*)ws + ibytes) : (uint32_t*)out_xy;
    uint8_t* d_st = (uint8_t*)ws + ibytes + obytes;
    if (mem == BZH_MEM_HOST) BZH_TRY(h2d_small(ctx, ws, in32, n * 32));
    BZH_TRY(decompress_run(ctx, curve, d_in, n, form, d_out, d_st));
    std::vector<uint8_t> st(n);
    BZH_TRY(d2h_async(ctx, st.data(), d_st, n));
    if (mem == BZH_MEM_HOST) BZH_TRY(d2h_async(ctx, out_xy, d_out, n * 64));
    BZH_TRY(d2h_finish(ctx));
    for (size_t i = 0; i < n; i++) all_points = all_points && st[i] != BZH_POINT_INVALID;
    if (status) memcpy(status, st.data(), n);
    return (status || all_points) ? BZH_OK : BZH_E_RANGE;
}
