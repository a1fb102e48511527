// Batched hash-to-curve: pasta_curves' CurveExt::hash_to_curve(domain_prefix)(msg) for n messages at once, one lane per message
// (bzh_hash_to_curve_batch, bzh_map_to_curve_batch, bzh_params_generators_device; Params::new's g, and pedersen_commit's V and
// R, src/utils/pedersen.rs:19-21).
//
// Two kernels around csrc/hash_to_curve.hpp -- the functions the host path (ctx == NULL) runs:
//   k_hash_to_field  expand_message_xmd over BLAKE2b-512: the block layout is a constant of the launch (H2fPlan, a kernel
//                    argument), the state, the 16 message words and the working vector stay in registers (twelve rounds unrolled,
//                    constant sigma indices), then two OS2IPs of 3 products each.  3 + 2 * ceil((65 + len(dst_prime)) / 128)
//                    compressions for a message that fits the first block (5 for the SRS), 6 products.
//   k_map_to_curve   iso_map(swu(u0) + swu(u1)) with every branch a select: 1 884 products per lane for Fq, 1 896 for Fp (one
//                    inversion for both 1 / ta, ONE root per map, one inversion for the addition and the isogeny together; the
//                    count is itemised in hash_to_curve.hpp).  A launch is a few dozen waves on 1 024 SIMDs, so its time is the
//                    length of that chain, not throughput.
// The map reads u0 || u1 from the slot its point goes to, so a hash needs no buffer besides its output.
// 256-thread blocks, no LDS, no scratch; VGPRs from the gfx950 compile: k_hash_to_field 168, k_map_to_curve 190 (Vesta and
// Pallas alike).  The only data-dependent branch is the tail guard.
#include <cstring>
#include <string>
#include <vector>

#include "blake2b.hpp"
#include "ctx.hpp"
#include "curve.cuh"
#include "hash_to_curve.hpp"

namespace bzh {
namespace {

template <class C>
static __global__ void __launch_bounds__(256) k_hash_to_field(const H2fPlan pl, const uint8_t* __restrict__ msgs, int srs, uint32_t first,
                                                              size_t n, uint32_t* __restrict__ out) {
    using PB = typename C::Base;
    const size_t i = blockIdx.x * (size_t)256 + threadIdx.x;
    if (i >= n) return;
    Fe<PB> u0, u1;
    h2c_hash_to_field<PB>(pl, msgs + i * pl.msg_len, srs != 0, first + (uint32_t)i, u0, u1);
    fe_store<PB>(out + i * 16, u0);
    fe_store<PB>(out + i * 16 + 8, u1);
}

// in: n x 16 words u0 || u1 (may be `out`: a lane reads its own slot before it writes it); out: n x 16 words x || y.
// A u that is not below p gives BZH_POINT_INVALID; zeros unless the status is BZH_POINT_OK.
template <class C>
static __global__ void __launch_bounds__(256) k_map_to_curve(const uint32_t* in, size_t n, int canonical_in, int canonical_out,
                                                             const H2cConsts<typename C::Base> K, const uint32_t* __restrict__ gpow,
                                                             uint32_t* out, uint8_t* __restrict__ status) {
    using PB = typename C::Base;
    const size_t i = blockIdx.x * (size_t)256 + threadIdx.x;
    if (i >= n) return;
    Fe<PB> u0 = fe_load<PB>(in + i * 16), u1 = fe_load<PB>(in + i * 16 + 8);
    const bool valid = fe_lt_p(u0) && fe_lt_p(u1);
    if (canonical_in) u0 = fe_to_mont(u0), u1 = fe_to_mont(u1);
    Fe<PB> x, y;
    const uint8_t st = h2c_map(u0, u1, K, gpow, x, y);
    if (canonical_out) x = fe_from_mont(x), y = fe_from_mont(y);
    const Fe<PB> z = fe_zero<PB>();
    fe_store<PB>(out + i * 16, fe_csel(valid, x, z));
    fe_store<PB>(out + i * 16 + 8, fe_csel(valid, y, z));
    status[i] = valid ? st : (uint8_t)BZH_POINT_INVALID;
}

static bool valid_form(int f) { return f == BZH_FORM_CANONICAL || f == BZH_FORM_MONTGOMERY; }
static bool valid_mem(int m) { return m == BZH_MEM_HOST || m == BZH_MEM_DEVICE; }
constexpr size_t kMaxCount = (size_t)1 << 28;   // 2^28 blocks of 256 lanes stay inside a 32-bit grid

// the launch constants of hash_to_field for messages of msg_len bytes under `dst` (hash_to_curve.hpp states the layout)
static void h2f_plan(const std::string& dst, size_t msg_len, H2fPlan* pl) {
    memset(pl, 0, sizeof(*pl));
    std::vector<uint8_t> dst_prime(dst.begin(), dst.end());
    dst_prime.push_back((uint8_t)dst.size());
    const uint8_t nopersonal[16] = {0};
    Blake2b h;
    h.init(64, nopersonal);
    const uint8_t zpad[128] = {0};
    h.t0 = 128;
    h.compress(zpad, false);
    memcpy(pl->h0, h.h, 64);
    uint8_t* t0 = (uint8_t*)pl->t0;
    t0[msg_len + 1] = 128;   // I2OSP(128, 2) || I2OSP(0, 1)
    memcpy(t0 + msg_len + 3, dst_prime.data(), dst_prime.size());
    memcpy((uint8_t*)pl->t1 + 65, dst_prime.data(), dst_prime.size());
    const size_t r0 = msg_len + 3 + dst_prime.size(), r1 = 65 + dst_prime.size();
    pl->msg_len = (uint32_t)msg_len;
    pl->nb0 = (uint32_t)((r0 + 127) / 128);
    pl->nb1 = (uint32_t)((r1 + 127) / 128);
    pl->len0 = (uint32_t)(128 + r0);
    pl->len1 = (uint32_t)r1;
}
// the ctx's device copy of g^(2^i), i <= S, of one field (shared with csrc/sqrt_decompress.hip through ctx->sqrt_tbl)
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

template <class C>
static int map_launch(bzh_ctx* ctx, const uint32_t* d_in, size_t n, int form_in, int form_out, uint32_t* d_out, uint8_t* d_status) {
    const H2cHost<C>& H = h2c_host<C>();
    if (!H.ok) return BZH_E_HIP;
    const uint32_t* gpow = nullptr;
    BZH_TRY(sqrt_table<typename C::Base>(ctx, &gpow));
    {
        ScopedTimer t(ctx, BZH_T_POLY);
        hipLaunchKernelGGL(k_map_to_curve<C>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_in, n,
                           form_in == BZH_FORM_CANONICAL ? 1 : 0, form_out == BZH_FORM_CANONICAL ? 1 : 0, H.K, gpow, d_out, d_status);
    }
    BZH_HIP_TRY(ctx, hipGetLastError());
    return BZH_OK;
}
template <class C>
static int hash_launch(bzh_ctx* ctx, const H2fPlan& pl, const uint8_t* d_msgs, bool srs, uint32_t first, size_t n, int form,
                       uint32_t* d_out, uint8_t* d_status, hipEvent_t* ev = nullptr) {
    if (ev) (void)hipEventRecord(ev[0], ctx->stream);
    {
        ScopedTimer t(ctx, BZH_T_POLY);
        hipLaunchKernelGGL(k_hash_to_field<C>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, pl, d_msgs, srs ? 1 : 0, first,
                           n, d_out);
    }
    BZH_HIP_TRY(ctx, hipGetLastError());
    if (ev) (void)hipEventRecord(ev[1], ctx->stream);
    const int rc = map_launch<C>(ctx, d_out, n, BZH_FORM_MONTGOMERY, form, d_out, d_status);
    if (ev) (void)hipEventRecord(ev[2], ctx->stream);
    return rc;
}

template <class C>
static uint8_t map_host(const Fe<typename C::Base>& u0, const Fe<typename C::Base>& u1, int form, uint64_t* out_xy) {
    using P = typename C::Base;
    Fe<P> x, y;
    const uint8_t st = h2c_map(u0, u1, h2c_host<C>().K, h_sqrt_table<P>(), x, y);
    if (st != BZH_POINT_OK) {
        memset(out_xy, 0, 64);
        return st;
    }
    fe_to_u64<P>(out_xy, x, form);
    fe_to_u64<P>(out_xy + 4, y, form);
    return st;
}

// What the three entry points share once their arguments are checked.  kind 0: hash n messages at `in`; 1: hash the SRS
// messages first .. first + n; 2: map the n pairs at `in`.  `in` / out_xy / status are in `mem`.
template <class C>
static int run(bzh_ctx* ctx, int kind, const H2fPlan* pl, const void* in, uint32_t first, size_t n, int form, int mem, uint64_t* out_xy,
               uint8_t* status) {
    using P = typename C::Base;
    if (!h2c_host<C>().ok) return BZH_E_HIP;
    const size_t in_bytes = kind == 0 ? n * pl->msg_len : (kind == 2 ? n * 64 : 0);
    bool any_bad = false;
    if (!ctx) {
        std::vector<uint8_t> st(n);
        for (size_t i = 0; i < n; i++) {
            Fe<P> u0, u1;
            if (kind == 2) {
                u0 = fe_from_u64<P>((const uint64_t*)in + 8 * i, form), u1 = fe_from_u64<P>((const uint64_t*)in + 8 * i + 4, form);
            } else {
                h2c_hash_to_field<P>(*pl, kind == 0 ? (const uint8_t*)in + i * pl->msg_len : nullptr, kind == 1, first + (uint32_t)i, u0, u1);
            }
            st[i] = map_host<C>(u0, u1, form, out_xy + 8 * i);
            any_bad = any_bad || st[i] != BZH_POINT_OK;
        }
        if (status) memcpy(status, st.data(), n);
        return (status || !any_bad) ? BZH_OK : BZH_E_RANGE;
    }
    std::lock_guard<std::mutex> lk(ctx->mu);
    BZH_HIP_TRY(ctx, hipSetDevice(ctx->device));
    auto launch = [&](const void* d_in, uint32_t* d_out, uint8_t* d_st) -> int {
        if (kind == 2) return map_launch<C>(ctx, (const uint32_t*)d_in, n, form, form, d_out, d_st);
        return hash_launch<C>(ctx, *pl, (const uint8_t*)d_in, kind == 1, first, n, form, d_out, d_st);
    };
    if (mem == BZH_MEM_DEVICE && status) return launch(in, (uint32_t*)out_xy, status);
    // staged in WS_STAGE: input | affine points | status bytes (the first two only for host buffers); hash_launch takes no
    // workspace slot
    const size_t ibytes = mem == BZH_MEM_HOST ? (in_bytes + 15) & ~(size_t)15 : 0, obytes = mem == BZH_MEM_HOST ? n * 64 : 0;
    void* ws = nullptr;
    BZH_TRY(ws_ensure(ctx, WS_STAGE, ibytes + obytes + n + 256, &ws));
    const void* d_in = mem == BZH_MEM_HOST ? ws : in;
    uint32_t* d_out = mem == BZH_MEM_HOST ? (uint32_t*)((char*)ws + ibytes) : (uint32_t*)out_xy;
    uint8_t* d_st = (uint8_t*)ws + ibytes + obytes;
    if (mem == BZH_MEM_HOST && in_bytes) {
        // the copy kernels move whole words: pad the messages to 16 bytes on the way up
        std::vector<uint8_t> padded(ibytes, 0);
        memcpy(padded.data(), in, in_bytes);
        BZH_TRY(h2d_small(ctx, ws, padded.data(), ibytes));
    }
    BZH_TRY(launch(d_in, d_out, d_st));
    std::vector<uint8_t> st(n);
    BZH_TRY(d2h_async(ctx, st.data(), d_st, n));
    if (mem == BZH_MEM_HOST) BZH_TRY(d2h_async(ctx, out_xy, d_out, n * 64));
    BZH_TRY(d2h_finish(ctx));
    for (size_t i = 0; i < n; i++) any_bad = any_bad || st[i] != BZH_POINT_OK;
    if (status) memcpy(status, st.data(), n);
    return (status || !any_bad) ? BZH_OK : BZH_E_RANGE;
}

}  // namespace

// Params::new's g[first .. first + count) into device memory (Montgomery affine points, 16-byte aligned) and one BZH_POINT_*
// byte each; enqueues only.  The caller holds ctx->mu.
int h2c_generators_run(bzh_ctx* ctx, uint32_t first, size_t count, uint32_t* d_out_xy, uint8_t* d_status, hipEvent_t* ev) {
    if (!count) return BZH_OK;
    H2fPlan pl;
    h2f_plan(h2c_dst<VestaCurve>("Halo2-Parameters"), 5, &pl);
    return hash_launch<VestaCurve>(ctx, pl, nullptr, true, first, count, BZH_FORM_MONTGOMERY, d_out_xy, d_status, ev);
}

}  // namespace bzh

using namespace bzh;

extern "C" int bzh_hash_to_curve_batch(bzh_ctx* ctx, int curve, const char* domain_prefix, const uint8_t* msgs, size_t msg_len, size_t n,
                                       int form, int mem, uint64_t* out_xy, uint8_t* status) {
    if ((curve != BZH_CURVE_VESTA && curve != BZH_CURVE_PALLAS) || !domain_prefix || msg_len > 128 || !valid_form(form) || !valid_mem(mem) ||
        n > kMaxCount || (n && (!out_xy || (!msgs && msg_len))))
        return BZH_E_ARG;
    if (strlen(domain_prefix) + 22 + (curve == BZH_CURVE_PALLAS ? 6 : 5) > 255) return BZH_E_ARG;   // the DST's length is one byte of dst_prime
    if (!ctx && mem != BZH_MEM_HOST) return BZH_E_ARG;
    if (mem == BZH_MEM_DEVICE && (((uintptr_t)msgs | (uintptr_t)out_xy) & 15)) return BZH_E_ARG;   // the kernels move 16 bytes at a time
    if (!n) return BZH_OK;
    return with_pasta_curve(curve, [&](auto c) -> int {
        using C = decltype(c);
        H2fPlan pl;
        h2f_plan(h2c_dst<C>(domain_prefix), msg_len, &pl);
        return run<C>(ctx, 0, &pl, msgs, 0, n, form, mem, out_xy, status);
    });
}

extern "C" int bzh_map_to_curve_batch(bzh_ctx* ctx, int curve, const uint64_t* u01, size_t n, int form, int mem, uint64_t* out_xy,
                                      uint8_t* status) {
    if ((curve != BZH_CURVE_VESTA && curve != BZH_CURVE_PALLAS) || !valid_form(form) || !valid_mem(mem) || n > kMaxCount || (n && (!u01 || !out_xy)))
        return BZH_E_ARG;
    if (!ctx && mem != BZH_MEM_HOST) return BZH_E_ARG;
    if (mem == BZH_MEM_DEVICE && (((uintptr_t)u01 | (uintptr_t)out_xy) & 15)) return BZH_E_ARG;
    if (!n) return BZH_OK;
    return with_pasta_curve(curve, [&](auto c) -> int {
        using C = decltype(c);
        if (mem == BZH_MEM_HOST)   // host operands are checked before anything is written; device operands by the kernel, per lane
            for (size_t i = 0; i < 2 * n; i++)
                if (!is_canonical(fe_from_u64<typename C::Base>(u01 + 4 * i))) return BZH_E_RANGE;
        return run<C>(ctx, 2, nullptr, u01, 0, n, form, mem, out_xy, status);
    });
}

extern "C" int bzh_params_generators_device(bzh_ctx* ctx, size_t first, size_t count, int form, int mem, uint64_t* g_xy) {
    if (!ctx || !valid_form(form) || !valid_mem(mem) || count > kMaxCount || (count && !g_xy)) return BZH_E_ARG;
    if (mem == BZH_MEM_DEVICE && ((uintptr_t)g_xy & 15)) return BZH_E_ARG;
    if (first > ((size_t)1 << 32) || count > ((size_t)1 << 32) - first) return BZH_E_RANGE;   // the message holds the index as a u32
    if (!count) return BZH_OK;
    H2fPlan pl;
    h2f_plan(h2c_dst<VestaCurve>("Halo2-Parameters"), 5, &pl);
    return run<VestaCurve>(ctx, 1, &pl, nullptr, (uint32_t)first, count, form, mem, g_xy, nullptr);
}
