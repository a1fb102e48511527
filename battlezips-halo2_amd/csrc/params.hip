// Params::new(k) for the reference's commitment scheme:
//   let params: Params<vesta::Affine> = Params::new(K);        benches/shot.rs:58, benches/board.rs:51,
//                                                               src/circuits/shot.rs:915, src/circuits/board.rs:907,
//                                                               src/wasm/circuit_wasm.rs:57,97,145,180 (on EVERY call)
// halo2_proofs 0.2.0 `poly::commitment::Params::new` (UPSTREAM, un-vendored) is a pure function of k:
//   g[i]       = hash_to_curve("Halo2-Parameters")(0u8 || i as u32 LE)          i < n = 2^k
//   g_lagrange = inverse group FFT of g (the commitments' Lagrange basis: g_lagrange[i] = sum_j L_i-coefficient_j g[j])
//   w = hash_to_curve(..)([1]),  u = hash_to_curve(..)([2])
// hash_to_curve is pasta_curves 0.4.1's: expand_message_xmd over BLAKE2b, simplified SWU on the 3-isogenous curve,
// the isogeny back (restated from RFC 9380 + Velu's formulas; the same construction on Pallas reproduces the
// reference's two `generator` known answers, src/utils/constants/fixed_bases/board_commit_{v,r}.rs:2941-2948, which
// tests/test_params_cpu.py checks through this very code).
//
// Host C++ for the hashing (setup work, threads over i), device kernels for the group FFT (n/2 log n scalar
// multiplications of points by roots of unity), results cached on disk keyed by (curve, k).
#include <dlfcn.h>
#include <sys/stat.h>
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <cstdio>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "blake2b.hpp"
#include "circuit/hostfield.hpp"
#include "ctx.hpp"
#include "curve.cuh"
#include "hash_to_curve.hpp"
#include "params_file.hpp"

namespace {

using namespace bzh;
using bzc::Fp;
using bzc::Fq;

// ---- hash_to_curve (host) -----------------------------------------------------------------------------------------
// iso-curve y^2 = x^3 + A x + 1265 and the x-coordinate x0 of the isogeny's kernel (the rational root of the
// 3-division polynomial 3x^4 + 6A x^2 + 12B x - A^2); checked at first use: psi3(x0) = 0, the Velu image has j = 0 and
// (1/3)^6 B' = 5.
template <class F>
struct IsoParams;
template <>
struct IsoParams<Fp> {   // Pallas (base field Fp)
    static constexpr uint64_t A[4] = {0x92bb4b0b657a014bull, 0xb74134581a27a59full, 0x49be2d7258370742ull, 0x18354a2eb0ea8c9cull};
    static constexpr uint64_t X0[4] = {0x6a57031b4ba19471ull, 0x4301a71d1ff0c7cdull, 0x52cfc0198fdb5ac3ull, 0x115468c111fb3180ull};
};
template <>
struct IsoParams<Fq> {   // Vesta (base field Fq)
    static constexpr uint64_t A[4] = {0xc515ad7242eaa6b1ull, 0x9673928c7d01b212ull, 0x81639c4d96f78773ull, 0x267f9b2ee592271aull};
    static constexpr uint64_t X0[4] = {0xea8f4dd1286f2e8cull, 0xbf4c98bd6fef5204ull, 0x75d5c33ad251d4a6ull, 0x1ae90dbd54bf6d15ull};
};

template <class F>
struct Iso {
    F a, b, z, x0, t, u, s2, s3;   // SWU Z = -13; Velu constants t, u; scaling s = 1/3
    bool ok = false;
    Iso() {
        F::from_limbs(IsoParams<F>::A, &a);
        F::from_limbs(IsoParams<F>::X0, &x0);
        b = F::from_u64(1265);
        z = -F::from_u64(13);
        const F x0sq = x0.sqr();
        // psi3(x0) = 3 x0^4 + 6 A x0^2 + 12 B x0 - A^2
        const F psi = F::from_u64(3) * x0sq.sqr() + F::from_u64(6) * a * x0sq + F::from_u64(12) * b * x0 - a.sqr();
        const F y0sq = x0sq * x0 + a * x0 + b;
        t = F::from_u64(6) * x0sq + a.dbl();
        u = y0sq.dbl().dbl();
        const F w = u + x0 * t;
        const F a_img = a - F::from_u64(5) * t, b_img = b - F::from_u64(7) * w;
        const F s = F::from_u64(3).inv();
        s2 = s.sqr();
        s3 = s2 * s;
        ok = psi.is_zero() && a_img.is_zero() && (s3.sqr() * b_img == F::from_u64(5));
    }
};
template <class F>
static const Iso<F>& iso() {
    static const Iso<F> v;
    return v;
}

// CurveExt::hash_to_curve(domain_prefix)(message), affine Montgomery: expand_message_xmd streamed over bzh::Blake2b -- a message
// and a prefix of any length, which the batch plan (H2fPlan, csrc/hash_to_curve.hpp) does not take --, then the two stages the
// batch and device paths run: h2f_os2ip and h2c_map with h2c_host's constants.  The caller has checked h2c_host<C>().ok.
// false only for the (never observed) identity result.
template <class C>
static bool hash_to_curve_t(const std::string& domain_prefix, const uint8_t* msg, size_t len, Fe<typename C::Base>* ox, Fe<typename C::Base>* oy) {
    using P = typename C::Base;
    const std::string dst = h2c_dst<C>(domain_prefix.c_str());
    std::vector<uint8_t> dst_prime(dst.begin(), dst.end());
    dst_prime.push_back((uint8_t)dst.size());
    const uint8_t nopersonal[16] = {0};
    uint8_t b0[64];
    uint64_t b1[8], b2[8];   // the digests as their eight little-endian words
    {
        Blake2b h;
        h.init(64, nopersonal);
        const uint8_t zpad[128] = {0};
        h.update(zpad, 128);
        h.update(msg, len);
        const uint8_t lib[3] = {0, 128, 0};
        h.update(lib, 3);
        h.update(dst_prime.data(), dst_prime.size());
        h.finalize(b0);
    }
    {
        Blake2b h;
        h.init(64, nopersonal);
        h.update(b0, 64);
        const uint8_t one = 1;
        h.update(&one, 1);
        h.update(dst_prime.data(), dst_prime.size());
        h.finalize((uint8_t*)b1);
    }
    {
        Blake2b h;
        h.init(64, nopersonal);
        uint8_t x[64];
        for (int i = 0; i < 64; i++) x[i] = b0[i] ^ ((const uint8_t*)b1)[i];
        h.update(x, 64);
        const uint8_t two = 2;
        h.update(&two, 1);
        h.update(dst_prime.data(), dst_prime.size());
        h.finalize((uint8_t*)b2);
    }
    return h2c_map(h2f_os2ip<P>(b1), h2f_os2ip<P>(b2), h2c_host<C>().K, h_sqrt_table<P>(), *ox, *oy) == BZH_POINT_OK;
}
// the same, canonical x || y: BZH_E_RANGE for the identity
template <class C>
static int hash_to_curve_canonical(const std::string& domain_prefix, const uint8_t* msg, size_t len, uint64_t* out_xy) {
    using P = typename C::Base;
    Fe<P> x, y;
    if (!hash_to_curve_t<C>(domain_prefix, msg, len, &x, &y)) return BZH_E_RANGE;
    fe_to_u64<P>(out_xy, x, BZH_FORM_CANONICAL);
    fe_to_u64<P>(out_xy + 4, y, BZH_FORM_CANONICAL);
    return BZH_OK;
}

// ---- group FFT (device) ------------------------------------------------------------------------------------------
template <class C>
__device__ Xyzz<typename C::Base> point_scalar_mul(const Xyzz<typename C::Base>& p, const uint32_t* k /* 8 canonical limbs */) {
    using P = typename C::Base;
    Xyzz<P> acc = xyzz_identity<P>();
    bool started = false;
    for (int bit = 255; bit >= 0; bit--) {
        if (started) acc = xyzz_dbl(acc);
        if ((k[bit >> 5] >> (bit & 31)) & 1u) {
            if (started) xyzz_add(acc, p);
            else acc = p, started = true;
        }
    }
    return acc;
}
template <class P>
__device__ __forceinline__ Xyzz<P> xyzz_ld(const uint32_t* a) {
    Xyzz<P> v;
    v.x = fe_load<P>(a), v.y = fe_load<P>(a + 8), v.zz = fe_load<P>(a + 16), v.zzz = fe_load<P>(a + 24);
    return v;
}
template <class P>
__device__ __forceinline__ void xyzz_st(uint32_t* a, const Xyzz<P>& v) {
    fe_store(a, v.x), fe_store(a + 8, v.y), fe_store(a + 16, v.zz), fe_store(a + 24, v.zzz);
}
// out[bitrev(i)] = g[i] (affine Montgomery -> XYZZ)
template <class C>
__global__ void __launch_bounds__(256) k_gfft_load(const uint32_t* __restrict__ g_xy, uint32_t* __restrict__ work, unsigned log_n) {
    using P = typename C::Base;
    const size_t i = blockIdx.x * (size_t)256 + threadIdx.x, n = (size_t)1 << log_n;
    if (i >= n) return;
    const size_t r = log_n ? (size_t)(__brevll((unsigned long long)i) >> (64 - log_n)) : 0;
    Affine<P> a;
    a.x = fe_load<P>(g_xy + i * 16), a.y = fe_load<P>(g_xy + i * 16 + 8);
    xyzz_st<P>(work + r * 32, xyzz_from_affine(a));
}
// one radix-2 decimation-in-time stage: butterflies (i0, i0 + m), twiddle tw[j * stride] (canonical limbs)
template <class C>
__global__ void __launch_bounds__(64) k_gfft_stage(uint32_t* __restrict__ work, size_t n, size_t m, const uint32_t* __restrict__ tw, size_t stride) {
    using P = typename C::Base;
    const size_t idx = blockIdx.x * (size_t)64 + threadIdx.x;
    if (idx >= n / 2) return;
    const size_t grp = idx / m, j = idx - grp * m, i0 = grp * 2 * m + j, i1 = i0 + m;
    const Xyzz<P> a = xyzz_ld<P>(work + i0 * 32);
    Xyzz<P> t = xyzz_ld<P>(work + i1 * 32);
    if (j) t = point_scalar_mul<C>(t, tw + j * stride * 8);
    Xyzz<P> s = a, d = a;
    xyzz_add(s, t);
    Xyzz<P> nt = t;
    nt.y = fe_neg(t.y);
    xyzz_add(d, nt);
    xyzz_st<P>(work + i0 * 32, s);
    xyzz_st<P>(work + i1 * 32, d);
}
// out_xy[i] = affine([scale] work[i])
template <class C>
__global__ void __launch_bounds__(64) k_gfft_finish(const uint32_t* __restrict__ work, size_t n, const uint32_t* __restrict__ scale,
                                                     uint32_t* __restrict__ out_xy) {
    using P = typename C::Base;
    const size_t i = blockIdx.x * (size_t)64 + threadIdx.x;
    if (i >= n) return;
    const Xyzz<P> v = point_scalar_mul<C>(xyzz_ld<P>(work + i * 32), scale);
    const Affine<P> a = xyzz_to_affine(v);
    fe_store(out_xy + i * 16, a.x);
    fe_store(out_xy + i * 16 + 8, a.y);
}

static std::string default_cache_dir() {
    const char* env = getenv("BZH_CACHE_DIR");
    if (env && *env) return env;
    Dl_info info;
    if (dladdr((void*)&default_cache_dir, &info) && info.dli_fname) {
        std::string p = info.dli_fname;
        const size_t s = p.rfind('/');
        return (s == std::string::npos ? std::string(".") : p.substr(0, s)) + "/.bzh2_cache";
    }
    return ".bzh2_cache";
}

}  // namespace

namespace bzh {
// the iso-curve and isogeny constants of hash_to_curve for csrc/hash_to_curve.hip, canonical limbs: A, B, Z, x0, t, u, 1/9, 1/27;
// BZH_E_HIP if Iso<F>'s self-check fails
template <class F>
static int iso_constants_t(uint64_t out[8][4]) {
    const Iso<F>& I = iso<F>();
    if (!I.ok) return BZH_E_HIP;
    const F* v[8] = {&I.a, &I.b, &I.z, &I.x0, &I.t, &I.u, &I.s2, &I.s3};
    for (int i = 0; i < 8; i++) v[i]->to_limbs(out[i]);
    return BZH_OK;
}
int h2c_iso_constants(int curve, uint64_t out[8][4]) {
    if (curve == BZH_CURVE_PALLAS) return iso_constants_t<Fp>(out);
    if (curve == BZH_CURVE_VESTA) return iso_constants_t<Fq>(out);
    return BZH_E_ARG;
}
}  // namespace bzh

struct bzh_params {
    unsigned k = 0;
    size_t n = 0;
    std::vector<uint64_t> g, g_lagrange;   // n x 8 canonical limbs (x || y)
    uint64_t w[8], u[8];
    bzh_bases *bases = nullptr, *bases_lagrange = nullptr;   // (g | u | w) and (g_lagrange | u | w), window tables
    bool from_cache = false;
};

// the inverse group FFT of the n = 2^k Montgomery affine points at d_g (device memory, left as it is) into the host array out_xy
// (n x 8 canonical limbs); returns once out_xy is written.  The caller holds ctx->mu.
static int group_ifft_device(bzh_ctx* ctx, const uint32_t* d_g, unsigned k, uint64_t* out_xy) {
    using C = VestaCurve;
    const size_t n = (size_t)1 << k;
    // twiddles omega^-j (j < n / 2) and the scale n^-1, canonical, computed on the host in the scalar field (Fp)
    uint64_t wl[4];
    int rc = bzh_field_omega(BZH_FIELD_FP, k, BZH_FORM_CANONICAL, wl);
    if (rc) return rc;
    Fp omega, pw = Fp::one();
    Fp::from_limbs(wl, &omega);
    const Fp omega_inv = omega.inv();
    std::vector<uint64_t> tw(std::max<size_t>(n / 2, 1) * 4 + 4);
    for (size_t j = 0; j < n / 2; j++) {
        pw.to_limbs(&tw[4 * j]);
        pw = pw * omega_inv;
    }
    Fp::from_u64((uint64_t)n).inv().to_limbs(&tw[std::max<size_t>(n / 2, 1) * 4]);
    uint32_t *d_work = nullptr, *d_tw = nullptr, *d_out = nullptr;
    auto cleanup = [&] {
        if (d_work) (void)hipFree(d_work);
        if (d_tw) (void)hipFree(d_tw);
        if (d_out) (void)hipFree(d_out);
    };
    hipError_t e = hipMalloc((void**)&d_work, n * 128);
    if (e == hipSuccess) e = hipMalloc((void**)&d_tw, tw.size() * 8);
    if (e == hipSuccess) e = hipMalloc((void**)&d_out, n * 64);
    if (e != hipSuccess) {
        cleanup();
        return BZH_E_OOM;
    }
    e = hipMemcpyAsync(d_tw, tw.data(), tw.size() * 8, hipMemcpyHostToDevice, ctx->stream);
    if (e != hipSuccess) {
        cleanup();
        return BZH_E_HIP;
    }
    hipLaunchKernelGGL((k_gfft_load<C>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_g, d_work, k);
    for (size_t m = 1; m < n; m <<= 1) {
        const size_t stride = n / (2 * m);
        hipLaunchKernelGGL((k_gfft_stage<C>), dim3((unsigned)((n / 2 + 63) / 64)), dim3(64), 0, ctx->stream, d_work, n, m, d_tw, stride);
    }
    hipLaunchKernelGGL((k_gfft_finish<C>), dim3((unsigned)((n + 63) / 64)), dim3(64), 0, ctx->stream, d_work, n,
                       d_tw + std::max<size_t>(n / 2, 1) * 8, d_out);
    e = hipGetLastError();
    if (e == hipSuccess) {
        rc = field_convert(ctx, BZH_FIELD_FQ, d_out, n * 2, 0);   // coordinates: Montgomery -> canonical
        if (rc) {
            (void)hipStreamSynchronize(ctx->stream);
            cleanup();
            return rc;
        }
        e = hipMemcpyAsync(out_xy, d_out, n * 64, hipMemcpyDeviceToHost, ctx->stream);
    }
    const hipError_t es = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = es;
    cleanup();
    if (e != hipSuccess) {
        ctx->last_error = std::string("bzh_group_ifft: ") + hipGetErrorString(e);
        return BZH_E_HIP;
    }
    return BZH_OK;
}

// Params::new's g, w, u with g made on the device (csrc/hash_to_curve.hip) and handed to the group FFT where it lies; g comes
// to the host once, after the FFT has read it.  Fills p->g, p->g_lagrange, p->w, p->u (canonical).
static int params_generate_device(bzh_ctx* ctx, bzh_params* p, bool trace) {
    const size_t n = p->n;
    uint64_t wu[16];
    const uint8_t msgs[2] = {1, 2};
    BZH_TRY(bzh_hash_to_curve_batch(nullptr, BZH_CURVE_VESTA, "Halo2-Parameters", msgs, 1, 2, BZH_FORM_CANONICAL, BZH_MEM_HOST, wu, nullptr));
    memcpy(p->w, wu, 64);
    memcpy(p->u, wu + 8, 64);
    std::lock_guard<std::mutex> lk(ctx->mu);
    BZH_HIP_TRY(ctx, hipSetDevice(ctx->device));
    uint32_t* d_g = nullptr;
    uint8_t* d_st = nullptr;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    auto cleanup = [&] {
        (void)hipStreamSynchronize(ctx->stream);
        if (d_g) (void)hipFree(d_g);
        if (d_st) (void)hipFree(d_st);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    };
    if (hipMalloc((void**)&d_g, n * 64) != hipSuccess || hipMalloc((void**)&d_st, (n + 15) & ~(size_t)15) != hipSuccess) {
        cleanup();
        return BZH_E_OOM;
    }
    if (trace)
        for (hipEvent_t& e : ev)
            if (hipEventCreate(&e) != hipSuccess) e = nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    int rc = h2c_generators_run(ctx, 0, n, d_g, d_st, (ev[0] && ev[1] && ev[2]) ? ev : nullptr);
    std::vector<uint8_t> st(n);
    if (!rc && hipMemcpyAsync(st.data(), d_st, n, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) rc = BZH_E_HIP;
    if (!rc && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = BZH_E_HIP;
    for (size_t i = 0; !rc && i < n; i++)
        if (st[i] != BZH_POINT_OK) rc = BZH_E_RANGE;
    if (!rc && trace) {
        float hf = 0, mc = 0;
        if (ev[0] && ev[1] && ev[2]) (void)hipEventElapsedTime(&hf, ev[0], ev[1]), (void)hipEventElapsedTime(&mc, ev[1], ev[2]);
        fprintf(stderr, "[bzh_params_create] %-22s %8.3f ms\n", "pg:k_hash_to_field", hf);
        fprintf(stderr, "[bzh_params_create] %-22s %8.3f ms\n", "pg:k_map_to_curve", mc);
        fprintf(stderr, "[bzh_params_create] %-22s %8.3f ms\n", "generators",
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    const auto t1 = std::chrono::steady_clock::now();
    if (!rc) rc = group_ifft_device(ctx, d_g, p->k, p->g_lagrange.data());
    if (!rc) rc = field_convert(ctx, BZH_FIELD_FQ, d_g, n * 2, 0);   // the FFT has read g: Montgomery -> canonical in place
    if (!rc && hipMemcpyAsync(p->g.data(), d_g, n * 64, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) rc = BZH_E_HIP;
    if (!rc && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = BZH_E_HIP;
    if (!rc && trace)
        fprintf(stderr, "[bzh_params_create] %-22s %8.3f ms\n", "group_fft",
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count());
    cleanup();
    return rc;
}

// ---- Params files (include/bzh2.h; the byte layout: csrc/params_file.hpp) ---------------------------------------------
// a table bzh_params_read made: the caller holds ctx->mu and has waited for the stream
static void params_table_release(bzh_bases* b) {
    if (!b) return;
    if (b->d_xy) (void)hipFree(b->d_xy);
    if (b->d_xy29) (void)hipFree(b->d_xy29);
    delete b;
}

// bzh_params_read between the argument checks and the hand-over: p has k, n and its host arrays sized; the caller holds ctx->mu.
// Fills p's two tables and host copies and *v.  On any failure the caller waits for the stream and releases what p holds.
static int params_read_locked(bzh_ctx* ctx, const uint8_t* bytes, size_t len, int window_bits, int check, bzh_params* p, bzh_params_verdict* v) {
    const size_t n = p->n, lanes = pf_points(n);
    const bool lagrange = check >= BZH_PARAMS_CHECK_LAGRANGE, full = check == BZH_PARAMS_CHECK_FULL;
    // what the host contributes, behind the strings in the one upload: the ChaCha key of r, then Params::new's w and u (Montgomery)
    uint32_t tail[8 + 32] = {0};
    if (lagrange) {
        const uint8_t personal[16] = {'b', 'z', 'h', '2', '-', 'p', 'a', 'r', 'a', 'm', 's', '-', 'f', 'i', 'l', 'e'};
        uint8_t digest[64];
        Blake2b h;
        h.init(64, personal);
        h.update(bytes, len);
        h.finalize(digest);
        memcpy(tail, digest, 32);
    }
    if (full) {
        const uint8_t msgs[2] = {1, 2};
        uint64_t wu[16];
        BZH_TRY(bzh_hash_to_curve_batch(nullptr, BZH_CURVE_VESTA, "Halo2-Parameters", msgs, 1, 2, BZH_FORM_MONTGOMERY, BZH_MEM_HOST, wu, nullptr));
        memcpy(tail + 8, wu, 128);
    }
    // WS_STAGE (no driver below takes it): accumulators | verdict | the two sums | strings, key, w, u | decoded points | status bytes
    // | the draws, r, intt(r) | the regenerated g and its status bytes
    auto pad = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t in_bytes = lanes * kPfPointBytes + sizeof(tail);
    const size_t o_verdict = 256, o_sums = 512, o_in = 768, o_pts = o_in + pad(in_bytes), o_st = o_pts + lanes * 64, o_raw = o_st + pad(lanes),
                 o_r = o_raw + (lagrange ? n * 64 : 0), o_ir = o_r + (lagrange ? n * 32 : 0), o_gen = o_ir + (lagrange ? n * 32 : 0),
                 o_gst = o_gen + (full ? n * 64 : 0), total = o_gst + (full ? pad(n) : 0);
    if (in_bytes > ((size_t)1 << 20)) BZH_TRY(pin_big_reserve(ctx, pad(in_bytes) + 2 * pad(n * 64) + 4096));   // the upload and the host copies: no recycling in between
    void* ws = nullptr;
    BZH_TRY(ws_ensure(ctx, WS_STAGE, total, &ws));
    auto at = [&](size_t o) { return (uint32_t*)((char*)ws + o); };
    uint32_t *d_in = at(o_in), *d_pts = at(o_pts), *d_sums = at(o_sums), *d_key = d_in + lanes * 8, *d_wu = d_key + 8;
    uint8_t* d_st = (uint8_t*)at(o_st);
    char* slot = nullptr;
    BZH_TRY(h2d_stage(ctx, in_bytes, &slot));
    memcpy(slot, bytes + kPfHeaderBytes, lanes * kPfPointBytes);
    memcpy(slot + lanes * kPfPointBytes, tail, sizeof(tail));
    BZH_TRY(h2d_commit(ctx, d_in, slot, in_bytes));
    BZH_TRY(decompress_run(ctx, BZH_CURVE_VESTA, d_in, lanes, BZH_FORM_MONTGOMERY, d_pts, d_st));
    // (g | u | w) and (g_lagrange | u | w | g_0), as bzh_params_create lays them out, from the decoded points where they lie
    auto section = [&](int s) { return d_pts + pf_first_lane(s, n) * 16; };
    for (int which = 0; which < 2; which++) {
        bzh_bases* b = new (std::nothrow) bzh_bases();
        if (!b) return BZH_E_OOM;
        (which ? p->bases_lagrange : p->bases) = b;
        b->curve = BZH_CURVE_VESTA;
        b->n = n + 2 + (which ? 1 : 0);
        b->device = ctx->device;
        if (hipMalloc((void**)&b->d_xy, b->n * 64) != hipSuccess) return BZH_E_OOM;
        BZH_TRY(xfer_launch(ctx, b->d_xy, section(which ? PF_G_LAGRANGE : PF_G), n * 64, hipMemcpyDeviceToDevice));
        BZH_TRY(xfer_launch(ctx, b->d_xy + n * 16, section(PF_U), 64, hipMemcpyDeviceToDevice));
        BZH_TRY(xfer_launch(ctx, b->d_xy + (n + 1) * 16, section(PF_W), 64, hipMemcpyDeviceToDevice));
        if (which) BZH_TRY(xfer_launch(ctx, b->d_xy + (n + 2) * 16, section(PF_G), 64, hipMemcpyDeviceToDevice));
        BZH_TRY(bases_precompute(ctx, b, window_bits));
    }
    PfVerdictArgs va;
    va.d_status = d_st, va.d_points = d_pts, va.d_acc = at(0), va.d_verdict = at(o_verdict), va.n = (uint32_t)n;
    if (lagrange) {
        // sum_j r_j g_lagrange[j] against sum_i intt(r)_i g[i]: the matrix of the inverse group FFT is symmetric
        uint32_t *d_raw = at(o_raw), *d_r = at(o_r), *d_ir = at(o_ir);
        BZH_TRY(rng_rows_device(ctx, d_key, 0, n, 1, d_raw));
        BZH_TRY(random_field(ctx, BZH_FIELD_FP, d_raw, n, d_r));
        BZH_TRY(xfer_launch(ctx, d_ir, d_r, n * 32, hipMemcpyDeviceToDevice));
        uint64_t omega[4];
        BZH_TRY(bzh_field_omega(BZH_FIELD_FP, p->k, BZH_FORM_MONTGOMERY, omega));
        BZH_TRY(ntt_run(ctx, BZH_FIELD_FP, d_ir, p->k, 1, omega, nullptr, 1, BZH_FORM_MONTGOMERY));
        BZH_TRY(msm_run(ctx, p->bases_lagrange, d_r, n, 1, BZH_FORM_MONTGOMERY, d_sums));
        BZH_TRY(msm_run(ctx, p->bases, d_ir, n, 1, BZH_FORM_MONTGOMERY, d_sums + 24));
        va.d_sums = d_sums;
    }
    if (full) {
        BZH_TRY(h2c_generators_run(ctx, 0, n, at(o_gen), (uint8_t*)at(o_gst)));
        va.d_gen = at(o_gen), va.d_gen_status = (const uint8_t*)at(o_gst), va.d_wu = d_wu;
    }
    BZH_TRY(params_file_verdict_run(ctx, va));
    // behind the verdict: the host copies bzh_params_points serves, canonical
    BZH_TRY(field_convert(ctx, BZH_FIELD_FQ, d_pts, lanes * 2, 0));
    BZH_TRY(d2h_async(ctx, v, va.d_verdict, sizeof(*v)));
    BZH_TRY(d2h_async(ctx, p->g.data(), section(PF_G), n * 64));
    BZH_TRY(d2h_async(ctx, p->g_lagrange.data(), section(PF_G_LAGRANGE), n * 64));
    BZH_TRY(d2h_async(ctx, p->w, section(PF_W), 64));
    BZH_TRY(d2h_async(ctx, p->u, section(PF_U), 64));
    BZH_TRY(d2h_finish(ctx));
    if (v->bits) {
        static const char* const names[kPfSections] = {"g", "g_lagrange", "w", "u"};
        char msg[224];
        if (v->bits == BZH_PARAMS_BAD_LAGRANGE)
            snprintf(msg, sizeof(msg), "bzh_params_read: refused (bits %u): g_lagrange is not the inverse group FFT of g", v->bits);
        else
            snprintf(msg, sizeof(msg), "bzh_params_read: refused (bits %u): %s[%u] %s, the first of %u such points%s", v->bits,
                     names[v->section & 3], v->first_bad, (v->bits & BZH_PARAMS_BAD_DECODE) ? "does not decode to a point of the curve" : "is not Params::new's",
                     v->n_bad, (v->bits & BZH_PARAMS_BAD_LAGRANGE) ? "; g_lagrange is not the inverse group FFT of g" : "");
        ctx->last_error = msg;
        return BZH_E_RANGE;
    }
    return BZH_OK;
}

extern "C" {

int bzh_params_read(bzh_ctx* ctx, const uint8_t* bytes, size_t len, int window_bits, int check, bzh_params** out, bzh_params_verdict* verdict) {
    if (out) *out = nullptr;
    if (verdict) memset(verdict, 0, sizeof(*verdict));
    if (!ctx || !bytes || !out || window_bits < 0 || check < BZH_PARAMS_CHECK_POINTS || check > BZH_PARAMS_CHECK_FULL) return BZH_E_ARG;
    unsigned k = 0;
    BZH_TRY(bzh_params_file_info(bytes, len, &k, nullptr));
    if (k < 1) return BZH_E_ARG;
    if (check == BZH_PARAMS_CHECK_FULL && !h2c_host<VestaCurve>().ok) return BZH_E_HIP;
    std::unique_ptr<bzh_params> p(new bzh_params());
    p->k = k;
    p->n = (size_t)1 << k;
    p->g.assign(p->n * 8, 0);
    p->g_lagrange.assign(p->n * 8, 0);
    bzh_params_verdict v = {0, 0, 0, 0};
    std::lock_guard<std::mutex> lk(ctx->mu);
    BZH_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int rc = params_read_locked(ctx, bytes, len, window_bits, check, p.get(), &v);
    if (verdict) *verdict = v;
    if (rc) {
        (void)pin_drain(ctx);   // nothing queued reads the tables or writes p's arrays any more
        params_table_release(p->bases);
        params_table_release(p->bases_lagrange);
        return rc;
    }
    *out = p.release();
    return BZH_OK;
}

int bzh_params_write(bzh_ctx* ctx, const bzh_params* p, uint8_t* out, size_t cap, size_t* len) {
    if (!p || !len) return BZH_E_ARG;
    const size_t n = p->n, need = pf_file_bytes(n);
    *len = need;
    if (!out) return BZH_OK;   // the size query
    if (!ctx || cap < need) return BZH_E_ARG;
    for (int b = 0; b < 4; b++) out[b] = (uint8_t)(p->k >> (8 * b));
    const uint64_t* src[kPfSections] = {p->g.data(), p->g_lagrange.data(), p->w, p->u};   // by section code
    for (int s = 0; s < kPfSections; s++)
        BZH_TRY(bzh_affine_compress_batch(ctx, BZH_CURVE_VESTA, src[s], pf_section_len(s, n), BZH_FORM_CANONICAL, BZH_MEM_HOST, out + pf_offset(s, 0, n)));
    return BZH_OK;
}

int bzh_hash_to_curve(int curve, const char* domain_prefix, const uint8_t* msg, size_t len, uint64_t* out_xy) {
    if (!domain_prefix || (!msg && len) || !out_xy) return BZH_E_ARG;
    return with_pasta_curve(curve, [&](auto c) -> int {
        using C = decltype(c);
        if (!h2c_host<C>().ok) return BZH_E_HIP;
        return hash_to_curve_canonical<C>(domain_prefix, msg, len, out_xy);
    });
}

// g, w, u of Params::new(k) on the host (no device): g_xy = n x 8 canonical limbs
int bzh_params_generators(unsigned k, uint64_t* g_xy, uint64_t* w_xy, uint64_t* u_xy, unsigned threads) {
    if (k > 24 || (!g_xy && !w_xy && !u_xy)) return BZH_E_ARG;
    if (!h2c_host<VestaCurve>().ok) return BZH_E_HIP;
    const size_t n = (size_t)1 << k;
    const std::string domain = "Halo2-Parameters";
    std::atomic<int> bad{0};
    if (g_xy) {
        if (!threads) threads = std::max(1u, std::min(32u, host_thread_budget()));
        threads = (unsigned)std::min<size_t>(threads, n);
        std::atomic<size_t> next{0};
        auto work = [&] {
            for (;;) {
                const size_t lo = next.fetch_add(256);
                if (lo >= n) return;
                for (size_t i = lo; i < std::min(n, lo + 256); i++) {
                    const uint8_t msg[5] = {0, (uint8_t)i, (uint8_t)(i >> 8), (uint8_t)(i >> 16), (uint8_t)(i >> 24)};
                    if (hash_to_curve_canonical<VestaCurve>(domain, msg, 5, g_xy + 8 * i)) bad = 1;
                }
            }
        };
        std::vector<std::thread> pool;
        for (unsigned t = 1; t < threads; t++) pool.emplace_back(work);
        work();
        for (auto& t : pool) t.join();
    }
    for (int which = 1; which <= 2; which++) {
        uint64_t* out = which == 1 ? w_xy : u_xy;
        if (!out) continue;
        const uint8_t msg[1] = {(uint8_t)which};
        BZH_TRY(hash_to_curve_canonical<VestaCurve>(domain, msg, 1, out));
    }
    return bad ? BZH_E_RANGE : BZH_OK;
}

// g_lagrange = inverse group FFT of g, on the device: g_xy / out_xy host arrays of n x 8 canonical limbs
int bzh_group_ifft(bzh_ctx* ctx, int curve, const uint64_t* g_xy, unsigned k, uint64_t* out_xy) {
    if (!ctx || !g_xy || !out_xy || curve != BZH_CURVE_VESTA || k > 24) return BZH_E_ARG;
    const size_t n = (size_t)1 << k;
    std::lock_guard<std::mutex> lk(ctx->mu);
    BZH_HIP_TRY(ctx, hipSetDevice(ctx->device));
    uint32_t* d_g = nullptr;
    if (hipMalloc((void**)&d_g, n * 64) != hipSuccess) return BZH_E_OOM;
    int rc = hipMemcpyAsync(d_g, g_xy, n * 64, hipMemcpyHostToDevice, ctx->stream) == hipSuccess ? BZH_OK : BZH_E_HIP;
    if (!rc) rc = bases_to_montgomery(ctx, curve, d_g, n);
    if (!rc) rc = group_ifft_device(ctx, d_g, k, out_xy);
    if (rc) (void)hipStreamSynchronize(ctx->stream);   // a failed call may have left work that reads d_g
    (void)hipFree(d_g);
    return rc;
}

int bzh_params_free(bzh_ctx* ctx, bzh_params* p) {
    if (!p) return BZH_OK;
    if (ctx) {
        if (p->bases) bzh_bases_free(ctx, p->bases);
        if (p->bases_lagrange) bzh_bases_free(ctx, p->bases_lagrange);
    }
    delete p;
    return BZH_OK;
}

// Params::new(k), cached under cache_dir (NULL: next to the library, or $BZH_CACHE_DIR; "" disables the cache);
// uploads (g | u | w) and (g_lagrange | u | w) with window tables of `window_bits` (0: the planner's).
// generators_where picks who makes g on a cache miss: BZH_GENERATORS_HOST (bzh_params_generators, host threads) or
// BZH_GENERATORS_DEVICE (csrc/hash_to_curve.hip; g goes to the group FFT without a host round trip).  Same points, same cache file.
int bzh_params_create(bzh_ctx* ctx, unsigned k, const char* cache_dir, int window_bits, bzh_params** out) {
    return bzh_params_create_with(ctx, k, cache_dir, window_bits, BZH_GENERATORS_HOST, out);
}
int bzh_params_create_with(bzh_ctx* ctx, unsigned k, const char* cache_dir, int window_bits, int generators_where, bzh_params** out) {
    if (!ctx || !out || k < 1 || k > 24) return BZH_E_ARG;
    if (generators_where != BZH_GENERATORS_HOST && generators_where != BZH_GENERATORS_DEVICE) return BZH_E_ARG;
    // BZH_PROVE_TRACE=1: where a cache miss's wall time goes, on stderr (tools/ubench_params.py reads these lines)
    const bool trace = getenv("BZH_PROVE_TRACE") != nullptr;
    auto t_last = std::chrono::steady_clock::now();
    auto mark = [&](const char* name) {
        if (!trace) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[bzh_params_create] %-22s %8.3f ms\n", name, std::chrono::duration<double, std::milli>(now - t_last).count());
        t_last = now;
    };
    std::unique_ptr<bzh_params> p(new bzh_params());
    p->k = k;
    p->n = (size_t)1 << k;
    const size_t n = p->n;
    p->g.assign(n * 8, 0);
    p->g_lagrange.assign(n * 8, 0);
    const std::string dir = cache_dir ? std::string(cache_dir) : default_cache_dir();
    const std::string path = dir + "/params_vesta_k" + std::to_string(k) + "_v1.bin";
    bool loaded = false;
    if (!dir.empty()) {
        if (FILE* f = fopen(path.c_str(), "rb")) {
            uint64_t hdr[2] = {0, 0};
            loaded = fread(hdr, 8, 2, f) == 2 && hdr[0] == 0x315352535a42ull /* "BZSRS1" */ && hdr[1] == k &&
                     fread(p->g.data(), 8, n * 8, f) == n * 8 && fread(p->g_lagrange.data(), 8, n * 8, f) == n * 8 &&
                     fread(p->w, 8, 8, f) == 8 && fread(p->u, 8, 8, f) == 8;
            fclose(f);
        }
    }
    mark("cache");
    if (!loaded && generators_where == BZH_GENERATORS_DEVICE) {
        const int rc = params_generate_device(ctx, p.get(), trace);   // prints its own marks
        if (rc) return rc;
        t_last = std::chrono::steady_clock::now();
    } else if (!loaded) {
        int rc = bzh_params_generators(k, p->g.data(), p->w, p->u, 0);
        if (rc) return rc;
        mark("generators");
        rc = bzh_group_ifft(ctx, BZH_CURVE_VESTA, p->g.data(), k, p->g_lagrange.data());
        if (rc) return rc;
        mark("group_fft");
    }
    if (!loaded) {
        if (!dir.empty()) {
            mkdir(dir.c_str(), 0755);
            const std::string tmp = path + ".tmp" + std::to_string((long)getpid());
            if (FILE* f = fopen(tmp.c_str(), "wb")) {
                const uint64_t hdr[2] = {0x315352535a42ull, k};
                const bool ok = fwrite(hdr, 8, 2, f) == 2 && fwrite(p->g.data(), 8, n * 8, f) == n * 8 &&
                                fwrite(p->g_lagrange.data(), 8, n * 8, f) == n * 8 && fwrite(p->w, 8, 8, f) == 8 && fwrite(p->u, 8, 8, f) == 8;
                fclose(f);
                if (ok) rename(tmp.c_str(), path.c_str());
                else remove(tmp.c_str());
            }
        }
    }
    p->from_cache = loaded;
    // (g | u | w) and (g_lagrange | u | w | g_0): sum_r g_lagrange[r] = g_0 (the Lagrange polynomials sum to 1), so a column with
    // a long constant stretch is committed as (column - c) + c * g_0 -- the grand products of the permutation argument stay at
    // their final value from the last copy constraint to the blinding rows (csrc/prove.hip: commit, shift_row)
    std::vector<uint64_t> tbl((n + 3) * 8);
    for (int which = 0; which < 2; which++) {
        memcpy(tbl.data(), which ? p->g_lagrange.data() : p->g.data(), n * 64);
        memcpy(&tbl[n * 8], p->u, 64);
        memcpy(&tbl[(n + 1) * 8], p->w, 64);
        memcpy(&tbl[(n + 2) * 8], p->g.data(), 64);
        bzh_bases* h = nullptr;
        int rc = bzh_bases_upload(ctx, BZH_CURVE_VESTA, tbl.data(), n + 2 + (which ? 1 : 0), BZH_FORM_CANONICAL, BZH_MEM_HOST, &h);
        if (!rc) rc = bzh_bases_precompute(ctx, h, window_bits);
        if (rc) {
            if (h) bzh_bases_free(ctx, h);
            bzh_params_free(ctx, p.release());
            return rc;
        }
        (which ? p->bases_lagrange : p->bases) = h;
    }
    if (trace) {
        std::lock_guard<std::mutex> lk(ctx->mu);
        (void)hipStreamSynchronize(ctx->stream);
    }
    mark("tables");
    *out = p.release();
    return BZH_OK;
}

int bzh_params_bases(const bzh_params* p, bzh_bases** g, bzh_bases** g_lagrange) {
    if (!p) return BZH_E_ARG;
    if (g) *g = p->bases;
    if (g_lagrange) *g_lagrange = p->bases_lagrange;
    return BZH_OK;
}
// host copies (canonical affine): any of the outputs may be NULL; g_xy / g_lagrange_xy hold n x 8 limbs
int bzh_params_points(const bzh_params* p, uint64_t* g_xy, uint64_t* g_lagrange_xy, uint64_t* w_xy, uint64_t* u_xy, int* from_cache) {
    if (!p) return BZH_E_ARG;
    if (g_xy) memcpy(g_xy, p->g.data(), p->n * 64);
    if (g_lagrange_xy) memcpy(g_lagrange_xy, p->g_lagrange.data(), p->n * 64);
    if (w_xy) memcpy(w_xy, p->w, 64);
    if (u_xy) memcpy(u_xy, p->u, 64);
    if (from_cache) *from_cache = p->from_cache ? 1 : 0;
    return BZH_OK;
}

}  // extern "C"
