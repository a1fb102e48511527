// Batched Fiat-Shamir transcripts on the device: halo2_proofs 0.2.0's transcript::{Blake2bWrite, Challenge255} for `batch`
// proofs in lockstep (bzh_transcript_batch_*).  The transcripts live in HBM, absorb affine points, Jacobian points (bzh_msm's
// output, through bzh_batch_normalize's launch) and scalars from device memory and squeeze their challenges into device memory,
// one launch per step for the whole batch: the device-resident path from MSM to challenge.  csrc/transcript.hip -- one host
// object per proof -- stays what the provers and the verifier use.
//
// Two kernels around csrc/transcript_batch.hpp -- the functions the host path (ctx == NULL) runs:
//   k_tb_absorb<C, KIND>  one lane per transcript takes `count` items (affine points or scalars, absorbed only or also written
//                         to the proof) from base + (b * stride + i): to canonical form in the lane (one fe_from_mont per
//                         coordinate of a Montgomery operand), 0x01 || x || y or 0x02 || repr built as whole words in
//                         registers, funnel-shifted by the uniform buflen % 8 and stored at the uniform word offset of the
//                         block buffer in HBM; a full buffer with more input to come is loaded back with constant indices and
//                         compressed (b2_compress: twelve rounds unrolled, constant sigma indices).  No register array is
//                         indexed with a runtime value.
//   k_tb_squeeze<C>       absorbs 0x00, finalises a copy of the state and reduces the digest mod the scalar field (3 products).
// t, buflen and the proof length are kernel arguments (the same for every transcript), so the only data-dependent branch is the
// tail guard.  256-thread blocks, one lane per transcript: a launch for 64 proofs is ONE wave, so its time is the length of the
// chain -- (65 or 33) * count / 128 compressions of 96 dependent G steps each --, not throughput.
// No LDS, no scratch.  From the gfx950 code object's notes, .vgpr_count for Vesta and Pallas / for BN254, and
// .private_segment_fixed_size = 0 for every one of them:
//   k_tb_absorb   common points 146 / 150, write points 158 / 162, common scalars 144 / 148, write scalars 154 / 158
//   k_tb_squeeze  133 / 133
// Next step, if tools/ubench_transcript.py shows that the chain matters: split one compression over the four lanes of a quad
// (a column of the working vector per lane, the diagonal step by DPP quad_perm), which shortens the chain about four times.
#include <cstring>
#include <new>
#include <vector>

#include "ctx.hpp"
#include "curve.cuh"
#include "transcript.hpp"
#include "transcript_batch.hpp"

struct bzh_transcript_batch {
    bzh_ctx* ctx = nullptr;   // null: host-resident
    int curve = 0;
    size_t batch = 0, proof_cap = 0;
    // the same for every transcript of the batch
    uint64_t t = 0;
    uint32_t buflen = 0;
    size_t proof_len = 0;
    bzh::TbState S{};
    std::vector<uint64_t> h_words;            // host-resident: h | buf
    std::vector<uint8_t> h_status, h_proofs;
    char* d_mem = nullptr;                    // device: h | buf | status | proofs
    char* d_scratch = nullptr;                // write_jacobian: affine points | status bytes
    size_t scratch_bytes = 0;
};

namespace bzh {
namespace {

template <class C, int KIND>
static __global__ void __launch_bounds__(256) k_tb_absorb(const TbState S, const void* base, size_t count, size_t stride, int canonical,
                                                          const uint8_t* pre, uint64_t t, uint32_t buflen, size_t proof_len) {
    const size_t b = blockIdx.x * (size_t)256 + threadIdx.x;
    if (b >= S.batch) return;
    tb_absorb<C, KIND>(S, b, base, count, stride, canonical != 0, pre, t, buflen, proof_len);
}
template <class C>
static __global__ void __launch_bounds__(256) k_tb_squeeze(const TbState S, uint64_t t, uint32_t buflen, int canonical, uint32_t* out) {
    const size_t b = blockIdx.x * (size_t)256 + threadIdx.x;
    if (b >= S.batch) return;
    tb_squeeze<C>(S, b, t, buflen, canonical != 0, out + b * 8);
}

static bool valid_form(int f) { return f == BZH_FORM_CANONICAL || f == BZH_FORM_MONTGOMERY; }
static bool valid_mem(int m) { return m == BZH_MEM_HOST || m == BZH_MEM_DEVICE; }
static bool valid_curve(int c) { return c >= BZH_CURVE_VESTA && c <= BZH_CURVE_BN254; }
constexpr size_t kMaxBatch = (size_t)1 << 20, kMaxProofCap = (size_t)1 << 24, kMaxItems = (size_t)1 << 28;
constexpr size_t kKindBytes[4] = {64, 64, 32, 32}, kKindLen[4] = {65, 65, 33, 33};

static size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
static int scalar_field_of(int curve) {
    int f = -1;
    with_curve(curve, [&](auto c) {
        f = CurveInfo<decltype(c)>::scalar_field;
        return BZH_OK;
    });
    return f;
}
// the fresh state: Blake2b-512 under "Halo2-Transcript"
static void fresh_words(size_t batch, std::vector<uint64_t>& w) {
    Blake2b s;
    s.init(64, reinterpret_cast<const uint8_t*>("Halo2-Transcript"));
    w.assign(24 * batch, 0);
    for (int i = 0; i < 8; i++)
        for (size_t b = 0; b < batch; b++) w[i * batch + b] = s.h[i];
}

// what every absorbing entry point checks before anything changes; item: bytes per operand item
static int check_call(const bzh_transcript_batch* tb, const void* p, size_t count, size_t stride, int form, int mem, bool write) {
    if (!tb || !valid_form(form) || !valid_mem(mem)) return BZH_E_ARG;
    if (!tb->ctx && mem != BZH_MEM_HOST) return BZH_E_ARG;
    if (!count) return BZH_OK;
    if (!p || stride < count || stride > kMaxItems / tb->batch) return BZH_E_ARG;
    if (mem == BZH_MEM_DEVICE && ((uintptr_t)p & 15)) return BZH_E_ARG;   // the kernels move 16 bytes at a time
    if (write && (count > tb->proof_cap / 32 || tb->proof_len + 32 * count > tb->proof_cap)) return BZH_E_RANGE;
    return BZH_OK;
}
// host operands in canonical form are checked before anything is absorbed; `per` field elements per item
template <class P>
static bool host_items_canonical(const uint64_t* p, size_t batch, size_t count, size_t stride, size_t per) {
    for (size_t b = 0; b < batch; b++)
        for (size_t i = 0; i < count * per; i++)
            if (!is_canonical(fe_from_u64<P>(p + 4 * (b * stride * per + i)))) return false;
    return true;
}
// the items of a strided host buffer side by side: batch x count items of `item` bytes
static std::vector<uint8_t> compact(const void* p, size_t batch, size_t count, size_t stride, size_t item) {
    std::vector<uint8_t> v(batch * count * item);
    for (size_t b = 0; b < batch; b++) memcpy(&v[b * count * item], (const char*)p + b * stride * item, count * item);
    return v;
}
static void advance(bzh_transcript_batch* tb, size_t count, uint32_t len, bool write) {
    for (size_t i = 0; i < count; i++) tb_advance(tb->t, tb->buflen, len);
    if (write) tb->proof_len += 32 * count;
}

template <int KIND>
static int absorb_launch(bzh_transcript_batch* tb, const void* d_base, size_t count, size_t stride, int form, const uint8_t* d_pre) {
    bzh_ctx* ctx = tb->ctx;
    return with_curve(tb->curve, [&](auto c) -> int {
        {
            ScopedTimer tm(ctx, BZH_T_POLY);
            hipLaunchKernelGGL((k_tb_absorb<decltype(c), KIND>), dim3((unsigned)((tb->batch + 255) / 256)), dim3(256), 0, ctx->stream, tb->S,
                               d_base, count, stride, form == BZH_FORM_CANONICAL ? 1 : 0, d_pre, tb->t, tb->buflen, tb->proof_len);
        }
        BZH_HIP_TRY(ctx, hipGetLastError());
        return BZH_OK;
    });
}

// common / write of affine points (KIND 0 / 1) and scalars (KIND 2 / 3)
template <int KIND>
static int absorb(bzh_transcript_batch* tb, const uint64_t* p, size_t count, size_t stride, int form, int mem) {
    constexpr bool point = KIND < 2, write = (KIND & 1) != 0;
    constexpr size_t item = kKindBytes[KIND];
    BZH_TRY(check_call(tb, p, count, stride, form, mem, write));
    if (!count) return BZH_OK;
    const bool canonical = form == BZH_FORM_CANONICAL;
    if (mem == BZH_MEM_HOST && canonical) {
        const int rc = with_curve(tb->curve, [&](auto c) -> int {
            using C = decltype(c);
            const bool ok = point ? host_items_canonical<typename C::Base>(p, tb->batch, count, stride, 2)
                                  : host_items_canonical<typename CurveInfo<C>::SF>(p, tb->batch, count, stride, 1);
            return ok ? BZH_OK : BZH_E_RANGE;
        });
        if (rc) return rc;
    }
    if (!tb->ctx) {
        with_curve(tb->curve, [&](auto c) -> int {
            for (size_t b = 0; b < tb->batch; b++)
                tb_absorb<decltype(c), KIND>(tb->S, b, p, count, stride, canonical, nullptr, tb->t, tb->buflen, tb->proof_len);
            return BZH_OK;
        });
    } else {
        bzh_ctx* ctx = tb->ctx;
        std::lock_guard<std::mutex> lk(ctx->mu);
        BZH_HIP_TRY(ctx, hipSetDevice(ctx->device));
        const void* d_base = p;
        if (mem == BZH_MEM_HOST) {   // staged in WS_STAGE, the items side by side (absorb_launch takes no workspace slot)
            const std::vector<uint8_t> v = compact(p, tb->batch, count, stride, item);
            void* ws = nullptr;
            BZH_TRY(ws_ensure(ctx, WS_STAGE, v.size() + 256, &ws));
            BZH_TRY(h2d_small(ctx, ws, v.data(), v.size()));
            d_base = ws;
            stride = count;
        }
        BZH_TRY(absorb_launch<KIND>(tb, d_base, count, stride, form, nullptr));
    }
    advance(tb, count, (uint32_t)kKindLen[KIND], write);
    return BZH_OK;
}

static int scratch_ensure(bzh_transcript_batch* tb, size_t bytes) {
    bzh_ctx* ctx = tb->ctx;
    if (tb->scratch_bytes >= bytes) return BZH_OK;
    if (tb->d_scratch) {
        BZH_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        BZH_HIP_TRY(ctx, hipFree(tb->d_scratch));
        tb->d_scratch = nullptr;
        tb->scratch_bytes = 0;
    }
    BZH_HIP_TRY(ctx, hipMalloc((void**)&tb->d_scratch, bytes));
    tb->scratch_bytes = bytes;
    return BZH_OK;
}

// device memory of a fresh batch: h | buf | status | proofs (the caller holds ctx->mu)
static int tb_device_init(bzh_transcript_batch* tb, const std::vector<uint64_t>& words) {
    bzh_ctx* ctx = tb->ctx;
    const size_t batch = tb->batch, st_off = 192 * batch, pr_off = st_off + round_up(batch, 256);
    BZH_HIP_TRY(ctx, hipMalloc((void**)&tb->d_mem, pr_off + batch * tb->S.pstride + 256));
    std::vector<uint8_t> img(pr_off, 0);
    memcpy(img.data(), words.data(), 192 * batch);
    BZH_TRY(h2d_small(ctx, tb->d_mem, img.data(), img.size()));
    tb->S.h = (uint64_t*)tb->d_mem, tb->S.buf = (uint64_t*)tb->d_mem + 8 * batch;
    tb->S.status = (uint8_t*)tb->d_mem + st_off, tb->S.proofs = (uint8_t*)tb->d_mem + pr_off;
    return BZH_OK;
}

}  // namespace

// ---------------------------------------------------------------------------
// the same object for a caller inside the library that already holds ctx->mu (the verifier's device pass, csrc/verifier.hpp):
// device operands only, enqueue only, no argument checks beyond the kind
// ---------------------------------------------------------------------------
int tb_new_locked(bzh_ctx* ctx, int curve, size_t batch, bzh_transcript_batch** out, size_t proof_cap) {
    if (!ctx || !out || !valid_curve(curve) || !batch || batch > kMaxBatch || proof_cap > kMaxProofCap) return BZH_E_ARG;
    const size_t pstride = round_up(proof_cap, 32);
    if (pstride && batch > ((size_t)1 << 32) / pstride) return BZH_E_ARG;
    bzh_transcript_batch* tb = new (std::nothrow) bzh_transcript_batch();
    if (!tb) return BZH_E_OOM;
    tb->ctx = ctx, tb->curve = curve, tb->batch = batch, tb->proof_cap = proof_cap;
    tb->S.batch = batch, tb->S.pstride = pstride;
    std::vector<uint64_t> words;
    fresh_words(batch, words);
    const int rc = tb_device_init(tb, words);
    if (rc) {
        if (tb->d_mem) (void)hipFree(tb->d_mem);
        delete tb;
        return rc;
    }
    *out = tb;
    return BZH_OK;
}
void tb_free_locked(bzh_transcript_batch* tb) {
    if (!tb) return;
    (void)hipStreamSynchronize(tb->ctx->stream);
    if (tb->d_mem) (void)hipFree(tb->d_mem);
    if (tb->d_scratch) (void)hipFree(tb->d_scratch);
    delete tb;
}
int tb_absorb_locked(bzh_transcript_batch* tb, int kind, const void* d_base, size_t count, size_t stride, int form, const uint8_t* d_pre) {
    if (!count) return BZH_OK;
    if (kind == 0)
        BZH_TRY(absorb_launch<0>(tb, d_base, count, stride, form, d_pre));
    else if (kind == 1)
        BZH_TRY(absorb_launch<1>(tb, d_base, count, stride, form, d_pre));
    else if (kind == 2)
        BZH_TRY(absorb_launch<2>(tb, d_base, count, stride, form, nullptr));
    else if (kind == 3)
        BZH_TRY(absorb_launch<3>(tb, d_base, count, stride, form, nullptr));
    else
        return BZH_E_ARG;
    advance(tb, count, (uint32_t)kKindLen[kind], (kind & 1) != 0);
    return BZH_OK;
}
// bzh_transcript_batch_write_jacobian's device half: bzh_batch_normalize's launch over the whole span the points lie in, into the
// batch's own scratch (which grows on first use), then the write kernel (kind 1) or the common kernel (kind 0)
int tb_write_jacobian_locked(bzh_transcript_batch* tb, const void* d_xyz, size_t count, size_t stride, int form, int kind) {
    if (!count) return BZH_OK;
    if (kind != 0 && kind != 1) return BZH_E_ARG;
    bzh_ctx* ctx = tb->ctx;
    const size_t n = (tb->batch - 1) * stride + count;
    BZH_TRY(scratch_ensure(tb, n * 64 + n + 256));
    uint8_t* d_st = (uint8_t*)tb->d_scratch + n * 64;
    BZH_TRY(normalize_run(ctx, tb->curve, d_xyz, n, form, tb->d_scratch, nullptr, d_st));
    if (kind) BZH_TRY(absorb_launch<1>(tb, tb->d_scratch, count, stride, form, d_st));
    else BZH_TRY(absorb_launch<0>(tb, tb->d_scratch, count, stride, form, d_st));
    advance(tb, count, 65, kind != 0);
    return BZH_OK;
}
TbInfo tb_info(const bzh_transcript_batch* tb) { return TbInfo{tb->ctx, tb->curve, tb->batch, tb->proof_cap, tb->proof_len}; }
int tb_squeeze_locked(bzh_transcript_batch* tb, int form, uint32_t* d_out) {
    bzh_ctx* ctx = tb->ctx;
    BZH_TRY(with_curve(tb->curve, [&](auto c) -> int {
        {
            ScopedTimer tm(ctx, BZH_T_POLY);
            hipLaunchKernelGGL((k_tb_squeeze<decltype(c)>), dim3((unsigned)((tb->batch + 255) / 256)), dim3(256), 0, ctx->stream, tb->S, tb->t,
                               tb->buflen, form == BZH_FORM_CANONICAL ? 1 : 0, d_out);
        }
        BZH_HIP_TRY(ctx, hipGetLastError());
        return BZH_OK;
    }));
    advance(tb, 1, 1, false);
    return BZH_OK;
}
const uint8_t* tb_status_device(const bzh_transcript_batch* tb) { return tb->S.status; }
uint8_t* tb_status_device_mut(bzh_transcript_batch* tb) { return tb->S.status; }
int tb_reserve_points_locked(bzh_transcript_batch* tb, size_t points) { return scratch_ensure(tb, points * 64 + points + 256); }
const uint8_t* tb_proofs_device(const bzh_transcript_batch* tb, size_t* pstride) {
    *pstride = tb->S.pstride;
    return tb->S.proofs;
}

}  // namespace bzh

using namespace bzh;

extern "C" int bzh_transcript_batch_new(bzh_ctx* ctx, int curve, size_t batch, size_t proof_cap, bzh_transcript_batch** out) {
    if (!out || !valid_curve(curve) || !batch || batch > kMaxBatch || proof_cap > kMaxProofCap) return BZH_E_ARG;
    const size_t pstride = round_up(proof_cap, 32);
    if (pstride && batch > ((size_t)1 << 32) / pstride) return BZH_E_ARG;
    bzh_transcript_batch* tb = new (std::nothrow) bzh_transcript_batch();
    if (!tb) return BZH_E_OOM;
    tb->ctx = ctx, tb->curve = curve, tb->batch = batch, tb->proof_cap = proof_cap;
    tb->S.batch = batch, tb->S.pstride = pstride;
    std::vector<uint64_t> words;
    fresh_words(batch, words);
    if (!ctx) {
        tb->h_words.swap(words);
        tb->h_status.assign(batch, 0);
        tb->h_proofs.assign(batch * pstride + 32, 0);
        tb->S.h = tb->h_words.data(), tb->S.buf = tb->h_words.data() + 8 * batch;
        tb->S.status = tb->h_status.data(), tb->S.proofs = tb->h_proofs.data();
        *out = tb;
        return BZH_OK;
    }
    const int rc = [&]() -> int {
        std::lock_guard<std::mutex> lk(ctx->mu);
        BZH_HIP_TRY(ctx, hipSetDevice(ctx->device));
        return tb_device_init(tb, words);
    }();
    if (rc) {
        if (tb->d_mem) (void)hipFree(tb->d_mem);
        delete tb;
        return rc;
    }
    *out = tb;
    return BZH_OK;
}

extern "C" int bzh_transcript_batch_free(bzh_transcript_batch* tb) {
    if (!tb) return BZH_E_ARG;
    if (tb->ctx) {
        std::lock_guard<std::mutex> lk(tb->ctx->mu);
        (void)hipSetDevice(tb->ctx->device);
        (void)hipStreamSynchronize(tb->ctx->stream);
        if (tb->d_mem) (void)hipFree(tb->d_mem);
        if (tb->d_scratch) (void)hipFree(tb->d_scratch);
    }
    delete tb;
    return BZH_OK;
}

extern "C" int bzh_transcript_batch_common_points(bzh_transcript_batch* tb, const uint64_t* xy, size_t count, size_t stride, int form, int mem) {
    return absorb<0>(tb, xy, count, stride, form, mem);
}
extern "C" int bzh_transcript_batch_write_points(bzh_transcript_batch* tb, const uint64_t* xy, size_t count, size_t stride, int form, int mem) {
    return absorb<1>(tb, xy, count, stride, form, mem);
}
extern "C" int bzh_transcript_batch_common_scalars(bzh_transcript_batch* tb, const uint64_t* s, size_t count, size_t stride, int form, int mem) {
    return absorb<2>(tb, s, count, stride, form, mem);
}
extern "C" int bzh_transcript_batch_write_scalars(bzh_transcript_batch* tb, const uint64_t* s, size_t count, size_t stride, int form, int mem) {
    return absorb<3>(tb, s, count, stride, form, mem);
}

// bzh_batch_normalize's launch into the batch's own scratch, then the write kernel: no arithmetic of its own
extern "C" int bzh_transcript_batch_write_jacobian(bzh_transcript_batch* tb, const uint64_t* xyz, size_t count, size_t stride, int form, int mem) {
    BZH_TRY(check_call(tb, xyz, count, stride, form, mem, true));
    if (!count) return BZH_OK;
    const bool canonical = form == BZH_FORM_CANONICAL, host = mem == BZH_MEM_HOST;
    if (host && canonical) {
        const int rc = with_curve(tb->curve, [&](auto c) -> int {
            return host_items_canonical<typename decltype(c)::Base>(xyz, tb->batch, count, stride, 3) ? BZH_OK : BZH_E_RANGE;
        });
        if (rc) return rc;
    }
    // host operands are normalised side by side; device operands as the whole span they lie in, gaps included (their results are
    // not read)
    const size_t n = host ? tb->batch * count : (tb->batch - 1) * stride + count;
    const size_t wstride = host ? count : stride;
    if (!tb->ctx) {
        const std::vector<uint8_t> jac = compact(xyz, tb->batch, count, stride, 96);
        std::vector<uint64_t> xy(n * 8);
        std::vector<uint8_t> st(n);
        NormIo io{jac.data(), xy.data(), nullptr, st.data(), n, 0, 0, canonical ? 1 : 0};
        normalize_plan(n, &io.lanes, &io.chain);
        with_curve(tb->curve, [&](auto c) -> int {
            for (size_t l = 0; l < io.lanes; l++) normalize_chain<decltype(c)>(io, l);
            for (size_t b = 0; b < tb->batch; b++)
                tb_absorb<decltype(c), 1>(tb->S, b, xy.data(), count, wstride, canonical, st.data(), tb->t, tb->buflen, tb->proof_len);
            return BZH_OK;
        });
    } else {
        bzh_ctx* ctx = tb->ctx;
        std::lock_guard<std::mutex> lk(ctx->mu);
        BZH_HIP_TRY(ctx, hipSetDevice(ctx->device));
        const void* d_in = xyz;
        if (host) {   // staged in WS_STAGE (tb_write_jacobian_locked takes no workspace slot)
            const std::vector<uint8_t> jac = compact(xyz, tb->batch, count, stride, 96);
            void* ws = nullptr;
            BZH_TRY(ws_ensure(ctx, WS_STAGE, jac.size() + 256, &ws));
            BZH_TRY(h2d_small(ctx, ws, jac.data(), jac.size()));
            d_in = ws;
        }
        return tb_write_jacobian_locked(tb, d_in, count, wstride, form);
    }
    advance(tb, count, 65, true);
    return BZH_OK;
}

extern "C" int bzh_transcript_batch_squeeze(bzh_transcript_batch* tb, int form, int mem, uint64_t* out) {
    if (!tb || !valid_form(form) || !valid_mem(mem) || !out) return BZH_E_ARG;
    if (!tb->ctx && mem != BZH_MEM_HOST) return BZH_E_ARG;
    if (mem == BZH_MEM_DEVICE && ((uintptr_t)out & 15)) return BZH_E_ARG;
    const bool canonical = form == BZH_FORM_CANONICAL;
    if (!tb->ctx) {
        with_curve(tb->curve, [&](auto c) -> int {
            for (size_t b = 0; b < tb->batch; b++) tb_squeeze<decltype(c)>(tb->S, b, tb->t, tb->buflen, canonical, out + 4 * b);
            return BZH_OK;
        });
        advance(tb, 1, 1, false);
        return BZH_OK;
    }
    bzh_ctx* ctx = tb->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    BZH_HIP_TRY(ctx, hipSetDevice(ctx->device));
    void* d_out = out;
    if (mem == BZH_MEM_HOST) BZH_TRY(ws_ensure(ctx, WS_STAGE, tb->batch * 32 + 256, &d_out));   // the squeeze kernel and its read-back only
    BZH_TRY(with_curve(tb->curve, [&](auto c) -> int {
        {
            ScopedTimer tm(ctx, BZH_T_POLY);
            hipLaunchKernelGGL((k_tb_squeeze<decltype(c)>), dim3((unsigned)((tb->batch + 255) / 256)), dim3(256), 0, ctx->stream, tb->S, tb->t,
                               tb->buflen, canonical ? 1 : 0, (uint32_t*)d_out);
        }
        BZH_HIP_TRY(ctx, hipGetLastError());
        return BZH_OK;
    }));
    advance(tb, 1, 1, false);
    if (mem == BZH_MEM_HOST) {
        BZH_TRY(d2h_async(ctx, out, d_out, tb->batch * 32));
        BZH_TRY(d2h_finish(ctx));
    }
    return BZH_OK;
}

extern "C" int bzh_transcript_batch_proofs(bzh_transcript_batch* tb, int mem, uint8_t* out, size_t out_stride, size_t* len) {
    if (!tb || !valid_mem(mem) || (!out && !len)) return BZH_E_ARG;
    if (out && (out_stride < tb->proof_len || (!tb->ctx && mem != BZH_MEM_HOST))) return BZH_E_ARG;
    if (len) *len = tb->proof_len;
    if (!out || !tb->proof_len) return BZH_OK;
    if (!tb->ctx) {
        for (size_t b = 0; b < tb->batch; b++) memcpy(out + b * out_stride, tb->S.proofs + b * tb->S.pstride, tb->proof_len);
        return BZH_OK;
    }
    bzh_ctx* ctx = tb->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    BZH_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (mem == BZH_MEM_DEVICE) {
        BZH_HIP_TRY(ctx, hipMemcpy2DAsync(out, out_stride, tb->S.proofs, tb->S.pstride, tb->proof_len, tb->batch, hipMemcpyDeviceToDevice, ctx->stream));
        return BZH_OK;
    }
    std::vector<uint8_t> rows(tb->batch * tb->S.pstride);
    BZH_TRY(d2h_async(ctx, rows.data(), tb->S.proofs, rows.size()));
    BZH_TRY(d2h_finish(ctx));
    for (size_t b = 0; b < tb->batch; b++) memcpy(out + b * out_stride, &rows[b * tb->S.pstride], tb->proof_len);
    return BZH_OK;
}

extern "C" int bzh_transcript_batch_status(bzh_transcript_batch* tb, uint8_t* out) {
    if (!tb || !out) return BZH_E_ARG;
    if (!tb->ctx) {
        memcpy(out, tb->S.status, tb->batch);
        return BZH_OK;
    }
    bzh_ctx* ctx = tb->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    BZH_HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::vector<uint8_t> st(round_up(tb->batch, 16));   // the copy kernels move whole words; the status bytes are padded to 256
    BZH_TRY(d2h_async(ctx, st.data(), tb->S.status, st.size()));
    BZH_TRY(d2h_finish(ctx));
    memcpy(out, st.data(), tb->batch);
    return BZH_OK;
}

extern "C" int bzh_transcript_batch_from_host(bzh_transcript_batch* tb, const bzh_transcript* const* hosts) {
    if (!tb || !hosts) return BZH_E_ARG;
    const size_t B = tb->batch, ps = tb->S.pstride;
    const int field = scalar_field_of(tb->curve);
    for (size_t b = 0; b < B; b++) {
        const bzh_transcript* h = hosts[b];
        if (!h || h->field != field || h->state.t1 || h->state.t0 != hosts[0]->state.t0 || h->state.buflen != hosts[0]->state.buflen ||
            h->state.buflen > 128 || h->proof.size() != hosts[0]->proof.size() || h->proof.size() > tb->proof_cap || h->proof.size() % 32)
            return BZH_E_ARG;
    }
    const size_t plen = hosts[0]->proof.size();
    std::vector<uint64_t> words(24 * B, 0);
    std::vector<uint8_t> proofs(plen ? B * ps : 0, 0);
    for (size_t b = 0; b < B; b++) {
        const Blake2b& s = hosts[b]->state;
        uint64_t m[16] = {0};
        memcpy(m, s.buf, s.buflen);   // the object's buffer may hold old bytes past buflen; the batch's is zero there
        for (int i = 0; i < 8; i++) words[i * B + b] = s.h[i];
        for (int w = 0; w < 16; w++) words[(8 + w) * B + b] = m[w];
        if (plen) memcpy(&proofs[b * ps], hosts[b]->proof.data(), plen);
    }
    if (!tb->ctx) {
        memcpy(tb->h_words.data(), words.data(), 192 * B);
        tb->h_status.assign(B, 0);
        if (plen) memcpy(tb->h_proofs.data(), proofs.data(), proofs.size());
    } else {
        bzh_ctx* ctx = tb->ctx;
        std::lock_guard<std::mutex> lk(ctx->mu);
        BZH_HIP_TRY(ctx, hipSetDevice(ctx->device));
        std::vector<uint8_t> img(192 * B + round_up(B, 256), 0);
        memcpy(img.data(), words.data(), 192 * B);
        BZH_TRY(h2d_small(ctx, tb->d_mem, img.data(), img.size()));
        if (plen) BZH_TRY(h2d_small(ctx, tb->S.proofs, proofs.data(), proofs.size()));
    }
    tb->t = hosts[0]->state.t0, tb->buflen = (uint32_t)hosts[0]->state.buflen, tb->proof_len = plen;
    return BZH_OK;
}

extern "C" int bzh_transcript_batch_to_host(bzh_transcript_batch* tb, bzh_transcript* const* hosts) {
    if (!tb || !hosts) return BZH_E_ARG;
    const size_t B = tb->batch, ps = tb->S.pstride;
    const int field = scalar_field_of(tb->curve);
    for (size_t b = 0; b < B; b++)
        if (!hosts[b] || hosts[b]->field != field) return BZH_E_ARG;
    std::vector<uint64_t> words(24 * B);
    std::vector<uint8_t> proofs(tb->proof_len ? B * ps : 0);
    if (!tb->ctx) {
        memcpy(words.data(), tb->h_words.data(), 192 * B);
        if (tb->proof_len) memcpy(proofs.data(), tb->S.proofs, proofs.size());
    } else {
        bzh_ctx* ctx = tb->ctx;
        std::lock_guard<std::mutex> lk(ctx->mu);
        BZH_HIP_TRY(ctx, hipSetDevice(ctx->device));
        BZH_TRY(d2h_async(ctx, words.data(), tb->d_mem, 192 * B));
        if (tb->proof_len) BZH_TRY(d2h_async(ctx, proofs.data(), tb->S.proofs, proofs.size()));
        BZH_TRY(d2h_finish(ctx));
    }
    for (size_t b = 0; b < B; b++) {
        Blake2b& s = hosts[b]->state;
        uint64_t m[16];
        for (int i = 0; i < 8; i++) s.h[i] = words[i * B + b];
        for (int w = 0; w < 16; w++) m[w] = words[(8 + w) * B + b];
        memcpy(s.buf, m, 128);
        s.t0 = tb->t, s.t1 = 0, s.buflen = tb->buflen;
        hosts[b]->proof.assign(proofs.begin() + (tb->proof_len ? b * ps : 0), proofs.begin() + (tb->proof_len ? b * ps + tb->proof_len : 0));
    }
    return BZH_OK;
}
