// Context, workspace and timing plumbing behind the C ABI (include/bzh2.h).
#pragma once
#include <hip/hip_runtime.h>
#include <sched.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/bzh2.h"

struct bzh_bases {
    int curve = 0;
    size_t n = 0;
    uint32_t* d_xy = nullptr;  // affine x||y, Montgomery form: n points, or pre_nwin rows of n
    int device = 0;
    int pre_c = 0;     // != 0: d_xy holds the window table, row w = 2^(pre_c * w) * G_i
    int pre_nwin = 0;
    // Several tables side by side (one per proof: the IPA's collapsed generators, msm_collapse_table): the rows of the table
    // array are row_stride points apart (0: n) and vector v of a batch reads the columns [v * vec_col_stride, + n)
    size_t row_stride = 0;
    size_t vec_col_stride = 0;
    // Window tables of the Pasta curves carry a second copy for k_msm_accumulate's unsaturated-limb loop: point i as 20 words --
    // x then y in 9 x 29-bit limbs (x 2^261, below 2 p, carried), 2 words of padding -- so that the loop loads its operands
    // ready-made instead of re-slicing and folding two coordinates per addition (csrc/fe29.cuh).  Same indexing as d_xy.
    uint32_t* d_xy29 = nullptr;
};

namespace bzh {
// The six grow-only device workspaces of a ctx (ws_ensure).  Calls on a ctx are serialised and stream-ordered, so a slot is shared
// by everything that names it, under two rules:
//   WS_SCRATCH_A..C are LEAF scratch.  Their content is dead once the function that took the slot has enqueued its launches, and
//   whoever holds data in one may call nothing that takes the same slot: msm_run / msm_run_paired take all three, ntt_run /
//   ntt_run_padded above 2^11 and poly_batch_invert take A, the prefix scans and poly_kate_division take C.
//   WS_STAGE, WS_IPA and WS_IPA_OUT live for a whole C ABI call.  No internal driver (msm_run*, ntt_run*, poly_*, lookup_permute)
//   takes them, so their holder may call all of those, but not another holder of the same slot.
//   The device synthesis (synth_device_enqueue) holds WS_STAGE -- layout, packed inputs, flags -- only while its three kernels
//   run.  A caller that goes on to other holders of the slot in the same call (the game-input prover: the prover's leaves stage in
//   WS_STAGE themselves) must therefore have the synthesis write what outlives those kernels, the status words and the
//   commitments, into memory of its own (the key's arena), and must enqueue whatever still reads the packed inputs
//   (k_pg_instances) before the first such holder.
enum WsSlot {
    WS_SCRATCH_A = 0,   // MSM digits | multi-pass NTT scratch | batch inversion's prefix products | generators of a one-off table build
    WS_SCRATCH_B = 1,   // MSM buckets | bzh_lookup_permute's working set | Pedersen operands | bzh_bases_read's canonical copy
    WS_SCRATCH_C = 2,   // MSM window sums | tile totals of the scans and of the Kate division
    WS_STAGE = 3,       // host staging: BZH_MEM_HOST operands and results of one C ABI call
    WS_IPA = 4,         // the opening's vectors and collapsed tables | the batch check's scalars and sums
    WS_IPA_OUT = 5,     // the opening's L / R points of a round
    kWsSlots = 6
};
// The NTT domain tables of one ctx (csrc/ntt.hip), opaque here; ntt.hip creates the cache on first use and sets its deleter.
struct NttCache;
// serial number of a ctx: process-wide, never reused (what a key files its per-ctx workspace under, csrc/key_runtime.hpp)
inline uint64_t next_ctx_serial() {
    static std::atomic<uint64_t> next{1};
    return next.fetch_add(1, std::memory_order_relaxed);
}
}  // namespace bzh

struct bzh_ctx {
    int device = 0;
    const uint64_t serial = bzh::next_ctx_serial();
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::mutex mu;
    std::string last_error;
    // grow-only device workspaces (calls on a ctx are serialised and stream-ordered)
    void* ws[bzh::kWsSlots] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // by bzh::WsSlot
    size_t ws_bytes[bzh::kWsSlots] = {0, 0, 0, 0, 0, 0};
    // profiling
    bool profiling = false;
    struct Span {
        int cls;
        hipEvent_t a, b;
    };
    std::vector<Span> spans;
    std::vector<hipEvent_t> event_pool;
    double acc_ms[BZH_T_COUNT] = {0};
    uint64_t acc_n[BZH_T_COUNT] = {0};
    double alg_bytes[BZH_T_COUNT] = {0};  // algorithmic bytes of the launches timed while profiling
    int num_cu = 256;
    unsigned long long* d_add_counter = nullptr;   // device counter of bucket additions (non-zero window digits), while profiling
    bool msm_attr_set[3] = {false, false, false};  // hipFuncSetAttribute(MaxDynamicSharedMemorySize) done on this ctx's device, per curve
    // pinned upload ring: small host->device copies stay asynchronous (a pageable hipMemcpyAsync waits for the copy)
    char* pin = nullptr;
    size_t pin_bytes = 0, pin_off = 0;
    char* pin_big = nullptr;  // grow-only pinned buffer for transfers above 1 MiB
    size_t pin_big_bytes = 0, pin_big_off = 0;
    struct PendingD2H {
        void* dst;
        const char* slot;
        size_t bytes;
    };
    std::vector<PendingD2H> pending_d2h;
    uint32_t* ped_tbl = nullptr;   // bzh_pedersen_commit_batch's direct-lookup table of V and R (csrc/pedersen.hip), built on first use
    uint32_t* syn_tbl = nullptr;   // device synthesis' copy of the circuits' fixed-base window tables (csrc/synthesize_device.hip), on first use
    uint32_t* sqrt_tbl[4] = {nullptr, nullptr, nullptr, nullptr};   // per field: g^(2^i), i <= S, for the square root (csrc/sqrt_decompress.hip), on first use
    std::unique_ptr<bzh::NttCache, void (*)(bzh::NttCache*)> ntt{nullptr, nullptr};   // the transforms' domain tables (csrc/ntt.hip), on first use
};

#define BZH_HIP_TRY(ctx, expr)                                                                    \
    do {                                                                                          \
        hipError_t e__ = (expr);                                                                  \
        if (e__ != hipSuccess) {                                                                  \
            (ctx)->last_error = std::string(#expr) + ": " + hipGetErrorString(e__);               \
            return (e__ == hipErrorOutOfMemory) ? BZH_E_OOM : BZH_E_HIP;                          \
        }                                                                                         \
    } while (0)
// hand a callee's status up unless it is BZH_OK
#define BZH_TRY(expr)          \
    do {                       \
        int rc__ = (expr);     \
        if (rc__) return rc__; \
    } while (0)

namespace bzh {

// Host threads one call may start (witness synthesis, the lookup's sort helpers, the verifier's per-proof pool, Params::new's
// hash-to-curve): $BZH_HOST_THREADS when set -- a multi-rank launcher gives every rank its share of the node's cores there
// (bench.py: affinity count / world size) --, else the calling thread's CPU affinity count (std::thread::hardware_concurrency
// counts the machine's cores, not the cgroup / taskset share).  Read per call: a launcher may set it after loading the library.
inline unsigned host_thread_budget() {
    if (const char* e = getenv("BZH_HOST_THREADS")) {
        const int v = atoi(e);
        if (v > 0) return (unsigned)v;
    }
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof(set), &set) == 0) {
        const int c = CPU_COUNT(&set);
        if (c > 0) return (unsigned)c;
    }
    return 1u;
}

// grow-only workspace slot
inline int ws_ensure(bzh_ctx* ctx, WsSlot slot, size_t bytes, void** out) {
    if (ctx->ws_bytes[slot] < bytes) {
        if (ctx->ws[slot]) {
            BZH_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            BZH_HIP_TRY(ctx, hipFree(ctx->ws[slot]));
            ctx->ws[slot] = nullptr;
            ctx->ws_bytes[slot] = 0;
        }
        size_t want = bytes + (bytes >> 3);
        BZH_HIP_TRY(ctx, hipMalloc(&ctx->ws[slot], want));
        ctx->ws_bytes[slot] = want;
    }
    *out = ctx->ws[slot];
    return BZH_OK;
}

// ---------------------------------------------------------------------------
// Host <-> device staging through pinned memory and copy KERNELS.  The runtime's own copy paths (SDMA / blit
// through hipMemcpyAsync) showed 3x slower transfers and multi-millisecond stalls on small copies in every
// process after the first one on a box ("transfers"); a kernel that reads or writes mapped pinned
// host memory has launch-like latency and is stream-ordered like everything else.
//   h2d_small  short-lived host buffer -> device, asynchronous (ring of pinned slots, or the big buffer)
//   d2h_async  device -> host destination, completed by d2h_finish (one stream sync for any number of them)
// ---------------------------------------------------------------------------
static __global__ void __launch_bounds__(256) k_xfer16(uint4* __restrict__ dst, const uint4* __restrict__ src, size_t n16) {
    for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256) dst[i] = src[i];
}
static __global__ void __launch_bounds__(256) k_xfer4(uint32_t* __restrict__ dst, const uint32_t* __restrict__ src, size_t n4) {
    for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) dst[i] = src[i];
}
// stream-ordered copy between two device-visible addresses (device memory or mapped pinned host memory)
inline int xfer_launch(bzh_ctx* ctx, void* dst, const void* src, size_t bytes, hipMemcpyKind fallback) {
    if (!bytes) return BZH_OK;
    const uintptr_t al = (uintptr_t)dst | (uintptr_t)src | (uintptr_t)bytes;
    if ((al & 15) == 0) {
        const size_t n16 = bytes / 16;
        const unsigned blocks = (unsigned)std::min<size_t>((n16 + 255) / 256, 2048);
        hipLaunchKernelGGL(k_xfer16, dim3(blocks), dim3(256), 0, ctx->stream, (uint4*)dst, (const uint4*)src, n16);
    } else if ((al & 3) == 0) {
        const size_t n4 = bytes / 4;
        const unsigned blocks = (unsigned)std::min<size_t>((n4 + 255) / 256, 2048);
        hipLaunchKernelGGL(k_xfer4, dim3(blocks), dim3(256), 0, ctx->stream, (uint32_t*)dst, (const uint32_t*)src, n4);
    } else {
        BZH_HIP_TRY(ctx, hipMemcpyAsync(dst, src, bytes, fallback, ctx->stream));
        return BZH_OK;
    }
    BZH_HIP_TRY(ctx, hipGetLastError());
    return BZH_OK;
}
// One stream synchronisation, then the staged results are handed to their destinations: afterwards nothing queued reads or
// writes a pinned slot, so the buffers may be recycled or replaced.
inline int pin_drain(bzh_ctx* ctx) {
    BZH_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (auto& p : ctx->pending_d2h) memcpy(p.dst, p.slot, p.bytes);
    ctx->pending_d2h.clear();
    return BZH_OK;
}
inline int pin_big_ensure(bzh_ctx* ctx, size_t bytes) {
    if (ctx->pin_big_bytes >= bytes) return BZH_OK;
    BZH_TRY(pin_drain(ctx));
    if (ctx->pin_big) BZH_HIP_TRY(ctx, hipHostFree(ctx->pin_big));
    ctx->pin_big = nullptr;
    ctx->pin_big_bytes = 0;
    const size_t want = bytes + (bytes >> 2) + 4096;
    BZH_HIP_TRY(ctx, hipHostMalloc((void**)&ctx->pin_big, want, hipHostMallocDefault));
    ctx->pin_big_bytes = want;
    ctx->pin_big_off = 0;
    return BZH_OK;
}
// slot of `bytes` in the big pinned buffer; waits for the stream when the buffer has to be recycled
inline int pin_big_take(bzh_ctx* ctx, size_t bytes, char** out) {
    const size_t need = (bytes + 255) & ~(size_t)255;
    if (ctx->pin_big_bytes < need) {
        int rc = pin_big_ensure(ctx, need);
        if (rc) return rc;
    }
    if (ctx->pin_big_off + need > ctx->pin_big_bytes) {
        BZH_TRY(pin_drain(ctx));   // staged results leave before their slots are reused
        ctx->pin_big_off = 0;
    }
    *out = ctx->pin_big + ctx->pin_big_off;
    ctx->pin_big_off += need;
    return BZH_OK;
}
// make room for a group of big slots that have to stay valid together (no recycling in between)
inline int pin_big_reserve(bzh_ctx* ctx, size_t total) {
    total += 4096;
    int rc = pin_big_ensure(ctx, total);
    if (rc) return rc;
    if (ctx->pin_big_off + total > ctx->pin_big_bytes) {
        BZH_TRY(pin_drain(ctx));
        ctx->pin_big_off = 0;
    }
    return BZH_OK;
}
inline int pin_ring_take(bzh_ctx* ctx, size_t bytes, char** out) {
    constexpr size_t kRing = (size_t)8 << 20;
    if (!ctx->pin) {
        BZH_HIP_TRY(ctx, hipHostMalloc((void**)&ctx->pin, kRing, hipHostMallocDefault));
        ctx->pin_bytes = kRing;
        ctx->pin_off = 0;
    }
    const size_t need = (bytes + 255) & ~(size_t)255;
    if (ctx->pin_off + need > ctx->pin_bytes) {  // wrap: everything queued from the ring has to have landed
        BZH_TRY(pin_drain(ctx));
        ctx->pin_off = 0;
    }
    *out = ctx->pin + ctx->pin_off;
    ctx->pin_off += need;
    return BZH_OK;
}
inline int h2d_small(bzh_ctx* ctx, void* dst, const void* src, size_t bytes) {
    if (!bytes) return BZH_OK;
    char* slot = nullptr;
    int rc = bytes > ((size_t)1 << 20) ? pin_big_take(ctx, bytes, &slot) : pin_ring_take(ctx, bytes, &slot);
    if (rc) return rc;
    memcpy(slot, src, bytes);
    return xfer_launch(ctx, dst, slot, bytes, hipMemcpyHostToDevice);
}
// pinned staging slot the caller fills itself (saves one host copy for large uploads), then h2d_commit
inline int h2d_stage(bzh_ctx* ctx, size_t bytes, char** slot) {
    return bytes > ((size_t)1 << 20) ? pin_big_take(ctx, bytes, slot) : pin_ring_take(ctx, bytes, slot);
}
inline int h2d_commit(bzh_ctx* ctx, void* dst, const char* slot, size_t bytes) {
    return xfer_launch(ctx, dst, slot, bytes, hipMemcpyHostToDevice);
}
inline int d2h_async(bzh_ctx* ctx, void* host_dst, const void* dev_src, size_t bytes) {
    if (!bytes) return BZH_OK;
    char* slot = nullptr;
    int rc = bytes > ((size_t)1 << 20) ? pin_big_take(ctx, bytes, &slot) : pin_ring_take(ctx, bytes, &slot);
    if (rc) return rc;
    rc = xfer_launch(ctx, slot, dev_src, bytes, hipMemcpyDeviceToHost);
    if (rc) return rc;
    ctx->pending_d2h.push_back({host_dst, slot, bytes});
    return BZH_OK;
}
// the end of a group of d2h_async: one stream synchronisation for any number of them
inline int d2h_finish(bzh_ctx* ctx) { return pin_drain(ctx); }

struct ScopedTimer {
    bzh_ctx* ctx;
    int cls;
    hipEvent_t a = nullptr, b = nullptr;
    ScopedTimer(bzh_ctx* c, int k) : ctx(c), cls(k) {
        if (!ctx->profiling) return;
        a = take();
        b = take();
        if (a && b) (void)hipEventRecord(a, ctx->stream);
    }
    ~ScopedTimer() {
        if (!ctx->profiling || !a || !b) return;
        (void)hipEventRecord(b, ctx->stream);
        ctx->spans.push_back({cls, a, b});
    }
    hipEvent_t take() {
        if (!ctx->event_pool.empty()) {
            hipEvent_t e = ctx->event_pool.back();
            ctx->event_pool.pop_back();
            return e;
        }
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess) return nullptr;
        return e;
    }
};

// implemented in msm.hip / ntt.hip
int msm_run(bzh_ctx* ctx, const bzh_bases* bases, const uint32_t* d_scalars, size_t n, size_t batch, int form,
            uint32_t* d_out_xyz);
int msm_run_paired(bzh_ctx* ctx, const bzh_bases* bases, const uint32_t* d_scalars, size_t n_pair, unsigned log_m, size_t batch,
                   int form, uint32_t* d_out_xyz);
int ntt_run(bzh_ctx* ctx, int field, uint32_t* d_data, unsigned log_n, size_t batch, const uint64_t* omega,
            const uint64_t* coset_shift, int inverse, int form);
// d_out29 != null (Pasta scalar fields): the evaluations leave the last pass as unsaturated planes (fe29.cuh, 9 * 2^log_n words per
// polynomial) instead of going to d_dst, which may then be null
int ntt_run_padded(bzh_ctx* ctx, int field, uint32_t* d_dst, const uint32_t* d_src, unsigned src_log, unsigned log_n, size_t batch,
                   const uint64_t* omega, const uint64_t* coset_shift, uint32_t* d_out29 = nullptr);
int bases_to_montgomery(bzh_ctx* ctx, int curve, uint32_t* d_xy, size_t n);
int bases_precompute(bzh_ctx* ctx, bzh_bases* bases, int window_bits);
// The IPA's generator collapse on the device.  For every proof b of `batch`: G'[b][i] = sum_{t < cnt} s[b][t] * G[i + t*m], i < m
// = n_srs / cnt, evaluated through the SRS window table `srs` (n_srs + 2 points), followed by U and W (the table's last two
// points), and expanded into a per-proof window table of c_tail-bit rows.  d_s: batch x cnt Montgomery scalars.
// d_table: ceil(256 / c_tail) rows of batch * (m + 2) affine points; d_scratch: msm_collapse_scratch_bytes() bytes.
// `out` is filled to describe the table array to msm_run_paired (it borrows d_table).
size_t msm_collapse_scratch_bytes(const bzh_bases* srs, size_t cnt, size_t batch, int c_tail);
// (d_table29: room for the fe29 copy of the collapsed tables, 20 words per point, or null)
int msm_collapse_table(bzh_ctx* ctx, const bzh_bases* srs, const uint32_t* d_s, size_t cnt, size_t batch, int c_tail, uint32_t* d_table29, uint32_t* d_table,
                       void* d_scratch, bzh_bases* out);
// polyops.hip (device pointers, Montgomery form)
int field_convert(bzh_ctx* ctx, int field, uint32_t* d, size_t count, int to_mont);
int poly_batch_invert(bzh_ctx* ctx, int field, uint32_t* d, size_t count);
int poly_prefix_product(bzh_ctx* ctx, int field, uint32_t* d, size_t n, size_t batch);
int poly_eval(bzh_ctx* ctx, int field, const uint32_t* coeffs, size_t n, size_t batch, const uint32_t* xs, size_t x_stride,
              uint32_t* out);
int poly_inner_product(bzh_ctx* ctx, int field, const uint32_t* a, const uint32_t* b, size_t n, size_t batch, uint32_t* out);
int poly_fold(bzh_ctx* ctx, int field, const uint32_t* in, size_t half, size_t batch, const uint32_t* u, size_t u_stride,
              uint32_t* out);
int poly_vec_mul(bzh_ctx* ctx, int field, uint32_t* a, const uint32_t* b, size_t count);
int poly_kate_division(bzh_ctx* ctx, int field, const uint32_t* d_c, size_t n, size_t batch, const uint32_t* d_xs, uint32_t* d_q);
// lookup_permute.hip: permute_expression_pair for `batch` (input, table) pairs on the device.  Vector b of d_in / d_tab starts at
// element b * stride and is read in `form`; the permuted pair goes, in the same form, to d_out_a / d_out_s + b * out_stride
// elements, rows [usable, rows) zero (rows <= out_stride).  d_ws: lookup_permute_ws_bytes() bytes.  *d_status: `batch` words
// in d_ws, 0 or BZH_E_RANGE per pair, valid once the stream has run.
size_t lookup_permute_ws_bytes(size_t usable, size_t batch);
int lookup_permute(bzh_ctx* ctx, int field, const uint32_t* d_in, const uint32_t* d_tab, size_t stride, size_t usable, size_t batch, int form,
                   uint32_t* d_out_a, uint32_t* d_out_s, size_t out_stride, size_t rows, void* d_ws, int32_t** d_status);
// exprvm.hip
int expr_eval(bzh_ctx* ctx, int field, const void* d_prog, int nops, const uint32_t* const* d_cols, const size_t* d_strides,
              const uint32_t* d_consts, size_t const_stride, size_t size, int result_slot, size_t batch, int nslots, uint32_t* d_out);
// VM v2 (stack-discipline registers + LDS slot file): the prover's quotient evaluator
int expr_eval2(bzh_ctx* ctx, int field, const void* d_prog, int nops, const uint32_t* const* d_cols, const size_t* d_strides,
               const uint32_t* d_consts, size_t const_stride, size_t size, size_t batch, int nlds, uint32_t* d_out);
// ... coset by coset: eight launches of 2^log_n lanes fill the 8 * 2^log_n rows of d_out (k_expr_vm2_cosets).  d_cols_by_coset: 8
// column pointer tables (host array of device pointers), d_shifts: 0 / 3 per column; refill(j), when set, runs before launch j
int expr_eval2_cosets(bzh_ctx* ctx, int field, const void* d_prog, int nops, const uint32_t* const* const* d_cols_by_coset,
                      const size_t* d_strides, const uint32_t* d_shifts, const uint32_t* d_consts, size_t const_stride, unsigned log_n,
                      size_t batch, int nlds, uint32_t* d_out, const std::function<int(unsigned)>& refill);
// prove.hip: the seeded provers' expansion of bzh_rng_expand's stream on the device (k_chacha20_rows).  d_raw[(b * count + i) * 16 ..]
// = the 64-byte draw counter0 + i of the stream keyed by the eight words at d_keys + 8 b, b < batch <= 65535; d_raw 16-byte
// aligned.  Enqueues only.
int rng_rows_device(bzh_ctx* ctx, const uint32_t* d_keys, uint64_t counter0, size_t count, size_t batch, uint32_t* d_raw);
// ipa.hip
int random_field(bzh_ctx* ctx, int field, const uint32_t* d_raw, size_t count, uint32_t* d_out);
int ipa_open(bzh_ctx* ctx, const bzh_bases* bases, const uint32_t* d_polys, size_t batch, const uint64_t* blinds,
             const uint64_t* x3s, const uint8_t* rng_bytes, size_t rng_stride, bzh_transcript* const* trs, uint64_t* out_v,
             const uint32_t* d_raw_in = nullptr);  // d_raw_in: the draws already on the device (batch x (n + 1 + 2k) x 64 B) instead of rng_bytes
// the same opening against a device-resident transcript batch of this ctx (the caller holds ctx->mu and has checked its curve, size
// and proof room): every operand in device memory, 16-byte aligned; d_polys Montgomery, d_blinds / d_x3s / d_out_v in `form`, draws
// of proof b at d_rng + b * rng_stride, d_status one byte per proof or null.  Enqueues only.
int ipa_open_device(bzh_ctx* ctx, const bzh_bases* bases, const uint32_t* d_polys, size_t batch, const uint32_t* d_blinds,
                    const uint32_t* d_x3s, int form, const uint8_t* d_rng, size_t rng_stride, bzh_transcript_batch* tb,
                    uint32_t* d_out_v, uint8_t* d_status);
// the blinded commitment the opening makes for S, for `batch` polynomials of n = bases->n - 2 Montgomery coefficients: scalars
// [poly_b, 0, blind_b] (d_scalars: batch x (n + 2) scratch) against g || u || w, the Jacobian sums into d_out_xyz.  Enqueues only.
int ipa_commit_blinded(bzh_ctx* ctx, const bzh_bases* bases, const uint32_t* d_polys, size_t batch, const uint32_t* d_blinds,
                       uint32_t* d_scalars, uint32_t* d_out_xyz);
// multiopen.hip: bzh_multiopen_batch_device for a caller that holds ctx->mu and has made every argument check.  The grouping of
// bzh_multiopen_plan comes in as MoPlan; every data pointer is device memory, 16-byte aligned; d_polys (batch x npolys_own x n) and
// d_shared (npolys_shared x n) Montgomery; blinds and points in `form`; d_scratch: multiopen_scratch_bytes() bytes that no callee
// takes (WS_STAGE).  Enqueues only.
struct MoPlan {
    size_t npolys_own = 0, npolys_shared = 0, npoints = 0, nsets = 0;
    std::vector<uint32_t> set_of_poly, group_order, set_sizes, set_points;   // as bzh_multiopen_plan fills them
};
// one Horner term of k_mo_combine, and one source of k_ev_multipoint: coefficient i of proof b at p + (b * stride + i) elements;
// stride 0: the polynomial is shared by every proof
struct MoSrc {
    const uint32_t* p;
    uint64_t stride;
};
size_t multiopen_scratch_bytes(const MoPlan& plan, size_t batch, size_t n);
int multiopen_device(bzh_ctx* ctx, const bzh_bases* bases, size_t batch, unsigned k, const MoPlan& plan, const uint32_t* d_polys,
                     const uint32_t* d_shared, const uint32_t* d_blinds, const uint32_t* d_shared_blinds, const uint32_t* d_points, int form,
                     const uint8_t* d_rng, size_t rng_stride, bzh_transcript_batch* tb, uint8_t* d_status, void* d_scratch);
// the same with every polynomial where it lies: srcs (host memory) holds one MoSrc per polynomial id, own ids first; d_blinds stays
// the dense [batch][npolys_own] row.  multiopen_device builds this table from its dense operands.
int multiopen_device_srcs(bzh_ctx* ctx, const bzh_bases* bases, size_t batch, unsigned k, const MoPlan& plan, const MoSrc* srcs,
                          const uint32_t* d_blinds, const uint32_t* d_shared_blinds, const uint32_t* d_points, int form, const uint8_t* d_rng,
                          size_t rng_stride, bzh_transcript_batch* tb, uint8_t* d_status, void* d_scratch);
// k_mo_combine for another caller (evaluations.hip's h(X)): out[z][b][i] = Horner in d_ch[b] over the sources d_first[z] ..
// d_first[z + 1) of d_srcs, z < lists, n coefficients each, list z at d_out + z * batch * n elements; device pointers, Montgomery
// form.  Enqueues only.
int mo_combine(bzh_ctx* ctx, int field, const MoSrc* d_srcs, const uint32_t* d_first, const uint32_t* d_ch, size_t n, size_t batch,
               size_t lists, uint32_t* d_out);
// evaluations.hip: bzh_evaluations_batch_device for a caller that holds ctx->mu and has made every argument check.  What
// bzh_evaluations_plan says about the queries comes in as EvPlan; every data pointer is device memory, 16-byte aligned; d_polys
// (batch x npolys_own x n), d_shared (npolys_shared x n), the pieces (piece i of proof b at d_h + (b * h_stride + i * n) elements)
// and d_out_h (batch x n) Montgomery; d_h_blinds, d_out_points (batch x nrot), d_out_evals (batch x nqueries, or null) and
// d_out_h_blind in `form`; d_scratch: evaluations_scratch_bytes() bytes that no callee takes (WS_STAGE).  Enqueues only.
struct EvPlan {
    size_t npolys_own = 0, npolys_shared = 0, nqueries = 0, nrot = 0;
    std::vector<int32_t> rotations;                              // the nrot distinct rotations, first-seen order
    std::vector<uint32_t> poly_of_query, point_of_query;         // per query: its polynomial, its index into rotations
    std::vector<uint32_t> poly_order, rot_count;                 // as bzh_evaluations_plan fills them
};
size_t evaluations_scratch_bytes(const EvPlan& plan, size_t batch, size_t npieces);
int evaluations_device(bzh_ctx* ctx, int curve, size_t batch, unsigned k, const EvPlan& plan, const uint32_t* d_polys, const uint32_t* d_shared,
                       const uint32_t* d_h, size_t npieces, size_t h_stride, const uint32_t* d_h_blinds, int form, bzh_transcript_batch* tb,
                       uint32_t* d_out_points, uint32_t* d_out_evals, uint32_t* d_out_h, uint32_t* d_out_h_blind, void* d_scratch);
// the same with every polynomial where it lies: srcs (host memory) holds one MoSrc per polynomial id, own ids first.
// evaluations_device builds this table from its dense operands.
int evaluations_device_srcs(bzh_ctx* ctx, int curve, size_t batch, unsigned k, const EvPlan& plan, const MoSrc* srcs, const uint32_t* d_h,
                            size_t npieces, size_t h_stride, const uint32_t* d_h_blinds, int form, bzh_transcript_batch* tb,
                            uint32_t* d_out_points, uint32_t* d_out_evals, uint32_t* d_out_h, uint32_t* d_out_h_blind, void* d_scratch);
// prove_device.hip: the two lane kernels of bzh_prove_batch_device (the call itself reads the key: csrc/prove_device.hpp); device
// pointers, enqueue only.  prove_device_blinds: d_out[b][nown] = the blind of every opened polynomial of proof b, gathered through
// the `nsrc` entries of d_srcs (PdBlindSrc, prove_device_scalars.hpp; a null pointer stands for Montgomery 1).
// prove_device_status: d_slot[b] = {the four leaves' bytes of proof b folded into bits 0 .. 3, proof_len} (two words per proof).
int prove_device_blinds(bzh_ctx* ctx, int field, const void* d_srcs, size_t nsrc, size_t nown, size_t batch, uint32_t* d_out);
int prove_device_status(bzh_ctx* ctx, const uint8_t* d_leaf, size_t leaf_stride, size_t batch, uint32_t proof_len, uint32_t* d_slot);
// prove_game.hip: the two lane kernels of bzh_prove_shots_device / bzh_prove_boards_device (the call itself reads the key:
// csrc/prove_game.hpp); device pointers, 16-byte aligned, enqueue only.  prove_game_instances: from d_cm[b][16] (the commitment's
// canonical x || y) and, for Shot, the low 128 bits of words 8 .. 11 and 12 .. 15 of d_in[b][in_words], the public inputs of proof
// b as d_mont[b][rows] (Montgomery) and d_canon[b][rows] (canonical), rows = 4 (Shot) or 2 (Board).  prove_game_status: bits
// 4 .. 6 of d_slot[b][0] |= d_syn_status[b] << 4 (d_slot: prove_device_status's two words per proof).
int prove_game_instances(bzh_ctx* ctx, bool shot, const uint32_t* d_cm, const uint64_t* d_in, size_t in_words, size_t batch, uint32_t* d_mont,
                         uint32_t* d_canon);
int prove_game_status(bzh_ctx* ctx, const uint32_t* d_syn_status, size_t batch, uint32_t* d_slot);
// vanishing.hip: the two kernels of bzh_vanishing_batch_device (the call itself reads the key: csrc/vanishing_device.hpp); device
// pointers, 16-byte aligned unless said otherwise; enqueue only.
// vanishing_consts: d_table[b][i] = value_i * challenge_b^exponent_i over the nconsts descriptors at d_descs (bzh_vanishing_const);
// d_theta / d_beta / d_gamma batch elements each in `form`, d_y Montgomery; a constant takes 8 saturated words, or with planes29
// the unsaturated quotient kernel's 12-word slot.  vanishing_degree: bit 0 of d_status[b] (any alignment, may be null) and of
// d_sticky[b] is set when an element [first, pitch) of row b of d_h (rows of `pitch` elements) is non-zero; first >= pitch
// launches nothing.
int vanishing_consts(bzh_ctx* ctx, int field, const void* d_descs, size_t nconsts, size_t batch, const uint32_t* d_theta,
                     const uint32_t* d_beta, const uint32_t* d_gamma, const uint32_t* d_y, int form, bool planes29, uint32_t* d_table);
int vanishing_degree(bzh_ctx* ctx, const uint32_t* d_h, size_t first, size_t pitch, size_t batch, uint8_t* d_status, uint8_t* d_sticky);
// products.hip: the two kernels of bzh_grand_products_batch_device (the call itself reads the key: csrc/products_device.hpp); device
// pointers, 16-byte aligned unless said otherwise, Montgomery unless said otherwise; enqueue only.
// products_factors: the numerator d_num[p][b][row] and denominator d_den[p][b][row] of every grand product's factors, nsets
// permutation sets and then nl lookups, from the column table d_cols (GpCol) / d_prods (GpProd, one per product) of
// products_scalars.hpp; d_beta / d_gamma batch elements each in `form`.  products_finish: d_raw is that buffer after the inversion,
// the product and the exclusive scan; d_drawn[b][p][bf + 1] the reduced draws (the bf blinding rows, then the blind);
// d_z[b][p][row] = raw * the set's carry, the draws in rows n - bf .. n - 1; d_blinds[b][p]; d_status[b] (any alignment, may be
// null) = bit 0: a product of proof b does not close, ORed into d_sticky[b].
int products_factors(bzh_ctx* ctx, int field, const void* d_cols, const void* d_prods, size_t nsets, size_t nl, size_t n, size_t batch,
                     const uint32_t* d_beta, const uint32_t* d_gamma, int form, uint32_t* d_num, uint32_t* d_den);
int products_finish(bzh_ctx* ctx, int field, const uint32_t* d_raw, const uint32_t* d_drawn, size_t n, size_t usable, size_t bf, size_t nsets,
                    size_t nl, size_t batch, uint32_t* d_z, uint32_t* d_blinds, uint8_t* d_status, uint8_t* d_sticky);
// commitments.hip: the four kernels of bzh_commitments_batch_device (the call itself reads the key: csrc/commitments_device.hpp);
// device pointers, 16-byte aligned unless said otherwise, Montgomery unless said otherwise; enqueue only.
// commitments_place: d_out_adv[b][na][n] = the caller's d_advice[b][na][n] (in `form`) below `usable`, from there on the drawn
// blinding rows d_drawn[b][c * (n - usable) ..] (d_drawn: batch rows of nd elements); d_out_blinds[b][na] = the na draws after
// them; d_out_inst[b][ni][n] = d_instances[b][ni][inst_rows] (in `form`; not read when inst_rows is 0) and zeros.
// commitments_consts: every entry of the CmConst list at d_descs (commitments_scalars.hpp) into its program's table, theta
// (batch elements) in `form`.  commitments_lookup_finish: per pair b * nl + l the 2 (n - usable) drawn rows from
// d_drawn[b][first + l * (2 (n - usable) + 2) ..] into rows usable .. n - 1 of d_permuted[pair][2][n], the two draws after them
// into d_blinds[pair][2]; d_status[b] (any alignment, may be null) = bit 0: one of d_words[b * nl ..][nl] is non-zero, ORed into
// d_sticky[b].  commitments_scalar_rows: d_scalars[v] = (d_evals[v][n] | 0 | d_blinds[v] [| 0]), cols = n + 2 or n + 3.
int commitments_place(bzh_ctx* ctx, int field, const uint32_t* d_advice, const uint32_t* d_instances, size_t inst_rows,
                      const uint32_t* d_drawn, size_t nd, size_t n, size_t usable, size_t na, size_t ni, size_t batch, int form,
                      uint32_t* d_out_adv, uint32_t* d_out_inst, uint32_t* d_out_blinds);
int commitments_consts(bzh_ctx* ctx, int field, const void* d_descs, size_t ndescs, size_t batch, const uint32_t* d_theta, int form);
int commitments_lookup_finish(bzh_ctx* ctx, int field, const uint32_t* d_drawn, size_t nd, size_t first, size_t n, size_t usable, size_t nl,
                              size_t batch, const int32_t* d_words, uint32_t* d_permuted, uint32_t* d_blinds, uint8_t* d_status,
                              uint8_t* d_sticky);
int commitments_scalar_rows(bzh_ctx* ctx, int field, const uint32_t* d_evals, const uint32_t* d_blinds, size_t n, size_t cols, size_t count,
                            uint32_t* d_scalars);
int ipa_verify(bzh_ctx* ctx, const bzh_bases* bases, const uint64_t* commitment_xy, const uint64_t* x3, const uint64_t* v,
               const uint8_t* proof, size_t proof_len, bzh_transcript* tr, const uint64_t* g0_u_w_xy);
int ipa_check_batch(bzh_ctx* ctx, const bzh_bases* bases, size_t batch, size_t nl, const uint64_t* lc_pts, const uint64_t* lc_scal,
                    const uint64_t* cu, int* ok);
// the same check with its operands already on the device (the verifier's device pass): d_pts batch x nl affine canonical points
// (taken to Montgomery form in place), d_scal canonical, d_cu batch x (k + 1) Montgomery; 16-byte aligned
// (pts_montgomery: as for ipa_check_sums_device below)
int ipa_check_batch_device(bzh_ctx* ctx, const bzh_bases* bases, size_t batch, size_t nl, uint32_t* d_pts, const uint32_t* d_scal,
                           const uint32_t* d_cu, int* ok, bool pts_montgomery = false);
// the same launches without the read-back and the host comparison: *d_sums = the batch right sides' Jacobian points, then the batch
// left sides', Montgomery, 24 words each, in WS_IPA -- valid until the next holder of that slot.  Enqueues only (msm_run's own waits
// aside).  pts_montgomery: d_pts are in Montgomery form already (ipa_check_accumulated_device ran on them) and are not converted.
int ipa_check_sums_device(bzh_ctx* ctx, const bzh_bases* bases, size_t batch, size_t nl, uint32_t* d_pts, const uint32_t* d_scal,
                          const uint32_t* d_cu, const uint32_t** d_sums, bool pts_montgomery = false);
// The accumulated check: ONE verdict for the whole batch, d_ok[0] = 1 when
//     sum_b w'_b * ( sum_i d_scal[b][i] * d_pts[b][i] )  ==  < sum_b w'_b * c_b * s(u_b), G >,   w'_b = d_exclude[b] ? 0 : d_weights[b].
// The operands are ipa_check_sums_device's (d_pts taken to Montgomery form in place); d_weights batch elements, Montgomery;
// d_exclude batch bytes, any alignment, or null; an excluded opening's rows are not read.  Two MSMs whatever the batch: n + 2 terms
// against `bases`, batch * nl terms on the ad-hoc table.  WS_IPA: O(n + batch * nl).  Enqueues only (msm_run's own waits aside).
int ipa_check_accumulated_device(bzh_ctx* ctx, const bzh_bases* bases, size_t batch, size_t nl, uint32_t* d_pts, const uint32_t* d_scal,
                                 const uint32_t* d_cu, const uint32_t* d_weights, const uint8_t* d_exclude, uint8_t* d_ok);
// the same with host operands (bzh_ipa_check_accumulated): lc_pts, lc_scal, cu and weights canonical; stages in WS_STAGE
int ipa_check_accumulated(bzh_ctx* ctx, const bzh_bases* bases, size_t batch, size_t nl, const uint64_t* lc_pts, const uint64_t* lc_scal,
                          const uint64_t* cu, const uint64_t* weights, const uint8_t* exclude, int* ok);
bool point_decompress(int curve, const uint8_t* in, uint64_t* xy_canonical);
// sqrt_decompress.hip (device pointers, 16-byte aligned; elements and points in `form`).  batch_sqrt_run: in place, d_status[i] = 1
// for a square (root written), 0 otherwise (element untouched).  decompress_run: n x 32 bytes -> n affine points x || y and one
// BZH_POINT_* byte each; zeros unless BZH_POINT_OK.
int batch_sqrt_run(bzh_ctx* ctx, int field, uint32_t* d_data, size_t count, int form, uint8_t* d_status);
int decompress_run(bzh_ctx* ctx, int curve, const uint32_t* d_in, size_t n, int form, uint32_t* d_out_xy, uint8_t* d_status);
// normalize_compress.hip (device pointers, 16-byte aligned; enqueues only): bzh_batch_normalize's launch.  d_out_xy, d_out32 and
// d_status may each be null, d_out_xy and d_out32 not both.
int normalize_run(bzh_ctx* ctx, int curve, const void* d_xyz, size_t n, int form, void* d_out_xy, void* d_out32, uint8_t* d_status);
// hash_to_curve.hip: Params::new's g[first .. first + count) as Montgomery affine points and one BZH_POINT_* byte each, into device
// memory (16-byte aligned); enqueues only, the caller holds ctx->mu.  ev: null, or three events recorded before k_hash_to_field,
// between the two kernels and after k_map_to_curve.
int h2c_generators_run(bzh_ctx* ctx, uint32_t first, size_t count, uint32_t* d_out_xy, uint8_t* d_status, hipEvent_t* ev = nullptr);
// transcript_batch.hip: a device-resident bzh_transcript_batch for a caller that holds ctx->mu; device operands, enqueue only.
// kind 0 / 1: common / write points (d_pre: a BZH_POINT_* byte per point at [b * stride + i], or null), kind 2 / 3: common / write
// scalars; item i of transcript b lies at d_base + (b * stride + i) items -- stride 0 gives every transcript the same items.  A
// write appends to the proofs without a capacity check: the caller has made it (tb_info).  tb_write_jacobian_locked is
// bzh_transcript_batch_write_jacobian for device operands; with kind 0 the normalised points are absorbed as COMMON points and
// nothing goes into the proofs.  tb_squeeze_locked writes batch x 32 bytes.  tb_free_locked waits for the stream.
struct TbInfo {
    bzh_ctx* ctx;   // null: host-resident
    int curve;
    size_t batch, proof_cap, proof_len;
};
// proof_cap: room per transcript for written messages (0: a verifier's batch, which writes none).  tb_reserve_points_locked sizes
// the batch's normalise scratch for writes of up to `points` Jacobian points each, so that no later write has to grow it (growing
// waits for the stream).  tb_proofs_device: the proofs in device memory, `*pstride` bytes apart.
int tb_new_locked(bzh_ctx* ctx, int curve, size_t batch, bzh_transcript_batch** out, size_t proof_cap = 0);
int tb_reserve_points_locked(bzh_transcript_batch* tb, size_t points);
const uint8_t* tb_proofs_device(const bzh_transcript_batch* tb, size_t* pstride);
void tb_free_locked(bzh_transcript_batch* tb);
int tb_absorb_locked(bzh_transcript_batch* tb, int kind, const void* d_base, size_t count, size_t stride, int form, const uint8_t* d_pre);
int tb_write_jacobian_locked(bzh_transcript_batch* tb, const void* d_xyz, size_t count, size_t stride, int form, int kind = 1);
int tb_squeeze_locked(bzh_transcript_batch* tb, int form, uint32_t* d_out);
const uint8_t* tb_status_device(const bzh_transcript_batch* tb);
uint8_t* tb_status_device_mut(bzh_transcript_batch* tb);   // for a kernel of the caller's that marks a transcript (vanishing.hip)
TbInfo tb_info(const bzh_transcript_batch* tb);
// verify_pass.hip: the kernels of the verifier's device pass (BZH_VERIFY_PASS_DEVICE); device pointers, enqueue only
struct VerifyPassArgs {
    size_t batch = 0, pstride = 0;           // proofs: batch rows of pstride bytes (a multiple of 32)
    const uint8_t* d_proofs = nullptr;
    // the key's program in device memory (verify_program.hpp)
    const uint32_t *d_ops = nullptr, *d_consts = nullptr, *d_ev_offsets = nullptr, *d_out_slots = nullptr, *d_pt_src = nullptr, *d_vp_offsets = nullptr;
    uint32_t nops = 0, nslots = 0, nch = 0, nev = 0, nl_cap = 0, ncu = 0, np = 0, ni = 0;
    const uint32_t* d_ch = nullptr;          // nch x batch challenges, Montgomery
    uint32_t* d_slots = nullptr;             // nslots x 8 x batch words
    uint32_t *d_lc_scal = nullptr, *d_cu = nullptr, *d_flags = nullptr;   // batch x nl_cap canonical, batch x ncu Montgomery, batch words
    // the points: decompressed proof points (batch x np) with their status bytes, the key's fixed | permutation commitments, the
    // instance commitments (batch x ni), G_0 U W; all affine canonical
    const uint32_t *d_proof_xy = nullptr, *d_key_xy = nullptr, *d_inst_xy = nullptr, *d_srs_xy = nullptr;
    uint32_t nfixed = 0;
    const uint8_t *d_point_status = nullptr, *d_tb_status = nullptr, *d_pre_reject = nullptr;
    uint32_t* d_lc_pts = nullptr;            // batch x nl_cap points
    uint8_t* d_reject = nullptr;             // batch bytes
};
int vp_gather_points(bzh_ctx* ctx, const VerifyPassArgs& a, uint32_t* d_out32);
int vp_scalars_run(bzh_ctx* ctx, int curve, const VerifyPassArgs& a);
int vp_assemble_run(bzh_ctx* ctx, const VerifyPassArgs& a);
// verify_records.hip: the four lane kernels of bzh_verify_records_device (the call itself reads the key: csrc/verifier.hpp); device
// pointers, 16-byte aligned unless said otherwise; enqueue only.  Lane bodies and what each argument holds: verify_records.hpp.
struct VerifyRecordsArgs {
    size_t batch = 0, rstride = 0, pstride = 0;   // records rstride bytes apart, proof rows pstride bytes apart: multiples of 16
    uint32_t n_inputs = 0, proof_len = 0;         // what a record must say; 144 + proof_len <= rstride, proof_len <= pstride
    const uint8_t* d_records = nullptr;
    uint32_t* d_inst = nullptr;                   // batch x n_inputs elements, Montgomery
    uint8_t* d_rows = nullptr;                    // batch x pstride bytes
    uint8_t* d_pre = nullptr;                     // batch bytes, any alignment
};
int verify_records_parse(bzh_ctx* ctx, int curve, const VerifyRecordsArgs& a);
// d_table: row 0 of the SRS window table (n_srs affine Montgomery points); d_given: 3 canonical points or null; d_out_xy: G_0 U W
// canonical; d_mismatch: 3 bytes, any alignment
int verify_records_srs(bzh_ctx* ctx, int curve, const uint32_t* d_table, size_t n_srs, const uint32_t* d_given, uint32_t* d_out_xy,
                       uint8_t* d_mismatch);
// d_jac: batch Jacobian sums, Montgomery in and canonical out; d_w_xy: W, affine Montgomery
int verify_records_add_w(bzh_ctx* ctx, int curve, uint32_t* d_jac, const uint32_t* d_w_xy, size_t batch);
// d_sums: ipa_check_sums_device's; d_out: results at [b], status at [pitch + b], any alignment
int verify_records_result(bzh_ctx* ctx, int curve, const uint32_t* d_sums, size_t batch, const uint8_t* d_pre, const uint8_t* d_reject,
                          uint8_t* d_out, size_t pitch);

}  // namespace bzh
