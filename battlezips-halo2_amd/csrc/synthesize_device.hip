// Witness synthesis on the device (bzh_synthesize_{shot,board}_with, BZH_SYNTH_DEVICE): three kernels over the lane bodies of
// csrc/synthesize_device.hpp, straight into the (batch, num_advice, 2^k) advice tensor in Montgomery form.
//   k_syn_cells      one lane per (proof, row < rows_used): every cell that is an integer of the proof's input words
//   k_syn_mulfixed   one block of two waves per (proof, base), lane = window (85 windows do not fit one wave64): table look-up,
//                    the 84 running sums by a 7-level scan with the complete XYZZ addition over an LDS tile, every lane's own
//                    fe_inv_ct for the affine cells, the exceptional-case test on the normalised neighbours
//   k_syn_ecc_tail   one lane per proof: the three complete additions, Shot's native commitment cells, the commitment
// The tensor is zeroed by a memset on the same stream first; a region's constants 0 and the rows >= rows_used are that fill.
// One staged upload (layout + inputs) and one read-back (status words + commitments) per call; the read-back is the call's only
// stream synchronisation.  synth_device_enqueue is the same call without that read-back, for a caller that goes on working on the
// device (the game-input prover, csrc/prove_game.hpp): the status words and the commitments go to device pointers of its own.
#include <cstdio>

#include "ctx.hpp"
#include "synthesize_device.hpp"

using namespace bzh;

namespace {

__global__ void __launch_bounds__(256) k_syn_cells(const SynLayout* __restrict__ L, const uint64_t* __restrict__ in, size_t batch, uint32_t* __restrict__ adv) {
    const size_t per = (L->rows_used + 255) / 256, proof = blockIdx.x / per, row = (blockIdx.x % per) * (size_t)256 + threadIdx.x;
    if (row >= L->rows_used || proof >= batch) return;
    syn_cells_row(L, in + proof * L->in_words, row, adv + proof * L->num_advice * (size_t)L->n * 8);
}

constexpr int SYN_SCAN = 128;   // two waves: 85 windows, 7 levels

__global__ void __launch_bounds__(SYN_SCAN) k_syn_mulfixed(const SynLayout* __restrict__ L, const uint32_t* __restrict__ tbl, const uint64_t* __restrict__ in,
                                                           uint32_t* __restrict__ adv, uint32_t* __restrict__ flags) {
    __shared__ SynXyzz tile[SYN_SCAN];
    const unsigned t = threadIdx.x;
    const size_t proof = blockIdx.x >> 1;
    const int base = (int)(blockIdx.x & 1);
    const uint64_t* pin = in + proof * L->in_words;
    uint32_t* padv = adv + proof * L->num_advice * (size_t)L->n * 8;
    uint32_t flag = 0;
    SynAff m;
    m.x = fe_zero<SynP>(), m.y = fe_zero<SynP>();
    if (t < (unsigned)SYN_NW) m = syn_mulfixed_gather(L, tbl, pin, base, t, padv, &flag);
    // windows 0..83 are summed; the last window's point meets the sum in the complete addition of the tail
    SynXyzz s = t < (unsigned)SYN_NW - 1 ? xyzz_from_affine(m) : xyzz_identity<SynP>();
    tile[t] = s;
    __syncthreads();
#pragma unroll 1
    for (unsigned d = 1; d < (unsigned)SYN_SCAN; d <<= 1) {
        SynXyzz o = xyzz_identity<SynP>();
        if (t >= d) o = tile[t - d];
        __syncthreads();
        s = syn_xyzz_add(o, s);
        tile[t] = s;
        __syncthreads();
    }
    SynAff a;
    a.x = fe_zero<SynP>(), a.y = fe_zero<SynP>();
    if (t < (unsigned)SYN_NW - 1) a = syn_mulfixed_finish(L, base, t, s, padv);
    tile[t].x = a.x;
    tile[t].y = a.y;
    __syncthreads();
    if (t >= 1 && t < (unsigned)SYN_NW - 1) {
        SynAff prev;
        prev.x = tile[t - 1].x, prev.y = tile[t - 1].y;
        flag |= syn_incomplete_exceptional(prev, m);
    }
    const int exc = __syncthreads_or((int)(flag & SYN_ST_EXCEPTIONAL)), x0 = __syncthreads_or((int)(flag & SYN_ST_WINDOW_X0));
    if (t == 0) flags[blockIdx.x] = (exc ? SYN_ST_EXCEPTIONAL : 0u) | (x0 ? SYN_ST_WINDOW_X0 : 0u);
}

// out: batch status words, then batch x 16 words of commitments (the start of the commitments is 16-byte aligned)
__global__ void __launch_bounds__(64) k_syn_ecc_tail(const SynLayout* __restrict__ L, const uint64_t* __restrict__ in, size_t batch, uint32_t* __restrict__ adv,
                                                     const uint32_t* __restrict__ flags, uint32_t* __restrict__ status, uint32_t* __restrict__ inst) {
    const size_t proof = blockIdx.x * (size_t)64 + threadIdx.x;
    if (proof >= batch) return;
    const uint32_t st = syn_ecc_tail(L, in + proof * L->in_words, adv + proof * L->num_advice * (size_t)L->n * 8, inst + proof * 16);
    status[proof] = st | flags[2 * proof] | flags[2 * proof + 1];
}

static size_t up16(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace

namespace bzh {

// WS_STAGE while the three kernels run: layout | inputs | flags (2 per proof), and for synth_device_run status (1 per proof) |
// commitments (16 words per proof) after them
struct SynStage {
    size_t o_in, in_bytes, o_flags, o_status, status_bytes, o_inst;
};
static SynStage synth_stage(const SynLayout& L, size_t batch) {
    SynStage s;
    s.o_in = up16(sizeof(SynLayout)), s.in_bytes = batch * L.in_words * 8, s.o_flags = s.o_in + up16(s.in_bytes);
    s.o_status = s.o_flags + up16(batch * 8), s.status_bytes = up16(batch * 4), s.o_inst = s.o_status + s.status_bytes;
    return s;
}

int synth_device_enqueue(bzh_ctx* ctx, const SynRun& run, uint32_t* d_status, uint32_t* d_commitments, const uint64_t** d_inputs,
                         hipEvent_t* ev) {
    const SynLayout& L = *run.layout;
    const size_t batch = run.batch;
    if (!ctx->syn_tbl) {
        uint32_t* tbl = nullptr;
        const size_t bytes = SYN_TBL_ENTRIES * SYN_TBL_WORDS * 4;
        BZH_HIP_TRY(ctx, hipMalloc((void**)&tbl, bytes));
        const int rc = h2d_small(ctx, tbl, run.table, bytes);
        if (rc) {
            (void)hipFree(tbl);
            return rc;
        }
        ctx->syn_tbl = tbl;
    }
    // the synthesis kernels below (and what the caller enqueues on *d_inputs right after them) are all that runs while the slot is
    // held.  The slot keeps synth_device_run's size whoever calls, so that the two forms never grow it in turns
    const SynStage S = synth_stage(L, batch);
    void* ws = nullptr;
    BZH_TRY(ws_ensure(ctx, WS_STAGE, S.o_inst + batch * 64, &ws));
    char* d = (char*)ws;
    char* slot = nullptr;
    BZH_TRY(h2d_stage(ctx, S.o_flags, &slot));
    memset(slot, 0, S.o_flags);
    memcpy(slot, &L, sizeof(SynLayout));
    memcpy(slot + S.o_in, run.inputs, S.in_bytes);
    BZH_TRY(h2d_commit(ctx, d, slot, S.o_flags));
    const SynLayout* d_L = (const SynLayout*)d;
    const uint64_t* d_in = (const uint64_t*)(d + S.o_in);
    uint32_t* d_flags = (uint32_t*)(d + S.o_flags);
    auto mark = [&](int i) {
        if (ev) (void)hipEventRecord(ev[i], ctx->stream);
    };
    mark(0);
    BZH_HIP_TRY(ctx, hipMemsetAsync(run.d_advice, 0, batch * L.num_advice * (size_t)L.n * 32, ctx->stream));
    mark(1);
    {
        ScopedTimer timer(ctx, BZH_T_POLY);
        hipLaunchKernelGGL(k_syn_cells, dim3((unsigned)(batch * ((L.rows_used + 255) / 256))), dim3(256), 0, ctx->stream, d_L, d_in, batch, run.d_advice);
        mark(2);
        hipLaunchKernelGGL(k_syn_mulfixed, dim3((unsigned)(2 * batch)), dim3(SYN_SCAN), 0, ctx->stream, d_L, (const uint32_t*)ctx->syn_tbl, d_in, run.d_advice,
                           d_flags);
        mark(3);
        hipLaunchKernelGGL(k_syn_ecc_tail, dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, ctx->stream, d_L, d_in, batch, run.d_advice,
                           (const uint32_t*)d_flags, d_status, d_commitments);
        mark(4);
    }
    BZH_HIP_TRY(ctx, hipGetLastError());
    if (d_inputs) *d_inputs = d_in;
    return BZH_OK;
}

int synth_device_run(bzh_ctx* ctx, const SynRun& run) {
    const size_t batch = run.batch;
    const SynStage S = synth_stage(*run.layout, batch);
    const size_t rb_bytes = S.status_bytes + batch * 64;
    void* ws = nullptr;
    BZH_TRY(ws_ensure(ctx, WS_STAGE, S.o_inst + batch * 64, &ws));   // (the enqueue asks for the same bytes: the slot does not move)
    char* d = (char*)ws;
    uint32_t *d_status = (uint32_t*)(d + S.o_status), *d_inst = (uint32_t*)(d + S.o_inst);
    // BZH_PROVE_TRACE=1: the three kernels' times by events, on stderr (tools/ubench_synthesize.py reads the line)
    const bool trace = getenv("BZH_PROVE_TRACE") != nullptr;
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    if (trace) {
        for (auto& e : ev) BZH_HIP_TRY(ctx, hipEventCreate(&e));
    }
    BZH_TRY(synth_device_enqueue(ctx, run, d_status, d_inst, nullptr, trace ? ev : nullptr));
    std::vector<uint32_t> rb(rb_bytes / 4);
    BZH_TRY(d2h_async(ctx, rb.data(), d_status, rb_bytes));
    BZH_TRY(d2h_finish(ctx));
    if (trace) {
        float ms[4] = {0, 0, 0, 0};
        for (int i = 0; i < 4; i++) (void)hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]);
        fprintf(stderr, "[bzh_synthesize] device batch=%zu zero_fill_ms=%.4f k_syn_cells_ms=%.4f k_syn_mulfixed_ms=%.4f k_syn_ecc_tail_ms=%.4f\n", batch, ms[0],
                ms[1], ms[2], ms[3]);
        for (auto& e : ev) (void)hipEventDestroy(e);
    }
    memcpy(run.status, rb.data(), batch * 4);
    if (run.commitments) memcpy(run.commitments, rb.data() + S.status_bytes / 4, batch * 64);
    return BZH_OK;
}

}  // namespace bzh
