// Part of the whole-proof translation unit (csrc/prove.hip): the VERIFIER -- verify_proof for a batch of proofs.
#pragma once
// ---------------------------------------------------------------------------
// the verifier (halo2_proofs plonk::verify_proof with SingleVerifier, benches/board.rs:80-86): transcript replay,
// expected h(x) from the evaluations, multiopen recombination and the IPA equation.  Host work per proof (threads):
// Blake2b, ~56 point decompressions, a few hundred field operations; device work for the whole batch: the instance
// commitments, one n-term MSM per proof against the SRS table and one small MSM over the proof's own points.
// ---------------------------------------------------------------------------
#include "verify_host.hpp"   // ProofView, PrePoints, HostPassTimes, verify_host: host code only

// The device side of the verifier and of keygen_vk: the shared column helpers (device_columns.hpp), with commitments of blind 1
// against a table the caller names -- the key itself is host data.
template <class C>
struct ColumnCommitter : DeviceColumns<C> {
    using DC = DeviceColumns<C>;
    using SF = typename DC::SF;
    using PB = typename DC::PB;
    using DC::arena;
    using DC::ctx;
    using DC::dalloc;
    using DC::n;
    using DC::read_points;
    using DC::upload;
    using DC::DeviceColumns;

    // Params::commit with blind 1 for `count` polynomials of n coefficients (contiguous) against srs = (g | u | w): affine
    // canonical points out
    int commit(const bzh_bases* srs, const uint32_t* polys, size_t count, std::vector<uint64_t>& xy) {
        return DC::commit(srs, polys, n, count, std::vector<Fe<SF>>(count, fe_one<SF>()), xy);
    }
    // Params::commit_lagrange with blind 1 for `count` columns of which only the first `len` rows are non-zero: `vals` holds
    // count x len values (host, Montgomery), committed against the first len points of g_lagrange by ONE prefix MSM; W (w_xy,
    // affine canonical) is added on the host.  Nothing of size n is allocated.
    int commit_prefix(const bzh_bases* g_lagrange, const Fe<SF>* vals, size_t len, size_t count, const uint64_t* w_xy, std::vector<uint64_t>& xy) {
        xy.assign(count * 8, 0);
        if (!count) return BZH_OK;
        std::vector<uint64_t> aff(count * 8, 0);   // the MSM's results, affine Montgomery ((0,0): identity)
        if (len) {
            ArenaScope scope(arena);
            uint32_t* sc = dalloc(count * len);
            uint32_t* d_out = dalloc(count * 3);
            if (!sc || !d_out) return BZH_E_OOM;
            BZH_TRY(upload(sc, vals, count * len));
            BZH_TRY(msm_run(ctx, g_lagrange, sc, len, count, BZH_FORM_MONTGOMERY, d_out));
            BZH_TRY(read_points(d_out, count, BZH_FORM_MONTGOMERY, aff.data()));
        }
        Affine<PB> w;
        w.x = fe_from_u64<PB>(w_xy, BZH_FORM_CANONICAL);
        w.y = fe_from_u64<PB>(w_xy + 4, BZH_FORM_CANONICAL);
        std::vector<uint64_t> jac(count * 12);
        for (size_t i = 0; i < count; i++) {
            Xyzz<PB> acc = xyzz_identity<PB>();
            Affine<PB> a;
            a.x = fe_from_u64<PB>(&aff[8 * i]);
            a.y = fe_from_u64<PB>(&aff[8 * i + 4]);
            if (!aff_is_id(a)) xyzz_madd(acc, a);
            xyzz_madd(acc, w);
            Fe<PB> X, Y, Z;
            xyzz_to_jacobian(acc, X, Y, Z);
            fe_to_u64<PB>(&jac[12 * i], X);
            fe_to_u64<PB>(&jac[12 * i + 4], Y);
            fe_to_u64<PB>(&jac[12 * i + 8], Z);
        }
        h_jac_to_affine<PB>(jac.data(), count, BZH_FORM_MONTGOMERY, BZH_FORM_CANONICAL, xy.data());
        return BZH_OK;
    }
};

// the instance commitments of a batch, affine canonical, batch x max(ni, 1) points
template <class C>
static int instance_commitments(ColumnCommitter<C>& pv, const KeyShape& key, const bzh_bases* srs, const bzh_bases* g_lagrange, size_t B,
                                const uint64_t* instances, size_t inst_rows, const uint64_t* g0_u_w, std::vector<uint64_t>& inst_xy) {
    using SF = typename CurveInfo<C>::SF;
    const size_t n = key.n;
    const int ni = key.ni;
    inst_xy.assign(B * std::max(ni, 1) * 8, 0);
    if (ni) {
        std::vector<Fe<SF>> hv(B * ni * inst_rows);
        for (size_t i = 0; i < hv.size(); i++) hv[i] = fe_to_mont(fe_from_u64<SF>(instances + 4 * i));
        if (g_lagrange) {
            // Params::commit_lagrange: the inst_rows values of a column against the first inst_rows Lagrange points, plus W
            BZH_TRY(pv.commit_prefix(g_lagrange, hv.data(), inst_rows, B * ni, g0_u_w + 16, inst_xy));
        } else {
            uint32_t* inst = pv.dalloc(B * ni * n);
            uint32_t* inst_polys = pv.dalloc(B * ni * n);
            if (!inst || !inst_polys) return BZH_E_OOM;
            BZH_TRY(pv.zero(inst, B * ni * n));
            if (inst_rows) {
                uint32_t* tmp = pv.dalloc(hv.size());
                if (!tmp) return BZH_E_OOM;
                BZH_TRY(pv.upload(tmp, hv.data(), hv.size()));
                BZH_TRY(pv.copy2d(inst, n, tmp, inst_rows, inst_rows, B * ni));
            }
            BZH_TRY(pv.to_coeff(inst_polys, inst, B * ni));
            BZH_TRY(pv.commit(srs, inst_polys, B * ni, inst_xy));
        }
    }
    return BZH_OK;
}

// verify_proof for a batch.  key: what the verifier reads of a key (a bzh_pk's or a bzh_vk's); srs: (g | u | w) with its window
// table; g_lagrange: (g_lagrange | u | w), or null for instance commitments through the coefficient basis; arena: the (key,
// ctx) workspace; points_on_device: BZH_VERIFY_POINTS_DEVICE.
template <class C>
static int verify_batch_t(bzh_ctx* ctx, const KeyShape& key, const bzh_bases* srs, const bzh_bases* g_lagrange, Arena& arena,
                          bool points_on_device, size_t batch, const uint64_t* instances, size_t inst_rows, const uint8_t* proofs,
                          size_t proof_stride, const size_t* proof_lens, const uint64_t* g0_u_w, int* results) {
    arena.reset();
    ColumnCommitter<C> pv(ctx, key, arena);
    const size_t B = batch;
    const int ni = key.ni;
    // BZH_PROVE_TRACE=1: where the call's wall time goes, on stderr (tools/ubench_verify_points.py reads these lines)
    const bool trace = getenv("BZH_PROVE_TRACE") != nullptr;
    auto t_last = std::chrono::steady_clock::now();
    auto mark = [&](const char* name) {
        if (!trace) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[bzh_verify_batch] %-22s %8.3f ms\n", name, std::chrono::duration<double, std::milli>(now - t_last).count());
        t_last = now;
    };
    // BZH_VERIFY_POINTS_DEVICE: the 32-byte strings of every point of every proof, gathered by the key's offset list, go up in
    // one copy and through one k_decompress launch; points and statuses come back with the instance commitments' read-back.
    static const std::vector<uint32_t> no_offsets;
    const std::vector<uint32_t>& vp_offs = points_on_device ? key.vp_offsets : no_offsets;
    const size_t np = vp_offs.size(), np_all = B * np, np_pad = (np_all + 15) & ~(size_t)15;
    std::vector<uint64_t> pre_xy;
    std::vector<uint8_t> pre_st;
    hipEvent_t ev_a = nullptr, ev_b = nullptr;
    if (np) {
        uint32_t* d_in = (uint32_t*)arena.alloc(np_all * 32);
        uint32_t* d_xy = (uint32_t*)arena.alloc(np_all * 64);
        uint8_t* d_st = (uint8_t*)arena.alloc(np_pad);
        if (!d_in || !d_xy || !d_st) return BZH_E_OOM;
        char* slot = nullptr;
        BZH_TRY(h2d_stage(ctx, np_all * 32, &slot));
        for (size_t b = 0; b < B; b++)
            for (size_t i = 0; i < np; i++) {
                char* dst = slot + (b * np + i) * 32;
                if ((size_t)vp_offs[i] + 32 <= proof_lens[b])
                    memcpy(dst, proofs + b * proof_stride + vp_offs[i], 32);
                else
                    memset(dst, 0, 32);   // past the end of a short proof: marked invalid below
            }
        BZH_TRY(h2d_commit(ctx, d_in, slot, np_all * 32));
        if (trace && hipEventCreate(&ev_a) == hipSuccess && hipEventCreate(&ev_b) == hipSuccess) (void)hipEventRecord(ev_a, ctx->stream);
        BZH_TRY(decompress_run(ctx, C::id, d_in, np_all, BZH_FORM_CANONICAL, d_xy, d_st));
        if (ev_b) (void)hipEventRecord(ev_b, ctx->stream);
        pre_xy.resize(np_all * 8);
        pre_st.resize(np_pad);
        BZH_TRY(d2h_async(ctx, pre_xy.data(), d_xy, np_all * 64));
        BZH_TRY(d2h_async(ctx, pre_st.data(), d_st, np_pad));
        mark("vp:stage+launch");
    }
    // instance commitments of the whole batch (the verifier recomputes them, as upstream does for IPA)
    std::vector<uint64_t> inst_xy;
    BZH_TRY(instance_commitments<C>(pv, key, srs, g_lagrange, B, instances, inst_rows, g0_u_w, inst_xy));
    mark("instance commitments");
    if (np) {
        BZH_TRY(d2h_finish(ctx));   // (already landed when a commitment was read back)
        for (size_t b = 0; b < B; b++)
            for (size_t i = 0; i < np; i++)
                if ((size_t)vp_offs[i] + 32 > proof_lens[b]) pre_st[b * np + i] = BZH_POINT_INVALID;
        if (ev_b) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, ev_a, ev_b) == hipSuccess)
                fprintf(stderr, "[bzh_verify_batch] %-22s %8.3f ms  (%zu points)\n", "vp:k_decompress", (double)ms, np_all);
        }
        if (ev_a) (void)hipEventDestroy(ev_a);
        if (ev_b) (void)hipEventDestroy(ev_b);
        mark("vp:read-back");
    }
    // host pass, one thread per proof
    const size_t nl_cap = vp_nl_cap(key);
    std::vector<ProofView<C>> views(B);
    {
        const size_t nthreads = std::min<size_t>({B, (size_t)host_thread_budget(), (size_t)32});
        std::vector<HostPassTimes> times(trace ? nthreads : 0);
        std::vector<std::thread> th;
        for (size_t t = 0; t < nthreads; t++)
            th.emplace_back([&, t]() {
                const auto t0 = std::chrono::steady_clock::now();
                for (size_t b = t; b < B; b += nthreads) {
                    PrePoints pre{vp_offs.data(), np, np ? &pre_xy[b * np * 8] : nullptr, np ? &pre_st[b * np] : nullptr};
                    verify_host<C>(key, &inst_xy[b * std::max(ni, 1) * 8], proofs + b * proof_stride, proof_lens[b], nl_cap, views[b],
                                   np ? &pre : nullptr, trace ? &times[t] : nullptr);
                }
                if (trace) times[t].total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            });
        for (auto& t : th) t.join();
        if (trace) {   // thread-summed split of the host pass: point decompression against everything else
            double dec = 0, tot = 0;
            for (auto& t : times) dec += t.decompress_ms, tot += t.total_ms;
            fprintf(stderr, "[bzh_verify_batch] %-22s %8.3f ms  (sum over %zu threads)\n", "vp:host decompress", dec, nthreads);
            fprintf(stderr, "[bzh_verify_batch] %-22s %8.3f ms  (sum over %zu threads)\n", "vp:host rest", tot - dec, nthreads);
        }
        mark("host pass");
    }
    // device pass over the proofs that parsed; the others are rejected outright
    std::vector<size_t> live;
    for (size_t b = 0; b < B; b++) {
        results[b] = 0;
        if (views[b].ok) live.push_back(b);
    }
    if (live.empty()) return BZH_OK;
    const size_t Bl = live.size(), kk = key.k;
    std::vector<uint64_t> lc_pts(Bl * nl_cap * 8), lc_scal(Bl * nl_cap * 4), cu(Bl * (kk + 1) * 4);
    for (size_t j = 0; j < Bl; j++) {
        ProofView<C>& v = views[live[j]];
        memcpy(&v.lc_pts[(nl_cap - 3) * 8], g0_u_w, 3 * 64);
        memcpy(&lc_pts[j * nl_cap * 8], v.lc_pts.data(), nl_cap * 64);
        memcpy(&lc_scal[j * nl_cap * 4], v.lc_scal.data(), nl_cap * 32);
        memcpy(&cu[j * (kk + 1) * 4], v.cu.data(), (kk + 1) * 32);
    }
    std::vector<int> ok(Bl, 0);
    BZH_TRY(ipa_check_batch(ctx, srs, Bl, nl_cap, lc_pts.data(), lc_scal.data(), cu.data(), ok.data()));
    for (size_t j = 0; j < Bl; j++) results[live[j]] = ok[j];
    mark("ipa check");
    return BZH_OK;
}

// verify_proof for a batch with the per-proof pass on the device (BZH_VERIFY_PASS_DEVICE): after the instance commitments, the
// proof bytes go up once and nothing comes back but the two Jacobian sums per proof and one reject byte per proof.  Between the
// upload and that read-back the stream is not waited for (msm_run's own waits aside, and a workspace that has to grow on a first
// call): one decompress_run over key.vp_offsets, one bzh_transcript_batch walking key.vprog.schedule, k_vp_scalars over the
// key's tape, the gather of the left side's points, ipa_check_batch_device.  A proof whose length is not the key's is rejected
// here and its row is zero-filled.
// The pass has two front doors, verify_batch_device_t (instances and proofs from the caller's arrays, the instance commitments through
// the host) and verify_records_t (records, everything on the device); what follows "instances and proofs are in HBM" is one body,
// verify_pass_enqueue_t.
static bool verify_pass_has_program(bzh_ctx* ctx, const KeyShape& key) {
    if (key.vprog.ok) return true;
    ctx->last_error = "bzh_verify_batch: this key's host pass has no device program (BZH_VERIFY_PASS_DEVICE)";
    return false;
}
// the proof rows' pitch in HBM
static size_t verify_pass_row_stride(const KeyShape& key) { return (key.vprog.proof_len + 31) & ~(size_t)31; }
// host bytes into the (key, ctx) workspace, asynchronously (h2d_small copies whole 16-byte units: sources are padded copies)
static int vd_put(bzh_ctx* ctx, Arena& arena, const void* src, size_t bytes, uint32_t** d) {
    *d = (uint32_t*)arena.alloc(bytes + 16);
    if (!*d) return BZH_E_OOM;
    return h2d_small(ctx, *d, src, (bytes + 15) & ~(size_t)15);
}
// [bzh_verify_batch] lines on stderr under BZH_PROVE_TRACE=1
struct VerifyTrace {
    const bool on = getenv("BZH_PROVE_TRACE") != nullptr;
    std::chrono::steady_clock::time_point t_last = std::chrono::steady_clock::now();
    void mark(const char* name) {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[bzh_verify_batch] %-22s %8.3f ms\n", name, std::chrono::duration<double, std::milli>(now - t_last).count());
        t_last = now;
    }
};
// what a front door leaves in the (key, ctx) workspace: batch rows of verify_pass_row_stride() proof bytes, zero-filled where the
// pre-reject byte is set; the instance commitments (batch x max(ni, 1)) and G_0 U W, affine canonical
struct VerifyPassFront {
    uint8_t* d_rows = nullptr;
    const uint8_t* d_pre = nullptr;
    const uint32_t *d_inst_xy = nullptr, *d_srs_xy = nullptr;
};
// what the body hands to the opening check: the left side's points (canonical) and scalars, (c, u_j), one reject byte per proof
struct VerifyPassSides {
    uint32_t *d_lc_pts = nullptr, *d_lc_scal = nullptr, *d_cu = nullptr;
    const uint8_t* d_reject = nullptr;
    size_t nl_cap = 0;
};

// The device pass from "instances and proofs are in HBM" on: enqueues everything up to k_vp_reject, then `finish` runs the opening
// check and delivers the results its own way (read-back and host comparison, or a kernel).
template <class C, class Finish>
static int verify_pass_enqueue_t(bzh_ctx* ctx, const KeyShape& key, Arena& arena, size_t batch, const VerifyPassFront& front, VerifyTrace& tr,
                                 Finish&& finish) {
    const VerifyTape& vp = key.vprog;
    const size_t B = batch, np = key.vp_offsets.size(), np_all = B * np, kk = key.k, nl_cap = vp.nl_cap;
    const size_t ni1 = std::max<size_t>((size_t)key.ni, 1), pstride = verify_pass_row_stride(key);
    const bool trace = tr.on;
    auto mark = [&](const char* name) { tr.mark(name); };
    // the key's program and points, this call's operands: device memory out of the (key, ctx) workspace
    auto words = [&](size_t w) { return (uint32_t*)arena.alloc(w * 4); };
    auto put = [&](const void* src, size_t bytes, uint32_t** d) -> int { return vd_put(ctx, arena, src, bytes, d); };
    auto padded = [](const void* p, size_t bytes) {
        std::vector<uint8_t> v((bytes + 15) & ~(size_t)15, 0);
        if (bytes) memcpy(v.data(), p, bytes);
        return v;
    };
    VerifyPassArgs a;
    a.batch = B, a.pstride = pstride;
    a.nops = (uint32_t)vp.nops(), a.nslots = vp.nslots, a.nch = vp.nch, a.nev = (uint32_t)vp.ev_offsets.size();
    a.nl_cap = (uint32_t)nl_cap, a.ncu = (uint32_t)(kk + 1), a.np = (uint32_t)np, a.ni = (uint32_t)ni1, a.nfixed = (uint32_t)(key.fixed_commitments.size() / 8);
    uint32_t *d_ops, *d_consts, *d_evo, *d_outs, *d_ptsrc, *d_vpo, *d_key_xy, *d_vk;
    uint8_t* const d_rows = front.d_rows;
    const uint32_t *d_inst_xy = front.d_inst_xy, *d_srs_xy = front.d_srs_xy;
    {
        const auto v = padded(vp.ops.data(), vp.ops.size() * 4);
        BZH_TRY(put(v.data(), v.size(), &d_ops));
    }
    {
        const auto v = padded(vp.consts.data(), vp.consts.size() * 4);
        BZH_TRY(put(v.data(), v.size(), &d_consts));
    }
    {
        const auto v = padded(vp.ev_offsets.data(), vp.ev_offsets.size() * 4);
        BZH_TRY(put(v.data(), v.size(), &d_evo));
    }
    {
        const auto v = padded(vp.out_slots.data(), vp.out_slots.size() * 4);
        BZH_TRY(put(v.data(), v.size(), &d_outs));
    }
    {
        const auto v = padded(vp.pt_src.data(), vp.pt_src.size() * 4);
        BZH_TRY(put(v.data(), v.size(), &d_ptsrc));
    }
    {
        const auto v = padded(key.vp_offsets.data(), key.vp_offsets.size() * 4);
        BZH_TRY(put(v.data(), v.size(), &d_vpo));
    }
    {
        std::vector<uint64_t> kx(key.fixed_commitments);
        kx.insert(kx.end(), key.sigma_commitments.begin(), key.sigma_commitments.end());
        kx.resize(kx.size() + 8, 0);
        BZH_TRY(put(kx.data(), kx.size() * 8, &d_key_xy));
    }
    BZH_TRY(put(key.vk_repr, 32, &d_vk));
    uint32_t* d_in = words(np_all * 8 + 8);
    uint32_t* d_xy = words(np_all * 16 + 16);
    uint8_t* d_st = (uint8_t*)arena.alloc(np_all + 16);
    uint32_t* d_ch = words((size_t)vp.nch * B * 8);
    uint32_t* d_slots = words((size_t)vp.nslots * 8 * B);
    uint32_t* d_lc_scal = words(B * nl_cap * 8);
    uint32_t* d_lc_pts = words(B * nl_cap * 16);
    uint32_t* d_cu = words(B * (kk + 1) * 8);
    uint32_t* d_flags = words(B + 4);
    uint8_t* d_reject = (uint8_t*)arena.alloc((B + 15) & ~(size_t)15);
    if (!d_in || !d_xy || !d_st || !d_ch || !d_slots || !d_lc_scal || !d_lc_pts || !d_cu || !d_flags || !d_reject) return BZH_E_OOM;
    a.d_proofs = d_rows, a.d_ops = d_ops, a.d_consts = d_consts, a.d_ev_offsets = d_evo, a.d_out_slots = d_outs, a.d_pt_src = d_ptsrc;
    a.d_vp_offsets = d_vpo, a.d_ch = d_ch, a.d_slots = d_slots, a.d_lc_scal = d_lc_scal, a.d_cu = d_cu, a.d_flags = d_flags;
    a.d_proof_xy = d_xy, a.d_key_xy = d_key_xy, a.d_inst_xy = d_inst_xy, a.d_srs_xy = d_srs_xy, a.d_point_status = d_st;
    a.d_pre_reject = front.d_pre, a.d_lc_pts = d_lc_pts, a.d_reject = d_reject;
    BZH_TRY(vp_gather_points(ctx, a, d_in));
    BZH_TRY(decompress_run(ctx, C::id, d_in, np_all, BZH_FORM_CANONICAL, d_xy, d_st));
    mark("vd:stage+decompress");
    // the transcripts of the whole batch, in lockstep
    bzh_transcript_batch* tb = nullptr;
    BZH_TRY(tb_new_locked(ctx, C::id, B, &tb));
    struct TbGuard {
        bzh_transcript_batch* t;
        ~TbGuard() { tb_free_locked(t); }
    } tb_guard{tb};
    for (size_t i = 0; i + 2 < vp.schedule.size(); i += 3) {
        const uint32_t kind = vp.schedule[i], first = vp.schedule[i + 1], count = vp.schedule[i + 2];
        switch (kind) {
            case VP_TS_VK: BZH_TRY(tb_absorb_locked(tb, 2, d_vk, 1, 0, BZH_FORM_CANONICAL, nullptr)); break;
            case VP_TS_INST: BZH_TRY(tb_absorb_locked(tb, 0, d_inst_xy, count, ni1, BZH_FORM_CANONICAL, nullptr)); break;
            case VP_TS_POINTS: BZH_TRY(tb_absorb_locked(tb, 0, d_xy + (size_t)first * 16, count, np, BZH_FORM_CANONICAL, d_st + first)); break;
            case VP_TS_SQUEEZE: BZH_TRY(tb_squeeze_locked(tb, BZH_FORM_MONTGOMERY, d_ch + (size_t)first * B * 8)); break;
            default: BZH_TRY(tb_absorb_locked(tb, 2, d_rows + first, count, pstride / 32, BZH_FORM_CANONICAL, nullptr));
        }
    }
    a.d_tb_status = tb_status_device(tb);
    mark("vd:transcripts");
    hipEvent_t ev_a = nullptr, ev_b = nullptr;
    if (trace && hipEventCreate(&ev_a) == hipSuccess && hipEventCreate(&ev_b) == hipSuccess) (void)hipEventRecord(ev_a, ctx->stream);
    BZH_TRY(vp_scalars_run(ctx, C::id, a));
    if (ev_b) (void)hipEventRecord(ev_b, ctx->stream);
    BZH_TRY(vp_assemble_run(ctx, a));
    VerifyPassSides sides;
    sides.d_lc_pts = d_lc_pts, sides.d_lc_scal = d_lc_scal, sides.d_cu = d_cu, sides.d_reject = d_reject, sides.nl_cap = nl_cap;
    BZH_TRY(finish(sides));
    if (ev_b) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, ev_a, ev_b) == hipSuccess)
            fprintf(stderr, "[bzh_verify_batch] %-22s %8.3f ms  (%zu proofs, %zu ops, %zu inversions)\n", "vd:scalars", (double)ms, B, vp.nops(), vp.n_inv);
    }
    if (ev_a) (void)hipEventDestroy(ev_a);
    if (ev_b) (void)hipEventDestroy(ev_b);
    mark("vd:ipa check");
    return BZH_OK;
}

// The accumulation weights of a batch (bzh_accumulation_weights): w_b = draw b of bzh_rng_expand(seed, ..), 64 bytes, reduced as
// Field::random reduces them (from_bytes_wide); out: batch x 4 limbs in `form`
template <class SF>
static void accumulation_weights_t(const uint8_t* seed, size_t batch, int form, uint64_t* out) {
    uint32_t key[8], blk[16];
    memcpy(key, seed, 32);
    for (size_t b = 0; b < batch; b++) {
        chacha20_block(key, b, blk);
        fe_to_u64<SF>(out + 4 * b, h_from_u512<SF>(reinterpret_cast<const uint8_t*>(blk)), form);
    }
}
// The accumulated ending of a device pass (bzh_verify_records_accumulated, bzh_verify_batch_vk_accumulated): ONE opening check for
// the batch, every proof the pass rejected -- its reject byte folds the pre-reject byte in -- excluded with weight 0; the verdict
// byte lands at d_ok.  skip: the host already knows that every record is refused, and no MSM is launched.
static int verify_pass_accumulated(bzh_ctx* ctx, const bzh_bases* srs, size_t batch, const VerifyPassSides& s, const uint32_t* d_weights,
                                   bool skip, uint8_t* d_ok) {
    if (skip) return BZH_OK;
    return ipa_check_accumulated_device(ctx, srs, batch, s.nl_cap, s.d_lc_pts, s.d_lc_scal, s.d_cu, d_weights, s.d_reject, d_ok);
}

// Front door of bzh_verify_batch / bzh_verify_batch_vk(_with) under BZH_VERIFY_PASS_DEVICE: the instance commitments through the
// host (instance_commitments), the proofs staged on the host -- a proof whose length is not the key's is rejected here and its row
// is zero-filled -- and, after the pass, the two sums per proof compared on the host.
// With a seed (bzh_verify_batch_vk_accumulated) the weights go up behind the proofs and the pass ends in the accumulated check; if
// that does not accept, the per-proof ending runs on the same operands and *path = 1.
template <class C>
static int verify_batch_device_t(bzh_ctx* ctx, const KeyShape& key, const bzh_bases* srs, const bzh_bases* g_lagrange, Arena& arena,
                                 size_t batch, const uint64_t* instances, size_t inst_rows, const uint8_t* proofs, size_t proof_stride,
                                 const size_t* proof_lens, const uint64_t* g0_u_w, const uint8_t* seed, int* results, int* path) {
    if (!verify_pass_has_program(ctx, key)) return BZH_E_RANGE;
    arena.reset();
    ColumnCommitter<C> pv(ctx, key, arena);
    const size_t B = batch, plen = key.vprog.proof_len, pstride = verify_pass_row_stride(key), weight_bytes = seed ? B * 32 : 0;
    VerifyTrace tr;
    std::vector<uint64_t> inst_xy;
    BZH_TRY(instance_commitments<C>(pv, key, srs, g_lagrange, B, instances, inst_rows, g0_u_w, inst_xy));
    tr.mark("instance commitments");
    uint32_t *d_srs_xy, *d_inst_xy, *d_pre;
    BZH_TRY(vd_put(ctx, arena, g0_u_w, 3 * 64, &d_srs_xy));
    BZH_TRY(vd_put(ctx, arena, inst_xy.data(), inst_xy.size() * 8, &d_inst_xy));
    std::vector<uint8_t> pre8((B + 15) & ~(size_t)15, 0);
    for (size_t b = 0; b < B; b++) pre8[b] = proof_lens[b] != plen ? 1 : 0;
    BZH_TRY(vd_put(ctx, arena, pre8.data(), pre8.size(), &d_pre));
    uint8_t* d_rows = (uint8_t*)arena.alloc(B * pstride + weight_bytes + 16);
    if (!d_rows) return BZH_E_OOM;
    {   // the proofs, and behind them the accumulation weights (Montgomery) when there is a seed: one upload
        char* slot = nullptr;
        BZH_TRY(h2d_stage(ctx, B * pstride + weight_bytes, &slot));
        for (size_t b = 0; b < B; b++) {
            char* dst = slot + b * pstride;
            if (pre8[b]) {
                memset(dst, 0, pstride);
            } else {
                memcpy(dst, proofs + b * proof_stride, plen);
                if (pstride > plen) memset(dst + plen, 0, pstride - plen);
            }
        }
        if (seed) accumulation_weights_t<typename CurveInfo<C>::SF>(seed, B, BZH_FORM_MONTGOMERY, (uint64_t*)(slot + B * pstride));
        BZH_TRY(h2d_commit(ctx, d_rows, slot, B * pstride + weight_bytes));
    }
    VerifyPassFront front;
    front.d_rows = d_rows, front.d_pre = (const uint8_t*)d_pre, front.d_inst_xy = d_inst_xy, front.d_srs_xy = d_srs_xy;
    // today's ending: the pass's reject bytes, and the two sums of every opening compared on the host
    auto per_proof = [&](const VerifyPassSides& s, bool pts_montgomery) -> int {
        std::vector<uint8_t> rej(pre8.size(), 1);
        BZH_TRY(d2h_async(ctx, rej.data(), s.d_reject, rej.size()));
        std::vector<int> ok(B, 0);
        BZH_TRY(ipa_check_batch_device(ctx, srs, B, s.nl_cap, s.d_lc_pts, s.d_lc_scal, s.d_cu, ok.data(), pts_montgomery));
        for (size_t b = 0; b < B; b++) results[b] = (ok[b] && !rej[b]) ? 1 : 0;
        return BZH_OK;
    };
    if (!seed) return verify_pass_enqueue_t<C>(ctx, key, arena, B, front, tr, [&](const VerifyPassSides& s) -> int { return per_proof(s, false); });
    uint8_t* d_ok = (uint8_t*)arena.alloc(16);
    if (!d_ok) return BZH_E_OOM;
    return verify_pass_enqueue_t<C>(ctx, key, arena, B, front, tr, [&](const VerifyPassSides& s) -> int {
        bool skip = true;   // a wrong length is all the host knows of a proof: when it refuses them all, no MSM is launched
        for (size_t b = 0; b < B; b++) skip = skip && pre8[b] != 0;
        BZH_TRY(verify_pass_accumulated(ctx, srs, B, s, (const uint32_t*)(d_rows + B * pstride), skip, d_ok));
        std::vector<uint8_t> rej(pre8.size(), 1);
        uint8_t okb[16] = {0};
        BZH_TRY(d2h_async(ctx, rej.data(), s.d_reject, rej.size()));
        if (!skip) BZH_TRY(d2h_async(ctx, okb, d_ok, 16));
        BZH_TRY(d2h_finish(ctx));   // the call's one wait when the batch is accepted
        if (path) *path = 0;
        if (skip || okb[0]) {
            for (size_t b = 0; b < B; b++) results[b] = rej[b] ? 0 : 1;
            return BZH_OK;
        }
        // not accepted: which proof fails is the per-proof ending's to say, on the same operands (the left sides' points are in
        // Montgomery form already and are not converted again)
        if (path) *path = 1;
        return per_proof(s, true);
    });
}

// bzh_verify_records_device: verify_board / verify_shot for a batch of binary records (csrc/record.hip), device-resident.  The
// record bytes go up once -- with the caller's G_0 U W behind them, when given --, k_vr_parse checks and unpacks them, the prefix
// MSM, k_vr_add_w and bzh_batch_normalize's launch make the instance commitments (Params::commit_lagrange with blind 1), the pass
// runs, and k_vr_result compares the two sums of every opening on the device; one read-back of a result and a status byte per
// record, and three bytes for the G_0 U W check, ends the call.  The stream is waited for by that read-back alone (msm_run's own
// waits aside, and a workspace that has to grow on a first call).  The caller has checked the arguments.
constexpr size_t kVerifyRecordsMaxBatch = 4096;   // bzh_verify_batch's own limit: what the pass's launches are exercised up to
template <class C>
static int verify_records_t(bzh_ctx* ctx, const KeyShape& key, const bzh_bases* srs, const bzh_bases* g_lagrange, Arena& arena, size_t batch,
                            size_t n_inputs, const uint8_t* records, size_t record_stride, const uint64_t* g0_u_w, const uint8_t* seed,
                            int* results, uint8_t* status, int* path) {
    if (!verify_pass_has_program(ctx, key)) return BZH_E_RANGE;
    arena.reset();
    const size_t B = batch, Bpad = (B + 15) & ~(size_t)15, plen = key.vprog.proof_len, pstride = verify_pass_row_stride(key);
    const size_t rstride = (record_stride + 15) & ~(size_t)15, given_bytes = g0_u_w ? 3 * 64 : 0, out_bytes = 2 * Bpad + 16;
    const size_t weight_bytes = seed ? B * 32 : 0;   // bzh_verify_records_accumulated: the weights (Montgomery) behind the records
    VerifyTrace tr;
    uint8_t* d_records = (uint8_t*)arena.alloc(B * rstride + given_bytes + weight_bytes);
    uint8_t* d_rows = (uint8_t*)arena.alloc(B * pstride + 16);
    uint8_t* d_pre = (uint8_t*)arena.alloc(Bpad);
    uint32_t* d_inst = (uint32_t*)arena.alloc(B * n_inputs * 32);
    uint32_t* d_jac = (uint32_t*)arena.alloc(B * 96);
    uint32_t* d_inst_xy = (uint32_t*)arena.alloc(B * 64 + 64);
    uint32_t* d_srs_xy = (uint32_t*)arena.alloc(3 * 64 + 64);
    uint8_t* d_out = (uint8_t*)arena.alloc(out_bytes);
    if (!d_records || !d_rows || !d_pre || !d_inst || !d_jac || !d_inst_xy || !d_srs_xy || !d_out) return BZH_E_OOM;
    {   // the records, G_0 U W and the weights behind them when given: one slot of all three, one upload
        char* slot = nullptr;
        BZH_TRY(h2d_stage(ctx, B * rstride + given_bytes + weight_bytes, &slot));
        for (size_t b = 0; b < B; b++) {
            memcpy(slot + b * rstride, records + b * record_stride, record_stride);
            if (rstride > record_stride) memset(slot + b * rstride + record_stride, 0, rstride - record_stride);
        }
        if (g0_u_w) memcpy(slot + B * rstride, g0_u_w, 3 * 64);
        if (seed)
            accumulation_weights_t<typename CurveInfo<C>::SF>(seed, B, BZH_FORM_MONTGOMERY, (uint64_t*)(slot + B * rstride + given_bytes));
        BZH_TRY(h2d_commit(ctx, d_records, slot, B * rstride + given_bytes + weight_bytes));
    }
    VerifyRecordsArgs ra;
    ra.batch = B, ra.rstride = rstride, ra.pstride = pstride, ra.n_inputs = (uint32_t)n_inputs, ra.proof_len = (uint32_t)plen;
    ra.d_records = d_records, ra.d_inst = d_inst, ra.d_rows = d_rows, ra.d_pre = d_pre;
    BZH_TRY(verify_records_parse(ctx, C::id, ra));
    BZH_TRY(verify_records_srs(ctx, C::id, srs->d_xy, srs->n, g0_u_w ? (const uint32_t*)(d_records + B * rstride) : nullptr, d_srs_xy,
                               d_out + 2 * Bpad));
    tr.mark("vr:stage+parse");
    // Params::commit_lagrange with blind 1: the inputs against the first n_inputs Lagrange points, plus W (the SRS table's last point)
    BZH_TRY(msm_run(ctx, g_lagrange, d_inst, n_inputs, B, BZH_FORM_MONTGOMERY, d_jac));
    BZH_TRY(verify_records_add_w(ctx, C::id, d_jac, srs->d_xy + (srs->n - 1) * 16, B));
    BZH_TRY(normalize_run(ctx, C::id, d_jac, B, BZH_FORM_CANONICAL, d_inst_xy, nullptr, nullptr));
    tr.mark("instance commitments");
    VerifyPassFront front;
    front.d_rows = d_rows, front.d_pre = d_pre, front.d_inst_xy = d_inst_xy, front.d_srs_xy = d_srs_xy;
    // today's ending: the two sums of every opening, compared on the device, one read-back
    auto per_proof = [&](const VerifyPassSides& s, bool pts_montgomery) -> int {
        const uint32_t* d_sums = nullptr;
        BZH_TRY(ipa_check_sums_device(ctx, srs, B, s.nl_cap, s.d_lc_pts, s.d_lc_scal, s.d_cu, &d_sums, pts_montgomery));
        BZH_TRY(verify_records_result(ctx, C::id, d_sums, B, d_pre, s.d_reject, d_out, Bpad));
        std::vector<uint8_t> out(out_bytes, 0);
        BZH_TRY(d2h_async(ctx, out.data(), d_out, out_bytes));
        BZH_TRY(d2h_finish(ctx));
        if (out[2 * Bpad] | out[2 * Bpad + 1] | out[2 * Bpad + 2]) {
            ctx->last_error = "bzh_verify_records_device: g0_u_w are not G_0, U, W of srs";
            return BZH_E_ARG;
        }
        for (size_t b = 0; b < B; b++) {
            results[b] = out[b];
            if (status) status[b] = out[Bpad + b];
        }
        return BZH_OK;
    };
    if (!seed) return verify_pass_enqueue_t<C>(ctx, key, arena, B, front, tr, [&](const VerifyPassSides& s) -> int { return per_proof(s, false); });
    return verify_pass_enqueue_t<C>(ctx, key, arena, B, front, tr, [&](const VerifyPassSides& s) -> int {
        // what k_vr_parse decides, on the host's copy of the records: when it refuses them all, no MSM is launched
        bool skip = true;
        for (size_t b = 0; b < B && skip; b++)
            skip = vr_record_refused_host<typename CurveInfo<C>::SF>(records + b * record_stride, (uint32_t)plen, (uint32_t)n_inputs);
        uint8_t* d_ok = d_out + 2 * Bpad + 8;   // behind the three G_0 U W bytes
        BZH_TRY(verify_pass_accumulated(ctx, srs, B, s, (const uint32_t*)(d_records + B * rstride + given_bytes), skip, d_ok));
        std::vector<uint8_t> rej(Bpad, 1), pre(Bpad, 1);
        uint8_t tail[16] = {0};
        BZH_TRY(d2h_async(ctx, rej.data(), s.d_reject, Bpad));
        BZH_TRY(d2h_async(ctx, pre.data(), d_pre, Bpad));
        BZH_TRY(d2h_async(ctx, tail, d_out + 2 * Bpad, 16));
        BZH_TRY(d2h_finish(ctx));   // the call's one wait when the batch is accepted
        if (tail[0] | tail[1] | tail[2]) {
            ctx->last_error = "bzh_verify_records_accumulated: g0_u_w are not G_0, U, W of srs";
            return BZH_E_ARG;
        }
        if (path) *path = 0;
        if (skip || tail[8]) {
            for (size_t b = 0; b < B; b++) {
                results[b] = rej[b] ? 0 : 1;
                if (status) status[b] = pre[b] ? 1 : 0;
            }
            return BZH_OK;
        }
        // not accepted: the per-proof ending on the same operands says which record fails (the points are in Montgomery form already)
        if (path) *path = 1;
        return per_proof(s, true);
    });
}
