// Part of the whole-proof translation unit (csrc/prove.hip): the DEVICE-RESIDENT BATCH PROVER (bzh_prove_device_plan,
// bzh_prove_batch_device, bzh_prove_batch_device_seeded) -- create_proof as the chain of the five leaves on ONE device transcript
// batch: commitments_device_t, products_device_t, vanishing_device_t, the evaluations and the multiopen with its opening.  A
// witness goes in and whole proofs come out, byte-identical to bzh_prove_batch's; no challenge, scalar or point comes to the host
// before the one read-back of the proofs and the status at the end.  What the call adds around the leaf bodies:
//   the query lists of the evaluations and the multiopen, built from the key's own KeyShape in upstream's order when the key first
//   needs them and kept with the key (PdPlan, proving_key.hpp);
//   the leaves' outputs stay where the leaves wrote them, in the key's workspace for this ctx: the evaluations and the multiopen
//   read every polynomial through a source table of (pointer, per-proof stride) -- the key's fixed_polys and sigma_polys in place
//   with stride 0 -- so no [batch][nown][n] table is ever made;
//   k_pd_blinds (csrc/prove_device.hip) gathers the [batch][nown] blind row of the multiopen, k_pd_status folds the four leaves'
//   status bytes into one byte per proof next to the proof's length;
//   the grand products are committed in the Lagrange basis when the key has g_lagrange (products_device_t keeps its evaluations).
// Every leaf body runs inside an ArenaScope: its own scratch is handed back when it has enqueued its work, the chain's buffers,
// allocated before the first leaf, stay.
// Included inside namespace bzh { namespace { after commitments_device.hpp.
#pragma once

// draws per proof of the four drawing leaves, in chain order
static void prove_device_draws(const KeyShape& ks, size_t nd[4]) {
    nd[0] = commitments_draws(ks);
    nd[1] = (size_t)(ks.nsets + ks.nl) * ((size_t)ks.bf + 1);
    nd[2] = ks.n + 1 + (size_t)ks.npieces;
    nd[3] = ks.n + 2 + 2 * (size_t)ks.k;
}
// the polynomials of a proof that get opened: instance, advice, the random polynomial, grand products, lookups (a, s), h(X)
static size_t prove_device_nown(const KeyShape& ks) {
    return (size_t)ks.ni + (size_t)ks.na + 1 + (size_t)(ks.nsets + ks.nl) + 2 * (size_t)ks.nl + 1;
}
// the bytes of a proof: KeyShape::max_proof_bytes counts three evaluations for every permutation set, the last set has two
static size_t prove_device_proof_bytes(const KeyShape& ks) { return ks.max_proof_bytes() - (ks.nsets ? 32 : 0); }
// the commitments of a kind are one launch with one row of its grid per commitment
static size_t prove_device_max_batch(const KeyShape& ks) {
    const size_t widest = std::max({(size_t)ks.na, (size_t)ks.ni, 2 * (size_t)ks.nl, (size_t)(ks.nsets + ks.nl), (size_t)ks.npieces, (size_t)1});
    return 65535 / widest;
}

// the query lists in upstream's order, and what bzh_evaluations_plan / bzh_multiopen_plan make of them.  Polynomial ids: the
// opened polynomials of a proof (above), then the key's fixed and permutation polynomials.  BZH_E_RANGE: a polynomial at more
// rotations, or a set of more points, than those two leaves take
static int prove_device_plan_build(const KeyShape& ks, PdPlan& P) {
    const size_t ni = (size_t)ks.ni, na = (size_t)ks.na, nf = (size_t)ks.nf, nl = (size_t)ks.nl, nsets = (size_t)ks.nsets, nz = nsets + nl,
                 m = ks.perm_columns.size();
    const uint32_t z0 = (uint32_t)(ni + na + 1), l0 = (uint32_t)(z0 + nz), nown = (uint32_t)prove_device_nown(ks), hid = nown - 1;
    const int32_t last_rot = -(ks.bf + 1);
    const size_t npolys = nown + nf + m;
    std::vector<bzh_eval_query> ev;
    for (auto& q : ks.instance_queries) ev.push_back({(uint32_t)q.first, q.second});
    for (auto& q : ks.advice_queries) ev.push_back({(uint32_t)(ni + (size_t)q.first), q.second});
    for (auto& q : ks.fixed_queries) ev.push_back({nown + (uint32_t)q.first, q.second});
    ev.push_back({(uint32_t)(ni + na), 0});
    for (size_t j = 0; j < m; j++) ev.push_back({(uint32_t)(nown + nf + j), 0});
    for (uint32_t i = 0; i < nsets; i++) {
        ev.push_back({z0 + i, 0}), ev.push_back({z0 + i, 1});
        if (i + 1 != nsets) ev.push_back({z0 + i, last_rot});
    }
    for (uint32_t l = 0; l < nl; l++) {
        const uint32_t lz = z0 + (uint32_t)nsets + l, la = l0 + 2 * l, ls = la + 1;
        ev.push_back({lz, 0}), ev.push_back({lz, 1}), ev.push_back({la, 0}), ev.push_back({la, -1}), ev.push_back({ls, 0});
    }
    EvPlan& e = P.ev;
    e.npolys_own = nown, e.npolys_shared = nf + m, e.nqueries = ev.size();
    e.rotations.resize(ev.size()), e.point_of_query.resize(ev.size()), e.poly_order.resize(npolys), e.rot_count.resize(npolys);
    if (bzh_evaluations_plan(ev.data(), ev.size(), npolys, e.rotations.data(), &e.nrot, e.point_of_query.data(), e.poly_order.data(),
                             e.rot_count.data()))
        return BZH_E_RANGE;
    e.rotations.resize(e.nrot);
    e.poly_of_query.resize(ev.size());
    for (size_t q = 0; q < ev.size(); q++) e.poly_of_query[q] = ev[q].poly;
    auto pt = [&](int32_t rot) { return (uint32_t)(std::find(e.rotations.begin(), e.rotations.end(), rot) - e.rotations.begin()); };

    std::vector<bzh_open_query> mo;
    for (auto& q : ks.instance_queries) mo.push_back({(uint32_t)q.first, pt(q.second)});
    for (auto& q : ks.advice_queries) mo.push_back({(uint32_t)(ni + (size_t)q.first), pt(q.second)});
    for (uint32_t i = 0; i < nsets; i++) {
        mo.push_back({z0 + i, pt(0)}), mo.push_back({z0 + i, pt(1)});
        if (i + 1 != nsets) mo.push_back({z0 + i, pt(last_rot)});
    }
    for (uint32_t l = 0; l < nl; l++) {
        const uint32_t lz = z0 + (uint32_t)nsets + l, la = l0 + 2 * l, ls = la + 1;
        mo.push_back({lz, pt(0)}), mo.push_back({la, pt(0)}), mo.push_back({ls, pt(0)}), mo.push_back({la, pt(-1)}), mo.push_back({lz, pt(1)});
    }
    for (auto& q : ks.fixed_queries) mo.push_back({nown + (uint32_t)q.first, pt(q.second)});
    for (size_t j = 0; j < m; j++) mo.push_back({(uint32_t)(nown + nf + j), pt(0)});
    mo.push_back({hid, pt(0)}), mo.push_back({(uint32_t)(ni + na), pt(0)});
    MoPlan& o = P.mo;
    o.npolys_own = nown, o.npolys_shared = nf + m, o.npoints = e.nrot;
    o.set_of_poly.resize(npolys), o.group_order.resize(npolys), o.set_sizes.resize(npolys), o.set_points.resize(npolys * BZH_MULTIOPEN_MAX_POINTS);
    if (bzh_multiopen_plan(mo.data(), mo.size(), npolys, e.nrot, o.set_of_poly.data(), o.group_order.data(), o.set_sizes.data(),
                           o.set_points.data(), &o.nsets))
        return BZH_E_RANGE;
    for (size_t s = 0; s < o.nsets; s++)
        if (o.set_sizes[s] >= ks.n) return BZH_E_RANGE;   // nothing is left of n coefficients after n divisions
    return BZH_OK;
}
// the key's plan, built on first use (the caller holds no lock)
static int prove_device_plan_of(bzh_pk* pk, const PdPlan** out) {
    std::lock_guard<std::mutex> lk(pk->rt.mu);
    if (!pk->pd_plan.ready) {
        pk->pd_plan.rc = prove_device_plan_build(*pk, pk->pd_plan);
        pk->pd_plan.ready = true;
    }
    *out = &pk->pd_plan;
    return pk->pd_plan.rc;
}

// The operands of the game-input calls (csrc/prove_game.hpp), which take them where they lie: the advice tensor is allocated from
// the arena like a host call's and FILLED by the synthesis kernels (the zero fill and the three k_syn_* launches go on the stream
// before the commitments leaf) instead of an upload; the instance buffer is the Montgomery [b][ni][inst_rows] that k_pg_instances
// writes on the device, ni = 1; the synthesis status words are a fifth status source, folded into bits 4 .. 6 by k_pg_status
// after k_pd_status.  The status words and the commitments lie in the arena, not in WS_STAGE (ctx.hpp, the slots' holders).
struct PdGame {
    const char* name;                 // the entry point, for bzh_last_error
    const SynLayout* layout;          // with `inputs`: what synth_pack_inputs made
    const uint64_t* inputs;           // host, batch x layout->in_words
    uint64_t* instances_out;          // host, batch x inst_rows canonical rows, or null
};

// the call, for a caller that holds ctx->mu and has made every argument check.  rng_stride == 0: `rng` holds batch x 32-byte
// seeds in host memory.  status: null, or one byte per proof (host).  game != null: `advice` and `instances` are not read, mem is
// BZH_MEM_DEVICE, inst_rows the circuit's public inputs per proof
template <class C>
static int prove_device_t(bzh_ctx* ctx, bzh_pk* pk, size_t B, const uint64_t* advice, int form, int mem, const uint64_t* instances,
                          size_t inst_rows, const uint8_t* rng, size_t rng_stride, const PdPlan& P, uint8_t* proofs, size_t proof_stride,
                          size_t* proof_lens, uint8_t* status, const PdGame* game = nullptr) {
    using SF = typename CurveInfo<C>::SF;
    Arena& arena = pk->rt.arena_for(ctx->serial, ctx->device);
    // (the merged-block rule and its one wait: vanishing_device_t)
    if (arena.blocks.size() > 1) BZH_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    arena.reset();
    hipStream_t st = ctx->stream;
    const int field = pk->field;
    const size_t n = pk->n, en = pk->en, na = (size_t)pk->na, ni = (size_t)pk->ni, nf = (size_t)pk->nf, nl = (size_t)pk->nl,
                 nsets = (size_t)pk->nsets, nz = nsets + nl, npieces = (size_t)pk->npieces, m = pk->perm_columns.size(),
                 nown = prove_device_nown(*pk), nrot = P.ev.nrot, cap = pk->max_proof_bytes();
    size_t nd[4];
    prove_device_draws(*pk, nd);
    const size_t total = nd[0] + nd[1] + nd[2] + nd[3];
    if (!ni) inst_rows = 0;
    if (!inst_rows) instances = nullptr;
    const bzh_bases* lagrange = nullptr;
    {
        std::lock_guard<std::mutex> lk(pk->rt.mu);
        lagrange = pk->srs_lagrange;
    }

    // BZH_PROVE_TRACE=1: wall time per leaf on stderr, with a stream wait after each
    const bool trace = getenv("BZH_PROVE_TRACE") != nullptr;
    auto t_last = std::chrono::steady_clock::now();
    auto mark = [&](const char* name) {
        if (!trace) return;
        (void)hipStreamSynchronize(st);
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[bzh_prove_batch_device] %-16s %8.2f ms\n", name, std::chrono::duration<double, std::milli>(now - t_last).count());
        t_last = now;
    };

    // the transcripts, with room for a whole proof and for the widest write
    struct Batch {
        bzh_ctx* ctx;
        bzh_transcript_batch* tb = nullptr;
        ~Batch() {
            if (tb) tb_free_locked(tb);   // (waits for the stream: whatever a failed call left queued ends before the memory goes)
            ctx->pending_d2h.clear();
        }
    } batch{ctx};
    BZH_TRY(tb_new_locked(ctx, pk->curve, B, &batch.tb, cap));
    bzh_transcript_batch* tb = batch.tb;
    BZH_TRY(tb_reserve_points_locked(tb, B * std::max({na, ni, 2 * nl, nz, npieces, (size_t)1})));

    // the chain's buffers, in elements of 32 bytes: they outlive the leaves' scopes
    bool oom = false;
    auto elems = [&](size_t count) {
        uint32_t* p = (uint32_t*)arena.alloc(std::max<size_t>(count, 1) * 32);
        oom |= !p;
        return p;
    };
    const bool host = mem == BZH_MEM_HOST;
    uint32_t* d_adv = (host || game) ? elems(B * na * n) : (uint32_t*)advice;
    uint32_t* d_inst = (instances || game) ? elems(B * ni * inst_rows) : nullptr;
    uint32_t* g_canon = game ? elems(B * inst_rows) : nullptr;                     // the canonical rows, read back with the proofs
    uint32_t* g_cm = game ? elems(2 * B) : nullptr;                                // k_syn_ecc_tail's commitments
    uint32_t* g_status = game ? (uint32_t*)arena.alloc(B * 4) : nullptr;           // ... and its status words
    uint32_t *o_adv = elems(B * na * n), *o_inst = elems(B * ni * n), *o_lc = elems(B * nl * 2 * n), *o_lp = elems(B * nl * 2 * n),
             *o_advp = elems(B * na * n), *o_instp = elems(B * ni * n), *o_lkp = elems(B * nl * 2 * n), *o_ab = elems(B * na),
             *o_lb = elems(B * nl * 2), *d_theta = elems(B), *d_beta = elems(B), *d_gamma = elems(B);
    uint32_t *zp = elems(B * nz * n), *zs = lagrange ? elems(B * nz * n) : nullptr, *zb = elems(B * nz);
    uint32_t *rp = elems(B * n), *rb = elems(B), *h = elems(B * en), *hb = elems(B * npieces);
    uint32_t *pts = elems(B * nrot), *hx = elems(B * n), *hx_blind = elems(B), *blinds = elems(B * nown), *shared_blinds = elems(nf + m);
    uint32_t* d_vk = elems(1);
    const size_t st_pitch = (B + 15) & ~(size_t)15;
    uint8_t* d_leaf = (uint8_t*)arena.alloc(4 * st_pitch);
    uint32_t* d_slot = (uint32_t*)arena.alloc(B * 8);
    PdBlindSrc* d_bsrc = (PdBlindSrc*)arena.alloc(6 * sizeof(PdBlindSrc));
    // the draws of every proof side by side in device memory, one stream of `total` draws each: in place when the caller's lie
    // there, expanded from the seeds, or staged up once
    bool rng_on_device = false;
    if (rng_stride && !host) {
        hipPointerAttribute_t at{};
        if (hipPointerGetAttributes(&at, rng) == hipSuccess) rng_on_device = at.type == hipMemoryTypeDevice;
        else (void)hipGetLastError();   // plain host memory the runtime has never seen
        if (rng_on_device && (((uintptr_t)rng | rng_stride) & 15)) return BZH_E_ARG;
    }
    uint8_t* d_rng = rng_on_device ? (uint8_t*)rng : (uint8_t*)arena.alloc(B * total * 64);
    const size_t d_stride = rng_on_device ? rng_stride : total * 64;
    uint32_t* d_keys = rng_stride ? nullptr : (uint32_t*)arena.alloc(B * 32);
    if (oom || !d_leaf || !d_slot || !d_bsrc || !d_rng || (!rng_stride && !d_keys) || (game && !g_status)) return BZH_E_OOM;

    // what depends on the key and the workspace pointers alone, before the first launch: the digest, the blinds of the key's own
    // polynomials, the blind table's sources.  (Each leaf body uploads its own programs, registries and descriptors as its first
    // work on the stream.)
    {
        const std::vector<Fe<SF>> one(std::max<size_t>(nf + m, 1), fe_one<SF>());
        BZH_TRY(h2d_small(ctx, shared_blinds, one.data(), (nf + m) * 32));
        BZH_TRY(h2d_small(ctx, d_vk, pk->vk_repr, 32));
        const uint32_t a0 = (uint32_t)ni, r0 = (uint32_t)(ni + na), z0 = r0 + 1, l0 = (uint32_t)(z0 + nz), h0 = (uint32_t)(nown - 1);
        const PdBlindSrc bs[6] = {{nullptr, 0, 0, (uint32_t)ni},           {o_ab, (uint64_t)na, a0, (uint32_t)na},
                                  {rb, 1, r0, 1},                          {zb, (uint64_t)nz, z0, (uint32_t)nz},
                                  {o_lb, (uint64_t)(2 * nl), l0, (uint32_t)(2 * nl)}, {hx_blind, 1, h0, 1}};
        BZH_TRY(h2d_small(ctx, d_bsrc, bs, sizeof(bs)));
    }
    BZH_HIP_TRY(ctx, hipMemsetAsync(d_leaf, 0, 4 * st_pitch, st));
    // the operands: Montgomery elements in device memory (the instance is canonical host memory, as in bzh_prove_batch)
    if (host) {
        BZH_TRY(h2d_small(ctx, d_adv, advice, B * na * n * 32));
        if (form == BZH_FORM_CANONICAL) BZH_TRY(field_convert(ctx, field, d_adv, B * na * n, 1));
    }
    if (instances) {
        BZH_TRY(h2d_small(ctx, d_inst, instances, B * ni * inst_rows * 32));
        BZH_TRY(field_convert(ctx, field, d_inst, B * ni * inst_rows, 1));
    }
    if (!rng_stride) {
        BZH_TRY(h2d_small(ctx, d_keys, rng, B * 32));
        hipLaunchKernelGGL(k_chacha20_rows, dim3((unsigned)((total + 255) / 256), (unsigned)B), dim3(256), 0, st, d_keys, (uint64_t)0, total,
                           (uint32_t*)d_rng);
        BZH_HIP_TRY(ctx, hipGetLastError());
    } else if (!rng_on_device) {
        char* stage = nullptr;
        BZH_TRY(h2d_stage(ctx, B * total * 64, &stage));
        for (size_t b = 0; b < B; b++) memcpy(stage + b * total * 64, rng + b * rng_stride, total * 64);
        BZH_TRY(h2d_commit(ctx, d_rng, stage, B * total * 64));
    }
    auto draws_at = [&](size_t first) { return (const uint8_t*)d_rng + 64 * first; };
    auto u64 = [](uint32_t* p) { return (uint64_t*)p; };
    const int MO = BZH_FORM_MONTGOMERY, DEV = BZH_MEM_DEVICE;
    mark("setup");
    if (game) {
        SynRun run;
        run.layout = game->layout, run.batch = B, run.inputs = game->inputs, run.table = synth_table_host(), run.d_advice = d_adv;
        const uint64_t* d_in = nullptr;
        BZH_TRY(synth_device_enqueue(ctx, run, g_status, g_cm, &d_in));
        // (reads the packed inputs in WS_STAGE: before the first leaf, which may take that slot)
        BZH_TRY(prove_game_instances(ctx, game->layout->kind == BZH_CIRCUIT_SHOT, g_cm, d_in, game->layout->in_words, B, d_inst, g_canon));
        mark("synthesis");
    }

    BZH_TRY(tb_absorb_locked(tb, 2, d_vk, 1, 0, BZH_FORM_CANONICAL, nullptr));
    {
        ArenaScope scope(arena);
        const bzh_commitments_out out{u64(o_adv),  u64(o_inst), u64(o_lc),   u64(o_lp),    u64(o_advp), u64(o_instp),
                                      u64(o_lkp),  u64(o_ab),   u64(o_lb),   u64(d_theta), u64(d_beta), u64(d_gamma)};
        BZH_TRY(commitments_device_t<C>(ctx, pk, B, u64(d_adv), u64(d_inst), inst_rows, MO, DEV, draws_at(0), d_stride, tb, out, d_leaf, true));
    }
    mark("commitments");
    if (nz) {
        ArenaScope scope(arena);
        BZH_TRY(products_device_t<C>(ctx, pk, B, u64(o_adv), u64(o_inst), u64(o_lc), u64(o_lp), u64(d_beta), u64(d_gamma), MO, DEV, draws_at(nd[0]),
                                     d_stride, tb, u64(zs), u64(zp), u64(zb), d_leaf + st_pitch, true, zs != nullptr));
    }
    mark("grand_products");
    {
        ArenaScope scope(arena);
        BZH_TRY(vanishing_device_t<C>(ctx, pk, B, u64(o_advp), u64(o_instp), u64(o_lkp), u64(zp), u64(d_theta), u64(d_beta), u64(d_gamma), MO, DEV,
                                      draws_at(nd[0] + nd[1]), d_stride, tb, u64(rp), u64(rb), u64(h), u64(hb), d_leaf + 2 * st_pitch, true));
    }
    mark("vanishing");
    // every polynomial where its leaf left it; the key's own in place, shared by every proof
    std::vector<MoSrc> srcs;
    for (size_t c = 0; c < ni; c++) srcs.push_back(MoSrc{o_instp + c * n * 8, (uint64_t)(ni * n)});
    for (size_t c = 0; c < na; c++) srcs.push_back(MoSrc{o_advp + c * n * 8, (uint64_t)(na * n)});
    srcs.push_back(MoSrc{rp, (uint64_t)n});
    for (size_t c = 0; c < nz; c++) srcs.push_back(MoSrc{zp + c * n * 8, (uint64_t)(nz * n)});
    for (size_t c = 0; c < 2 * nl; c++) srcs.push_back(MoSrc{o_lkp + c * n * 8, (uint64_t)(2 * nl * n)});
    srcs.push_back(MoSrc{hx, (uint64_t)n});
    for (size_t c = 0; c < nf; c++) srcs.push_back(MoSrc{pk->fixed_polys + c * n * 8, 0});
    for (size_t c = 0; c < m; c++) srcs.push_back(MoSrc{pk->sigma_polys + c * n * 8, 0});
    if (srcs.size() != nown + nf + m) return BZH_E_ARG;
    {
        ArenaScope scope(arena);
        void* scratch = arena.alloc(evaluations_scratch_bytes(P.ev, B, npieces));
        if (!scratch) return BZH_E_OOM;
        BZH_TRY(evaluations_device_srcs(ctx, pk->curve, B, pk->k, P.ev, srcs.data(), h, npieces, en, hb, MO, tb, pts, nullptr, hx, hx_blind,
                                        scratch));
    }
    mark("evaluations");
    BZH_TRY(prove_device_blinds(ctx, field, d_bsrc, 6, nown, B, blinds));
    {
        ArenaScope scope(arena);
        void* scratch = arena.alloc(multiopen_scratch_bytes(P.mo, B, n));
        if (!scratch) return BZH_E_OOM;
        BZH_TRY(multiopen_device_srcs(ctx, pk->srs, B, pk->k, P.mo, srcs.data(), blinds, shared_blinds, pts, MO, draws_at(nd[0] + nd[1] + nd[2]),
                                      d_stride, tb, d_leaf + 3 * st_pitch, scratch));
    }
    mark("multiopen");

    // the one read-back: the proofs, and per proof the folded status and the length
    const TbInfo ti = tb_info(tb);
    if (ti.proof_len > proof_stride) return BZH_E_RANGE;
    BZH_TRY(prove_device_status(ctx, d_leaf, st_pitch, B, (uint32_t)ti.proof_len, d_slot));
    if (game) BZH_TRY(prove_game_status(ctx, g_status, B, d_slot));
    size_t pstride = 0;
    const uint8_t* d_proofs = tb_proofs_device(tb, &pstride);
    std::vector<uint8_t> rows(B * pstride);
    std::vector<uint32_t> slot(2 * B);
    BZH_TRY(d2h_async(ctx, rows.data(), d_proofs, rows.size()));
    BZH_TRY(d2h_async(ctx, slot.data(), d_slot, B * 8));
    std::vector<uint64_t> canon(game && game->instances_out ? B * inst_rows * 4 : 0);
    BZH_TRY(d2h_async(ctx, canon.data(), g_canon, canon.size() * 8));
    BZH_TRY(d2h_finish(ctx));
    mark("proofs");
    if (!status)
        for (size_t b = 0; b < B; b++)
            if (slot[2 * b]) {
                char text[320];
                if (!game)
                    snprintf(text, sizeof(text), "bzh_prove_batch_device: proof %zu is flagged (status 0x%x: bit 0 lookup, 1 grand product, 2 degree, 3 opening)",
                             b, (unsigned)slot[2 * b]);
                else if (slot[2 * b] >> PG_STATUS_SHIFT)   // the text bzh_synthesize_* gives for the word
                    snprintf(text, sizeof(text), "%s: proof %zu is flagged (status 0x%x: bits 4 to 6 synthesis): %s", game->name, b,
                             (unsigned)slot[2 * b], syn_status_text(slot[2 * b] >> PG_STATUS_SHIFT));
                else
                    snprintf(text, sizeof(text), "%s: proof %zu is flagged (status 0x%x: bit 0 lookup, 1 grand product, 2 degree, 3 opening)", game->name,
                             b, (unsigned)slot[2 * b]);
                ctx->last_error = text;
                return BZH_E_RANGE;
            }
    if (!canon.empty()) memcpy(game->instances_out, canon.data(), canon.size() * 8);
    for (size_t b = 0; b < B; b++) {
        memcpy(proofs + b * proof_stride, &rows[b * pstride], slot[2 * b + 1]);
        proof_lens[b] = slot[2 * b + 1];
        if (status) status[b] = (uint8_t)slot[2 * b];
    }
    return BZH_OK;
}
