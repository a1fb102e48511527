// Part of the whole-proof translation unit (csrc/prove.hip): the VANISHING ARGUMENT on device-resident transcripts
// (bzh_vanishing_plan, bzh_vanishing_batch_device) -- phase 5 of Prover::prove as a leaf for a caller whose Fiat-Shamir
// transcripts are a bzh_transcript_batch in HBM.  It is the Prover's own machinery -- q29, ext_alloc, to_extended, the column
// registry, launch_quotient, the extended iNTT -- around three differences:
//   the constant table of the quotient program is built on the device (k_vn_consts, csrc/vanishing.hip) from theta, beta, gamma
//   in the caller's device memory and y squeezed into device memory, out of descriptors that depend on the key alone;
//   the degree check is per proof (k_vn_degree): a status byte and the transcript's sticky byte, nothing read back;
//   the commitments take their blinds from device memory (ipa_commit_blinded) and end in the batch's normalise + absorb launches.
// Included inside namespace bzh { namespace { after prover.hpp.
#pragma once

// the plan's descriptors from a parsed key: one per entry of the VM v2 constant table.  BZH_E_RANGE: no VM v2 program, or a
// symbol this phase does not bind
template <class SF>
static int vanishing_consts_plan(const bzh_pk& pk, std::vector<VnConst>& out) {
    if (!pk.q_ok) return BZH_E_RANGE;
    const size_t m = pk.perm_columns.size();
    Fe<SF> delta;
    memcpy(delta.l, pk.delta, 32);
    std::vector<Fe<SF>> dpow(std::max<size_t>(m, 1), fe_one<SF>());
    for (size_t j = 1; j < m; j++) dpow[j] = fe_mul(dpow[j - 1], delta);
    const Fe<SF> one = fe_one<SF>();
    out.clear();
    for (const ConstEnt& c : pk.qprog.consts) {
        VnConst d{};
        const Fe<SF>* val = &one;
        if (c.sym < 0) {
            d.challenge = -1;
            memcpy(d.value, c.val, 32);
            val = nullptr;
        } else if (c.sym <= SY_Y) {
            d.challenge = c.sym, d.exponent = 1;   // SY_THETA .. SY_Y are 0 .. 3, the descriptor's numbering
        } else if (c.sym >= SY_YPOW0) {
            if ((uint32_t)(c.sym - SY_YPOW0) > kVnMaxExponent) return BZH_E_RANGE;
            d.challenge = SY_Y, d.exponent = (uint32_t)(c.sym - SY_YPOW0);
        } else if (c.sym >= SY_BD0 && (size_t)(c.sym - SY_BD0) < m) {
            d.challenge = SY_BETA, d.exponent = 1;
            val = &dpow[c.sym - SY_BD0];
        } else {
            return BZH_E_RANGE;
        }
        if (val) memcpy(d.value, val->l, 32);
        out.push_back(d);
    }
    return BZH_OK;
}
static_assert(SY_THETA == 0 && SY_BETA == 1 && SY_GAMMA == 2 && SY_Y == 3, "bzh_vanishing_const numbers the challenges like the symbols");

// Two steps every leaf on the key's arena shares (vanishing_device_t below, products_device.hpp).
// the first `nd` 64-byte draws of every proof (proof b at rng + b * rng_stride: host memory, or device memory with `host` false),
// reduced into drawn[b][nd]: one upload or one strided device copy of the batch's bytes, none when they already lie dense
template <class C>
static int leaf_draws(Prover<C>& pv, bool host, const uint8_t* rng, size_t rng_stride, size_t nd, uint32_t* drawn) {
    bzh_ctx* ctx = pv.ctx;
    const size_t B = pv.B;
    const uint8_t* raw = rng;
    if (host) {
        char* stage = nullptr;
        uint8_t* d = (uint8_t*)pv.arena.alloc(B * nd * 64);
        if (!d) return BZH_E_OOM;
        BZH_TRY(h2d_stage(ctx, B * nd * 64, &stage));
        for (size_t b = 0; b < B; b++) memcpy(stage + b * nd * 64, rng + b * rng_stride, nd * 64);
        BZH_TRY(h2d_commit(ctx, d, stage, B * nd * 64));
        raw = d;
    } else if (rng_stride != nd * 64) {
        uint8_t* d = (uint8_t*)pv.arena.alloc(B * nd * 64);
        if (!d) return BZH_E_OOM;
        BZH_HIP_TRY(ctx, hipMemcpy2DAsync(d, nd * 64, rng, rng_stride, nd * 64, B, hipMemcpyDeviceToDevice, pv.st));
        raw = d;
    }
    return random_field(ctx, pv.field, (const uint32_t*)raw, B * nd, drawn);
}
// `count` polynomials of n coefficients under their blinds in device memory, into the transcripts: `per_proof` points each,
// written (kind 1) or absorbed as common points (kind 0).  evals: the same columns over the domain; when the caller has them and
// the key offers g_lagrange (bzh_pk_set_lagrange) they are committed in that basis, where witness columns are sparse
// (DeviceColumns::commit) -- the same group elements, the same bytes
template <class C>
static int leaf_commit_write(Prover<C>& pv, bzh_transcript_batch* tb, const uint32_t* polys, const uint32_t* blinds, size_t count,
                             size_t per_proof, const uint32_t* evals = nullptr, int kind = 1) {
    ArenaScope scope(pv.arena);   // (dead once enqueued: everything that reuses the memory is queued behind it on the one stream)
    const bzh_bases* lagrange = nullptr;
    if (evals) {
        std::lock_guard<std::mutex> lk(pv.pk.rt.mu);
        lagrange = pv.pk.srs_lagrange;
    }
    const size_t cols = lagrange ? lagrange->n : pv.n + 2;
    uint32_t* scalars = pv.dalloc(count * cols);
    uint32_t* xyz = pv.dalloc(count * 3);
    if (!scalars || !xyz) return BZH_E_OOM;
    if (lagrange) {
        BZH_TRY(commitments_scalar_rows(pv.ctx, pv.field, evals, blinds, pv.n, cols, count, scalars));
        BZH_TRY(msm_run(pv.ctx, lagrange, scalars, cols, count, BZH_FORM_MONTGOMERY, xyz));
    } else {
        BZH_TRY(ipa_commit_blinded(pv.ctx, pv.pk.srs, polys, count, blinds, scalars, xyz));
    }
    return tb_write_jacobian_locked(tb, xyz, per_proof, per_proof, BZH_FORM_MONTGOMERY, kind);
}

// the call, for a caller that holds ctx->mu and has made every argument check
template <class C>
static int vanishing_device_t(bzh_ctx* ctx, bzh_pk* pk, size_t B, const uint64_t* advice_polys, const uint64_t* instance_polys,
                              const uint64_t* lookup_polys, const uint64_t* z_polys, const uint64_t* theta, const uint64_t* beta,
                              const uint64_t* gamma, int form, int mem, const uint8_t* rng, size_t rng_stride, bzh_transcript_batch* tb,
                              uint64_t* out_random, uint64_t* out_random_blind, uint64_t* out_h, uint64_t* out_h_blinds, uint8_t* status,
                              bool chained = false) {
    using SF = typename CurveInfo<C>::SF;
    Arena& arena = pk->rt.arena_for(ctx->serial, ctx->device);
    // A BZH_MEM_DEVICE call returns with its work still queued on ctx->stream, and that work reads and writes the arena
    // (bzh_prove_batch never leaves any: it waits for its proofs).  Reusing the one merged block from its start is ordered
    // behind that work by the stream.  While the arena is still a list of blocks -- after a key's first call of a shape --
    // reset() frees them and allocates the merged block, so the queued work is waited for first: one stream wait on that
    // call, none on the calls after it (include/bzh2.h says so).  `chained`: a step of bzh_prove_batch_device (prove_device.hpp),
    // which has reset the arena itself, keeps its own buffers in it and wraps every step in an ArenaScope.
    if (!chained) {
        if (arena.blocks.size() > 1) BZH_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        arena.reset();
    }
    Prover<C> pv(ctx, *pk, B, arena);
    const bool host = mem == BZH_MEM_HOST, canonical = form == BZH_FORM_CANONICAL;
    const int field = pk->field;
    const size_t n = pk->n, en = pk->en, na = (size_t)pk->na, ni = (size_t)pk->ni, nl = (size_t)pk->nl, nz = (size_t)(pk->nsets + pk->nl),
                 npieces = (size_t)pk->npieces, nd = n + 1 + npieces;
    hipStream_t st = ctx->stream;
    std::vector<VnConst> descs;
    BZH_TRY(vanishing_consts_plan<SF>(*pk, descs));
    const size_t nc = descs.size();

    // the operands as Montgomery elements in device memory: in place, or a copy in the workspace
    auto operand = [&](const uint64_t* src, size_t elems, bool convert, const uint32_t** dev) -> int {
        *dev = (const uint32_t*)src;
        if (!elems || (!host && !(convert && canonical))) return BZH_OK;
        uint32_t* d = pv.dalloc(elems);
        if (!d) return BZH_E_OOM;
        if (host) BZH_TRY(h2d_small(ctx, d, src, elems * 32));
        else BZH_HIP_TRY(ctx, hipMemcpyAsync(d, src, elems * 32, hipMemcpyDeviceToDevice, st));
        if (convert && canonical) BZH_TRY(field_convert(ctx, field, d, elems, 1));
        *dev = d;
        return BZH_OK;
    };
    const uint32_t *d_adv, *d_inst, *d_lk, *d_z, *d_theta, *d_beta, *d_gamma;
    BZH_TRY(operand(advice_polys, B * na * n, true, &d_adv));
    BZH_TRY(operand(instance_polys, B * ni * n, true, &d_inst));
    BZH_TRY(operand(lookup_polys, B * nl * 2 * n, true, &d_lk));
    BZH_TRY(operand(z_polys, B * nz * n, true, &d_z));
    BZH_TRY(operand(theta, B, false, &d_theta));   // (k_vn_consts reads the challenges in the caller's form)
    BZH_TRY(operand(beta, B, false, &d_beta));
    BZH_TRY(operand(gamma, B, false, &d_gamma));

    // every column on the extended coset (fe29 planes when the unsaturated kernel will run), as extend_witness / grand_products;
    // BZH_WORKSPACE_COSETWISE: none of them -- n-sized buffers over the coefficient forms, refilled coset by coset at the launch
    uint32_t *adv_cosets = nullptr, *inst_cosets = nullptr, *z_cosets = nullptr, *lk_cosets = nullptr;
    typename Prover<C>::CosetWork cw;
    if (pv.cosetwise) {
        BZH_TRY(pv.cosetwise_setup(d_adv, d_inst, d_z, std::vector<const uint32_t*>(1, d_lk), 2 * nl, cw));
    } else {
        adv_cosets = pv.ext_alloc(B * std::max<size_t>(na, 1));
        inst_cosets = pv.ext_alloc(B * std::max<size_t>(ni, 1));
        z_cosets = pv.ext_alloc(B * std::max<size_t>(nz, 1));
        lk_cosets = pv.ext_alloc(B * std::max<size_t>(2 * nl, 1));
        if (!adv_cosets || !inst_cosets || !z_cosets || !lk_cosets) return BZH_E_OOM;
        BZH_TRY(pv.to_extended(inst_cosets, d_inst, B * ni));
        BZH_TRY(pv.to_extended(adv_cosets, d_adv, B * na));
        BZH_TRY(pv.to_extended(z_cosets, d_z, B * nz));
        BZH_TRY(pv.to_extended(lk_cosets, d_lk, B * nl * 2));
    }

    // the results: the caller's device buffers (Montgomery until the call's last launches), or the workspace
    uint32_t* rp = host ? pv.dalloc(B * n) : (uint32_t*)out_random;
    uint32_t* rb = host ? pv.dalloc(B) : (uint32_t*)out_random_blind;
    uint32_t* h = host ? pv.dalloc(B * en) : (uint32_t*)out_h;
    uint32_t* hb = host ? pv.dalloc(B * npieces) : (uint32_t*)out_h_blinds;
    const size_t st_bytes = (B + 15) & ~(size_t)15;
    uint8_t* d_st = host ? (uint8_t*)arena.alloc(st_bytes) : status;
    uint32_t* d_y = pv.dalloc(B);
    uint32_t* drawn = pv.dalloc(B * nd);
    if (!rp || !rb || !h || !hb || (host && !d_st) || !d_y || !drawn) return BZH_E_OOM;

    // the draws: one upload of the batch's bytes, reduced, then scattered into the random polynomial, its blind, the piece blinds
    BZH_TRY(leaf_draws(pv, host, rng, rng_stride, nd, drawn));
    BZH_TRY(pv.copy2d(rp, n, drawn, nd, n, B));
    BZH_TRY(pv.copy2d(rb, 1, drawn + n * 8, nd, 1, B));
    BZH_TRY(pv.copy2d(hb, npieces, drawn + (n + 1) * 8, nd, npieces, B));
    auto commit_write = [&](const uint32_t* polys, const uint32_t* blinds, size_t count, size_t per_proof) -> int {
        return leaf_commit_write(pv, tb, polys, blinds, count, per_proof);
    };
    BZH_TRY(commit_write(rp, rb, B, 1));
    BZH_TRY(tb_squeeze_locked(tb, BZH_FORM_MONTGOMERY, d_y));

    // the quotient on the extended coset: the registry and the launch are the Prover's, the constants come from k_vn_consts
    Cols reg;
    QuotientPtrs qp;
    qp.adv = adv_cosets, qp.inst = inst_cosets, qp.z = z_cosets, qp.lk_cols = 2 * nl;
    for (size_t i = 0; i < nl && !pv.cosetwise; i++) qp.lk.push_back(lk_cosets + i * 2 * en * (pv.q29 ? 9 : 8));
    if (!pv.cosetwise) quotient_registry(*pk, qp, pv.q29, reg);
    typename Prover<C>::ProgramArgs pa;
    BZH_TRY(pv.quotient_args(pv.cosetwise ? cw.reg : reg, nullptr, std::max<size_t>(B * nc, 1) * pv.quotient_const_words() * 4, pa));
    void* d_descs = arena.alloc(std::max<size_t>(nc, 1) * sizeof(VnConst));
    if (!d_descs) return BZH_E_OOM;
    BZH_TRY(h2d_small(ctx, d_descs, descs.data(), nc * sizeof(VnConst)));
    BZH_TRY(vanishing_consts(ctx, field, d_descs, nc, B, d_theta, d_beta, d_gamma, d_y, form, pv.q29, pa.consts));
    if (pv.cosetwise) BZH_TRY(pv.cosetwise_launch(cw, pa, h));
    else BZH_TRY(pv.launch_quotient(reg, en, pa, h));
    BZH_TRY(ntt_run(ctx, field, h, pk->ek, B, pk->eomega, pk->zeta, 1, BZH_FORM_MONTGOMERY));

    // the degree check, per proof
    if (d_st) BZH_HIP_TRY(ctx, hipMemsetAsync(d_st, 0, host ? st_bytes : B, st));
    BZH_TRY(vanishing_degree(ctx, h, npieces * n, en, B, d_st, tb_status_device_mut(tb)));

    // the pieces where they lie when they fill the rows of h, else side by side through one copy
    if (npieces * n == en) {
        BZH_TRY(commit_write(h, hb, B * npieces, npieces));
    } else {
        ArenaScope scope(arena);
        uint32_t* pieces = pv.dalloc(B * npieces * n);
        if (!pieces) return BZH_E_OOM;
        BZH_TRY(pv.copy2d(pieces, npieces * n, h, en, npieces * n, B));
        BZH_TRY(commit_write(pieces, hb, B * npieces, npieces));
    }

    // the outputs in the caller's form, and to the host
    if (canonical) {
        BZH_TRY(field_convert(ctx, field, rp, B * n, 0));
        BZH_TRY(field_convert(ctx, field, rb, B, 0));
        BZH_TRY(field_convert(ctx, field, h, B * en, 0));
        BZH_TRY(field_convert(ctx, field, hb, B * npieces, 0));
    }
    if (!host) return BZH_OK;
    std::vector<uint8_t> st_host(st_bytes);
    BZH_TRY(d2h_async(ctx, out_random, rp, B * n * 32));
    BZH_TRY(d2h_async(ctx, out_random_blind, rb, B * 32));
    BZH_TRY(d2h_async(ctx, out_h, h, B * en * 32));
    BZH_TRY(d2h_async(ctx, out_h_blinds, hb, B * npieces * 32));
    BZH_TRY(d2h_async(ctx, st_host.data(), d_st, st_bytes));
    BZH_TRY(d2h_finish(ctx));
    if (status) memcpy(status, st_host.data(), B);
    return BZH_OK;
}
