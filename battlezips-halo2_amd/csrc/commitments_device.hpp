// Part of the whole-proof translation unit (csrc/prove.hip): the WITNESS COMMITMENTS on device-resident transcripts
// (bzh_commitments_plan, bzh_commitments_batch_device) -- phases 1 to 3 of Prover::prove as a leaf for a caller whose Fiat-Shamir
// transcripts are a bzh_transcript_batch in HBM: the head of the chain whose other leaves read theta, beta and gamma from HBM.
// Prover::commit_instances(), commit_advice() and lookups() convert the instance on the host, assemble the columns with a device
// copy, a fill and strided copies, draw every blind on the host, bring theta down and send it back up inside the compress
// programs' constant tables, and read every commitment back for a host transcript.  Here:
//   k_cm_place (csrc/commitments.hip) writes the advice and instance columns, blinding rows and form conversion included, and
//   the advice blinds, in one launch;
//   the lookups' compress programs are the key's cached VM v1 programs (Prover::run_args / run_launch), their constant tables
//   written by k_cm_consts from theta where it was squeezed; their descriptors, instructions and column registries depend on the
//   key and the operand pointers alone and go up before the first launch;
//   ONE lookup_permute call permutes the batch * nl pairs, from the compressed columns in out.lookup_compressed's layout
//   [b][l][2][n] (pair b * nl + l: input at 2 n pair, table n after it) straight into out.lookup_permuted's; the interpreter
//   writes dense [b][n] rows, so each compressed column takes one strided device copy into that layout;
//   k_cm_lookup_finish places the drawn rows and blinds of every pair and folds lookup_permute's status words into the per-proof
//   byte and the transcript's sticky byte;
//   the commitments take their blinds from device memory, in the basis the key offers (leaf_commit_write, vanishing_device.hpp);
//   the instance commitments go through the same normalise launch and are absorbed as common points.
// Included inside namespace bzh { namespace { after products_device.hpp.
#pragma once

// draws per proof, in upstream's order: the advice blinding rows, the advice blinds, per lookup 2 (bf + 1) rows and two blinds
static size_t commitments_draws(const KeyShape& ks) {
    const size_t bf1 = (size_t)ks.bf + 1;
    return (size_t)ks.na * bf1 + (size_t)ks.na + (size_t)ks.nl * (2 * bf1 + 2);
}

// the call, for a caller that holds ctx->mu and has made every argument check
template <class C>
static int commitments_device_t(bzh_ctx* ctx, bzh_pk* pk, size_t B, const uint64_t* advice, const uint64_t* instances, size_t inst_rows,
                                int form, int mem, const uint8_t* rng, size_t rng_stride, bzh_transcript_batch* tb,
                                const bzh_commitments_out& out, uint8_t* status, bool chained = false) {
    using SF = typename CurveInfo<C>::SF;
    Arena& arena = pk->rt.arena_for(ctx->serial, ctx->device);
    // (the merged-block rule and its one wait, and `chained`: vanishing_device_t)
    if (!chained) {
        if (arena.blocks.size() > 1) BZH_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        arena.reset();
    }
    Prover<C> pv(ctx, *pk, B, arena);
    const bool host = mem == BZH_MEM_HOST, canonical = form == BZH_FORM_CANONICAL;
    const int field = pk->field;
    const size_t n = pk->n, usable = pk->usable, na = (size_t)pk->na, ni = (size_t)pk->ni, nl = (size_t)pk->nl, bf1 = (size_t)pk->bf + 1,
                 nd = commitments_draws(*pk);
    if (!inst_rows) instances = nullptr;

    // the operands in device memory, in the caller's form (k_cm_place converts): in place, or a copy in the workspace
    const uint32_t *d_adv_in = (const uint32_t*)advice, *d_inst_in = (const uint32_t*)instances;
    if (host) {
        uint32_t* a = pv.dalloc(std::max<size_t>(B * na * n, 1));
        uint32_t* i = pv.dalloc(std::max<size_t>(B * ni * inst_rows, 1));
        if (!a || !i) return BZH_E_OOM;
        d_adv_in = a, d_inst_in = instances ? i : nullptr;   // (staged up below, after everything that can still refuse the call)
    }

    // the results: the caller's device buffers (Montgomery until the call's last launches), or the workspace
    struct Result {
        uint64_t* dst;
        size_t elems;
        bool convert;   // (the challenges are squeezed in the caller's form)
        uint32_t* dev;
    };
    Result res[12] = {{out.advice, B * na * n, true, nullptr},
                      {out.instance, B * ni * n, true, nullptr},
                      {out.lookup_compressed, B * nl * 2 * n, true, nullptr},
                      {out.lookup_permuted, B * nl * 2 * n, true, nullptr},
                      {out.advice_polys, B * na * n, true, nullptr},
                      {out.instance_polys, B * ni * n, true, nullptr},
                      {out.lookup_polys, B * nl * 2 * n, true, nullptr},
                      {out.advice_blinds, B * na, true, nullptr},
                      {out.lookup_blinds, B * nl * 2, true, nullptr},
                      {out.theta, B, false, nullptr},
                      {out.beta, B, false, nullptr},
                      {out.gamma, B, false, nullptr}};
    for (Result& r : res) {
        r.dev = host ? pv.dalloc(std::max<size_t>(r.elems, 1)) : (uint32_t*)r.dst;
        if (host && !r.dev) return BZH_E_OOM;
    }
    uint32_t *o_adv = res[0].dev, *o_inst = res[1].dev, *o_lc = res[2].dev, *o_lp = res[3].dev, *o_advp = res[4].dev, *o_instp = res[5].dev,
             *o_lkp = res[6].dev, *o_ab = res[7].dev, *o_lb = res[8].dev, *d_theta = res[9].dev, *d_beta = res[10].dev, *d_gamma = res[11].dev;
    const size_t st_bytes = (B + 15) & ~(size_t)15;
    uint8_t* d_st = host ? (uint8_t*)arena.alloc(st_bytes) : status;
    uint32_t* drawn = pv.dalloc(B * std::max<size_t>(nd, 1));
    uint32_t* ones = pv.dalloc(std::max<size_t>(B * ni, 1));   // the instance commitments' blinds
    uint32_t* dense = pv.dalloc(std::max<size_t>(B * n, 1));   // one compressed column as the interpreter writes it
    if ((host && !d_st) || !drawn || !ones || !dense) return BZH_E_OOM;

    // everything that depends on the key and the operand pointers alone, before the first launch: the compress programs with their
    // column registries (constants: room only), the descriptors of their constants, the instance blinds; a host call's operands
    // are staged up after them.  A program that does not fit the interpreter or names another symbol than theta is refused
    // here, with at most the uploads of the programs before it queued on the stream and nothing absorbed
    pv.adv = o_adv, pv.inst = o_inst;
    std::vector<typename Prover<C>::RunProgram> progs(2 * nl);
    std::vector<CmConst> descs;
    for (size_t l = 0; l < nl; l++) {
        Cols reg;
        pv.lag_registry(reg);
        for (int side = 0; side < 2; side++) {
            typename Prover<C>::RunProgram& rp = progs[2 * l + (size_t)side];
            BZH_TRY(pv.run_args(key(20 + side, (int)l), [&](EPool& ep) { return pv.compress_root((int)l, side, ep, reg); }, reg, true, rp));
            const std::vector<ConstEnt>& cs = rp.pg->consts;
            for (size_t i = 0; i < cs.size(); i++) {
                if (cs[i].sym >= 0 && cs[i].sym != SY_THETA) return BZH_E_RANGE;
                CmConst d{};
                d.table = rp.pa.consts, d.sym = cs[i].sym >= 0 ? 0 : -1, d.nconsts = (uint32_t)cs.size(), d.index = (uint32_t)i,
                d.per_proof = rp.per_proof ? 1u : 0u;
                memcpy(d.value, cs[i].val, 32);
                descs.push_back(d);
            }
        }
    }
    void* d_descs = arena.alloc(std::max<size_t>(descs.size(), 1) * sizeof(CmConst));
    if (!d_descs) return BZH_E_OOM;
    BZH_TRY(h2d_small(ctx, d_descs, descs.data(), descs.size() * sizeof(CmConst)));
    if (ni) {
        const std::vector<Fe<SF>> one(B * ni, fe_one<SF>());
        BZH_TRY(pv.upload(ones, one.data(), one.size()));
    }

    if (host) {
        BZH_TRY(h2d_small(ctx, (void*)d_adv_in, advice, B * na * n * 32));
        if (instances) BZH_TRY(h2d_small(ctx, (void*)d_inst_in, instances, B * ni * inst_rows * 32));
    }

    // 1, 2: the columns, the instance commitments (common), the advice commitments (written), theta
    BZH_TRY(leaf_draws(pv, host, rng, rng_stride, nd, drawn));
    BZH_TRY(commitments_place(ctx, field, d_adv_in, d_inst_in, inst_rows, drawn, nd, n, usable, na, ni, B, form, o_adv, o_inst, o_ab));
    BZH_TRY(pv.to_coeff(o_instp, o_inst, B * ni));
    if (ni) BZH_TRY(leaf_commit_write(pv, tb, o_instp, ones, B * ni, ni, o_inst, 0));
    BZH_TRY(pv.to_coeff(o_advp, o_adv, B * na));
    if (na) BZH_TRY(leaf_commit_write(pv, tb, o_advp, o_ab, B * na, na, o_adv));
    BZH_TRY(tb_squeeze_locked(tb, form, d_theta));

    // 3: the lookups
    if (d_st) BZH_HIP_TRY(ctx, hipMemsetAsync(d_st, 0, host ? st_bytes : B, ctx->stream));
    if (nl) {
        BZH_TRY(commitments_consts(ctx, field, d_descs, descs.size(), B, d_theta, form));
        for (size_t c = 0; c < 2 * nl; c++) {
            BZH_TRY(pv.run_launch(progs[c], n, dense));
            BZH_TRY(pv.copy2d(o_lc + c * n * 8, nl * 2 * n, dense, n, n, B));
        }
        {
            ArenaScope scope(arena);   // (dead once enqueued, like Prover::permute_on_device's)
            void* ws = arena.alloc(lookup_permute_ws_bytes(usable, B * nl));
            if (!ws) return BZH_E_OOM;
            int32_t* d_words = nullptr;
            BZH_TRY(lookup_permute(ctx, field, o_lc, o_lc + n * 8, 2 * n, usable, B * nl, BZH_FORM_MONTGOMERY, o_lp, o_lp + n * 8, 2 * n, n, ws,
                                   &d_words));
            BZH_TRY(commitments_lookup_finish(ctx, field, drawn, nd, na * bf1 + na, n, usable, nl, B, d_words, o_lp, o_lb, d_st,
                                              tb_status_device_mut(tb)));
        }
        BZH_TRY(pv.to_coeff(o_lkp, o_lp, B * nl * 2));
        BZH_TRY(leaf_commit_write(pv, tb, o_lkp, o_lb, B * nl * 2, nl * 2, o_lp));
    }
    BZH_TRY(tb_squeeze_locked(tb, form, d_beta));
    BZH_TRY(tb_squeeze_locked(tb, form, d_gamma));

    // the outputs in the caller's form, and to the host
    if (canonical)
        for (const Result& r : res)
            if (r.convert && r.elems) BZH_TRY(field_convert(ctx, field, r.dev, r.elems, 0));
    if (!host) return BZH_OK;
    std::vector<uint8_t> st_host(st_bytes);
    for (const Result& r : res) BZH_TRY(d2h_async(ctx, r.dst, r.dev, r.elems * 32));
    BZH_TRY(d2h_async(ctx, st_host.data(), d_st, st_bytes));
    BZH_TRY(d2h_finish(ctx));
    if (status) memcpy(status, st_host.data(), B);
    return BZH_OK;
}
