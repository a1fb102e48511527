// Part of the whole-proof translation unit (csrc/prove.hip): the GRAND PRODUCTS on device-resident transcripts
// (bzh_grand_products_plan, bzh_grand_products_batch_device) -- phase 4 of Prover::prove as a leaf for a caller whose Fiat-Shamir
// transcripts are a bzh_transcript_batch in HBM and whose beta and gamma were squeezed into HBM.  Prover::grand_products() builds
// every numerator and denominator through the VM v1 interpreter -- 2 nsets + 2 nl launches, each with a staged program whose
// constant table the host fills from the challenges -- and finishes each product with a scale, a blind and a copy of its own.
// Here the columns are read in place through one table that depends on the key and the operand pointers alone:
//   k_gp_factors (csrc/products.hip) writes every numerator and denominator in one launch;
//   poly_batch_invert, poly_vec_mul and poly_prefix_product run over all of them, as in the Prover;
//   k_gp_finish chains the permutation sets, places the blinding rows and the blinds and reports per proof whether the products
//   close, in one launch.  Set i starts from set i - 1's z[usable], and a product started from c is c times the product started
//   from 1: z_i = raw_i * prod_{j < i} raw_j[usable], so no set has to wait for the one before it;
//   the commitments take their blinds from device memory (leaf_commit_write, vanishing_device.hpp).
// Included inside namespace bzh { namespace { after vanishing_device.hpp.
#pragma once

// the call, for a caller that holds ctx->mu and has made every argument check; nz > 0
template <class C>
static int products_device_t(bzh_ctx* ctx, bzh_pk* pk, size_t B, const uint64_t* advice, const uint64_t* instance, const uint64_t* lookup_compressed,
                             const uint64_t* lookup_permuted, const uint64_t* beta, const uint64_t* gamma, int form, int mem, const uint8_t* rng,
                             size_t rng_stride, bzh_transcript_batch* tb, uint64_t* out_z, uint64_t* out_z_polys, uint64_t* out_z_blinds,
                             uint8_t* status, bool chained = false, bool commit_evals = false) {
    Arena& arena = pk->rt.arena_for(ctx->serial, ctx->device);
    // (the merged-block rule and its one wait, and `chained`: vanishing_device_t)
    if (!chained) {
        if (arena.blocks.size() > 1) BZH_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        arena.reset();
    }
    Prover<C> pv(ctx, *pk, B, arena);
    const bool host = mem == BZH_MEM_HOST, canonical = form == BZH_FORM_CANONICAL;
    const int field = pk->field;
    const size_t n = pk->n, na = (size_t)pk->na, ni = (size_t)pk->ni, nl = (size_t)pk->nl, nsets = (size_t)pk->nsets, nz = nsets + nl,
                 bf = (size_t)pk->bf, m = pk->perm_columns.size(), nd = nz * (bf + 1);
    hipStream_t st = ctx->stream;

    // the operands as Montgomery elements in device memory: in place, or a copy in the workspace.  The copies get their place
    // first: the column table names it, and the table goes up before the first launch
    struct Operand {
        const uint64_t* src;
        size_t elems;
        bool convert;   // (k_gp_factors reads the challenges in the caller's form)
        uint32_t* copy;
        const uint32_t* dev() const { return copy ? copy : (const uint32_t*)src; }
    };
    Operand ops[6] = {{advice, B * na * n, true, nullptr},  {instance, B * ni * n, true, nullptr}, {lookup_compressed, B * nl * 2 * n, true, nullptr},
                      {lookup_permuted, B * nl * 2 * n, true, nullptr}, {beta, B, false, nullptr}, {gamma, B, false, nullptr}};
    for (Operand& o : ops) {
        if (!o.elems || (!host && !(o.convert && canonical))) continue;
        if (!(o.copy = pv.dalloc(o.elems))) return BZH_E_OOM;
    }
    const uint32_t *d_adv = ops[0].dev(), *d_inst = ops[1].dev(), *d_lc = ops[2].dev(), *d_lp = ops[3].dev();

    // the column table: per permutation set the columns of its chunk, per lookup a_c, s_c, a, s
    std::vector<GpCol> cols;
    std::vector<GpProd> prods;
    for (size_t i = 0; i < nsets; i++) {
        const size_t c0 = i * (size_t)pk->chunk_len, c1 = std::min(m, c0 + (size_t)pk->chunk_len);
        prods.push_back({(uint32_t)cols.size(), (uint32_t)(c1 - c0)});
        for (size_t gj = c0; gj < c1; gj++) {
            const std::pair<int, int> pc = pk->perm_columns[gj];
            const size_t at = (size_t)pc.second * n * 8;
            GpCol g{};
            if (pc.first == CX_ADVICE) g.v = d_adv + at, g.stride = na * n;
            else if (pc.first == CX_FIXED) g.v = pk->fixed + at, g.stride = 0;
            else g.v = d_inst + at, g.stride = ni * n;
            g.sigma = pk->sigma + gj * n * 8, g.ident = pk->ident + gj * n * 8;
            cols.push_back(g);
        }
    }
    for (size_t l = 0; l < nl; l++) {
        prods.push_back({(uint32_t)cols.size(), 4u});
        for (int j = 0; j < 4; j++) cols.push_back({(j < 2 ? d_lc : d_lp) + (2 * l + (size_t)(j & 1)) * n * 8, nl * 2 * n, nullptr, nullptr});
    }
    const size_t cols_bytes = cols.size() * sizeof(GpCol), prods_bytes = prods.size() * sizeof(GpProd);
    char* d_table = (char*)arena.alloc(cols_bytes + prods_bytes);
    if (!d_table) return BZH_E_OOM;
    {
        std::vector<char> table(cols_bytes + prods_bytes);
        memcpy(table.data(), cols.data(), cols_bytes);
        memcpy(table.data() + cols_bytes, prods.data(), prods_bytes);
        BZH_TRY(h2d_small(ctx, d_table, table.data(), table.size()));
    }
    for (const Operand& o : ops) {
        if (!o.copy) continue;
        if (host) BZH_TRY(h2d_small(ctx, o.copy, o.src, o.elems * 32));
        else BZH_HIP_TRY(ctx, hipMemcpyAsync(o.copy, o.src, o.elems * 32, hipMemcpyDeviceToDevice, st));
        if (o.convert && canonical) BZH_TRY(field_convert(ctx, field, o.copy, o.elems, 1));
    }

    // the results: the caller's device buffers (Montgomery until the call's last launches), or the workspace.  Without out_z the
    // evaluations are written where the coefficients will be and transformed in place
    uint32_t* zp = host ? pv.dalloc(B * nz * n) : (uint32_t*)out_z_polys;
    uint32_t* zs = !out_z ? zp : host ? pv.dalloc(B * nz * n) : (uint32_t*)out_z;
    uint32_t* zb = host ? pv.dalloc(B * nz) : (uint32_t*)out_z_blinds;
    const size_t st_bytes = (B + 15) & ~(size_t)15;
    uint8_t* d_st = host ? (uint8_t*)arena.alloc(st_bytes) : status;
    uint32_t* den_all = pv.dalloc(B * nz * n);
    uint32_t* zt_all = pv.dalloc(B * nz * n);
    uint32_t* drawn = pv.dalloc(B * nd);
    if (!zp || !zs || !zb || (host && !d_st) || !den_all || !zt_all || !drawn) return BZH_E_OOM;

    BZH_TRY(leaf_draws(pv, host, rng, rng_stride, nd, drawn));
    BZH_TRY(products_factors(ctx, field, d_table, d_table + cols_bytes, nsets, nl, n, B, ops[4].dev(), ops[5].dev(), form, zt_all, den_all));
    BZH_TRY(poly_batch_invert(ctx, field, den_all, nz * B * n));
    BZH_TRY(poly_vec_mul(ctx, field, zt_all, den_all, nz * B * n));
    BZH_TRY(poly_prefix_product(ctx, field, zt_all, n, nz * B));
    BZH_TRY(products_finish(ctx, field, zt_all, drawn, n, pk->usable, bf, nsets, nl, B, zs, zb, d_st, tb_status_device_mut(tb)));
    if (zs != zp) BZH_TRY(pv.to_coeff(zp, zs, B * nz));
    else BZH_TRY(ntt_run(ctx, field, zp, pk->k, B * nz, pk->omega, nullptr, 1, BZH_FORM_MONTGOMERY));
    // commit_evals (bzh_prove_batch_device, with out_z): the products over the domain go to leaf_commit_write as well, which commits
    // them against g_lagrange when the key has that table -- the same points; this leaf's own entry passes none
    BZH_TRY(leaf_commit_write(pv, tb, zp, zb, B * nz, nz, commit_evals && zs != zp ? zs : nullptr));

    // the outputs in the caller's form, and to the host
    if (canonical) {
        if (zs != zp) BZH_TRY(field_convert(ctx, field, zs, B * nz * n, 0));
        BZH_TRY(field_convert(ctx, field, zp, B * nz * n, 0));
        BZH_TRY(field_convert(ctx, field, zb, B * nz, 0));
    }
    if (!host) return BZH_OK;
    std::vector<uint8_t> st_host(st_bytes);
    if (out_z) BZH_TRY(d2h_async(ctx, out_z, zs, B * nz * n * 32));
    BZH_TRY(d2h_async(ctx, out_z_polys, zp, B * nz * n * 32));
    BZH_TRY(d2h_async(ctx, out_z_blinds, zb, B * nz * 32));
    BZH_TRY(d2h_async(ctx, st_host.data(), d_st, st_bytes));
    BZH_TRY(d2h_finish(ctx));
    if (status) memcpy(status, st_host.data(), B);
    return BZH_OK;
}
