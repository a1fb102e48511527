// Part of the whole-proof translation unit (csrc/prove.hip): the device-column helpers the PROVER, the VERIFIER and keygen_vk
// share -- columns of n Montgomery elements out of an arena on the ctx's stream, their transform to coefficients and their
// commitments.  The key itself is host data: only its shape (n, field, k, omega) is read here.
#pragma once
template <class C>
struct DeviceColumns {
    using SF = typename CurveInfo<C>::SF;
    using PB = typename C::Base;
    bzh_ctx* ctx;
    Arena& arena;   // this ctx's workspace of the key
    hipStream_t st;
    const size_t n;
    const int field;
    const unsigned k;
    const uint64_t* omega;   // the key's (Montgomery limbs for ntt_run)
    DeviceColumns(bzh_ctx* c, const KeyShape& ks, Arena& ar) : ctx(c), arena(ar), st(c->stream), n(ks.n), field(ks.field), k(ks.k), omega(ks.omega) {}

    uint32_t* dalloc(size_t elems) { return (uint32_t*)arena.alloc(elems * 32); }
    int zero(uint32_t* p, size_t elems) {
        BZH_HIP_TRY(ctx, hipMemsetAsync(p, 0, elems * 32, st));
        return BZH_OK;
    }
    // strided device copy of `rows` rows of `width` elements
    int copy2d(uint32_t* dst, size_t dpitch, const uint32_t* src, size_t spitch, size_t width, size_t rows) {
        if (!rows || !width) return BZH_OK;
        BZH_HIP_TRY(ctx, hipMemcpy2DAsync(dst, dpitch * 32, src, spitch * 32, width * 32, rows, hipMemcpyDeviceToDevice, st));
        return BZH_OK;
    }
    // host Montgomery elements -> device
    int upload(uint32_t* dst, const Fe<SF>* src, size_t elems) { return h2d_small(ctx, dst, src, elems * 32); }
    // `count` columns of evaluations over the domain -> coefficients (src is kept)
    int to_coeff(uint32_t* dst, const uint32_t* src, size_t count) {
        if (!count) return BZH_OK;
        BZH_HIP_TRY(ctx, hipMemcpyAsync(dst, src, count * n * 32, hipMemcpyDeviceToDevice, st));
        return ntt_run(ctx, field, dst, k, count, omega, nullptr, 1, BZH_FORM_MONTGOMERY);
    }
    // `count` Jacobian Montgomery points of an MSM -> host, affine in out_form; ends in a stream sync (d2h_finish)
    int read_points(const uint32_t* d_jac, size_t count, int out_form, uint64_t* xy) {
        std::vector<uint64_t> jac(count * 12);
        BZH_TRY(d2h_async(ctx, jac.data(), d_jac, count * 96));
        BZH_TRY(d2h_finish(ctx));
        h_jac_to_affine<PB>(jac.data(), count, BZH_FORM_MONTGOMERY, out_form, xy);
        return BZH_OK;
    }
    // Params::commit for `count` polynomials (rows of `pitch` elements) against `table` = (g | u | w): affine canonical points
    // out.  The scalar rows are (coefficients | 0 | blind).
    // (lagrange: the rows are evaluations over the domain and the table g_lagrange -- Params::commit_lagrange; the group
    // element is the same as committing the interpolated coefficients to g, but witness columns are sparse and small in
    // this basis, so most window digits are zero and cost the MSM nothing)
    // shift_row >= 0 (Lagrange basis only): the columns are constant over a long stretch that contains that row (the grand
    // products: from the last copy constraint to the blinding rows); the constant is taken out and committed on g_0, the rest
    // of the stretch becomes zero digits that the MSM's sort skips -- the same group element, the same proof bytes.
    int commit(const bzh_bases* table, const uint32_t* polys, size_t pitch, size_t count, const std::vector<Fe<SF>>& blinds,
               std::vector<uint64_t>& xy, bool lagrange = false, long shift_row = -1) {
        xy.assign(count * 8, 0);
        if (!count) return BZH_OK;
        ArenaScope scope(arena);   // the scalar vectors and the result buffer are dead when this returns (d2h_finish below)
        static const bool no_shift = getenv("BZH_NO_COMMIT_SHIFT") != nullptr;
        const bool wide = lagrange && table->n == n + 3;   // (g_lagrange | u | w | g_0): every vector spans the whole row
        const bool shift = wide && shift_row >= 0 && !no_shift && count <= 65535;
        const size_t cols = wide ? n + 3 : n + 2;
        uint32_t* sc = dalloc(count * cols);
        uint32_t* bl = dalloc(count);
        uint32_t* d_out = dalloc(count * 3);
        if (!sc || !bl || !d_out) return BZH_E_OOM;
        BZH_TRY(upload(bl, blinds.data(), count));
        if (shift) {
            hipLaunchKernelGGL((k_commit_shift<SF>), dim3((unsigned)((n + 3 + 255) / 256), (unsigned)count), dim3(256), 0, st, polys, pitch, n,
                               (size_t)shift_row, bl, sc);
            BZH_HIP_TRY(ctx, hipGetLastError());
        } else {
            BZH_TRY(zero(sc, count * cols));
            BZH_TRY(copy2d(sc, cols, polys, pitch, n, count));
            BZH_TRY(copy2d(sc + (n + 1) * 8, cols, bl, 1, 1, count));
        }
        BZH_TRY(msm_run(ctx, table, sc, cols, count, BZH_FORM_MONTGOMERY, d_out));
        return read_points(d_out, count, BZH_FORM_CANONICAL, xy.data());
    }
};
