// Whole-proof entry points: bzh_pk_create / bzh_prove_batch (boundary row b:
// "a coarser seam (whole create_proof) is what batching needs").
//
// Native counterpart of halo2_proofs 0.2.0 `plonk::{keygen_pk, create_proof}` (UPSTREAM, un-vendored:
// Cargo.lock:382-385) as called by the reference at benches/shot.rs:58-71, benches/board.rs:51-71,
// src/circuits/shot.rs:915-930, src/circuits/board.rs:907-922: one call proves `batch` independent
// witnesses of one circuit in lockstep -- every MSM, NTT, gate evaluation, scan and IPA round is ONE launch
// carrying all of them -- with the protocol, message order and randomness draw order per proof of
// create_proof, so each proof is byte-identical to proving its witness alone (the staged test drivers tests/helpers/prover_dev.py,
// oracle/halo2_oracle.py) under the same randomness stream.
//
// The circuit arrives as DATA (serialised constraint system + fixed assignment, format below): the reference's
// own constraint systems include 19 gates of the halo2_gadgets crate that is not on disk.  Host work left:
// transcripts (Blake2b), the lookup sort, challenges and blinds; everything else runs on the device out of
// one grow-only arena owned by the proving key.
//
// Circuit blob, little-endian:
//   u32 magic "BZC1" or "BZC2" | u32 k | u32 num_advice | u32 num_fixed | u32 num_instance | u32 min_degree | u8[32] vk_repr
//   u32 ngates, ngates x expr                                                   (every constraint polynomial of every gate, flattened)
//   u32 nperm, nperm x (u8 kind {0 advice, 1 fixed, 2 instance}, u32 index)
//   u32 nlookups, per lookup: u32 m, m x expr (inputs), m x expr (table)
//   u32 ncopies, ncopies x (u32 col_a, u32 row_a, u32 col_b, u32 row_b)        (indices into the permutation columns)
//   num_fixed x (u32 len, len x u8[32] canonical values)                        (rows past len are zero)
//   "BZC2" only: advice, fixed, instance query lists, each u32 count, count x (u32 column, i32 rotation), in upstream's
//   query REGISTRATION order (= the order of the evaluations in the proof); written by csrc/circuits.hip
//   expr := u8 tag, then  0 const: u8[32] | 1 advice / 2 fixed / 3 instance: u32 column, i32 rotation
//                       | 4 neg: expr | 5 add: expr expr | 6 mul: expr expr | 7 scale: expr, u8[32]
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "chacha.hpp"
#include "ctx.hpp"
#include "curve.cuh"
#include "fe29.cuh"
#include "host_field.hpp"
#include "vanishing_scalars.hpp"   // (bzh_vanishing_const as the lane body reads it)
#include "products_scalars.hpp"    // (the column table as k_gp_factors reads it)
#include "commitments_scalars.hpp" // (the constant descriptors as k_cm_consts reads them)
#include "prove_device_scalars.hpp" // (the blind sources as k_pd_blinds reads them)
#include "prove_game_scalars.hpp"   // (the status shift of k_pg_status; with it synthesize_device.hpp: the layout, the launch)
#include "vm2_isa.hpp"
#include "verify_records.hpp"      // (a record's refusal as k_vr_parse decides it: vr_record_refused_host)

// the table of quotient kernels generated at build time (quotient_builtin.hip); absent (null) in the generator's own link
extern "C" const bzh_builtin_quotient* bzh_builtin_quotients(size_t* count) __attribute__((weak));

#include "prove_kernels.cuh"     // opens namespace bzh { namespace {
#include "key_shape.hpp"         // what both keys share: blob reader, arena, KeyShape and its parser (host only)
#include "expr_compiler.hpp"     // the expression pool, the VM v1 compiler (host only)
#include "quotient_compiler.hpp" // the quotient's VM v2 program (host only)
#include "quotient_emit.hpp"     // ... as HIP source, in two limb forms (host only)
#include "proving_key.hpp"       // closes them around the global struct bzh_pk, reopens; keygen
#include "verifying_key.hpp"     // likewise around bzh_vk; its byte format and host-only entry points
#include "device_columns.hpp"     // columns on the device, their commitments: shared by prover, verifier and keygen_vk
#include "prover.hpp"
#include "vanishing_device.hpp"   // phase 5 of the prover as a leaf on device-resident transcripts
#include "products_device.hpp"    // phase 4 likewise
#include "commitments_device.hpp" // phases 1 to 3 likewise
#include "prove_device.hpp"       // the five leaves as one call: the device-resident batch prover
#include "prove_game.hpp"         // the device synthesis in front of it: game inputs in, proofs out
#include "verifier.hpp"

// pk.get_vk(): the commitments to the fixed and permutation polynomials (blind 1), computed once per key
template <class C>
static int pk_fill_vk(bzh_ctx* ctx, bzh_pk* pk) {
    Arena& arena = pk->rt.arena_for(ctx->serial, ctx->device);   // (before the lock below: arena_for takes it)
    std::lock_guard<std::mutex> lkv(pk->rt.mu);
    if (pk->vk_ready) return BZH_OK;
    ColumnCommitter<C> cc(ctx, *pk, arena);
    BZH_TRY(cc.commit(pk->srs, pk->fixed_polys, (size_t)pk->nf, pk->fixed_commitments));
    BZH_TRY(cc.commit(pk->srs, pk->sigma_polys, pk->perm_columns.size(), pk->sigma_commitments));
    pk->vk_ready = true;
    return BZH_OK;
}

// keygen_vk: the host half of keygen without the quotient program, then the fixed and permutation columns -- uploaded, taken
// to coefficients, committed with blind 1 against `srs` -- out of a workspace that is released before this returns
template <class C>
static int vk_create_t(bzh_ctx* ctx, const bzh_bases* srs, const uint8_t* blob, size_t len, bzh_vk** out) {
    using SF = typename CurveInfo<C>::SF;
    bzh_pk pk;   // host fields only: nothing below allocates into it
    ParsedKey<SF> po;
    BZH_TRY(pk_parse_t<C>(blob, len, pk, po, false));
    if (srs->n != pk.n + 2 || srs->curve != C::id) return BZH_E_ARG;
    const size_t n = pk.n, nf = (size_t)pk.nf, m = pk.perm_columns.size();
    std::unique_ptr<bzh_vk> vk(new bzh_vk());
    vk->shape = static_cast<const KeyShape&>(pk);
    vk->cs = std::move(pk.cs_bytes);
    Arena arena;
    arena.device = ctx->device;
    struct Release {
        bzh_ctx* ctx;
        Arena& a;
        ~Release() {
            (void)hipStreamSynchronize(ctx->stream);
            a.release();
        }
    } release{ctx, arena};
    ColumnCommitter<C> cc(ctx, vk->shape, arena);
    auto commit_columns = [&](const std::vector<Fe<SF>>& host, size_t count, std::vector<uint64_t>& xy) -> int {
        xy.clear();
        if (!count) return BZH_OK;
        ArenaScope scope(arena);
        uint32_t* lag = cc.dalloc(count * n);
        uint32_t* polys = cc.dalloc(count * n);
        if (!lag || !polys) return BZH_E_OOM;
        for (size_t c = 0; c < count; c++) BZH_TRY(cc.upload(lag + c * n * 8, host.data() + c * n, n));   // column by column: the staging buffer stays small
        BZH_TRY(cc.to_coeff(polys, lag, count));
        return cc.commit(srs, polys, count, xy);
    };
    BZH_TRY(commit_columns(po.fixed_h, nf, vk->shape.fixed_commitments));
    {   // the permutation polynomials' values: column j, row r -> delta^(column) omega^(row) of the cell the cycle maps it to
        std::vector<Fe<SF>> wp(n), dpow(m ? m : 1), host(m * n);
        wp[0] = fe_one<SF>();
        for (size_t i = 1; i < n; i++) wp[i] = fe_mul(wp[i - 1], po.omega);
        dpow[0] = fe_one<SF>();
        for (size_t j = 1; j < m; j++) dpow[j] = fe_mul(dpow[j - 1], po.delta);
        for (size_t i = 0; i < m * n; i++) host[i] = fe_mul(dpow[po.map_c[i]], wp[po.map_r[i]]);
        BZH_TRY(commit_columns(host, m, vk->shape.sigma_commitments));
    }
    *out = vk.release();
    return BZH_OK;
}

}  // namespace

// k_chacha20_rows for a caller outside this translation unit (bzh_params_read, csrc/params.hip): see csrc/ctx.hpp
int rng_rows_device(bzh_ctx* ctx, const uint32_t* d_keys, uint64_t counter0, size_t count, size_t batch, uint32_t* d_raw) {
    if (!count || !batch) return BZH_OK;
    if (batch > 65535) return BZH_E_ARG;
    hipLaunchKernelGGL(k_chacha20_rows, dim3((unsigned)((count + 255) / 256), (unsigned)batch), dim3(256), 0, ctx->stream, d_keys, counter0, count,
                       d_raw);
    BZH_HIP_TRY(ctx, hipGetLastError());
    return BZH_OK;
}
}  // namespace bzh

namespace {
// degree (in units of n - 1: every column polynomial has degree < n) and tree multiplications of the quotient's terms
template <class C>
static int quotient_histogram_t(const uint8_t* circuit, size_t circuit_len, uint32_t* polys, uint32_t* muls) {
    using SF = typename bzh::CurveInfo<C>::SF;
    bzh_pk pk;
    bzh::ParsedKey<SF> po;
    const int rc = bzh::pk_parse_t<C>(circuit, circuit_len, pk, po);
    if (rc) return rc;
    bzh::Cols reg;
    bzh::quotient_registry(pk, bzh::QuotientPtrs{}, false, reg);
    bzh::EPool ep;
    int tinv = -1;
    const std::vector<int> terms = bzh::quotient_terms<SF>(pk, reg, ep, &tinv);
    std::vector<int> deg(ep.n.size(), 0), mu(ep.n.size(), 0);
    for (size_t i = 0; i < ep.n.size(); i++) {   // children precede parents in the pool
        const bzh::ENode& e = ep.n[i];
        switch (e.tag) {
            case bzh::EX_QUERY: deg[i] = 1; break;
            case bzh::EX_NEG: deg[i] = deg[e.a], mu[i] = mu[e.a]; break;
            case bzh::EX_SCALE: deg[i] = deg[e.a], mu[i] = mu[e.a] + 1; break;
            case bzh::EX_ADD: deg[i] = std::max(deg[e.a], deg[e.b]), mu[i] = mu[e.a] + mu[e.b]; break;
            case bzh::EX_MUL: deg[i] = deg[e.a] + deg[e.b], mu[i] = mu[e.a] + mu[e.b] + 1; break;
            default: break;
        }
    }
    for (int d = 0; d < 16; d++) polys[d] = muls[d] = 0;
    for (int t : terms) {
        const int d = std::min(deg[t], 15);
        polys[d]++;
        muls[d] += (uint32_t)mu[t];
    }
    return BZH_OK;
}
}  // namespace


namespace {
// G_0, U, W of a table (g | u | w), canonical affine: row 0 of a window table is the raw table
static int srs_g0_u_w(bzh_ctx* ctx, const bzh_bases* srs, std::vector<uint64_t>& canon) {
    uint64_t m[3 * 8];
    const size_t idx[3] = {0, srs->n - 2, srs->n - 1};
    for (int i = 0; i < 3; i++)
        BZH_HIP_TRY(ctx, hipMemcpyAsync(&m[i * 8], srs->d_xy + idx[i] * 16, 64, hipMemcpyDeviceToHost, ctx->stream));
    BZH_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    canon.assign(24, 0);
    return bzh::with_pasta_curve(srs->curve, [&](auto c) {
        using PB = typename decltype(c)::Base;
        for (int i = 0; i < 6; i++) bzh::fe_to_u64<PB>(&canon[i * 4], bzh::fe_from_u64<PB>(&m[i * 4]), BZH_FORM_CANONICAL);
        return BZH_OK;
    });
}
}  // namespace

extern "C" {

int bzh_pk_create(bzh_ctx* ctx, const bzh_bases* srs, const uint8_t* circuit, size_t circuit_len, bzh_pk** out) {
    if (!ctx || !srs || !circuit || !out || srs->device != ctx->device) return BZH_E_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    BZH_HIP_TRY(ctx, hipSetDevice(ctx->device));
    // (not BN254: no cube root of unity in Fr's multiplicative generator convention used here)
    return bzh::with_pasta_curve(srs->curve, [&](auto c) { return bzh::pk_create_t<decltype(c)>(ctx, srs, circuit, circuit_len, out); });
}

int bzh_pk_free(bzh_ctx* ctx, bzh_pk* pk) {
    if (!ctx || !pk) return BZH_E_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!pk->rt.retire()) {   // another ctx is proving / verifying on this key: its arena and code would vanish under it
        ctx->last_error = "bzh_pk_free: a bzh_prove_batch / bzh_verify_batch call on this key is still running";
        return BZH_E_ARG;
    }
    // (retire has synchronised every device the key holds a workspace on; a key without one has run no call, and
    // bzh_pk_create waited for its own work: nothing queued reads what goes now)
    (void)hipSetDevice(pk->device);
    if (pk->dev) (void)hipFree(pk->dev);
    if (pk->hoist) (void)hipFree(pk->hoist);
    if (pk->key29) (void)hipFree(pk->key29);
    if (pk->q_module) (void)hipModuleUnload(pk->q_module);
    delete pk;
    return BZH_OK;
}

int bzh_pk_set_lagrange(bzh_pk* pk, const bzh_bases* g_lagrange) {
    if (!pk) return BZH_E_ARG;
    if (g_lagrange && ((g_lagrange->n != pk->n + 2 && g_lagrange->n != pk->n + 3) || g_lagrange->curve != pk->curve || g_lagrange->device != pk->device || !g_lagrange->pre_c))
        return BZH_E_ARG;
    std::lock_guard<std::mutex> lk(pk->rt.mu);
    pk->srs_lagrange = g_lagrange;
    return BZH_OK;
}

int bzh_pk_quotient_stats(bzh_pk* pk, uint32_t* ops, uint32_t* multiplications, uint32_t* lds_slots, uint32_t* hoisted_columns) {
    if (!pk) return BZH_E_ARG;
    uint32_t no = 0, nm = 0, nl = 0;
    if (pk->q_ok) {
        no = (uint32_t)pk->qprog.ops.size();
        nl = (uint32_t)pk->qprog.nlds;
        nm = (uint32_t)bzh::program2_muls(pk->qprog);
    }
    if (ops) *ops = no;
    if (multiplications) *multiplications = nm;
    if (lds_slots) *lds_slots = nl;
    if (hoisted_columns) *hoisted_columns = (uint32_t)pk->hoist_cols;
    return BZH_OK;
}

int bzh_pk_quotient_loads(bzh_pk* pk, uint32_t* loads_per_row, uint32_t* leaf_slots) {
    if (!pk) return BZH_E_ARG;
    if (loads_per_row) *loads_per_row = pk->q_ok ? (uint32_t)bzh::program2_loads(pk->qprog) : 0;
    if (leaf_slots) *leaf_slots = pk->q_ok ? (uint32_t)pk->qprog.leaf_slots : 0;
    return BZH_OK;
}

static int copy_text(const std::string& src, char* buf, size_t cap, size_t* len) {
    *len = src.size();
    if (buf && cap) {
        const size_t n = std::min(cap - 1, src.size());
        memcpy(buf, src.data(), n);
        buf[n] = 0;
    }
    return BZH_OK;
}

int bzh_pk_quotient_source(bzh_pk* pk, char* buf, size_t cap, size_t* len) {
    if (!pk || !len) return BZH_E_ARG;
    if (!pk->q_ok) return BZH_E_RANGE;   // the circuit does not fit VM v2
    return copy_text(bzh::program2_source(pk->qprog, pk->field), buf, cap, len);
}

int bzh_quotient_source_for_circuit(int curve, const uint8_t* circuit, size_t circuit_len, char* buf, size_t cap, size_t* len,
                                    uint64_t* program_hash) {
    if (!circuit || !len) return BZH_E_ARG;
    bzh_pk pk;
    BZH_TRY(bzh::with_pasta_curve(curve, [&](auto c) {
        using C = decltype(c);
        bzh::ParsedKey<typename bzh::CurveInfo<C>::SF> po;
        return bzh::pk_parse_t<C>(circuit, circuit_len, pk, po);
    }));
    if (!pk.q_ok) return BZH_E_RANGE;
    if (program_hash) *program_hash = pk.q_hash;
    // two flavours of the same program: saturated limbs (namespace bzh_q_<hash>) and unsaturated 9 x 29-bit limbs (bzh_q29_<hash>)
    return copy_text(bzh::program2_source(pk.qprog, pk.field, true) + "\n" + bzh::program2_source29(pk.qprog, pk.field), buf, cap, len);
}

int bzh_quotient_program_for_circuit(int curve, const uint8_t* circuit, size_t circuit_len, void* ops, size_t ops_cap, size_t* nops,
                                     void* consts, size_t consts_cap, size_t* nconsts, uint32_t* stats8) {
    if (!circuit || !nops || !nconsts) return BZH_E_ARG;
    bzh_pk pk;
    BZH_TRY(bzh::with_pasta_curve(curve, [&](auto c) {
        using C = decltype(c);
        bzh::ParsedKey<typename bzh::CurveInfo<C>::SF> po;
        return bzh::pk_parse_t<C>(circuit, circuit_len, pk, po);
    }));
    if (!pk.q_ok) return BZH_E_RANGE;
    const bzh::Program2& pg = pk.qprog;
    *nops = pg.ops.size();
    *nconsts = pg.consts.size();
    if (stats8) {
        const uint32_t st[8] = {(uint32_t)pg.ops.size(), (uint32_t)bzh::program2_muls(pg), (uint32_t)pg.nlds, (uint32_t)bzh::program2_loads(pg), (uint32_t)pg.leaf_slots,
                                (uint32_t)pg.leaf_base, (uint32_t)pk.hoist_cols, 0};
        memcpy(stats8, st, sizeof(st));
    }
    if (ops) {
        if (ops_cap < pg.ops.size() * sizeof(bzh::ExprOp2)) return BZH_E_ARG;
        memcpy(ops, pg.ops.data(), pg.ops.size() * sizeof(bzh::ExprOp2));
    }
    if (consts) {
        if (consts_cap < pg.consts.size() * 40) return BZH_E_ARG;
        for (size_t i = 0; i < pg.consts.size(); i++) {
            uint32_t w[10] = {(uint32_t)pg.consts[i].sym, 0};
            memcpy(w + 2, pg.consts[i].val, 32);
            memcpy((uint8_t*)consts + 40 * i, w, 40);
        }
    }
    return BZH_OK;
}

int bzh_quotient_degree_histogram(int curve, const uint8_t* circuit, size_t circuit_len, uint32_t* polys, uint32_t* muls) {
    if (!circuit || !polys || !muls) return BZH_E_ARG;
    return bzh::with_pasta_curve(curve, [&](auto c) { return quotient_histogram_t<decltype(c)>(circuit, circuit_len, polys, muls); });
}

int bzh_pk_quotient_select(bzh_pk* pk, int flavour) {
    if (!pk) return BZH_E_ARG;
    std::lock_guard<std::mutex> lk(pk->rt.mu);
    switch (flavour) {
        case BZH_QUOTIENT_INTERPRETER: break;
        case BZH_QUOTIENT_BUILTIN:
            if (!pk->q_builtin) return BZH_E_RANGE;
            break;
        case BZH_QUOTIENT_MODULE:
            if (!pk->q_fn) return BZH_E_RANGE;
            break;
        default: return BZH_E_ARG;
    }
    pk->q_select = flavour;
    return BZH_OK;
}

int bzh_pk_quotient_selected(bzh_pk* pk, int* flavour, int* builtin_available) {
    if (!pk) return BZH_E_ARG;
    std::lock_guard<std::mutex> lk(pk->rt.mu);
    if (flavour) *flavour = pk->q_select;
    if (builtin_available) *builtin_available = pk->q_builtin != nullptr;
    return BZH_OK;
}

int bzh_pk_lookup_select(bzh_pk* pk, int where) {
    if (!pk || (where != BZH_LOOKUP_HOST && where != BZH_LOOKUP_DEVICE)) return BZH_E_ARG;
    std::lock_guard<std::mutex> lk(pk->rt.mu);
    pk->lk_select = where;
    pk->lk_chosen = true;
    return BZH_OK;
}

int bzh_pk_lookup_selected(bzh_pk* pk, int* where) {
    if (!pk) return BZH_E_ARG;
    std::lock_guard<std::mutex> lk(pk->rt.mu);
    if (where) *where = pk->lk_select;
    return BZH_OK;
}

int bzh_pk_workspace_select(bzh_pk* pk, int mode) {
    if (!pk || (mode != BZH_WORKSPACE_EXTENDED && mode != BZH_WORKSPACE_COSETWISE)) return BZH_E_ARG;
    std::lock_guard<std::mutex> lk(pk->rt.mu);
    pk->ws_select = mode;
    return BZH_OK;
}

int bzh_pk_workspace_selected(bzh_pk* pk, int* mode) {
    if (!pk) return BZH_E_ARG;
    std::lock_guard<std::mutex> lk(pk->rt.mu);
    if (mode) *mode = pk->ws_select;
    return BZH_OK;
}

int bzh_workspace_plan_items(int curve, const uint8_t* circuit, size_t circuit_len, size_t batch, int mode, bzh_workspace_items* items) {
    if (!circuit || !items || !batch || batch > 65535 || (mode != BZH_WORKSPACE_EXTENDED && mode != BZH_WORKSPACE_COSETWISE))
        return BZH_E_ARG;
    bzh_pk pk;
    BZH_TRY(bzh::with_pasta_curve(curve, [&](auto c) {
        bzh::ParsedKey<typename bzh::CurveInfo<decltype(c)>::SF> po;
        return bzh::pk_parse_t<decltype(c)>(circuit, circuit_len, pk, po, false);   // counts only: no quotient program is compiled
    }));
    const bzh::WorkspaceItems w = bzh::workspace_items(pk, batch, mode);
    items->n = pk.n, items->extended = pk.en;
    items->columns = (uint64_t)std::max(pk.na, 1) + (uint64_t)std::max(pk.ni, 1) + (uint64_t)std::max(pk.nsets + pk.nl, 1) + 2 * (uint64_t)pk.nl;
    items->column_bytes = w.column_bytes;
    items->cosets_bytes = w.cosets_bytes, items->cosets_extended_bytes = w.cosets_extended_bytes;
    items->witness_bytes = w.witness_bytes, items->quotient_bytes = w.quotient_bytes, items->tail_bytes = w.tail_bytes;
    items->staging_bytes = w.staging_bytes;
    items->total_bytes = w.total_bytes;
    return BZH_OK;
}

int bzh_pk_workspace_peak(const bzh_pk* pk, size_t* arena_bytes) {
    if (!pk || !arena_bytes) return BZH_E_ARG;
    std::lock_guard<std::mutex> lk(const_cast<bzh_pk*>(pk)->rt.mu);
    size_t peak = 0;
    for (auto& kv : pk->rt.arenas) peak = std::max(peak, kv.second->peak);
    *arena_bytes = peak;
    return BZH_OK;
}

int bzh_workspace_plan(int curve, const uint8_t* circuit, size_t circuit_len, size_t batch, int mode, size_t* arena_bytes) {
    if (!arena_bytes) return BZH_E_ARG;
    bzh_workspace_items items;
    BZH_TRY(bzh_workspace_plan_items(curve, circuit, circuit_len, batch, mode, &items));
    *arena_bytes = (size_t)items.total_bytes;
    return BZH_OK;
}

int bzh_pk_verify_select(bzh_pk* pk, int where) {
    if (!pk || (where != BZH_VERIFY_POINTS_HOST && where != BZH_VERIFY_POINTS_DEVICE)) return BZH_E_ARG;
    std::lock_guard<std::mutex> lk(pk->rt.mu);
    pk->vp_select = where;
    return BZH_OK;
}

int bzh_pk_verify_selected(bzh_pk* pk, int* where) {
    if (!pk) return BZH_E_ARG;
    std::lock_guard<std::mutex> lk(pk->rt.mu);
    if (where) *where = pk->vp_select;
    return BZH_OK;
}

int bzh_pk_verify_pass_select(bzh_pk* pk, int where) {
    if (!pk || (where != BZH_VERIFY_PASS_HOST && where != BZH_VERIFY_PASS_DEVICE)) return BZH_E_ARG;
    std::lock_guard<std::mutex> lk(pk->rt.mu);
    pk->vpass_select = where;
    return BZH_OK;
}

int bzh_pk_verify_pass_selected(bzh_pk* pk, int* where) {
    if (!pk) return BZH_E_ARG;
    std::lock_guard<std::mutex> lk(pk->rt.mu);
    if (where) *where = pk->vpass_select;
    return BZH_OK;
}

int bzh_pk_set_quotient_module(bzh_ctx* ctx, bzh_pk* pk, const void* code_object, size_t len) {
    if (!ctx || !pk || pk->device != ctx->device) return BZH_E_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    std::lock_guard<std::mutex> lkp(pk->rt.mu);
    BZH_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (pk->rt.calls) {   // a call on another ctx may hold q_fn and be about to launch it
        ctx->last_error = "bzh_pk_set_quotient_module: a bzh_prove_batch / bzh_verify_batch call on this key is still running";
        return BZH_E_ARG;
    }
    if (pk->q_module) {
        (void)hipDeviceSynchronize();   // launches of the old code object queued on ANY ctx's stream
        (void)hipModuleUnload(pk->q_module);
        pk->q_module = nullptr;
        pk->q_fn = nullptr;
    }
    if (pk->q_select == BZH_QUOTIENT_MODULE) pk->q_select = pk->q_builtin ? BZH_QUOTIENT_BUILTIN : BZH_QUOTIENT_INTERPRETER;
    if (!code_object || !len) return BZH_OK;   // back to the key's default
    if (!pk->q_ok) return BZH_E_RANGE;
    hipModule_t mod = nullptr;
    BZH_HIP_TRY(ctx, hipModuleLoadData(&mod, code_object));
    hipFunction_t fn = nullptr;
    hipDeviceptr_t hsym = nullptr;
    size_t hbytes = 0;
    unsigned long long have = 0;
    const bool ok = hipModuleGetFunction(&fn, mod, "jit_quotient") == hipSuccess &&
                    hipModuleGetGlobal(&hsym, &hbytes, mod, "jit_program_hash") == hipSuccess && hbytes == 8 &&
                    hipMemcpy(&have, hsym, 8, hipMemcpyDeviceToHost) == hipSuccess && have == pk->q_hash;
    if (!ok) {
        (void)hipModuleUnload(mod);
        ctx->last_error = "bzh_pk_set_quotient_module: not a module generated from this key's quotient program";
        return BZH_E_ARG;
    }
    pk->q_module = mod;
    pk->q_fn = fn;
    pk->q_select = BZH_QUOTIENT_MODULE;
    return BZH_OK;
}

int bzh_pk_info(const bzh_pk* pk, size_t* rng_bytes_per_proof, size_t* max_proof_bytes, uint32_t* num_advice, uint32_t* n_rows,
                uint32_t* usable_rows) {
    if (!pk) return BZH_E_ARG;
    if (rng_bytes_per_proof) *rng_bytes_per_proof = pk->rng_bytes;
    if (max_proof_bytes) *max_proof_bytes = pk->max_proof_bytes();
    if (num_advice) *num_advice = (uint32_t)pk->na;
    if (n_rows) *n_rows = (uint32_t)pk->n;
    if (usable_rows) *usable_rows = (uint32_t)pk->usable;
    return BZH_OK;
}

int bzh_pk_vk_repr(const bzh_pk* pk, uint8_t* out_repr32, int* is_placeholder) {
    if (!pk) return BZH_E_ARG;
    if (out_repr32) memcpy(out_repr32, pk->vk_repr, 32);
    if (is_placeholder) *is_placeholder = pk->vk_repr_is_placeholder() ? 1 : 0;
    return BZH_OK;
}

int bzh_verify_batch(bzh_ctx* ctx, bzh_pk* pk, size_t batch, const uint64_t* instances, size_t instance_rows, const uint8_t* proofs,
                     size_t proof_stride, const size_t* proof_lens, const uint64_t* g0_u_w, int* results) {
    if (!ctx || !pk || !batch || batch > 4096 || !proofs || !proof_lens || !g0_u_w || !results) return BZH_E_ARG;
    bzh::KeyRuntime::Call in_flight(pk->rt);   // registered before the wait for ctx->mu: a queued call already makes bzh_pk_free refuse
    if (pk->device != ctx->device || (pk->ni && instance_rows && !instances) || instance_rows > pk->usable) return BZH_E_ARG;
    for (size_t b = 0; b < batch; b++)
        if (proof_lens[b] > proof_stride) return BZH_E_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    BZH_HIP_TRY(ctx, hipSetDevice(ctx->device));
    // The commitments of the key and G'_0 are computed against pk->srs: the three points the caller passes must be the
    // same SRS's, or every valid proof would be rejected without an error.  Row 0 of the window table is the raw SRS.
    std::unique_lock<std::mutex> lkp(pk->rt.mu);
    if (pk->srs_g0_u_w.empty()) {
        std::vector<uint64_t> canon;
        BZH_TRY(srs_g0_u_w(ctx, pk->srs, canon));
        pk->srs_g0_u_w = std::move(canon);
    }
    if (memcmp(pk->srs_g0_u_w.data(), g0_u_w, 3 * 64) != 0) {
        ctx->last_error = "bzh_verify_batch: g0_u_w are not G_0, U, W of the SRS this key was built on";
        return BZH_E_ARG;
    }
    const bool points_on_device = pk->vp_select == BZH_VERIFY_POINTS_DEVICE;
    const bool pass_on_device = pk->vpass_select == BZH_VERIFY_PASS_DEVICE;
    lkp.unlock();
    bzh::Arena& arena = pk->rt.arena_for(ctx->serial, ctx->device);
    const int rc = bzh::with_pasta_curve(pk->curve, [&](auto c) {
        using C = decltype(c);
        arena.reset();
        BZH_TRY(bzh::pk_fill_vk<C>(ctx, pk));
        if (pass_on_device)
            return bzh::verify_batch_device_t<C>(ctx, *pk, pk->srs, nullptr, arena, batch, instances, instance_rows, proofs, proof_stride, proof_lens,
                                                 g0_u_w, nullptr, results, nullptr);
        return bzh::verify_batch_t<C>(ctx, *pk, pk->srs, nullptr, arena, points_on_device, batch, instances, instance_rows, proofs, proof_stride,
                                      proof_lens, g0_u_w, results);
    });
    (void)hipStreamSynchronize(ctx->stream);
    return rc;
}

int bzh_pk_device_bytes(const bzh_pk* pk, size_t* key_bytes, size_t* workspace_bytes) {
    if (!pk) return BZH_E_ARG;
    std::lock_guard<std::mutex> lk(const_cast<bzh_pk*>(pk)->rt.mu);
    if (key_bytes) *key_bytes = pk->dev_bytes + pk->hoist_bytes + pk->key29_bytes;
    if (workspace_bytes) *workspace_bytes = pk->rt.held_locked();
    return BZH_OK;
}

int bzh_vk_create(bzh_ctx* ctx, const bzh_bases* srs, const uint8_t* circuit, size_t circuit_len, bzh_vk** out) {
    if (!ctx || !srs || !circuit || !out || srs->device != ctx->device) return BZH_E_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    BZH_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return bzh::with_pasta_curve(srs->curve, [&](auto c) { return bzh::vk_create_t<decltype(c)>(ctx, srs, circuit, circuit_len, out); });
}

int bzh_vk_from_pk(bzh_ctx* ctx, bzh_pk* pk, bzh_vk** out) {
    if (!ctx || !pk || !out) return BZH_E_ARG;
    bzh::KeyRuntime::Call in_flight(pk->rt);
    if (pk->device != ctx->device) return BZH_E_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    BZH_HIP_TRY(ctx, hipSetDevice(ctx->device));
    bzh::Arena& arena = pk->rt.arena_for(ctx->serial, ctx->device);
    BZH_TRY(bzh::with_pasta_curve(pk->curve, [&](auto c) {
        arena.reset();
        return bzh::pk_fill_vk<decltype(c)>(ctx, pk);
    }));
    std::unique_ptr<bzh_vk> vk(new bzh_vk());
    vk->shape = static_cast<const bzh::KeyShape&>(*pk);
    vk->cs = pk->cs_bytes;
    *out = vk.release();
    return BZH_OK;
}

int bzh_verify_batch_vk(bzh_ctx* ctx, const bzh_vk* vk, const bzh_bases* srs, const bzh_bases* g_lagrange, size_t batch,
                        const uint64_t* instances, size_t instance_rows, const uint8_t* proofs, size_t proof_stride,
                        const size_t* proof_lens, const uint64_t* g0_u_w, int* results) {
    return bzh_verify_batch_vk_with(ctx, vk, srs, g_lagrange, BZH_VERIFY_PASS_HOST, batch, instances, instance_rows, proofs, proof_stride,
                                    proof_lens, g0_u_w, results);
}

// bzh_verify_batch_vk_with, and with a seed bzh_verify_batch_vk_accumulated: the same checks, the same front door
static int verify_batch_vk_entry(bzh_ctx* ctx, const bzh_vk* vk, const bzh_bases* srs, const bzh_bases* g_lagrange, int pass_where,
                                 size_t batch, const uint64_t* instances, size_t instance_rows, const uint8_t* proofs, size_t proof_stride,
                                 const size_t* proof_lens, const uint64_t* g0_u_w, const uint8_t* seed, int* results, int* path) {
    if (pass_where != BZH_VERIFY_PASS_HOST && pass_where != BZH_VERIFY_PASS_DEVICE) return BZH_E_ARG;
    if (!ctx || !vk || !srs || !batch || batch > 4096 || !proofs || !proof_lens || !g0_u_w || !results) return BZH_E_ARG;
    bzh::KeyRuntime::Call in_flight(vk->rt);
    const bzh::KeyShape& key = vk->shape;
    if (srs->device != ctx->device || srs->curve != key.curve || srs->n != key.n + 2) return BZH_E_ARG;
    if (g_lagrange && (g_lagrange->device != ctx->device || g_lagrange->curve != key.curve || (g_lagrange->n != key.n + 2 && g_lagrange->n != key.n + 3)))
        return BZH_E_ARG;
    if ((key.ni && instance_rows && !instances) || instance_rows > key.usable) return BZH_E_ARG;
    for (size_t b = 0; b < batch; b++)
        if (proof_lens[b] > proof_stride) return BZH_E_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    BZH_HIP_TRY(ctx, hipSetDevice(ctx->device));
    // the key's commitments and G'_0 belong to one SRS: the three points the caller passes must be that table's
    std::vector<uint64_t> canon;
    BZH_TRY(srs_g0_u_w(ctx, srs, canon));
    if (memcmp(canon.data(), g0_u_w, 3 * 64) != 0) {
        ctx->last_error = "bzh_verify_batch_vk: g0_u_w are not G_0, U, W of srs";
        return BZH_E_ARG;
    }
    bzh::Arena& arena = vk->rt.arena_for(ctx->serial, ctx->device);
    const int rc = bzh::with_pasta_curve(key.curve, [&](auto c) {
        if (pass_where == BZH_VERIFY_PASS_DEVICE)
            return bzh::verify_batch_device_t<decltype(c)>(ctx, key, srs, g_lagrange, arena, batch, instances, instance_rows, proofs, proof_stride,
                                                           proof_lens, g0_u_w, seed, results, path);
        return bzh::verify_batch_t<decltype(c)>(ctx, key, srs, g_lagrange, arena, false, batch, instances, instance_rows, proofs, proof_stride,
                                                proof_lens, g0_u_w, results);
    });
    (void)hipStreamSynchronize(ctx->stream);
    return rc;
}

int bzh_verify_batch_vk_with(bzh_ctx* ctx, const bzh_vk* vk, const bzh_bases* srs, const bzh_bases* g_lagrange, int pass_where,
                             size_t batch, const uint64_t* instances, size_t instance_rows, const uint8_t* proofs, size_t proof_stride,
                             const size_t* proof_lens, const uint64_t* g0_u_w, int* results) {
    return verify_batch_vk_entry(ctx, vk, srs, g_lagrange, pass_where, batch, instances, instance_rows, proofs, proof_stride, proof_lens, g0_u_w,
                                 nullptr, results, nullptr);
}

// bzh_verify_records_device, and with a seed bzh_verify_records_accumulated: the same checks, the same front door
static int verify_records_entry(bzh_ctx* ctx, const bzh_vk* vk, const bzh_bases* srs, const bzh_bases* g_lagrange, size_t batch, size_t n_inputs,
                                const uint8_t* records, size_t record_stride, const uint64_t* g0_u_w, const uint8_t* seed, int* results,
                                uint8_t* status, int* path) {
    if (!ctx || !vk || !srs || !g_lagrange || !records || !results) return BZH_E_ARG;
    if (!n_inputs || n_inputs > BZH_RECORD_MAX_INPUTS || batch > bzh::kVerifyRecordsMaxBatch) return BZH_E_ARG;
    bzh::KeyRuntime::Call in_flight(vk->rt);
    const bzh::KeyShape& key = vk->shape;
    // what reads the key alone comes before what reads the tables
    if (key.ni != 1 || n_inputs > key.usable) return BZH_E_ARG;   // the reference's circuits: one instance column, its first rows
    // (a key without a tape has no proof length to hold the stride against: that is BZH_E_RANGE below, whatever the stride)
    if (key.vprog.ok && (record_stride < BZH_RECORD_HEADER_BYTES || record_stride - BZH_RECORD_HEADER_BYTES < key.vprog.proof_len)) return BZH_E_ARG;
    if (srs->device != ctx->device || srs->curve != key.curve || srs->n != key.n + 2) return BZH_E_ARG;
    if (g_lagrange->device != ctx->device || g_lagrange->curve != key.curve || (g_lagrange->n != key.n + 2 && g_lagrange->n != key.n + 3))
        return BZH_E_ARG;
    if (!batch) return BZH_OK;
    std::lock_guard<std::mutex> lk(ctx->mu);
    BZH_HIP_TRY(ctx, hipSetDevice(ctx->device));
    bzh::Arena& arena = vk->rt.arena_for(ctx->serial, ctx->device);
    return bzh::with_pasta_curve(key.curve, [&](auto c) {
        return bzh::verify_records_t<decltype(c)>(ctx, key, srs, g_lagrange, arena, batch, n_inputs, records, record_stride, g0_u_w, seed,
                                                  results, status, path);
    });
}

int bzh_verify_records_device(bzh_ctx* ctx, const bzh_vk* vk, const bzh_bases* srs, const bzh_bases* g_lagrange, size_t batch, size_t n_inputs,
                              const uint8_t* records, size_t record_stride, const uint64_t* g0_u_w, int* results, uint8_t* status) {
    return verify_records_entry(ctx, vk, srs, g_lagrange, batch, n_inputs, records, record_stride, g0_u_w, nullptr, results, status, nullptr);
}

// rng_stride == 0: `rng` holds batch x 32-byte seeds (bzh_prove_batch_seeded)
static int prove_batch_entry(bzh_ctx* ctx, bzh_pk* pk, size_t batch, const uint64_t* advice, int form, int mem, const uint64_t* instances,
                             size_t instance_rows, const uint8_t* rng, size_t rng_stride, uint8_t* proofs, size_t proof_stride,
                             size_t* proof_lens) {
    if (!ctx || !pk || !batch || batch > 4096 || !advice || !rng || !proofs || !proof_lens) return BZH_E_ARG;
    bzh::KeyRuntime::Call in_flight(pk->rt);   // until the proofs are in the caller's buffers (prove_batch_t synchronises the stream before it returns)
    if ((form != BZH_FORM_CANONICAL && form != BZH_FORM_MONTGOMERY) || (mem != BZH_MEM_HOST && mem != BZH_MEM_DEVICE)) return BZH_E_ARG;
    if (pk->device != ctx->device || (rng_stride != 0 && rng_stride < pk->rng_bytes) || (pk->ni && instance_rows && !instances) ||
        instance_rows > pk->usable)
        return BZH_E_ARG;
    if (mem == BZH_MEM_DEVICE && form != BZH_FORM_MONTGOMERY) return BZH_E_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    BZH_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint32_t* d_adv = (const uint32_t*)advice;
    void* staged = nullptr;
    const size_t elems = batch * (size_t)pk->na * pk->n;
    if (mem == BZH_MEM_HOST) {
        int rc = bzh::ws_ensure(ctx, bzh::WS_STAGE, elems * 32 + 256, &staged);
        if (rc) return rc;
        BZH_HIP_TRY(ctx, hipMemcpyAsync(staged, advice, elems * 32, hipMemcpyHostToDevice, ctx->stream));
        if (form == BZH_FORM_CANONICAL && (rc = bzh::field_convert(ctx, pk->field, (uint32_t*)staged, elems, 1))) return rc;
        d_adv = (const uint32_t*)staged;
    }
    return bzh::with_pasta_curve(pk->curve, [&](auto c) {
        return bzh::prove_batch_t<decltype(c)>(ctx, pk, batch, d_adv, instances, instance_rows, rng, rng_stride, proofs, proof_stride, proof_lens);
    });
}

int bzh_prove_batch(bzh_ctx* ctx, bzh_pk* pk, size_t batch, const uint64_t* advice, int form, int mem, const uint64_t* instances,
                    size_t instance_rows, const uint8_t* rng, size_t rng_stride, uint8_t* proofs, size_t proof_stride,
                    size_t* proof_lens) {
    if (rng_stride == 0) return BZH_E_ARG;
    return prove_batch_entry(ctx, pk, batch, advice, form, mem, instances, instance_rows, rng, rng_stride, proofs, proof_stride, proof_lens);
}

int bzh_prove_batch_seeded(bzh_ctx* ctx, bzh_pk* pk, size_t batch, const uint64_t* advice, int form, int mem, const uint64_t* instances,
                           size_t instance_rows, const uint8_t* seeds, uint8_t* proofs, size_t proof_stride, size_t* proof_lens) {
    return prove_batch_entry(ctx, pk, batch, advice, form, mem, instances, instance_rows, seeds, 0, proofs, proof_stride, proof_lens);
}

int bzh_vanishing_plan(int curve, const uint8_t* circuit, size_t circuit_len, uint32_t shape8[8], bzh_vanishing_const* consts,
                       size_t consts_cap, size_t* nconsts) {
    if (!circuit || !shape8 || !consts || !nconsts) return BZH_E_ARG;
    bzh_pk pk;
    std::vector<bzh::VnConst> descs;
    BZH_TRY(bzh::with_pasta_curve(curve, [&](auto c) {
        using SF = typename bzh::CurveInfo<decltype(c)>::SF;
        bzh::ParsedKey<SF> po;
        BZH_TRY(bzh::pk_parse_t<decltype(c)>(circuit, circuit_len, pk, po));
        return bzh::vanishing_consts_plan<SF>(pk, descs);
    }));
    if (consts_cap < descs.size()) return BZH_E_ARG;
    const uint32_t shape[8] = {(uint32_t)pk.n,  (uint32_t)pk.en, (uint32_t)pk.na,      (uint32_t)pk.ni, (uint32_t)(pk.nsets + pk.nl),
                               (uint32_t)pk.nl, (uint32_t)pk.npieces, (uint32_t)(pk.n + 1 + (size_t)pk.npieces)};
    memcpy(shape8, shape, sizeof(shape));
    if (!descs.empty()) memcpy(consts, descs.data(), descs.size() * sizeof(bzh::VnConst));
    *nconsts = descs.size();
    return BZH_OK;
}

int bzh_vanishing_batch_device(bzh_ctx* ctx, bzh_pk* pk, size_t batch, const uint64_t* advice_polys, const uint64_t* instance_polys,
                               const uint64_t* lookup_polys, const uint64_t* z_polys, const uint64_t* theta, const uint64_t* beta,
                               const uint64_t* gamma, int form, int mem, const uint8_t* rng, size_t rng_stride,
                               bzh_transcript_batch* transcripts, uint64_t* out_random, uint64_t* out_random_blind, uint64_t* out_h,
                               uint64_t* out_h_blinds, uint8_t* status) {
    // what reads neither the key nor the device
    if (!ctx || !pk || !transcripts || !rng || !theta || !beta || !gamma || !out_random || !out_random_blind || !out_h || !out_h_blinds)
        return BZH_E_ARG;
    if (!batch || batch > 65535 || (form != BZH_FORM_CANONICAL && form != BZH_FORM_MONTGOMERY) || (mem != BZH_MEM_HOST && mem != BZH_MEM_DEVICE))
        return BZH_E_ARG;
    const bzh::TbInfo ti = bzh::tb_info(transcripts);
    if (!ti.ctx) return BZH_E_ARG;   // a host-resident batch
    bzh::KeyRuntime::Call in_flight(pk->rt);   // registered before the wait for ctx->mu, like every other call on a key
    // what reads the key
    const size_t n = pk->n, npieces = (size_t)pk->npieces, nz = (size_t)(pk->nsets + pk->nl);
    if (pk->device != ctx->device || ti.ctx != ctx || ti.curve != pk->curve || ti.batch != batch) return BZH_E_ARG;
    if ((pk->na && !advice_polys) || (pk->ni && !instance_polys) || (pk->nl && !lookup_polys) || (nz && !z_polys)) return BZH_E_ARG;
    // (batch * npieces: ipa_commit_blinded puts the number of commitments into grid.y, and the pieces of a batch are one launch)
    if (rng_stride < 64 * (n + 1 + npieces) || batch * npieces > 65535) return BZH_E_ARG;
    const uintptr_t all = (uintptr_t)advice_polys | (uintptr_t)instance_polys | (uintptr_t)lookup_polys | (uintptr_t)z_polys | (uintptr_t)theta |
                          (uintptr_t)beta | (uintptr_t)gamma | (uintptr_t)rng | (uintptr_t)out_random | (uintptr_t)out_random_blind |
                          (uintptr_t)out_h | (uintptr_t)out_h_blinds;
    if (mem == BZH_MEM_DEVICE && (all & 15)) return BZH_E_ARG;
    if (!pk->q_ok || pk->en % 128) return BZH_E_RANGE;   // no VM v2 program, or a domain below its workgroup: the VM v1 fold is not offered
    if (ti.proof_len + 32 * (1 + npieces) > ti.proof_cap) return BZH_E_RANGE;
    std::lock_guard<std::mutex> lk(ctx->mu);
    BZH_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int rc = bzh::with_pasta_curve(pk->curve, [&](auto c) {
        return bzh::vanishing_device_t<decltype(c)>(ctx, pk, batch, advice_polys, instance_polys, lookup_polys, z_polys, theta, beta, gamma, form,
                                                    mem, rng, rng_stride, transcripts, out_random, out_random_blind, out_h, out_h_blinds, status);
    });
    if (rc && !ctx->pending_d2h.empty()) {   // a host call that failed between its read-backs and their end: they must not land later
        (void)hipStreamSynchronize(ctx->stream);
        ctx->pending_d2h.clear();
    }
    return rc;
}

int bzh_grand_products_plan(int curve, const uint8_t* circuit, size_t circuit_len, uint32_t shape8[8]) {
    if (!circuit || !shape8) return BZH_E_ARG;
    bzh_pk pk;
    BZH_TRY(bzh::with_pasta_curve(curve, [&](auto c) {
        bzh::ParsedKey<typename bzh::CurveInfo<decltype(c)>::SF> po;
        return bzh::pk_parse_t<decltype(c)>(circuit, circuit_len, pk, po);
    }));
    const uint32_t nz = (uint32_t)(pk.nsets + pk.nl);
    const uint32_t shape[8] = {(uint32_t)pk.n, (uint32_t)pk.usable, (uint32_t)pk.bf, (uint32_t)pk.nsets, (uint32_t)pk.nl, nz, (uint32_t)pk.chunk_len,
                               nz * (uint32_t)(pk.bf + 1)};
    memcpy(shape8, shape, sizeof(shape));
    return BZH_OK;
}

int bzh_grand_products_batch_device(bzh_ctx* ctx, bzh_pk* pk, size_t batch, const uint64_t* advice, const uint64_t* instance,
                                    const uint64_t* lookup_compressed, const uint64_t* lookup_permuted, const uint64_t* beta,
                                    const uint64_t* gamma, int form, int mem, const uint8_t* rng, size_t rng_stride,
                                    bzh_transcript_batch* transcripts, uint64_t* out_z, uint64_t* out_z_polys, uint64_t* out_z_blinds,
                                    uint8_t* status) {
    // what reads neither the key nor the device
    if (!ctx || !pk || !transcripts || !rng || !beta || !gamma || !out_z_polys || !out_z_blinds) return BZH_E_ARG;
    if (!batch || batch > 65535 || (form != BZH_FORM_CANONICAL && form != BZH_FORM_MONTGOMERY) || (mem != BZH_MEM_HOST && mem != BZH_MEM_DEVICE))
        return BZH_E_ARG;
    const bzh::TbInfo ti = bzh::tb_info(transcripts);
    if (!ti.ctx) return BZH_E_ARG;   // a host-resident batch
    bzh::KeyRuntime::Call in_flight(pk->rt);   // registered before the wait for ctx->mu, like every other call on a key
    // what reads the key
    const size_t nz = (size_t)(pk->nsets + pk->nl);
    if (pk->device != ctx->device || ti.ctx != ctx || ti.curve != pk->curve || ti.batch != batch) return BZH_E_ARG;
    if ((pk->na && !advice) || (pk->ni && !instance) || (pk->nl && (!lookup_compressed || !lookup_permuted))) return BZH_E_ARG;
    // (batch * nz: ipa_commit_blinded puts the number of commitments into grid.y, and the commitments of a batch are one launch)
    if (rng_stride < 64 * nz * (size_t)(pk->bf + 1) || batch * nz > 65535) return BZH_E_ARG;
    const uintptr_t all = (uintptr_t)advice | (uintptr_t)instance | (uintptr_t)lookup_compressed | (uintptr_t)lookup_permuted | (uintptr_t)beta |
                          (uintptr_t)gamma | (uintptr_t)rng | (uintptr_t)out_z | (uintptr_t)out_z_polys | (uintptr_t)out_z_blinds;
    if (mem == BZH_MEM_DEVICE && (all & 15)) return BZH_E_ARG;
    if (!nz) return BZH_OK;   // no permutation and no lookup: nothing to write
    if (ti.proof_len + 32 * nz > ti.proof_cap) return BZH_E_RANGE;
    std::lock_guard<std::mutex> lk(ctx->mu);
    BZH_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int rc = bzh::with_pasta_curve(pk->curve, [&](auto c) {
        return bzh::products_device_t<decltype(c)>(ctx, pk, batch, advice, instance, lookup_compressed, lookup_permuted, beta, gamma, form, mem, rng,
                                                   rng_stride, transcripts, out_z, out_z_polys, out_z_blinds, status);
    });
    if (rc && !ctx->pending_d2h.empty()) {   // a host call that failed between its read-backs and their end: they must not land later
        (void)hipStreamSynchronize(ctx->stream);
        ctx->pending_d2h.clear();
    }
    return rc;
}

int bzh_commitments_plan(int curve, const uint8_t* circuit, size_t circuit_len, uint32_t shape8[8]) {
    if (!circuit || !shape8) return BZH_E_ARG;
    bzh_pk pk;
    BZH_TRY(bzh::with_pasta_curve(curve, [&](auto c) {
        bzh::ParsedKey<typename bzh::CurveInfo<decltype(c)>::SF> po;
        return bzh::pk_parse_t<decltype(c)>(circuit, circuit_len, pk, po);
    }));
    const uint32_t shape[8] = {(uint32_t)pk.n,  (uint32_t)pk.usable, (uint32_t)pk.bf, (uint32_t)pk.na, (uint32_t)pk.ni,
                               (uint32_t)pk.nl, (uint32_t)bzh::commitments_draws(pk), 32u * (uint32_t)(pk.na + 2 * pk.nl)};
    memcpy(shape8, shape, sizeof(shape));
    return BZH_OK;
}

int bzh_commitments_batch_device(bzh_ctx* ctx, bzh_pk* pk, size_t batch, const uint64_t* advice, const uint64_t* instances,
                                 size_t instance_rows, int form, int mem, const uint8_t* rng, size_t rng_stride,
                                 bzh_transcript_batch* transcripts, const bzh_commitments_out* out, uint8_t* status) {
    // what reads neither the key nor the device
    if (!ctx || !pk || !transcripts || !rng || !out || !out->theta || !out->beta || !out->gamma) return BZH_E_ARG;
    if (!batch || batch > 65535 || (form != BZH_FORM_CANONICAL && form != BZH_FORM_MONTGOMERY) || (mem != BZH_MEM_HOST && mem != BZH_MEM_DEVICE))
        return BZH_E_ARG;
    const bzh::TbInfo ti = bzh::tb_info(transcripts);
    if (!ti.ctx) return BZH_E_ARG;   // a host-resident batch
    bzh::KeyRuntime::Call in_flight(pk->rt);   // registered before the wait for ctx->mu, like every other call on a key
    // what reads the key
    const size_t na = (size_t)pk->na, ni = (size_t)pk->ni, nl = (size_t)pk->nl;
    if (pk->device != ctx->device || ti.ctx != ctx || ti.curve != pk->curve || ti.batch != batch) return BZH_E_ARG;
    // (instance_rows == 0: the instance columns are zero and `instances` is not read, NULL or not -- as in bzh_prove_batch)
    if ((na && !advice) || (ni && instance_rows && !instances) || instance_rows > pk->usable) return BZH_E_ARG;
    if ((na && (!out->advice || !out->advice_polys || !out->advice_blinds)) || (ni && (!out->instance || !out->instance_polys)) ||
        (nl && (!out->lookup_compressed || !out->lookup_permuted || !out->lookup_polys || !out->lookup_blinds)))
        return BZH_E_ARG;
    // (one row of a launch's grid per commitment, and the commitments of a kind are one launch; batch * 2 nl <= 65535 also keeps
    // the batch * nl pairs within the 32767 that one lookup_permute call takes)
    if (rng_stride < 64 * bzh::commitments_draws(*pk) || batch * std::max({na, ni, 2 * nl}) > 65535) return BZH_E_ARG;
    const uintptr_t all = (uintptr_t)advice | (uintptr_t)(instance_rows ? instances : nullptr) | (uintptr_t)rng | (uintptr_t)out->advice |
                          (uintptr_t)out->instance | (uintptr_t)out->lookup_compressed | (uintptr_t)out->lookup_permuted |
                          (uintptr_t)out->advice_polys | (uintptr_t)out->instance_polys | (uintptr_t)out->lookup_polys |
                          (uintptr_t)out->advice_blinds | (uintptr_t)out->lookup_blinds | (uintptr_t)out->theta | (uintptr_t)out->beta |
                          (uintptr_t)out->gamma;
    if (mem == BZH_MEM_DEVICE && (all & 15)) return BZH_E_ARG;
    if (ti.proof_len + 32 * (na + 2 * nl) > ti.proof_cap) return BZH_E_RANGE;
    std::lock_guard<std::mutex> lk(ctx->mu);
    BZH_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int rc = bzh::with_pasta_curve(pk->curve, [&](auto c) {
        return bzh::commitments_device_t<decltype(c)>(ctx, pk, batch, advice, instances, instance_rows, form, mem, rng, rng_stride, transcripts,
                                                      *out, status);
    });
    if (rc && !ctx->pending_d2h.empty()) {   // a host call that failed between its read-backs and their end: they must not land later
        (void)hipStreamSynchronize(ctx->stream);
        ctx->pending_d2h.clear();
    }
    return rc;
}

int bzh_prove_device_plan(int curve, const uint8_t* circuit, size_t circuit_len, uint32_t shape8[8]) {
    if (!circuit || !shape8) return BZH_E_ARG;
    bzh_pk pk;
    BZH_TRY(bzh::with_pasta_curve(curve, [&](auto c) {
        bzh::ParsedKey<typename bzh::CurveInfo<decltype(c)>::SF> po;
        return bzh::pk_parse_t<decltype(c)>(circuit, circuit_len, pk, po);
    }));
    size_t nd[4];
    bzh::prove_device_draws(pk, nd);
    const uint32_t shape[8] = {(uint32_t)nd[0], (uint32_t)nd[1], (uint32_t)nd[2], (uint32_t)nd[3], (uint32_t)(nd[0] + nd[1] + nd[2] + nd[3]),
                               (uint32_t)bzh::prove_device_proof_bytes(pk), (uint32_t)bzh::prove_device_nown(pk), (uint32_t)bzh::prove_device_max_batch(pk)};
    memcpy(shape8, shape, sizeof(shape));
    return BZH_OK;
}

// rng_stride == 0: `rng` holds batch x 32-byte seeds (bzh_prove_batch_device_seeded)
static int prove_batch_device_entry(bzh_ctx* ctx, bzh_pk* pk, size_t batch, const uint64_t* advice, int form, int mem, const uint64_t* instances,
                                    size_t instance_rows, const uint8_t* rng, size_t rng_stride, uint8_t* proofs, size_t proof_stride,
                                    size_t* proof_lens, uint8_t* status) {
    // what reads neither the key nor the device
    if (!ctx || !pk || !batch || !advice || !rng || !proofs || !proof_lens) return BZH_E_ARG;
    if ((form != BZH_FORM_CANONICAL && form != BZH_FORM_MONTGOMERY) || (mem != BZH_MEM_HOST && mem != BZH_MEM_DEVICE)) return BZH_E_ARG;
    if (mem == BZH_MEM_DEVICE && (form != BZH_FORM_MONTGOMERY || ((uintptr_t)advice & 15))) return BZH_E_ARG;
    bzh::KeyRuntime::Call in_flight(pk->rt);   // until the proofs are in the caller's buffers
    // what reads the key
    if (pk->device != ctx->device || (rng_stride != 0 && rng_stride < pk->rng_bytes) || (pk->ni && instance_rows && !instances) ||
        instance_rows > pk->usable || batch > bzh::prove_device_max_batch(*pk))
        return BZH_E_ARG;
    if (!pk->q_ok || pk->en % 128) return BZH_E_RANGE;   // no VM v2 program, or a domain below its workgroup (bzh_vanishing_batch_device)
    if (proof_stride < bzh::prove_device_proof_bytes(*pk)) return BZH_E_RANGE;
    const bzh::PdPlan* plan = nullptr;
    BZH_TRY(bzh::prove_device_plan_of(pk, &plan));
    std::lock_guard<std::mutex> lk(ctx->mu);
    BZH_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return bzh::with_pasta_curve(pk->curve, [&](auto c) {
        return bzh::prove_device_t<decltype(c)>(ctx, pk, batch, advice, form, mem, instances, instance_rows, rng, rng_stride, *plan, proofs,
                                                proof_stride, proof_lens, status);
    });
}

int bzh_prove_batch_device(bzh_ctx* ctx, bzh_pk* pk, size_t batch, const uint64_t* advice, int form, int mem, const uint64_t* instances,
                           size_t instance_rows, const uint8_t* rng, size_t rng_stride, uint8_t* proofs, size_t proof_stride,
                           size_t* proof_lens, uint8_t* status) {
    if (rng_stride == 0) return BZH_E_ARG;
    return prove_batch_device_entry(ctx, pk, batch, advice, form, mem, instances, instance_rows, rng, rng_stride, proofs, proof_stride,
                                    proof_lens, status);
}

int bzh_prove_batch_device_seeded(bzh_ctx* ctx, bzh_pk* pk, size_t batch, const uint64_t* advice, int form, int mem,
                                  const uint64_t* instances, size_t instance_rows, const uint8_t* seeds, uint8_t* proofs, size_t proof_stride,
                                  size_t* proof_lens, uint8_t* status) {
    return prove_batch_device_entry(ctx, pk, batch, advice, form, mem, instances, instance_rows, seeds, 0, proofs, proof_stride, proof_lens,
                                    status);
}

int bzh_prove_shots_device(bzh_ctx* ctx, bzh_pk* pk, const bzh_circuit* circuit, size_t batch, const uint64_t* boards, const uint64_t* trapdoors,
                           const uint64_t* shots, const uint64_t* hits, const uint8_t* seeds, uint64_t* instances, uint8_t* proofs,
                           size_t proof_stride, size_t* proof_lens, uint8_t* status) {
    return bzh::prove_game_entry("bzh_prove_shots_device", BZH_CIRCUIT_SHOT, ctx, pk, circuit, batch, boards, trapdoors, shots, hits, seeds, instances,
                                 proofs, proof_stride, proof_lens, status);
}

int bzh_prove_boards_device(bzh_ctx* ctx, bzh_pk* pk, const bzh_circuit* circuit, size_t batch, const uint64_t* ship_commitments,
                            const uint64_t* boards, const uint64_t* trapdoors, const uint8_t* seeds, uint64_t* instances, uint8_t* proofs,
                            size_t proof_stride, size_t* proof_lens, uint8_t* status) {
    return bzh::prove_game_entry("bzh_prove_boards_device", BZH_CIRCUIT_BOARD, ctx, pk, circuit, batch, ship_commitments, boards, trapdoors, nullptr,
                                 seeds, instances, proofs, proof_stride, proof_lens, status);
}

int bzh_rng_expand(const uint8_t* seed, uint64_t first_draw, size_t draws, uint8_t* out) {
    if (!seed || (!out && draws)) return BZH_E_ARG;
    uint32_t key[8], blk[16];
    memcpy(key, seed, 32);
    for (size_t i = 0; i < draws; i++) {
        bzh::chacha20_block(key, first_draw + i, blk);
        memcpy(out + i * 64, blk, 64);
    }
    return BZH_OK;
}

int bzh_accumulation_weights(int curve, const uint8_t* seed, size_t batch, uint64_t* out) {
    if (!seed || (!out && batch) || (curve != bzh::VestaCurve::id && curve != bzh::PallasCurve::id)) return BZH_E_ARG;
    return bzh::with_pasta_curve(curve, [&](auto c) {
        bzh::accumulation_weights_t<typename bzh::CurveInfo<decltype(c)>::SF>(seed, batch, BZH_FORM_CANONICAL, out);
        return BZH_OK;
    });
}

int bzh_verify_records_accumulated(bzh_ctx* ctx, const bzh_vk* vk, const bzh_bases* srs, const bzh_bases* g_lagrange, size_t batch,
                                   size_t n_inputs, const uint8_t* records, size_t record_stride, const uint64_t* g0_u_w, const uint8_t* seed,
                                   int* results, uint8_t* status, int* path) {
    if (!seed) return BZH_E_ARG;
    return verify_records_entry(ctx, vk, srs, g_lagrange, batch, n_inputs, records, record_stride, g0_u_w, seed, results, status, path);
}

int bzh_verify_batch_vk_accumulated(bzh_ctx* ctx, const bzh_vk* vk, const bzh_bases* srs, const bzh_bases* g_lagrange, size_t batch,
                                    const uint64_t* instances, size_t instance_rows, const uint8_t* proofs, size_t proof_stride,
                                    const size_t* proof_lens, const uint64_t* g0_u_w, const uint8_t* seed, int* results, int* path) {
    if (!seed) return BZH_E_ARG;
    return verify_batch_vk_entry(ctx, vk, srs, g_lagrange, BZH_VERIFY_PASS_DEVICE, batch, instances, instance_rows, proofs, proof_stride,
                                 proof_lens, g0_u_w, seed, results, path);
}

}  // extern "C"
