// Part of the whole-proof translation unit (csrc/prove.hip): the KEY -- bzh_pk, keygen's host half (blob parser, constraint-system
// shape, permutation cycles, multiopen structure, quotient program) and device half (columns, cosets, hoisted columns).
#pragma once
}  // namespace

}  // namespace bzh

// ---------------------------------------------------------------------------
// the proving key
// ---------------------------------------------------------------------------
namespace bzh {
// what bzh_prove_batch_device derives from the KeyShape when the key first needs it (csrc/prove_device.hpp): the query structure
// of the evaluations and the multiopen over the opened polynomials of a proof and the key's own.  rc: BZH_E_RANGE when those two
// leaves do not take the circuit's queries
struct PdPlan {
    bool ready = false;
    int rc = 0;
    EvPlan ev;
    MoPlan mo;
};
}  // namespace bzh

// (the constraint system's shape, the multiopen structure and the vk commitments -- what the verifier reads -- are the KeyShape)
struct bzh_pk : bzh::KeyShape {
    int device = 0;
    size_t en = 0, ext = 0;
    const bzh_bases* srs = nullptr;
    std::vector<uint64_t> srs_g0_u_w;           // G_0, U, W of `srs`, canonical affine, read back once (bzh_verify_batch checks its argument against these)
    const bzh_bases* srs_lagrange = nullptr;   // (g_lagrange | u | w): Params::commit_lagrange for the columns upstream commits in that basis
    uint64_t eomega[4], zeta[4];  // Montgomery limbs for ntt_run
    // device, one allocation
    void* dev = nullptr;
    size_t dev_bytes = 0, hoist_bytes = 0, key29_bytes = 0;   // sizes of dev / hoist / key29 (bzh_pk_device_bytes)
    uint32_t *fixed = nullptr, *fixed_polys = nullptr, *fixed_cosets = nullptr, *sigma = nullptr, *ident = nullptr, *sigma_polys = nullptr,
             *sigma_cosets = nullptr, *l0 = nullptr, *l_last = nullptr, *l_blind = nullptr, *x_col = nullptr, *tinv_col = nullptr;
    std::map<uint64_t, bzh::Program> progs;
    // The quotient's VM v2 program: compiled on the host at bzh_pk_create (it depends on the circuit only, not on k or on
    // any witness); q_ok = false when the circuit does not fit VM v2 (the prover then folds through VM v1).
    bzh::Program2 qprog;
    bool q_ok = false;
    uint64_t q_hash = 0;
    // proof-independent subexpressions of the quotient (selector products ...): one VM v1 program each, evaluated once on the
    // extended coset into `hoist` at bzh_pk_create
    std::vector<bzh::Program> hoist_progs;
    uint32_t* hoist = nullptr;
    size_t hoist_cols = 0;
    // The same program as compiled code, launched instead of the interpreter:
    //   q_builtin: a kernel generated at build time and linked into libbzh2.so (the reference's two circuits), found by q_hash;
    //   q_module / q_fn: a code object the caller compiled from bzh_pk_quotient_source (any other circuit).
    // q_select: BZH_QUOTIENT_* -- which of the three runs.
    bzh_quotient_launch_fn q_builtin = nullptr;
    // the builtin kernel's unsaturated-limb flavour (csrc/fe29.cuh) and the key-owned columns it reads as fe29 planes, converted
    // once at bzh_pk_create (Key29Layout)
    bzh_quotient_launch_fn q_builtin29 = nullptr;
    uint32_t* key29 = nullptr;
    hipModule_t q_module = nullptr;
    hipFunction_t q_fn = nullptr;
    int q_select = BZH_QUOTIENT_INTERPRETER;
    int ws_select = BZH_WORKSPACE_EXTENDED;   // BZH_WORKSPACE_*: where the quotient reads the per-proof columns (bzh_pk_workspace_select)
    int lk_select = BZH_LOOKUP_DEVICE;   // BZH_LOOKUP_*: where the lookup argument's columns are permuted (bzh_pk_lookup_select)
    bool lk_chosen = false;   // bzh_pk_lookup_select was called: lk_select holds for every batch size (else see kLookupDeviceMinBatch, prover.hpp)
    int vpass_select = BZH_VERIFY_PASS_HOST;  // BZH_VERIFY_PASS_*: where bzh_verify_batch runs the per-proof pass (bzh_pk_verify_pass_select)
    int vp_select = BZH_VERIFY_POINTS_HOST;   // BZH_VERIFY_POINTS_*: where bzh_verify_batch decompresses the proofs' points (bzh_pk_verify_select)
    size_t rng_bytes = 0;
    bzh::PdPlan pd_plan;   // guarded by rt.mu until `ready`, read-only after
    // verifying key: the KeyShape's commitments to the fixed and permutation polynomials are computed at the first verification
    bool vk_ready = false;
    // the constraint-system part of the blob the key was made from, as bzh_vk keeps it (csrc/verifying_key.hpp)
    std::vector<uint8_t> cs_bytes;
    // The key is immutable after bzh_pk_create except for caches filled on first use (programs, hoisted columns, the vk
    // commitments, G_0/U/W, the quotient module) and the runtime state: `rt.mu` guards those in short sections.  Calls through
    // different ctxs run concurrently on one key; a call holds its ctx's mutex throughout (lock order: ctx->mu, then pk->rt.mu).
    // rt: the per-(key, ctx) workspaces and the count of running calls -- bzh_pk_set_quotient_module and bzh_pk_free refuse while
    // it is non-zero: they unload code / free arenas that a call on ANOTHER ctx may be launching from.
    bzh::KeyRuntime rt;
};

namespace bzh {
namespace {

// column registry of one batched evaluation: (device pointer, elements between consecutive proofs; 0 = shared)
struct Cols {
    std::vector<const uint32_t*> ptr;
    std::vector<size_t> stride;
    std::map<uint64_t, int> index;
    int add(uint64_t key, const uint32_t* p, size_t s) {
        auto it = index.find(key);
        if (it != index.end()) return it->second;
        const int i = (int)ptr.size();
        index[key] = i;
        ptr.push_back(p);
        stride.push_back(s);
        return i;
    }
    int at(uint64_t key) const { return index.at(key); }
};

// circuit expression -> evaluator expression over `reg` (columns looked up by (kind, index))
static int lower(const bzh_pk& pk, int i, EPool& ep, const Cols& reg, int rot_scale) {
    const CNode& e = pk.cx[i];
    switch (e.tag) {
        case CX_CONST: {
            ENode nd;
            nd.tag = EX_CONST;
            memcpy(nd.val, e.val, 32);
            return ep.push(nd);
        }
        case CX_ADVICE: return ep.query(reg.at(key(K_ADV, e.col)), e.rot * rot_scale);
        case CX_FIXED: return ep.query(reg.at(key(K_FIX, e.col)), e.rot * rot_scale);
        case CX_INSTANCE: return ep.query(reg.at(key(K_INST, e.col)), e.rot * rot_scale);
        case CX_NEG: return ep.neg(lower(pk, e.a, ep, reg, rot_scale));
        case CX_SCALE: {
            ENode nd;
            nd.tag = EX_SCALE;
            nd.a = lower(pk, e.a, ep, reg, rot_scale);
            memcpy(nd.val, e.val, 32);
            return ep.push(nd);
        }
        case CX_ADD: {
            const int a = lower(pk, e.a, ep, reg, rot_scale), b = lower(pk, e.b, ep, reg, rot_scale);
            return ep.add(a, b);
        }
        default: {
            const int a = lower(pk, e.a, ep, reg, rot_scale), b = lower(pk, e.b, ep, reg, rot_scale);
            return ep.mul(a, b);
        }
    }
}

// ---------------------------------------------------------------------------
// keygen
// ---------------------------------------------------------------------------
// ---------------------------------------------------------------------------
// the quotient program of a key (host): column registry, terms in protocol order, compilation, hoisted columns
// ---------------------------------------------------------------------------
// per-proof columns of one prove call; all null when only the program is wanted (compile_quotient, materialize_hoist)
struct QuotientPtrs {
    const uint32_t* adv = nullptr;    // na columns of en elements per proof
    const uint32_t* inst = nullptr;   // ni
    const uint32_t* z = nullptr;      // nsets + nl grand products
    std::vector<const uint32_t*> lk;  // per lookup: A' | S'
    size_t lk_cols = 2;               // columns between consecutive proofs of one lookup's pair (2: a buffer per lookup)
};
// The key's columns as fe29 planes (pk.key29), where each block begins, in columns of 9 en words:
// fixed cosets | sigma cosets | l0, l_last, l_blind, X, 1/(X^n - 1) | hoisted columns
struct Key29Layout {
    size_t fixed, sigma, misc, hoist, end;
    explicit Key29Layout(const bzh_pk& pk)
        : fixed(0), sigma((size_t)pk.nf), misc(sigma + pk.perm_columns.size()), hoist(misc + 5), end(hoist + pk.hoist_cols) {}
};
// The registry fixes the column INDEX every instruction of the compiled program refers to: it must be built by this one
// function, for the compile, the hoisted columns' evaluation and every launch.  The per-proof columns and the key's are
//   saturated elements (planes = false): 8 words an element, stride = ELEMENTS between consecutive proofs, the key's own columns; or
//   fe29 planes (planes = true): 9 en words a column, stride = WORDS between consecutive proofs, the key's columns out of pk.key29;
// stride 0 = shared (key-owned).  The hoisted columns come last.  Cols::add keeps what it has: compile_quotient calls this a
// second time, once it knows how many hoisted columns there are.
// proof_elems (saturated elements only): the elements of ONE per-proof column when that is not en -- n, for the coset-wise
// workspace, whose per-proof columns hold one coset of n points at a time (workspace_items below); the key's stay at en.
static void quotient_registry(const bzh_pk& pk, const QuotientPtrs& q, bool planes, Cols& reg, size_t proof_elems = 0) {
    const size_t en = pk.en, pe = proof_elems && !planes ? proof_elems : en, m = pk.perm_columns.size(), w = planes ? 9 : 8,
                 su = planes ? 9 * en : pe;
    const int na = pk.na, nf = pk.nf, ni = pk.ni, nsets = pk.nsets, nl = pk.nl, nz = pk.nsets + pk.nl;
    auto at = [&](const uint32_t* base, size_t elems) -> const uint32_t* { return base ? base + elems * w : nullptr; };
    const Key29Layout k29(pk);
    // (l0, l_last, l_blind, X, 1/(X^n - 1) are consecutive columns of the key's allocation too)
    const uint32_t* k_fixed = planes ? at(pk.key29, k29.fixed * en) : pk.fixed_cosets;
    const uint32_t* k_sigma = planes ? at(pk.key29, k29.sigma * en) : pk.sigma_cosets;
    const uint32_t* k_misc = planes ? at(pk.key29, k29.misc * en) : pk.l0;
    const uint32_t* k_hoist = planes ? at(pk.key29, k29.hoist * en) : pk.hoist;
    for (int i = 0; i < na; i++) reg.add(key(K_ADV, i), at(q.adv, (size_t)i * pe), (size_t)na * su);
    for (int i = 0; i < nf; i++) reg.add(key(K_FIX, i), at(k_fixed, (size_t)i * en), 0);
    for (int i = 0; i < ni; i++) reg.add(key(K_INST, i), at(q.inst, (size_t)i * pe), (size_t)ni * su);
    for (size_t j = 0; j < m; j++) reg.add(key(K_SIGMA, j), at(k_sigma, j * en), 0);
    for (int i = 0; i < nsets; i++) reg.add(key(K_PZ, i), at(q.z, (size_t)i * pe), (size_t)nz * su);
    for (int i = 0; i < nl; i++) {
        const uint32_t* c = (size_t)i < q.lk.size() ? q.lk[i] : nullptr;
        reg.add(key(K_LA, i), c, q.lk_cols * su);
        reg.add(key(K_LS, i), at(c, pe), q.lk_cols * su);
        reg.add(key(K_LZ, i), at(q.z, (size_t)(nsets + i) * pe), (size_t)nz * su);
    }
    static const int misc[5] = {M_L0, M_LLAST, M_LBLIND, M_X, M_TINV};
    for (size_t i = 0; i < 5; i++) reg.add(key(K_MISC, misc[i]), at(k_misc, i * en), 0);
    for (size_t hi = 0; hi < pk.hoist_cols; hi++) reg.add(key(K_HOIST, hi), at(k_hoist, hi * en), 0);
}

// What one prove call of `batch` proofs takes from its arena, by item (bzh_workspace_plan; host only).  The `cosets` items are
// the buffers the quotient reads the per-proof columns from -- every one on the whole extended coset (BZH_WORKSPACE_EXTENDED:
// en elements a column, what Prover::ext_alloc hands out in saturated limbs) or on one coset of n points at a time
// (BZH_WORKSPACE_COSETWISE: n elements a column; Prover::cosetwise_setup carves exactly these four sizes).  The other items
// count the call's column-sized buffers as the phases of prover.hpp allocate them: per-proof columns over the domain and as
// coefficients with the grand products' factors (witness), h (quotient), and the largest stretch of the phases after it
// (tail: random polynomial and its draws, the pieces, then the evaluation gather or the multiopen's buffers with the opening's
// draws).  What the launches stage besides (programs, constants, blinds, status words) is covered by an allowance, staging:
// 1 MiB + 64 KiB a proof.  tests/test_gpu_workspace_cosetwise.py holds the total against the arena's high-water mark.
struct WorkspaceItems {
    size_t column_bytes = 0;                                    // one per-proof column where the quotient reads it
    size_t adv_bytes = 0, inst_bytes = 0, z_bytes = 0, lk_bytes = 0;   // the four coset buffers of the batch
    size_t cosets_bytes = 0, cosets_extended_bytes = 0;         // their sum in this mode | in BZH_WORKSPACE_EXTENDED
    size_t witness_bytes = 0, quotient_bytes = 0, tail_bytes = 0, staging_bytes = 0, total_bytes = 0;
};
static WorkspaceItems workspace_items(const bzh_pk& pk, size_t batch, int mode) {
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };   // Arena::alloc's rounding
    const size_t B = batch, n = pk.n, en = pk.en, na = (size_t)pk.na, ni = (size_t)std::max(pk.ni, 1), nl = (size_t)pk.nl,
                 nz = (size_t)std::max(pk.nsets + pk.nl, 1), npieces = (size_t)pk.npieces, m = pk.perm_columns.size(),
                 nq = pk.rot_sets.size(), col = n * 32;
    WorkspaceItems w;
    auto cosets = [&](size_t elems, size_t* sum) {
        const size_t a = al(B * std::max<size_t>(na, 1) * elems * 32), i = al(B * ni * elems * 32), z = al(B * nz * elems * 32), l = nl * al(B * 2 * elems * 32);
        *sum = a + i + z + l;
        if (elems == (mode == BZH_WORKSPACE_COSETWISE ? n : en)) w.adv_bytes = a, w.inst_bytes = i, w.z_bytes = z, w.lk_bytes = l;
    };
    cosets(en, &w.cosets_extended_bytes);
    if (mode == BZH_WORKSPACE_COSETWISE) cosets(n, &w.cosets_bytes);
    else w.cosets_bytes = w.cosets_extended_bytes;
    w.column_bytes = (mode == BZH_WORKSPACE_COSETWISE ? n : en) * 32;
    // (per lookup: compressed input and table, the permuted pair, its coefficients -- and the two canonical copies the host
    // permutation sorts from, Prover::permute_on_host, counted for every batch though batches of 8 and more permute on the device)
    w.witness_bytes = B * col * (2 * ni + 2 * na + 8 * nl + 4 * nz);
    w.quotient_bytes = al(B * en * 32);
    size_t J = pk.instance_queries.size() + pk.advice_queries.size() + pk.fixed_queries.size() + 1 + m + 5 * nl, J2 = 0;
    if (pk.nsets) J += 3 * (size_t)pk.nsets - 1;
    for (auto& rs : pk.rot_sets) J2 += rs.size();
    const size_t ipa_draws = al(B * 64 * (n + 1 + 2 * (size_t)pk.k));
    const size_t multiopen = std::max(B * col * (3 + nq + J2), B * col * (5 + 5 * nq) + ipa_draws);
    w.tail_bytes = B * col * (3 + npieces) + std::max(B * col * J, multiopen);
    // an allowance, not a count: programs and their constant tables, blinding draws, blinds, status words, point tables
    w.staging_bytes = ((size_t)1 << 20) + B * ((size_t)64 << 10);
    w.total_bytes = w.witness_bytes + w.cosets_bytes + w.quotient_bytes + w.tail_bytes + w.staging_bytes;
    return w;
}

// every term of the quotient's numerator in protocol order (gates, permutation argument, lookups); *tinv = the 1 / (X^n - 1) column
template <class SF>
static std::vector<int> quotient_terms(const bzh_pk& pk, const Cols& reg, EPool& ep, int* tinv) {
    const int e = (int)pk.ext, nsets = pk.nsets, nl = pk.nl, last_rot = -(pk.bf + 1);
    const size_t m = pk.perm_columns.size();
    auto Q = [&](uint64_t kk, int rot = 0) { return ep.query(reg.at(kk), rot); };
    auto col_q = [&](std::pair<int, int> col) {
        return Q(key(col.first == CX_ADVICE ? K_ADV : (col.first == CX_FIXED ? K_FIX : K_INST), col.second));
    };
    const Fe<SF> onef = fe_one<SF>();
    auto one = [&] { return ep.cnst(onef); };
    auto l0 = [&] { return Q(key(K_MISC, M_L0)); };
    auto l_last = [&] { return Q(key(K_MISC, M_LLAST)); };
    auto active = [&] { return ep.sub(one(), ep.add(l_last(), Q(key(K_MISC, M_LBLIND)))); };
    std::vector<int> terms;
    for (int g : pk.gates) terms.push_back(lower(pk, g, ep, reg, e));
    if (nsets) {
        terms.push_back(ep.mul(l0(), ep.sub(one(), Q(key(K_PZ, 0)))));
        const uint64_t zl = key(K_PZ, nsets - 1);
        terms.push_back(ep.mul(l_last(), ep.sub(ep.mul(Q(zl), Q(zl)), Q(zl))));
        for (int i = 1; i < nsets; i++) terms.push_back(ep.mul(l0(), ep.sub(Q(key(K_PZ, i)), Q(key(K_PZ, i - 1), last_rot * e))));
        for (int i = 0; i < nsets; i++) {
            const size_t c0 = (size_t)i * pk.chunk_len, c1 = std::min(m, c0 + pk.chunk_len);
            int left = Q(key(K_PZ, i), e), right = Q(key(K_PZ, i));
            for (size_t gj = c0; gj < c1; gj++) {
                left = ep.mul(left, ep.add(ep.add(col_q(pk.perm_columns[gj]), ep.mul(ep.sym(SY_BETA), Q(key(K_SIGMA, gj)))), ep.sym(SY_GAMMA)));
                const int cur = ep.mul(ep.sym(SY_BD0 + (int)gj), Q(key(K_MISC, M_X)));
                right = ep.mul(right, ep.add(ep.add(col_q(pk.perm_columns[gj]), cur), ep.sym(SY_GAMMA)));
            }
            terms.push_back(ep.mul(active(), ep.sub(left, right)));
        }
    }
    for (int i = 0; i < nl; i++) {
        auto z0 = [&] { return Q(key(K_LZ, i)); };
        auto a_p = [&] { return Q(key(K_LA, i)); };
        auto s_p = [&] { return Q(key(K_LS, i)); };
        auto comp = [&](const std::vector<int>& es) {
            std::vector<int> t;
            for (int x : es) t.push_back(lower(pk, x, ep, reg, e));
            return ep.horner(t, ep.sym(SY_THETA));
        };
        terms.push_back(ep.mul(l0(), ep.sub(one(), z0())));
        terms.push_back(ep.mul(l_last(), ep.sub(ep.mul(z0(), z0()), z0())));
        const int lhs = ep.mul(ep.mul(Q(key(K_LZ, i), e), ep.add(a_p(), ep.sym(SY_BETA))), ep.add(s_p(), ep.sym(SY_GAMMA)));
        const int rhs = ep.mul(ep.mul(z0(), ep.add(comp(pk.lookups[i].first), ep.sym(SY_BETA))),
                               ep.add(comp(pk.lookups[i].second), ep.sym(SY_GAMMA)));
        terms.push_back(ep.mul(active(), ep.sub(lhs, rhs)));
        terms.push_back(ep.mul(l0(), ep.sub(a_p(), s_p())));
        terms.push_back(ep.mul(ep.mul(active(), ep.sub(a_p(), s_p())), ep.sub(a_p(), Q(key(K_LA, i), -e))));
    }
    *tinv = Q(key(K_MISC, M_TINV));
    return terms;
}

// Compile the quotient for VM v2 (host only).  Hoisting: maximal subexpressions over proof-independent columns (stride 0:
// fixed / permutation / Lagrange columns of the key) and literal constants that contain a multiplication -- the
// compressed-selector products q prod (j - q) of every gate -- get one VM v1 program each (pk.hoist_progs) and are referred
// to by the main program as extra registry columns; materialize_hoist evaluates them once on the extended coset.
template <class SF>
static void compile_quotient(bzh_pk& pk) {
    pk.q_ok = false;
    pk.hoist_progs.clear();
    pk.hoist_cols = 0;
    if (pk.en % 128) return;   // VM v2 runs whole 128-row workgroups (tiny test domains take the plain fold)
    Cols reg;
    quotient_registry(pk, QuotientPtrs{}, false, reg);
    EPool ep;
    int tinv = -1;
    const std::vector<int> terms = quotient_terms<SF>(pk, reg, ep, &tinv);
    Compiler2 cc(ep);
    if (!getenv("BZH_NO_HOIST")) {
        const size_t nn = ep.n.size();
        std::vector<char> indep(nn, 0);
        std::vector<int> muls(nn, 0);
        for (size_t i = 0; i < nn; i++) {   // children precede parents in the pool
            const ENode& e = ep.n[i];
            if (e.tag == EX_CONST) indep[i] = 1;
            else if (e.tag == EX_SYMBOL) indep[i] = 0;
            else if (e.tag == EX_QUERY) indep[i] = reg.stride[e.col] == 0;
            else if (e.tag == EX_NEG) indep[i] = indep[e.a], muls[i] = muls[e.a];
            else if (e.tag == EX_SCALE) indep[i] = indep[e.a], muls[i] = muls[e.a] + 1;
            else indep[i] = indep[e.a] && indep[e.b], muls[i] = muls[e.a] + muls[e.b] + (e.tag == EX_MUL);
        }
        std::vector<int> picked;
        std::vector<char> seen(nn, 0);
        std::vector<int> stack(terms.begin(), terms.end());
        while (!stack.empty()) {
            const int i = stack.back();
            stack.pop_back();
            if (seen[i]) continue;
            seen[i] = 1;
            const ENode& e = ep.n[i];
            if (e.tag == EX_CONST || e.tag == EX_SYMBOL || e.tag == EX_QUERY) continue;
            if (indep[i] && muls[i] >= 1) {
                picked.push_back(i);
                continue;
            }
            if (e.a >= 0) stack.push_back(e.a);
            if (e.b >= 0) stack.push_back(e.b);
        }
        std::sort(picked.begin(), picked.end());
        if (!picked.empty() && picked.size() <= 512) {
            pk.hoist_cols = picked.size();
            quotient_registry(pk, QuotientPtrs{}, false, reg);   // ... and the hoisted columns
            for (size_t hi = 0; hi < picked.size(); hi++) {
                Compiler c1(ep);
                c1.prog.result_slot = c1.emit(picked[hi]);
                if (c1.overflow) {
                    pk.hoist_progs.clear();
                    pk.hoist_cols = 0;
                    return;   // does not fit the evaluators' slot file: the prover folds through VM v1
                }
                pk.hoist_progs.push_back(std::move(c1.prog));
                cc.hoisted[picked[hi]] = reg.at(key(K_HOIST, hi));
            }
        }
    }
    cc.quotient(terms, tinv);
    cc.prog.nlds = cc.nlds();
    if (getenv("BZH_PROVE_TRACE")) {
        const size_t muls = program2_muls(cc.prog);
        fprintf(stderr, "[bzh_pk_create] quotient program (VM v2): %zu terms, %zu ops, %zu multiplications, %d LDS slots, %zu constants, %zu hoisted columns%s\n",
                terms.size(), cc.prog.ops.size(), muls, cc.prog.nlds, cc.prog.consts.size(), pk.hoist_progs.size(), cc.prog.ok ? "" : " -- NOT usable");
        // instruction mix: form (SS/SL/LL/UN) x operation, and the kinds of the memory operands
        size_t hist[4][4] = {{0}}, kinds[4] = {0};
        for (auto& o : cc.prog.ops) {
            hist[o.form()][o.op()]++;
            if (o.reads_b()) kinds[o.b_kind & 3]++;
            if (o.reads_a() || o.is_store()) kinds[o.a_kind & 3]++;   // (the slot a STORE writes counts as an operand here)
        }
        fprintf(stderr, "[bzh_pk_create]   mix  SS add/sub/mul/rsub %zu/%zu/%zu/%zu  SL %zu/%zu/%zu/%zu  LL %zu/%zu/%zu/%zu  UN neg/load/store %zu/%zu/%zu ; operands column/const/lds %zu/%zu/%zu\n",
                hist[0][0], hist[0][1], hist[0][2], hist[0][3], hist[1][0], hist[1][1], hist[1][2], hist[1][3], hist[2][0], hist[2][1],
                hist[2][2], hist[2][3], hist[3][0], hist[3][1], hist[3][2], kinds[BZH_EXPR_COLUMN], kinds[BZH_EXPR_CONST], kinds[BZH_EXPR_LDS]);
    }
    pk.qprog = std::move(cc.prog);
    pk.q_ok = pk.qprog.ok;
    pk.q_hash = program2_hash(pk.qprog, pk.field);
    pk.hoist_cols = pk.hoist_progs.size();
    if (!pk.q_ok) {
        pk.hoist_progs.clear();
        pk.hoist_cols = 0;
    }
}

// evaluate the hoisted columns on the extended coset (device; once per key, at bzh_pk_create)
template <class SF>
static int materialize_hoist(bzh_ctx* ctx, bzh_pk& pk) {
    if (!pk.q_ok || pk.hoist_progs.empty()) return BZH_OK;
    const size_t size = pk.en;
    BZH_HIP_TRY(ctx, hipMalloc((void**)&pk.hoist, pk.hoist_cols * size * 32));
    pk.hoist_bytes = pk.hoist_cols * size * 32;
    Cols reg;
    quotient_registry(pk, QuotientPtrs{}, false, reg);   // hoisted programs read key-owned columns only
    const size_t ncols = reg.ptr.size();
    size_t stage_bytes = 0;
    for (const Program& pg : pk.hoist_progs)
        stage_bytes = std::max(stage_bytes, std::max<size_t>(pg.consts.size(), 1) * 32 + pg.ops.size() * sizeof(bzh_expr_op) + ncols * 16 + 1024);
    char* stage_all = nullptr;
    BZH_HIP_TRY(ctx, hipMalloc((void**)&stage_all, stage_bytes * pk.hoist_progs.size()));
    int rc = BZH_OK;
    for (size_t hi = 0; hi < pk.hoist_progs.size() && !rc; hi++) {
        const Program& pg = pk.hoist_progs[hi];
        std::vector<uint32_t> cv(std::max<size_t>(pg.consts.size(), 1) * 8);
        for (size_t i = 0; i < pg.consts.size(); i++) memcpy(&cv[i * 8], pg.consts[i].val, 32);
        char* stage = stage_all + hi * stage_bytes;
        uint32_t* d_consts = (uint32_t*)stage;
        char* d_prog = stage + ((cv.size() * 4 + 255) & ~(size_t)255);
        char* d_ptrs = d_prog + ((pg.ops.size() * sizeof(bzh_expr_op) + 255) & ~(size_t)255);
        char* d_strides = d_ptrs + ((ncols * 8 + 255) & ~(size_t)255);
        if ((rc = h2d_small(ctx, d_consts, cv.data(), cv.size() * 4))) break;
        if ((rc = h2d_small(ctx, d_prog, pg.ops.data(), pg.ops.size() * sizeof(bzh_expr_op)))) break;
        if ((rc = h2d_small(ctx, d_ptrs, reg.ptr.data(), ncols * 8))) break;
        if ((rc = h2d_small(ctx, d_strides, reg.stride.data(), ncols * 8))) break;
        int nslots = pg.result_slot + 1;
        for (auto& o : pg.ops) nslots = std::max(nslots, (int)o.dst + 1);
        rc = expr_eval(ctx, pk.field, d_prog, (int)pg.ops.size(), (const uint32_t* const*)d_ptrs, (const size_t*)d_strides, d_consts, 0, size,
                       pg.result_slot, 1, nslots, pk.hoist + hi * size * 8);
    }
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipFree(stage_all);
    return rc;
}

// what the host half of keygen hands to the device half
template <class SF>
struct ParsedKey {
    std::vector<Fe<SF>> fixed_h;                 // nf x n fixed assignment, Montgomery
    std::vector<uint32_t> map_c, map_r;          // permutation: (column, row) -> (column, row)
    Fe<SF> omega, eomega, delta, zeta;
};

// The constraint-system part of a circuit blob as a blob of its own: everything up to the copy constraints, no copy
// constraints, `nf` empty fixed columns, then the query lists -- a valid circuit blob with the same shape (csrc/verifying_key.hpp).
static std::vector<uint8_t> constraint_system_bytes(const uint8_t* blob, size_t head_end, size_t tail_begin, size_t tail_end, int nf) {
    std::vector<uint8_t> cs(blob, blob + head_end);
    cs.resize(cs.size() + 4 + 4 * (size_t)nf, 0);   // u32 ncopies = 0, nf x u32 len = 0
    cs.insert(cs.end(), blob + tail_begin, blob + tail_end);
    return cs;
}

// keygen, host half: parse the circuit blob, derive the constraint-system shape (queries, degree, blinding factors,
// extended domain), the permutation cycles and the multiopen structure, and compile the quotient program (with_quotient; keygen_vk
// does without).  No device work: this is also what the build-time kernel generator runs (bzh_quotient_source_for_circuit).
template <class C>
static int pk_parse_t(const uint8_t* blob, size_t len, bzh_pk& pk, ParsedKey<typename CurveInfo<C>::SF>& po, bool with_quotient = true) {
    using SF = typename CurveInfo<C>::SF;
    using FM = FieldInfo<SF>;
    Reader r{blob, blob + len};
    ShapeHead head;
    BZH_TRY(shape_parse_head<C>(r, pk, head));
    const size_t head_end = (size_t)(r.p - blob);
    const uint32_t nperm = head.nperm;
    const uint32_t ncopies = r.u32();
    struct Copy {
        uint32_t lc, lr, rc, rr;
    };
    std::vector<Copy> copies;
    for (uint32_t i = 0; i < ncopies && r.ok; i++) {
        Copy c{r.u32(), r.u32(), r.u32(), r.u32()};
        if (c.lc >= nperm || c.rc >= nperm || c.lr >= pk.n || c.rr >= pk.n) return BZH_E_ARG;
        copies.push_back(c);
    }
    if (!r.ok) return BZH_E_ARG;
    const size_t n = pk.n;
    std::vector<Fe<SF>>& fixed_h = po.fixed_h;
    fixed_h.assign((size_t)pk.nf * n, fe_zero<SF>());
    for (int f = 0; f < pk.nf; f++) {
        const uint32_t fl = r.u32();
        if (!r.ok || fl > n) return BZH_E_ARG;
        const uint8_t* b = r.bytes((size_t)fl * 32);
        if (!b) return BZH_E_ARG;
        for (uint32_t i = 0; i < fl; i++) fixed_h[(size_t)f * n + i] = h_from_bytes<SF>(b + 32 * (size_t)i);
    }
    if (!r.ok) return BZH_E_ARG;
    const size_t tail_begin = (size_t)(r.p - blob);
    BZH_TRY(shape_parse_tail<C>(r, pk, head));
    pk.cs_bytes = constraint_system_bytes(blob, head_end, tail_begin, (size_t)(r.p - blob), pk.nf);
    pk.en = (size_t)1 << pk.ek;
    pk.ext = pk.en / n;

    // domain constants
    const Fe<SF> gen = fe_from_u32<SF>(FM::gen);
    const Fe<SF> root = h_root_of_unity<SF>();
    const Fe<SF> omega = h_omega(root, pk.k), eomega = h_omega(root, pk.ek);
    Fe<SF> delta;
    memcpy(delta.l, pk.delta, 32);
    Fe<SF> zeta;
    {  // g^((p-1)/3)
        uint32_t q[8];
        uint64_t rem = 0;
        uint32_t pm1[8];
        for (int i = 0; i < 8; i++) pm1[i] = SF::mod(i);
        pm1[0] -= 1;
        for (int i = 7; i >= 0; i--) {
            const uint64_t cur = (rem << 32) | pm1[i];
            q[i] = (uint32_t)(cur / 3);
            rem = cur % 3;
        }
        if (rem) return BZH_E_RANGE;  // no cube root of unity: the coset fast path needs 3 | p - 1
        zeta = fe_pow(gen, q);
    }
    fe_to_u64<SF>(pk.eomega, eomega);
    fe_to_u64<SF>(pk.zeta, zeta);
    po.omega = omega, po.eomega = eomega, po.delta = delta, po.zeta = zeta;

    // permutation cycles (upstream permutation::keygen::Assembly::copy)
    const size_t m = nperm;
    std::vector<uint32_t>& map_c = po.map_c;
    std::vector<uint32_t>& map_r = po.map_r;
    map_c.resize(m * n), map_r.resize(m * n);
    std::vector<uint32_t> aux_c(m * n), aux_r(m * n), sizes(m * n, 1);
    for (size_t c = 0; c < m; c++)
        for (size_t rr = 0; rr < n; rr++) {
            map_c[c * n + rr] = aux_c[c * n + rr] = (uint32_t)c;
            map_r[c * n + rr] = aux_r[c * n + rr] = (uint32_t)rr;
        }
    for (auto& cp : copies) {
        size_t li = cp.lc * n + cp.lr, ri = cp.rc * n + cp.rr;
        uint32_t lc = aux_c[li], lr = aux_r[li], rc = aux_c[ri], rr = aux_r[ri];
        if (lc == rc && lr == rr) continue;
        if (sizes[lc * n + lr] < sizes[rc * n + rr]) {
            std::swap(lc, rc);
            std::swap(lr, rr);
        }
        sizes[lc * n + lr] += sizes[rc * n + rr];
        uint32_t ic = rc, ir = rr;
        do {
            const size_t ii = ic * n + ir;
            aux_c[ii] = lc;
            aux_r[ii] = lr;
            const uint32_t nc = map_c[ii], nr = map_r[ii];
            ic = nc;
            ir = nr;
        } while (!(ic == rc && ir == rr));
        std::swap(map_c[li], map_c[ri]);
        std::swap(map_r[li], map_r[ri]);
    }

    // randomness per proof: blinding rows and blinds in create_proof's draw order, then the IPA opening
    {
        const size_t bf1 = (size_t)pk.bf + 1;
        size_t draws = (size_t)pk.na * bf1 + pk.na;
        draws += (size_t)pk.nl * (2 * bf1 + 2);
        draws += (size_t)(pk.nsets + pk.nl) * ((size_t)pk.bf + 1);
        draws += n + 1;                 // random polynomial + its blind
        draws += (size_t)pk.npieces;    // h pieces
        draws += 1;                     // f blind
        draws += n + 1 + 2 * (size_t)pk.k;
        pk.rng_bytes = draws * 64;
    }
    if (with_quotient) compile_quotient<SF>(pk);
    return BZH_OK;
}

// keygen, device half: fixed / permutation / identity polynomials in Lagrange, coefficient and extended-coset form,
// l_0 / l_last / l_blind, X and 1 / (X^n - 1) on the extended coset, the hoisted columns of the quotient program.
template <class C>
static int pk_create_t(bzh_ctx* ctx, const bzh_bases* srs, const uint8_t* blob, size_t len, bzh_pk** out) {
    using SF = typename CurveInfo<C>::SF;
    std::unique_ptr<bzh_pk> pkp(new bzh_pk());
    bzh_pk& pk = *pkp;
    ParsedKey<SF> po;
    BZH_TRY(pk_parse_t<C>(blob, len, pk, po));
    pk.device = ctx->device;
    pk.srs = srs;
    if (srs->n != pk.n + 2 || srs->curve != C::id) return BZH_E_ARG;
    const size_t n = pk.n, m = pk.perm_columns.size();
    const std::vector<Fe<SF>>& fixed_h = po.fixed_h;
    const std::vector<uint32_t>&map_c = po.map_c, &map_r = po.map_r;
    const Fe<SF> omega = po.omega, eomega = po.eomega, delta = po.delta, zeta = po.zeta;
    // device allocation: fixed / sigma / ident columns in the three forms, l0 / l_last / l_blind, X and 1/(X^n - 1)
    const size_t en = pk.en, nf = pk.nf;
    const size_t words = (2 * nf * n + nf * en + 3 * m * n + m * en + 3 * en + 2 * en + 3 * n) * 8;
    BZH_HIP_TRY(ctx, hipMalloc(&pk.dev, words * 4 + 256));
    pk.dev_bytes = words * 4 + 256;
    uint32_t* cur = (uint32_t*)pk.dev;
    auto take = [&](size_t elems) {
        uint32_t* p = cur;
        cur += elems * 8;
        return p;
    };
    pk.fixed = take(nf * n);
    pk.fixed_polys = take(nf * n);
    pk.fixed_cosets = take(nf * en);
    pk.sigma = take(m * n);
    pk.ident = take(m * n);
    pk.sigma_polys = take(m * n);
    pk.sigma_cosets = take(m * en);
    pk.l0 = take(en);
    pk.l_last = take(en);
    pk.l_blind = take(en);
    pk.x_col = take(en);
    pk.tinv_col = take(en);
    uint32_t* l_tmp = take(3 * n);
    hipStream_t st = ctx->stream;
    std::vector<Fe<SF>> wp(n), host(std::max(std::max(m * n, en), 3 * n));
    wp[0] = fe_one<SF>();
    for (size_t i = 1; i < n; i++) wp[i] = fe_mul(wp[i - 1], omega);
    std::vector<Fe<SF>> dpow(m ? m : 1);
    dpow[0] = fe_one<SF>();
    for (size_t j = 1; j < m; j++) dpow[j] = fe_mul(dpow[j - 1], delta);
    auto up = [&](uint32_t* dst, const Fe<SF>* src, size_t elems) -> int {
        if (!elems) return BZH_OK;
        BZH_HIP_TRY(ctx, hipMemcpyAsync(dst, src, elems * 32, hipMemcpyHostToDevice, st));
        BZH_HIP_TRY(ctx, hipStreamSynchronize(st));
        return BZH_OK;
    };
    auto to_coeff = [&](uint32_t* dst, const uint32_t* src, size_t count) -> int {
        if (!count) return BZH_OK;
        BZH_HIP_TRY(ctx, hipMemcpyAsync(dst, src, count * n * 32, hipMemcpyDeviceToDevice, st));
        return ntt_run(ctx, pk.field, dst, pk.k, count, pk.omega, nullptr, 1, BZH_FORM_MONTGOMERY);
    };
    auto to_extended = [&](uint32_t* dst, const uint32_t* polys, size_t count) -> int {
        if (!count) return BZH_OK;
        return ntt_run_padded(ctx, pk.field, dst, polys, pk.k, pk.ek, count, pk.eomega, pk.zeta);
    };
    BZH_TRY(up(pk.fixed, fixed_h.data(), nf * n));
    BZH_TRY(to_coeff(pk.fixed_polys, pk.fixed, nf));
    BZH_TRY(to_extended(pk.fixed_cosets, pk.fixed_polys, nf));
    for (size_t j = 0; j < m; j++)
        for (size_t rr = 0; rr < n; rr++) host[j * n + rr] = fe_mul(dpow[j], wp[rr]);
    BZH_TRY(up(pk.ident, host.data(), m * n));
    for (size_t j = 0; j < m; j++)
        for (size_t rr = 0; rr < n; rr++) host[j * n + rr] = fe_mul(dpow[map_c[j * n + rr]], wp[map_r[j * n + rr]]);
    BZH_TRY(up(pk.sigma, host.data(), m * n));
    BZH_TRY(to_coeff(pk.sigma_polys, pk.sigma, m));
    BZH_TRY(to_extended(pk.sigma_cosets, pk.sigma_polys, m));
    for (size_t i = 0; i < 3 * n; i++) host[i] = fe_zero<SF>();
    host[0] = fe_one<SF>();
    host[n + pk.usable] = fe_one<SF>();
    for (size_t i = pk.usable + 1; i < n; i++) host[2 * n + i] = fe_one<SF>();
    BZH_TRY(up(l_tmp, host.data(), 3 * n));
    BZH_TRY(ntt_run(ctx, pk.field, l_tmp, pk.k, 3, pk.omega, nullptr, 1, BZH_FORM_MONTGOMERY));
    BZH_TRY(to_extended(pk.l0, l_tmp, 3));  // l0, l_last, l_blind are consecutive
    {
        Fe<SF> x = zeta;
        for (size_t i = 0; i < en; i++) {
            host[i] = x;
            x = fe_mul(x, eomega);
        }
        BZH_TRY(up(pk.x_col, host.data(), en));
        std::vector<Fe<SF>> tinv(pk.ext);
        for (size_t i = 0; i < pk.ext; i++) tinv[i] = fe_inv(fe_sub(h_pow_u64(host[i], n), fe_one<SF>()));
        for (size_t i = 0; i < en; i++) host[i] = tinv[i % pk.ext];
        BZH_TRY(up(pk.tinv_col, host.data(), en));
    }

    BZH_TRY(materialize_hoist<SF>(ctx, pk));
    pk.q_builtin = nullptr;
    if (pk.q_ok) {
        size_t nb = 0;
        const bzh_builtin_quotient* tab = bzh_builtin_quotients ? bzh_builtin_quotients(&nb) : nullptr;
        for (size_t i = 0; i < nb; i++)
            if (tab[i].program_hash == pk.q_hash) {
                pk.q_builtin = tab[i].launch;
                pk.q_builtin29 = tab[i].launch29;
            }
    }
    if constexpr (fe29_supported<SF>()) {
        if (pk.q_builtin29 && !getenv("BZH_QUOTIENT_SATURATED")) {
            const Key29Layout k29(pk);
            BZH_HIP_TRY(ctx, hipMalloc((void**)&pk.key29, k29.end * 9 * en * 4));
            pk.key29_bytes = k29.end * 9 * en * 4;
            const dim3 blk(256);
            auto conv = [&](const uint32_t* src, size_t first, size_t ncols) {
                if (ncols) hipLaunchKernelGGL((k_sat_to_fe29_planes<SF>), dim3((unsigned)((en + 255) / 256), (unsigned)ncols), blk, 0, st, src, pk.key29 + first * 9 * en, en);
            };
            conv(pk.fixed_cosets, k29.fixed, (size_t)pk.nf);
            conv(pk.sigma_cosets, k29.sigma, m);
            conv(pk.l0, k29.misc, 5);       // l0, l_last, l_blind, x_col, tinv_col are consecutive columns of the key's allocation
            conv(pk.hoist, k29.hoist, pk.hoist_cols);
            BZH_HIP_TRY(ctx, hipGetLastError());
        } else {
            pk.q_builtin29 = nullptr;
        }
    } else {
        pk.q_builtin29 = nullptr;
    }
    const char* qenv = getenv("BZH_QUOTIENT");
    pk.q_select = (pk.q_builtin && !(qenv && !strcmp(qenv, "interp"))) ? BZH_QUOTIENT_BUILTIN : BZH_QUOTIENT_INTERPRETER;
    BZH_HIP_TRY(ctx, hipStreamSynchronize(st));
    *out = pkp.release();
    return BZH_OK;
}
