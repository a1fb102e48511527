// Part of the whole-proof translation unit (csrc/prove.hip): the PROVER -- create_proof for a batch of witnesses in lockstep.
#pragma once
// ---------------------------------------------------------------------------
// the lockstep prover
// ---------------------------------------------------------------------------
// prove() is the list of the protocol's phases (upstream's create_proof); each phase is a member function whose head comment
// names the members it reads and the members it fills.  Columns on the device, their transforms and commitments come from
// DeviceColumns (device_columns.hpp), shared with the verifier and keygen_vk.
template <class C>
struct Prover : DeviceColumns<C> {
    using DC = DeviceColumns<C>;
    using SF = typename DC::SF;
    using DC::arena;   // this ctx's workspace of the (shared) key
    using DC::commit;
    using DC::copy2d;
    using DC::ctx;
    using DC::dalloc;
    using DC::field;
    using DC::n;
    using DC::st;
    using DC::to_coeff;
    using DC::upload;
    using DC::zero;
    bzh_pk& pk;
    const size_t B;
    const size_t en, usable;
    // the key's shape, as every phase names it
    const int na, nf, ni, bf, nsets, nl, npieces, nz;
    const size_t bf1, m;
    std::vector<bzh_transcript*> T;
    std::vector<const uint8_t*> rng;  // per-proof cursor into the caller's randomness
    // seeded mode (bzh_prove_batch_seeded): the stream of proof b is ChaCha20(seed_b), addressed by 64-byte block; every
    // proof of a batch draws in lockstep, so one counter serves the batch
    bool seeded = false;
    std::vector<uint32_t> seed_keys;   // B x 8 words
    uint32_t* d_seed_keys = nullptr;
    uint64_t seed_ctr = 0;
    std::vector<uint64_t> host_ctr;    // draws taken on the host per proof since the last row draw (must stay in lockstep)
    std::vector<std::map<int, Fe<SF>>> env;   // per proof: the challenges and their powers, by symbol

    // ---- what one phase leaves for the later ones (device pointers: arena memory of this call) ----------------------------
    uint32_t *inst = nullptr, *inst_polys = nullptr, *inst_cosets = nullptr;   // evaluations | coefficients | extended coset
    uint32_t *adv = nullptr, *adv_polys = nullptr, *adv_cosets = nullptr;
    std::vector<Fe<SF>> adv_blinds;
    struct Lk {
        uint32_t *a_c, *s_c, *as, *polys, *cosets;   // compressed input, table | permuted (a, s) pair | its coefficients | cosets
        std::vector<Fe<SF>> blinds;  // (a, s) per proof
        std::vector<int32_t> status; // device permutation: one word per proof, landed by the d2h_finish of this lookup's commitment
    };
    std::vector<Lk> lk;
    uint32_t *zs = nullptr, *z_polys = nullptr, *z_cosets = nullptr;   // grand products: permutation sets, then lookups
    std::vector<Fe<SF>> z_blinds;
    uint32_t* random_poly = nullptr;
    std::vector<Fe<SF>> random_blinds;
    uint32_t* h = nullptr;                      // the quotient's coefficients (B x en)
    std::vector<Fe<SF>> h_blinds, h_blind;      // per piece | of h(X) = sum_i x^(n i) h_i(X)
    std::vector<Fe<SF>> xs;                     // the evaluation challenge x per proof
    Fe<SF> omega_m, omega_inv;
    std::map<int, Fe<SF>> wp;                   // omega^r by rotation (rot)
    // where each committed polynomial lives: (pointer of proof 0, elements between proofs)
    std::map<uint64_t, std::pair<const uint32_t*, size_t>> where;
    uint32_t* p_poly = nullptr;                 // multiopen's final polynomial with its blinds and point x3 (canonical limbs)
    std::vector<uint64_t> p_blinds, x3c;

    Prover(bzh_ctx* c, bzh_pk& p, size_t batch, Arena& ar)
        : DC(c, p, ar), pk(p), B(batch), en(p.en), usable(p.usable), na(p.na), nf(p.nf), ni(p.ni), bf(p.bf), nsets(p.nsets), nl(p.nl),
          npieces(p.npieces), nz(p.nsets + p.nl), bf1((size_t)p.bf + 1), m(p.perm_columns.size()), T(batch, nullptr), rng(batch), env(batch) {}
    ~Prover() {
        for (auto t : T)
            if (t) bzh_transcript_free(t);
    }

    // BZH_PROVE_TRACE=1: phase wall times on stderr, with a device sync at every phase boundary
    const bool trace = getenv("BZH_PROVE_TRACE") != nullptr;
    std::chrono::steady_clock::time_point t_last = std::chrono::steady_clock::now();
    void mark(const char* name) {
        if (!trace) return;
        (void)hipStreamSynchronize(st);
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[bzh_prove_batch] %-22s %8.2f ms\n", name, std::chrono::duration<double, std::milli>(now - t_last).count());
        t_last = now;
    }

    // BZH_WORKSPACE_COSETWISE (bzh_pk_workspace_select, read once per call): no per-proof column is taken to the extended coset;
    // the quotient is evaluated one coset of n points at a time out of n-sized buffers (cosetwise_setup, cosetwise_launch).
    const bool cosetwise = [&] {
        std::lock_guard<std::mutex> lk(pk.rt.mu);
        return pk.ws_select == BZH_WORKSPACE_COSETWISE;
    }();
    // The quotient's per-proof columns on the extended coset exist for the quotient alone.  When the builtin kernel's
    // unsaturated-limb flavour will run (decided once per call), coeff_to_extended writes them straight as fe29 planes
    // (9 words per element, ntt_store_out) and no saturated copy is ever made.
    const bool q29 = [&] {
        if constexpr (!fe29_supported<SF>()) return false;
        if (cosetwise) return false;   // (that mode always runs the interpreter, in saturated limbs)
        std::lock_guard<std::mutex> lk(pk.rt.mu);
        return pk.q_ok && pk.q_builtin29 && pk.key29 && pk.q_select == BZH_QUOTIENT_BUILTIN && pk.en % 128 == 0 && pk.ek >= 12 &&
               pk.ek <= 27 /* 32-bit byte offsets into a plane (fe29_load_planes_g) */ && !getenv("BZH_QUOTIENT_V1");
    }();
    uint32_t* ext_alloc(size_t cols) { return q29 ? (uint32_t*)arena.alloc(cols * 9 * en * 4) : dalloc(cols * en); }
    // an expression program's four host-side pieces -- constants | instructions | column pointers | column strides -- laid out
    // 256-byte aligned in one arena block and sent with ONE staging copy (they were four: ~130 of a proof's ~145 small uploads)
    struct ProgramArgs {
        uint32_t* consts = nullptr;
        char *prog = nullptr, *ptrs = nullptr, *strides = nullptr;
    };
    int upload_program(const void* cv, size_t cv_bytes, const void* ops, size_t op_bytes, const void* ptrs, const void* strides, size_t ncols,
                       ProgramArgs& out) {
        auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
        const size_t o_prog = al(cv_bytes), o_ptrs = o_prog + al(op_bytes), o_strides = o_ptrs + al(ncols * 8), total = o_strides + al(ncols * 8);
        char* dev = (char*)arena.alloc(total);
        if (!dev) return BZH_E_OOM;
        char* slot = nullptr;
        // (cv == null: the constants are written on the device -- vanishing_device.hpp --, their room is left alone)
        const size_t from = cv ? 0 : o_prog;
        BZH_TRY(h2d_stage(ctx, total - from, &slot));
        if (cv) memcpy(slot, cv, cv_bytes);
        memcpy(slot + (o_prog - from), ops, op_bytes);
        if (ncols) {
            memcpy(slot + (o_ptrs - from), ptrs, ncols * 8);
            memcpy(slot + (o_strides - from), strides, ncols * 8);
        }
        BZH_TRY(h2d_commit(ctx, dev + from, slot, total - from));
        out.consts = (uint32_t*)dev;
        out.prog = dev + o_prog;
        out.ptrs = dev + o_ptrs;
        out.strides = dev + o_strides;
        return BZH_OK;
    }

    Fe<SF> draw(size_t b) {
        if (seeded) {
            uint32_t blk[16];
            chacha20_block(&seed_keys[b * 8], seed_ctr + host_ctr[b]++, blk);
            return h_from_u512<SF>(reinterpret_cast<const uint8_t*>(blk));
        }
        const Fe<SF> v = h_from_u512<SF>(rng[b]);
        rng[b] += 64;
        return v;
    }
    // seeded mode: fold the host-side draws into the batch counter (every proof must have taken the same number)
    int seed_sync() {
        for (size_t b = 1; b < B; b++)
            if (host_ctr[b] != host_ctr[0]) return BZH_E_ARG;
        seed_ctr += host_ctr[0];
        std::fill(host_ctr.begin(), host_ctr.end(), 0);
        return BZH_OK;
    }
    // seeded mode: the next `count` 64-byte draws of every proof, generated on the device (B x count x 16 words)
    int seed_rows(size_t count, uint32_t* raw) {
        BZH_TRY(seed_sync());
        hipLaunchKernelGGL(k_chacha20_rows, dim3((unsigned)((count + 255) / 256), (unsigned)B), dim3(256), 0, st, d_seed_keys, seed_ctr, count, raw);
        BZH_HIP_TRY(ctx, hipGetLastError());
        seed_ctr += count;
        return BZH_OK;
    }
    // the next `count` draws of every proof, reduced on the device into dst (B x count, proof-major)
    int draw_rows(size_t count, uint32_t* dst) {
        if (!count) return BZH_OK;
        uint32_t* raw = (uint32_t*)arena.alloc(B * count * 64);
        if (!raw) return BZH_E_OOM;
        if (seeded) {
            BZH_TRY(seed_rows(count, raw));
            return random_field(ctx, field, raw, B * count, dst);
        }
        char* stage = nullptr;  // one upload for the whole batch, assembled in pinned memory
        BZH_TRY(h2d_stage(ctx, B * count * 64, &stage));
        for (size_t b = 0; b < B; b++) {
            memcpy(stage + b * count * 64, rng[b], count * 64);
            rng[b] += count * 64;
        }
        BZH_TRY(h2d_commit(ctx, raw, stage, B * count * 64));
        return random_field(ctx, field, raw, B * count, dst);
    }
    // `rows` fresh draws into rows first_row.. of each of the batch's B x cols_per_proof columns at dst (`pitch` elements apart):
    // advice and lookup columns take bf + 1 rows at `usable`, grand products bf rows at n - bf
    int blind_rows(uint32_t* dst, size_t first_row, size_t rows, size_t cols_per_proof, size_t pitch) {
        uint32_t* drawn = dalloc(B * cols_per_proof * rows);
        if (!drawn) return BZH_E_OOM;
        BZH_TRY(draw_rows(cols_per_proof * rows, drawn));
        return copy2d(dst + first_row * 8, pitch, drawn, rows, rows, B * cols_per_proof);
    }
    Fe<SF> squeeze(size_t b) {
        uint64_t ch[4];
        bzh_transcript_squeeze_challenge(T[b], ch);
        return fe_to_mont(fe_from_u64<SF>(ch));
    }
    void write_scalar(size_t b, const Fe<SF>& v) {
        uint64_t s[4];
        fe_to_u64<SF>(s, fe_from_mont(v));
        bzh_transcript_write_scalar(T[b], s);
    }

    // ---- transforms ------------------------------------------------------------------------------
    int to_extended(uint32_t* dst, const uint32_t* polys, size_t count) {
        if (!count) return BZH_OK;
        if (q29) return ntt_run_padded(ctx, field, nullptr, polys, pk.k, pk.ek, count, pk.eomega, pk.zeta, dst);
        return ntt_run_padded(ctx, field, dst, polys, pk.k, pk.ek, count, pk.eomega, pk.zeta);
    }
    // commit `count` columns of n rows in the basis the key offers: their evaluations against g_lagrange when the key has that
    // table (bzh_pk_set_lagrange; shift_row: see DeviceColumns::commit), their coefficients against the SRS otherwise
    int commit_columns(const uint32_t* evals, const uint32_t* polys, size_t count, const std::vector<Fe<SF>>& blinds, std::vector<uint64_t>& xy,
                       long shift_row = -1) {
        if (pk.srs_lagrange) return commit(pk.srs_lagrange, evals, n, count, blinds, xy, true, shift_row);
        return commit(pk.srs, polys, n, count, blinds, xy);
    }
    // evaluate `count` polynomials (contiguous, n coefficients each) at one point each
    int evals(const uint32_t* stacked, size_t count, const std::vector<Fe<SF>>& points, std::vector<Fe<SF>>& out) {
        out.resize(count);
        if (!count) return BZH_OK;
        ArenaScope scope(arena);
        uint32_t* xs = dalloc(count);
        uint32_t* res = dalloc(count);
        if (!xs || !res) return BZH_E_OOM;
        BZH_TRY(upload(xs, points.data(), count));
        BZH_TRY(poly_eval(ctx, field, stacked, n, count, xs, 1, res));
        BZH_TRY(d2h_async(ctx, out.data(), res, count * 32));
        BZH_TRY(d2h_finish(ctx));
        return BZH_OK;
    }

    // ---- compiled programs -------------------------------------------------------------------------
    // a program's constant table for `rows` proofs, `words` 32-bit words per constant: a symbol takes proof b's value from env[b]
    // (BZH_E_ARG when the proof has none yet), a literal its own; put(dst, value) writes one constant in the evaluator's format
    template <class Put>
    int fill_consts(const std::vector<ConstEnt>& consts, size_t rows, size_t words, Put put, std::vector<uint32_t>& cv) {
        const size_t nc = consts.size();
        cv.assign(std::max<size_t>(rows * nc, 1) * words, 0u);
        for (size_t b = 0; b < rows; b++)
            for (size_t i = 0; i < nc; i++) {
                const ConstEnt& c = consts[i];
                Fe<SF> v;
                if (c.sym >= 0) {
                    auto f = env[b].find(c.sym);
                    if (f == env[b].end()) return BZH_E_ARG;
                    v = f->second;
                } else {
                    memcpy(v.l, c.val, 32);
                }
                put(&cv[(b * nc + i) * words], v);
            }
        return BZH_OK;
    }
    static void put_saturated(uint32_t* dst, const Fe<SF>& v) { memcpy(dst, v.l, 32); }
    // run is two halves, like run_quotient.  The first finds or compiles the key's cached program and builds its arguments in
    // device memory: the constant table from env (host transcripts), or only its room (consts_on_device:
    // commitments_device.hpp fills it on the device from theta in HBM).  The second, run_launch, is the interpreter's launch.
    struct RunProgram {
        const Program* pg = nullptr;
        ProgramArgs pa;
        bool per_proof = false;   // a constant is a symbol: the table has one row per proof
    };
    template <class Build>
    int run(uint64_t pkey, Build build, const Cols& reg, size_t size, uint32_t* d_out) {
        RunProgram rp;
        BZH_TRY(run_args(pkey, build, reg, false, rp));
        return run_launch(rp, size, d_out);
    }
    template <class Build>
    int run_args(uint64_t pkey, Build build, const Cols& reg, bool consts_on_device, RunProgram& rp) {
        const Program* pgp = nullptr;
        {
            std::lock_guard<std::mutex> lk(pk.rt.mu);   // map nodes are stable: the program outlives the lock
            auto it = pk.progs.find(pkey);
            if (it == pk.progs.end()) {
                EPool ep;
                const int root = build(ep);
                Compiler cc(ep);
                cc.prog.result_slot = cc.emit(root);
                if (cc.overflow) return BZH_E_RANGE;
                it = pk.progs.insert({pkey, std::move(cc.prog)}).first;
            }
            pgp = &it->second;
        }
        const Program& pg = *pgp;
        const size_t nc = pg.consts.size(), ncols = reg.ptr.size();
        rp.pg = pgp, rp.per_proof = false;
        for (auto& c : pg.consts) rp.per_proof |= c.sym >= 0;
        const size_t rows = rp.per_proof ? B : 1;
        std::vector<uint32_t> cv;
        if (!consts_on_device) BZH_TRY(fill_consts(pg.consts, rows, 8, put_saturated, cv));
        return upload_program(consts_on_device ? nullptr : cv.data(), std::max<size_t>(rows * nc, 1) * 32, pg.ops.data(),
                              pg.ops.size() * sizeof(bzh_expr_op), reg.ptr.data(), reg.stride.data(), ncols, rp.pa);
    }
    int run_launch(const RunProgram& rp, size_t size, uint32_t* d_out) {
        const Program& pg = *rp.pg;
        int nslots = pg.result_slot + 1;
        for (auto& o : pg.ops) nslots = std::max(nslots, (int)o.dst + 1);  // operands only read slots written before
        return expr_eval(ctx, field, rp.pa.prog, (int)pg.ops.size(), (const uint32_t* const*)rp.pa.ptrs, (const size_t*)rp.pa.strides,
                         rp.pa.consts, rp.per_proof ? pg.consts.size() : 0, size, pg.result_slot, B, nslots, d_out);
    }

    // The quotient through VM v2 (the program compiled at bzh_pk_create), in one of four flavours: the builtin kernel in unsaturated
    // limbs (q29: `reg` then holds fe29 PLANES -- to_extended wrote the per-proof ones, the key's were converted at bzh_pk_create --
    // and the constants are converted here, 9 limbs in a 12-word slot), the builtin kernel in saturated limbs, the caller's module,
    // the interpreter.  Returns BZH_E_RANGE when the circuit does not fit VM v2 (the caller falls back to the plain fold through `run`).
    static void put_fe29(uint32_t* dst, const Fe<SF>& v) {
        const Fe29<SF> w = fe29_from_sat_reduced(v);
        memcpy(dst, w.l, 36);
    }
    // run_quotient is two halves.  The first builds the program's arguments in device memory: the constant table from env (host
    // transcripts), or only its room (cv == null: vanishing_device.hpp fills it on the device from challenges in HBM).  The
    // second, launch_quotient, picks the flavour and launches; both callers share it.
    bool quotient_fits(size_t size) const { return pk.q_ok && size % 128 == 0 && size == pk.en; }
    size_t quotient_const_words() const { return q29 ? 12 : 8; }
    int quotient_args(const Cols& reg, const void* cv, size_t cv_bytes, ProgramArgs& pa) {
        const Program2& pg = pk.qprog;   // (the unsaturated kernel's launch carries no instructions: only the interpreter reads them)
        return upload_program(cv, cv_bytes, pg.ops.data(), q29 ? 0 : pg.ops.size() * sizeof(ExprOp2), reg.ptr.data(), reg.stride.data(),
                              reg.ptr.size(), pa);
    }
    int run_quotient(const Cols& reg, size_t size, uint32_t* d_out) {
        if (!quotient_fits(size)) return BZH_E_RANGE;
        std::vector<uint32_t> cv;
        BZH_TRY(fill_consts(pk.qprog.consts, B, quotient_const_words(), q29 ? put_fe29 : put_saturated, cv));
        ProgramArgs pa;
        BZH_TRY(quotient_args(reg, cv.data(), cv.size() * 4, pa));
        return launch_quotient(reg, size, pa, d_out);
    }
    int launch_quotient(const Cols& reg, size_t size, const ProgramArgs& pa, uint32_t* d_out) {
        hipFunction_t q_fn = nullptr;
        bzh_quotient_launch_fn q_builtin = nullptr;
        if (q29) {
            q_builtin = pk.q_builtin29;
        } else {
            std::lock_guard<std::mutex> lk(pk.rt.mu);
            if (pk.q_select == BZH_QUOTIENT_MODULE) q_fn = pk.q_fn;
            else if (pk.q_select == BZH_QUOTIENT_BUILTIN) q_builtin = pk.q_builtin;
        }
        const Program2& pg = pk.qprog;
        const size_t nc = pg.consts.size(), ncols = reg.ptr.size();
        const uint32_t* const* d_ptrs = (const uint32_t* const*)pa.ptrs;
        const size_t* d_strides = (const size_t*)pa.strides;
        const uint32_t* d_consts = pa.consts;
        if (ctx->profiling) {   // the quotient pass reads every extended column once and writes h: per-proof columns
            double cols_read = 0;   // count per proof, columns of the key once per launch (the hoisted ones not at all)
            for (size_t i = 0; i < ncols - pk.hoist_cols; i++) cols_read += reg.stride[i] ? (double)B : 1.0;
            ctx->alg_bytes[BZH_T_QUOTIENT] += (cols_read + (double)B) * (double)size * 32.0;
        }
        if (q_builtin) {   // the same program as a kernel generated at build time
            ScopedTimer t(ctx, BZH_T_QUOTIENT);
            q_builtin((unsigned)(size / 128), (unsigned)B, (void*)st, d_ptrs, d_strides, d_consts, nc, size, d_out);
            BZH_HIP_TRY(ctx, hipGetLastError());
            return BZH_OK;
        }
        if (q_fn) {   // the same program as a code object of the caller's (bzh_pk_set_quotient_module)
            ScopedTimer t(ctx, BZH_T_QUOTIENT);
            size_t a_nc = nc, a_size = size;
            void* args[] = {&d_ptrs, &d_strides, &d_consts, &a_nc, &a_size, &d_out};
            BZH_HIP_TRY(ctx, hipModuleLaunchKernel(q_fn, (unsigned)(size / 128), (unsigned)B, 1, 128, 1, 1, 0, st, args, nullptr));
            return BZH_OK;
        }
        return expr_eval2(ctx, field, pa.prog, (int)pg.ops.size(), d_ptrs, d_strides, d_consts, nc, size, B, pg.nlds, d_out);
    }

    // ---- the quotient coset by coset (BZH_WORKSPACE_COSETWISE) --------------------------------------------------------------
    // The extended domain is eight cosets of the n-sized one: with w = eomega^8 and zeta_j = zeta eomega^j, extended point 8 r + j
    // is zeta_j w^r.  A column's values on coset j are ONE n-point transform of its coefficients with coset shift zeta_j, and a
    // rotation (a multiple of 8 extended steps) never leaves the coset.  So: per-proof coefficient forms -> n-sized buffers
    // (carved once, refilled for every j: a copy and an in-place ntt_run per buffer), one k_expr_vm2_cosets launch per j for the
    // whole batch, the key's own columns read where they lie at 8 r + j, h written at 8 r + j.  Always the interpreter.
    struct CosetSeg {
        const uint32_t* polys;   // `count` polynomials of n coefficients
        uint32_t* buf;           // their values on the current coset
        size_t count;
    };
    struct CosetWork {
        std::vector<CosetSeg> segs;
        Cols reg;
        uint32_t* d_shifts = nullptr;
    };
    bool cosetwise_fits() const { return pk.q_ok && pk.ek == pk.k + 3 && !getenv("BZH_QUOTIENT_V1"); }
    // carves the four buffers (their sizes are workspace_items': the plan and the carve cannot drift apart), builds the registry
    // over them and uploads the per-column shifts.  lk_p: one (B, 2, n) block per lookup (lk_cols == 2), or one (B, 2 nl, n) block
    int cosetwise_setup(const uint32_t* adv_p, const uint32_t* inst_p, const uint32_t* z_p, const std::vector<const uint32_t*>& lk_p,
                        size_t lk_cols, CosetWork& cw) {
        if (!cosetwise_fits()) {
            ctx->last_error = "BZH_WORKSPACE_COSETWISE needs a circuit the quotient interpreter fits and an extended domain of 8 n";
            return BZH_E_RANGE;
        }
        const WorkspaceItems wi = workspace_items(pk, B, BZH_WORKSPACE_COSETWISE);
        uint32_t* b_adv = (uint32_t*)arena.alloc(wi.adv_bytes);
        uint32_t* b_inst = (uint32_t*)arena.alloc(wi.inst_bytes);
        uint32_t* b_z = (uint32_t*)arena.alloc(wi.z_bytes);
        uint32_t* b_lk = nl ? (uint32_t*)arena.alloc(wi.lk_bytes) : nullptr;
        if (!b_adv || !b_inst || !b_z || (nl && !b_lk)) return BZH_E_OOM;
        cw.segs.push_back({adv_p, b_adv, B * (size_t)na});
        if (ni) cw.segs.push_back({inst_p, b_inst, B * (size_t)ni});
        if (nz) cw.segs.push_back({z_p, b_z, B * (size_t)nz});
        QuotientPtrs qp;
        qp.adv = b_adv, qp.inst = b_inst, qp.z = b_z, qp.lk_cols = lk_cols;
        const size_t lk_block = wi.lk_bytes / 4 / (size_t)std::max(nl, 1);   // words of one lookup's (B, 2, n) block
        for (int i = 0; i < nl; i++) {
            if (lk_cols == 2) {
                cw.segs.push_back({lk_p[i], b_lk + (size_t)i * lk_block, B * 2});
                qp.lk.push_back(b_lk + (size_t)i * lk_block);
            } else {
                if (i == 0) cw.segs.push_back({lk_p[0], b_lk, B * lk_cols});
                qp.lk.push_back(b_lk + (size_t)i * 2 * n * 8);
            }
        }
        quotient_registry(pk, qp, false, cw.reg, n);
        std::vector<uint32_t> shifts(cw.reg.ptr.size());
        for (size_t c = 0; c < shifts.size(); c++) shifts[c] = cw.reg.stride[c] ? 3u : 0u;   // per-proof: n-sized | the key's: on 8 n
        cw.d_shifts = (uint32_t*)arena.alloc(shifts.size() * 4);
        if (!cw.d_shifts) return BZH_E_OOM;
        return h2d_small(ctx, cw.d_shifts, shifts.data(), shifts.size() * 4);
    }
    int cosetwise_launch(const CosetWork& cw, const ProgramArgs& pa, uint32_t* d_out) {
        const Program2& pg = pk.qprog;
        Fe<SF> w, shift;
        {
            uint64_t t[4];
            memcpy(t, pk.eomega, 32);
            w = fe_from_u64<SF>(t);
            memcpy(t, pk.zeta, 32);
            shift = fe_from_u64<SF>(t);
        }
        if (ctx->profiling) {   // as launch_quotient counts: every column read once over the 8 n rows and h written -- plus what
            double cols_read = 0, refilled = 0;   // this mode adds: each per-proof polynomial copied (read + write) eight times
            for (size_t i = 0; i < cw.reg.ptr.size() - pk.hoist_cols; i++) cols_read += cw.reg.stride[i] ? (double)B : 1.0;
            for (const CosetSeg& sg : cw.segs) refilled += (double)sg.count;
            ctx->alg_bytes[BZH_T_QUOTIENT] += ((cols_read + (double)B) * (double)en + refilled * 8.0 * 2.0 * (double)n) * 32.0;
        }   // (the eight n-point transforms per polynomial are counted by ntt_run itself, under BZH_T_NTT)
        const uint32_t* const* tables[8];
        for (auto& t : tables) t = (const uint32_t* const*)pa.ptrs;
        auto refill = [&](unsigned j) -> int {
            uint64_t sh[4];
            fe_to_u64<SF>(sh, shift);   // zeta eomega^j, Montgomery limbs as ntt_run takes them
            shift = fe_mul(shift, w);
            (void)j;
            for (const CosetSeg& sg : cw.segs) {
                BZH_HIP_TRY(ctx, hipMemcpyAsync(sg.buf, sg.polys, sg.count * n * 32, hipMemcpyDeviceToDevice, st));
                BZH_TRY(ntt_run(ctx, field, sg.buf, pk.k, sg.count, pk.omega, sh, 0, BZH_FORM_MONTGOMERY));
            }
            return BZH_OK;
        };
        return expr_eval2_cosets(ctx, field, pa.prog, (int)pg.ops.size(), tables, (const size_t*)pa.strides, cw.d_shifts, pa.consts,
                                 pg.consts.size(), pk.k, B, pg.nlds, d_out, refill);
    }

    // ---- the phases of create_proof, in protocol order ---------------------------------------------------------------------
    // the opening point x w^r of proof b.  reads xs, omega_m, omega_inv; caches omega^r in wp
    Fe<SF> rot(size_t b, int r) {
        auto it = wp.find(r);
        if (it == wp.end()) it = wp.insert({r, r >= 0 ? h_pow_u64(omega_m, (uint64_t)r) : h_pow_u64(omega_inv, (uint64_t)(-(int64_t)r))}).first;
        return fe_mul(xs[b], it->second);
    }
    // rows of n elements from J (pointer of proof 0, elements between proofs) sources -> dst, (B, J, n)
    int gather(const std::vector<std::pair<const uint32_t*, size_t>>& srcs, uint32_t* dst) {
        const size_t J = srcs.size();
        std::vector<const uint32_t*> ps(J);
        std::vector<size_t> ss(J);
        for (size_t j = 0; j < J; j++) {
            ps[j] = srcs[j].first;
            ss[j] = srcs[j].second;
        }
        char* stage = (char*)arena.alloc(J * 16 + 512);
        if (!stage) return BZH_E_OOM;
        char* d_ss = stage + ((J * 8 + 255) & ~(size_t)255);
        BZH_TRY(h2d_small(ctx, stage, ps.data(), J * 8));
        BZH_TRY(h2d_small(ctx, d_ss, ss.data(), J * 8));
        hipLaunchKernelGGL(k_gather_rows, dim3((unsigned)((2 * n + 255) / 256), (unsigned)J, (unsigned)B), dim3(256), 0, st, (uint4*)dst,
                           (const uint4* const*)stage, (const size_t*)d_ss, n, J);
        BZH_HIP_TRY(ctx, hipGetLastError());
        return BZH_OK;
    }
    // the witness and fixed columns over the domain, as the lookup compress programs name them.  reads adv, inst
    void lag_registry(Cols& reg) {
        for (int i = 0; i < na; i++) reg.add(key(K_ADV, i), adv + (size_t)i * n * 8, (size_t)na * n);
        for (int i = 0; i < nf; i++) reg.add(key(K_FIX, i), pk.fixed + (size_t)i * n * 8, 0);
        for (int i = 0; i < ni; i++) reg.add(key(K_INST, i), inst + (size_t)i * n * 8, (size_t)ni * n);
    }
    // one permutation column over the domain.  reads adv, inst
    int lag_col(Cols& reg, std::pair<int, int> col) {
        if (col.first == CX_ADVICE) return reg.add(key(K_ADV, col.second), adv + (size_t)col.second * n * 8, (size_t)na * n);
        if (col.first == CX_FIXED) return reg.add(key(K_FIX, col.second), pk.fixed + (size_t)col.second * n * 8, 0);
        return reg.add(key(K_INST, col.second), inst + (size_t)col.second * n * 8, (size_t)ni * n);
    }

    // fills T (one transcript per proof, the key absorbed)
    int begin_transcripts() {
        for (size_t b = 0; b < B; b++) {
            BZH_TRY(bzh_transcript_new(field, &T[b]));
            bzh_transcript_common_scalar(T[b], pk.vk_repr);
        }
        return BZH_OK;
    }

    // 1. instance columns.  fills inst, inst_polys; the commitments go into the transcripts unwritten (the verifier recomputes them)
    int commit_instances(const uint64_t* instances, size_t inst_rows) {
        inst = dalloc(B * std::max(ni, 1) * n);
        inst_polys = dalloc(B * std::max(ni, 1) * n);
        if (!inst || !inst_polys) return BZH_E_OOM;
        if (!ni) return BZH_OK;
        BZH_TRY(zero(inst, B * ni * n));
        if (inst_rows) {
            std::vector<Fe<SF>> hv(B * ni * inst_rows);
            for (size_t i = 0; i < hv.size(); i++) hv[i] = fe_to_mont(fe_from_u64<SF>(instances + 4 * i));
            uint32_t* tmp = dalloc(hv.size());
            if (!tmp) return BZH_E_OOM;
            BZH_TRY(upload(tmp, hv.data(), hv.size()));
            BZH_TRY(copy2d(inst, n, tmp, inst_rows, inst_rows, B * ni));
        }
        BZH_TRY(to_coeff(inst_polys, inst, B * ni));
        std::vector<uint64_t> xy;
        BZH_TRY(commit_columns(inst, inst_polys, B * ni, std::vector<Fe<SF>>(B * ni, fe_one<SF>()), xy));
        for (size_t b = 0; b < B; b++)
            for (int i = 0; i < ni; i++) bzh_transcript_common_point(T[b], &xy[(b * ni + i) * 8]);
        return BZH_OK;
    }

    // 2. advice columns: the caller's witness, blinding rows, commitments, theta.  fills adv, adv_polys, adv_blinds, env[SY_THETA]
    int commit_advice(const uint32_t* d_advice_in) {
        adv = dalloc(B * na * n);
        adv_polys = dalloc(B * na * n);
        if (!adv || !adv_polys) return BZH_E_OOM;
        BZH_HIP_TRY(ctx, hipMemcpyAsync(adv, d_advice_in, B * na * n * 32, hipMemcpyDeviceToDevice, st));
        BZH_TRY(blind_rows(adv, usable, bf1, na, n));
        adv_blinds.resize(B * na);
        for (size_t b = 0; b < B; b++)
            for (int i = 0; i < na; i++) adv_blinds[b * na + i] = draw(b);
        BZH_TRY(to_coeff(adv_polys, adv, B * na));
        std::vector<uint64_t> xy;
        BZH_TRY(commit_columns(adv, adv_polys, B * na, adv_blinds, xy));
        for (size_t b = 0; b < B; b++) {
            for (int i = 0; i < na; i++) bzh_transcript_write_point(T[b], C::id, &xy[(b * na + i) * 8]);
            env[b][SY_THETA] = squeeze(b);
        }
        return BZH_OK;
    }

    // The witness on the extended coset.  Queued late on purpose: after the lookups' compress programs and before the host sort,
    // so that it runs on the device while the host sorts the lookups (a second call does nothing).
    // reads inst_polys, adv_polys; fills inst_cosets, adv_cosets
    int extend_witness() {
        if (adv_cosets || cosetwise) return BZH_OK;
        inst_cosets = ext_alloc(B * std::max(ni, 1));
        adv_cosets = ext_alloc(B * na);
        if (!inst_cosets || !adv_cosets) return BZH_E_OOM;
        BZH_TRY(to_extended(inst_cosets, inst_polys, B * ni));
        return to_extended(adv_cosets, adv_polys, B * na);
    }

    // A key on which bzh_pk_lookup_select was never called permutes on the device from this batch size up and on the host below
    // it.  Measured per bzh_prove_batch call on one MI355X box (Board, k = 14, seeded, HOST and DEVICE alternating on one key,
    // median of five): B = 1 HOST 14.96 ms, DEVICE 15.03; B = 8 HOST 26.02, DEVICE 25.76; B = 64 HOST 103.94, DEVICE 101.66 --
    // and `bench.py --batch 1 --concurrency 1 --no-kernel-timers` 9.51 ms per proof on the host path against 9.61 on the device
    // (three runs each, the host path's spread 0.04 ms): with one pair the device path is a chain of one- and two-workgroup
    // launches.  8 is the smallest size measured at which DEVICE is not worse.
    static constexpr size_t kLookupDeviceMinBatch = 8;

    // The lookup permutation on the device (csrc/lookup_permute.hip), straight from the Montgomery columns into d.as in its
    // (B, 2, n) layout.  Nothing is waited for here: the B status words are queued with d2h_async into d.status (a member of Lk,
    // so the destination outlives this scope) and land at the d2h_finish of this lookup's own commitment; lookups() reads them
    // there, before anything of this lookup goes into a transcript.  Committing the columns of a pair that turns out to have
    // failed is safe: such a pair keeps every index in bounds and still writes every row below `usable` of both columns with a
    // reduced field element (a run start without a table copy is filled with a leftover like a repeated row: csrc/lookup_permute.hip).
    // The workspace goes back to the arena when the scope ends, before the device has run any of this: its kernels and the copy
    // of the status words are queued on the ctx's stream, and so is everything that takes the same arena memory afterwards (all
    // device work of a prove call runs on that one stream), so the later work cannot overtake them.
    // reads d.a_c, d.s_c; fills d.as up to `usable`, queues d.status
    int permute_on_device(Lk& d) {
        mark(" lk:compress");
        d.status.assign(B, 0);
        ArenaScope scope(arena);
        void* ws = arena.alloc(lookup_permute_ws_bytes(usable, B));
        if (!ws) return BZH_E_OOM;
        int32_t* d_status = nullptr;
        BZH_TRY(lookup_permute(ctx, field, d.a_c, d.s_c, n, usable, B, BZH_FORM_MONTGOMERY, d.as, d.as + n * 8, 2 * n, n, ws, &d_status));
        BZH_TRY(d2h_async(ctx, d.status.data(), d_status, B * sizeof(int32_t)));
        mark(" lk:permute");
        return BZH_OK;
    }

    // The lookup permutation as one host sort per proof.  The compressed columns come back through pinned memory; the permuted
    // pair is assembled in a pinned slot in the device layout (B, 2, n) (rows past `usable` zero until the blinding rows land)
    // and goes up in one piece.  reads d.a_c, d.s_c; fills d.as; queues extend_witness under the sort
    int permute_on_host(Lk& d) {
        char *ah_c = nullptr, *sh_c = nullptr, *as_c = nullptr;
        BZH_TRY(pin_big_reserve(ctx, 4 * B * n * 32 + ((size_t)3 << 20)));
        BZH_TRY(pin_big_take(ctx, B * n * 32, &ah_c));
        BZH_TRY(pin_big_take(ctx, B * n * 32, &sh_c));
        BZH_TRY(pin_big_take(ctx, B * 2 * n * 32, &as_c));
        // the host sorts canonical integers: convert on the device (copies; the Montgomery originals feed the grand product)
        uint32_t* canon = dalloc(2 * B * n);
        if (!canon) return BZH_E_OOM;
        BZH_HIP_TRY(ctx, hipMemcpyAsync(canon, d.a_c, B * n * 32, hipMemcpyDeviceToDevice, st));
        BZH_HIP_TRY(ctx, hipMemcpyAsync(canon + B * n * 8, d.s_c, B * n * 32, hipMemcpyDeviceToDevice, st));
        BZH_TRY(field_convert(ctx, field, canon, 2 * B * n, 0));
        BZH_TRY(xfer_launch(ctx, ah_c, canon, B * n * 32, hipMemcpyDeviceToHost));
        BZH_TRY(xfer_launch(ctx, sh_c, canon + B * n * 8, B * n * 32, hipMemcpyDeviceToHost));
        BZH_HIP_TRY(ctx, hipStreamSynchronize(st));
        const uint64_t* ah = (const uint64_t*)ah_c;
        const uint64_t* sh = (const uint64_t*)sh_c;
        mark(" lk:compress+d2h");
        BZH_TRY(extend_witness());
        mark(" lk:extend_witness");
        uint64_t* as = (uint64_t*)as_c;
        for (size_t v = 0; v < 2 * B; v++) memset(as + (v * n + usable) * 4, 0, (n - usable) * 32);
        {  // one sort per proof on host threads
            // short-lived pool, capped: several provers (threads, ranks) run this at once on the same host
            const size_t nthreads = std::min<size_t>({B, (size_t)host_thread_budget(), (size_t)8});
            std::vector<int> rcs(B, BZH_OK);
            std::vector<std::thread> th;
            auto work = [&](size_t t) {
                for (size_t b = t; b < B; b += nthreads)
                    rcs[b] = bzh_permute_expression_pair(field, &ah[b * n * 4], &sh[b * n * 4], usable, BZH_FORM_CANONICAL,
                                                         as + (b * 2) * n * 4, as + (b * 2 + 1) * n * 4);
            };
            for (size_t t = 1; t < nthreads; t++) th.emplace_back(work, t);
            work(0);   // the calling thread takes a share (a single proof starts no thread at all)
            for (auto& t : th) t.join();
            for (int rc : rcs)
                if (rc) return rc;
        }
        mark(" lk:sort");
        BZH_TRY(h2d_commit(ctx, d.as, as_c, B * 2 * n * 32));
        BZH_TRY(field_convert(ctx, field, d.as, B * 2 * n, 1));  // back to Montgomery form (the zero rows stay zero)
        mark(" lk:h2d");
        return BZH_OK;
    }

    // the compress expression of lookup li's input (side 0) or table (side 1) over lag_registry's columns: Horner in theta over
    // its expressions -- the key's cached programs key(20 + side, li)
    int compress_root(int li, int side, EPool& ep, Cols& reg) {
        std::vector<int> terms;
        for (int e : side ? pk.lookups[li].second : pk.lookups[li].first) terms.push_back(lower(pk, e, ep, reg, 1));
        return ep.horner(terms, ep.sym(SY_THETA));
    }

    // 3. lookups: compress, permute (device kernels or host sort: bzh_pk_lookup_select), blind and commit; then beta, gamma.
    // reads adv, inst, env[SY_THETA]; fills lk (all but the cosets), inst_cosets, adv_cosets, env[SY_BETA], env[SY_GAMMA]
    int lookups() {
        const bool lk_device = [&] {
            std::lock_guard<std::mutex> g(pk.rt.mu);
            if (!pk.lk_chosen) return B >= kLookupDeviceMinBatch;
            return pk.lk_select == BZH_LOOKUP_DEVICE;
        }();
        lk.resize(nl);
        std::vector<uint64_t> xy;
        for (int li = 0; li < nl; li++) {
            Lk& d = lk[li];
            d.a_c = dalloc(B * n);
            d.s_c = dalloc(B * n);
            d.as = dalloc(B * 2 * n);
            d.polys = dalloc(B * 2 * n);
            if (!d.a_c || !d.s_c || !d.as || !d.polys) return BZH_E_OOM;
            Cols reg;
            lag_registry(reg);
            for (int side = 0; side < 2; side++)
                BZH_TRY(run(key(20 + side, li), [&](EPool& ep) { return compress_root(li, side, ep, reg); }, reg, n, side ? d.s_c : d.a_c));
            BZH_TRY(lk_device ? permute_on_device(d) : permute_on_host(d));
            BZH_TRY(blind_rows(d.as, usable, bf1, 2, n));
            d.blinds.resize(B * 2);
            for (size_t b = 0; b < B; b++) {
                d.blinds[2 * b] = draw(b);
                d.blinds[2 * b + 1] = draw(b);
            }
            BZH_TRY(to_coeff(d.polys, d.as, B * 2));
            BZH_TRY(commit_columns(d.as, d.polys, B * 2, d.blinds, xy));
            for (int32_t rc : d.status)   // (device permutation) landed with the commitments; the first failed pair's status
                if (rc) return rc;
            for (size_t b = 0; b < B; b++) {
                bzh_transcript_write_point(T[b], C::id, &xy[(2 * b) * 8]);
                bzh_transcript_write_point(T[b], C::id, &xy[(2 * b + 1) * 8]);
            }
        }
        BZH_TRY(extend_witness());
        for (size_t b = 0; b < B; b++) {
            env[b][SY_BETA] = squeeze(b);
            env[b][SY_GAMMA] = squeeze(b);
        }
        return BZH_OK;
    }

    // numerator (zt) and denominator (den) of every grand product's factors, B x n each per product: permutation sets, then
    // lookups.  reads adv, inst, lk, env[SY_BETA], env[SY_GAMMA]
    int product_factors(uint32_t* den_all, uint32_t* zt_all) {
        for (int i = 0; i < nsets; i++) {
            const size_t c0 = (size_t)i * pk.chunk_len, c1 = std::min(m, c0 + pk.chunk_len);
            uint32_t *den = den_all + (size_t)i * B * n * 8, *zt = zt_all + (size_t)i * B * n * 8;
            Cols reg;
            for (size_t gj = c0; gj < c1; gj++) {
                lag_col(reg, pk.perm_columns[gj]);
                reg.add(key(K_SIGMA, gj), pk.sigma + gj * n * 8, 0);
                reg.add(key(K_IDENT, gj), pk.ident + gj * n * 8, 0);
            }
            for (int which = 0; which < 2; which++) {  // 0: denominator, 1: numerator
                BZH_TRY(run(key(30 + which, i), [&](EPool& ep) {
                    int acc = -1;
                    for (size_t gj = c0; gj < c1; gj++) {
                        const int v = ep.query(lag_col(reg, pk.perm_columns[gj]));
                        const int f = which == 0 ? ep.add(ep.add(ep.mul(ep.sym(SY_BETA), ep.query(reg.at(key(K_SIGMA, gj)))), ep.sym(SY_GAMMA)), v)
                                                 : ep.add(ep.add(ep.mul(ep.query(reg.at(key(K_IDENT, gj))), ep.sym(SY_BETA)), ep.sym(SY_GAMMA)), v);
                        acc = acc < 0 ? f : ep.mul(acc, f);
                    }
                    return acc;
                }, reg, n, which == 0 ? den : zt));
            }
            mark(" gp:perm_set");
        }
        for (int li = 0; li < nl; li++) {
            uint32_t *den = den_all + (size_t)(nsets + li) * B * n * 8, *zt = zt_all + (size_t)(nsets + li) * B * n * 8;
            Cols reg;
            reg.add(key(K_MISC, M_AC), lk[li].a_c, n);
            reg.add(key(K_MISC, M_SC), lk[li].s_c, n);
            reg.add(key(K_MISC, M_A), lk[li].as, 2 * n);
            reg.add(key(K_MISC, M_S), lk[li].as + n * 8, 2 * n);
            BZH_TRY(run(key(32, li), [&](EPool& ep) {
                return ep.mul(ep.add(ep.query(0), ep.sym(SY_BETA)), ep.add(ep.query(1), ep.sym(SY_GAMMA)));
            }, reg, n, zt));
            BZH_TRY(run(key(33, li), [&](EPool& ep) {
                return ep.mul(ep.add(ep.query(2), ep.sym(SY_BETA)), ep.add(ep.query(3), ep.sym(SY_GAMMA)));
            }, reg, n, den));
            mark(" gp:lookup_product");
        }
        return BZH_OK;
    }
    // one scanned product (zt, B x n) into its place in zs: chained to the previous permutation set's last value (prev_slot >= 0),
    // blinding rows, blind.  fills zs[slot], z_blinds[slot]
    int finish_product(int slot, int prev_slot, uint32_t* zt) {
        if (prev_slot >= 0)
            hipLaunchKernelGGL((k_scale_rows<SF>), dim3((unsigned)((n + 255) / 256), (unsigned)B), dim3(256), 0, st, zt, n,
                               zs + ((size_t)prev_slot * n + usable) * 8, (size_t)nz * n);
        BZH_TRY(blind_rows(zt, n - bf, bf, 1, n));
        for (size_t b = 0; b < B; b++) z_blinds[b * nz + slot] = draw(b);
        return copy2d(zs + (size_t)slot * n * 8, (size_t)nz * n, zt, n, n, B);
    }

    // 4. permutation and lookup grand products, and the lookup columns on the extended coset.
    // reads adv, inst, lk, env[SY_BETA], env[SY_GAMMA]; fills zs, z_polys, z_cosets, z_blinds, lk[].cosets
    int grand_products() {
        zs = dalloc(B * std::max(nz, 1) * n);
        z_polys = dalloc(B * std::max(nz, 1) * n);
        z_cosets = cosetwise ? nullptr : ext_alloc(B * std::max(nz, 1));
        // numerators and denominators of ALL grand products side by side, [product][proof][row]: one batch inversion, one
        // element-wise product and one scan for the lot (they were per product; the permutation sets are chained only through a
        // scalar carried from one set's last row into the next, applied afterwards)
        uint32_t* den_all = dalloc(B * std::max(nz, 1) * n);
        uint32_t* zt_all = dalloc(B * std::max(nz, 1) * n);
        if (!zs || !z_polys || (!z_cosets && !cosetwise) || !den_all || !zt_all) return BZH_E_OOM;
        z_blinds.resize(B * std::max(nz, 1));
        BZH_TRY(product_factors(den_all, zt_all));
        if (nz) {
            mark("  fp:exprs");
            BZH_TRY(poly_batch_invert(ctx, field, den_all, (size_t)nz * B * n));
            mark("  fp:invert");
            BZH_TRY(poly_vec_mul(ctx, field, zt_all, den_all, (size_t)nz * B * n));
            BZH_TRY(poly_prefix_product(ctx, field, zt_all, n, (size_t)nz * B));
            mark("  fp:mul+scan");
            // blinding rows and blinds in the order the products are made upstream: permutation sets, then lookups
            for (int i = 0; i < nsets; i++) BZH_TRY(finish_product(i, i ? i - 1 : -1, zt_all + (size_t)i * B * n * 8));
            for (int li = 0; li < nl; li++) BZH_TRY(finish_product(nsets + li, -1, zt_all + (size_t)(nsets + li) * B * n * 8));
            BZH_TRY(to_coeff(z_polys, zs, B * nz));
            std::vector<uint64_t> xy;
            BZH_TRY(commit_columns(zs, z_polys, B * nz, z_blinds, xy, (long)usable - 1));
            for (size_t b = 0; b < B; b++)
                for (int i = 0; i < nz; i++) bzh_transcript_write_point(T[b], C::id, &xy[(b * nz + i) * 8]);
            mark(" gp:commit");
            if (!cosetwise) BZH_TRY(to_extended(z_cosets, z_polys, B * nz));
            mark(" gp:extend_z");
        }
        if (cosetwise) return BZH_OK;
        for (auto& d : lk) {
            d.cosets = ext_alloc(B * 2);
            if (!d.cosets) return BZH_E_OOM;
            BZH_TRY(to_extended(d.cosets, d.polys, B * 2));
        }
        return BZH_OK;
    }

    // the quotient's values on the extended coset -> h (B x en).  reads the cosets of every column, env
    int quotient() {
        if (cosetwise) {
            CosetWork cw;
            std::vector<const uint32_t*> lk_p;
            for (int i = 0; i < nl; i++) lk_p.push_back(lk[i].polys);
            BZH_TRY(cosetwise_setup(adv_polys, inst_polys, z_polys, lk_p, 2, cw));
            std::vector<uint32_t> cv;
            BZH_TRY(fill_consts(pk.qprog.consts, B, 8, put_saturated, cv));
            ProgramArgs pa;
            BZH_TRY(quotient_args(cw.reg, cv.data(), cv.size() * 4, pa));
            return cosetwise_launch(cw, pa, h);
        }
        Cols reg;
        QuotientPtrs qp;
        qp.adv = adv_cosets, qp.inst = inst_cosets, qp.z = z_cosets;
        for (int i = 0; i < nl; i++) qp.lk.push_back(lk[i].cosets);
        quotient_registry(pk, qp, q29, reg);
        // VM v2 (gate-factored fold, shared subexpressions in LDS); the plain Horner fold through VM v1 if it does not fit
        int qrc = !q29 && getenv("BZH_QUOTIENT_V1") ? BZH_E_RANGE : run_quotient(reg, en, h);
        if (qrc == BZH_E_RANGE && !q29) {
            qrc = run(key(40, 0), [&](EPool& ep) {
                int tinv = -1;
                const std::vector<int> terms = quotient_terms<SF>(pk, reg, ep, &tinv);
                return ep.mul(ep.horner(terms, ep.sym(SY_Y)), tinv);
            }, reg, en, h);
        }
        return qrc;
    }

    // 5. the vanishing argument: random polynomial, y, the quotient and its pieces (with the degree flag), x.
    // reads every coset, env; fills random_poly, random_blinds, h, h_blinds, xs, omega_m, omega_inv, env[SY_Y.., SY_BD0.., SY_XN]
    int vanishing() {
        std::vector<uint64_t> xy;
        random_poly = dalloc(B * n);
        if (!random_poly) return BZH_E_OOM;
        BZH_TRY(draw_rows(n, random_poly));
        random_blinds.resize(B);
        for (size_t b = 0; b < B; b++) random_blinds[b] = draw(b);
        BZH_TRY(commit(pk.srs, random_poly, n, B, random_blinds, xy));
        Fe<SF> delta;
        memcpy(delta.l, pk.delta, 32);
        for (size_t b = 0; b < B; b++) {
            bzh_transcript_write_point(T[b], C::id, &xy[b * 8]);
            env[b][SY_Y] = squeeze(b);
            Fe<SF> yp = env[b][SY_Y];
            for (int mpow = 2; mpow <= 64; mpow++) {   // y^m for the gate-factored fold (m = constraints per gate)
                yp = fe_mul(yp, env[b][SY_Y]);
                env[b][SY_YPOW0 + mpow] = yp;
            }
            Fe<SF> bd = env[b][SY_BETA];
            for (size_t gj = 0; gj < m; gj++) {
                env[b][SY_BD0 + (int)gj] = bd;
                bd = fe_mul(bd, delta);
            }
        }
        mark("vanishing_setup");
        h = dalloc(B * en);
        if (!h) return BZH_E_OOM;
        BZH_TRY(quotient());
        BZH_TRY(ntt_run(ctx, field, h, pk.ek, B, pk.eomega, pk.zeta, 1, BZH_FORM_MONTGOMERY));
        uint32_t* d_flag = (uint32_t*)arena.alloc(256);
        if (!d_flag) return BZH_E_OOM;
        uint32_t h_flag = 0;
        if ((size_t)npieces * n < en) {
            BZH_HIP_TRY(ctx, hipMemsetAsync(d_flag, 0, 4, st));
            const size_t words = (en - (size_t)npieces * n) * 8;
            hipLaunchKernelGGL(k_any_nonzero, dim3((unsigned)((words + 255) / 256), (unsigned)B), dim3(256), 0, st,
                               h + (size_t)npieces * n * 8, words, en * 8, d_flag);
            BZH_TRY(d2h_async(ctx, &h_flag, d_flag, 4));  // lands at the commit's d2h_finish
        }
        h_blinds.resize(B * npieces);
        for (size_t b = 0; b < B; b++)
            for (int i = 0; i < npieces; i++) h_blinds[b * npieces + i] = draw(b);
        {
            // pieces of proof b: h[b][i*n .. (i+1)*n) -> (B * npieces) rows; piece rows are n apart inside a proof, proofs en apart
            uint32_t* pieces = dalloc(B * npieces * n);
            if (!pieces) return BZH_E_OOM;
            BZH_TRY(copy2d(pieces, (size_t)npieces * n, h, en, (size_t)npieces * n, B));
            BZH_TRY(commit(pk.srs, pieces, n, B * npieces, h_blinds, xy));
        }
        if (h_flag) {
            ctx->last_error = "quotient has higher degree than expected: a witness does not satisfy the constraints";
            return BZH_E_RANGE;
        }
        {
            uint64_t t[4];
            memcpy(t, pk.omega, 32);
            omega_m = fe_from_u64<SF>(t);
        }
        omega_inv = fe_inv(omega_m);
        xs.resize(B);
        for (size_t b = 0; b < B; b++) {
            for (int i = 0; i < npieces; i++) bzh_transcript_write_point(T[b], C::id, &xy[(b * npieces + i) * 8]);
            xs[b] = squeeze(b);
            env[b][SY_XN] = h_pow_u64(xs[b], n);
        }
        return BZH_OK;
    }

    // 6. evaluations: one gather of (polynomial, rotation) jobs, one evaluation launch, the values into the transcripts.
    // reads every *_polys, random_poly, xs; fills where (all but h(X): phase 7)
    int evaluations() {
        for (int i = 0; i < ni; i++) where[key(K_INST, i)] = {inst_polys + (size_t)i * n * 8, (size_t)ni * n};
        for (int i = 0; i < na; i++) where[key(K_ADV, i)] = {adv_polys + (size_t)i * n * 8, (size_t)na * n};
        for (int i = 0; i < nf; i++) where[key(K_FIX, i)] = {pk.fixed_polys + (size_t)i * n * 8, 0};
        for (size_t j = 0; j < m; j++) where[key(K_SIGMA, j)] = {pk.sigma_polys + j * n * 8, 0};
        where[key(K_MISC, M_F)] = {random_poly, n};
        for (int i = 0; i < nsets; i++) where[key(K_PZ, i)] = {z_polys + (size_t)i * n * 8, (size_t)nz * n};
        for (int i = 0; i < nl; i++) {
            where[key(K_LZ, i)] = {z_polys + (size_t)(nsets + i) * n * 8, (size_t)nz * n};
            where[key(K_LA, i)] = {lk[i].polys, 2 * n};
            where[key(K_LS, i)] = {lk[i].polys + n * 8, 2 * n};
        }
        const int last_rot = -(bf + 1);
        std::vector<std::pair<uint64_t, int>> jobs;
        for (auto& a : pk.instance_queries) jobs.push_back({key(K_INST, a.first), a.second});
        for (auto& a : pk.advice_queries) jobs.push_back({key(K_ADV, a.first), a.second});
        for (auto& a : pk.fixed_queries) jobs.push_back({key(K_FIX, a.first), a.second});
        jobs.push_back({key(K_MISC, M_F), 0});
        for (size_t j = 0; j < m; j++) jobs.push_back({key(K_SIGMA, j), 0});
        for (int i = 0; i < nsets; i++) {
            jobs.push_back({key(K_PZ, i), 0});
            jobs.push_back({key(K_PZ, i), 1});
            if (i != nsets - 1) jobs.push_back({key(K_PZ, i), last_rot});
        }
        for (int i = 0; i < nl; i++) {
            jobs.push_back({key(K_LZ, i), 0});
            jobs.push_back({key(K_LZ, i), 1});
            jobs.push_back({key(K_LA, i), 0});
            jobs.push_back({key(K_LA, i), -1});
            jobs.push_back({key(K_LS, i), 0});
        }
        const size_t J = jobs.size();
        std::vector<std::pair<const uint32_t*, size_t>> srcs(J);
        for (size_t j = 0; j < J; j++) srcs[j] = where.at(jobs[j].first);
        ArenaScope scope(arena);   // `gathered` is read by evals() (which ends in a stream sync) and by nothing else
        uint32_t* gathered = dalloc(B * J * n);
        if (!gathered) return BZH_E_OOM;
        BZH_TRY(gather(srcs, gathered));
        std::vector<Fe<SF>> pts(B * J), vals;
        for (size_t b = 0; b < B; b++)
            for (size_t j = 0; j < J; j++) pts[b * J + j] = rot(b, jobs[j].second);
        BZH_TRY(evals(gathered, B * J, pts, vals));
        for (size_t b = 0; b < B; b++)
            for (size_t j = 0; j < J; j++) write_scalar(b, vals[b * J + j]);
        return BZH_OK;
    }

    // 7. h(X) = sum_i x^(n i) h_i(X): Horner from the top piece.  reads h, h_blinds, env[SY_XN]; fills h_blind, where[M_H0]
    int h_poly() {
        uint32_t* hx = dalloc(B * n);
        if (!hx) return BZH_E_OOM;
        Cols reg;
        for (int i = 0; i < npieces; i++) reg.add(key(K_MISC, M_H0 + i), h + (size_t)i * n * 8, en);
        BZH_TRY(run(key(41, 0), [&](EPool& ep) {
            std::vector<int> t;
            for (int i = npieces - 1; i >= 0; i--) t.push_back(ep.query(i));
            return ep.horner(t, ep.sym(SY_XN));
        }, reg, n, hx));
        h_blind.resize(B);
        for (size_t b = 0; b < B; b++) {
            Fe<SF> acc = fe_zero<SF>();
            for (int i = npieces - 1; i >= 0; i--) acc = fe_add(fe_mul(acc, env[b][SY_XN]), h_blinds[b * npieces + i]);
            h_blind[b] = acc;
        }
        where[key(K_MISC, M_H0)] = {hx, n};
        return BZH_OK;
    }

    // the blind of committed polynomial `cid` of proof b.  reads every *_blinds
    Fe<SF> blind_of(size_t b, uint64_t cid) {
        const int kind = (int)(cid >> 32);
        const size_t i = (size_t)(cid & 0xffffffffu);
        switch (kind) {
            case K_ADV: return adv_blinds[b * na + i];
            case K_PZ: return z_blinds[b * nz + i];
            case K_LZ: return z_blinds[b * nz + nsets + i];
            case K_LA: return lk[i].blinds[2 * b];
            case K_LS: return lk[i].blinds[2 * b + 1];
            case K_MISC: return i == M_H0 ? h_blind[b] : random_blinds[b];
            default: return fe_one<SF>();  // instance, fixed, sigma
        }
    }
    // multiopen, first part: x1, x2 and per point set si the polynomial q_si = Horner in x1 over the set's polynomials, with its
    // blind.  reads where, every *_blinds; fills q_polys (B x nq x n), q_blinds, env[SY_X1], env[SY_X2]
    int open_q_polys(uint32_t*& q_polys, std::vector<Fe<SF>>& q_blinds) {
        for (size_t b = 0; b < B; b++) {
            env[b][SY_X1] = squeeze(b);
            env[b][SY_X2] = squeeze(b);
        }
        const size_t nq = pk.rot_sets.size();
        q_polys = dalloc(B * nq * n);
        uint32_t* acc_a = dalloc(B * n);
        uint32_t* acc_b = dalloc(B * n);
        if (!q_polys || !acc_a || !acc_b) return BZH_E_OOM;
        q_blinds.resize(B * nq);
        for (size_t si = 0; si < nq; si++) {
            const std::vector<uint64_t>& cids = pk.groups[si];
            for (size_t b = 0; b < B; b++) {
                Fe<SF> acc = fe_zero<SF>();
                for (uint64_t cid : cids) acc = fe_add(fe_mul(acc, env[b][SY_X1]), blind_of(b, cid));
                q_blinds[b * nq + si] = acc;
            }
            // Horner in x1 over the group's polynomials, in chunks that fit the evaluator's slot file
            uint32_t* prev = nullptr;
            for (size_t s0 = 0; s0 < cids.size(); s0 += 16) {
                const size_t s1 = std::min(cids.size(), s0 + 16);
                Cols reg;
                if (prev) reg.add(key(K_MISC, M_ACC), prev, n);
                for (size_t c = s0; c < s1; c++) {
                    const auto& w = where.at(cids[c]);
                    reg.add(cids[c], w.first, w.second);
                }
                uint32_t* outp = prev == acc_a ? acc_b : acc_a;
                BZH_TRY(run(key(50 + si, s0), [&](EPool& ep) {
                    std::vector<int> t;
                    for (size_t c = 0; c < reg.ptr.size(); c++) t.push_back(ep.query((int)c));
                    return ep.horner(t, ep.sym(SY_X1));
                }, reg, n, outp));
                prev = outp;
            }
            BZH_TRY(copy2d(q_polys + si * n * 8, nq * n, prev, n, n, B));
        }
        return BZH_OK;
    }

    // multiopen, second part: the q polynomials at their own points and the remainders r_si(X) through (points, evaluations),
    // np coefficients each at r_small[(b * nq + si) * maxpts ..].  reads q_polys, xs
    int open_remainders(const uint32_t* q_polys, size_t maxpts, std::vector<Fe<SF>>& r_small) {
        const size_t nq = pk.rot_sets.size();
        std::vector<std::pair<size_t, int>> ev_jobs;
        for (size_t si = 0; si < nq; si++)
            for (int r : pk.rot_sets[si]) ev_jobs.push_back({si, r});
        const size_t J2 = ev_jobs.size();
        std::vector<std::pair<const uint32_t*, size_t>> srcs(J2);
        for (size_t j = 0; j < J2; j++) srcs[j] = {q_polys + ev_jobs[j].first * n * 8, nq * n};
        std::vector<Fe<SF>> pts(B * J2), ev;
        for (size_t b = 0; b < B; b++)
            for (size_t j = 0; j < J2; j++) pts[b * J2 + j] = rot(b, ev_jobs[j].second);
        {
            ArenaScope scope(arena);   // `gathered` lives until evals() returns (stream sync)
            uint32_t* gathered = dalloc(B * J2 * n);
            if (!gathered) return BZH_E_OOM;
            BZH_TRY(gather(srcs, gathered));
            BZH_TRY(evals(gathered, B * J2, pts, ev));
        }
        r_small.assign(B * nq * maxpts, fe_zero<SF>());
        // Lagrange interpolation through (points, evals) per proof and point set: the denominators prod_(m != j) (x_j - x_m) of
        // the whole batch are inverted together (one field inversion per batch instead of one per point: ~12 us each on the host)
        std::vector<Fe<SF>> dinv(B * J2);
        for (size_t b = 0; b < B; b++) {
            size_t o2 = 0;
            for (size_t si = 0; si < nq; si++) {
                const size_t np = pk.rot_sets[si].size();
                for (size_t j = 0; j < np; j++) {
                    Fe<SF> dn = fe_one<SF>();
                    for (size_t mm = 0; mm < np; mm++)
                        if (mm != j) dn = fe_mul(dn, fe_sub(pts[b * J2 + o2 + j], pts[b * J2 + o2 + mm]));
                    dinv[b * J2 + o2 + j] = dn;
                }
                o2 += np;
            }
        }
        if (!h_batch_invert(dinv.data(), dinv.size())) return BZH_E_ARG;   // two opening points of one set coincide: not a valid domain
        for (size_t b = 0; b < B; b++) {
            size_t o2 = 0;
            for (size_t si = 0; si < nq; si++) {
                const size_t np = pk.rot_sets[si].size();
                h_interpolate(&pts[b * J2 + o2], &ev[b * J2 + o2], &dinv[b * J2 + o2], np, &r_small[(b * nq + si) * maxpts]);
                o2 += np;
            }
        }
        return BZH_OK;
    }

    // multiopen, third part: f_si = (q_si - r_si) / prod_(r in set si) (X - x w^r): one division per point, chained within a set,
    // independent between sets.  The sets are ordered by the number of their points (most first) and step t divides every set that
    // still has a t-th point in ONE launch: all of them hold n - t coefficients at that step and they are a prefix of the order,
    // so the vectors [position][proof] stay densely packed from step to step.  (Was one launch chain per set: 16 divisions -> 4.)
    // reads q_polys, r_small, xs; fills f_parts (B x nq x n)
    int open_quotients(const uint32_t* q_polys, size_t maxpts, const std::vector<Fe<SF>>& r_small, uint32_t*& f_parts) {
        const size_t nq = pk.rot_sets.size();
        uint32_t* rcols = dalloc(B * nq * n);
        uint32_t* rs_dev = dalloc(B * nq * maxpts);
        f_parts = dalloc(B * nq * n);
        uint32_t* k_a = dalloc(B * nq * n);
        uint32_t* k_b = dalloc(B * nq * n);
        if (!rcols || !rs_dev || !f_parts || !k_a || !k_b) return BZH_E_OOM;
        BZH_TRY(zero(rcols, B * nq * n));
        BZH_TRY(zero(f_parts, B * nq * n));
        BZH_TRY(upload(rs_dev, r_small.data(), r_small.size()));
        BZH_TRY(copy2d(rcols, n, rs_dev, maxpts, maxpts, B * nq));
        std::vector<size_t> order(nq);
        for (size_t si = 0; si < nq; si++) order[si] = si;
        std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return pk.rot_sets[x].size() > pk.rot_sets[y].size(); });
        const size_t steps = nq ? pk.rot_sets[order[0]].size() : 0;
        size_t nkate = 0;
        for (size_t si = 0; si < nq; si++) nkate += pk.rot_sets[si].size();
        uint32_t* d_xall = dalloc(std::max<size_t>(nkate, 1) * B);
        if (!d_xall) return BZH_E_OOM;
        {   // the opening points, [step][position][proof], in one upload
            std::vector<Fe<SF>> xv(nkate * B);
            size_t at = 0;
            for (size_t t = 0; t < steps; t++)
                for (size_t pos = 0; pos < nq && pk.rot_sets[order[pos]].size() > t; pos++)
                    for (size_t b = 0; b < B; b++) xv[at++] = rot(b, pk.rot_sets[order[pos]][t]);
            BZH_TRY(upload(d_xall, xv.data(), xv.size()));
        }
        for (size_t pos = 0; pos < nq; pos++) {
            const size_t si = order[pos];
            Cols reg;
            reg.add(key(K_MISC, M_Q), q_polys + si * n * 8, nq * n);
            reg.add(key(K_MISC, M_R), rcols + si * n * 8, nq * n);
            BZH_TRY(run(key(42, 0), [&](EPool& ep) { return ep.sub(ep.query(0), ep.query(1)); }, reg, n, k_a + pos * B * n * 8));
        }
        uint32_t* cur = k_a;
        uint32_t* nxt = k_b;
        size_t len = n, x_at = 0;
        for (size_t t = 0; t < steps; t++) {
            size_t active = 0;
            while (active < nq && pk.rot_sets[order[active]].size() > t) active++;
            BZH_TRY(poly_kate_division(ctx, field, cur, len, active * B, d_xall + x_at * 8, nxt));
            x_at += active * B;
            std::swap(cur, nxt);
            len--;
            for (size_t pos = 0; pos < active; pos++)   // the sets whose last point this was
                if (pk.rot_sets[order[pos]].size() == t + 1)
                    BZH_TRY(copy2d(f_parts + order[pos] * n * 8, nq * n, cur + pos * B * len * 8, len, len, B));
        }
        for (size_t pos = 0; pos < nq; pos++)   // a set without points (not produced by the key builder): q - r itself
            if (pk.rot_sets[order[pos]].empty()) BZH_TRY(copy2d(f_parts + order[pos] * n * 8, nq * n, k_a + pos * B * n * 8, n, n, B));
        return BZH_OK;
    }

    // multiopen, last part: f = sum_si x2^(..) f_si (Horner), its commitment, x3, the q evaluations at x3, x4, and the opened
    // polynomial p = Horner in x4 over (f, q_0, ..).  reads q_polys, q_blinds, f_parts; fills p_poly, p_blinds, x3c, env[SY_X4]
    int open_final_poly(const uint32_t* q_polys, const std::vector<Fe<SF>>& q_blinds, const uint32_t* f_parts) {
        const size_t nq = pk.rot_sets.size();
        uint32_t* f_poly = dalloc(B * n);
        p_poly = dalloc(B * n);
        if (!f_poly || !p_poly) return BZH_E_OOM;
        if (nq == 1) {
            BZH_TRY(copy2d(f_poly, n, f_parts, n, n, B));
        } else {
            Cols reg;
            for (size_t si = 0; si < nq; si++) reg.add(key(K_MISC, M_H0 + si), f_parts + si * n * 8, nq * n);
            BZH_TRY(run(key(43, 0), [&](EPool& ep) {
                std::vector<int> t;
                for (size_t si = 0; si < nq; si++) t.push_back(ep.query((int)si));
                return ep.horner(t, ep.sym(SY_X2));
            }, reg, n, f_poly));
        }
        std::vector<Fe<SF>> f_blinds(B), x3s(B);
        for (size_t b = 0; b < B; b++) f_blinds[b] = draw(b);
        std::vector<uint64_t> xy;
        BZH_TRY(commit(pk.srs, f_poly, n, B, f_blinds, xy));
        for (size_t b = 0; b < B; b++) {
            bzh_transcript_write_point(T[b], C::id, &xy[b * 8]);
            x3s[b] = squeeze(b);
        }
        std::vector<Fe<SF>> p3(B * nq), v3;
        for (size_t b = 0; b < B; b++)
            for (size_t si = 0; si < nq; si++) p3[b * nq + si] = x3s[b];
        BZH_TRY(evals(q_polys, B * nq, p3, v3));
        for (size_t b = 0; b < B; b++) {
            for (size_t si = 0; si < nq; si++) write_scalar(b, v3[b * nq + si]);
            env[b][SY_X4] = squeeze(b);
        }
        {
            Cols reg;
            reg.add(key(K_MISC, M_F), f_poly, n);
            for (size_t si = 0; si < nq; si++) reg.add(key(K_MISC, M_H0 + si), q_polys + si * n * 8, nq * n);
            BZH_TRY(run(key(44, 0), [&](EPool& ep) {
                std::vector<int> t;
                for (size_t c = 0; c <= nq; c++) t.push_back(ep.query((int)c));
                return ep.horner(t, ep.sym(SY_X4));
            }, reg, n, p_poly));
        }
        p_blinds.resize(B * 4);
        x3c.resize(B * 4);
        for (size_t b = 0; b < B; b++) {
            Fe<SF> acc = f_blinds[b];
            for (size_t si = 0; si < nq; si++) acc = fe_add(fe_mul(acc, env[b][SY_X4]), q_blinds[b * nq + si]);
            fe_to_u64<SF>(&p_blinds[4 * b], fe_from_mont(acc));
            fe_to_u64<SF>(&x3c[4 * b], fe_from_mont(x3s[b]));
        }
        return BZH_OK;
    }

    // 8. multiopen: every opening of the proof folded into one polynomial and one point per proof.
    // reads where, every *_blinds, xs; fills p_poly, p_blinds, x3c
    int multiopen() {
        uint32_t *q_polys = nullptr, *f_parts = nullptr;
        std::vector<Fe<SF>> q_blinds, r_small;
        BZH_TRY(open_q_polys(q_polys, q_blinds));
        size_t maxpts = 1;
        for (auto& rs : pk.rot_sets) maxpts = std::max(maxpts, rs.size());
        BZH_TRY(open_remainders(q_polys, maxpts, r_small));
        BZH_TRY(open_quotients(q_polys, maxpts, r_small, f_parts));
        mark("multiopen_q_kate");
        BZH_TRY(open_final_poly(q_polys, q_blinds, f_parts));
        mark("multiopen_f_p");
        return BZH_OK;
    }

    // 9. the inner-product argument on p at x3.  reads p_poly, p_blinds, x3c; writes the rest of every transcript
    int open() {
        // the opening draws from each proof's own cursor: a zero stride is not possible, so pass proof 0's cursor and the
        // common distance between the per-proof streams
        const size_t need = 64 * (n + 1 + 2 * (size_t)pk.k);
        std::vector<uint64_t> out_v(B * 4);
        if (seeded) {
            uint32_t* raw = (uint32_t*)arena.alloc(B * need);
            if (!raw) return BZH_E_OOM;
            BZH_TRY(seed_rows(need / 64, raw));
            return ipa_open(ctx, pk.srs, p_poly, B, p_blinds.data(), x3c.data(), nullptr, need, T.data(), out_v.data(), raw);
        }
        std::vector<uint8_t> ipa_rng(B * need);
        for (size_t b = 0; b < B; b++) memcpy(&ipa_rng[b * need], rng[b], need);
        return ipa_open(ctx, pk.srs, p_poly, B, p_blinds.data(), x3c.data(), ipa_rng.data(), need, T.data(), out_v.data());
    }

    // create_proof for the batch: the phases in protocol order, a trace mark after each
    int prove(const uint32_t* d_advice_in, const uint64_t* instances, size_t inst_rows, uint8_t* proofs, size_t proof_stride,
              size_t* proof_lens) {
        BZH_TRY(begin_transcripts());
        mark("setup");
        BZH_TRY(commit_instances(instances, inst_rows));
        mark("instance");
        BZH_TRY(commit_advice(d_advice_in));
        mark("advice");
        BZH_TRY(lookups());
        mark("lookup");
        BZH_TRY(grand_products());
        mark("grand_products");
        BZH_TRY(vanishing());
        mark("quotient+h_commit");
        BZH_TRY(evaluations());
        mark("evaluations");
        BZH_TRY(h_poly());
        mark("h_poly");
        BZH_TRY(multiopen());
        BZH_TRY(open());
        mark("ipa");
        for (size_t b = 0; b < B; b++) {
            const uint8_t* data = nullptr;
            size_t plen = 0;
            BZH_TRY(bzh_transcript_proof(T[b], &data, &plen));
            if (plen > proof_stride) return BZH_E_ARG;
            memcpy(proofs + b * proof_stride, data, plen);
            proof_lens[b] = plen;
        }
        return BZH_OK;
    }
};

template <class C>
static int prove_batch_t(bzh_ctx* ctx, bzh_pk* pk, size_t batch, const uint32_t* d_advice, const uint64_t* instances, size_t inst_rows,
                         const uint8_t* rng, size_t rng_stride, uint8_t* proofs, size_t proof_stride, size_t* proof_lens) {
    Arena& arena = pk->rt.arena_for(ctx->serial, ctx->device);
    arena.reset();
    Prover<C> pv(ctx, *pk, batch, arena);
    if (rng_stride == 0) {  // seeded: rng holds batch x 32 bytes
        pv.seeded = true;
        pv.seed_keys.resize(batch * 8);
        memcpy(pv.seed_keys.data(), rng, batch * 32);
        pv.host_ctr.assign(batch, 0);
        pv.d_seed_keys = (uint32_t*)arena.alloc(batch * 32);
        if (!pv.d_seed_keys) return BZH_E_OOM;
        int rcu = h2d_small(ctx, pv.d_seed_keys, pv.seed_keys.data(), batch * 32);
        if (rcu) return rcu;
    } else {
        for (size_t b = 0; b < batch; b++) pv.rng[b] = rng + b * rng_stride;
    }
    const int rc = pv.prove(d_advice, instances, inst_rows, proofs, proof_stride, proof_lens);
    (void)hipStreamSynchronize(ctx->stream);
    // a phase that failed between a d2h_async and its d2h_finish leaves read-backs whose destinations die with `pv`: they must
    // not land at the next call's d2h_finish
    if (rc) ctx->pending_d2h.clear();
    return rc;
}
