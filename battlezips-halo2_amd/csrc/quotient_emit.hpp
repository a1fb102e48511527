// Part of the whole-proof translation unit (csrc/prove.hip): a compiled VM v2 program (csrc/quotient_compiler.hpp) as straight-line
// HIP source, in saturated limbs (program2_source) and in unsaturated 29-bit limbs (program2_source29).  KernelText is what the two
// print alike -- the frame of the file, the kernel's prologue, the walk over the instructions -- and nothing of their arithmetic.
// Host code only.  Included inside namespace bzh { namespace { (prove_kernels.cuh opens them).
#pragma once
struct KernelText {
    std::string src;
    char buf[640];
    template <class... A>
    void add(const char* fmt, A... a) {
        snprintf(buf, sizeof(buf), fmt, a...);
        src += buf;
    }
    // ns: the builtin flavours live in a namespace named after the program hash; null: a module of the caller's own
    void open(const char* ns, unsigned long long hash, int field) {
        if (ns) add("namespace %s_%016llx {\n", ns, hash);
        else src += "#include \"field.cuh\"\n";
        src += "using namespace bzh;\n";
        add("typedef %s P;\n", field == BZH_FIELD_FQ ? "FqParams" : "FpParams");
    }
    // one thread per row, one grid row per proof; the evaluation stack r0..r3 and the slot file are local values of type `vtype`,
    // a proof's constants `pitch` words apart
    void prologue(const char* kname, const char* vtype, const char* zero, int pitch, int nslots) {
        add("extern \"C\" __global__ void __launch_bounds__(128) %s(const uint32_t* const* __restrict__ cols, ", kname);
        src += "const size_t* __restrict__ strides, const uint32_t* __restrict__ consts, size_t const_stride, size_t size, "
               "uint32_t* __restrict__ out) {\n"
               "    const size_t r = blockIdx.x * (size_t)128 + threadIdx.x, v = blockIdx.y;\n"
               "    if (r >= size) return;\n"
               "    const size_t mask = size - 1;\n";
        add("    const uint32_t* cv = consts + v * const_stride * %d;\n", pitch);
        add("    %s r0 = %s(), r1 = r0, r2 = r0, r3 = r0;\n", vtype, zero);
        for (int i = 0; i < nslots; i++) add("    %s s%d = r0;\n", vtype, i);
    }
    // Every memory operand is loaded one instruction ahead of its use and a scheduling barrier follows every instruction:
    // load(name, i, kind, idx, rot) prints the load of operand `name` of instruction i, body(i, op) the instruction itself;
    // skip(i): the instruction is not printed (the unsaturated emitter's fused products)
    template <class Skip, class Load, class Body>
    void walk(const Program2& pg, Skip skip, Load load, Body body) {
        const size_t nops = pg.ops.size();
        auto loads = [&](size_t i) {
            if (i >= nops || skip(i)) return;
            const ExprOp2& o = pg.ops[i];
            if (o.reads_a()) load("la", i, o.a_kind, o.a_idx, o.a_rot);
            if (o.reads_b()) load("lb", i, o.b_kind, o.b_idx, o.b_rot);
        };
        loads(0);
        for (size_t i = 0; i < nops; i++) {
            loads(i + 1);
            if (skip(i)) continue;
            body(i, pg.ops[i]);
            src += "    __builtin_amdgcn_sched_barrier(0);\n";
        }
    }
    // the builtin flavours' host launcher, and the end of their namespace
    void close(const char* ns, unsigned long long hash, const char* kname) {
        add("static void launch(unsigned gx, unsigned gy, void* st, const uint32_t* const* cols, const size_t* strides, const uint32_t* consts, "
            "size_t nc, size_t size, uint32_t* out) {\n    hipLaunchKernelGGL(%s, dim3(gx, gy), dim3(128), 0, (hipStream_t)st, cols, strides, consts, nc, size, out);\n}\n", kname);
        add("}  // namespace %s_%016llx\n", ns, hash);
    }
    // the kernel's name for an operand: the value loaded ahead for instruction i, or the slot
    static std::string operand(const char* name, size_t i, int kind, int idx) {
        char t[32];
        if (kind == BZH_EXPR_COLUMN || kind == BZH_EXPR_CONST) snprintf(t, sizeof(t), "%s%zu", name, i);
        else snprintf(t, sizeof(t), "s%d", idx);
        return t;
    }
};
static const char* const kV2RegNames[4] = {"r0", "r1", "r2", "r3"};

// The VM v2 program as straight-line HIP source (compiled by the caller with hipcc / hiprtc against csrc/field.cuh and handed
// back through bzh_pk_set_quotient_module).  The evaluation stack r0..r3 and the slot file become local values; every memory
// operand is loaded one instruction ahead of its use and a scheduling barrier follows every instruction -- without it the
// compiler hoists all ~750 leaf loads to the top (255 VGPRs and scratch); with it 106 VGPRs, four waves per SIMD.  Measured
// on the BoardCircuit program (1 361 instructions, 16 x 2^17 rows): 9.0 ms against the interpreter's 12.5 ms, same bits.
// builtin != 0: the flavour linked into libbzh2.so at build time (csrc/gen_quotient.cpp -> quotient_builtin.hip): kernel named
// after the program hash inside its own namespace, a host launcher, no module-level hash symbol.
static std::string program2_source(const Program2& pg, int field, bool builtin = false) {
    KernelText kt;
    std::string& src = kt.src;
    auto add = [&](const char* fmt, auto... a) { kt.add(fmt, a...); };
    const unsigned long long hash = (unsigned long long)program2_hash(pg, field);
    char kname[64];
    if (builtin) snprintf(kname, sizeof(kname), "bzh_quotient_%016llx", hash);
    else snprintf(kname, sizeof(kname), "jit_quotient");
    add("// generated by libbzh2 (%s): quotient evaluator, %zu instructions\n", builtin ? "bzh_quotient_source_for_circuit" : "bzh_pk_quotient_source",
        pg.ops.size());
    kt.open(builtin ? "bzh_q" : nullptr, hash, field);
    if (!builtin) add("extern \"C\" __device__ __attribute__((used)) unsigned long long jit_program_hash = 0x%llxull;\n", hash);
    // measured alternatives, all slower: the multiplication inlined (492 vs 514 proofs/s), barriers after multiplications only
    // (498), 0 / 4 / 6 shared-subexpression slots instead of 2 (478 / 503 / 505)
    src += "__device__ __noinline__ Fe<P> mulx(const Fe<P> a, const Fe<P> b) { return fe_mul(a, b); }\n";
    kt.prologue(kname, "Fe<P>", "fe_zero<P>", 8, std::max(pg.nlds, 1));
    auto emit_load = [&](const char* name, size_t i, int kind, int idx, int rot) {
        if (kind == BZH_EXPR_COLUMN)
            add("    const Fe<P> %s%zu = fe_load<P>(cols[%d] + (v * strides[%d] + ((r + (size_t)(long)(%d)) & mask)) * 8);\n", name, i, idx, idx, rot);
        else if (kind == BZH_EXPR_CONST)
            add("    const Fe<P> %s%zu = fe_load<P>(cv + %d * 8);\n", name, i, idx);
    };
    auto operand = KernelText::operand;
    auto arith = [&](int op, const std::string& a, const std::string& b) -> std::string {
        switch (op) {
            case V2_ADD: return "fe_add(" + a + ", " + b + ")";
            case V2_SUB: return "fe_sub(" + a + ", " + b + ")";
            case V2_MUL: return "mulx(" + a + ", " + b + ")";
            default: return "fe_sub(" + b + ", " + a + ")";   // RSUB: b - a
        }
    };
    const char* const* regs = kV2RegNames;
    kt.walk(pg, [](size_t) { return false; }, emit_load, [&](size_t i, const ExprOp2& o) {
        const int form = o.form(), op = o.op(), pos = o.pos();
        const std::string ra = regs[pos];
        if (form == V2_SS) {
            src += "    " + ra + " = " + arith(op, ra, regs[(pos + 1) & 3]) + ";\n";
        } else if (form == V2_SL) {
            src += "    " + ra + " = " + arith(op, ra, operand("lb", i, o.b_kind, o.b_idx)) + ";\n";
        } else if (form == V2_LL) {
            src += "    " + ra + " = " + arith(op, operand("la", i, o.a_kind, o.a_idx), operand("lb", i, o.b_kind, o.b_idx)) + ";\n";
        } else if (op == V2_NEG) {
            src += "    " + ra + " = fe_neg(" + ra + ");\n";
        } else if (op == V2_LOAD) {
            src += "    " + ra + " = " + operand("la", i, o.a_kind, o.a_idx) + ";\n";
        } else {
            add("    s%d = %s;\n", o.a_idx, ra.c_str());
        }
    });
    src += "    fe_store(out + (v * size + r) * 8, r0);\n}\n";
    if (builtin) kt.close("bzh_q", hash, kname);
    return src;
}

// The same program over UNSATURATED limbs (csrc/fe29.cuh): values are 9 x 29-bit limbs in R' = 2^261 Montgomery form, not kept
// canonical.  For every value the emitter tracks, while it writes the straight-line code, a bound V in multiples of p and bounds
// L, T on the limbs 0..7 and on limb 8:
//   leaves / constants  carried, V = 2;   a product  V = 2, limbs < 2^29;
//   a + b   limb-wise, NO carry pass (V, L, T add);   a - b   a + K p - b limb-wise, no carry pass either (fe29_sub_lazy: K p written
//   as J copies of (K / J) p so that it dominates b limb by limb; V grows by K, L by J 1.5 2^30);
//   a carry pass (fe29_carry, ~25 instructions) only where a consumer needs it: a product whose operands' limb bounds multiply past
//   1.8e18 (a column of the schoolbook product is 9 such terms + 4 reduction terms of 2^58 in one 64-bit accumulator), a sum or
//   difference that would pass 2^32, a subtrahend above 2 (2^30 - 2), a value parked in a shared-subexpression slot;
//   a fold below 2 p (fe29_fold, ~45 instructions) where bounds would multiply past 100 or add past 100 (the limbs hold 128 p).
// Board: 598 carry passes (one per + and -, the first version) -> 234.  A bound the emitter cannot establish fails the generation
// (empty source), never the arithmetic.  Columns are fe29 planes (fe29_load_planes), constants 12 words apart; the result is
// converted back to the saturated form by fe29_to_sat_div32 as it is stored, so h is what the saturated kernel writes, bit for bit.
static std::string program2_source29_policy(const Program2& pg, int field, bool carry_at_store, int* passes) {
    KernelText kt;
    std::string& src = kt.src;
    int npass = 0;          // carry passes + folds emitted (what the two store policies are compared by)
    bool pg_fail = false;   // a bound the emitter could not establish: no source (the saturated kernel is then the only flavour)
    auto add = [&](const char* fmt, auto... a) { kt.add(fmt, a...); };
    const unsigned long long hash = (unsigned long long)program2_hash(pg, field);
    char kname[64];
    snprintf(kname, sizeof(kname), "bzh_quotient29_%016llx", hash);
    add("// generated by libbzh2 (bzh_quotient_source_for_circuit): quotient evaluator in unsaturated limbs, %zu instructions\n", pg.ops.size());
    kt.open("bzh_q29", hash, field);
    // (out of line like the saturated flavour's, for the instruction cache; operands as 9-lane vectors: a 36-byte struct would
    // cross the call through scratch memory)
    src += "__device__ __noinline__ fe29_vec mulv(fe29_vec a, fe29_vec b) { return fe29_pack_vec(fe29_mul(fe29_unpack_vec<P>(a), fe29_unpack_vec<P>(b))); }\n"
           "__device__ __forceinline__ Fe29<P> mulx(const Fe29<P>& a, const Fe29<P>& b) { return fe29_unpack_vec<P>(mulv(fe29_pack_vec(a), fe29_pack_vec(b))); }\n"
           // a b + c d with ONE reduction; d is a per-proof constant the callee fetches itself (four 9-lane operands would not fit the
           // 32 argument registers), first thing, so that the a b multiply-adds cover the load
           "__device__ __noinline__ fe29_vec dot2v(fe29_vec a, fe29_vec b, fe29_vec c, fe29_gbytes d) {\n"
           "    const Fe29<P> dd = fe29_load_const_g<P>(d);\n"
           "    return fe29_pack_vec(fe29_dot2(fe29_unpack_vec<P>(a), fe29_unpack_vec<P>(b), fe29_unpack_vec<P>(c), dd));\n}\n"
           "__device__ __forceinline__ Fe29<P> dot2x(const Fe29<P>& a, const Fe29<P>& b, const Fe29<P>& c, const uint32_t* d) {\n"
           "    return fe29_unpack_vec<P>(dot2v(fe29_pack_vec(a), fe29_pack_vec(b), fe29_pack_vec(c), (fe29_gbytes)d));\n}\n";
    // (132 VGPRs, three waves per SIMD: forcing four with amdgpu_waves_per_eu(4, 4) -- 128 VGPRs, 3 spilled -- measured slower,
    // 34.2 against 33.4 ms per batch of 64)
    // A scheduling barrier after every operation keeps the compiler from hoisting the column loads of the whole program to its top.
    // Without them (and the kernel capped at three waves' registers) LLVM merges the program's repeated products (mulv is pure:
    // Board 565 -> 426 calls) but spills ~1 900 words per row to scratch -- measured 30.2 vs 31.1 ms for Board and ShotCircuit's
    // throughput -4 %.
    const int nslots = std::max(pg.nlds, 1);
    kt.prologue(kname, "Fe29<P>", "fe29_zero<P>", 12, nslots);
    // what is known about a value: V (its bound in multiples of p), L (limbs 0..7 at most L), T (limb 8 at most T)
    struct Bnd {
        double V;
        uint64_t L, T;
    };
    // carry passes only where a consumer needs one (a carry pass after every + and - was measured: 598 against 115 passes per row
    // for Board, 33.8 against 32.4 ms)
    constexpr uint64_t kCarried = ((uint64_t)1 << 29) + 8;                          // fe29_carry's output: limbs 0..7 below this
    constexpr uint64_t kBiasLimb = ((uint64_t)1 << 30) + ((uint64_t)1 << 29);       // a limb of a bias K p stays below this
    constexpr double kColumn = 1.8e18;                                              // A * B of a product's limb bounds (header)
    const Bnd zero{0.0, 0, 0}, leaf{2.0, kCarried, ((uint64_t)1 << 23) + 16}, product{2.0, ((uint64_t)1 << 29) - 1, (uint64_t)1 << 23};   // (a product is below 1.8 p: limb 8 < 2^23)
    std::vector<Bnd> bs((size_t)nslots, zero);
    Bnd br[4] = {zero, zero, zero, zero};
    const size_t nops = pg.ops.size();
    auto emit_load = [&](const char* name, size_t i, int kind, int idx, int rot) {
        if (kind == BZH_EXPR_COLUMN)
            add("    const Fe29<P> %s%zu = fe29_load_planes_g<P>((fe29_gbytes)(cols[%d] + v * strides[%d]), (uint32_t)((r + (size_t)(long)(%d)) & mask), size);\n", name, i, idx, idx, rot);
        else if (kind == BZH_EXPR_CONST)
            add("    const Fe29<P> %s%zu = fe29_load_const<P>(cv + %d * 12);\n", name, i, idx);
    };
    // ---- fused pairs: X = (product) ; Y = slot * constant ; X + Y  ->  one dot2 with one reduction.  Two shapes come out of
    //      Compiler2::quotient: [rP = a * b] [rP+1 = ACC * y^m] [rP += rP+1] (adjacent), and Horner's [rP = IN * y] ... [rP+1 = a * b]
    //      [rP += rP+1] (the first product is deferred to the second: its operands are a slot nothing stores to in between and a constant).
    //      Measured against the two products apart: Board 283 instead of 386 instructions per pair, 26.7 -> 25.3 ms per batch of 64.
    struct Fuse {
        int slot = -1, cst = -1, dst = -1;   // at the surviving product: the other product's slot and constant, the register that gets the sum
    };
    std::vector<Fuse> fuse(nops);
    std::vector<char> skip(nops, 0);
    {
        auto fm = [&](size_t i) { return pg.ops[i].form(); };
        auto opc = [&](size_t i) { return pg.ops[i].op(); };
        auto ps = [&](size_t i) { return pg.ops[i].pos(); };
        auto is_mul = [&](size_t i) { return pg.ops[i].is_mul(); };
        auto slot_times_const = [&](size_t i) {
            return is_mul(i) && fm(i) == V2_LL && pg.ops[i].a_kind == BZH_EXPR_LDS && pg.ops[i].b_kind == BZH_EXPR_CONST;
        };
        auto reads = [&](size_t i, int p) {
            if (fm(i) == V2_SS) return ps(i) == p || ps(i) + 1 == p;
            if (fm(i) == V2_SL) return ps(i) == p;
            if (fm(i) == V2_UN) return opc(i) != V2_LOAD && ps(i) == p;
            return false;
        };
        auto writes = [&](size_t i, int p) { return !pg.ops[i].is_store() && ps(i) == p; };
        for (size_t k = 2; k < nops; k++) {
            if (!(fm(k) == V2_SS && opc(k) == V2_ADD) || skip[k]) continue;
            const int P = ps(k);
            if (skip[k - 1] || skip[k - 2] || fuse[k - 1].dst >= 0 || fuse[k - 2].dst >= 0) continue;
            if (slot_times_const(k - 1) && ps(k - 1) == P + 1 && is_mul(k - 2) && ps(k - 2) == P) {   // adjacent
                fuse[k - 2] = Fuse{pg.ops[k - 1].a_idx, pg.ops[k - 1].b_idx, P};
                skip[k - 1] = skip[k] = 1;
                continue;
            }
            if (!(is_mul(k - 1) && ps(k - 1) == P + 1)) continue;
            size_t j = k - 1;
            bool ok = false;
            while (j-- > 0) {   // the last writer of rP before the second product
                if (writes(j, P)) {
                    ok = slot_times_const(j) && !skip[j] && fuse[j].dst < 0;
                    break;
                }
                if (reads(j, P)) break;
            }
            if (!ok) continue;
            for (size_t x = j + 1; x < k && ok; x++)   // its slot operand must still hold the same value
                ok = !(pg.ops[x].is_store() && pg.ops[x].a_idx == pg.ops[j].a_idx);
            if (!ok) continue;
            fuse[k - 1] = Fuse{pg.ops[j].a_idx, pg.ops[j].b_idx, P};
            skip[j] = skip[k] = 1;
        }
    }
    struct Val {
        std::string name;
        Bnd b;
        bool mem;   // a freshly loaded leaf (const Fe29, carried, below 2 p: never needs a carry pass or a fold)
    };
    auto operand = [&](const char* name, size_t i, int kind, int idx) -> Val {
        const bool mem = kind == BZH_EXPR_COLUMN || kind == BZH_EXPR_CONST;
        return Val{KernelText::operand(name, i, kind, idx), mem ? leaf : bs[(size_t)idx], mem};
    };
    // what the kernel's variable `name` is known to be, after an in-place carry / fold
    auto remember = [&](const Val& x) {
        if (x.mem) return;
        if (x.name[0] == 'r') br[x.name[1] - '0'] = x.b;
        else if (x.name[0] == 's') bs[(size_t)atoi(x.name.c_str() + 1)] = x.b;
    };
    auto carry = [&](Val& x) {
        if (x.b.L <= kCarried) return;
        if (x.mem) {   // (cannot happen: leaves arrive carried)
            pg_fail = true;
            return;
        }
        add("    %s = fe29_carry(%s);\n", x.name.c_str(), x.name.c_str());
        npass++;
        x.b.T += x.b.L >> 29;
        x.b.L = (((uint64_t)1 << 29) - 1) + (x.b.L >> 29);
        remember(x);
    };
    // bring an operand below 2 p (fe29_fold takes a carried value)
    auto fold = [&](Val& x) {
        if (x.b.V <= 2.0) return;
        if (x.mem) {
            pg_fail = true;
            return;
        }
        carry(x);
        add("    %s = fe29_fold(%s);\n", x.name.c_str(), x.name.c_str());
        npass += 2;
        x.b = Bnd{2.0, kCarried, ((uint64_t)1 << 23) + 16};
        remember(x);
    };
    auto pow2_over = [](double b) {
        int k = 4;
        while ((double)k < b + 1.0) k *= 2;
        return k;
    };
    auto limb_max = [](const Bnd& b) { return (double)std::max(b.L, b.T); };
    // dst = a (op) b; returns what dst then is.  When a and b name the same variable (a square) every in-place change of one is
    // a change of the other: `same` keeps the two descriptions equal.
    auto arith = [&](int op, const std::string& dst, Val a, Val b) -> Bnd {
        if (op == V2_RSUB) {   // b - a
            std::swap(a, b);
            op = V2_SUB;
        }
        const bool same = !a.mem && !b.mem && a.name == b.name;
        auto sync = [&](Val& from, Val& to) {
            if (same) to.b = from.b;
        };
        if (op == V2_MUL) {
            for (int pass = 0; pass < 2 && a.b.V * b.b.V > 100.0; pass++) {
                if (a.b.V >= b.b.V) fold(a), sync(a, b);
                else fold(b), sync(b, a);
            }
            for (int pass = 0; pass < 2 && limb_max(a.b) * limb_max(b.b) > kColumn; pass++) {
                if (a.b.L >= b.b.L) carry(a), sync(a, b);
                else carry(b), sync(b, a);
            }
            if (a.b.V * b.b.V > 100.0 || limb_max(a.b) * limb_max(b.b) > kColumn) pg_fail = true;
            add("    %s = mulx(%s, %s);\n", dst.c_str(), a.name.c_str(), b.name.c_str());
            return product;
        }
        if (op == V2_ADD) {
            for (int pass = 0; pass < 2 && a.b.V + b.b.V > 100.0; pass++) {
                if (a.b.V >= b.b.V) fold(a), sync(a, b);
                else fold(b), sync(b, a);
            }
            for (int pass = 0; pass < 2 && a.b.L + b.b.L > 0xffffffffull; pass++) {
                if (a.b.L >= b.b.L) carry(a), sync(a, b);
                else carry(b), sync(b, a);
            }
            if (a.b.V + b.b.V > 100.0 || a.b.L + b.b.L > 0xffffffffull) pg_fail = true;
            const Bnd sum{a.b.V + b.b.V, a.b.L + b.b.L, a.b.T + b.b.T};
            add("    %s = fe29_add(%s, %s);\n", dst.c_str(), a.name.c_str(), b.name.c_str());
            return sum;
        }
        // a - b: the bias K p = J copies of (K / J) p has to dominate b limb by limb
        if (b.b.V > 60.0) fold(b), sync(b, a);
        if (b.b.L > 2 * (((uint64_t)1 << 30) - 2)) carry(b), sync(b, a);
        const int J = b.b.L > ((uint64_t)1 << 30) - 2 ? 2 : 1;
        int K = pow2_over(b.b.V);
        while ((uint64_t)K * ((uint64_t)1 << 22) < b.b.T + 2 * (uint64_t)J) K *= 2;
        if (a.b.V + K > 100.0) fold(a), sync(a, b);
        if (a.b.L + (uint64_t)J * kBiasLimb > 0xffffffffull) carry(a), sync(a, b);
        if (same || a.b.V + K > 100.0 || K > 64 || a.b.L + (uint64_t)J * kBiasLimb > 0xffffffffull) pg_fail = true;   // (x - x is never emitted)
        const Bnd diff{a.b.V + K, a.b.L + (uint64_t)J * kBiasLimb, a.b.T + (uint64_t)K * ((uint64_t)1 << 22) + (uint64_t)K};
        add("    %s = fe29_sub_lazy<P, %d, %d>(%s, %s);\n", dst.c_str(), K, J, a.name.c_str(), b.name.c_str());
        return diff;
    };
    // dst = a * b + slot * constant (one reduction)
    auto dot2 = [&](const std::string& dst, Val a, Val b, const Fuse& f) -> Bnd {
        char sn[32];
        snprintf(sn, sizeof(sn), "s%d", f.slot);
        Val c{sn, bs[(size_t)f.slot], false};
        const bool same = !a.mem && !b.mem && a.name == b.name;
        auto sync = [&](Val& from, Val& to) {
            if (same) to.b = from.b;
        };
        // (the constant: carried, below 2 p)
        for (int pass = 0; pass < 4 && a.b.V * b.b.V + c.b.V * 2.0 > 100.0; pass++) {
            if (c.b.V * 2.0 >= a.b.V * b.b.V) fold(c);
            else if (a.b.V >= b.b.V) fold(a), sync(a, b);
            else fold(b), sync(b, a);
        }
        // one column holds 9 terms of each product: A B + C D <= kColumn (the constant's limbs: carried)
        if (limb_max(c.b) * (double)kCarried > 0.5 * kColumn) carry(c);
        if (a.name == c.name) a.b = c.b;
        if (b.name == c.name) b.b = c.b;
        const double room = kColumn - limb_max(c.b) * (double)kCarried;
        for (int pass = 0; pass < 2 && limb_max(a.b) * limb_max(b.b) > room; pass++) {
            if (a.b.L >= b.b.L) carry(a), sync(a, b);
            else carry(b), sync(b, a);
        }
        if (a.b.V * b.b.V + c.b.V * 2.0 > 100.0 || limb_max(a.b) * limb_max(b.b) > room || limb_max(c.b) * (double)kCarried > 0.5 * kColumn)
            pg_fail = true;
        add("    %s = dot2x(%s, %s, %s, cv + %d * 12);\n", dst.c_str(), a.name.c_str(), b.name.c_str(), c.name.c_str(), f.cst);
        return product;
    };
    const char* const* regs = kV2RegNames;
    // (a skipped product's operands are a slot and a constant the callee fetches: nothing is loaded ahead for it)
    kt.walk(pg, [&](size_t i) { return skip[i] != 0; }, emit_load, [&](size_t i, const ExprOp2& o) {
        const int form = o.form(), op = o.op(), pos = o.pos();
        const std::string ra = regs[pos];
        if (fuse[i].dst >= 0) {   // this product and a skipped slot * constant one, summed
            const std::string rd = regs[fuse[i].dst];
            const Val a = form == V2_LL ? operand("la", i, o.a_kind, o.a_idx) : Val{ra, br[pos], false};
            const Val b = form == V2_SS ? Val{regs[(pos + 1) & 3], br[(pos + 1) & 3], false} : operand("lb", i, o.b_kind, o.b_idx);
            br[fuse[i].dst] = dot2(rd, a, b, fuse[i]);
            return;
        }
        if (form == V2_SS) {
            br[pos] = arith(op, ra, Val{ra, br[pos], false}, Val{regs[(pos + 1) & 3], br[(pos + 1) & 3], false});
        } else if (form == V2_SL) {
            br[pos] = arith(op, ra, Val{ra, br[pos], false}, operand("lb", i, o.b_kind, o.b_idx));
        } else if (form == V2_LL) {
            br[pos] = arith(op, ra, operand("la", i, o.a_kind, o.a_idx), operand("lb", i, o.b_kind, o.b_idx));
        } else if (op == V2_NEG) {
            src += "    { const Fe29<P> z = fe29_zero<P>();\n";
            const Bnd d = arith(V2_SUB, ra, Val{"z", zero, true}, Val{ra, br[pos], false});
            src += "    }\n";
            br[pos] = d;
        } else if (op == V2_LOAD) {
            const Val a = operand("la", i, o.a_kind, o.a_idx);
            src += "    " + ra + " = " + a.name + ";\n";
            br[pos] = a.b;
        } else {
            // a value kept for later uses: carried once here rather than once per copy (policy; the cheaper one is kept)
            Val x{ra, br[pos], false};
            if (carry_at_store) carry(x);
            add("    s%d = %s;\n", o.a_idx, ra.c_str());
            bs[(size_t)o.a_idx] = br[pos];
        }
    });
    if (br[0].L > 0xfffffff0ull || br[0].V > 120.0) pg_fail = true;
    if (pg_fail) return std::string();
    *passes = npass;
    src += "    fe_store(out + (v * size + r) * 8, fe29_to_sat_div32(r0));\n}\n";
    kt.close("bzh_q29", hash, kname);
    return src;
}
static std::string program2_source29(const Program2& pg, int field) {
    int pa = 0, pb = 0;
    const std::string a = program2_source29_policy(pg, field, true, &pa), b = program2_source29_policy(pg, field, false, &pb);
    if (a.empty() || b.empty()) return a.empty() ? b : a;
    return pb < pa ? b : a;
}
