// Part of the whole-proof translation unit (csrc/prove.hip): the VM v2 quotient compiler (y-folding by gate, shared
// subexpressions, hoisting, column leaves in slots) and what is asked of a compiled program: its hash, its loads and
// multiplications per row.  The instruction set: csrc/vm2_isa.hpp; the pool it compiles from: csrc/expr_compiler.hpp.
// Host code only.  Included inside namespace bzh { namespace { (prove_kernels.cuh opens them).
#pragma once
// ---------------------------------------------------------------------------------------------------------------
// Compiler2: the quotient's program for VM v2 (csrc/exprvm.hip: four stack registers + an LDS slot file).
//   value = (sum_j term_j y^(N-1-j)) * t_inv, terms in protocol order.  Consecutive terms of the form S * C_j with the
//   same S (a gate's constraints under its -- compressed -- selector) are folded as
//       ACC <- ACC y^m + S (C_0 y^(m-1) + ... + C_(m-1))
//   so the selector product is evaluated and multiplied in once per gate; inside a gate, subexpressions used more than
//   once are computed once and parked in LDS slots.  The arithmetic is exact field arithmetic: the value, hence every
//   proof byte, is the same as the plain Horner fold's.
// ---------------------------------------------------------------------------------------------------------------
// LDS slots: 0 ACC, 1 IN, then the shared-subexpression slots, spill slots last (allocated only if a program uses them)
static constexpr int kV2Regs = 4, kV2LdsAcc = 0, kV2LdsInner = 1, kV2LdsCse0 = 2, kV2LdsCseMax = 8, kV2LdsSpills = 2, kV2LdsGlobalMax = 6;
// ... and the column-leaf slots after the cross-group ones (Compiler2::select_leaves)
// The default is ONE number for every circuit: 3 is what the builtin kernels of both of the reference's circuits have registers
// for (9 VGPRs per slot, 162 of the 168 that three waves per SIMD allow).  A foreign circuit gets the same 3:
// it has no builtin kernel, its slots are the interpreter's LDS or whatever its own compiled module makes of them.
static constexpr int kV2LdsLeafMax = 8, kV2LdsLeafDefault = 3;
// BZH_VM2_LEAF = 0...8: how many of them a program may use (0: no leaf is kept; like BZH_VM2_CSE / BZH_VM2_GLOBAL another value is
// another program, which the interpreter runs).  Pinned bit for bit by tests/test_gpu_quotient_leaf_slots.py.
static constexpr char kV2LeafEnv[] = "BZH_VM2_LEAF";
enum { SY_YPOW0 = 4096 /* + m: y^m */ };

struct Program2 {
    std::vector<ExprOp2> ops;
    std::vector<ConstEnt> consts;
    bool ok = true;
    int nlds = 2;
    int leaf_base = 0, leaf_slots = 0;   // the slots that hold column leaves: [leaf_base, leaf_base + leaf_slots)
};
// column loads per row: the operands of kind BZH_EXPR_COLUMN the program reads
static size_t program2_loads(const Program2& pg) {
    size_t n = 0;
    for (const ExprOp2& o : pg.ops) n += (o.reads_a() && o.a_kind == BZH_EXPR_COLUMN) + (o.reads_b() && o.b_kind == BZH_EXPR_COLUMN);
    return n;
}
// field multiplications per row
static size_t program2_muls(const Program2& pg) {
    size_t n = 0;
    for (const ExprOp2& o : pg.ops) n += o.is_mul();
    return n;
}

// FNV-1a over the instruction words: ties a compiled quotient module to the program it was generated from
static uint64_t program2_hash(const Program2& pg, int field) {
    uint64_t h = 1469598103934665603ull;
    auto mix = [&](const void* p, size_t n) {
        for (size_t i = 0; i < n; i++) h = (h ^ ((const uint8_t*)p)[i]) * 1099511628211ull;
    };
    mix(&field, sizeof(field));
    mix(&pg.nlds, sizeof(pg.nlds));
    for (const ExprOp2& o : pg.ops) {
        const int32_t w[7] = {o.code, o.a_kind, o.a_idx, o.a_rot, o.b_kind, o.b_idx, o.b_rot};
        mix(w, sizeof(w));
    }
    return h;
}

struct Compiler2 {
    const EPool& pool;
    Program2 prog;
    int depth = 0;                       // registers r0..r(depth-1) hold the evaluation stack
    std::map<int, int> cse;              // node -> LDS slot holding its value (current scope)
    std::map<int, int> hoisted;          // node -> registry column holding its precomputed values (proof-independent)
    std::vector<int> label;              // Sethi-Ullman numbers (leaves 0), memoised per scope
    // shared-subexpression slots per gate group.  Round 2 measured 2 against 0, 4, 6, 8 on the INTERPRETER (slots are LDS there:
    // occupancy mattered more than the last 40 multiplications); the builtin kernels hold them in registers and have room
    // (130 -> 138 VGPRs of the 168 that three waves allow): 6 takes 41 more products out of the Board program (581 -> 540)
    int spill_used = 0, cse_slots = 6, max_lds = kV2LdsInner;
    // Values shared ACROSS gate groups (the same sub-polynomial in several gates: Board 94, Shot 71 products that per-group slots
    // recompute): up to `global_slots` more slots, each holding one value from the first to the last group that uses it; values
    // with disjoint ranges share a slot (select_globals).
    struct GlobalEnt {
        int slot, first, last;
    };
    int global_slots = 6;   // Board 541 -> 475 products, Shot 398 -> 356 (2: 495 / 376; perfect sharing: 447 / 327); 138 -> 146 VGPRs
    std::map<int, GlobalEnt> gsel;
    // COLUMN LEAVES kept across (and inside) gate groups.  A (column, rotation) leaf is an operand of the instruction that uses it,
    // so the program loaded it again at every use: Board 564 column loads per row for 130 distinct leaves, the eight rotation-0
    // advice leaves most of them.  Up to `leaf_slots` slots hold one leaf each over a range of groups: filled by LOAD + STORE when
    // the first group of the range opens, a slot operand until the last one closes -- no new operation, the products unchanged.
    // A leaf may reside several times (the ranges are chosen, not first-to-last use: select_leaves).  Each slot is 9 VGPRs in
    // the unsaturated builtin kernel: 3 keep it at three waves per SIMD without scratch (162 of 168 VGPRs; Board 564 -> 340, Shot 421 -> 258 loads).
    struct LeafEnt {
        int col, rot, slot, first, last;
    };
    int leaf_slots = kV2LdsLeafDefault, cur_group = -1;
    std::vector<LeafEnt> lsel;
    explicit Compiler2(const EPool& p) : pool(p), label(p.n.size(), -1) {
        if (const char* e = getenv("BZH_VM2_CSE")) cse_slots = std::max(0, std::min(kV2LdsCseMax, atoi(e)));
        if (const char* e = getenv("BZH_VM2_GLOBAL")) global_slots = std::max(0, std::min(kV2LdsGlobalMax, atoi(e)));
        if (const char* e = getenv(kV2LeafEnv)) leaf_slots = std::max(0, std::min(kV2LdsLeafMax, atoi(e)));
    }
    int leaf_base() const { return kV2LdsCse0 + cse_slots + kV2LdsSpills + global_slots; }
    int nlds() const { return max_lds + 1; }

    struct Leaf {
        int kind, idx, rot;
    };
    int const_index(int sym, const uint32_t* val) {
        for (size_t i = 0; i < prog.consts.size(); i++) {
            const ConstEnt& c = prog.consts[i];
            if (sym >= 0 ? c.sym == sym : (c.sym < 0 && !memcmp(c.val, val, 32))) return (int)i;
        }
        ConstEnt c;
        c.sym = sym;
        if (sym < 0) memcpy(c.val, val, 32);
        prog.consts.push_back(c);
        return (int)prog.consts.size() - 1;
    }
    bool is_leaf(int i) const {
        const ENode& e = pool.n[i];
        return e.tag == EX_CONST || e.tag == EX_SYMBOL || e.tag == EX_QUERY || cse.count(i) || hoisted.count(i);
    }
    // a column leaf: the slot it resides in while the current group is inside one of its ranges, else the column itself
    Leaf column_leaf(int col, int rot) const {
        for (const LeafEnt& l : lsel)
            if (l.col == col && l.rot == rot && l.first <= cur_group && cur_group <= l.last) return {BZH_EXPR_LDS, l.slot, 0};
        return {BZH_EXPR_COLUMN, col, rot};
    }
    Leaf leaf_of(int i) {
        auto ih = hoisted.find(i);
        if (ih != hoisted.end()) return column_leaf(ih->second, 0);
        auto it = cse.find(i);
        if (it != cse.end()) return {BZH_EXPR_LDS, it->second, 0};
        const ENode& e = pool.n[i];
        if (e.tag == EX_CONST) return {BZH_EXPR_CONST, const_index(-1, e.val), 0};
        if (e.tag == EX_SYMBOL) return {BZH_EXPR_CONST, const_index(e.col, nullptr), 0};
        if (e.rot < -32768 || e.rot > 32767) prog.ok = false;
        return column_leaf(e.col, e.rot);
    }
    int label_of(int i) {
        if (is_leaf(i)) return 0;
        if (label[i] >= 0) return label[i];
        const ENode& e = pool.n[i];
        int d;
        if (e.tag == EX_NEG || e.tag == EX_SCALE) d = std::max(1, label_of(e.a));
        else {
            const int la = label_of(e.a), lb = label_of(e.b);
            d = (la == 0 && lb == 0) ? 1 : (la == lb ? la + 1 : std::max(la, lb));
        }
        return label[i] = d;
    }
    void op(int form, int o, int pos, Leaf a = {0, 0, 0}, Leaf b = {0, 0, 0}) {
        if (pos < 0 || pos >= kV2Regs) prog.ok = false;
        ExprOp2 x;
        x.code = ExprOp2::encode(form, o, pos);
        x.a_kind = (uint8_t)a.kind, x.b_kind = (uint8_t)b.kind, x.pad = 0;
        x.a_idx = a.idx, x.b_idx = b.idx;
        x.a_rot = (int16_t)a.rot, x.b_rot = (int16_t)b.rot;
        prog.ops.push_back(x);
    }
    // a - b is add(a, neg(b)) in the pool: peel the negation so that it costs no instruction
    bool is_plain_neg(int i) const { return pool.n[i].tag == EX_NEG && !cse.count(i); }

    // emit node i: its value ends up in a new top-of-stack register
    void emit(int i) {
        if (is_leaf(i)) {
            op(V2_UN, V2_LOAD, depth, leaf_of(i));
            depth++;
            return;
        }
        const ENode& e = pool.n[i];
        if (e.tag == EX_NEG) {
            emit(e.a);
            op(V2_UN, V2_NEG, depth - 1);
        } else if (e.tag == EX_SCALE) {
            const Leaf c{BZH_EXPR_CONST, const_index(-1, e.val), 0};
            if (is_leaf(e.a)) {
                op(V2_LL, V2_MUL, depth, leaf_of(e.a), c);
                depth++;
            } else {
                emit(e.a);
                op(V2_SL, V2_MUL, depth - 1, Leaf{0, 0, 0}, c);
            }
        } else {
            int a = e.a, b = e.b, o = e.tag == EX_ADD ? V2_ADD : V2_MUL;
            if (e.tag == EX_ADD) {   // a + (-b') = a - b' ; (-a') + b = b - a'
                if (is_plain_neg(b)) b = pool.n[b].a, o = V2_SUB;
                else if (is_plain_neg(a)) {
                    const int t = pool.n[a].a;
                    a = b, b = t, o = V2_SUB;
                }
            }
            binary(o, a, b);
        }
        park(i);
    }
    void binary(int o, int a, int b) {
        const bool la = is_leaf(a), lb = is_leaf(b);
        const int rev = o == V2_SUB ? V2_RSUB : o;   // operands swapped
        if (la && lb) {
            op(V2_LL, o, depth, leaf_of(a), leaf_of(b));
            depth++;
        } else if (lb) {
            emit(a);
            op(V2_SL, o, depth - 1, Leaf{0, 0, 0}, leaf_of(b));
        } else if (la) {
            emit(b);
            op(V2_SL, rev, depth - 1, Leaf{0, 0, 0}, leaf_of(a));
        } else {
            const int na = label_of(a), nb = label_of(b);
            const bool a_first = na >= nb;
            const int first = a_first ? a : b, second = a_first ? b : a;
            emit(first);
            if (depth + std::max(1, label_of(second)) > kV2Regs) {
                // not enough registers for the other side: park this one in a spill slot and use it as a leaf
                if (spill_used >= kV2LdsSpills) {
                    prog.ok = false;
                    return;
                }
                const int sl = kV2LdsCse0 + cse_slots + spill_used++;
                max_lds = std::max(max_lds, sl);
                op(V2_UN, V2_STORE, depth - 1, Leaf{BZH_EXPR_LDS, sl, 0});
                depth--;
                emit(second);
                op(V2_SL, a_first ? rev : o, depth - 1, Leaf{0, 0, 0}, Leaf{BZH_EXPR_LDS, sl, 0});
                spill_used--;
            } else {
                emit(second);
                op(V2_SS, a_first ? o : rev, depth - 2);
                depth--;
            }
        }
    }
    // shared subexpression bookkeeping for the current scope
    std::map<int, int> want;   // node -> LDS slot it is to be parked in after its first evaluation
    void park(int i) {
        auto it = want.find(i);
        if (it == want.end() || cse.count(i)) return;
        op(V2_UN, V2_STORE, depth - 1, Leaf{BZH_EXPR_LDS, it->second, 0});
        cse[i] = it->second;
        if (gsel.count(i)) gparked.insert(i);
        std::fill(label.begin(), label.end(), -1);   // nodes above it are cheaper to reach now
    }
    void count_uses(int i, std::map<int, int>& uses, std::map<int, int>& weight) {
        const ENode& e = pool.n[i];
        if (e.tag == EX_CONST || e.tag == EX_SYMBOL || e.tag == EX_QUERY || hoisted.count(i) || cse.count(i)) return;
        if (uses[i]++) return;
        int w = 1;
        if (e.a >= 0) {
            count_uses(e.a, uses, weight);
            w += weight.count(e.a) ? weight[e.a] : 0;
        }
        if (e.b >= 0) {
            count_uses(e.b, uses, weight);
            w += weight.count(e.b) ? weight[e.b] : 0;
        }
        weight[i] = w;
    }
    // distinct operation nodes under i (`stop` and parked / hoisted values are leaves): products and other operations
    void reach(int i, std::set<int>& seen, const std::set<int>& stop, int* products, int* others) const {
        const ENode& e = pool.n[i];
        if (e.tag == EX_CONST || e.tag == EX_SYMBOL || e.tag == EX_QUERY || hoisted.count(i) || stop.count(i)) return;
        if (!seen.insert(i).second) return;
        if (e.tag == EX_MUL || e.tag == EX_SCALE) ++*products;
        else ++*others;
        if (e.a >= 0) reach(e.a, seen, stop, products, others);
        if (e.b >= 0) reach(e.b, seen, stop, products, others);
    }
    // choose the values kept across groups: greedily the best saving per group of residence that still finds a free slot
    void select_globals(const std::vector<std::vector<int>>& group_roots) {
        gsel.clear();
        if (global_slots <= 0) return;
        const int base = kV2LdsCse0 + cse_slots + kV2LdsSpills;
        std::vector<std::vector<std::pair<int, int>>> busy((size_t)global_slots);
        std::set<int> chosen;
        for (int round = 0; round < 256; round++) {
            std::map<int, std::vector<int>> where;
            for (size_t gi = 0; gi < group_roots.size(); gi++) {
                std::set<int> seen;
                int p = 0, o = 0;
                for (int r : group_roots[gi]) reach(r, seen, chosen, &p, &o);
                for (int n : seen) where[n].push_back((int)gi);
            }
            double best_score = 0;
            int best_n = -1, best_slot = -1;
            for (auto& kv : where) {
                if (kv.second.size() < 2) continue;
                std::set<int> seen;
                int p = 0, o = 0;
                reach(kv.first, seen, chosen, &p, &o);
                if (p == 0) continue;   // sums alone are cheaper to redo than to hold
                const int first = kv.second.front(), last = kv.second.back();
                int slot = -1;
                for (int sl = 0; sl < global_slots && slot < 0; sl++) {
                    bool free_ = true;
                    for (auto& iv : busy[(size_t)sl]) free_ &= last < iv.first || first > iv.second;
                    if (free_) slot = sl;
                }
                if (slot < 0) continue;
                const double benefit = (double)(kv.second.size() - 1) * (200.0 * p + 25.0 * o) - 30.0;   // (- the store)
                const double score = benefit / (double)(last - first + 1);
                if (benefit > 0 && score > best_score) best_score = score, best_n = kv.first, best_slot = slot;
            }
            if (best_n < 0) break;
            const std::vector<int>& gs = where[best_n];
            gsel[best_n] = GlobalEnt{base + best_slot, gs.front(), gs.back()};
            busy[(size_t)best_slot].push_back({gs.front(), gs.back()});
            chosen.insert(best_n);
            max_lds = std::max(max_lds, base + best_slot);
        }
    }
    // Choose the residences of column leaves from the program emitted WITHOUT them (`group_of[i]`: the group of instruction i):
    // caching a leaf changes operand kinds only, so the loads counted there are exact.  A candidate is a leaf over a range of
    // groups [first, last] that begins and ends at a use; its saving is the loads inside the range minus the one that fills
    // the slot.  Greedy like select_globals: the best saving per group of residence that still finds a slot free over its range;
    // re-evaluated after every choice, because a chosen range takes its loads away from the leaf's other candidates.
    // Cost: every round takes at least two loads out of `uses`, so there are at most loads / 2 rounds (Board 65, Shot 51 at the
    // default), each a scan of leaves x groups^2 / 2 ranges x slots: Board 130 leaves, a few milliseconds of host time per
    // bzh_pk_create (not visible beside the two emissions).  It grows with the cube of the group count; a circuit with many hundreds of gates would want per-group
    // free-slot masks kept between rounds.
    void select_leaves(const std::vector<int>& group_of, int ngroups) {
        lsel.clear();
        if (leaf_slots <= 0 || ngroups <= 0) return;
        std::map<std::pair<int, int>, std::vector<int>> uses;   // (column, rotation) -> loads per group
        auto count = [&](int kind, int col, int rot, int g) {
            if (kind != BZH_EXPR_COLUMN) return;
            std::vector<int>& u = uses[{col, rot}];
            if (u.empty()) u.assign((size_t)ngroups, 0);
            u[(size_t)g]++;
        };
        for (size_t i = 0; i < prog.ops.size(); i++) {
            const ExprOp2& o = prog.ops[i];
            if (o.reads_a()) count(o.a_kind, o.a_idx, o.a_rot, group_of[i]);
            if (o.reads_b()) count(o.b_kind, o.b_idx, o.b_rot, group_of[i]);
        }
        std::vector<std::vector<char>> busy((size_t)leaf_slots, std::vector<char>((size_t)ngroups, 0));
        for (;;) {
            double best_score = 0;
            int best_saving = 0, best_slot = -1, best_first = 0, best_last = 0;
            std::pair<int, int> best_leaf{0, 0};
            for (auto& kv : uses) {
                const std::vector<int>& u = kv.second;
                for (int first = 0; first < ngroups; first++) {
                    if (!u[(size_t)first]) continue;
                    int loads = 0;
                    unsigned free_ = (1u << leaf_slots) - 1;   // slots free over [first, last] so far
                    for (int last = first; last < ngroups && free_; last++) {
                        for (int sl = 0; sl < leaf_slots; sl++)
                            if (busy[(size_t)sl][(size_t)last]) free_ &= ~(1u << sl);
                        if (!free_) break;
                        if (!u[(size_t)last]) continue;
                        loads += u[(size_t)last];
                        const int saving = loads - 1;
                        const double score = (double)saving / (double)(last - first + 1);
                        if (saving > 0 && (score > best_score || (score == best_score && saving > best_saving))) {
                            best_score = score, best_saving = saving, best_leaf = kv.first, best_first = first, best_last = last;
                            best_slot = __builtin_ctz(free_);
                        }
                    }
                }
            }
            if (best_slot < 0) break;
            lsel.push_back(LeafEnt{best_leaf.first, best_leaf.second, leaf_base() + best_slot, best_first, best_last});
            std::vector<int>& u = uses[best_leaf];
            for (int g = best_first; g <= best_last; g++) busy[(size_t)best_slot][(size_t)g] = 1, u[(size_t)g] = 0;
        }
    }
    // fill the slots of the leaves whose residence begins with this group
    void fill_leaves(int group) {
        for (const LeafEnt& l : lsel) {
            if (l.first != group) continue;
            op(V2_UN, V2_LOAD, 0, Leaf{BZH_EXPR_COLUMN, l.col, l.rot});
            op(V2_UN, V2_STORE, 0, Leaf{BZH_EXPR_LDS, l.slot, 0});
            max_lds = std::max(max_lds, l.slot);
        }
    }
    std::set<int> gparked;
    void open_scope(const std::vector<int>& roots, int group = -1) {
        cse.clear();
        want.clear();
        for (auto& kv : gsel) {   // values living across groups: parked ones are leaves here, the others are parked when first computed
            if (group < kv.second.first || group > kv.second.last) continue;
            if (gparked.count(kv.first)) cse[kv.first] = kv.second.slot;
            else want[kv.first] = kv.second.slot;
        }
        std::fill(label.begin(), label.end(), -1);
        std::map<int, int> uses, weight;
        for (int r : roots) count_uses(r, uses, weight);
        std::vector<std::pair<long, int>> cand;
        for (auto& kv : uses) {
            if (kv.second >= 2 && !gsel.count(kv.first)) cand.push_back({-(long)(kv.second - 1) * weight[kv.first], kv.first});
        }
        std::sort(cand.begin(), cand.end());
        for (size_t k = 0; k < cand.size() && k < (size_t)cse_slots; k++) {
            want[cand[k].second] = kV2LdsCse0 + (int)k;
            max_lds = std::max(max_lds, kV2LdsCse0 + (int)k);
        }
    }

    // the whole quotient: terms in protocol order, y = symbol SY_Y, result (times t_inv) in r0
    void quotient(const std::vector<int>& terms, int tinv_node) {
        struct Group {
            int s;                  // shared left factor (-1: none)
            std::vector<int> c;     // the other factors, or the whole terms
        };
        std::vector<Group> groups;
        for (int t : terms) {
            const ENode& e = pool.n[t];
            const int s = (e.tag == EX_MUL) ? e.a : -1;
            if (s >= 0 && !groups.empty() && groups.back().s == s) groups.back().c.push_back(e.b);
            else groups.push_back(Group{s, {s >= 0 ? e.b : t}});
        }
        if (getenv("BZH_VM2_DEBUG")) {   // how many products a perfect (unbounded) sharing across all groups would leave
            std::map<int, int> uses, weight;
            size_t horner = 0;
            for (auto& g : groups) {
                for (int r : g.c) count_uses(r, uses, weight);
                if (g.s >= 0) count_uses(g.s, uses, weight);
                horner += g.c.size() - 1 + (g.s >= 0 ? 1 : 0) + 1;
            }
            size_t uniq_mul = 0, shared = 0;
            for (auto& kv : uses) {
                const ENode& e = pool.n[kv.first];
                if (e.tag == EX_MUL || e.tag == EX_SCALE) uniq_mul++;
                if (kv.second >= 2) shared++;
            }
            {   // shared nodes: weight (products under them), the groups that use them
                std::map<int, std::vector<int>> where;
                for (size_t gi = 0; gi < groups.size(); gi++) {
                    std::map<int, int> u2, w2;
                    for (int r : groups[gi].c) count_uses(r, u2, w2);
                    if (groups[gi].s >= 0) count_uses(groups[gi].s, u2, w2);
                    for (auto& kv : u2) where[kv.first].push_back((int)gi);
                }
                for (auto& kv : uses) {
                    if (kv.second < 2 || where[kv.first].size() < 2) continue;
                    const ENode& e = pool.n[kv.first];
                    fprintf(stderr, "[vm2-shared] node %d tag %d weight %d uses %d groups", kv.first, (int)e.tag, weight[kv.first], kv.second);
                    for (int gi : where[kv.first]) fprintf(stderr, " %d", gi);
                    fprintf(stderr, "\n");
                }
            }
            fprintf(stderr, "[vm2] groups %zu, unique product nodes %zu, glue products (y powers, selectors, ACC) ~%zu, nodes used more than once %zu\n",
                    groups.size(), uniq_mul, horner, shared);
        }
        const Leaf y{BZH_EXPR_CONST, const_index(SY_Y, nullptr), 0};
        const Leaf acc{BZH_EXPR_LDS, kV2LdsAcc, 0}, inner{BZH_EXPR_LDS, kV2LdsInner, 0};
        {
            std::vector<std::vector<int>> group_roots;
            for (auto& g : groups) {
                group_roots.push_back(g.c);
                if (g.s >= 0) group_roots.back().push_back(g.s);
            }
            gparked.clear();
            select_globals(group_roots);
        }
        // (the accumulator's Horner form ACC <- ACC y^m + S inner fixes the order of the groups: the power of y a constraint gets is
        // the number of constraints after it, so the groups run in protocol order and the leaf ranges are chosen for that order)
        std::vector<int> group_of;
        auto emit_groups = [&]() {
            prog.ops.clear();
            group_of.clear();
            gparked.clear();
            spill_used = 0;
            bool first_group = true;
            int group_index = -1;
            for (auto& g : groups) {
                group_index++;
                cur_group = group_index;
                std::vector<int> roots = g.c;
                if (g.s >= 0) roots.push_back(g.s);
                open_scope(roots, group_index);
                fill_leaves(group_index);
                const size_t m = g.c.size();
                if (m > 64) prog.ok = false;   // y^m symbols are provided up to 64
                for (size_t j = 0; j < m; j++) {
                    depth = 0;
                    if (j == 0) {
                        emit(g.c[0]);
                    } else if (label_of(g.c[j]) < kV2Regs) {
                        op(V2_LL, V2_MUL, 0, inner, y);          // r0 = IN y
                        depth = 1;
                        emit(g.c[j]);                            // r1 = C_j
                        op(V2_SS, V2_ADD, 0);
                        depth = 1;
                    } else {
                        emit(g.c[j]);                            // r0 = C_j (needs every register)
                        op(V2_LL, V2_MUL, 1, inner, y);          // r1 = IN y
                        op(V2_SS, V2_ADD, 0);
                    }
                    if (j + 1 < m) op(V2_UN, V2_STORE, 0, inner);
                }
                // r0 = sum_j C_j y^(m-1-j); times the shared factor
                if (g.s >= 0) {
                    if (is_leaf(g.s)) {
                        op(V2_SL, V2_MUL, 0, Leaf{0, 0, 0}, leaf_of(g.s));
                    } else if (label_of(g.s) < kV2Regs) {
                        depth = 1;
                        emit(g.s);
                        op(V2_SS, V2_MUL, 0);
                    } else {
                        op(V2_UN, V2_STORE, 0, inner);
                        depth = 0;
                        emit(g.s);
                        op(V2_SL, V2_MUL, 0, Leaf{0, 0, 0}, inner);
                    }
                }
                if (!first_group) {                              // ACC = ACC y^m + r0
                    const Leaf ym{BZH_EXPR_CONST, const_index(m == 1 ? SY_Y : SY_YPOW0 + (int)m, nullptr), 0};
                    op(V2_LL, V2_MUL, 1, acc, ym);
                    op(V2_SS, V2_ADD, 0);
                }
                op(V2_UN, V2_STORE, 0, acc);
                first_group = false;
                group_of.resize(prog.ops.size(), group_index);
            }
            cse.clear();
            want.clear();
            cur_group = -1;
            op(V2_SL, V2_MUL, 0, Leaf{0, 0, 0}, leaf_of(tinv_node));
            group_of.resize(prog.ops.size(), group_index);
        };
        emit_groups();
        if (leaf_slots > 0 && prog.ok) {   // the same program again with the chosen leaves in slots (0: the first emission is the program)
            select_leaves(group_of, (int)groups.size());
            if (!lsel.empty()) emit_groups();
        }
        std::set<int> used;
        for (const LeafEnt& l : lsel) used.insert(l.slot);
        prog.leaf_base = leaf_base(), prog.leaf_slots = (int)used.size();
    }
};
