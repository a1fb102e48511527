// Part of the whole-proof translation unit (csrc/prove.hip): the evaluator's expression pool (hash-consed DAG) and the VM v1
// compiler.  (Circuit expressions as serialised, the registry keys, the device arena and the blob reader: csrc/key_shape.hpp,
// included before this file.)
// Host code only.  Included inside namespace bzh { namespace { (prove_kernels.cuh opens them).
#pragma once
// ---------------------------------------------------------------------------
// evaluator expressions (over a column registry)
// ---------------------------------------------------------------------------
enum { EX_CONST, EX_SYMBOL, EX_QUERY, EX_NEG, EX_ADD, EX_MUL, EX_SCALE };
struct ENode {
    uint8_t tag;
    int32_t col = 0, rot = 0;  // EX_QUERY: registry index, rotation; EX_SYMBOL: col = symbol id
    uint32_t val[8] = {0};
    int a = -1, b = -1;
};
// challenge symbols bound per proof
enum { SY_THETA, SY_BETA, SY_GAMMA, SY_Y, SY_XN, SY_X1, SY_X2, SY_X4, SY_BD0 /* + permutation column index */ };

struct ConstEnt {
    int sym = -1;  // >= 0: symbol id, else literal
    uint32_t val[8] = {0};
};
struct Program {
    std::vector<bzh_expr_op> ops;
    std::vector<ConstEnt> consts;
    int result_slot = 0;
};

struct EPool {
    std::vector<ENode> n;
    // hash-consing: structurally equal nodes are one node, so that shared subexpressions of the constraint polynomials
    // (a gate's selector product, x_q - x_p of the addition gates, ...) show up as shared nodes of a DAG
    struct NodeKey {
        uint8_t tag;
        int32_t col, rot, a, b;
        uint32_t val[8];
        bool operator<(const NodeKey& o) const { return memcmp(this, &o, sizeof(NodeKey)) < 0; }
    };
    std::map<NodeKey, int> interned;
    int push(const ENode& e) {
        NodeKey k;
        memset(&k, 0, sizeof(k));
        k.tag = e.tag;
        k.col = e.col, k.rot = e.rot, k.a = e.a, k.b = e.b;
        memcpy(k.val, e.val, 32);
        auto it = interned.find(k);
        if (it != interned.end()) return it->second;
        n.push_back(e);
        interned[k] = (int)n.size() - 1;
        return (int)n.size() - 1;
    }
    template <class F>
    int cnst(const F& v) {
        ENode e;
        e.tag = EX_CONST;
        memcpy(e.val, v.l, 32);
        return push(e);
    }
    int sym(int id) {
        ENode e;
        e.tag = EX_SYMBOL;
        e.col = id;
        return push(e);
    }
    int query(int col, int rot = 0) {
        ENode e;
        e.tag = EX_QUERY;
        e.col = col;
        e.rot = rot;
        return push(e);
    }
    int un(uint8_t tag, int a) {
        ENode e;
        e.tag = tag;
        e.a = a;
        return push(e);
    }
    int bin(uint8_t tag, int a, int b) {
        ENode e;
        e.tag = tag;
        e.a = a;
        e.b = b;
        return push(e);
    }
    int neg(int a) { return un(EX_NEG, a); }
    int add(int a, int b) { return bin(EX_ADD, a, b); }
    int sub(int a, int b) { return add(a, neg(b)); }
    int mul(int a, int b) { return bin(EX_MUL, a, b); }
    int horner(const std::vector<int>& terms, int ch) {  // ((t0 * ch + t1) * ch + t2) ...
        int acc = terms[0];
        for (size_t i = 1; i < terms.size(); i++) acc = add(mul(acc, ch), terms[i]);
        return acc;
    }
};

// Sethi-Ullman ordered emission into at most BZH_EXPR_MAX_SLOTS live intermediates (VM v1; tests/helpers/expr.py
// compiles the same format for the public bzh_expr_eval entry point); leaves are free operands
struct Compiler {
    const EPool& pool;
    Program prog;
    std::vector<int> free_slots, depth;
    bool overflow = false;
    explicit Compiler(const EPool& p) : pool(p), depth(p.n.size(), -1) {
        for (int s = BZH_EXPR_MAX_SLOTS - 1; s >= 0; s--) free_slots.push_back(s);
    }
    int depth_of(int i) {
        if (depth[i] >= 0) return depth[i];
        const ENode& e = pool.n[i];
        int d;
        if (e.tag == EX_CONST || e.tag == EX_SYMBOL || e.tag == EX_QUERY) d = 0;
        else if (e.tag == EX_NEG || e.tag == EX_SCALE) d = std::max(1, depth_of(e.a));
        else {
            const int da = depth_of(e.a), db = depth_of(e.b);
            d = da != db ? std::max(da, db) : da + 1;
        }
        return depth[i] = d;
    }
    int alloc() {
        if (free_slots.empty()) {
            overflow = true;
            return 0;
        }
        const int s = free_slots.back();
        free_slots.pop_back();
        return s;
    }
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
    struct Opnd {
        int kind, idx, rot, release;
    };
    Opnd operand(int i) {
        const ENode& e = pool.n[i];
        if (e.tag == EX_CONST) return {BZH_EXPR_CONST, const_index(-1, e.val), 0, -1};
        if (e.tag == EX_SYMBOL) return {BZH_EXPR_CONST, const_index(e.col, nullptr), 0, -1};
        if (e.tag == EX_QUERY) return {BZH_EXPR_COLUMN, e.col, e.rot, -1};
        const int s = emit(i);
        return {BZH_EXPR_SLOT, s, 0, s};
    }
    void push(int op, int dst, const Opnd& a, const Opnd& b) {
        bzh_expr_op o;
        o.op = (uint8_t)op;
        o.dst = (uint8_t)dst;
        o.a_kind = (uint8_t)a.kind;
        o.b_kind = (uint8_t)b.kind;
        o.a_idx = a.idx;
        o.b_idx = b.idx;
        o.a_rot = a.rot;
        o.b_rot = b.rot;
        prog.ops.push_back(o);
    }
    int emit(int i) {
        const ENode& e = pool.n[i];
        const Opnd none{BZH_EXPR_SLOT, 0, 0, -1};
        if (e.tag == EX_CONST || e.tag == EX_SYMBOL || e.tag == EX_QUERY) {
            const Opnd a = operand(i);
            const int d = alloc();
            push(BZH_EXPR_COPY, d, a, none);
            return d;
        }
        if (e.tag == EX_NEG) {
            const Opnd a = operand(e.a);
            const int d = a.release >= 0 ? a.release : alloc();
            push(BZH_EXPR_NEG, d, a, none);
            return d;
        }
        if (e.tag == EX_SCALE) {
            const Opnd a = operand(e.a);
            const int d = a.release >= 0 ? a.release : alloc();
            push(BZH_EXPR_MUL, d, a, Opnd{BZH_EXPR_CONST, const_index(-1, e.val), 0, -1});
            return d;
        }
        // the deeper child first, so that the shallower one never needs more slots than are left
        Opnd a, b;
        if (depth_of(e.b) > depth_of(e.a)) {
            b = operand(e.b);
            a = operand(e.a);
        } else {
            a = operand(e.a);
            b = operand(e.b);
        }
        const int d = a.release >= 0 ? a.release : (b.release >= 0 ? b.release : alloc());
        push(e.tag == EX_ADD ? BZH_EXPR_ADD : BZH_EXPR_MUL, d, a, b);
        if (a.release >= 0 && a.release != d) free_slots.push_back(a.release);
        if (b.release >= 0 && b.release != d) free_slots.push_back(b.release);
        return d;
    }
};
