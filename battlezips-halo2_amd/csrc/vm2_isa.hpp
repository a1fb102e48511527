// The VM v2 instruction set: what the interpreter (csrc/exprvm.hip, k_expr_vm2), the quotient compiler (csrc/quotient_compiler.hpp)
// and the source emitters (csrc/quotient_emit.hpp) agree on.  The one place that knows how an instruction word is packed.
//   forms  SS r[p] = r[p] op r[p+1];  SL r[p] = r[p] op leaf b;  LL r[p] = leaf a op leaf b;  UN: NEG r[p] / LOAD r[p] = leaf a /
//          STORE slot a = r[p];   op in {ADD, SUB, MUL, RSUB (b - a)};   p = the result register, fixed at compile time
//   leaves (kind, idx, rot): a column at a rotation, a constant, a slot of the slot file (LDS in the interpreter)
#pragma once
#include <cstdint>

namespace bzh {

enum { BZH_EXPR_LDS = 3 };   // operand kind, after the public BZH_EXPR_SLOT / COLUMN / CONST (include/bzh2.h)
enum { V2_SS = 0, V2_SL = 1, V2_LL = 2, V2_UN = 3 };
enum { V2_ADD = 0, V2_SUB = 1, V2_MUL = 2, V2_RSUB = 3 };
enum { V2_NEG = 0, V2_LOAD = 1, V2_STORE = 2 };   // the operations of form UN

struct ExprOp2 {
    uint8_t code, a_kind, b_kind, pad;
    int32_t a_idx, b_idx;
    int16_t a_rot, b_rot;
    static constexpr uint8_t encode(int form, int op, int pos) { return (uint8_t)((form << 4) | (op << 2) | (pos & 3)); }
    constexpr int form() const { return code >> 4; }
    constexpr int op() const { return (code >> 2) & 3; }
    constexpr int pos() const { return code & 3; }
    // which operand fields the instruction READS (a STORE names the slot it writes in a)
    constexpr bool reads_a() const { return form() == V2_LL || (form() == V2_UN && op() == V2_LOAD); }
    constexpr bool reads_b() const { return form() == V2_SL || form() == V2_LL; }
    constexpr bool is_store() const { return form() == V2_UN && op() == V2_STORE; }
    constexpr bool is_mul() const { return form() != V2_UN && op() == V2_MUL; }
};
static_assert(sizeof(ExprOp2) == 16, "ExprOp2 layout");

}  // namespace bzh
