// The verifier's per-proof host pass as a straight-line scalar program, compiled once per key (BZH_VERIFY_PASS_DEVICE).
//
// Everything verify_host (csrc/verifier.hpp) computes after the transcript -- from x^n down to the scalars of the left-side
// linear combination, c, the u_j and the three trailing scalars -- is a fixed sequence of field operations whose shape depends
// on the KeyShape only.  vp_body is that sequence, generic over its value type: verify_host runs it on Fe<SF> (VpHostEval), and
// vp_compile runs it ONCE per key on a recording type (VpRecorder) that writes a tape of {op, dst, a, b} over a slot file, so the
// two cannot drift apart.  h_pow_u64(omega, row), delta, n, the expression constants and the rotation offsets are evaluated when
// the tape is recorded and land in its constant pool.  vp_run interprets the tape, on the host (tests/helpers/
// verify_pass_check.hip) and one lane per proof in k_vp_scalars (csrc/verify_pass.hip).
//
//   ops      VP_MUL, VP_ADD, VP_SUB, VP_NEG, VP_SQR, VP_CONST (a: index into the pool) and VP_INV, which writes 0 for a zero operand
//            and, with b != 0, raises the lane's reject flag -- where verify_host returns false (x^n = 1, a Lagrange denominator, a
//            vanishing product, u_j = 0).  The Lagrange values l_i(x) invert without a check, as verify_host does.  The u_j are
//            inverted together (Montgomery's trick, as h_batch_invert on the host): a zero among them zeroes the product, so the
//            one checked VP_INV rejects that lane and no other.
//   inputs   slots [0, nch): theta, beta, gamma, y, x, x1, x2, x3, x4, xi, z, u_1 .. u_k; then the evaluation scalars in the
//            order the proof carries them, then c and f (ev_offsets: where each lies in the proof).  Montgomery form.
//   outputs  out_slots: the nl_cap scalars of the left side in verify_host's order (VP_NONE: padding, zero), then c, u_1 .. u_k;
//            pt_src names the point that goes with each of the nl_cap scalars.
//   schedule the transcript replay: what is absorbed and squeezed, in verify_host's order.
// Values are fully reduced after every operation on both sides, so interpreter and verify_host agree word for word.
// The tape is recorded in SSA form and then mapped onto slots by last use (vp_allocate): the slot file stays a few hundred entries.
//
// Included inside namespace bzh { namespace { by csrc/key_shape.hpp (which defines BZH_VP_WITH_COMPILER: the part that reads a
// KeyShape) and by csrc/verify_pass.hip (types and interpreter only).  Depends on host_field.hpp; vp_run and vp_lane also on
// hash_to_curve.hpp (fe_inv_ct, fe_lt_p) where they are instantiated.
#pragma once

enum : uint32_t { VP_MUL = 0, VP_ADD = 1, VP_SUB = 2, VP_NEG = 3, VP_SQR = 4, VP_INV = 5, VP_CONST = 6 };
constexpr uint32_t VP_NONE = 0xffffffffu;
// where a point of the left side comes from: kind << 28 | index
enum : uint32_t { VP_PT_PROOF = 0, VP_PT_FIXED = 1, VP_PT_SIGMA = 2, VP_PT_INST = 3, VP_PT_SRS = 4, VP_PT_ZERO = 5 };
// transcript steps: (kind, first, count) -- first: point index in read order / challenge slot / byte offset in the proof
enum : uint32_t { VP_TS_VK = 0, VP_TS_INST = 1, VP_TS_POINTS = 2, VP_TS_SQUEEZE = 3, VP_TS_SCALARS = 4 };
constexpr size_t kVpMaxOps = (size_t)1 << 20;   // a key whose tape would be longer has no device pass (BZH_E_RANGE when selected)

struct VerifyTape {
    bool ok = false;
    std::vector<uint32_t> ops;      // 4 words per instruction: op, dst, a, b
    std::vector<uint32_t> consts;   // 8 Montgomery limbs each
    uint32_t nslots = 0, nch = 0;
    std::vector<uint32_t> ev_offsets, out_slots, pt_src, schedule;
    size_t nl_cap = 0, proof_len = 0;
    size_t n_inv = 0, n_mul = 0;    // inversions and products (squarings included) per proof, for DESIGN.md section 7
    size_t nops() const { return ops.size() / 4; }
};

template <class P>
BZH_HD Fe<P> vp_load(const uint32_t* slots, size_t B, size_t b, uint32_t slot) {
    Fe<P> r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.l[i] = slots[((size_t)slot * 8 + i) * B + b];
    return r;
}
template <class P>
BZH_HD void vp_store(uint32_t* slots, size_t B, size_t b, uint32_t slot, const Fe<P>& v) {
#pragma unroll
    for (int i = 0; i < 8; i++) slots[((size_t)slot * 8 + i) * B + b] = v.l[i];
}
// 32 aligned bytes <-> a field element
template <class P>
BZH_HD Fe<P> vp_ld32(const void* p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return fe_load<P>((const uint32_t*)p);
#else
    Fe<P> r;
    memcpy(r.l, p, 32);
    return r;
#endif
}
template <class P>
BZH_HD void vp_st32(void* p, const Fe<P>& v) {
#if defined(__HIP_DEVICE_COMPILE__)
    fe_store<P>((uint32_t*)p, v);
#else
    memcpy(p, v.l, 32);
#endif
}
// the tape for lane b of B over slots[slot][limb][lane]; returns the reject flag.  The tape index and every branch are the same
// for all lanes.
template <class P>
BZH_HD uint32_t vp_run(const uint32_t* ops, uint32_t nops, const uint32_t* consts, uint32_t* slots, size_t B, size_t b) {
    uint32_t reject = 0;
#pragma unroll 1
    for (uint32_t i = 0; i < nops; i++) {
        const uint32_t op = ops[4 * i], dst = ops[4 * i + 1], a = ops[4 * i + 2], bb = ops[4 * i + 3];
        Fe<P> r;
        if (op == VP_CONST) {
#pragma unroll
            for (int j = 0; j < 8; j++) r.l[j] = consts[(size_t)a * 8 + j];
        } else {
            const Fe<P> va = vp_load<P>(slots, B, b, a);
            switch (op) {
                case VP_MUL: r = fe_mul(va, vp_load<P>(slots, B, b, bb)); break;
                case VP_ADD: r = fe_add(va, vp_load<P>(slots, B, b, bb)); break;
                case VP_SUB: r = fe_sub(va, vp_load<P>(slots, B, b, bb)); break;
                case VP_NEG: r = fe_neg(va); break;
                case VP_SQR: r = fe_sqr(va); break;
                default:
                    reject |= (bb != 0 && fe_is_zero(va)) ? 1u : 0u;
                    r = fe_inv_ct(va);   // a^(p - 2): zero for zero
            }
        }
        vp_store<P>(slots, B, b, dst, r);
    }
    return reject;
}

// Lane b of k_vp_scalars, as a host / device function (A: VerifyPassArgs, csrc/ctx.hpp): the challenges and the evaluation scalars
// into the slot file -- a scalar that is not below the modulus counts as zero and raises the flag --, the tape, then the left
// side's scalars in canonical form, (c, u_j) in Montgomery form and the lane's reject word.
template <class P, class A>
BZH_HD void vp_lane(const A& a, size_t b) {
    const size_t B = a.batch;
    uint32_t reject = 0;
#pragma unroll 1
    for (uint32_t j = 0; j < a.nch; j++) vp_store<P>(a.d_slots, B, b, j, vp_ld32<P>(a.d_ch + ((size_t)j * B + b) * 8));
    const uint8_t* row = a.d_proofs + b * a.pstride;
    const Fe<P> zero = fe_zero<P>();
#pragma unroll 1
    for (uint32_t i = 0; i < a.nev; i++) {
        const Fe<P> v = vp_ld32<P>(row + a.d_ev_offsets[i]);
        const bool ok = fe_lt_p(v);
        reject |= ok ? 0u : 1u;
        vp_store<P>(a.d_slots, B, b, a.nch + i, fe_to_mont(fe_csel(ok, v, zero)));
    }
    reject |= vp_run<P>(a.d_ops, a.nops, a.d_consts, a.d_slots, B, b);
#pragma unroll 1
    for (uint32_t t = 0; t < a.nl_cap; t++) {
        const uint32_t s = a.d_out_slots[t];
        Fe<P> v = zero;
        if (s != VP_NONE) v = fe_from_mont(vp_load<P>(a.d_slots, B, b, s));
        vp_st32<P>(a.d_lc_scal + (b * a.nl_cap + t) * 8, v);
    }
#pragma unroll 1
    for (uint32_t t = 0; t < a.ncu; t++) vp_st32<P>(a.d_cu + (b * a.ncu + t) * 8, vp_load<P>(a.d_slots, B, b, a.d_out_slots[a.nl_cap + t]));
    a.d_flags[b] = reject;
}

#if defined(BZH_VP_WITH_COMPILER)
// ---------------------------------------------------------------------------
// the arithmetic of the host pass, generic over the evaluator E (E::V: a value)
// ---------------------------------------------------------------------------
template <class V>
struct VpIn {
    V theta, beta, gamma, y, x, x1, x2, x3, x4, xi, z;
    std::vector<V> us;
    std::vector<V> inst_ev, adv_ev, fix_ev;
    V rand_ev;
    std::vector<V> sig_ev, pz0, pz1, pzl, lz0, lz1, la0, lam1, ls0, q_evals;   // pzl[nsets - 1]: zero
    V cm, fm;
};
template <class V>
struct VpOut {
    std::vector<uint32_t> pts;   // VP_PT_* << 28 | index, one per term
    std::vector<V> terms;        // the scalars of those points
    V tail[3];                   // the scalars of G_0, U, W
    std::vector<V> cu;           // c, u_1 .. u_k
};
// indices of a proof's points in read order (verify_point_offsets)
template <class Key>
struct VpPointIndex {
    size_t adv, lka, pz, lkz, rnd, h, f, S, L;
    explicit VpPointIndex(const Key& pk) {
        adv = 0;
        lka = (size_t)pk.na;
        pz = lka + 2 * (size_t)pk.nl;
        lkz = pz + (size_t)pk.nsets;
        rnd = lkz + (size_t)pk.nl;
        h = rnd + 1;
        f = h + (size_t)pk.npieces;
        S = f + 1;
        L = S + 1;
    }
};

template <class E, class Key>
static typename E::V vp_cx_eval(E& e, const Key& pk, int i, const VpIn<typename E::V>& in, bool& bad) {
    using V = typename E::V;
    using SF = typename E::Field;
    const CNode& nd = pk.cx[i];
    auto find = [&](const std::vector<std::pair<int, int>>& qs, const std::vector<V>& ev, int col, int rot) -> V {
        for (size_t k = 0; k < qs.size(); k++)
            if (qs[k].first == col && qs[k].second == rot) return ev[k];
        bad = true;
        return e.cst(fe_zero<SF>());
    };
    auto val = [&]() {
        Fe<SF> v;
        memcpy(v.l, nd.val, 32);
        return v;
    };
    switch (nd.tag) {
        case CX_CONST: return e.cst(val());
        case CX_ADVICE: return find(pk.advice_queries, in.adv_ev, (int)nd.col, nd.rot);
        case CX_FIXED: return find(pk.fixed_queries, in.fix_ev, (int)nd.col, nd.rot);
        case CX_INSTANCE: return find(pk.instance_queries, in.inst_ev, (int)nd.col, nd.rot);
        case CX_NEG: return e.neg(vp_cx_eval(e, pk, nd.a, in, bad));
        case CX_SCALE: {
            const V a = vp_cx_eval(e, pk, nd.a, in, bad);
            return e.mul(a, e.cst(val()));
        }
        case CX_ADD: {
            const V a = vp_cx_eval(e, pk, nd.a, in, bad);
            const V b = vp_cx_eval(e, pk, nd.b, in, bad);
            return e.add(a, b);
        }
        default: {
            const V a = vp_cx_eval(e, pk, nd.a, in, bad);
            const V b = vp_cx_eval(e, pk, nd.b, in, bad);
            return e.mul(a, b);
        }
    }
}

// false: the key's shape does not fit (a query the constraint system never registered, more terms than nl_cap)
template <class E, class Key>
static bool vp_body(E& e, const Key& pk, const VpIn<typename E::V>& in, size_t nl_cap, VpOut<typename E::V>& out) {
    using V = typename E::V;
    using SF = typename E::Field;
    const int nsets = pk.nsets, nl = pk.nl, npieces = pk.npieces;
    const size_t n = pk.n, m = pk.perm_columns.size();
    const unsigned k = pk.k;
    const VpPointIndex<Key> pi(pk);
    bool bad = false;
    auto pt = [](uint32_t kind, size_t idx) { return (kind << 28) | (uint32_t)idx; };
    const V one = e.cst(fe_one<SF>()), zero = e.cst(fe_zero<SF>());
    const V &x = in.x, &y = in.y, &beta = in.beta, &gamma = in.gamma, &theta = in.theta;
    // x^n by square-and-multiply over the bits of n (h_pow_u64)
    V xn = one;
    {
        V base = x;
        for (uint64_t ee = n; ee; ee >>= 1) {
            if (ee & 1) xn = e.mul(xn, base);
            base = e.sqr(base);
        }
    }
    // Lagrange values at x: l_i(x) = (x^n - 1) w^i / (n (x - w^i))
    Fe<SF> omega;
    {
        uint64_t t[4];
        memcpy(t, pk.omega, 32);
        omega = fe_from_u64<SF>(t);
    }
    Fe<SF> nfe_c;
    {
        uint64_t t[4] = {(uint64_t)n, 0, 0, 0};
        nfe_c = fe_to_mont(fe_from_u64<SF>(t));
    }
    const V nfe = e.cst(nfe_c);
    const V xn1 = e.sub(xn, one);
    auto lag = [&](size_t row) {
        const V wi = e.cst(h_pow_u64(omega, row));
        const V num = e.mul(xn1, wi);
        return e.mul(num, e.inv(e.mul(nfe, e.sub(x, wi)), false));
    };
    const V l0 = lag(0), l_last = lag(pk.usable);
    V l_blind = zero;
    for (size_t r = pk.usable + 1; r < n; r++) l_blind = e.add(l_blind, lag(r));
    const V active = e.sub(one, e.add(l_last, l_blind));
    Fe<SF> delta_c;
    memcpy(delta_c.l, pk.delta, 32);
    const V delta = e.cst(delta_c);
    // the quotient's terms in protocol order, folded with y
    V hacc = zero;
    auto push = [&](const V& t) { hacc = e.add(e.mul(hacc, y), t); };
    for (int g : pk.gates) push(vp_cx_eval(e, pk, g, in, bad));
    auto col_at0 = [&](std::pair<int, int> col) -> V {
        const auto& qs = col.first == CX_ADVICE ? pk.advice_queries : (col.first == CX_FIXED ? pk.fixed_queries : pk.instance_queries);
        const auto& ev = col.first == CX_ADVICE ? in.adv_ev : (col.first == CX_FIXED ? in.fix_ev : in.inst_ev);
        for (size_t q = 0; q < qs.size(); q++)
            if (qs[q].first == col.second && qs[q].second == 0) return ev[q];
        bad = true;
        return zero;
    };
    if (nsets) {
        push(e.mul(l0, e.sub(one, in.pz0[0])));
        const V zl = in.pz0[nsets - 1];
        push(e.mul(l_last, e.sub(e.sqr(zl), zl)));
        for (int i = 1; i < nsets; i++) push(e.mul(l0, e.sub(in.pz0[i], in.pzl[i - 1])));
        V cur_delta = e.mul(beta, x);
        for (int i = 0; i < nsets; i++) {
            const size_t c0 = (size_t)i * pk.chunk_len, c1 = std::min(m, c0 + pk.chunk_len);
            V left = in.pz1[i], right = in.pz0[i];
            for (size_t gj = c0; gj < c1; gj++) {
                const V v = col_at0(pk.perm_columns[gj]);
                left = e.mul(left, e.add(e.add(v, e.mul(beta, in.sig_ev[gj])), gamma));
                right = e.mul(right, e.add(e.add(v, cur_delta), gamma));
                cur_delta = e.mul(cur_delta, delta);
            }
            push(e.mul(active, e.sub(left, right)));
        }
    }
    for (int i = 0; i < nl; i++) {
        auto comp = [&](const std::vector<int>& es) {
            V acc = zero;
            for (int ex : es) {
                const V t = e.mul(acc, theta);
                acc = e.add(t, vp_cx_eval(e, pk, ex, in, bad));
            }
            return acc;
        };
        push(e.mul(l0, e.sub(one, in.lz0[i])));
        push(e.mul(l_last, e.sub(e.sqr(in.lz0[i]), in.lz0[i])));
        const V lhs = e.mul(e.mul(in.lz1[i], e.add(in.la0[i], beta)), e.add(in.ls0[i], gamma));
        const V ci = comp(pk.lookups[i].first);
        const V ct = comp(pk.lookups[i].second);
        const V rhs = e.mul(e.mul(in.lz0[i], e.add(ci, beta)), e.add(ct, gamma));
        push(e.mul(active, e.sub(lhs, rhs)));
        push(e.mul(l0, e.sub(in.la0[i], in.ls0[i])));
        push(e.mul(e.mul(active, e.sub(in.la0[i], in.ls0[i])), e.sub(in.la0[i], in.lam1[i])));
    }
    if (bad) return false;
    const V expected_h = e.mul(hacc, e.inv(xn1, true));   // (x^n = 1: rejected)

    // multiopen: evaluation of commitment `cid` at rotation r (a permutation product's third rotation is -(blinding + 1)),
    // and its place in the linear combination
    auto eval_of = [&](uint64_t cid, int r) -> V {
        const int kind = (int)(cid >> 32);
        const size_t i = (size_t)(cid & 0xffffffffu);
        auto from = [&](const std::vector<std::pair<int, int>>& qs, const std::vector<V>& ev) {
            for (size_t q = 0; q < qs.size(); q++)
                if (qs[q].first == (int)i && qs[q].second == r) return ev[q];
            bad = true;
            return zero;
        };
        switch (kind) {
            case K_INST: return from(pk.instance_queries, in.inst_ev);
            case K_ADV: return from(pk.advice_queries, in.adv_ev);
            case K_FIX: return from(pk.fixed_queries, in.fix_ev);
            case K_SIGMA: return in.sig_ev[i];
            case K_PZ: return r == 0 ? in.pz0[i] : (r == 1 ? in.pz1[i] : in.pzl[i]);
            case K_LZ: return r == 0 ? in.lz0[i] : in.lz1[i];
            case K_LA: return r == 0 ? in.la0[i] : in.lam1[i];
            case K_LS: return in.ls0[i];
            default: return i == M_H0 ? expected_h : in.rand_ev;
        }
    };
    const V &x1 = in.x1, &x2 = in.x2, &x3 = in.x3, &x4 = in.x4;
    const size_t nq = pk.rot_sets.size();
    // left-side linear combination: (point, scalar) pairs; proof / key commitments are weighted later by x4 powers
    struct Term {
        uint32_t pt;
        V s;
    };
    std::vector<std::vector<Term>> q_terms(nq);
    std::vector<std::vector<V>> q_evalsets(nq);
    std::vector<V> xn_pows(npieces, one);
    {
        V pw = one;
        for (int i = 0; i < npieces; i++) {
            xn_pows[i] = pw;
            pw = e.mul(pw, xn);
        }
    }
    for (size_t si = 0; si < nq; si++) {
        const auto& cids = pk.groups[si];
        const auto& rots = pk.rot_sets[si];
        std::vector<V> evs(rots.size(), zero);
        for (size_t j = 0; j < cids.size(); j++) {
            for (auto& t : q_terms[si]) t.s = e.mul(t.s, x1);  // cm = x1 * cm + C
            const uint64_t cid = cids[j];
            const int kind = (int)(cid >> 32);
            const size_t i = (size_t)(cid & 0xffffffffu);
            auto add_term = [&](uint32_t p, const V& s) { q_terms[si].push_back({p, s}); };
            switch (kind) {
                case K_INST: add_term(pt(VP_PT_INST, i), one); break;
                case K_ADV: add_term(pt(VP_PT_PROOF, pi.adv + i), one); break;
                case K_FIX: add_term(pt(VP_PT_FIXED, i), one); break;
                case K_SIGMA: add_term(pt(VP_PT_SIGMA, i), one); break;
                case K_PZ: add_term(pt(VP_PT_PROOF, pi.pz + i), one); break;
                case K_LZ: add_term(pt(VP_PT_PROOF, pi.lkz + i), one); break;
                case K_LA: add_term(pt(VP_PT_PROOF, pi.lka + 2 * i), one); break;
                case K_LS: add_term(pt(VP_PT_PROOF, pi.lka + 2 * i + 1), one); break;
                default:
                    if (i == M_H0) {
                        for (int p = 0; p < npieces; p++) add_term(pt(VP_PT_PROOF, pi.h + p), xn_pows[p]);
                    } else {
                        add_term(pt(VP_PT_PROOF, pi.rnd), one);
                    }
            }
            for (size_t t = 0; t < rots.size(); t++) {
                const V sc = e.mul(evs[t], x1);
                evs[t] = e.add(sc, eval_of(cid, rots[t]));
            }
        }
        q_evalsets[si] = evs;
    }
    if (bad) return false;
    const Fe<SF> omega_inv = fe_inv(omega);
    auto rot = [&](int r) {
        return e.mul(x, e.cst(r >= 0 ? h_pow_u64(omega, (uint64_t)r) : h_pow_u64(omega_inv, (uint64_t)(-(int64_t)r))));
    };
    V f_eval = zero;
    for (size_t si = 0; si < nq; si++) {
        const auto& rots = pk.rot_sets[si];
        const size_t np = rots.size();
        std::vector<V> ptv(np, zero);
        for (size_t t = 0; t < np; t++) ptv[t] = rot(rots[t]);
        // r(x3) by Lagrange's formula on (points, evals)
        V r_eval = zero, den = one;
        for (size_t j = 0; j < np; j++) {
            V num = one, dn = one;
            for (size_t mm = 0; mm < np; mm++) {
                if (mm == j) continue;
                num = e.mul(num, e.sub(x3, ptv[mm]));
                dn = e.mul(dn, e.sub(ptv[j], ptv[mm]));
            }
            const V w = e.mul(num, e.inv(dn, true));
            r_eval = e.add(r_eval, e.mul(q_evalsets[si][j], w));
            den = e.mul(den, e.sub(x3, ptv[j]));
        }
        const V lhs = e.mul(f_eval, x2);
        f_eval = e.add(lhs, e.mul(e.sub(in.q_evals[si], r_eval), e.inv(den, true)));
    }
    // final commitment = x4^nq f + sum_si x4^(nq-1-si) q_si, final value likewise
    V final_v = f_eval;
    for (size_t si = 0; si < nq; si++) final_v = e.add(e.mul(final_v, x4), in.q_evals[si]);
    std::vector<V> x4p(nq + 1, one);
    for (size_t i = 1; i <= nq; i++) x4p[i] = e.mul(x4p[i - 1], x4);
    out.pts.clear();
    out.terms.clear();
    auto lc_push = [&](uint32_t p, const V& s) {
        out.pts.push_back(p);
        out.terms.push_back(s);
    };
    lc_push(pt(VP_PT_PROOF, pi.f), x4p[nq]);
    for (size_t si = 0; si < nq; si++)
        for (auto& t : q_terms[si]) lc_push(t.pt, e.mul(t.s, x4p[nq - 1 - si]));
    // the opening argument: S, xi, z, (L_j, R_j, u_j), c, f
    std::vector<V> xp(k ? k : 1, one);
    if (k) {
        xp[0] = x3;
        for (unsigned i = 1; i < k; i++) xp[i] = e.sqr(xp[i - 1]);
    }
    V b0 = one;
    for (unsigned j = 0; j < k; j++) b0 = e.mul(b0, e.add(one, e.mul(in.us[j], xp[k - 1 - j])));
    std::vector<V> uinv = in.us;
    e.batch_inv(uinv.data(), k);   // (a zero u_j: rejected)
    for (unsigned j = 0; j < k; j++) {
        lc_push(pt(VP_PT_PROOF, pi.L + 2 * j), uinv[j]);
        lc_push(pt(VP_PT_PROOF, pi.L + 2 * j + 1), in.us[j]);
    }
    lc_push(pt(VP_PT_PROOF, pi.S), in.xi);
    if (out.terms.size() + 3 > nl_cap) return false;
    // scalars of G_0 (-v), U (-c b0 z), W (-f)
    out.tail[0] = e.neg(final_v);
    out.tail[1] = e.neg(e.mul(e.mul(in.cm, b0), in.z));
    out.tail[2] = e.neg(in.fm);
    out.cu.assign(1, in.cm);
    for (unsigned j = 0; j < k; j++) out.cu.push_back(in.us[j]);
    return true;
}

// verify_host's evaluator: the values themselves
template <class SF>
struct VpHostEval {
    using V = Fe<SF>;
    using Field = SF;
    bool reject = false;
    V cst(const Fe<SF>& c) { return c; }
    V mul(const V& a, const V& b) { return fe_mul(a, b); }
    V add(const V& a, const V& b) { return fe_add(a, b); }
    V sub(const V& a, const V& b) { return fe_sub(a, b); }
    V neg(const V& a) { return fe_neg(a); }
    V sqr(const V& a) { return fe_sqr(a); }
    V inv(const V& a, bool check) {
        if (check && fe_is_zero(a)) reject = true;
        return fe_inv(a);
    }
    void batch_inv(V* v, size_t n) {
        if (!h_batch_invert(v, n)) reject = true;
    }
};

// the recording evaluator: a value is an SSA id; inputs are ids [0, nin)
template <class SF>
struct VpRecorder {
    using V = int32_t;
    using Field = SF;
    struct Ins {
        uint32_t op;
        int32_t dst, a, b;
    };
    std::vector<Ins> ins;
    std::vector<Fe<SF>> consts;
    int32_t next = 0;
    size_t n_inv = 0, n_mul = 0;
    V input() { return next++; }
    V emit(uint32_t op, int32_t a, int32_t b) {
        ins.push_back({op, next, a, b});
        return next++;
    }
    V cst(const Fe<SF>& c) {
        size_t i = 0;
        for (; i < consts.size(); i++)
            if (fe_eq(consts[i], c)) break;
        if (i == consts.size()) consts.push_back(c);
        return emit(VP_CONST, (int32_t)i, 0);
    }
    V mul(V a, V b) {
        n_mul++;
        return emit(VP_MUL, a, b);
    }
    V add(V a, V b) { return emit(VP_ADD, a, b); }
    V sub(V a, V b) { return emit(VP_SUB, a, b); }
    V neg(V a) { return emit(VP_NEG, a, 0); }
    V sqr(V a) {
        n_mul++;
        return emit(VP_SQR, a, 0);
    }
    V inv(V a, bool check) {
        n_inv++;
        return emit(VP_INV, a, check ? 1 : 0);
    }
    // Montgomery's trick: the prefix products, one checked inversion, and the walk back
    void batch_inv(V* v, size_t n) {
        if (!n) return;
        std::vector<V> pre(n);
        pre[0] = v[0];
        for (size_t i = 1; i < n; i++) pre[i] = mul(pre[i - 1], v[i]);
        V acc = inv(pre[n - 1], true);
        for (size_t i = n; i-- > 1;) {
            const V d = v[i];
            v[i] = mul(acc, pre[i - 1]);
            acc = mul(acc, d);
        }
        v[0] = acc;
    }
};

// SSA ids -> slots: inputs keep slots [0, nin); every other value takes a free slot and hands it back after its last use;
// `outs` stay live to the end.  Fills tape.ops / tape.nslots / tape.out_slots (VP_NONE passes through).
template <class SF>
static void vp_allocate(const VpRecorder<SF>& rec, int32_t nin, const std::vector<int32_t>& outs, VerifyTape& tape) {
    const size_t ni = rec.ins.size();
    std::vector<int64_t> last((size_t)rec.next, -1);
    for (size_t i = 0; i < ni; i++) {
        const auto& in = rec.ins[i];
        if (in.op == VP_CONST) continue;
        last[in.a] = (int64_t)i;
        if (in.op == VP_MUL || in.op == VP_ADD || in.op == VP_SUB) last[in.b] = (int64_t)i;
    }
    for (int32_t o : outs)
        if (o >= 0) last[o] = (int64_t)ni;
    std::vector<uint32_t> slot((size_t)rec.next, VP_NONE), free_list;
    uint32_t nslots = (uint32_t)nin;
    for (int32_t i = 0; i < nin; i++) slot[i] = (uint32_t)i;
    tape.ops.clear();
    tape.ops.reserve(ni * 4);
    for (size_t i = 0; i < ni; i++) {
        const auto& in = rec.ins[i];
        const bool binary = in.op == VP_MUL || in.op == VP_ADD || in.op == VP_SUB;
        const uint32_t sa = in.op == VP_CONST ? (uint32_t)in.a : slot[in.a];
        const uint32_t sb = binary ? slot[in.b] : (uint32_t)in.b;
        // operands are read before the result is written: a slot that dies here may take the result
        if (in.op != VP_CONST) {
            if (in.a >= nin && last[in.a] == (int64_t)i) free_list.push_back(slot[in.a]);
            if (binary && in.b != in.a && in.b >= nin && last[in.b] == (int64_t)i) free_list.push_back(slot[in.b]);
        }
        uint32_t sd;
        if (!free_list.empty()) {
            sd = free_list.back();
            free_list.pop_back();
        } else {
            sd = nslots++;
        }
        slot[in.dst] = sd;
        tape.ops.insert(tape.ops.end(), {in.op, sd, sa, sb});
        if (last[in.dst] < 0) free_list.push_back(sd);   // never read
    }
    tape.nslots = nslots;
    tape.out_slots.clear();
    for (int32_t o : outs) tape.out_slots.push_back(o < 0 ? VP_NONE : slot[o]);
}

// the left side's capacity (verify_batch_t): every commitment once, L_j and R_j, S and f, G_0 U W, and room to spare
template <class Key>
static size_t vp_nl_cap(const Key& key) {
    const size_t ncommit = (size_t)key.na + 3 * key.nl + key.nsets + 1 + key.npieces + 1 + key.nf + key.perm_columns.size() + key.ni;
    return ncommit + 2 * (size_t)key.k + 1 + 3 + 4;
}

// The tape, its constants, the input / output tables and the transcript schedule of a key.  tape.ok stays false when the shape
// does not fit (vp_body) or the tape would pass kVpMaxOps.
template <class SF, class Key>
static void vp_compile(const Key& pk, VerifyTape& tape) {
    tape = VerifyTape();
    const size_t nl = (size_t)pk.nl, nsets = (size_t)pk.nsets, m = pk.perm_columns.size(), nq = pk.rot_sets.size(), k = pk.k;
    const size_t blind_rows = pk.n - pk.usable;
    const size_t est = 64 * (pk.cx.size() + blind_rows + m + 8 * nl + k) + 16 * (size_t)pk.npieces * nq;
    size_t set_work = 0, group_work = 0;
    for (size_t si = 0; si < nq; si++) {
        set_work += pk.rot_sets[si].size() * pk.rot_sets[si].size();
        group_work += pk.groups[si].size() * (pk.groups[si].size() + (size_t)pk.npieces + pk.rot_sets[si].size());
    }
    if (est + 8 * set_work + 4 * group_work > kVpMaxOps) return;
    VpRecorder<SF> rec;
    VpIn<int32_t> in;
    in.theta = rec.input(), in.beta = rec.input(), in.gamma = rec.input(), in.y = rec.input(), in.x = rec.input();
    in.x1 = rec.input(), in.x2 = rec.input(), in.x3 = rec.input(), in.x4 = rec.input(), in.xi = rec.input(), in.z = rec.input();
    for (size_t j = 0; j < k; j++) in.us.push_back(rec.input());
    tape.nch = (uint32_t)rec.next;
    // the evaluation scalars in proof order, with their byte offsets (verify_point_offsets walks the same layout)
    const VpPointIndex<Key> pi(pk);
    size_t off = 32 * pi.f;   // every point before the evaluations
    auto scalar = [&]() {
        tape.ev_offsets.push_back((uint32_t)off);
        off += 32;
        return rec.input();
    };
    const size_t ev_first = off;
    for (size_t i = 0; i < pk.instance_queries.size(); i++) in.inst_ev.push_back(scalar());
    for (size_t i = 0; i < pk.advice_queries.size(); i++) in.adv_ev.push_back(scalar());
    for (size_t i = 0; i < pk.fixed_queries.size(); i++) in.fix_ev.push_back(scalar());
    in.rand_ev = scalar();
    for (size_t i = 0; i < m; i++) in.sig_ev.push_back(scalar());
    in.pzl.assign(nsets, -1);
    for (size_t i = 0; i < nsets; i++) {
        in.pz0.push_back(scalar());
        in.pz1.push_back(scalar());
        if (i != nsets - 1) in.pzl[i] = scalar();
    }
    for (size_t i = 0; i < nl; i++) {
        in.lz0.push_back(scalar());
        in.lz1.push_back(scalar());
        in.la0.push_back(scalar());
        in.lam1.push_back(scalar());
        in.ls0.push_back(scalar());
    }
    const size_t ev_count = (off - ev_first) / 32;
    off += 32;   // f
    const size_t q_first = off;
    for (size_t i = 0; i < nq; i++) in.q_evals.push_back(scalar());
    off += 32 * (1 + 2 * k);   // S, L_j, R_j
    in.cm = scalar();
    in.fm = scalar();
    tape.proof_len = off;
    const int32_t nin = rec.next;
    if (nsets) in.pzl[nsets - 1] = rec.cst(fe_zero<SF>());
    tape.nl_cap = vp_nl_cap(pk);
    VpOut<int32_t> out;
    if (!vp_body(rec, pk, in, tape.nl_cap, out) || rec.ins.size() > kVpMaxOps) return;
    std::vector<int32_t> outs(tape.nl_cap, -1);
    tape.pt_src.assign(tape.nl_cap, VP_PT_ZERO << 28);
    for (size_t i = 0; i < out.terms.size(); i++) {
        outs[i] = out.terms[i];
        tape.pt_src[i] = out.pts[i];
    }
    for (int i = 0; i < 3; i++) {
        outs[tape.nl_cap - 3 + i] = out.tail[i];
        tape.pt_src[tape.nl_cap - 3 + i] = (VP_PT_SRS << 28) | (uint32_t)i;
    }
    outs.insert(outs.end(), out.cu.begin(), out.cu.end());
    vp_allocate(rec, nin, outs, tape);
    for (auto& c : rec.consts) tape.consts.insert(tape.consts.end(), c.l, c.l + 8);
    tape.n_inv = rec.n_inv;
    tape.n_mul = rec.n_mul;
    // the transcript replay, in verify_host's order
    auto step = [&](uint32_t kind, size_t first, size_t count) {
        if (count || kind == VP_TS_SQUEEZE || kind == VP_TS_VK) tape.schedule.insert(tape.schedule.end(), {kind, (uint32_t)first, (uint32_t)count});
    };
    uint32_t ch = 0;
    step(VP_TS_VK, 0, 1);
    step(VP_TS_INST, 0, (size_t)pk.ni);
    step(VP_TS_POINTS, pi.adv, (size_t)pk.na);
    step(VP_TS_SQUEEZE, ch++, 1);   // theta
    step(VP_TS_POINTS, pi.lka, 2 * nl);
    step(VP_TS_SQUEEZE, ch++, 1);   // beta
    step(VP_TS_SQUEEZE, ch++, 1);   // gamma
    step(VP_TS_POINTS, pi.pz, nsets + nl + 1);   // permutation products, lookup products, the random polynomial
    step(VP_TS_SQUEEZE, ch++, 1);   // y
    step(VP_TS_POINTS, pi.h, (size_t)pk.npieces);
    step(VP_TS_SQUEEZE, ch++, 1);   // x
    step(VP_TS_SCALARS, ev_first, ev_count);
    step(VP_TS_SQUEEZE, ch++, 1);   // x1
    step(VP_TS_SQUEEZE, ch++, 1);   // x2
    step(VP_TS_POINTS, pi.f, 1);
    step(VP_TS_SQUEEZE, ch++, 1);   // x3
    step(VP_TS_SCALARS, q_first, nq);
    step(VP_TS_SQUEEZE, ch++, 1);   // x4
    step(VP_TS_POINTS, pi.S, 1);
    step(VP_TS_SQUEEZE, ch++, 1);   // xi
    step(VP_TS_SQUEEZE, ch++, 1);   // z
    for (size_t j = 0; j < k; j++) {
        step(VP_TS_POINTS, pi.L + 2 * j, 2);
        step(VP_TS_SQUEEZE, ch++, 1);   // u_j
    }
    tape.ok = true;
}
#endif  // BZH_VP_WITH_COMPILER
