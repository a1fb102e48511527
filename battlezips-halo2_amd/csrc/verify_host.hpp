// Part of the whole-proof translation unit (csrc/prove.hip): the verifier's HOST PASS over one proof -- transcript replay and
// point decompression here, then the arithmetic of csrc/verify_program.hpp's vp_body on the values themselves.  Host code only
// (key_shape.hpp, the C ABI's transcript, point_decompress), so that tests/helpers/verify_pass_check.hip can build it into a
// stand-alone program next to the tape's interpreter.
#pragma once
template <class C>
struct ProofView {
    using SF = typename CurveInfo<C>::SF;
    // outputs of the host pass: left-side linear combination and the right side's (c, u_j)
    std::vector<uint64_t> lc_pts, lc_scal, cu;
    bool ok = false;
};

// the points of one proof decoded ahead of the host pass (BZH_VERIFY_POINTS_DEVICE): affine canonical, one BZH_POINT_* each
struct PrePoints {
    const uint32_t* offsets = nullptr;
    size_t count = 0;
    const uint64_t* xy = nullptr;
    const uint8_t* status = nullptr;
};
// wall time a host pass spent decompressing points / in all (BZH_PROVE_TRACE only)
struct HostPassTimes {
    double decompress_ms = 0, total_ms = 0;
};

// host pass over one proof; inst_xy: this proof's instance commitments.  Returns false on any malformed input.
template <class C>
static bool verify_host(const KeyShape& pk, const uint64_t* inst_xy, const uint8_t* proof, size_t len, size_t nl_cap,
                        ProofView<C>& out, const PrePoints* pre = nullptr, HostPassTimes* times = nullptr) {
    using SF = typename CurveInfo<C>::SF;
    const int na = pk.na, ni = pk.ni, nsets = pk.nsets, nl = pk.nl, npieces = pk.npieces;
    const size_t m = pk.perm_columns.size();
    const unsigned k = pk.k;
    bzh_transcript* T = nullptr;
    if (bzh_transcript_new(pk.field, &T)) return false;
    struct Guard {
        bzh_transcript* t;
        ~Guard() { bzh_transcript_free(t); }
    } guard{T};
    size_t off = 0;
    bool bad = false;
    std::vector<uint64_t> pts;     // every point read from the proof, affine canonical
    pts.reserve(((size_t)na + 3 * nl + nsets + npieces + 3 + 2 * (size_t)k + 8) * 8);  // terms keep pointers into it: no regrowth
    auto read_point = [&]() -> size_t {  // index into pts (units of 8 u64)
        const size_t idx = pts.size() / 8;
        pts.resize(pts.size() + 8, 0);
        if (off + 32 > len) {
            bad = true;
            return idx;
        }
        bool ok;
        if (pre && idx < pre->count && pre->offsets[idx] == off) {   // decoded on the device; INVALID and IDENTITY leave zeros
            ok = pre->status[idx] == BZH_POINT_OK;
            if (ok) memcpy(&pts[idx * 8], pre->xy + idx * 8, 64);
        } else if (times) {
            const auto t0 = std::chrono::steady_clock::now();
            ok = point_decompress(C::id, proof + off, &pts[idx * 8]);
            times->decompress_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        } else {
            ok = point_decompress(C::id, proof + off, &pts[idx * 8]);
        }
        if (!ok) {
            bad = true;
            return idx;
        }
        // upstream's Blake2bRead::common_point fails on the identity ("cannot write points at infinity to the
        // transcript"): a proof carrying an identity commitment is rejected, not absorbed as (0, 0)
        {
            uint64_t any = 0;
            for (int i = 0; i < 8; i++) any |= pts[idx * 8 + i];
            if (!any) {
                bad = true;
                return idx;
            }
        }
        off += 32;
        bzh_transcript_common_point(T, &pts[idx * 8]);
        return idx;
    };
    auto read_scalar = [&]() -> Fe<SF> {
        uint64_t l[4] = {0, 0, 0, 0};
        if (off + 32 > len) {
            bad = true;
            return fe_zero<SF>();
        }
        memcpy(l, proof + off, 32);
        off += 32;
        const Fe<SF> v = fe_from_u64<SF>(l);
        if (!is_canonical(v)) bad = true;
        bzh_transcript_common_scalar(T, l);
        return fe_to_mont(v);
    };
    auto squeeze = [&]() {
        uint64_t ch[4];
        bzh_transcript_squeeze_challenge(T, ch);
        return fe_to_mont(fe_from_u64<SF>(ch));
    };
    // the transcript replay and the proof's operands first; the arithmetic on them (verify_program.hpp's vp_body, the code the
    // device pass's tape is recorded from) follows
    VpIn<Fe<SF>> in;
    bzh_transcript_common_scalar(T, pk.vk_repr);
    for (int i = 0; i < ni; i++) bzh_transcript_common_point(T, inst_xy + 8 * i);
    for (int i = 0; i < na; i++) read_point();
    in.theta = squeeze();
    for (int i = 0; i < 2 * nl; i++) read_point();
    in.beta = squeeze();
    in.gamma = squeeze();
    for (int i = 0; i < nsets; i++) read_point();
    for (int i = 0; i < nl; i++) read_point();
    read_point();   // the vanishing argument's random polynomial
    in.y = squeeze();
    for (int i = 0; i < npieces; i++) read_point();
    in.x = squeeze();
    if (bad) return false;
    in.inst_ev.resize(pk.instance_queries.size());
    in.adv_ev.resize(pk.advice_queries.size());
    in.fix_ev.resize(pk.fixed_queries.size());
    for (auto& v : in.inst_ev) v = read_scalar();
    for (auto& v : in.adv_ev) v = read_scalar();
    for (auto& v : in.fix_ev) v = read_scalar();
    in.rand_ev = read_scalar();
    in.sig_ev.resize(m);
    for (auto& v : in.sig_ev) v = read_scalar();
    in.pz0.resize(nsets), in.pz1.resize(nsets), in.pzl.assign(nsets, fe_zero<SF>());
    for (int i = 0; i < nsets; i++) {
        in.pz0[i] = read_scalar();
        in.pz1[i] = read_scalar();
        if (i != nsets - 1) in.pzl[i] = read_scalar();
    }
    in.lz0.resize(nl), in.lz1.resize(nl), in.la0.resize(nl), in.lam1.resize(nl), in.ls0.resize(nl);
    for (int i = 0; i < nl; i++) {
        in.lz0[i] = read_scalar();
        in.lz1[i] = read_scalar();
        in.la0[i] = read_scalar();
        in.lam1[i] = read_scalar();
        in.ls0[i] = read_scalar();
    }
    if (bad) return false;
    in.x1 = squeeze();
    in.x2 = squeeze();
    read_point();   // multiopen: f
    in.x3 = squeeze();
    in.q_evals.resize(pk.rot_sets.size());
    for (auto& v : in.q_evals) v = read_scalar();
    if (bad) return false;
    in.x4 = squeeze();
    // the opening argument: S, xi, z, (L_j, R_j, u_j), c, f
    read_point();
    in.xi = squeeze();
    in.z = squeeze();
    in.us.resize(k);
    for (unsigned j = 0; j < k; j++) {
        read_point();
        read_point();
        in.us[j] = squeeze();
        if (fe_is_zero(in.us[j])) bad = true;
    }
    if (bad || off + 64 != len) return false;
    uint64_t cl[4], fl[4];
    memcpy(cl, proof + off, 32);
    memcpy(fl, proof + off + 32, 32);
    const Fe<SF> cc = fe_from_u64<SF>(cl), ff = fe_from_u64<SF>(fl);
    if (!is_canonical(cc) || !is_canonical(ff)) return false;
    in.cm = fe_to_mont(cc), in.fm = fe_to_mont(ff);
    VpHostEval<SF> ev;
    VpOut<Fe<SF>> lc;
    if (!vp_body(ev, pk, in, nl_cap, lc) || ev.reject) return false;
    // G_0, U, W are the first and the last two SRS points: supplied by the caller right after this table
    out.lc_pts.assign(nl_cap * 8, 0);
    out.lc_scal.assign(nl_cap * 4, 0);
    for (size_t o = 0; o < lc.terms.size(); o++) {
        const uint32_t kind = lc.pts[o] >> 28, idx = lc.pts[o] & 0x0fffffffu;
        const uint64_t* pt = kind == VP_PT_PROOF ? &pts[(size_t)idx * 8]
                             : kind == VP_PT_FIXED ? &pk.fixed_commitments[8 * (size_t)idx]
                             : kind == VP_PT_SIGMA ? &pk.sigma_commitments[8 * (size_t)idx]
                                                   : inst_xy + 8 * (size_t)idx;
        memcpy(&out.lc_pts[o * 8], pt, 64);
        fe_to_u64<SF>(&out.lc_scal[o * 4], fe_from_mont(lc.terms[o]));
    }
    // scalars of G_0 (-v), U (-c b0 z), W (-f): points filled in by the caller (slots nl_cap-3 .. nl_cap-1)
    for (int i = 0; i < 3; i++) fe_to_u64<SF>(&out.lc_scal[(nl_cap - 3 + i) * 4], fe_from_mont(lc.tail[i]));
    out.cu.assign((size_t)(k + 1) * 4, 0);
    for (unsigned j = 0; j <= k; j++) fe_to_u64<SF>(&out.cu[j * 4], fe_from_mont(lc.cu[j]));
    out.ok = true;
    return true;
}
