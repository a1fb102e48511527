// Part of the whole-proof translation unit (csrc/prove.hip): what the PROVING key and the VERIFYING key have in common -- the
// circuit expressions as serialised, the blob reader, the registry keys, the runtime state (csrc/key_runtime.hpp), and KeyShape: the constraint
// system's shape with the multiopen structure and the key's commitments, i.e. everything the verifier reads of a key.
// bzh_pk derives from KeyShape, bzh_vk holds one.  Host code only; depends on host_field.hpp and the HIP runtime header (the
// arena).  Included inside namespace bzh { namespace { (prove_kernels.cuh opens them; tests/helpers/vk_check.hip does the same).
#pragma once
// ---------------------------------------------------------------------------
// circuit expressions (as serialised)
// ---------------------------------------------------------------------------
enum { CX_CONST = 0, CX_ADVICE = 1, CX_FIXED = 2, CX_INSTANCE = 3, CX_NEG = 4, CX_ADD = 5, CX_MUL = 6, CX_SCALE = 7 };
struct CNode {
    uint8_t tag;
    uint32_t col = 0;
    int32_t rot = 0;
    uint32_t val[8] = {0};  // Montgomery
    int a = -1, b = -1;
};

// registry keys
enum { K_ADV = 1, K_FIX, K_INST, K_SIGMA, K_IDENT, K_PZ, K_LA, K_LS, K_LZ, K_MISC, K_HOIST };
enum { M_L0, M_LLAST, M_LBLIND, M_X, M_TINV, M_AC, M_SC, M_A, M_S, M_ACC, M_Q, M_R, M_F, M_H0 /* + i */ };
static inline uint64_t key(int kind, uint64_t i) { return ((uint64_t)kind << 32) | i; }

// the device arena and the per-key runtime state (mutex, arenas, call count)
#include "key_runtime.hpp"

struct Reader {
    const uint8_t* p;
    const uint8_t* end;
    bool ok = true;
    uint32_t u32() {
        if (end - p < 4) {
            ok = false;
            return 0;
        }
        uint32_t v;
        memcpy(&v, p, 4);
        p += 4;
        return v;
    }
    uint8_t u8() {
        if (end - p < 1) {
            ok = false;
            return 0;
        }
        return *p++;
    }
    const uint8_t* bytes(size_t n) {
        if ((size_t)(end - p) < n) {
            ok = false;
            return nullptr;
        }
        const uint8_t* r = p;
        p += n;
        return r;
    }
};

// the host pass as a tape (BZH_VERIFY_PASS_DEVICE): VerifyTape, its interpreter, and -- for this file -- its compiler
#define BZH_VP_WITH_COMPILER 1
#include "verify_program.hpp"

// ---------------------------------------------------------------------------
// the part of a key the verifier reads (verify_host, verify_batch_t): fixed by the constraint-system part of the circuit blob,
// except for the two commitment lists, which keygen computes against an SRS
// ---------------------------------------------------------------------------
struct KeyShape {
    int curve = 0, field = 0;
    unsigned k = 0, ek = 0;   // ek: log2 of the extended domain (degree - 1 pieces of n coefficients fit in it)
    size_t n = 0;
    int na = 0, nf = 0, ni = 0, degree = 0, bf = 0, chunk_len = 0, nsets = 0, nl = 0, npieces = 0;
    size_t usable = 0;
    uint64_t vk_repr[4] = {0};
    std::vector<CNode> cx;
    std::vector<int> gates;
    std::vector<std::pair<int, int>> perm_columns;  // (kind tag CX_*, index)
    std::vector<std::pair<std::vector<int>, std::vector<int>>> lookups;
    std::vector<std::pair<int, int>> advice_queries, fixed_queries, instance_queries;
    uint64_t omega[4] = {0};  // Montgomery limbs for ntt_run
    uint32_t delta[8] = {0};  // Montgomery
    // multiopen structure: rotation sets and the commitments grouped under each
    std::vector<std::vector<int>> rot_sets;
    std::vector<std::vector<uint64_t>> groups;
    std::vector<uint32_t> vp_offsets;   // byte offset of every point of a proof, in read order (verify_point_offsets)
    VerifyTape vprog;                   // the host pass as a scalar program (verify_program.hpp): host memory, derived like the above
    // commitments to the fixed and permutation polynomials, blind 1: affine canonical x || y
    std::vector<uint64_t> fixed_commitments, sigma_commitments;

    bool vk_repr_is_placeholder() const { return vk_repr[0] == BZH_VK_REPR_PLACEHOLDER && !vk_repr[1] && !vk_repr[2] && !vk_repr[3]; }
    size_t max_proof_bytes() const {
        const size_t points = (size_t)na + 2 * nl + nsets + nl + 1 + npieces + 1 + 1 + 2 * (size_t)k;
        const size_t scalars = instance_queries.size() + advice_queries.size() + fixed_queries.size() + 1 + perm_columns.size() +
                               3 * (size_t)nsets + 5 * (size_t)nl + rot_sets.size() + 2;
        return 32 * (points + scalars);
    }
};

static int cx_degree(const KeyShape& pk, int i) {
    const CNode& e = pk.cx[i];
    switch (e.tag) {
        case CX_CONST: return 0;
        case CX_ADVICE:
        case CX_FIXED:
        case CX_INSTANCE: return 1;
        case CX_NEG:
        case CX_SCALE: return cx_degree(pk, e.a);
        case CX_ADD: return std::max(cx_degree(pk, e.a), cx_degree(pk, e.b));
        default: return cx_degree(pk, e.a) + cx_degree(pk, e.b);
    }
}
struct Query3 {
    int tag, col, rot;
    bool operator==(const Query3& o) const { return tag == o.tag && col == o.col && rot == o.rot; }
};
static void cx_queries(const KeyShape& pk, int i, std::vector<Query3>& out) {
    const CNode& e = pk.cx[i];
    if (e.tag >= CX_ADVICE && e.tag <= CX_INSTANCE) {
        const Query3 q{e.tag, (int)e.col, e.rot};
        if (std::find(out.begin(), out.end(), q) == out.end()) out.push_back(q);
    } else if (e.tag == CX_NEG || e.tag == CX_SCALE) {
        cx_queries(pk, e.a, out);
    } else if (e.tag == CX_ADD || e.tag == CX_MUL) {
        cx_queries(pk, e.a, out);
        cx_queries(pk, e.b, out);
    }
}

template <class SF>
static int parse_expr(Reader& r, KeyShape& pk, int depth = 0) {
    if (depth > 4096) {
        r.ok = false;
        return -1;
    }
    CNode nd;
    nd.tag = r.u8();
    if (!r.ok) return -1;
    switch (nd.tag) {
        case CX_CONST: {
            const uint8_t* b = r.bytes(32);
            if (!b) return -1;
            const Fe<SF> v = h_from_bytes<SF>(b);
            memcpy(nd.val, v.l, 32);
            break;
        }
        case CX_ADVICE:
        case CX_FIXED:
        case CX_INSTANCE:
            nd.col = r.u32();
            nd.rot = (int32_t)r.u32();
            if ((nd.tag == CX_ADVICE && nd.col >= (uint32_t)pk.na) || (nd.tag == CX_FIXED && nd.col >= (uint32_t)pk.nf) ||
                (nd.tag == CX_INSTANCE && nd.col >= (uint32_t)pk.ni))
                r.ok = false;
            break;
        case CX_NEG: nd.a = parse_expr<SF>(r, pk, depth + 1); break;
        case CX_ADD:
        case CX_MUL:
            nd.a = parse_expr<SF>(r, pk, depth + 1);
            nd.b = parse_expr<SF>(r, pk, depth + 1);
            break;
        case CX_SCALE: {
            nd.a = parse_expr<SF>(r, pk, depth + 1);
            const uint8_t* b = r.bytes(32);
            if (!b) return -1;
            const Fe<SF> v = h_from_bytes<SF>(b);
            memcpy(nd.val, v.l, 32);
            break;
        }
        default: r.ok = false;
    }
    if (!r.ok) return -1;
    pk.cx.push_back(nd);
    return (int)pk.cx.size() - 1;
}

// Byte offsets of the points of a proof, in the order verify_host reads them.  They depend on the key only: the counts below
// are the ones verify_host reads with, and its read_point checks every offset it arrives at against this list.
static std::vector<uint32_t> verify_point_offsets(const KeyShape& pk) {
    std::vector<uint32_t> offs;
    size_t off = 0;
    auto points = [&](size_t c) {
        for (; c; c--, off += 32) offs.push_back((uint32_t)off);
    };
    auto scalars = [&](size_t c) { off += 32 * c; };
    const size_t nl = (size_t)pk.nl, nsets = (size_t)pk.nsets;
    points((size_t)pk.na);          // advice
    points(2 * nl);                 // permuted lookup inputs and tables
    points(nsets);                  // permutation products
    points(nl);                     // lookup products
    points(1);                      // the vanishing argument's random polynomial
    points((size_t)pk.npieces);     // h pieces
    scalars(pk.instance_queries.size() + pk.advice_queries.size() + pk.fixed_queries.size() + 1 + pk.perm_columns.size());
    scalars(nsets ? 3 * nsets - 1 : 0);
    scalars(5 * nl);
    points(1);                      // multiopen: f
    scalars(pk.rot_sets.size());
    points(1);                      // the opening's S
    points(2 * (size_t)pk.k);       // L_j, R_j
    return offs;
}

// A circuit blob (format: csrc/prove.hip) is read in three steps -- shape_parse_head, the copy constraints and the fixed
// assignment (keygen only: pk_parse_t; bzh_vk_read requires both to be empty), shape_parse_tail.
struct ShapeHead {
    bool explicit_queries = false;   // "BZC2": the blob carries the query lists
    int min_degree = 0;
    uint32_t nperm = 0;
};
// header, gates, permutation columns, lookups
template <class C>
static int shape_parse_head(Reader& r, KeyShape& pk, ShapeHead& h) {
    using SF = typename CurveInfo<C>::SF;
    using FM = FieldInfo<SF>;
    const uint32_t magic = r.u32();
    if (magic != 0x31435A42u && magic != 0x32435A42u) return BZH_E_ARG;  // "BZC1" / "BZC2"
    h.explicit_queries = magic == 0x32435A42u;
    pk.curve = C::id;
    pk.field = FM::id;
    pk.k = r.u32();
    pk.na = (int)r.u32();
    pk.nf = (int)r.u32();
    pk.ni = (int)r.u32();
    h.min_degree = (int)r.u32();
    const uint8_t* vk = r.bytes(32);
    if (!r.ok || pk.k < 1 || pk.k > 24 || pk.na > 4096 || pk.nf > 4096 || pk.ni > 4096 || pk.na < 0 || pk.nf < 0 || pk.ni < 0)
        return BZH_E_ARG;
    {   // the vk digest is a scalar of the circuit field (upstream: C::Scalar::from_bytes_wide): refuse a non-canonical one
        uint32_t w[8];
        memcpy(w, vk, 32);
        bool lt = false;
        for (int i = 7; i >= 0 && !lt; i--) {
            if (w[i] > SF::mod(i)) return BZH_E_RANGE;
            lt = w[i] < SF::mod(i);
        }
        if (!lt) return BZH_E_RANGE;
    }
    memcpy(pk.vk_repr, vk, 32);
    pk.n = (size_t)1 << pk.k;
    const uint32_t ngates = r.u32();
    for (uint32_t g = 0; g < ngates && r.ok; g++) pk.gates.push_back(parse_expr<SF>(r, pk));
    const uint32_t nperm = r.u32();
    for (uint32_t j = 0; j < nperm && r.ok; j++) {
        const int kind = r.u8() + CX_ADVICE;
        const int idx = (int)r.u32();
        if (kind > CX_INSTANCE || idx < 0 || idx >= (kind == CX_ADVICE ? pk.na : (kind == CX_FIXED ? pk.nf : pk.ni))) return BZH_E_ARG;
        pk.perm_columns.push_back({kind, idx});
    }
    const uint32_t nlk = r.u32();
    for (uint32_t l = 0; l < nlk && r.ok; l++) {
        const uint32_t m = r.u32();
        if (!m || m > 64) return BZH_E_ARG;
        std::vector<int> ins, tabs;
        for (uint32_t i = 0; i < m && r.ok; i++) ins.push_back(parse_expr<SF>(r, pk));
        for (uint32_t i = 0; i < m && r.ok; i++) tabs.push_back(parse_expr<SF>(r, pk));
        pk.lookups.push_back({ins, tabs});
    }
    if (!r.ok) return BZH_E_ARG;
    h.nperm = nperm;
    return BZH_OK;
}

// the query lists ("BZC2") and everything derived: degree, blinding factors, usable rows, the permutation argument's chunks, the
// extended domain's size, omega and delta, the multiopen structure, the offsets of a proof's points
template <class C>
static int shape_parse_tail(Reader& r, KeyShape& pk, const ShapeHead& h) {
    using SF = typename CurveInfo<C>::SF;
    using FM = FieldInfo<SF>;
    const size_t n = pk.n;
    // shape: queries, degree, blinding factors (upstream ConstraintSystem).  "BZC2" carries the query lists in
    // upstream's registration order (a query is registered when it is made: `enable_equality` registers the column's
    // current-row query at once, before any gate of the reference's configure functions -- src/chips/board.rs:199,217
    // before :275); "BZC1" derives them in first-use order: gates, lookups, then the permutation columns.
    std::vector<Query3> used, qs;
    for (int g : pk.gates) cx_queries(pk, g, used);
    for (auto& lk : pk.lookups) {
        for (int e : lk.first) cx_queries(pk, e, used);
        for (int e : lk.second) cx_queries(pk, e, used);
    }
    for (auto& pc : pk.perm_columns) {
        const Query3 q{pc.first, pc.second, 0};
        if (std::find(used.begin(), used.end(), q) == used.end()) used.push_back(q);
    }
    if (h.explicit_queries) {
        const int tags[3] = {CX_ADVICE, CX_FIXED, CX_INSTANCE};
        const int limits[3] = {pk.na, pk.nf, pk.ni};
        for (int t = 0; t < 3; t++) {
            const uint32_t nq = r.u32();
            if (!r.ok || nq > 65536) return BZH_E_ARG;
            for (uint32_t i = 0; i < nq && r.ok; i++) {
                const Query3 q{tags[t], (int)r.u32(), (int)r.u32()};
                if (q.col < 0 || q.col >= limits[t] || q.rot < -(int)n || q.rot > (int)n) return BZH_E_ARG;
                if (std::find(qs.begin(), qs.end(), q) != qs.end()) return BZH_E_ARG;
                qs.push_back(q);
            }
        }
        if (!r.ok) return BZH_E_ARG;
        for (auto& q : used) {   // every cell the constraint system reads must be in the lists
            if (std::find(qs.begin(), qs.end(), q) == qs.end()) return BZH_E_ARG;
        }
    } else {
        qs = used;
    }
    std::map<int, int> per_col;
    for (auto& q : qs) {
        if (q.tag == CX_ADVICE) {
            pk.advice_queries.push_back({q.col, q.rot});
            per_col[q.col]++;
        } else if (q.tag == CX_FIXED) {
            pk.fixed_queries.push_back({q.col, q.rot});
        } else {
            pk.instance_queries.push_back({q.col, q.rot});
        }
    }
    int deg = 3;
    for (int g : pk.gates) deg = std::max(deg, cx_degree(pk, g));
    for (auto& lk : pk.lookups) {
        int di = 1, dt = 1;
        for (int e : lk.first) di = std::max(di, cx_degree(pk, e));
        for (int e : lk.second) dt = std::max(dt, cx_degree(pk, e));
        deg = std::max(deg, std::max(4, 2 + di + dt));
    }
    pk.degree = std::max(deg, h.min_degree);
    int maxq = 1;
    for (auto& kv : per_col) maxq = std::max(maxq, kv.second);
    pk.bf = std::max(3, maxq) + 2;
    if ((size_t)pk.bf + 2 > n) return BZH_E_ARG;
    pk.usable = n - (size_t)(pk.bf + 1);
    pk.chunk_len = pk.degree - 2;
    unsigned bl = 0;
    for (int v = pk.degree - 2; v; v >>= 1) bl++;
    pk.ek = pk.k + std::max(1u, bl);
    if (pk.ek > FM::S) return BZH_E_RANGE;
    pk.nl = (int)pk.lookups.size();
    pk.nsets = h.nperm ? (int)((h.nperm + pk.chunk_len - 1) / pk.chunk_len) : 0;
    pk.npieces = pk.degree - 1;
    if ((size_t)pk.npieces * n > ((size_t)1 << pk.ek)) return BZH_E_ARG;

    // domain constants
    const Fe<SF> omega = h_omega(h_root_of_unity<SF>(), pk.k);
    Fe<SF> delta = fe_from_u32<SF>(FM::gen);  // gen^(2^S)
    for (unsigned i = 0; i < FM::S; i++) delta = fe_sqr(delta);
    fe_to_u64<SF>(pk.omega, omega);
    memcpy(pk.delta, delta.l, 32);

    // multiopen structure (rotations stand in for the points: distinct rotations <-> distinct points x * omega^r)
    {
        struct Q {
            uint64_t cid;
            int rot;
        };
        std::vector<Q> q;
        const size_t m = pk.perm_columns.size();
        const int last_rot = -(pk.bf + 1);
        for (auto& a : pk.instance_queries) q.push_back({key(K_INST, a.first), a.second});
        for (auto& a : pk.advice_queries) q.push_back({key(K_ADV, a.first), a.second});
        for (int i = 0; i < pk.nsets; i++) {
            q.push_back({key(K_PZ, i), 0});
            q.push_back({key(K_PZ, i), 1});
            if (i != pk.nsets - 1) q.push_back({key(K_PZ, i), last_rot});
        }
        for (int i = 0; i < pk.nl; i++) {
            q.push_back({key(K_LZ, i), 0});
            q.push_back({key(K_LA, i), 0});
            q.push_back({key(K_LS, i), 0});
            q.push_back({key(K_LA, i), -1});
            q.push_back({key(K_LZ, i), 1});
        }
        for (auto& a : pk.fixed_queries) q.push_back({key(K_FIX, a.first), a.second});
        for (size_t j = 0; j < m; j++) q.push_back({key(K_SIGMA, j), 0});
        q.push_back({key(K_MISC, M_H0), 0});
        q.push_back({key(K_MISC, M_F), 0});  // the random polynomial
        std::vector<uint64_t> order;
        std::map<uint64_t, std::vector<int>> pts_of;
        for (auto& e2 : q) {
            auto it = pts_of.find(e2.cid);
            if (it == pts_of.end()) {
                order.push_back(e2.cid);
                it = pts_of.insert({e2.cid, {}}).first;
            }
            if (std::find(it->second.begin(), it->second.end(), e2.rot) == it->second.end()) it->second.push_back(e2.rot);
        }
        for (uint64_t cid : order) {
            std::vector<int> ks = pts_of[cid];
            std::sort(ks.begin(), ks.end());
            size_t si = 0;
            for (; si < pk.rot_sets.size(); si++)
                if (pk.rot_sets[si] == ks) break;
            if (si == pk.rot_sets.size()) {
                pk.rot_sets.push_back(ks);
                pk.groups.push_back({});
            }
            pk.groups[si].push_back(cid);
        }
    }
    pk.vp_offsets = verify_point_offsets(pk);
    vp_compile<SF>(pk, pk.vprog);
    return BZH_OK;
}
