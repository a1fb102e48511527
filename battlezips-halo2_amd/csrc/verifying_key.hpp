// Part of the whole-proof translation unit (csrc/prove.hip): the VERIFYING KEY -- bzh_vk, its byte format and the host-only
// entry points (bzh_vk_read / write / info / vk_repr / device_bytes / free).  keygen_vk (bzh_vk_create), bzh_vk_from_pk and
// bzh_verify_batch_vk need the device and live in prove.hip.  Depends on csrc/key_shape.hpp only, so that
// tests/helpers/vk_check.hip can build the reader and the writer into a stand-alone program under the host sanitizers.
//
// "BZV1", this library's own format (upstream's VerifyingKey::write stores the commitments only and re-derives the constraint
// system from the Circuit type, which a C ABI cannot do).  Little-endian, no padding:
//
//   offset  size
//        0     4   magic "BZV1"
//        4     4   u32 k
//        8     4   u32 curve              (bzh_curve: 0 Vesta, 1 Pallas)
//       12    32   vk_repr                (canonical scalar; equal to the constraint-system bytes' own copy)
//       44     4   u32 placeholder flag   (1 if vk_repr is BZH_VK_REPR_PLACEHOLDER, else 0)
//       48     4   u32 num_fixed          (fixed commitments = fixed columns of the constraint system)
//       52     4   u32 num_permutation    (permutation commitments = permutation columns of the constraint system)
//       56     4   u32 cs_len
//       60    64 x num_fixed              fixed commitments, affine canonical x || y
//        .    64 x num_permutation        permutation commitments, likewise
//        .    cs_len                      the constraint system: the circuit blob ("BZC1" / "BZC2", format at the top of
//                                         csrc/prove.hip) with everything up to the copy constraints verbatim, ncopies = 0,
//                                         every fixed column's length 0, and the "BZC2" query lists verbatim
//        .     4   u32 CRC-32 (IEEE 802.3, reflected, as zlib's crc32) of every byte before it
//
// bzh_vk_read accepts exactly what bzh_vk_write produces: the lengths must add up to the input's, the header must agree with
// the constraint-system bytes, those must parse to their last byte with no copy constraint and no fixed value, the checksum
// must match (all BZH_E_ARG), and every commitment must be a point of the curve with coordinates below p (BZH_E_RANGE; the
// identity (0, 0) is not on the curve).  What the verifier derives -- rotation sets, groups, the offsets of a proof's points
// -- is rebuilt from the constraint system by the code keygen runs (shape_parse_head / shape_parse_tail).
#pragma once
}  // namespace
}  // namespace bzh

struct bzh_vk {
    bzh::KeyShape shape;
    std::vector<uint8_t> cs;   // the constraint-system bytes
    // the only mutable state (csrc/key_runtime.hpp): per-call device workspaces, one per ctx that has verified on the key, and the
    // count of running calls (bzh_vk_free refuses while it is non-zero)
    mutable bzh::KeyRuntime rt;
};

namespace bzh {
namespace {

static uint32_t crc32_ieee(const uint8_t* p, size_t len) {
    uint32_t c = 0xffffffffu;
    for (size_t i = 0; i < len; i++) {
        c ^= p[i];
        for (int b = 0; b < 8; b++) c = (c >> 1) ^ (0xedb88320u & (0u - (c & 1u)));
    }
    return ~c;
}

constexpr size_t kVkHeaderBytes = 60;

static size_t vk_bytes_len(const bzh_vk& vk) {
    return kVkHeaderBytes + 8 * (vk.shape.fixed_commitments.size() + vk.shape.sigma_commitments.size()) + vk.cs.size() + 4;
}
static void vk_write_bytes(const bzh_vk& vk, uint8_t* out) {
    const KeyShape& s = vk.shape;
    uint8_t* p = out;
    auto u32 = [&](uint32_t v) {
        memcpy(p, &v, 4);
        p += 4;
    };
    memcpy(p, "BZV1", 4);
    p += 4;
    u32(s.k);
    u32((uint32_t)s.curve);
    memcpy(p, s.vk_repr, 32);
    p += 32;
    u32(s.vk_repr_is_placeholder() ? 1u : 0u);
    u32((uint32_t)(s.fixed_commitments.size() / 8));
    u32((uint32_t)(s.sigma_commitments.size() / 8));
    u32((uint32_t)vk.cs.size());
    if (!s.fixed_commitments.empty()) memcpy(p, s.fixed_commitments.data(), s.fixed_commitments.size() * 8);
    p += s.fixed_commitments.size() * 8;
    if (!s.sigma_commitments.empty()) memcpy(p, s.sigma_commitments.data(), s.sigma_commitments.size() * 8);
    p += s.sigma_commitments.size() * 8;
    if (!vk.cs.empty()) memcpy(p, vk.cs.data(), vk.cs.size());
    p += vk.cs.size();
    u32(crc32_ieee(out, (size_t)(p - out)));
}

// the shape of a key from constraint-system bytes: a circuit blob without copy constraints and fixed values, read to its end
template <class C>
static int vk_shape_from_cs(const uint8_t* cs, size_t len, KeyShape& s) {
    Reader r{cs, cs + len};
    ShapeHead head;
    BZH_TRY(shape_parse_head<C>(r, s, head));
    if (r.u32() != 0 || !r.ok) return BZH_E_ARG;   // ncopies
    for (int f = 0; f < s.nf; f++)
        if (r.u32() != 0 || !r.ok) return BZH_E_ARG;   // length of fixed column f
    BZH_TRY(shape_parse_tail<C>(r, s, head));
    if (r.p != r.end) return BZH_E_ARG;
    // what a verification allocates per proof is linear in these: a key whose degree no circuit reaches is refused here
    if (s.degree > 4096) return BZH_E_ARG;
    return BZH_OK;
}

// canonical coordinates below p and y^2 = x^3 + b
template <class C>
static bool vk_point_ok(const uint64_t* xy) {
    using PB = typename C::Base;
    const Fe<PB> x = fe_from_u64<PB>(xy), y = fe_from_u64<PB>(xy + 4);
    if (!is_canonical(x) || !is_canonical(y)) return false;
    const Fe<PB> xm = fe_to_mont(x), ym = fe_to_mont(y);
    return fe_eq(fe_sqr(ym), fe_add(fe_mul(fe_sqr(xm), xm), fe_from_u32<PB>(C::b)));
}

static int vk_read_bytes(const uint8_t* b, size_t len, std::unique_ptr<bzh_vk>& out) {
    if (len < kVkHeaderBytes + 4 || memcmp(b, "BZV1", 4) != 0) return BZH_E_ARG;
    auto u32_at = [&](size_t off) {
        uint32_t v;
        memcpy(&v, b + off, 4);
        return v;
    };
    const uint32_t k = u32_at(4), curve = u32_at(8), flag = u32_at(44), nfix = u32_at(48), nperm = u32_at(52), cs_len = u32_at(56);
    if (k < 1 || k > 24 || (curve != BZH_CURVE_VESTA && curve != BZH_CURVE_PALLAS) || flag > 1 || nfix > 4096 || nperm > 65536) return BZH_E_ARG;
    // (every term is small: no overflow)
    if ((uint64_t)kVkHeaderBytes + 64 * ((uint64_t)nfix + nperm) + cs_len + 4 != (uint64_t)len) return BZH_E_ARG;
    if (crc32_ieee(b, len - 4) != u32_at(len - 4)) return BZH_E_ARG;
    const uint8_t* pts = b + kVkHeaderBytes;
    const uint8_t* cs = pts + 64 * ((size_t)nfix + nperm);
    std::unique_ptr<bzh_vk> vk(new bzh_vk());
    BZH_TRY(with_pasta_curve((int)curve, [&](auto c) { return vk_shape_from_cs<decltype(c)>(cs, cs_len, vk->shape); }));
    KeyShape& s = vk->shape;
    if (s.k != k || (uint32_t)s.nf != nfix || s.perm_columns.size() != nperm || memcmp(s.vk_repr, b + 12, 32) != 0 ||
        (s.vk_repr_is_placeholder() ? 1u : 0u) != flag)
        return BZH_E_ARG;
    s.fixed_commitments.resize((size_t)nfix * 8);
    s.sigma_commitments.resize((size_t)nperm * 8);
    if (nfix) memcpy(s.fixed_commitments.data(), pts, (size_t)nfix * 64);
    if (nperm) memcpy(s.sigma_commitments.data(), pts + (size_t)nfix * 64, (size_t)nperm * 64);
    bool on_curve = true;
    with_pasta_curve((int)curve, [&](auto c) {
        for (size_t i = 0; i < nfix; i++) on_curve = on_curve && vk_point_ok<decltype(c)>(&s.fixed_commitments[8 * i]);
        for (size_t i = 0; i < nperm; i++) on_curve = on_curve && vk_point_ok<decltype(c)>(&s.sigma_commitments[8 * i]);
        return BZH_OK;
    });
    if (!on_curve) return BZH_E_RANGE;
    vk->cs.assign(cs, cs + cs_len);
    out = std::move(vk);
    return BZH_OK;
}

}  // namespace
}  // namespace bzh

extern "C" {

int bzh_vk_write(const bzh_vk* vk, uint8_t* out, size_t cap, size_t* len) {
    if (!vk || !len) return BZH_E_ARG;
    *len = bzh::vk_bytes_len(*vk);
    if (!out) return BZH_OK;   // size query
    if (cap < *len) return BZH_E_ARG;
    bzh::vk_write_bytes(*vk, out);
    return BZH_OK;
}

int bzh_vk_read(const uint8_t* bytes, size_t len, bzh_vk** out) {
    if (!bytes || !out) return BZH_E_ARG;
    *out = nullptr;
    std::unique_ptr<bzh_vk> vk;
    try {
        BZH_TRY(bzh::vk_read_bytes(bytes, len, vk));
    } catch (const std::bad_alloc&) {
        return BZH_E_OOM;
    }
    *out = vk.release();
    return BZH_OK;
}

int bzh_vk_info(const bzh_vk* vk, int* curve, unsigned* k, uint32_t* num_instance, uint32_t* num_fixed_commitments,
                uint32_t* num_permutation_commitments, size_t* max_proof_bytes) {
    if (!vk) return BZH_E_ARG;
    const bzh::KeyShape& s = vk->shape;
    if (curve) *curve = s.curve;
    if (k) *k = s.k;
    if (num_instance) *num_instance = (uint32_t)s.ni;
    if (num_fixed_commitments) *num_fixed_commitments = (uint32_t)(s.fixed_commitments.size() / 8);
    if (num_permutation_commitments) *num_permutation_commitments = (uint32_t)(s.sigma_commitments.size() / 8);
    if (max_proof_bytes) *max_proof_bytes = s.max_proof_bytes();
    return BZH_OK;
}

int bzh_vk_vk_repr(const bzh_vk* vk, uint8_t* out_repr32, int* is_placeholder) {
    if (!vk) return BZH_E_ARG;
    if (out_repr32) memcpy(out_repr32, vk->shape.vk_repr, 32);
    if (is_placeholder) *is_placeholder = vk->shape.vk_repr_is_placeholder() ? 1 : 0;
    return BZH_OK;
}

int bzh_vk_device_bytes(const bzh_vk* vk, size_t* key_bytes, size_t* workspace_bytes) {
    if (!vk) return BZH_E_ARG;
    std::lock_guard<std::mutex> lk(vk->rt.mu);
    if (key_bytes) *key_bytes = 0;   // a bzh_vk has no member that could hold a device pointer
    if (workspace_bytes) *workspace_bytes = vk->rt.held_locked();
    return BZH_OK;
}

int bzh_vk_free(bzh_vk* vk) {
    if (!vk) return BZH_E_ARG;
    if (!vk->rt.retire()) return BZH_E_ARG;   // a bzh_verify_batch_vk is running out of one of the key's workspaces
    delete vk;
    return BZH_OK;
}

}  // extern "C"

namespace bzh {
namespace {
