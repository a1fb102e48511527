// TEST HELPER (stand-alone host program, no GPU): the verifier's device pass without the device.  For every proof of a file
// (tests/test_verify_pass_cpu.py writes it) it runs csrc/verify_host.hpp's verify_host -- the code BZH_VERIFY_PASS_HOST runs --
// and, next to it, what BZH_VERIFY_PASS_DEVICE runs one lane per proof, on the host: the points decoded by the key's offset
// list, a host-resident transcript batch (csrc/transcript_batch.hpp) walking the key's schedule, vp_lane over the key's tape
// (csrc/verify_program.hpp) and the gather of the left side's points.  Every proof verify_host accepts must come out of the
// tape not rejected and with lc_scal, cu and the left side's points equal to verify_host's word for word; every proof
// verify_host refuses must be rejected.  Built with the host's address and undefined-behaviour sanitizers.
// File: u32 circuits; per circuit u32 length + "BZV1" key bytes, u32 points per proof's instance block, u32 proofs; per proof
// u32 expectation (1: verify_host must accept, 0: must refuse, 2: either), the instance commitments (64 bytes each, affine
// canonical), u32 length + proof bytes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <vector>

#include "ctx.hpp"
#include "host_field.hpp"
#include "transcript.hpp"
#include "transcript_batch.hpp"

// csrc/transcript.hip is linked for the transcript verify_host reads through; its write_point wants the library's compressor,
// which nothing here calls
extern "C" int bzh_affine_compress(int, const uint64_t*, size_t, int, uint8_t*) { return BZH_E_ARG; }

namespace bzh {
// (csrc/ipa.hip's, which the library links: pasta_curves from_bytes for one compressed point)
bool point_decompress(int curve, const uint8_t* in, uint64_t* xy_canonical) {
    bool ok = false;
    with_curve(curve, [&](auto c) {
        ok = h_decompress<decltype(c)>(in, xy_canonical);
        return BZH_OK;
    });
    return ok;
}
namespace {
#include "key_shape.hpp"
#include "verifying_key.hpp"
#include "verify_host.hpp"

struct Reader32 {
    FILE* f;
    bool ok = true;
    uint32_t u32() {
        uint32_t v = 0;
        if (fread(&v, 4, 1, f) != 1) ok = false;
        return v;
    }
    std::vector<uint8_t> bytes(size_t n) {
        std::vector<uint8_t> v(n);
        if (n && fread(v.data(), 1, n, f) != n) ok = false;
        return v;
    }
};

// the device pass for one proof, on the host.  lc_scal canonical, cu canonical, lc_pts without G_0 U W; returns the reject decision
template <class C>
static bool tape_pass(const KeyShape& key, const uint64_t* inst_xy, size_t ni1, const uint8_t* proof, size_t len, std::vector<uint64_t>& lc_pts,
                      std::vector<uint64_t>& lc_scal, std::vector<uint64_t>& cu) {
    using SF = typename CurveInfo<C>::SF;
    const VerifyTape& vp = key.vprog;
    const size_t np = key.vp_offsets.size(), plen = vp.proof_len, pstride = (plen + 31) & ~(size_t)31, k = key.k;
    bool reject = len != plen;
    // exact-size heap buffers: a read past an end is caught
    std::vector<uint8_t> row(pstride, 0);
    if (!reject) memcpy(row.data(), proof, plen);
    std::vector<uint64_t> xy(np * 8, 0);
    std::vector<uint8_t> st(np, 0);
    for (size_t i = 0; i < np; i++) {
        uint64_t p[8];
        if (!h_decompress<C>(row.data() + key.vp_offsets[i], p)) {
            st[i] = BZH_POINT_INVALID;
            continue;
        }
        uint64_t any = 0;
        for (int w = 0; w < 8; w++) any |= p[w];
        if (!any) {
            st[i] = BZH_POINT_IDENTITY;
            continue;
        }
        memcpy(&xy[i * 8], p, 64);
    }
    for (size_t i = 0; i < np; i++) reject = reject || st[i] != BZH_POINT_OK;
    // one host-resident transcript of a batch of one
    std::vector<uint64_t> words(24, 0);
    {
        Blake2b s;
        s.init(64, reinterpret_cast<const uint8_t*>("Halo2-Transcript"));
        for (int i = 0; i < 8; i++) words[i] = s.h[i];
    }
    uint8_t tb_status = 0;
    TbState S{words.data(), words.data() + 8, &tb_status, nullptr, 1, 0};
    uint64_t t = 0;
    uint32_t buflen = 0;
    std::vector<uint32_t> ch((size_t)vp.nch * 8, 0);
    for (size_t i = 0; i + 2 < vp.schedule.size(); i += 3) {
        const uint32_t kind = vp.schedule[i], first = vp.schedule[i + 1], count = vp.schedule[i + 2];
        auto absorb_points = [&](const void* base, const uint8_t* pre) {
            tb_absorb<C, 0>(S, 0, base, count, 0, true, pre, t, buflen, 0);
            for (uint32_t c = 0; c < count; c++) tb_advance(t, buflen, 65);
        };
        auto absorb_scalars = [&](const void* base, size_t cnt) {
            tb_absorb<C, 2>(S, 0, base, cnt, 0, true, nullptr, t, buflen, 0);
            for (size_t c = 0; c < cnt; c++) tb_advance(t, buflen, 33);
        };
        switch (kind) {
            case VP_TS_VK: absorb_scalars(key.vk_repr, 1); break;
            case VP_TS_INST: absorb_points(inst_xy, nullptr); break;
            case VP_TS_POINTS: absorb_points(&xy[(size_t)first * 8], &st[first]); break;
            case VP_TS_SQUEEZE:
                tb_squeeze<C>(S, 0, t, buflen, false, &ch[(size_t)first * 8]);
                tb_advance(t, buflen, 1);
                break;
            default: absorb_scalars(row.data() + first, count);
        }
    }
    reject = reject || tb_status != BZH_POINT_OK;
    // the lane
    const size_t nl_cap = vp.nl_cap;
    std::vector<uint32_t> slots((size_t)vp.nslots * 8, 0), scal(nl_cap * 8, 0), cum((k + 1) * 8, 0), flags(1, 0);
    VerifyPassArgs a;
    a.batch = 1, a.pstride = pstride, a.d_proofs = row.data();
    a.d_ops = vp.ops.data(), a.d_consts = vp.consts.data(), a.d_ev_offsets = vp.ev_offsets.data(), a.d_out_slots = vp.out_slots.data();
    a.nops = (uint32_t)vp.nops(), a.nslots = vp.nslots, a.nch = vp.nch, a.nev = (uint32_t)vp.ev_offsets.size();
    a.nl_cap = (uint32_t)nl_cap, a.ncu = (uint32_t)(k + 1);
    a.d_ch = ch.data(), a.d_slots = slots.data(), a.d_lc_scal = scal.data(), a.d_cu = cum.data(), a.d_flags = flags.data();
    vp_lane<SF>(a, 0);
    reject = reject || flags[0] != 0;
    lc_scal.assign(nl_cap * 4, 0);
    memcpy(lc_scal.data(), scal.data(), nl_cap * 32);
    cu.assign((k + 1) * 4, 0);
    for (size_t j = 0; j <= k; j++) {
        Fe<SF> v;
        memcpy(v.l, &cum[j * 8], 32);
        fe_to_u64<SF>(&cu[j * 4], fe_from_mont(v));
    }
    lc_pts.assign(nl_cap * 8, 0);
    for (size_t o = 0; o < nl_cap; o++) {
        const uint32_t kind = vp.pt_src[o] >> 28, idx = vp.pt_src[o] & 0x0fffffffu;
        const uint64_t* p = nullptr;
        switch (kind) {
            case VP_PT_PROOF: p = &xy[(size_t)idx * 8]; break;
            case VP_PT_FIXED: p = &key.fixed_commitments[(size_t)idx * 8]; break;
            case VP_PT_SIGMA: p = &key.sigma_commitments[(size_t)idx * 8]; break;
            case VP_PT_INST: p = idx < ni1 ? inst_xy + (size_t)idx * 8 : nullptr; break;
            default: break;   // G_0 U W: the caller's, zero here as in verify_host's view
        }
        if (p) memcpy(&lc_pts[o * 8], p, 64);
    }
    return reject;
}

}  // namespace
}  // namespace bzh

int main(int argc, char** argv) {
    using namespace bzh;
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    Reader32 r{f};
    const uint32_t ncirc = r.u32();
    size_t proofs = 0, accepted = 0, bad = 0;
    for (uint32_t c = 0; c < ncirc && r.ok; c++) {
        const std::vector<uint8_t> kb = r.bytes(r.u32());
        const uint32_t ni1 = r.u32(), count = r.u32();
        bzh_vk* vk = nullptr;
        if (!r.ok || bzh_vk_read(kb.data(), kb.size(), &vk) != BZH_OK) {
            printf("FAIL circuit %u: the key does not read\n", c);
            return 1;
        }
        const KeyShape& key = vk->shape;
        const VerifyTape& vp = key.vprog;
        if (!vp.ok || key.curve != BZH_CURVE_VESTA) {
            printf("FAIL circuit %u: no tape\n", c);
            return 1;
        }
        // the last three points are the caller's G_0 U W; the schedule squeezes every challenge slot once, in order
        bool shape_ok = vp.nl_cap >= 3 && vp.out_slots.size() == vp.nl_cap + key.k + 1 && vp.pt_src.size() == vp.nl_cap;
        for (size_t i = 0; shape_ok && i < 3; i++) shape_ok = vp.pt_src[vp.nl_cap - 3 + i] == ((VP_PT_SRS << 28) | i);
        uint32_t squeezes = 0;
        for (size_t i = 0; i + 2 < vp.schedule.size(); i += 3)
            if (vp.schedule[i] == VP_TS_SQUEEZE) shape_ok = shape_ok && vp.schedule[i + 1] == squeezes++;
        shape_ok = shape_ok && squeezes == vp.nch && vp.nch == 11 + key.k;
        for (size_t i = 0; i < vp.nops() && shape_ok; i++)
            shape_ok = vp.ops[4 * i] <= VP_CONST && vp.ops[4 * i + 1] < vp.nslots &&
                       (vp.ops[4 * i] == VP_CONST ? vp.ops[4 * i + 2] < vp.consts.size() / 8 : vp.ops[4 * i + 2] < vp.nslots);
        if (!shape_ok) {
            printf("FAIL circuit %u: the tape's tables are malformed\n", c);
            bad++;
        }
        printf("circuit %u: %zu ops, %u slots, %zu constants, %zu inversions, %zu products, nl_cap %zu, proof %zu bytes\n", c, vp.nops(), vp.nslots,
               vp.consts.size() / 8, vp.n_inv, vp.n_mul, vp.nl_cap, vp.proof_len);
        for (uint32_t p = 0; p < count && r.ok; p++) {
            const uint32_t expect = r.u32();
            const std::vector<uint8_t> ib = r.bytes((size_t)ni1 * 64);
            const std::vector<uint8_t> pb = r.bytes(r.u32());
            if (!r.ok) break;
            std::vector<uint64_t> inst((size_t)ni1 * 8 + 8, 0);
            memcpy(inst.data(), ib.data(), ib.size());
            proofs++;
            ProofView<VestaCurve> view;
            const bool host_ok = verify_host<VestaCurve>(key, inst.data(), pb.data(), pb.size(), vp.nl_cap, view);
            std::vector<uint64_t> lc_pts, lc_scal, cu;
            const bool reject = tape_pass<VestaCurve>(key, inst.data(), ni1, pb.data(), pb.size(), lc_pts, lc_scal, cu);
            bool ok = expect == 2 || host_ok == (expect == 1);
            if (host_ok) {
                accepted++;
                ok = ok && !reject && lc_scal == view.lc_scal && cu == view.cu && lc_pts == view.lc_pts;
            } else {
                ok = ok && reject;
            }
            if (!ok) {
                printf("FAIL circuit %u proof %u (length %zu): verify_host %d (expected %u), tape reject %d, scalars %d, cu %d, points %d\n", c, p,
                       pb.size(), (int)host_ok, expect, (int)reject, (int)(lc_scal == view.lc_scal), (int)(cu == view.cu), (int)(lc_pts == view.lc_pts));
                bad++;
            }
        }
        bzh_vk_free(vk);
    }
    fclose(f);
    if (!r.ok || bad || !proofs) return 1;
    printf("%zu proofs, %zu accepted by verify_host\nverify_pass_check: ok\n", proofs, accepted);
    return 0;
}
