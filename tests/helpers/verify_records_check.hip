// TEST HELPER (stand-alone host program, no GPU): the lane bodies of csrc/verify_records.hpp -- what the kernels of
// bzh_verify_records_device run -- lane by lane over exact-size heap buffers.
//   vr_parse_lane against bzh_record_decode (csrc/record.hip, linked in): a record is expected to be refused exactly when decode
//     refuses it or decodes another n_inputs or another proof length than the call's; the Montgomery instance column taken back to
//     canonical form must be decode's public inputs (zeros for a refused record) and the proof row decode's proof bytes (zeros
//     for a refused record).  Records: every header field at its bounds -- proof_len 0, the key's - 1, the key's, the key's + 1,
//     the stride's room, one past it, 2^32 - 1; n_inputs 0 .. 5 and 255 against calls for 2 and 4; each reserved byte and the
//     reserved word non-zero; kind and index with every bit set, which must change nothing -- and the inputs p - 1, p, p + 1,
//     2^255, 2^256 - 1 and 0 in every position.
//   vr_add_w_lane: the identity gives W; (X l^2, Y l^3, l) + W is the same point whatever l.
//   vr_result_lane: a point against its rescaling, against another point, the identity against itself and against a point, each
//     with the reject and the pre-reject byte set and clear.
// tests/test_verify_records_cpu.py builds it for the host, and again under the host's address and undefined-behaviour sanitizers.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "verify_records.hpp"
using namespace bzh;

static const uint64_t MOD[4] = {0x992d30ed00000001ull, 0x224698fc094cf91bull, 0, 0x4000000000000000ull};   // Fp
static const size_t PLEN = 64, CAP = 80, STRIDE = BZH_RECORD_HEADER_BYTES + CAP;                              // STRIDE: a multiple of 16

static uint32_t lcg = 4242u;
static uint32_t next_word() {
    lcg = lcg * 1664525u + 1013904223u;
    return lcg;
}

// input `which`: p - 1, p, p + 1, 2^255, 2^256 - 1, 0, then seeded values below 2^254
static void input(int which, uint64_t out[4]) {
    memset(out, 0, 32);
    switch (which) {
        case 0: memcpy(out, MOD, 32), out[0] -= 1; break;
        case 1: memcpy(out, MOD, 32); break;
        case 2: memcpy(out, MOD, 32), out[0] += 1; break;
        case 3: out[3] = 0x8000000000000000ull; break;
        case 4: out[0] = out[1] = out[2] = out[3] = ~(uint64_t)0; break;
        case 5: break;
        default:
            for (int w = 0; w < 4; w++) out[w] = ((uint64_t)next_word() << 32) | next_word();
            out[3] &= 0x3fffffffffffffffull;
    }
}
static void put32(uint8_t* p, uint32_t v) { memcpy(p, &v, 4); }

struct Rec {
    uint32_t proof_len = (uint32_t)PLEN, index = 7, word3 = 0;
    uint8_t n = 4, kind = 1, r6 = 0, r7 = 0;
    int in[4] = {6, 6, 6, 6};
};
static void build(const Rec& r, uint8_t* rec) {
    memset(rec, 0, STRIDE);
    put32(rec, r.proof_len);
    rec[4] = r.n, rec[5] = r.kind, rec[6] = r.r6, rec[7] = r.r7;
    put32(rec + 8, r.index);
    put32(rec + 12, r.word3);
    for (int i = 0; i < 4; i++) {
        uint64_t v[4];
        input(r.in[i], v);
        memcpy(rec + 16 + 32 * i, v, 32);
    }
    for (size_t i = 0; i < CAP; i++) rec[BZH_RECORD_HEADER_BYTES + i] = (uint8_t)(next_word() | 1u);   // never zero: a zeroed row shows
}

static size_t lanes = 0;
// the records of one call through vr_parse_lane, every record held against bzh_record_decode
static int parse_case(const std::vector<Rec>& recs, uint32_t n_inputs) {
    using SF = FpParams;
    const size_t B = recs.size();
    uint8_t* records = (uint8_t*)malloc(B * STRIDE);
    uint32_t* inst = (uint32_t*)malloc(B * n_inputs * 32);
    uint8_t *rows = (uint8_t*)malloc(B * PLEN), *pre = (uint8_t*)malloc(B);
    memset(inst, 0xa5, B * n_inputs * 32), memset(rows, 0xa5, B * PLEN), memset(pre, 0xa5, B);
    for (size_t b = 0; b < B; b++) build(recs[b], records + b * STRIDE);
    VerifyRecordsArgs a;
    a.batch = B, a.rstride = STRIDE, a.pstride = PLEN, a.n_inputs = n_inputs, a.proof_len = (uint32_t)PLEN;
    a.d_records = records, a.d_inst = inst, a.d_rows = rows, a.d_pre = pre;
    for (size_t b = 0; b < B; b++)
        for (uint32_t i = 0; i < n_inputs; i++, lanes++) vr_parse_lane<SF>(a, b, i);
    int bad = 0;
    for (size_t b = 0; b < B; b++) {
        uint64_t pub[16] = {0};
        size_t n = 0, plen = 0;
        const uint8_t* proof = nullptr;
        const int rc = bzh_record_decode(records + b * STRIDE, STRIDE, pub, &n, &proof, &plen, nullptr, nullptr);
        const bool refused = rc != BZH_OK || n != n_inputs || plen != PLEN;
        int mine = pre[b] != (refused ? 1 : 0);
        for (uint32_t i = 0; i < n_inputs; i++) {
            Fe<SF> m;
            memcpy(m.l, inst + (b * n_inputs + i) * 8, 32);
            const Fe<SF> c = fe_from_mont(m);
            uint64_t want[4] = {0, 0, 0, 0};
            if (!refused) memcpy(want, pub + 4 * i, 32);
            if (memcmp(c.l, want, 32) != 0) mine = 1;
        }
        for (size_t i = 0; i < PLEN; i++)
            if (rows[b * PLEN + i] != (refused ? 0 : proof[i])) mine = 1;
        if (mine) printf("FAIL record %zu of a call for %u inputs (decode rc %d, n %zu, proof_len %zu, pre %u)\n", b, n_inputs, rc, n, plen, pre[b]);
        bad |= mine;
    }
    free(records), free(inst), free(rows), free(pre);
    return bad;
}

template <class PB>
static Fe<PB> seeded() {
    uint64_t v[4];
    input(6, v);
    Fe<PB> r;
    memcpy(r.l, v, 32);
    return r;
}
template <class PB>
static void put_jac(uint32_t* p, const Fe<PB>& X, const Fe<PB>& Y, const Fe<PB>& Z) {
    memcpy(p, X.l, 32), memcpy(p + 8, Y.l, 32), memcpy(p + 16, Z.l, 32);
}
// (x, y) rescaled by l: (x l^2, y l^3, l)
template <class PB>
static void put_scaled(uint32_t* p, const Fe<PB>& x, const Fe<PB>& y, const Fe<PB>& l) {
    const Fe<PB> l2 = fe_sqr(l);
    put_jac(p, fe_mul(x, l2), fe_mul(y, fe_mul(l2, l)), l);
}

static int curve_cases() {
    using C = VestaCurve;
    using PB = C::Base;
    int bad = 0;
    const Fe<PB> zero = fe_zero<PB>();
    // vr_result_lane: pairs (right, left); want: equal?
    {
        const Fe<PB> x = seeded<PB>(), y = seeded<PB>(), x2 = seeded<PB>(), l1 = seeded<PB>(), l2 = seeded<PB>();
        const size_t B = 6;
        uint32_t* sums = (uint32_t*)malloc(2 * B * 96);
        const int want[B] = {1, 0, 0, 1, 0, 0};
        put_scaled(sums + 0 * 24, x, y, l1), put_scaled(sums + (B + 0) * 24, x, y, l2);     // the same point
        put_scaled(sums + 1 * 24, x, y, l1), put_scaled(sums + (B + 1) * 24, x2, y, l2);    // another x
        put_scaled(sums + 2 * 24, x, y, l1), put_scaled(sums + (B + 2) * 24, x, fe_neg(y), l2);   // the negative
        put_jac(sums + 3 * 24, zero, zero, zero), put_jac(sums + (B + 3) * 24, x, y, zero);  // both the identity (Z = 0 decides)
        put_jac(sums + 4 * 24, zero, zero, zero), put_scaled(sums + (B + 4) * 24, x, y, l2);
        put_scaled(sums + 5 * 24, x, y, l1), put_jac(sums + (B + 5) * 24, zero, zero, zero);
        for (int rej = 0; rej < 2; rej++)
            for (int pr = 0; pr < 2; pr++) {
                uint8_t *pre = (uint8_t*)malloc(B), *reject = (uint8_t*)malloc(B), *out = (uint8_t*)malloc(2 * B);
                memset(pre, pr ? 0x80 : 0, B), memset(reject, rej, B), memset(out, 0xa5, 2 * B);
                for (size_t b = 0; b < B; b++, lanes++) vr_result_lane<C>(sums, B, b, pre, reject, out, B);
                for (size_t b = 0; b < B; b++)
                    if (out[b] != ((want[b] && !rej && !pr) ? 1 : 0) || out[B + b] != (pr ? 1 : 0)) {
                        printf("FAIL result lane %zu (reject %d, pre %d): %u %u\n", b, rej, pr, out[b], out[B + b]);
                        bad = 1;
                    }
                free(pre), free(reject), free(out);
            }
        free(sums);
    }
    // vr_add_w_lane
    {
        const Fe<PB> wx = seeded<PB>(), wy = seeded<PB>(), x = seeded<PB>(), y = seeded<PB>(), l = seeded<PB>();
        uint32_t* w = (uint32_t*)malloc(64);
        memcpy(w, wx.l, 32), memcpy(w + 8, wy.l, 32);
        const size_t B = 3;
        uint32_t* jac = (uint32_t*)malloc(B * 96);
        put_jac(jac, x, y, zero);                      // the identity, whatever X and Y hold
        put_scaled(jac + 24, x, y, fe_one<PB>());
        put_scaled(jac + 48, x, y, l);
        for (size_t b = 0; b < B; b++, lanes++) vr_add_w_lane<C>(jac, w, b);
        // the outputs are canonical: back to Montgomery form, then compared projectively by vr_result_lane
        uint32_t* sums = (uint32_t*)malloc(4 * 96);
        auto mont = [&](uint32_t* dst, const uint32_t* src) {
            for (int c = 0; c < 3; c++) {
                Fe<PB> v;
                memcpy(v.l, src + 8 * c, 32);
                if (!fe_lt_p(v)) bad = 1;              // (canonical means below p)
                v = fe_to_mont(v);
                memcpy(dst + 8 * c, v.l, 32);
            }
        };
        mont(sums, jac), put_jac(sums + 48, wx, wy, fe_one<PB>());   // identity + W against W
        mont(sums + 24, jac + 24), mont(sums + 72, jac + 48);        // (x, y) + W against its rescaling + W
        uint8_t pre[2] = {0, 0}, reject[2] = {0, 0}, out[4] = {9, 9, 9, 9};
        for (size_t b = 0; b < 2; b++, lanes++) vr_result_lane<C>(sums, 2, b, pre, reject, out, 2);
        if (out[0] != 1 || out[1] != 1) {
            printf("FAIL add_w: %u %u\n", out[0], out[1]);
            bad = 1;
        }
        free(w), free(jac), free(sums);
    }
    return bad;
}

int main() {
    int bad = 0, records = 0;
    for (uint32_t n_inputs : {2u, 4u}) {
        std::vector<Rec> recs;
        Rec base;
        base.n = (uint8_t)n_inputs;
        recs.push_back(base);
        for (uint32_t len : {0u, (uint32_t)PLEN - 1, (uint32_t)PLEN, (uint32_t)PLEN + 1, (uint32_t)CAP, (uint32_t)CAP + 1, 0xffffffffu}) {
            Rec r = base;
            r.proof_len = len;
            recs.push_back(r);
        }
        for (int n : {0, 1, 2, 3, 4, 5, 255}) {
            Rec r = base;
            r.n = (uint8_t)n;
            recs.push_back(r);
        }
        {
            Rec r = base;
            r.r6 = 1, recs.push_back(r);
            r = base, r.r7 = 0x80, recs.push_back(r);
            r = base, r.word3 = 1, recs.push_back(r);
            r = base, r.word3 = 0x80000000u, recs.push_back(r);
            r = base, r.kind = 255, r.index = 0xffffffffu, recs.push_back(r);   // the caller's tags: ignored
            r = base, r.kind = 0, r.index = 0, recs.push_back(r);
        }
        for (int pos = 0; pos < 4; pos++)
            for (int which = 0; which < 6; which++) {
                Rec r = base;
                r.in[pos] = which;   // (a position past n_inputs is not an input: it must not matter)
                recs.push_back(r);
            }
        {
            Rec r = base;   // every input zero; every input p - 1
            for (int i = 0; i < 4; i++) r.in[i] = 5;
            recs.push_back(r);
            for (int i = 0; i < 4; i++) r.in[i] = 0;
            recs.push_back(r);
        }
        while (recs.size() < 70) recs.push_back(base);   // more records than a wave has lanes
        records += (int)recs.size();
        bad |= parse_case(recs, n_inputs);
    }
    bad |= curve_cases();
    printf("%d records, %zu lanes\n", records, lanes);
    printf(bad ? "verify_records_check: FAILED\n" : "verify_records_check: ok\n");
    return bad ? 1 : 0;
}
