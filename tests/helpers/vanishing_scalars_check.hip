// TEST HELPER (stand-alone host program, no GPU): the lane body of csrc/vanishing_scalars.hpp -- what k_vn_consts runs one lane per
// (proof, constant) for bzh_vanishing_batch_device -- lane by lane over exact-size heap buffers, against fe_mul / h_pow_u64 of
// csrc/host_field.hpp, word for word, for both Pasta scalar fields, both operand forms and both table formats (8 saturated words;
// the 12-word slot against fe29_from_sat_reduced of the host result).  The challenges are random in proof 0 and 0, 1 and p - 1 in
// proofs 1, 2 and 3; the exponents 0, 1, 2, 63 and 64 on every challenge, one beta * value entry and one literal.
// tests/test_vanishing_device_cpu.py builds it with the host's address and undefined-behaviour sanitizers and runs it.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#include "host_field.hpp"
#include "vanishing_scalars.hpp"
using namespace bzh;

template <class P>
static Fe<P> rnd(std::mt19937_64& rng) {   // a random element, Montgomery form
    uint64_t l[4] = {rng(), rng(), rng(), rng() >> 4};   // below 2^252 < p
    return fe_to_mont(fe_from_u64<P>(l));
}

template <class P>
static int run(int form, bool planes29, unsigned seed, size_t* lanes_run) {
    std::mt19937_64 rng(seed * 100 + form * 10 + (planes29 ? 1 : 0));
    const bool canonical = form == BZH_FORM_CANONICAL;
    constexpr size_t B = 4;
    const uint32_t exps[5] = {0, 1, 2, 63, 64};
    std::vector<VnConst> descs;
    const Fe<P> one = fe_one<P>(), dj = rnd<P>(rng), lit = rnd<P>(rng);
    auto push = [&](int32_t ch, uint32_t e, const Fe<P>& v) {
        VnConst d{};
        d.challenge = ch, d.exponent = e;
        memcpy(d.value, v.l, 32);
        descs.push_back(d);
    };
    for (int32_t ch = 0; ch < 4; ch++)
        for (uint32_t e : exps) push(ch, e, one);
    push(1, 1, dj);      // beta * delta^j
    push(-1, 0, lit);    // a literal: its exponent and the challenges do not matter
    push(-1, 64, lit);
    const size_t nc = descs.size();
    // exact sizes: a lane that reads or writes past its vector is caught
    VnConst* dd = (VnConst*)malloc(nc * sizeof(VnConst));
    memcpy(dd, descs.data(), nc * sizeof(VnConst));
    Fe<P>* ch[4];
    std::vector<Fe<P>> chm[4];
    for (int c = 0; c < 4; c++) {
        ch[c] = (Fe<P>*)malloc(B * sizeof(Fe<P>));
        chm[c] = {rnd<P>(rng), fe_zero<P>(), fe_one<P>(), fe_neg(fe_one<P>())};
        std::rotate(chm[c].begin() + 1, chm[c].begin() + 1 + c % 3, chm[c].end());   // not the same special value in every challenge
        for (size_t b = 0; b < B; b++) ch[c][b] = (canonical && c < 3) ? fe_from_mont(chm[c][b]) : chm[c][b];   // y is always Montgomery
    }
    const size_t words = planes29 ? kVnSlot29 : 8;
    uint32_t* table = (uint32_t*)malloc(B * nc * words * 4);
    memset(table, 0xa5, B * nc * words * 4);
    for (size_t g = 0; g < B * nc; g++) vn_const_lane<P>(g, dd, nc, ch[0], ch[1], ch[2], ch[3], canonical, planes29, table), ++*lanes_run;
    int bad = 0;
    for (size_t b = 0; b < B; b++)
        for (size_t i = 0; i < nc; i++) {
            const VnConst& d = descs[i];
            Fe<P> val;
            memcpy(val.l, d.value, 32);
            const Fe<P> want = d.challenge < 0 ? val : fe_mul(val, h_pow_u64(chm[d.challenge][b], d.exponent));
            const uint32_t* got = table + (b * nc + i) * words;
            if (planes29) {
                const Fe29<P> w = fe29_from_sat_reduced(want);
                if (memcmp(got, w.l, 36) != 0 || got[9] || got[10] || got[11]) bad |= 1;
            } else if (memcmp(got, want.l, 32) != 0) {
                bad |= 2;
            }
        }
    free(dd), free(table);
    for (int c = 0; c < 4; c++) free(ch[c]);
    if (bad) printf("FAIL field %d form %d planes29 %d: %d\n", FieldInfo<P>::id, form, (int)planes29, bad);
    return bad;
}

int main() {
    int bad = 0;
    size_t lanes = 0;
    for (int form = 0; form < 2; form++)
        for (int planes = 0; planes < 2; planes++)
            bad |= run<FpParams>(form, planes != 0, 1, &lanes), bad |= run<FqParams>(form, planes != 0, 11, &lanes);
    printf("%zu lanes\n", lanes);
    printf(bad ? "vanishing_scalars_check: FAILED\n" : "vanishing_scalars_check: ok\n");
    return bad ? 1 : 0;
}
