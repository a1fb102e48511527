// TEST HELPER (stand-alone host program, no GPU): the lane bodies of csrc/ipa_scalars.hpp -- what k_ipa_head_scalars and
// k_ipa_round_scalars run one lane per proof for bzh_ipa_open_batch_device -- lane by lane over exact-size heap buffers, against
// the arithmetic the host-transcript opening does between its rounds (csrc/ipa.hip, IpaHostDriver: fe_mul, fe_add,
// h_batch_invert), word for word, for both Pasta scalar fields and both operand forms.  The round challenges are 1, 2, p - 1, a
// random value and 0: the zero lane is the only place the status flag can be exercised -- status != 0, u^-1 = 0, f unchanged.
// tests/test_ipa_open_device_cpu.py builds it with the host's address and undefined-behaviour sanitizers and runs it.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#include "ipa_scalars.hpp"
using namespace bzh;

template <class P>
static Fe<P> rnd(std::mt19937_64& rng) {   // a random element, Montgomery form
    uint64_t l[4] = {rng(), rng(), rng(), rng() >> 4};   // below 2^252 < p
    return fe_to_mont(fe_from_u64<P>(l));
}
template <class P>
static bool same(const Fe<P>& a, const Fe<P>& b) {
    return memcmp(a.l, b.l, 32) == 0;
}
template <class P>
static Fe<P>* alloc(size_t count) {   // exact size: a lane that reads or writes past its vector is caught
    return (Fe<P>*)malloc(count * sizeof(Fe<P>));
}

template <class P>
static int run(int form, unsigned seed, size_t* lanes_run) {
    std::mt19937_64 rng(seed * 10 + form);
    const bool canonical = form == BZH_FORM_CANONICAL;
    constexpr size_t B = 5, ZERO = 4;   // lane 4 gets the zero challenge in every round
    const unsigned k = 3;
    const size_t n = 1u << k, nrand = n + 1 + 2 * k;
    int bad = 0;
    Fe<P> minus_one = fe_neg(fe_one<P>());
    Fe<P>* rands = alloc<P>(B * nrand);
    Fe<P>* hc = alloc<P>(B * kHc);
    Fe<P>* f = alloc<P>(B);
    Fe<P>* ch = alloc<P>(2 * B);
    Fe<P>* blinds = alloc<P>(B);
    Fe<P>* x3s = alloc<P>(B);
    uint8_t* status = (uint8_t*)malloc(B);
    for (size_t i = 0; i < B * nrand; i++) rands[i] = rnd<P>(rng);
    for (size_t i = 0; i < B * kHc; i++) hc[i] = rnd<P>(rng);
    std::vector<Fe<P>> blind_m(B), x3_m(B), want_f(B);
    for (size_t b = 0; b < B; b++) {
        blind_m[b] = rnd<P>(rng), x3_m[b] = rnd<P>(rng);
        blinds[b] = canonical ? fe_from_mont(blind_m[b]) : blind_m[b];
        x3s[b] = canonical ? fe_from_mont(x3_m[b]) : x3_m[b];
        status[b] = 0xff;
        f[b] = rnd<P>(rng);
    }
    // the start of a call: x3 into hc[0], the status byte cleared
    for (size_t b = 0; b < B; b++) ipa_x3_lane<P>(b, x3s, canonical, hc, status), ++*lanes_run;
    for (size_t b = 0; b < B; b++)
        if (!same(hc[b * kHc], x3_m[b]) || status[b] != 0) bad |= 1;
    // head: xi, z and the start of f, as IpaHostDriver::head
    for (size_t i = 0; i < 2 * B; i++) ch[i] = rnd<P>(rng);
    for (size_t b = 0; b < B; b++) ipa_head_lane<P>(b, B, ch, rands, nrand, n, blinds, canonical, hc, f), ++*lanes_run;
    for (size_t b = 0; b < B; b++) {
        const Fe<P> xi = ch[b];
        want_f[b] = fe_add(fe_mul(rands[b * nrand + n], xi), blind_m[b]);
        if (!same(hc[b * kHc + 1], xi) || !same(hc[b * kHc + 2], ch[B + b]) || !same(f[b], want_f[b]) || !same(hc[b * kHc], x3_m[b])) bad |= 2;
    }
    // rounds: u = 1, 2, p - 1, random, 0
    for (unsigned j = 0; j < k; j++) {
        std::vector<Fe<P>> us = {fe_one<P>(), fe_add(fe_one<P>(), fe_one<P>()), minus_one, rnd<P>(rng), fe_zero<P>()};
        for (size_t b = 0; b < B; b++) ch[b] = us[b];
        const Fe<P> f_zero_before = f[ZERO];
        for (size_t b = 0; b < B; b++) ipa_round_lane<P>(b, ch, rands, nrand, n, j, hc, f, status), ++*lanes_run;
        // the host path: one batch inversion; a zero among the challenges makes it refuse (BZH_E_ARG there)
        std::vector<Fe<P>> with_zero = us;
        if (h_batch_invert(with_zero.data(), B)) bad |= 4;
        std::vector<Fe<P>> us_inv(us.begin(), us.begin() + ZERO);
        if (!h_batch_invert(us_inv.data(), ZERO)) bad |= 4;
        for (size_t b = 0; b < ZERO; b++) {
            want_f[b] = fe_add(want_f[b], fe_add(fe_mul(rands[b * nrand + n + 1 + 2 * j], us_inv[b]), fe_mul(rands[b * nrand + n + 2 + 2 * j], us[b])));
            if (!same(hc[b * kHc + 3], us[b]) || !same(hc[b * kHc + 4], us_inv[b]) || !same(f[b], want_f[b]) || status[b] != 0) bad |= 8;
            if (!same(fe_mul(hc[b * kHc + 4], us[b]), fe_one<P>())) bad |= 8;
        }
        // the zero lane: flagged, u^-1 = 0, f as it was (the l_j term adds nothing, and neither does r_j * 0)
        if (status[ZERO] == 0 || !fe_is_zero(hc[ZERO * kHc + 3]) || !fe_is_zero(hc[ZERO * kHc + 4]) || !same(f[ZERO], f_zero_before)) bad |= 16;
    }
    // the flag is sticky, and the rounds left x3 alone
    if (status[ZERO] == 0) bad |= 16;
    for (size_t b = 0; b < B; b++)
        if (!same(hc[b * kHc], x3_m[b])) bad |= 16;
    // tail: (c, f) for the transcript and v in `form`
    Fe<P>* p = alloc<P>(B);
    Fe<P>* v = alloc<P>(B);
    Fe<P>* cf = alloc<P>(2 * B);
    Fe<P>* out_v = alloc<P>(B);
    for (size_t b = 0; b < B; b++) p[b] = rnd<P>(rng), v[b] = rnd<P>(rng);
    for (size_t b = 0; b < B; b++) ipa_tail_lane<P>(b, p, f, v, canonical, cf, out_v), ++*lanes_run;
    for (size_t b = 0; b < B; b++)
        if (!same(cf[2 * b], p[b]) || !same(cf[2 * b + 1], f[b]) || !same(out_v[b], canonical ? fe_from_mont(v[b]) : v[b])) bad |= 32;
    free(rands), free(hc), free(f), free(ch), free(blinds), free(x3s), free(status), free(p), free(v), free(cf), free(out_v);
    if (bad) printf("FAIL field %d form %d: %d\n", FieldInfo<P>::id, form, bad);
    return bad;
}

int main() {
    int bad = 0;
    size_t lanes = 0;
    for (unsigned seed = 1; seed <= 4; seed++)
        for (int form = 0; form < 2; form++) bad |= run<FpParams>(form, seed, &lanes), bad |= run<FqParams>(form, 100 + seed, &lanes);
    printf("%zu lanes\n", lanes);
    printf(bad ? "ipa_scalars_check: FAILED\n" : "ipa_scalars_check: ok\n");
    return bad ? 1 : 0;
}
