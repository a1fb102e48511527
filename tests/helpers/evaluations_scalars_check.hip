// TEST HELPER (stand-alone host program, no GPU): the lane bodies of csrc/evaluations_scalars.hpp -- what k_ev_scalars and
// k_ev_export run one lane per proof or per (proof, query) for bzh_evaluations_batch_device -- lane by lane over exact-size heap
// buffers, against fe_mul / fe_sqr / fe_add / h_pow_u64 of csrc/host_field.hpp, word for word, for both Pasta scalar fields and both
// operand forms.  x is random in lane 0 and 0, 1 and p - 1 in lanes 1, 2 and 3; k = 0, 1 and 17; 1, 3 and 8 rotations; 0, 1 and 3
// pieces.  tests/test_evaluations_device_cpu.py builds it with the host's address and undefined-behaviour sanitizers and runs it.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#include "host_field.hpp"
#include "evaluations_scalars.hpp"
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
    return (Fe<P>*)malloc(count ? count * sizeof(Fe<P>) : 1);
}

template <class P>
static int run(int form, unsigned k, size_t nrot, size_t npieces, unsigned seed, size_t* lanes_run) {
    std::mt19937_64 rng(seed * 1000 + form * 100 + k);
    const bool canonical = form == BZH_FORM_CANONICAL;
    constexpr size_t B = 4;
    int bad = 0;
    auto as_form = [&](const Fe<P>& v) { return canonical ? fe_from_mont(v) : v; };
    Fe<P>* xs = alloc<P>(B);
    xs[0] = rnd<P>(rng), xs[1] = fe_zero<P>(), xs[2] = fe_one<P>(), xs[3] = fe_neg(fe_one<P>());
    // the points: x * omega^rotation from a table of omega^rotation
    const Fe<P> omega = h_omega<P>(k);
    Fe<P>* omegas = alloc<P>(nrot);
    for (size_t j = 0; j < nrot; j++) omegas[j] = h_pow_u64(omega, (uint64_t)(j * 5 + (j & 1)));
    Fe<P>* points = alloc<P>(B * nrot);
    for (size_t b = 0; b < B; b++) ev_points_lane<P>(b, xs, omegas, nrot, canonical, points), ++*lanes_run;
    for (size_t b = 0; b < B; b++)
        for (size_t j = 0; j < nrot; j++)
            if (!same(points[b * nrot + j], as_form(fe_mul(xs[b], omegas[j])))) bad |= 1;
    // x^n, n = 2^k
    Fe<P>* xn = alloc<P>(B);
    for (size_t b = 0; b < B; b++) ev_xn_lane<P>(b, xs, k, xn), ++*lanes_run;
    for (size_t b = 0; b < B; b++)
        if (!same(xn[b], h_pow_u64(xs[b], (uint64_t)1 << k))) bad |= 2;
    // h_blind = sum_i xn^i * blind_i
    Fe<P>* hb = alloc<P>(B * npieces);
    std::vector<Fe<P>> hm(B * npieces);
    for (size_t i = 0; i < B * npieces; i++) hm[i] = rnd<P>(rng), hb[i] = as_form(hm[i]);
    Fe<P>* out = alloc<P>(B);
    for (size_t b = 0; b < B; b++) ev_hblind_lane<P>(b, xn, hb, npieces, canonical, out), ++*lanes_run;
    for (size_t b = 0; b < B; b++) {
        Fe<P> acc = fe_zero<P>(), pw = fe_one<P>();
        for (size_t i = 0; i < npieces; i++) acc = fe_add(acc, fe_mul(pw, hm[b * npieces + i])), pw = fe_mul(pw, xn[b]);
        if (!same(out[b], as_form(acc))) bad |= 4;
    }
    // the export of the values
    const size_t nev = B * 3;
    Fe<P>* ev = alloc<P>(nev);
    Fe<P>* exported = alloc<P>(nev);
    for (size_t g = 0; g < nev; g++) ev[g] = g == 1 ? fe_zero<P>() : rnd<P>(rng);
    for (size_t g = 0; g < nev; g++) ev_export_lane<P>(g, ev, canonical, exported), ++*lanes_run;
    for (size_t g = 0; g < nev; g++)
        if (!same(exported[g], as_form(ev[g]))) bad |= 8;
    free(xs), free(omegas), free(points), free(xn), free(hb), free(out), free(ev), free(exported);
    if (bad) printf("FAIL field %d form %d k %u: %d\n", FieldInfo<P>::id, form, k, bad);
    return bad;
}

int main() {
    int bad = 0;
    size_t lanes = 0;
    const unsigned ks[3] = {0, 1, 17};
    const size_t nrots[3] = {1, 3, 8}, npieces[3] = {0, 1, 3};
    for (int c = 0; c < 3; c++)
        for (int form = 0; form < 2; form++)
            bad |= run<FpParams>(form, ks[c], nrots[c], npieces[c], 1 + c, &lanes), bad |= run<FqParams>(form, ks[c], nrots[c], npieces[c], 11 + c, &lanes);
    printf("%zu lanes\n", lanes);
    printf(bad ? "evaluations_scalars_check: FAILED\n" : "evaluations_scalars_check: ok\n");
    return bad ? 1 : 0;
}
