// TEST HELPER (stand-alone host program, no GPU): the lane bodies of csrc/multiopen_scalars.hpp -- what k_mo_points, k_mo_blinds,
// k_mo_interpolate, k_mo_final_blind and k_mo_status run one lane per (proof, set) or per proof for bzh_multiopen_batch_device --
// lane by lane over exact-size heap buffers, against h_interpolate / h_batch_invert and fe_mul / fe_add of csrc/host_field.hpp,
// word for word, for both Pasta scalar fields and both operand forms.  Set sizes 1, 2, 3 and 8; the points of a lane are random,
// and lanes 1, 2 and 3 carry 0, 1 and p - 1 among theirs.  The last lane of every set of two or more points has two equal
// points: it is the only place the flag can be exercised -- flag set, finite output, no fault -- and the host path refuses it.
// tests/test_multiopen_device_cpu.py builds it with the host's address and undefined-behaviour sanitizers and runs it.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#include "host_field.hpp"
#include "multiopen_scalars.hpp"
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
    constexpr size_t B = 5, EQ = 4;   // lane 4 has two equal points in every set that has two
    const size_t sizes[4] = {8, 3, 2, 1};   // positions: most points first
    const size_t nsets = 4, npoints = 8;
    int bad = 0;
    const Fe<P> minus_one = fe_neg(fe_one<P>());
    // the caller's points, in `form`: point number j of proof b; set `pos` opens the point numbers 0 .. sizes[pos] - 1
    Fe<P>* points = alloc<P>(B * npoints);
    std::vector<Fe<P>> pm(B * npoints);
    for (size_t b = 0; b < B; b++)
        for (size_t j = 0; j < npoints; j++) pm[b * npoints + j] = rnd<P>(rng);
    pm[1 * npoints + 0] = fe_zero<P>(), pm[2 * npoints + 1] = fe_one<P>(), pm[3 * npoints + 0] = minus_one, pm[3 * npoints + 1] = fe_zero<P>();
    pm[EQ * npoints + 1] = pm[EQ * npoints + 0];
    for (size_t i = 0; i < B * npoints; i++) points[i] = canonical ? fe_from_mont(pm[i]) : pm[i];
    // the division's order: step t holds the sets with a t-th point
    uint32_t at[kMoMaxPoints];
    std::vector<uint32_t> pid;
    for (size_t t = 0; t < sizes[0]; t++) {
        at[t] = (uint32_t)pid.size();
        for (size_t pos = 0; pos < nsets && sizes[pos] > t; pos++) pid.push_back((uint32_t)t);
    }
    const size_t entries = pid.size();
    Fe<P>* xall = alloc<P>(entries * B);
    Fe<P>* evals = alloc<P>(entries * B);
    for (size_t e = 0; e < entries; e++)
        for (size_t b = 0; b < B; b++) mo_point_lane<P>(b, points, npoints, pid[e], canonical, xall, e * B + b), ++*lanes_run;
    for (size_t e = 0; e < entries; e++)
        for (size_t b = 0; b < B; b++)
            if (!same(xall[e * B + b], pm[b * npoints + pid[e]])) bad |= 1;
    for (size_t i = 0; i < entries * B; i++) evals[i] = rnd<P>(rng);
    // interpolation
    Fe<P>* r = alloc<P>(nsets * B * kMoMaxPoints);
    uint8_t* flags = (uint8_t*)malloc(nsets * B);
    for (size_t i = 0; i < nsets * B; i++) flags[i] = 0xff;
    for (size_t pos = 0; pos < nsets; pos++)
        for (size_t b = 0; b < B; b++)
            mo_interpolate_lane<P>(xall, evals, pos * B + b, at, B, sizes[pos], r + (pos * B + b) * kMoMaxPoints, flags + pos * B + b), ++*lanes_run;
    for (size_t pos = 0; pos < nsets; pos++)
        for (size_t b = 0; b < B; b++) {
            const size_t np = sizes[pos];
            std::vector<Fe<P>> x(np), ev(np), den(np), want(np);
            for (size_t j = 0; j < np; j++) x[j] = xall[(at[j] + pos) * B + b], ev[j] = evals[(at[j] + pos) * B + b];
            for (size_t j = 0; j < np; j++) {
                den[j] = fe_one<P>();
                for (size_t m = 0; m < np; m++)
                    if (m != j) den[j] = fe_mul(den[j], fe_sub(x[j], x[m]));
            }
            const Fe<P>* got = r + (pos * B + b) * kMoMaxPoints;
            const bool equal = b == EQ && np >= 2;
            if (h_batch_invert(den.data(), np) == equal) bad |= 2;   // the host path refuses exactly the lane with equal points
            if (flags[pos * B + b] != (equal ? 1 : 0)) bad |= 4;
            for (size_t i = np; i < kMoMaxPoints; i++)
                if (!fe_is_zero(got[i])) bad |= 8;
            if (equal) {   // finite: every word below p, i.e. a value the field arithmetic accepts back unchanged
                for (size_t i = 0; i < np; i++)
                    if (!same(fe_add(got[i], fe_zero<P>()), got[i])) bad |= 16;
                continue;
            }
            h_interpolate(x.data(), ev.data(), den.data(), np, want.data());
            for (size_t i = 0; i < np; i++)
                if (!same(got[i], want[i])) bad |= 32;
            // and r passes through the points
            for (size_t j = 0; j < np; j++) {
                Fe<P> acc = fe_zero<P>();
                for (size_t i = np; i-- > 0;) acc = fe_add(fe_mul(acc, x[j]), got[i]);
                if (!same(acc, ev[j])) bad |= 64;
            }
        }
    // blinds: Horner in x1 over a group of own and shared polynomials
    const size_t nown = 3, nshared = 2;
    const uint32_t ids[4] = {2, 4, 0, 3};   // 3 and 4 are shared
    Fe<P>* x1 = alloc<P>(B);
    Fe<P>* blinds = alloc<P>(B * nown);
    Fe<P>* sblinds = alloc<P>(nshared);
    Fe<P>* qb = alloc<P>(nsets * B);
    std::vector<Fe<P>> bm(B * nown), sm(nshared);
    for (size_t b = 0; b < B; b++) x1[b] = rnd<P>(rng);
    x1[1] = fe_zero<P>(), x1[2] = fe_one<P>(), x1[3] = minus_one;
    for (size_t i = 0; i < B * nown; i++) bm[i] = rnd<P>(rng), blinds[i] = canonical ? fe_from_mont(bm[i]) : bm[i];
    for (size_t i = 0; i < nshared; i++) sm[i] = rnd<P>(rng), sblinds[i] = canonical ? fe_from_mont(sm[i]) : sm[i];
    for (size_t s = 0; s < nsets; s++)   // set s: the first s + 1 ids
        for (size_t b = 0; b < B; b++) mo_blind_lane<P>(b, x1, blinds, nown, sblinds, ids, s + 1, canonical, qb, s * B + b), ++*lanes_run;
    for (size_t s = 0; s < nsets; s++)
        for (size_t b = 0; b < B; b++) {
            Fe<P> acc = fe_zero<P>();
            for (size_t c = 0; c <= s; c++) acc = fe_add(fe_mul(acc, x1[b]), ids[c] < nown ? bm[b * nown + ids[c]] : sm[ids[c] - nown]);
            if (!same(qb[s * B + b], acc)) bad |= 128;
        }
    // the final blind and the status byte
    Fe<P>* fb = alloc<P>(B);
    Fe<P>* pb = alloc<P>(B);
    uint8_t* ipa_st = (uint8_t*)malloc(B);
    uint8_t* status = (uint8_t*)malloc(B);
    for (size_t b = 0; b < B; b++) fb[b] = rnd<P>(rng), ipa_st[b] = b == 2 ? 1 : 0, status[b] = 0xff;
    for (size_t b = 0; b < B; b++) mo_final_blind_lane<P>(b, B, x1, fb, qb, nsets, pb), ++*lanes_run;
    for (size_t b = 0; b < B; b++) mo_status_lane(b, B, flags, nsets, ipa_st, status), ++*lanes_run;
    for (size_t b = 0; b < B; b++) {
        Fe<P> acc = fb[b];
        for (size_t s = 0; s < nsets; s++) acc = fe_add(fe_mul(acc, x1[b]), qb[s * B + b]);
        if (!same(pb[b], acc)) bad |= 256;
        if (status[b] != ((b == EQ ? 1 : 0) | (b == 2 ? 2 : 0))) bad |= 512;
    }
    free(points), free(xall), free(evals), free(r), free(flags), free(x1), free(blinds), free(sblinds), free(qb), free(fb), free(pb);
    free(ipa_st), free(status);
    if (bad) printf("FAIL field %d form %d: %d\n", FieldInfo<P>::id, form, bad);
    return bad;
}

int main() {
    int bad = 0;
    size_t lanes = 0;
    for (unsigned seed = 1; seed <= 4; seed++)
        for (int form = 0; form < 2; form++) bad |= run<FpParams>(form, seed, &lanes), bad |= run<FqParams>(form, 100 + seed, &lanes);
    printf("%zu lanes\n", lanes);
    printf(bad ? "multiopen_scalars_check: FAILED\n" : "multiopen_scalars_check: ok\n");
    return bad ? 1 : 0;
}
