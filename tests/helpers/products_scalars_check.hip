// TEST HELPER (stand-alone host program, no GPU): the lane bodies of csrc/products_scalars.hpp -- what k_gp_finish runs once per
// workgroup (gp_carry_lane) and once per proof (gp_status_lane) for bzh_grand_products_batch_device -- lane by lane over an
// exact-size heap buffer, against fe_mul of csrc/host_field.hpp, word for word, for both Pasta scalar fields, nsets = 0, 1, 2 and
// 5 with 0 and 2 lookups.  The four proofs of a buffer: 0 closes (the last set's raw[usable] is the inverse of the product of the
// others, every lookup's is 1); 1 has random values (the sets do not close); 2 closes in its sets but not in its last lookup (in
// its last set when there is no lookup); 3 closes but for a zero raw[usable] in set 0.
// tests/test_products_device_cpu.py builds it with the host's address and undefined-behaviour sanitizers and runs it.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#include "host_field.hpp"
#include "products_scalars.hpp"
using namespace bzh;

template <class P>
static Fe<P> rnd(std::mt19937_64& rng) {   // a random non-zero element, Montgomery form
    uint64_t l[4] = {rng() | 1, rng(), rng(), rng() >> 4};   // below 2^252 < p
    return fe_to_mont(fe_from_u64<P>(l));
}

template <class P>
static int run(size_t nsets, size_t nl, unsigned seed, size_t* lanes_run) {
    std::mt19937_64 rng(seed * 1000 + nsets * 10 + nl);
    constexpr size_t B = 4, n = 8, usable = 5;
    const size_t nz = nsets + nl;
    const Fe<P> one = fe_one<P>();
    // exact size: a lane that reads past the buffer is caught
    Fe<P>* raw = (Fe<P>*)malloc((nz ? nz : 1) * B * n * sizeof(Fe<P>));
    auto at = [&](size_t p, size_t b) -> Fe<P>& { return raw[(p * B + b) * n + usable]; };
    for (size_t i = 0; i < nz * B * n; i++) raw[i] = rnd<P>(rng);
    uint8_t want_status[B] = {0, (uint8_t)(nz ? 1 : 0), (uint8_t)(nz ? 1 : 0), (uint8_t)(nsets ? 1 : 0)};
    for (size_t b = 0; b < B; b++) {
        if (b == 1) continue;
        for (size_t l = 0; l < nl; l++) at(nsets + l, b) = one;
        if (nsets) {
            Fe<P> acc = one;
            for (size_t j = 0; j + 1 < nsets; j++) acc = fe_mul(acc, at(j, b));
            at(nsets - 1, b) = fe_inv(acc);
        }
        if (b == 2 && nz) at(nz - 1, b) = fe_add(at(nz - 1, b), one);   // 2 in a lookup; in a set the chain becomes 1 + acc
        if (b == 3 && nsets) at(0, b) = fe_zero<P>();
    }
    int bad = 0;
    for (size_t b = 0; b < B; b++) {
        for (size_t p = 0; p < nz; p++) {
            Fe<P> want = one;
            if (p < nsets)
                for (size_t j = 0; j < p; j++) want = fe_mul(want, at(j, b));
            const Fe<P> got = gp_carry_lane<P>(raw, B, n, usable, p, b, nsets);
            ++*lanes_run;
            if (memcmp(got.l, want.l, 32) != 0) bad |= 1;
            if (b == 3 && p >= 1 && p < nsets && !fe_is_zero(got)) bad |= 4;   // a zero hand-over value zeroes every later set
        }
        ++*lanes_run;
        if (gp_status_lane<P>(raw, B, n, usable, b, nsets, nl) != want_status[b]) bad |= 2;
    }
    free(raw);
    if (bad) printf("FAIL field %d nsets %zu nl %zu: %d\n", FieldInfo<P>::id, nsets, nl, bad);
    return bad;
}

int main() {
    int bad = 0;
    size_t lanes = 0;
    const size_t sets[4] = {0, 1, 2, 5};
    for (size_t nsets : sets)
        for (size_t nl = 0; nl <= 2; nl += 2) bad |= run<FpParams>(nsets, nl, 1, &lanes), bad |= run<FqParams>(nsets, nl, 11, &lanes);
    printf("%zu lanes\n", lanes);
    printf(bad ? "products_scalars_check: FAILED\n" : "products_scalars_check: ok\n");
    return bad ? 1 : 0;
}
