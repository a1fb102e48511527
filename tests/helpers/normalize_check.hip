// TEST HELPER (stand-alone host program, no GPU): csrc/normalize.hpp's chain code -- what k_batch_normalize runs -- lane by lane
// over exact-size heap buffers and an unaligned out32, against h_jac_to_affine and h_compress.  tests/test_normalize_compress_cpu.py
// builds it with the host's address and undefined-behaviour sanitizers and runs it.  which: 0 = out_xy only, 1 = out32 only, 2 = both.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#include "normalize.hpp"
using namespace bzh;
template <class C>
static int run(size_t n, int form, int which) {
    using P = typename C::Base;
    std::mt19937_64 rng(n * 7 + form);
    std::vector<uint64_t> xyz(n * 12);
    for (size_t i = 0; i < n; i++)
        for (int c = 0; c < 3; c++) {
            uint64_t l[4] = {rng(), rng(), rng(), rng() >> 3};
            Fe<P> v = fe_from_u64<P>(l);   // < 2^253 < p: fine in either form
            if (c == 2 && (i % 5 == 3 || n - 1 == i)) v = fe_zero<P>();
            fe_to_u64<P>(&xyz[12 * i + 4 * c], v);
        }
    std::vector<uint64_t> want_xy(n * 8);
    std::vector<uint8_t> want_e(n * 32);
    h_jac_to_affine<P>(xyz.data(), n, form, form, want_xy.data());
    for (size_t i = 0; i < n; i++) h_compress<C>(&want_xy[8 * i], form, &want_e[32 * i]);
    uint64_t* xy = which != 1 ? (uint64_t*)malloc(n * 64) : nullptr;
    uint8_t* eraw = which != 0 ? (uint8_t*)malloc(n * 32 + 1) : nullptr;
    uint8_t* e = eraw ? eraw + 1 : nullptr;
    uint8_t* st = (uint8_t*)malloc(n);
    NormIo io{xyz.data(), xy, e, st, n, 0, 0, form == BZH_FORM_CANONICAL ? 1 : 0};
    normalize_plan(n, &io.lanes, &io.chain);
    for (size_t t = 0; t < io.lanes; t++) normalize_chain<C>(io, t);
    int bad = 0;
    if (xy && memcmp(xy, want_xy.data(), n * 64)) bad |= 1;
    if (e && memcmp(e, want_e.data(), n * 32)) bad |= 2;
    for (size_t i = 0; i < n; i++) {
        const bool inf = !(xyz[12 * i + 8] | xyz[12 * i + 9] | xyz[12 * i + 10] | xyz[12 * i + 11]);
        if (st[i] != (inf ? BZH_POINT_IDENTITY : BZH_POINT_OK)) bad |= 4;
    }
    // affine_encode on its own
    for (size_t i = 0; i < n && i < 300; i++) {
        uint8_t b[32];
        norm_store<P>(b, affine_encode(norm_load<P>(&want_xy[8 * i]), norm_load<P>(&want_xy[8 * i + 4]), form == BZH_FORM_CANONICAL));
        if (memcmp(b, &want_e[32 * i], 32)) bad |= 8;
    }
    free(xy), free(eraw), free(st);
    if (bad) printf("FAIL curve %d n %zu form %d which %d: %d\n", C::id, n, form, which, bad);
    return bad;
}
int main() {
    int bad = 0;
    const size_t ns[] = {1, 2, 7, 257, 16385, 32774};
    for (size_t n : ns)
        for (int form = 0; form < 2; form++)
            for (int which = 0; which < 3; which++) {
                bad |= run<VestaCurve>(n, form, which);
                if (n < 20000) bad |= run<PallasCurve>(n, form, which), bad |= run<Bn254Curve>(n, form, which);
            }
    printf(bad ? "normalize_check: FAILED\n" : "normalize_check: ok\n");
    return bad ? 1 : 0;
}
