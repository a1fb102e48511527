// TEST HELPER (stand-alone host program, no GPU): csrc/transcript_batch.hpp's step code -- what k_tb_absorb and k_tb_squeeze run --
// transcript by transcript over exact-size heap buffers, against csrc/blake2b.hpp's Blake2b fed the same bytes.  Random mixes of
// point calls, scalar calls and squeezes move the buffer fill through every byte position, the full buffer included.
// tests/test_transcript_batch_cpu.py builds it with the host's address and undefined-behaviour sanitizers and runs it.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#include "blake2b.hpp"
#include "transcript_batch.hpp"
using namespace bzh;
template <class C>
static int run(size_t batch, int form, unsigned seed) {
    using PB = typename C::Base;
    using SF = typename CurveInfo<C>::SF;
    std::mt19937_64 rng(seed * 1000 + batch * 2 + form);
    const size_t cap = 32 * 40, pstride = cap;
    uint64_t* words = (uint64_t*)calloc(24 * batch, 8);
    uint8_t* status = (uint8_t*)calloc(batch, 1);
    uint8_t* proofs = (uint8_t*)malloc(batch * pstride);
    TbState S{words, words + 8 * batch, status, proofs, batch, pstride};
    std::vector<Blake2b> ref(batch);
    std::vector<std::vector<uint8_t>> ref_proof(batch);
    for (size_t b = 0; b < batch; b++) {
        ref[b].init(64, reinterpret_cast<const uint8_t*>("Halo2-Transcript"));
        for (int i = 0; i < 8; i++) words[i * batch + b] = ref[b].h[i];
    }
    uint64_t t = 0;
    uint32_t buflen = 0;
    size_t proof_len = 0;
    bool seen[129] = {false};
    int bad = 0;
    const bool canonical = form == BZH_FORM_CANONICAL;
    for (int step = 0; step < 400; step++) {
        seen[buflen] = true;
        const int kind = (int)(rng() % 6);   // 0-3: tb_absorb's KIND, 4-5: squeeze
        if (kind >= 4) {
            uint64_t* out = (uint64_t*)malloc(batch * 32);
            for (size_t b = 0; b < batch; b++) tb_squeeze<C>(S, b, t, buflen, canonical, out + 4 * b);
            tb_advance(t, buflen, 1);
            for (size_t b = 0; b < batch; b++) {
                const uint8_t z = 0;
                ref[b].update(&z, 1);
                uint8_t d[64];
                ref[b].finalize(d);
                uint64_t want[4];
                fe_to_u64<SF>(want, h_from_u512<SF>(d), form);
                if (memcmp(want, out + 4 * b, 32)) bad |= 1;
            }
            free(out);
            continue;
        }
        const bool point = kind < 2, write = kind & 1;
        const size_t count = 1 + rng() % 3, stride = count + rng() % 2, per = point ? 8 : 4;
        if (write && proof_len + 32 * count > cap) continue;
        uint64_t* ops = (uint64_t*)malloc(batch * stride * per * 8);   // exact size: a read past an item's end is caught
        for (size_t i = 0; i < batch * stride * per; i++) ops[i] = (i % 4 == 3) ? rng() >> 3 : rng();   // every element below 2^253
        if (point && batch > 1) memset(ops + 1 * stride * per, 0, 64);   // transcript 1 absorbs the identity first
        for (size_t b = 0; b < batch; b++) {
            switch (kind) {
                case 0: tb_absorb<C, 0>(S, b, ops, count, stride, canonical, nullptr, t, buflen, proof_len); break;
                case 1: tb_absorb<C, 1>(S, b, ops, count, stride, canonical, nullptr, t, buflen, proof_len); break;
                case 2: tb_absorb<C, 2>(S, b, ops, count, stride, canonical, nullptr, t, buflen, proof_len); break;
                default: tb_absorb<C, 3>(S, b, ops, count, stride, canonical, nullptr, t, buflen, proof_len); break;
            }
            for (size_t i = 0; i < count; i++) {
                const uint64_t* src = ops + (b * stride + i) * per;
                uint8_t item[65];
                item[0] = point ? 1 : 2;
                uint64_t c[8];
                if (point) {
                    fe_to_u64<PB>(c, fe_from_u64<PB>(src, form), BZH_FORM_CANONICAL);
                    fe_to_u64<PB>(c + 4, fe_from_u64<PB>(src + 4, form), BZH_FORM_CANONICAL);
                } else {
                    fe_to_u64<SF>(c, fe_from_u64<SF>(src, form), BZH_FORM_CANONICAL);
                }
                memcpy(item + 1, c, point ? 64 : 32);
                ref[b].update(item, point ? 65 : 33);
                if (write) {
                    uint8_t e[32];
                    memcpy(e, c, 32);
                    if (point) e[31] |= (uint8_t)((c[4] & 1) << 7);
                    ref_proof[b].insert(ref_proof[b].end(), e, e + 32);
                }
            }
        }
        for (size_t i = 0; i < count; i++) tb_advance(t, buflen, point ? 65 : 33);
        if (write) proof_len += 32 * count;
        free(ops);
    }
    for (size_t b = 0; b < batch; b++) {
        if (ref[b].t0 != t || ref[b].buflen != buflen) bad |= 2;
        if (ref_proof[b].size() != proof_len || memcmp(ref_proof[b].data(), proofs + b * pstride, proof_len)) bad |= 4;
        if (status[b] != ((b == 1) ? BZH_POINT_IDENTITY : BZH_POINT_OK)) bad |= 8;
    }
    size_t fills = 0;
    for (int i = 0; i <= 128; i++) fills += seen[i];
    if (fills < 100 || !seen[128]) bad |= 16;   // the buffer fill has been (nearly) everywhere, a full buffer included
    free(words), free(status), free(proofs);
    if (bad) printf("FAIL curve %d batch %zu form %d: %d (fills %zu)\n", C::id, batch, form, bad, fills);
    return bad;
}
int main() {
    int bad = 0;
    for (size_t batch : {(size_t)1, (size_t)3})
        for (int form = 0; form < 2; form++)
            bad |= run<VestaCurve>(batch, form, 1), bad |= run<PallasCurve>(batch, form, 2), bad |= run<Bn254Curve>(batch, form, 3);
    printf(bad ? "transcript_batch_check: FAILED\n" : "transcript_batch_check: ok\n");
    return bad ? 1 : 0;
}
