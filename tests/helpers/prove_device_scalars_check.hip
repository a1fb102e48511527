// TEST HELPER (stand-alone host program, no GPU): the lane bodies of csrc/prove_device_scalars.hpp -- what k_pd_blinds runs once
// per (proof, opened polynomial) (pd_blind_lane) and k_pd_status once per proof (pd_status_lane) for bzh_prove_batch_device --
// lane by lane over exact-size heap buffers, against a plain loop over hand-made tables.  The blind-table cases: the chain's six
// runs (instance with a null pointer = Montgomery 1, advice, random, grand products, lookups, h) with every count, among them
// ni = 0 and nl = 0, per-proof strides, and strides of 0 (every proof reads the same elements); batches of 1, 3 and 70 (more lanes
// than a wave).  The status fold: all 16 combinations of flagged leaves, each with the byte 1, with a byte whose high bits alone
// are set (0x80, 0xf0) and with 0xff, at a leaf pitch equal to the batch (16) and above it (70 in rows of 80).
// tests/test_prove_device_cpu.py builds it for the host, and again under the host's address and undefined-behaviour sanitizers.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "host_field.hpp"
#include "prove_device_scalars.hpp"
using namespace bzh;

static uint32_t lcg = 12345u;
static uint32_t next_word() {
    lcg = lcg * 1664525u + 1013904223u;
    return lcg;
}

template <class P>
static int blinds_case(size_t batch, const size_t counts[6], const bool shared[6], size_t* lanes) {
    size_t nown = 0;
    for (int s = 0; s < 6; s++) nown += counts[s];
    if (!nown) return 0;
    PdBlindSrc* srcs = (PdBlindSrc*)malloc(6 * sizeof(PdBlindSrc));
    std::vector<uint32_t*> bufs(6, nullptr);
    size_t first = 0;
    for (int s = 0; s < 6; s++) {
        const size_t rows = shared[s] ? 1 : batch, words = rows * counts[s] * 8;
        if (s > 0) {   // (run 0 is the instance columns: no array, Montgomery 1)
            bufs[s] = (uint32_t*)malloc(words ? words * 4 : 4);   // exact size: a lane that reads past its run is caught
            for (size_t i = 0; i < words; i++) bufs[s][i] = next_word();
        }
        srcs[s] = PdBlindSrc{bufs[s], shared[s] ? 0 : (uint64_t)counts[s], (uint32_t)first, (uint32_t)counts[s]};
        first += counts[s];
    }
    uint32_t* out = (uint32_t*)malloc(batch * nown * 32);
    memset(out, 0xa5, batch * nown * 32);
    for (size_t g = 0; g < batch * nown; g++, ++*lanes) pd_blind_lane<P>(g, srcs, 6, nown, out);
    // the plain loop
    int bad = 0;
    const Fe<P> one = fe_one<P>();
    for (size_t b = 0; b < batch; b++) {
        size_t j = 0;
        for (int s = 0; s < 6; s++)
            for (size_t i = 0; i < counts[s]; i++, j++) {
                const uint32_t* want = s == 0 ? one.l : bufs[s] + ((shared[s] ? 0 : b * counts[s]) + i) * 8;
                if (memcmp(out + (b * nown + j) * 8, want, 32) != 0) bad = 1;
            }
    }
    for (int s = 0; s < 6; s++) free(bufs[s]);
    free(srcs);
    free(out);
    return bad;
}

static int status_case(size_t batch, size_t pitch, uint8_t flagged, size_t* lanes) {
    uint8_t* leaf = (uint8_t*)malloc(3 * pitch + batch);   // exact size: the last row ends with the batch
    memset(leaf, 0, 3 * pitch + batch);
    uint32_t* slot = (uint32_t*)malloc(2 * batch * 4);
    memset(slot, 0xa5, 2 * batch * 4);
    int bad = 0;
    for (size_t b = 0; b < batch; b++) {
        const unsigned combo = (unsigned)(b & 15);
        for (int i = 0; i < 4; i++)
            if ((combo >> i) & 1) leaf[(size_t)i * pitch + b] = flagged;
    }
    for (size_t b = 0; b < batch; b++, ++*lanes) pd_status_lane(b, leaf, pitch, 1000u + (uint32_t)batch, slot);
    for (size_t b = 0; b < batch; b++) {
        uint32_t want = 0;
        for (int i = 0; i < 4; i++)
            if (leaf[(size_t)i * pitch + b] != 0) want |= 1u << i;
        if (want != (uint32_t)(b & 15) || slot[2 * b] != want || slot[2 * b + 1] != 1000u + (uint32_t)batch) bad = 1;
    }
    free(leaf);
    free(slot);
    return bad;
}

int main() {
    int bad = 0, cases = 0;
    size_t lanes = 0;
    const size_t shapes[5][6] = {{1, 3, 1, 5, 2, 1}, {0, 3, 1, 3, 0, 1}, {2, 11, 1, 2, 2, 1}, {0, 1, 1, 0, 0, 1}, {1, 0, 1, 1, 4, 1}};
    const bool strides[3][6] = {{false, false, false, false, false, false}, {true, true, true, true, true, true}, {false, true, false, true, false, true}};
    const size_t batches[3] = {1, 3, 70};
    for (auto& counts : shapes)
        for (auto& shared : strides)
            for (size_t batch : batches) {
                int rc = blinds_case<FpParams>(batch, counts, shared, &lanes);
                rc |= blinds_case<FqParams>(batch, counts, shared, &lanes);
                if (rc) printf("FAIL blinds case %d\n", cases);
                bad |= rc;
                cases++;
            }
    const uint8_t bytes[4] = {1, 0x80, 0xf0, 0xff};
    for (uint8_t f : bytes)
        for (size_t batch : {(size_t)16, (size_t)70}) {
            const int rc = status_case(batch, (batch + 15) & ~(size_t)15, f, &lanes);
            if (rc) printf("FAIL status case %d\n", cases);
            bad |= rc;
            cases++;
        }
    printf("%d cases, %zu lanes\n", cases, lanes);
    printf(bad ? "prove_device_scalars_check: FAILED\n" : "prove_device_scalars_check: ok\n");
    return bad ? 1 : 0;
}
