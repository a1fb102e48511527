// TEST HELPER (stand-alone host program, no GPU): the lane bodies of csrc/prove_game_scalars.hpp -- what k_pg_instances and
// k_pg_status run once per proof for bzh_prove_shots_device / bzh_prove_boards_device -- lane by lane over exact-size heap buffers.
// The instance rows are held against the arithmetic of the host's synthesize_device (csrc/circuits.hip): the canonical rows are
// the 64 bytes of the commitment followed, for Shot, by {word 0, word 1, 0, 0} of the shot and of the hit input
// (from_u128(lower_u128())); the Montgomery rows are those integers times 2^256 mod p, computed here by 256 doublings on plain
// words, which shares nothing with fe_mul.  Commitment coordinates: 0, 1, p - 1 and seeded values below p; shot and hit words with
// every bit set and with seeded bits above bit 127, which must be dropped; batches of 1, 3 and 70 (more lanes than a wave); the
// Board lanes get a null input pointer, which they must not read.  The status fold: pd_status_lane then pg_status_lane over all
// 8 x 16 combinations of synthesis word and leaf bytes, the synthesis word also with bits above its three set.
// tests/test_prove_game_cpu.py builds it for the host, and again under the host's address and undefined-behaviour sanitizers.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "host_field.hpp"
#include "prove_device_scalars.hpp"
#include "prove_game_scalars.hpp"
using namespace bzh;

static uint32_t lcg = 777u;
static uint32_t next_word() {
    lcg = lcg * 1664525u + 1013904223u;
    return lcg;
}
static uint64_t next_u64() { return ((uint64_t)next_word() << 32) | next_word(); }

// Pallas base field modulus (the circuits' field), little-endian words
static const uint64_t MOD[4] = {0x992d30ed00000001ull, 0x224698fc094cf91bull, 0, 0x4000000000000000ull};

// v * 2^256 mod p for v < p: 256 times (double, subtract p once if >= p), on five words
static void ref_to_mont(const uint64_t v[4], uint64_t out[4]) {
    uint64_t a[5] = {v[0], v[1], v[2], v[3], 0};
    for (int i = 0; i < 256; i++) {
        for (int w = 4; w > 0; w--) a[w] = (a[w] << 1) | (a[w - 1] >> 63);
        a[0] <<= 1;
        bool ge = a[4] != 0;
        if (!ge) {
            ge = true;
            for (int w = 3; w >= 0; w--)
                if (a[w] != MOD[w]) {
                    ge = a[w] > MOD[w];
                    break;
                }
        }
        if (ge) {
            uint64_t borrow = 0;
            for (int w = 0; w < 4; w++) {
                const uint64_t m = MOD[w], x = a[w], d = x - m - borrow;
                borrow = (x < m) || (x == m && borrow);
                a[w] = d;
            }
            a[4] -= borrow;
        }
    }
    memcpy(out, a, 32);
}

// coordinate `which`: 0, 1, p - 1, then seeded values below 2^254 < p
static void coordinate(int which, uint64_t out[4]) {
    out[0] = out[1] = out[2] = out[3] = 0;
    if (which == 1) out[0] = 1;
    if (which == 2) memcpy(out, MOD, 32), out[0] -= 1;
    if (which >= 3) {
        for (int w = 0; w < 4; w++) out[w] = next_u64();
        out[3] &= 0x3fffffffffffffffull;
    }
}

static int instances_case(bool shot, size_t batch, int first_coordinate, bool all_ones, size_t* lanes) {
    const size_t rows = shot ? 4 : 2, in_words = shot ? 16 : 48;
    uint32_t* cm = (uint32_t*)malloc(batch * 64);
    uint64_t* in = shot ? (uint64_t*)malloc(batch * in_words * 8) : nullptr;   // exact sizes: a lane that reads past its proof is caught
    uint32_t *mont = (uint32_t*)malloc(batch * rows * 32), *canon = (uint32_t*)malloc(batch * rows * 32);
    memset(mont, 0xa5, batch * rows * 32);
    memset(canon, 0xa5, batch * rows * 32);
    for (size_t b = 0; b < batch; b++) {
        uint64_t xy[8];
        coordinate(first_coordinate + (int)(2 * b), xy);
        coordinate(first_coordinate + (int)(2 * b) + 1, xy + 4);
        memcpy(cm + b * 16, xy, 64);
        if (shot)
            for (size_t w = 0; w < in_words; w++) in[b * in_words + w] = all_ones ? ~(uint64_t)0 : next_u64();
    }
    for (size_t b = 0; b < batch; b++, ++*lanes) pg_instance_lane(b, shot, cm, in, in_words, mont, canon);
    int bad = 0;
    for (size_t b = 0; b < batch; b++) {
        // the host's synthesize_device: the commitment's 64 bytes, then from_u128(lower_u128()) of the shot and the hit
        uint64_t want[4][4];
        memcpy(want, cm + b * 16, 64);
        if (shot) {
            const uint64_t *s = in + b * in_words + 8, *h = in + b * in_words + 12;
            const uint64_t pub[2][4] = {{s[0], s[1], 0, 0}, {h[0], h[1], 0, 0}};
            memcpy(want[2], pub, 64);
            if (!all_ones && !(s[2] | s[3] | h[2] | h[3])) bad = 1;   // (the case is meant to have bits above bit 127)
        }
        for (size_t r = 0; r < rows; r++) {
            uint64_t m[4];
            ref_to_mont(want[r], m);
            if (memcmp(canon + (b * rows + r) * 8, want[r], 32) != 0 || memcmp(mont + (b * rows + r) * 8, m, 32) != 0) bad = 1;
        }
    }
    free(cm), free(in), free(mont), free(canon);
    return bad;
}

// proof b: leaf combination b & 15, synthesis word (b >> 4) & 7, over 128 proofs
static int status_case(uint8_t flagged, uint32_t junk, size_t* lanes) {
    const size_t batch = 128, pitch = 128;
    uint8_t* leaf = (uint8_t*)malloc(4 * pitch);
    memset(leaf, 0, 4 * pitch);
    uint32_t *slot = (uint32_t*)malloc(2 * batch * 4), *syn = (uint32_t*)malloc(batch * 4);
    memset(slot, 0xa5, 2 * batch * 4);
    for (size_t b = 0; b < batch; b++) {
        for (int i = 0; i < 4; i++)
            if ((b >> i) & 1) leaf[(size_t)i * pitch + b] = flagged;
        syn[b] = (uint32_t)((b >> 4) & 7) | junk;
    }
    for (size_t b = 0; b < batch; b++) pd_status_lane(b, leaf, pitch, 2000u + (uint32_t)b, slot);
    for (size_t b = 0; b < batch; b++, ++*lanes) pg_status_lane(b, syn, slot);
    int bad = 0;
    for (size_t b = 0; b < batch; b++) {
        const uint32_t want = (uint32_t)(b & 15) | ((SYN_ST_EXCEPTIONAL * (uint32_t)((b >> 4) & 1)) << 4) |
                              ((SYN_ST_WINDOW_X0 * (uint32_t)((b >> 5) & 1)) << 4) | ((SYN_ST_MESSAGE * (uint32_t)((b >> 6) & 1)) << 4);
        if (want != (uint32_t)(b & 0x7f) || slot[2 * b] != want || slot[2 * b + 1] != 2000u + (uint32_t)b) bad = 1;
    }
    free(leaf), free(slot), free(syn);
    return bad;
}

int main() {
    int bad = 0, cases = 0;
    size_t lanes = 0;
    for (int shot = 0; shot < 2; shot++)
        for (size_t batch : {(size_t)1, (size_t)3, (size_t)70})
            for (int first : {0, 1, 2, 3})            // which coordinate the batch starts with: 0, 1, p - 1, seeded
                for (int ones = 0; ones < 2; ones++) {
                    const int rc = instances_case(shot != 0, batch, first, ones != 0, &lanes);
                    if (rc) printf("FAIL instances case %d (shot %d batch %zu first %d ones %d)\n", cases, shot, batch, first, ones);
                    bad |= rc;
                    cases++;
                }
    for (uint8_t f : {(uint8_t)1, (uint8_t)0x80, (uint8_t)0xff})
        for (uint32_t junk : {0u, 0xfffffff8u}) {
            const int rc = status_case(f, junk, &lanes);
            if (rc) printf("FAIL status case %d\n", cases);
            bad |= rc;
            cases++;
        }
    printf("%d cases, %zu lanes\n", cases, lanes);
    printf(bad ? "prove_game_scalars_check: FAILED\n" : "prove_game_scalars_check: ok\n");
    return bad ? 1 : 0;
}
