// The lane bodies of device witness synthesis (csrc/synthesize_device.hpp) run on the host, lane by lane in the kernels' order,
// against the Layouter path (bzh_synthesize_{shot,board}, host memory, Montgomery form): every word of the advice tensor, the
// instances and the status, for operands that steer the fixed-base multiplications and the complete additions.  The wave scan
// is stood in for by syn_scan_host.  Also syn_incomplete_exceptional on hand-made operands, which no scalar reaches through
// the entry points.  Stand-alone: built with csrc/circuits.hip and csrc/synthesize_device.hip, needs no device.
#include <cstdio>
#include <cstring>
#include <vector>

#include "ctx.hpp"
#include "synthesize_device.hpp"

using namespace bzh;

static int g_fail = 0;
#define CHECK(cond, ...)                  \
    do {                                  \
        if (!(cond)) {                    \
            printf("FAIL: " __VA_ARGS__); \
            printf("\n");                 \
            g_fail++;                     \
        }                                 \
    } while (0)

typedef std::vector<uint64_t> W;   // 4-limb words
static W word(uint64_t a, uint64_t b = 0, uint64_t c = 0, uint64_t d = 0) { return W{a, b, c, d}; }
static const uint64_t Q[4] = {0x8c46eb2100000001ull, 0x224698fc0994a8ddull, 0, 0x4000000000000000ull};   // Pallas scalar modulus

static std::vector<W> trapdoors() {
    std::vector<W> t;
    t.push_back(word(0));
    t.push_back(word(1));
    t.push_back(word(Q[0] - 1, Q[1], Q[2], Q[3]));                                    // q - 1
    t.push_back(word(~0ull, ~0ull, ~0ull, 0x3fffffffffffffffull));                    // 2^254 - 1
    t.push_back(word(0, 0, 0, 1ull << 60));                                           // 2^252
    W all7 = word(~0ull, ~0ull, ~0ull, 0x7fffffffffffffffull);                        // 85 windows of 7 = 2^255 - 1: not canonical
    t.push_back(all7);
    W alt(4, 0);                                                                      // windows 0 / 7 alternating, from window 1
    for (int w = 1; w < 85; w += 2)
        for (int b = 0; b < 3; b++) alt[(3 * w + b) / 64] |= 1ull << ((3 * w + b) % 64);
    t.push_back(alt);
    W alt0(4, 0);                                                                     // ... from window 0, top window 0
    for (int w = 0; w < 84; w += 2)
        for (int b = 0; b < 3; b++) alt0[(3 * w + b) / 64] |= 1ull << ((3 * w + b) % 64);
    t.push_back(alt0);
    t.push_back(word(0x5eed));
    t.push_back(word(Q[0], Q[1], Q[2], Q[3]));                                        // q: refused
    return t;
}

struct Twin {
    SynLayout L;
    std::vector<uint32_t> adv;
    uint32_t status = 0;
    uint32_t inst[16];
};
// one proof through the kernels' lane bodies
static void run_twin(Twin& t, const uint64_t* in) {
    const SynLayout* L = &t.L;
    t.adv.assign((size_t)L->num_advice * L->n * 8, 0);
    uint32_t* adv = t.adv.data();
    for (size_t row = 0; row < L->rows_used; row++) syn_cells_row(L, in, row, adv);
    uint32_t flags = 0;
    for (int base = 0; base < 2; base++) {
        SynAff m[SYN_NW], a[SYN_NW];
        SynXyzz s[SYN_NW];
        for (int w = 0; w < SYN_NW; w++) m[w] = syn_mulfixed_gather(L, synth_table_host(), in, base, w, adv, &flags);
        for (int w = 0; w < SYN_NW - 1; w++) s[w] = xyzz_from_affine(m[w]);
        syn_scan_host(s, SYN_NW - 1);
        for (int w = 0; w < SYN_NW - 1; w++) a[w] = syn_mulfixed_finish(L, base, w, s[w], adv);
        for (int w = 1; w < SYN_NW - 1; w++) flags |= syn_incomplete_exceptional(a[w - 1], m[w]);
    }
    t.status = flags | syn_ecc_tail(L, in, adv, t.inst);
}

static void compare(const char* what, int kind, unsigned k, const std::vector<W>& inputs /* per proof: the words in the entry point's order */,
                    size_t* lanes) {
    bzh_circuit* c = nullptr;
    CHECK(bzh_circuit_create(kind, k, 0, &c) == BZH_OK, "%s: circuit_create", what);
    if (!c) return;
    Twin t;
    CHECK(synth_layout(c, &t.L) == BZH_OK, "%s: layout", what);
    const size_t na = t.L.num_advice, n = t.L.n, ni = kind == BZH_CIRCUIT_SHOT ? 4 : 2;
    std::vector<uint64_t> want(na * n * 4), winst(ni * 4);
    for (size_t p = 0; p < inputs.size(); p++) {
        const uint64_t* in = inputs[p].data();
        int rc;
        if (kind == BZH_CIRCUIT_SHOT)
            rc = bzh_synthesize_shot(nullptr, c, 1, in, in + 4, in + 8, in + 12, want.data(), BZH_FORM_MONTGOMERY, BZH_MEM_HOST, winst.data(), 1);
        else
            rc = bzh_synthesize_board(nullptr, c, 1, in, in + 40, in + 44, want.data(), BZH_FORM_MONTGOMERY, BZH_MEM_HOST, winst.data(), 1);
        const uint64_t* trap = in + (kind == BZH_CIRCUIT_SHOT ? 4 : 44);
        const bool canonical = is_canonical(fe_from_u64<FqParams>(trap));
        if (!canonical) {   // refused before any lane runs, on either path
            CHECK(rc == BZH_E_RANGE, "%s #%zu: host takes a non-canonical trapdoor", what, p);
            continue;
        }
        run_twin(t, in);
        *lanes += t.L.rows_used + 2 * SYN_NW + 1;
        CHECK((rc != BZH_OK) == (t.status != 0), "%s #%zu: host status %d, lane status %u", what, p, rc, t.status);
        if (rc != BZH_OK || t.status) continue;
        size_t bad = 0;
        for (size_t i = 0; i < na * n * 4; i++) {
            const uint64_t got = (uint64_t)t.adv[2 * i] | ((uint64_t)t.adv[2 * i + 1] << 32);
            if (got != want[i] && bad++ < 5) printf("  %s #%zu: column %zu row %zu limb %zu differs\n", what, p, i / 4 / n, i / 4 % n, i % 4);
        }
        CHECK(bad == 0, "%s #%zu: %zu words differ", what, p, bad);
        uint64_t ginst[16] = {0};
        memcpy(ginst, t.inst, 64);
        if (kind == BZH_CIRCUIT_SHOT) ginst[8] = in[8], ginst[9] = in[9], ginst[12] = in[12], ginst[13] = in[13];
        CHECK(memcmp(ginst, winst.data(), ni * 32) == 0, "%s #%zu: instances differ", what, p);
    }
    bzh_circuit_free(c);
}

int main() {
    size_t lanes = 0;
    // a valid game: pattern #1 of the reference's tests
    const int8_t ships[15] = {3, 3, 1, 5, 4, 0, 0, 1, 0, 0, 5, 1, 6, 1, 0};
    uint64_t commits[40], state[4];
    if (bzh_board_witness(ships, nullptr, commits, state) != BZH_OK) return 2;
    const std::vector<W> traps = trapdoors();
    W bit_board = word(0), full_board = word(~0ull, (1ull << 36) - 1);
    int hit_bit = -1, miss_bit = -1;
    for (int i = 0; i < 100; i++) {
        const bool set = (state[i / 64] >> (i % 64)) & 1;
        if (set && hit_bit < 0) hit_bit = i;
        if (!set && miss_bit < 0) miss_bit = i;
    }
    bit_board[1] = 1ull << 35;   // bit 99
    auto shot_word = [](int i) {
        W s = word(0);
        s[i / 64] = 1ull << (i % 64);
        return s;
    };
    std::vector<W> boards = {W(state, state + 4), word(0), full_board, bit_board};
    // Shot
    {
        std::vector<W> in;
        auto push = [&](const W& board, const W& trap, const W& shot, uint64_t hit) {
            W v = board;
            v.insert(v.end(), trap.begin(), trap.end());
            v.insert(v.end(), shot.begin(), shot.end());
            const W h = word(hit);
            v.insert(v.end(), h.begin(), h.end());
            in.push_back(v);
        };
        for (const W& t : traps) push(boards[0], t, shot_word(hit_bit), 1);
        push(boards[0], traps[8], shot_word(miss_bit), 0);
        for (size_t b = 1; b < boards.size(); b++) {
            push(boards[b], traps[0], shot_word(99), b >= 2);
            push(boards[b], traps[2], shot_word(0), b == 2);
        }
        push(word(~0ull, ~0ull, ~0ull, ~0ull), traps[6], word(~0ull, ~0ull, 5, 0), 3);   // nothing assumes a well-formed game
        compare("shot k=11", BZH_CIRCUIT_SHOT, 11, in, &lanes);
    }
    // Board
    {
        std::vector<W> in;
        auto push = [&](const uint64_t* com, const W& board, const W& trap) {
            W v(com, com + 40);
            v.insert(v.end(), board.begin(), board.end());
            v.insert(v.end(), trap.begin(), trap.end());
            in.push_back(v);
        };
        const uint64_t zeros[40] = {0};
        for (const W& t : traps) push(commits, boards[0], t);
        for (size_t b = 1; b < boards.size(); b++) {
            push(zeros, boards[b], traps[0]);
            push(commits, boards[b], traps[3]);
        }
        uint64_t odd[40];   // full windows at every offset, ships that overlap nothing: H only
        memset(odd, 0, sizeof(odd));
        for (int i = 0; i < 5; i++) odd[8 * i] = ~0ull, odd[8 * i + 1] = (1ull << 36) - 1;
        push(odd, full_board, traps[6]);
        compare("board k=12", BZH_CIRCUIT_BOARD, 12, in, &lanes);
    }
    // add_incomplete_assign_region's refusal: equal x (P, P and P, -P) and an identity operand on either side
    {
        const uint32_t* e = synth_table_host();
        SynAff p, q, id;
        memcpy(p.x.l, e, 32), memcpy(p.y.l, e + 8, 32);
        memcpy(q.x.l, e + SYN_TBL_WORDS, 32), memcpy(q.y.l, e + SYN_TBL_WORDS + 8, 32);
        id.x = fe_zero<SynP>(), id.y = fe_zero<SynP>();
        SynAff np = p;
        np.y = fe_neg(p.y);
        CHECK(syn_incomplete_exceptional(p, q) == 0, "distinct points flagged");
        CHECK(syn_incomplete_exceptional(p, p) == SYN_ST_EXCEPTIONAL, "P, P not flagged");
        CHECK(syn_incomplete_exceptional(p, np) == SYN_ST_EXCEPTIONAL, "P, -P not flagged");
        CHECK(syn_incomplete_exceptional(id, q) == SYN_ST_EXCEPTIONAL && syn_incomplete_exceptional(p, id) == SYN_ST_EXCEPTIONAL, "identity operand not flagged");
        // and the complete addition's branches on the same operands, against the group law in XYZZ
        const SynAff ops[4] = {p, q, np, id};
        for (const SynAff& a : ops)
            for (const SynAff& b : ops) {
                const SynAdd r = syn_complete_add(a.x, a.y, b.x, b.y);
                const SynAff w = syn_xyzz_to_affine_ct(syn_xyzz_add(xyzz_from_affine(a), xyzz_from_affine(b)));
                CHECK(fe_eq(r.xr, w.x) && fe_eq(r.yr, w.y), "complete addition differs from the group law");
            }
    }
    printf("%zu lanes\n", lanes);
    if (g_fail) {
        printf("synth_device_check: %d failures\n", g_fail);
        return 1;
    }
    printf("synth_device_check: ok\n");
    return 0;
}
