// The two lane bodies of the game-input prover (bzh_prove_shots_device / bzh_prove_boards_device), as host/device functions: what
// csrc/prove_game.hip's k_pg_instances and k_pg_status run is what tests/helpers/prove_game_scalars_check.hip runs on the host
// against the arithmetic of the host's synthesize_device (csrc/circuits.hip).
//   pg_instance_lane   the public inputs of proof b from what the synthesis left on the device: the commitment's canonical x || y
//                      (16 words, k_syn_ecc_tail) and, for Shot, the low 128 bits of the shot and hit input words
//                      (from_u128(lower_u128())).  Written twice: in Montgomery form into the [b][rows] instance buffer the
//                      commitments leaf reads (one instance column), and canonical into the call's read-back slot -- the rows
//                      bzh_synthesize_* hands to the host.
//   pg_status_lane     the synthesis status word of proof b (SYN_ST_*, three bits) shifted to bits 4 .. 6 and ORed into the status
//                      word of the slot pd_status_lane filled.  A lane owns its slot: a plain load and a plain store.
// The circuit kind is the launch's, the same for every lane; nothing depends on a lane's data.
#pragma once
#include "synthesize_device.hpp"

namespace bzh {

constexpr unsigned PG_SHOT_ROWS = 4, PG_BOARD_ROWS = 2;   // commitment x, y[, shot, hit]
constexpr unsigned PG_STATUS_SHIFT = 4;                   // above the four leaves' bits

// the canonical integer of four words as the element it is (no reduction: the value is below p)
BZH_HD SynFe pg_canonical(SynU256 v) {
    SynFe r;
    r.l[0] = (uint32_t)v.a, r.l[1] = (uint32_t)(v.a >> 32), r.l[2] = (uint32_t)v.b, r.l[3] = (uint32_t)(v.b >> 32);
    r.l[4] = (uint32_t)v.c, r.l[5] = (uint32_t)(v.c >> 32), r.l[6] = (uint32_t)v.d, r.l[7] = (uint32_t)(v.d >> 32);
    return r;
}
BZH_HD void pg_put_row(uint32_t* mont, uint32_t* canon, size_t row, const SynFe& c) {
    norm_store<SynP>(canon + row * 8, c);
    norm_store<SynP>(mont + row * 8, fe_to_mont(c));
}
// cm: batch x 16 words; in: batch x in_words packed input words (Shot: board, trapdoor, shot, hit, four words each), read for
// Shot only; mont, canon: batch x rows elements, rows = 4 (Shot) or 2 (Board)
BZH_HD void pg_instance_lane(size_t b, bool shot, const uint32_t* cm, const uint64_t* in, size_t in_words, uint32_t* mont, uint32_t* canon) {
    const size_t rows = shot ? PG_SHOT_ROWS : PG_BOARD_ROWS;
    pg_put_row(mont, canon, b * rows, norm_load<SynP>(cm + b * 16));
    pg_put_row(mont, canon, b * rows + 1, norm_load<SynP>(cm + b * 16 + 8));
    if (shot) {
        const uint64_t* w = in + b * in_words;
        pg_put_row(mont, canon, b * rows + 2, pg_canonical(syn_low(syn_load(w + 8), 128)));
        pg_put_row(mont, canon, b * rows + 3, pg_canonical(syn_low(syn_load(w + 12), 128)));
    }
}

// slot: two words per proof (status, proof length), as pd_status_lane wrote them
BZH_HD void pg_status_lane(size_t b, const uint32_t* syn_status, uint32_t* slot) {
    const uint32_t all = SYN_ST_EXCEPTIONAL | SYN_ST_WINDOW_X0 | SYN_ST_MESSAGE;
    slot[2 * b] = slot[2 * b] | ((syn_status[b] & all) << PG_STATUS_SHIFT);
}

}  // namespace bzh
