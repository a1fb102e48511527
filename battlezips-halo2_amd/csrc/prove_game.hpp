// Part of the whole-proof translation unit (csrc/prove.hip): the GAME-INPUT PROVER (bzh_prove_shots_device,
// bzh_prove_boards_device) -- the reference's top-level operation, game inputs in and {commitment, proof} out
// (src/wasm/circuit_wasm.rs, benches/{shot,board}.rs), as one device-resident call.  It joins the two halves that exist:
// the device synthesis (csrc/synthesize_device.hip) and the device-resident batch prover (prove_device.hpp).  Between them the
// two-call path waits for the stream, reads the status words and the commitments back, rebuilds the instance rows on the host and
// uploads them again; here
//   the inputs are checked and packed on the host (synth_pack_inputs, csrc/circuits.hip), the call's only per-proof upload besides
//   the seeds: 128 bytes a Shot proof, 384 a Board proof;
//   prove_device_t allocates the advice tensor from the key's arena and has the synthesis kernels fill it (PdGame);
//   k_pg_instances (csrc/prove_game.hip) makes the instance rows on the device from the commitment k_syn_ecc_tail wrote;
//   k_pg_status folds the synthesis status word into bits 4 .. 6 of the per-proof status byte;
//   the canonical instances ride the one read-back of the proofs.
// What is refused before anything is launched is listed with the entry points in include/bzh2.h.
// Included inside namespace bzh { namespace { after prove_device.hpp.
#pragma once

// a .. d: the input arrays of bzh_synthesize_shot (boards, trapdoors, shots, hits) or bzh_synthesize_board (ship_commitments,
// boards, trapdoors, null)
static int prove_game_entry(const char* name, int kind, bzh_ctx* ctx, bzh_pk* pk, const bzh_circuit* c, size_t batch, const uint64_t* a,
                            const uint64_t* b, const uint64_t* c_in, const uint64_t* d, const uint8_t* seeds, uint64_t* instances, uint8_t* proofs,
                            size_t proof_stride, size_t* proof_lens, uint8_t* status) {
    // what reads neither the key nor the device
    if (!ctx || !pk || !c || !batch || batch > 65536 || !a || !b || !c_in || (kind == BZH_CIRCUIT_SHOT && !d) || !seeds || !proofs || !proof_lens)
        return BZH_E_ARG;
    SynShape shape;
    BZH_TRY(synth_shape(c, &shape));
    if (shape.kind != kind) return BZH_E_ARG;
    KeyRuntime::Call in_flight(pk->rt);   // until the proofs are in the caller's buffers
    // what reads the key.  The circuit must be the key's: the curve (the circuits are over Vesta's scalar field), n, the advice
    // columns, the one instance column and room for its rows
    if (pk->device != ctx->device) return BZH_E_ARG;
    if (pk->curve != BZH_CURVE_VESTA || pk->n != shape.n || (size_t)pk->na != shape.num_advice || (size_t)pk->ni != shape.num_instance ||
        pk->ni != 1 || shape.inst_rows > pk->usable)
        return BZH_E_ARG;
    if (batch > prove_device_max_batch(*pk)) return BZH_E_RANGE;
    if (!pk->q_ok || pk->en % 128) return BZH_E_RANGE;   // (bzh_prove_batch_device)
    if (proof_stride < prove_device_proof_bytes(*pk)) return BZH_E_RANGE;
    const PdPlan* plan = nullptr;
    BZH_TRY(prove_device_plan_of(pk, &plan));
    // step one of the synthesis: the refusals the host path makes on the inputs alone, with its texts
    SynLayout layout;
    std::vector<uint64_t> packed;
    std::string err;
    const int prc = synth_pack_inputs(c, batch, a, b, c_in, d, &layout, &packed, &err);
    if (prc) {
        if (prc == BZH_E_RANGE) {
            std::lock_guard<std::mutex> lk(ctx->mu);
            ctx->last_error = err;
        }
        return prc;
    }
    if ((size_t)layout.n != pk->n || (size_t)layout.num_advice != (size_t)pk->na) return BZH_E_ARG;   // (every write stays inside the tensor)
    const PdGame game{name, &layout, packed.data(), instances};
    std::lock_guard<std::mutex> lk(ctx->mu);
    BZH_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return with_pasta_curve(pk->curve, [&](auto cv) {
        return prove_device_t<decltype(cv)>(ctx, pk, batch, nullptr, BZH_FORM_MONTGOMERY, BZH_MEM_DEVICE, nullptr, shape.inst_rows, seeds, 0, *plan,
                                            proofs, proof_stride, proof_lens, status, &game);
    });
}
