/*
 * bzh2 -- MI355X (gfx950) prover-backend primitives for the BattleZips Halo2
 * circuits, flat C ABI.  This is the drop-in boundary: the entry points are
 * what an FFI shim inside `halo2_proofs` (the crate the reference calls into)
 * would bind for the create_proof hot path.  See INTEGRATION.md for the Rust
 * `extern "C"` block and the three call sites it replaces.
 *
 * The reference itself contains no prover arithmetic: its
 * hot path is the call
 *     create_proof(&params, &pk, &[circuit], &[&[&instances]], OsRng, &mut transcript)
 *   benches/shot.rs:68, benches/board.rs:61-68,
 *   src/circuits/shot.rs:921-928, src/circuits/board.rs:913-920,
 *   src/wasm/circuit_wasm.rs:66-73,151-158
 * which funnels into halo2_proofs 0.2.0 (Cargo.lock:382-385, un-vendored):
 *     arithmetic::best_multiexp(&[Scalar], &[Affine]) -> Curve      -> bzh_msm
 *     Params::{commit, commit_lagrange}                              -> bzh_bases_upload + bzh_msm
 *     arithmetic::best_fft(&mut [Scalar], omega, log_n)              -> bzh_ntt
 *     EvaluationDomain::{ifft, coeff_to_extended, extended_to_coeff} -> bzh_ntt (inverse / coset_shift)
 *
 * Data conventions
 *   field element : 4 x uint64 little-endian limbs (32 bytes).
 *                   form = BZH_FORM_MONTGOMERY  (x*2^256 mod p; pasta_curves' in-memory form,
 *                          so `&[Fp]` crosses the boundary without repacking) or
 *                   form = BZH_FORM_CANONICAL   (ff::PrimeField::to_repr, src/utils/binary.rs:36).
 *   affine point  : x || y (64 bytes, 8 limbs); (0,0) is the identity.
 *   Jacobian point: X || Y || Z (96 bytes, 12 limbs), x = X/Z^2, y = Y/Z^3, Z = 0 identity.
 *   mem           : BZH_MEM_HOST   - pointer is host memory, the call copies in/out and
 *                                    returns when the result is in the caller's buffer;
 *                   BZH_MEM_DEVICE - pointer is HBM on the ctx's device; the call only
 *                                    enqueues work on the ctx's stream (use bzh_ctx_sync).
 *
 * Ownership / errors / threading
 *   The caller owns every buffer; the library never keeps a host pointer past
 *   return.  Device tables are explicit handles (bzh_bases).  Every function
 *   returns 0 (BZH_OK) or a negative bzh_status and never throws or aborts
 *   across the boundary (halo2's callers `assert_eq!(coeffs.len(), bases.len())`
 *   and panic: a shim maps nonzero to panic!/Error::Synthesis).  One ctx = one
 *   device + one HIP stream; calls on one ctx are serialised by an internal
 *   mutex, several ctxs may be used from several threads.
 */
#ifndef BZH2_H
#define BZH2_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bzh_ctx bzh_ctx;
typedef struct bzh_bases bzh_bases;
typedef struct bzh_transcript bzh_transcript;

typedef enum {
    BZH_OK = 0,
    BZH_E_ARG = -1,    /* null pointer, bad enum, size mismatch               */
    BZH_E_OOM = -2,    /* hipMalloc / host allocation failed                  */
    BZH_E_HIP = -3,    /* a HIP runtime call failed (see bzh_last_error)      */
    BZH_E_RANGE = -4,  /* log_n beyond the field's 2-adicity, n too large ... */
    BZH_E_NOGPU = -5,  /* no usable gfx950 device                             */
    BZH_E_VERIFY = -6  /* bzh_ipa_verify: the proof does not verify           */
} bzh_status;

typedef enum { BZH_CURVE_VESTA = 0, BZH_CURVE_PALLAS = 1, BZH_CURVE_BN254 = 2 } bzh_curve;
typedef enum { BZH_FIELD_FP = 0, BZH_FIELD_FQ = 1, BZH_FIELD_BN254_FR = 2, BZH_FIELD_BN254_FQ = 3 } bzh_field;
typedef enum { BZH_FORM_CANONICAL = 0, BZH_FORM_MONTGOMERY = 1 } bzh_form;
typedef enum { BZH_MEM_HOST = 0, BZH_MEM_DEVICE = 1 } bzh_mem;

/* kernel classes timed by bzh_ctx_profile (indices into bzh_ctx_timings) */
typedef enum {
    BZH_T_MSM_DIGITS = 0,
    BZH_T_MSM_ACCUMULATE = 1,
    BZH_T_MSM_REDUCE = 2,
    BZH_T_MSM_FINALIZE = 3,
    BZH_T_NTT = 4,
    BZH_T_POLY = 5,
    BZH_T_QUOTIENT = 6, /* the quotient's gate evaluation over the extended coset (k_expr_vm2) */
    BZH_T_COUNT = 8
} bzh_timer;

/* ---- library / context -------------------------------------------------- */
const char* bzh_version(void);
const char* bzh_strerror(int status);
/* number of HIP devices visible (0 when there is no GPU); never fails */
int bzh_device_count(void);

/* One ctx = one device + one stream owned by the ctx. */
int bzh_ctx_create(int device, bzh_ctx** out);
/* Same, but work is enqueued on a caller-owned hipStream_t (e.g. the stream a
 * host framework already uses).  The stream must outlive the ctx. */
int bzh_ctx_create_on_stream(int device, void* hip_stream, bzh_ctx** out);
int bzh_ctx_destroy(bzh_ctx* ctx);
int bzh_ctx_sync(bzh_ctx* ctx);
/* text of the last HIP error seen on this ctx ("" if none) */
const char* bzh_last_error(const bzh_ctx* ctx);

/* Per-kernel-class timing with HIP events on the ctx's stream.  enable != 0
 * starts collecting (and clears the accumulators); bzh_ctx_timings syncs the
 * stream and returns, per class, accumulated milliseconds and launch counts
 * since enabling.  ms / launches must each hold BZH_T_COUNT entries.
 * A measurement aid, off by default: the event records are stream commands too -- one proof at a time they cost ~10 % of
 * its latency (10.4 -> 11.7 ms, BoardCircuit k = 14), 0.5 % of a batch's throughput.  Leave it off in production. */
int bzh_ctx_profile(bzh_ctx* ctx, int enable);
int bzh_ctx_timings(bzh_ctx* ctx, double* ms, uint64_t* launches);
/* Algorithmic bytes (MSM 32*B*N + 64*N per launch, NTT 64*N per transform) of the launches timed since
 * profiling was enabled, per kernel class (BZH_T_COUNT entries); divides by bzh_ctx_timings' ms for GB/s. */
int bzh_ctx_work(bzh_ctx* ctx, double* algorithmic_bytes);
/* bucket additions the MSM accumulation made since profiling was enabled (one per non-zero window digit: zero scalars and
 * zero digits of small scalars cost nothing) -- the work the integer multipliers actually did, for the ALU-side roofline */
int bzh_ctx_msm_additions(bzh_ctx* ctx, uint64_t* additions);

/* ---- commitment bases (Params.g / Params.g_lagrange of halo2's IPA params) -
 * Replaces the `bases: &[C]` argument of best_multiexp for tables that live
 * across many MSMs: n affine points are copied to HBM once (converted to
 * Montgomery form if needed) and referenced by handle afterwards. */
int bzh_bases_upload(bzh_ctx* ctx, int curve, const uint64_t* xy, size_t n, int form, int mem, bzh_bases** out);
/* Expand a table in place into the fixed-base window table  row w = 2^(c*w) * G_i  (w < ceil(256/c)),
 * c = window_bits or 0 for the library's choice.  Worth it for tables that serve many MSMs (the SRS:
 * every commitment of every proof uses Params.g or Params.g_lagrange): all windows of an MSM then
 * share one bucket set and the final doubling chain disappears.  Costs ceil(256/c) x the table's HBM
 * (k=14: 25 MB) and a one-time build; results are identical with or without it. */
int bzh_bases_precompute(bzh_ctx* ctx, bzh_bases* bases, int window_bits);
/* A synthetic table made on the device: bases[i] = [i + 1] G for i < n (SURVEY 8d's "cheap generator walk" for the 2^24-point
 * MSM microbench, BASELINE.json configs[4]: 1 GB of points that never cross PCIe).  g_xy: one affine point in `form` (host).
 * The CPU oracle's orc_point_walk makes the same set. */
int bzh_bases_walk(bzh_ctx* ctx, int curve, const uint64_t* g_xy, int form, size_t n, bzh_bases** out);
/* `count` points of a table from index `first`, affine canonical x || y into out_xy (host); a window table continues through
 * its rows (row w starts at w * n).  BZH_E_RANGE past the end. */
int bzh_bases_points(bzh_ctx* ctx, const bzh_bases* bases, size_t first, size_t count, uint64_t* out_xy);
int bzh_bases_free(bzh_ctx* ctx, bzh_bases* bases);
size_t bzh_bases_len(const bzh_bases* bases);

/* ---- multi-scalar multiplication  (halo2_proofs arithmetic::best_multiexp) -
 * out[b] = sum_{i<n} scalars[b*n + i] * bases[i]   for b < batch.
 * scalars: batch*n field elements of the curve's scalar field (`form`).
 * n may be smaller than the table (prefix is used, as Params::commit does for
 * short polynomials).  out: batch Jacobian points (12 limbs each) in `form`.
 * `mem` applies to both scalars and out. */
int bzh_msm(bzh_ctx* ctx, const bzh_bases* bases, const uint64_t* scalars, size_t n, size_t batch, int form, int mem,
            uint64_t* out_xyz);

/* ---- NTT  (halo2_proofs arithmetic::best_fft + EvaluationDomain) ----------
 * In place over `batch` contiguous vectors of 2^log_n elements; natural order
 * in and out.
 *   inverse == 0 : a_i <- sum_j a_j * omega^(ij); if coset_shift != NULL element j is
 *                  first multiplied by shift^j (coeff_to_extended's zeta powers).
 *   inverse != 0 : uses omega^-1, multiplies by n^-1 (EvaluationDomain::ifft); if
 *                  coset_shift != NULL result i is multiplied by shift^-i
 *                  (extended_to_coeff).
 * omega must be a primitive 2^log_n-th root of unity; omega and coset_shift are
 * host pointers to 4 limbs in `form`. */
int bzh_ntt(bzh_ctx* ctx, int field, uint64_t* data, unsigned log_n, size_t batch, const uint64_t* omega,
            const uint64_t* coset_shift, int inverse, int form, int mem);

/* EvaluationDomain::coeff_to_extended (halo2_proofs 0.2.0 poly/domain.rs, UPSTREAM; reached from create_proof at
 * benches/shot.rs:68): `batch` polynomials of 2^log_n coefficients at `coeffs` (contiguous) -> their evaluations over
 * the 2^log_ext-point coset shift*<omega_ext> at `out` (contiguous vectors of 2^log_ext).  Same result as zero-padding
 * each polynomial to 2^log_ext and calling bzh_ntt(..., coset_shift, inverse = 0), without the padded copy: the first
 * pass reads only the 2^log_n coefficients.  `coeffs` is not written; `out` must not overlap it. */
int bzh_coeff_to_extended(bzh_ctx* ctx, int field, const uint64_t* coeffs, unsigned log_n, uint64_t* out, unsigned log_ext,
                          size_t batch, const uint64_t* omega_ext, const uint64_t* coset_shift, int form, int mem);

/* ---- prover-stage vector primitives (N4, N5, N6) ------------
 * Field elements in `form`; `mem` applies to every pointer of the call.  With BZH_MEM_DEVICE the
 * read-only inputs must already be in Montgomery form (the library does not write to them).
 *
 * bzh_batch_invert     ff::BatchInvert: data[i] <- data[i]^-1, zeros stay zero (grand-product denominators)
 * bzh_prefix_product   in place, per vector of n: out[0] = 1, out[i] = prod_{j<i} in[j]
 *                      (the running products z(X) of permutation::Argument::commit / lookup commit_product)
 * bzh_eval_polynomial  arithmetic::eval_polynomial: out[b] = sum_i coeffs[b][i] * x_b^i;
 *                      nx = 1 (one point for every polynomial) or nx = batch
 * bzh_inner_product    arithmetic::compute_inner_product per vector pair
 * bzh_fold             IPA round fold: out[b][i] = in[b][i] + u_b * in[b][half + i], i < half; nu = 1 or batch
 * bzh_vec_mul          a[i] <- a[i] * b[i]
 */
/* canonical <-> Montgomery (x * 2^256 mod p) in place; device-resident pipelines keep Montgomery form throughout */
int bzh_field_convert(bzh_ctx* ctx, int field, uint64_t* data, size_t count, int to_montgomery, int mem);
/* ff::Field::random for `count` draws from a caller-supplied RNG byte stream (host pointer, 64 bytes per draw, the
 * 8 x next_u64 of pasta_curves): out[i] = bytes[64i .. 64i+64) as a 512-bit little-endian integer mod p.
 * The prover's random polynomials (vanishing argument, IPA s(X)) are n draws each; `mem` applies to out. */
int bzh_random_field(bzh_ctx* ctx, int field, const uint8_t* rng_bytes, size_t count, int form, int mem, uint64_t* out);
int bzh_batch_invert(bzh_ctx* ctx, int field, uint64_t* data, size_t count, int form, int mem);
/* ff::Field::sqrt for `count` elements in place, one lane each (csrc/sqrt_decompress.hip).  The root is the one pasta_curves
 * 0.4.1's `sqrt` returns: with p - 1 = 2^S T, g = gen^T and t in [0, 2^S) such that u^T g^t = 1, it is u^((T+1)/2) g^(t/2)
 * (the same formula with the generators 7 and 3 for the two BN254 fields).  status (may be NULL): 1 = a square (zero
 * included), 0 = not a square: that element is left as it was.  Returns BZH_OK when the call ran; with status == NULL,
 * BZH_E_RANGE if any element was not a square.  ctx == NULL with BZH_MEM_HOST runs on the host.  With BZH_MEM_DEVICE and a
 * status buffer the call only enqueues; otherwise it returns when the statuses are known.  Device buffers: 16-byte aligned. */
int bzh_batch_sqrt(bzh_ctx* ctx, int field, uint64_t* data, size_t count, int form, int mem, uint8_t* status);
int bzh_prefix_product(bzh_ctx* ctx, int field, uint64_t* data, size_t n, size_t batch, int form, int mem);
int bzh_eval_polynomial(bzh_ctx* ctx, int field, const uint64_t* coeffs, size_t n, size_t batch, const uint64_t* xs, size_t nx,
                        int form, int mem, uint64_t* out);
int bzh_inner_product(bzh_ctx* ctx, int field, const uint64_t* a, const uint64_t* b, size_t n, size_t batch, int form, int mem,
                      uint64_t* out);
int bzh_fold(bzh_ctx* ctx, int field, const uint64_t* in, size_t half, size_t batch, const uint64_t* u, size_t nu, int form,
             int mem, uint64_t* out);
int bzh_vec_mul(bzh_ctx* ctx, int field, uint64_t* a, const uint64_t* b, size_t count, int form, int mem);
/* arithmetic::kate_division (multiopen): out (n-1 coefficients) = quotient of the n-coefficient p(X) by (X - x);
 * the remainder p(x) is dropped.  x: 4 limbs in `form` (host). */
int bzh_kate_division(bzh_ctx* ctx, int field, const uint64_t* coeffs, size_t n, const uint64_t* x, int form, int mem,
                      uint64_t* out);
/* `batch` divisions in one pass: vector v = coeffs + v*n elements is divided by (X - xs[v]); out holds batch x (n-1). */
int bzh_kate_division_batch(bzh_ctx* ctx, int field, const uint64_t* coeffs, size_t n, size_t batch, const uint64_t* xs, int form,
                            int mem, uint64_t* out);
/* lookup::prover::permute_expression_pair (host: one sort per lookup argument): over the first usable_rows rows,
 * out_input = the input column sorted by canonical value; out_table holds the input value wherever a new run of
 * equal inputs starts and the table's unused values elsewhere (ascending, filled from the last repeated row
 * backwards, as upstream).  BZH_E_RANGE if an input value is missing from the table. */
int bzh_permute_expression_pair(int field, const uint64_t* input, const uint64_t* table, size_t usable_rows, int form,
                                uint64_t* out_input, uint64_t* out_table);
/* The same for `batch` pairs on the device (csrc/lookup_permute.hip): vector b of every array starts at element b * stride,
 * usable_rows <= stride.  Elements are read and written in `form` whichever `mem` is (Montgomery input is converted on the
 * device); rows usable_rows .. stride of every output vector are written as zero.  Pairs whose values are all below 2^16 (range
 * tables) are sorted by LDS histograms, any other pair by an LDS tile sort and co-rank merge passes; the choice is made on the
 * device, per pair.  status (host, `batch` words, may be NULL): 0, or BZH_E_RANGE for a pair with an input value missing from
 * its table -- the call then returns BZH_E_RANGE and the other pairs' outputs are still correct.  BZH_E_ARG: NULL ctx,
 * usable_rows > stride, usable_rows = 0.  Returns when status is known (and, for BZH_MEM_HOST, the outputs are in place). */
int bzh_permute_expression_pair_batch(bzh_ctx* ctx, int field, const uint64_t* input, const uint64_t* table, size_t stride,
                                      size_t usable_rows, size_t batch, int form, int mem, uint64_t* out_input, uint64_t* out_table,
                                      int32_t* status);

/* ---- Fiat-Shamir transcript (host; halo2_proofs transcript::{Blake2bWrite, Challenge255}) --
 * What every create_proof caller builds first (benches/shot.rs:66-67, src/circuits/board.rs:911-912:
 * `Blake2bWrite::<_, vesta::Affine, Challenge255<_>>::init(vec![])`).  Blake2b-512, personal
 * "Halo2-Transcript"; points and scalars are passed in canonical form (8 / 4 limbs).
 *   common_*  absorb only;  write_*  absorb and append to the proof bytes (compressed point / repr);
 *   squeeze_challenge  absorbs 0x00 and returns the digest reduced as a 512-bit LE integer mod the
 *   challenge field (4 canonical limbs);  proof  borrows the bytes written so far (finalize()). */
typedef struct bzh_transcript bzh_transcript;
int bzh_transcript_new(int challenge_field, bzh_transcript** out);
int bzh_transcript_free(bzh_transcript* t);
int bzh_transcript_common_point(bzh_transcript* t, const uint64_t* xy_canonical);
int bzh_transcript_common_scalar(bzh_transcript* t, const uint64_t* s_canonical);
int bzh_transcript_write_point(bzh_transcript* t, int curve, const uint64_t* xy_canonical);
int bzh_transcript_write_scalar(bzh_transcript* t, const uint64_t* s_canonical);
int bzh_transcript_squeeze_challenge(bzh_transcript* t, uint64_t* out_canonical);
int bzh_transcript_proof(const bzh_transcript* t, const uint8_t** data, size_t* len);

/* ---- gate-expression evaluation over the extended coset (row a13: poly::Evaluator + vanishing::construct) --
 * A straight-line program evaluated at every row r < 2^log_size:
 *   operand kinds  BZH_EXPR_SLOT (idx = slot), BZH_EXPR_COLUMN (idx = column, rot = row offset, wraps mod size),
 *                  BZH_EXPR_CONST (idx = constant);
 *   ops            ADD, SUB, MUL (a, b);  NEG, COPY (a);  dst = slot < BZH_EXPR_MAX_SLOTS.
 * out[r] = slot `result_slot` after the last op.  columns: host array of ncols pointers (each 2^log_size
 * elements, `mem` says where they live); consts: nconsts elements (host).  A rotation by t rows of the
 * 2^k-row circuit is rot = t * 2^(log_size - k) on the extended domain. */
enum { BZH_EXPR_ADD = 0, BZH_EXPR_SUB = 1, BZH_EXPR_MUL = 2, BZH_EXPR_NEG = 3, BZH_EXPR_COPY = 4 };
enum { BZH_EXPR_SLOT = 0, BZH_EXPR_COLUMN = 1, BZH_EXPR_CONST = 2 };
enum { BZH_EXPR_MAX_SLOTS = 24 };
typedef struct {
    uint8_t op, dst, a_kind, b_kind;
    int32_t a_idx, b_idx, a_rot, b_rot;
} bzh_expr_op;
int bzh_expr_eval(bzh_ctx* ctx, int field, const bzh_expr_op* prog, size_t nops, const uint64_t* const* columns, size_t ncols,
                  const uint64_t* consts, size_t nconsts, unsigned log_size, int result_slot, int form, int mem, uint64_t* out);

/* The same program over `batch` vectors (independent proofs) in one launch: vector v reads column c at
 * columns[c] + v * column_strides[c] elements (0, or column_strides == NULL: the column is shared, e.g. fixed /
 * permutation columns of the proving key) and its constants at consts + v * const_stride elements (0: shared;
 * otherwise >= nconsts, e.g. per-proof challenges); out holds batch x 2^log_size results. */
int bzh_expr_eval_batch(bzh_ctx* ctx, int field, const bzh_expr_op* prog, size_t nops, const uint64_t* const* columns,
                        const size_t* column_strides, size_t ncols, const uint64_t* consts, size_t nconsts, size_t const_stride,
                        unsigned log_size, int result_slot, size_t batch, int form, int mem, uint64_t* out);

/* One VM v2 program -- the quotient interpreter of bzh_prove_batch, run without a proving key -- over `batch` vectors: out holds
 * batch x 2^log_size values of register r0 after the last instruction.  ops: nops 16-byte instruction words as
 * bzh_quotient_program_for_circuit hands them out (layout there; the instruction set: csrc/vm2_isa.hpp); operand kinds are
 * BZH_EXPR_COLUMN, BZH_EXPR_CONST and 3 = slot of the slot file (nlds slots, kept in LDS).  columns, column_strides, consts,
 * const_stride, form and mem as for bzh_expr_eval_batch.  The registers start at zero; the slot file is NOT cleared, a program
 * reads only slots it has stored to.  The program is checked before anything is launched.  BZH_E_ARG, out untouched: an
 * instruction word the interpreter has no case for (form SS at register 3, form LL with RSUB, form UN with operation 3, a code
 * above 63); an operand that is read and is not a column, a constant or a slot; a column index not below ncols, a constant
 * index not below nconsts, a slot index (a STORE's target included) not below nlds; 2^log_size not a multiple of 128; batch 0 or
 * above 65535; a field other than the two Pasta fields.  BZH_E_RANGE: more slots than 64 KB of LDS hold at 64 rows (nlds > 32). */
int bzh_vm2_eval(bzh_ctx* ctx, int field, const void* ops, size_t nops, const uint64_t* const* columns, const size_t* column_strides,
                 size_t ncols, const uint64_t* consts, size_t nconsts, size_t const_stride, unsigned log_size, size_t batch, int nlds,
                 int form, int mem, uint64_t* out);

/* The same program evaluated COSET BY COSET, as the prover's BZH_WORKSPACE_COSETWISE does it, without a proving key.  The 8 n
 * rows of a vector (n = 2^log_n) are eight cosets of n rows: row R = 8 r + j is row r of coset j.  One launch per coset; a leaf
 * of column c at rotation rot reads index ((R + rot) & (8 n - 1)) >> shift, shift 0 for a column with column_extended[c] != 0 (8 n
 * elements per vector, laid out as for bzh_vm2_eval) and 3 for an n-sized one, which is given as EIGHT blocks, one per coset:
 * coset j's values of vector v start at columns[c] + j * block + v * column_strides[c] elements, block = batch * column_strides[c],
 * or n for a shared column (stride 0); block j holds the column's rows j, j + 8, j + 16, ...  out: batch x 8 n values, equal word
 * for word to bzh_vm2_eval's over the same data.  BZH_E_ARG, out untouched: whatever bzh_vm2_eval refuses (the multiple of 128
 * excepted: a last workgroup may be partial); a column leaf that is read with a rotation that is not a multiple of 8 (it would
 * leave the coset); out_size != 8 * 2^log_n; log_n above 27; a stride below the column's rows; `out`, `consts` or a column
 * pointer that is not aligned to 8 bytes (BZH_MEM_HOST) or to 32 bytes (BZH_MEM_DEVICE). */
int bzh_vm2_eval_cosets(bzh_ctx* ctx, int field, const void* ops, size_t nops, const uint64_t* const* columns, const size_t* column_strides,
                        const uint8_t* column_extended, size_t ncols, const uint64_t* consts, size_t nconsts, size_t const_stride,
                        unsigned log_n, size_t out_size, size_t batch, int nlds, int form, int mem, uint64_t* out);

/* ---- inner-product-argument opening (halo2_proofs poly::commitment::{create_proof, verify_proof}) --
 * Step 9 of plonk::create_proof and the heart of verify_proof (benches/board.rs:80-86).
 * `bases` must hold n + 2 points: the n = 2^k SRS generators followed by U and W (Params.u, Params.w);
 * a window table (bzh_bases_precompute) is recommended: every round is two MSMs against it.
 * bzh_ipa_open   writes S, (L_j, R_j) for j < k, then the scalars c and f to the transcript, exactly
 *                the upstream message order.  poly: n coefficients (`form`, `mem`); blind, x3: 4 canonical
 *                limbs (host); rng: 64 bytes of RNG output per drawn scalar in upstream's draw order
 *                (n for s(X), 1 for its blind, 2 per round) = 64 * (n + 1 + 2k) bytes; out_v = p(x3).
 * bzh_ipa_verify checks  sum_j (u_j^-1 L_j + u_j R_j) + P - [v]G_0 + [xi]S == [c]G'_0 + [c b_0 z]U + [f]W
 *                against a transcript in the same state the prover's was before bzh_ipa_open;
 *                g0_u_w: G_0, U, W as 3 canonical affine points.  Returns BZH_OK or BZH_E_VERIFY. */
int bzh_ipa_open(bzh_ctx* ctx, const bzh_bases* bases, const uint64_t* poly, int form, int mem, const uint64_t* blind,
                 const uint64_t* x3, const uint8_t* rng, size_t rng_len, bzh_transcript* transcript, uint64_t* out_v);
/* `batch` independent openings against the same bases, advanced in lockstep (every round is one MSM launch of
 * 2*batch vectors and one host round trip): polys = batch x n coefficients, blinds / x3s / out_v = batch x 4 limbs,
 * proof b draws from rng + b*rng_stride and writes to transcripts[b].  bzh_ipa_open is the batch = 1 case. */
int bzh_ipa_open_batch(bzh_ctx* ctx, const bzh_bases* bases, const uint64_t* polys, int form, int mem, size_t batch,
                       const uint64_t* blinds, const uint64_t* x3s, const uint8_t* rng, size_t rng_stride,
                       bzh_transcript* const* transcripts, uint64_t* out_v);
/* bzh_ipa_open_batch against a device-resident bzh_transcript_batch, which is declared below (csrc/ipa.hip, csrc/ipa_scalars.hpp): the
 * same openings, proof for proof and byte for byte -- S, (L_j, R_j) for j < k, then c and f go into transcript b of `transcripts`,
 * out_v[b] = p_b(x3_b); the message order, the draw order of rng, the generator collapse and BZH_IPA_COLLAPSE / BZH_IPA_TAIL_C
 * are those of bzh_ipa_open_batch -- with the rounds on the device: every point is normalised and absorbed from HBM, every
 * challenge squeezed into HBM, and a lane per proof inverts u_j and folds f.  `transcripts` belongs to this ctx, its curve is the
 * curve of `bases` and its batch is `batch`.  `mem` applies to every data pointer of the call: with BZH_MEM_DEVICE polys, blinds,
 * x3s, rng, out_v (16-byte aligned) and status are device pointers -- blinds, x3s and out_v batch x 4 limbs in `form`, the 64-byte
 * draws of proof b at rng + b * rng_stride -- and the call only enqueues: x3, itself a squeezed challenge, never leaves HBM.  With
 * BZH_MEM_HOST the operands are staged up once at the start and out_v / status read back once at the end.
 * status (may be NULL): one byte per proof, 0, or nonzero if a round challenge of that proof was zero and so has no inverse
 * (bzh_ipa_open_batch returns BZH_E_ARG there; without a read-back there is nothing to return it from).  Identity or invalid
 * points are reported by bzh_transcript_batch_status as ever.
 * Between its first launch and its last the call copies no point, scalar or challenge to the host, does no host field or curve
 * arithmetic and adds no stream synchronisation of its own; what bzh_msm itself waits for, and a workspace (the ctx's, or the
 * batch's normalisation scratch) that grows on first use, stay as they are.
 * BZH_E_ARG, the batch left as it was: a NULL ctx, bases, transcripts or data pointer; a host-resident batch; a batch of another
 * ctx, curve or size; n not a power of two; batch == 0 or > 65535; unknown form or mem; a misaligned device pointer; rng_stride
 * < 64 * (n + 1 + 2k).  BZH_E_RANGE, nothing absorbed: proof_cap cannot take 32 * (1 + 2k) + 64 more bytes. */
struct bzh_transcript_batch;
int bzh_ipa_open_batch_device(bzh_ctx* ctx, const bzh_bases* bases, const uint64_t* polys, int form, int mem, size_t batch,
                              const uint64_t* blinds, const uint64_t* x3s, const uint8_t* rng, size_t rng_stride,
                              struct bzh_transcript_batch* transcripts, uint64_t* out_v, uint8_t* status);
/* poly::multiopen::prover::create_proof against a device-resident bzh_transcript_batch -- csrc/multiopen.hip,
 * csrc/multiopen_scalars.hpp: every opening of a proof folded into one polynomial and one point, and that one opened by
 * bzh_ipa_open_batch_device's rounds -- the multiopen() phase of bzh_prove_batch as a leaf, with its challenges in HBM.
 *
 * bzh_multiopen_plan is upstream's construct_intermediate_sets, pure host code (no ctx, no device).  A query says "open
 * polynomial `poly` at point number `point`".  Polynomials are taken in first-seen order, a repeated (poly, point) pair counts
 * once, a polynomial's set is the set of its point numbers, and sets are numbered in the order their first polynomial appears.
 * Grouping is by point NUMBER, not by value: the caller gives equal values one number (two numbers with one value in the same
 * set are the coincident points of status bit 0 below).  set_of_poly[p]: the set of polynomial p, 0xffffffff if never queried;
 * group_order: the queried polynomials set by set, first-seen order inside a set (0xffffffff from their count on); set_sizes[s]:
 * points of set s; set_points: row s (BZH_MULTIOPEN_MAX_POINTS entries) holds the point numbers of set s in ascending order,
 * padded with 0xffffffff -- the order inside a set does not reach the proof bytes.  set_sizes and set_points have room for npolys
 * sets.  BZH_E_ARG: a NULL pointer, a poly or point number out of range, nqueries == 0, a set of more than
 * BZH_MULTIOPEN_MAX_POINTS points.
 *
 * bzh_multiopen_batch_device: n = 2^k coefficients per polynomial; `bases` is the SRS as the IPA entry points take it
 * (g || u || w, n + 2 points); polynomial ids below npolys_own are proof b's own (polys[b][id], blinds[b][id]), the rest are
 * shared by every proof (shared[id - npolys_own], shared_blinds[..]; both may be NULL only if npolys_shared == 0); points[b][j]
 * is point number j of proof b.  `form` and `mem` apply to every data pointer except `queries` (host), as in
 * bzh_ipa_open_batch_device: with BZH_MEM_DEVICE they are 16-byte-aligned device pointers (status: any alignment) and the call
 * only enqueues; with BZH_MEM_HOST everything is staged up once at the start and status read back once at the end.
 * Messages, per proof, in upstream's order: squeeze x1, x2; q_s = Horner in x1 over the polynomials of set s in group order
 * (q_blind_s likewise over their blinds); r_s = the interpolant through (point, q_s(point)) over the set's points;
 * f_s = (q_s - r_s) / prod (X - point), zero-padded to n; f = Horner in x2 over f_0, ..; WRITE the commitment of f under f_blind;
 * squeeze x3; WRITE q_s(x3) for every s; squeeze x4; p = Horner in x4 over (f, q_0, ..), p_blind likewise; then the opening
 * of p at x3: S, (L_j, R_j) for j < k, c, f as bzh_ipa_open_batch_device writes them.
 * rng: the 64-byte draws of proof b at rng + b * rng_stride; the first is f_blind, the opening takes the n + 1 + 2k after it,
 * so rng_stride >= 64 * (n + 2 + 2k).  The proof grows by 32 + 32 * nsets + 32 * (1 + 2k) + 64 bytes.
 * status (may be NULL), one byte per proof: bit 0 -- two points of one set coincide in that proof (an interpolation denominator
 * is zero; its inverse is taken as 0 and the proof's bytes mean nothing); bit 1 -- what bzh_ipa_open_batch_device reports, a
 * zero round challenge.  A flagged proof disturbs no other proof, and the call returns BZH_OK.
 * Between its first launch and its last the call copies no point, scalar or challenge to the host, does no host field or curve
 * arithmetic and adds no stream synchronisation of its own; what bzh_msm itself waits for, and a workspace (the ctx's, or the
 * batch's normalisation scratch) that grows on first use, stay as they are.  Its scratch -- q, the division's two buffers and
 * the f_s at nsets x batch x n elements each, f and p -- is the ctx's staging workspace.
 * BZH_E_ARG, the batch left as it was: a NULL ctx, bases, transcripts or required data pointer; a host-resident batch; a batch
 * of another ctx, curve or size; batch == 0 or > 65535; unknown form or mem; a misaligned device pointer; rng_stride too small;
 * bases that do not hold exactly n + 2 points (n + 2 larger than the table included); a set of n or more points; no own
 * polynomial; anything bzh_multiopen_plan refuses.  BZH_E_RANGE, nothing absorbed: proof_cap
 * cannot take the bytes above.  Every check that needs no device comes before the first use of ctx. */
typedef struct {
    uint32_t poly;
    uint32_t point;
} bzh_open_query;
#define BZH_MULTIOPEN_MAX_POINTS 8
int bzh_multiopen_plan(const bzh_open_query* queries, size_t nqueries, size_t npolys, size_t npoints, uint32_t* set_of_poly,
                       uint32_t* group_order, uint32_t* set_sizes, uint32_t* set_points, size_t* nsets);
int bzh_multiopen_batch_device(bzh_ctx* ctx, const bzh_bases* bases, size_t batch, unsigned k, const uint64_t* polys, size_t npolys_own,
                               const uint64_t* shared, size_t npolys_shared, const uint64_t* blinds, const uint64_t* shared_blinds,
                               const uint64_t* points, size_t npoints, const bzh_open_query* queries, size_t nqueries, int form, int mem,
                               const uint8_t* rng, size_t rng_stride, struct bzh_transcript_batch* transcripts, uint8_t* status);
/* The evaluation phase of plonk::create_proof against a device-resident bzh_transcript_batch -- csrc/evaluations.hip,
 * csrc/evaluations_scalars.hpp: the step between the quotient commitments and the multiopen argument, the evaluations() and
 * h_poly() phases of bzh_prove_batch as a leaf, with x in HBM.  Its out_points is the `points` operand of
 * bzh_multiopen_batch_device, and its out_h / out_h_blind one more own polynomial and blind of that call, so the arguments after
 * the quotient commitments (evaluations, multiopen, opening) run back to back on a device batch.
 *
 * bzh_evaluations_plan is pure host code (no ctx, no device).  A query says "write `poly` at x * omega^rotation"; any int32
 * rotation is taken.  rotations / *nrotations: the distinct rotations in first-seen order (room for nqueries); point_of_query[q]:
 * the index of query q's rotation in `rotations`; poly_order: the queried polynomials in first-seen order, 0xffffffff from their
 * count on, and rot_count[p]: the distinct rotations of polynomial p, 0 if it is never queried (room for npolys each).
 * BZH_E_ARG, nothing written: a NULL pointer, a poly id out of range, nqueries == 0, a polynomial at more than
 * BZH_EVAL_MAX_ROTATIONS distinct rotations.
 *
 * bzh_evaluations_batch_device: the field is the scalar field of the batch's curve, n = 2^k coefficients per polynomial, omega
 * the 2^k-th root bzh_field_omega returns (a negative rotation uses its inverse).  Polynomial ids below npolys_own are proof b's
 * own (polys[b][id]), the rest are shared by every proof (shared[id - npolys_own]; may be NULL only if npolys_shared == 0).  Piece
 * i of proof b lies at h_pieces + (b * h_stride + i * n) elements -- a prover's batch x extended-size quotient buffer goes in as it
 * is -- and h_blinds[b][i] is its blind.  `form` and `mem` apply to every data pointer except `queries` (host), as in the two calls
 * above: with BZH_MEM_DEVICE they are 16-byte-aligned device pointers and the call only enqueues; with BZH_MEM_HOST the operands
 * are staged up once at the start and the outputs read back once at the end.
 * Messages, per proof, in upstream's order: squeeze x; for each query in the order given WRITE poly(x * omega^rotation) -- a
 * repeated query is evaluated and written again.  The proof grows by 32 * nqueries bytes.
 * Outputs, in `form`: out_points[b][j] = x_b * omega^rotations[j], j as bzh_evaluations_plan numbers the rotations;
 * out_evals[b][q] (may be NULL); with npieces > 0, out_h[b] = sum_i x_b^(n i) * piece_i (n coefficients) and out_h_blind[b] the
 * same sum over h_blinds -- h_pieces, h_blinds, out_h and out_h_blind are required iff npieces > 0.  The transcripts and the
 * outputs are the only things written.
 * Between its first launch and its last the call copies no scalar or challenge to the host, does no host field arithmetic on
 * anything that depends on x and adds no stream synchronisation of its own; omega^rotation, which depends on (field, k,
 * rotation) alone, is computed on the host and uploaded before the first launch.  A polynomial is read once per proof however
 * many rotations it is queried at (twice above 5), in place: there is no gathered copy, and the scratch -- x, x^n, the values
 * per (proof, query) and the small tables, in the ctx's staging workspace -- holds no buffer of n elements per query.
 * BZH_E_ARG, the batch left as it was and nothing written: a NULL ctx, transcripts or required data pointer; a host-resident
 * batch; a batch of another ctx or size; batch == 0 or > 65535; k larger than the field's two-adicity; nqueries == 0; no own
 * polynomial; h_stride < npieces * n; unknown form or mem; a misaligned device pointer; anything bzh_evaluations_plan refuses.
 * BZH_E_RANGE, nothing absorbed and x not squeezed: proof_cap cannot take 32 * nqueries more bytes.  Every check that needs no
 * device comes before the first use of ctx. */
typedef struct {
    uint32_t poly;
    int32_t rotation;
} bzh_eval_query;
#define BZH_EVAL_MAX_ROTATIONS 8
int bzh_evaluations_plan(const bzh_eval_query* queries, size_t nqueries, size_t npolys, int32_t* rotations, size_t* nrotations,
                         uint32_t* point_of_query, uint32_t* poly_order, uint32_t* rot_count);
int bzh_evaluations_batch_device(bzh_ctx* ctx, size_t batch, unsigned k, const uint64_t* polys, size_t npolys_own, const uint64_t* shared,
                                 size_t npolys_shared, const bzh_eval_query* queries, size_t nqueries, const uint64_t* h_pieces,
                                 size_t npieces, size_t h_stride, const uint64_t* h_blinds, int form, int mem,
                                 struct bzh_transcript_batch* transcripts, uint64_t* out_points, uint64_t* out_evals, uint64_t* out_h,
                                 uint64_t* out_h_blind);
/* The vanishing argument of plonk::create_proof against a device-resident bzh_transcript_batch -- csrc/vanishing_device.hpp,
 * csrc/vanishing.hip, csrc/vanishing_scalars.hpp: the step between the grand products and the evaluations, the vanishing() phase
 * of bzh_prove_batch as a leaf, with theta, beta, gamma and y in HBM.  Its out_h goes into bzh_evaluations_batch_device as
 * h_pieces with h_stride = the extended size, its out_h_blinds as h_blinds and its out_random as one more own polynomial, so the
 * arguments from the random polynomial's commitment on (vanishing, evaluations, multiopen, opening) run back to back on a device
 * batch.  Its speed has not been measured.
 *
 * bzh_vanishing_plan is pure host code (no ctx, no device), like bzh_quotient_program_for_circuit.  shape8: n, the extended size
 * en, num_advice, num_instance, nz (permutation sets + lookups), the number of lookups, npieces, and the draws per proof
 * (n + 1 + npieces).  consts / *nconsts: one bzh_vanishing_const per entry of the circuit's VM v2 constant table, in the table's
 * order (consts_cap counts entries).  A literal (challenge -1) carries its value; a symbol means value * challenge^exponent in
 * Montgomery form: theta, beta, gamma, y are (0 .. 3, 1, one), y^m is (3, m, one) with m <= 64, and beta * delta^j -- the
 * permutation argument's column j -- is (1, 1, delta^j); delta^j depends on the key alone and is computed here.  BZH_E_RANGE if
 * the circuit does not fit VM v2.  BZH_E_ARG, nothing written: a NULL pointer, a blob that does not parse, consts_cap below the
 * number of constants.
 *
 * bzh_vanishing_batch_device takes its operands in the prover's own layouts, n = 2^k coefficients each: advice_polys[b][i][n],
 * instance_polys[b][i][n], lookup_polys[b][l][2][n] (the permuted input, then the permuted table) and z_polys[b][nz][n] (the
 * permutation sets' grand products, then the lookups'); an operand whose count is 0 may be NULL.  theta, beta, gamma: one element
 * per proof each, as bzh_transcript_batch_squeeze writes them.  `form` and `mem` apply to every data pointer, as in the three
 * calls above: with BZH_MEM_DEVICE they are 16-byte-aligned device pointers (`status` any alignment) and the call only enqueues;
 * with BZH_MEM_HOST the operands are staged up once at the start and the outputs read back once at the end.  rng: proof b's
 * 64-byte draws at rng + b * rng_stride, in upstream's order -- the n coefficients of the random polynomial, its blind, the
 * npieces piece blinds --, so rng_stride >= 64 * (n + 1 + npieces).
 * Messages, per proof, in upstream's order: WRITE the commitment of the random polynomial; squeeze y; WRITE the commitment of each
 * piece h[i * n .. (i + 1) * n), i < npieces, under its blind.  The proof grows by 32 * (1 + npieces) bytes; x is not squeezed.
 * Outputs, in `form`: out_random[b][n] and out_random_blind[b]; out_h[b][en], the quotient's coefficients, all en of them;
 * out_h_blinds[b][npieces]; status (may be NULL), one byte per proof: bit 0 is set when a coefficient at or above npieces * n is
 * non-zero -- the witness does not satisfy the circuit.  Such a proof still gets its messages, built from the low coefficients,
 * disturbs no other proof, and the call returns BZH_OK; the bit is also ORed into the batch's sticky status byte.  A circuit
 * whose pieces fill the extended domain (npieces * n == en: degree 3, 5, 9 ..) has no such coefficient and never sets the bit.
 * The quotient runs in the flavour the key has selected (bzh_pk_quotient_select), with the launches of bzh_prove_batch, from a
 * constant table that one launch builds on the device out of the challenges; the plan's descriptors are uploaded before the
 * first launch.  Between its first launch and its last the call copies nothing that depends on a challenge to the host, does no
 * host field or curve arithmetic on such a value and adds no stream synchronisation of its own.  The scratch -- the extended
 * cosets of every column, the commitments' scalar rows -- is the key's workspace for this ctx, as in bzh_prove_batch, and the
 * call counts as running on the key like every other call on it (bzh_pk_free).  A BZH_MEM_DEVICE call returns with its work
 * queued on that workspace.  The workspace grows during a key's first call of a shape on a ctx and is merged into one block at
 * the start of the next call on that key and ctx, which therefore waits once for the stream, before its own first launch; the
 * calls after it wait for nothing.
 * BZH_E_ARG, the batch left as it was and nothing written: a NULL ctx, pk, transcripts, rng, challenge, output or required
 * operand pointer; a host-resident batch; a batch of another ctx, curve or size; a key on another device than ctx; batch == 0
 * or > 65535, or batch * npieces > 65535 (the piece commitments of a batch are one launch with one row of its grid per
 * commitment: at most 8191 proofs for Shot and Board, whose npieces is 8); unknown form or mem; a misaligned device pointer; rng_stride too small.  BZH_E_RANGE, nothing absorbed: proof_cap
 * cannot take 32 * (1 + npieces) more bytes; the key's circuit does not fit VM v2 or its extended size is no multiple of 128
 * (the VM v1 fold is not offered here).  Every check that reads neither the key nor the device comes first, then those that read
 * the key; all of them come before the first use of ctx. */
typedef struct {
    int32_t challenge; /* -1 literal, 0 theta, 1 beta, 2 gamma, 3 y */
    uint32_t exponent;
    uint32_t value[8]; /* Montgomery */
} bzh_vanishing_const;
int bzh_vanishing_plan(int curve, const uint8_t* circuit, size_t circuit_len, uint32_t shape8[8], bzh_vanishing_const* consts,
                       size_t consts_cap, size_t* nconsts);
struct bzh_pk; /* (a proving key: the next section) */
int bzh_vanishing_batch_device(bzh_ctx* ctx, struct bzh_pk* pk, size_t batch, const uint64_t* advice_polys, const uint64_t* instance_polys,
                               const uint64_t* lookup_polys, const uint64_t* z_polys, const uint64_t* theta, const uint64_t* beta,
                               const uint64_t* gamma, int form, int mem, const uint8_t* rng, size_t rng_stride,
                               struct bzh_transcript_batch* transcripts, uint64_t* out_random, uint64_t* out_random_blind,
                               uint64_t* out_h, uint64_t* out_h_blinds, uint8_t* status);
/* The permutation and lookup grand products of plonk::create_proof against a device-resident bzh_transcript_batch --
 * csrc/products_device.hpp, csrc/products.hip, csrc/products_scalars.hpp: the step between the squeeze of beta and gamma and the
 * vanishing argument, the grand_products() phase of bzh_prove_batch as a leaf, with beta and gamma in HBM.  Its out_z_polys is
 * the z_polys operand of bzh_vanishing_batch_device and its out_z_blinds goes into the multiopen's blind table, so the arguments
 * from the grand products on (grand products, vanishing, evaluations, multiopen, opening) run back to back on a device batch.
 *
 * bzh_grand_products_plan is pure host code (no ctx, no device).  shape8: n, the usable rows, the blinding factors bf, the
 * permutation sets nsets, the lookups nl, nz = nsets + nl, the columns per permutation set chunk_len, and the draws per proof
 * nz * (bf + 1).  BZH_E_ARG, nothing written: a NULL pointer, an unknown curve, a blob that does not parse.
 *
 * bzh_grand_products_batch_device takes the witness over the domain, n = 2^k rows each, blinding rows in place: advice[b][na][n],
 * instance[b][ni][n], lookup_compressed[b][l][2][n] (the compressed input a_c, then the compressed table s_c) and
 * lookup_permuted[b][l][2][n] (the permuted pair a, s with their blinding rows); an operand whose count is 0 may be NULL.  The
 * fixed columns, sigma and the identity rows delta^j omega^r are the key's.  beta, gamma: one element per proof each, as
 * bzh_transcript_batch_squeeze writes them.  `form` and `mem` apply to every data pointer, as in the four calls above: with
 * BZH_MEM_DEVICE they are 16-byte-aligned device pointers (`status` any alignment) and the call only enqueues; with BZH_MEM_HOST
 * the operands are staged up once at the start and the outputs read back once at the end.  rng: proof b's 64-byte draws at
 * rng + b * rng_stride, in upstream's order -- per product, permutation sets first and then lookups, the bf blinding rows
 * n - bf .. n - 1 and then the blind --, so rng_stride >= 64 * nz * (bf + 1).
 * Messages, per proof: WRITE the nz commitments in product order, the coefficients committed under the drawn blinds.  The proof
 * grows by 32 * nz bytes; nothing is squeezed.
 * Outputs, in `form`: out_z[b][nz][n] (may be NULL), the products over the domain; out_z_polys[b][nz][n], their coefficients;
 * out_z_blinds[b][nz]; status (may be NULL), one byte per proof: 1 when the last permutation set's z[usable] is not 1 or a
 * lookup product's z[usable] is not 1 -- a copy constraint or a lookup of that witness does not hold --, else 0.  Such a proof
 * still gets its messages, disturbs no other proof, and the call returns BZH_OK; the bit is also ORed into the batch's sticky
 * status byte.  A zero denominator is left zero by the batch inversion, as upstream's batch_invert leaves it: that product is 0
 * from the next row on, in that proof alone.
 * One launch (k_gp_factors) writes the numerator and the denominator of every product's factors, reading the columns in place
 * through a table built from the key and uploaded before the first launch; the inversion, the product and the scan are those of
 * bzh_prove_batch; one launch (k_gp_finish) chains the permutation sets -- set i is its own scanned product times the z[usable]
 * of the sets before it --, places the blinding rows and the blinds and sets the status.  Between its first launch and its last
 * the call copies nothing that depends on a challenge to the host, does no host field arithmetic on such a value, adds no stream
 * synchronisation of its own and runs no expression program.  The scratch is the key's workspace for this ctx, under the rule
 * bzh_vanishing_batch_device states: a BZH_MEM_DEVICE call returns with its work queued on it, and the call that merges the
 * workspace's blocks waits once for the stream before its own first launch.  A key with nz == 0 returns BZH_OK with nothing
 * written.  Its speed against the host path: DESIGN.md section 7.
 * BZH_E_ARG, the batch left as it was and nothing written: a NULL ctx, pk, transcripts, rng, beta, gamma, out_z_polys,
 * out_z_blinds or required operand pointer; a host-resident batch; a batch of another ctx, curve or size; a key on another device
 * than ctx; batch == 0 or > 65535, or batch * nz > 65535 (the commitments of a batch are one launch with one row of its grid per
 * commitment); unknown form or mem; a misaligned device pointer; rng_stride too small.  BZH_E_RANGE, nothing absorbed: proof_cap
 * cannot take 32 * nz more bytes.  Every check that reads neither the key nor the device comes first, then those that read the
 * key; all of them come before the first use of ctx. */
int bzh_grand_products_plan(int curve, const uint8_t* circuit, size_t circuit_len, uint32_t shape8[8]);
int bzh_grand_products_batch_device(bzh_ctx* ctx, struct bzh_pk* pk, size_t batch, const uint64_t* advice, const uint64_t* instance,
                                    const uint64_t* lookup_compressed, const uint64_t* lookup_permuted, const uint64_t* beta,
                                    const uint64_t* gamma, int form, int mem, const uint8_t* rng, size_t rng_stride,
                                    struct bzh_transcript_batch* transcripts, uint64_t* out_z, uint64_t* out_z_polys, uint64_t* out_z_blinds,
                                    uint8_t* status);
/* The witness commitments of plonk::create_proof against a device-resident bzh_transcript_batch -- csrc/commitments_device.hpp,
 * csrc/commitments.hip, csrc/commitments_scalars.hpp: the instance and advice commitments, theta, the lookups' compressed and
 * permuted columns with their commitments, beta and gamma; the commit_instances(), commit_advice() and lookups() phases of
 * bzh_prove_batch as a leaf.  It is the head of the chain: its outputs are the operands of bzh_grand_products_batch_device and
 * bzh_vanishing_batch_device, and theta, beta, gamma land where those calls read them, so a witness goes in here and whole
 * proofs come out of the transcript batch after the opening with no challenge, scalar or point crossing to the host.
 *
 * bzh_commitments_plan is pure host code (no ctx, no device).  shape8: n, the usable rows, the blinding factors bf, num_advice na,
 * num_instance ni, the lookups nl, the draws per proof nd = na * (bf + 1) + na + nl * (2 * (bf + 1) + 2), and the proof bytes
 * appended, 32 * (na + 2 * nl).  BZH_E_ARG, nothing written: a NULL pointer, an unknown curve, a blob that does not parse.
 *
 * bzh_commitments_batch_device takes advice[b][na][n], the caller's witness over the domain, n = 2^k rows each -- its rows from
 * `usable` on are ignored and overwritten in the output, as in bzh_prove_batch -- and instances[b][ni][instance_rows], which is
 * padded with zeros to n; with instance_rows == 0 the instance columns are zero and `instances` is not read, NULL or not, as in
 * bzh_prove_batch.  `form` and `mem` apply to every data pointer, as in the four calls above: with BZH_MEM_DEVICE they are
 * 16-byte-aligned device pointers (`status` any alignment; `out` itself is a host struct) and the call only enqueues; with
 * BZH_MEM_HOST the operands are staged up once at the start and the outputs read back once at the end.  rng: proof b's 64-byte
 * draws at rng + b * rng_stride, in upstream's order -- the advice blinding rows usable .. n - 1, column by column; the na advice
 * blinds; then per lookup the bf + 1 rows of the permuted input, the bf + 1 rows of the permuted table, the input's blind, the
 * table's blind --, so rng_stride >= 64 * nd.
 * Messages, per proof, in upstream's order: COMMON each instance commitment (blind one); WRITE each advice commitment; squeeze
 * theta; per lookup WRITE the commitment of the permuted input and then of the permuted table; squeeze beta; squeeze gamma.  The
 * proof grows by 32 * (na + 2 * nl) bytes.  The key's vk_repr is NOT absorbed here: the caller does that first, with
 * bzh_transcript_batch_common_scalars, as for every batch.
 * Outputs, in `form`, through the struct bzh_commitments_out; a member whose count is 0 may be NULL.  Over the domain, blinding rows in
 * place: advice[b][na][n], instance[b][ni][n], lookup_compressed[b][nl][2][n] (a_c, then s_c), lookup_permuted[b][nl][2][n] --
 * the four operands of bzh_grand_products_batch_device.  Coefficients: advice_polys, instance_polys, lookup_polys[b][nl][2][n] --
 * operands of bzh_vanishing_batch_device.  Blinds: advice_blinds[b][na], lookup_blinds[b][nl][2].  Challenges: theta[b], beta[b],
 * gamma[b], as bzh_transcript_batch_squeeze writes them.  status (may be NULL), one byte per proof: bit 0 is set when a lookup of
 * that proof has an input that is not in its table (the device permutation's non-zero status word).  Such a proof still gets all
 * its messages -- a failed pair keeps every index in bounds and writes a reduced element in every row --, disturbs no other
 * proof, and the call returns BZH_OK; the bit is also ORed into the batch's sticky status byte.
 * One launch (k_cm_place) writes the advice and instance columns from the caller's arrays and the drawn rows, converting from
 * the caller's form in the same pass.  The lookups' compressed columns come from the key's cached expression programs, whose
 * constant tables one launch (k_cm_consts) builds on the device from theta where it was squeezed; one device permutation call
 * takes all batch * nl pairs; one launch (k_cm_lookup_finish) places their drawn rows and blinds and folds the status.  The
 * commitments take their blinds from device memory and are made in the basis the key offers: the evaluations against g_lagrange
 * when the key has that table (bzh_pk_set_lagrange), the coefficients against the SRS otherwise -- the same bytes.  Between its
 * first launch and its last the call copies nothing that depends on a challenge or on the permutation's status to the host, does
 * no host field or curve arithmetic on such a value and adds no stream synchronisation of its own; everything that depends on
 * the key and the operand pointers alone -- expression programs, column registries, descriptor tables -- is uploaded before the
 * first launch.  The scratch is the key's workspace for this ctx, under the rule bzh_vanishing_batch_device states: a
 * BZH_MEM_DEVICE call returns with its work queued on it, and the call that merges the workspace's blocks waits once for the
 * stream before its own first launch.  Its speed against the host path: DESIGN.md section 7.
 * BZH_E_ARG, the batch left as it was and nothing written: a NULL ctx, pk, transcripts, rng, out, required operand or required
 * output member; a host-resident batch; a batch of another ctx, curve or size; a key on another device than ctx; batch == 0 or
 * > 65535, or batch * max(na, ni, 2 * nl) > 65535 (the commitments of a kind are one launch with one row of its grid per
 * commitment); instance_rows > usable; unknown form or mem; a misaligned device pointer; rng_stride too small.  BZH_E_RANGE,
 * nothing absorbed and nothing squeezed: proof_cap cannot take 32 * (na + 2 * nl) more bytes; a lookup whose expressions do not
 * fit the expression interpreter.  That last refusal is decided when the call finds or compiles the key's cached programs, which
 * is after ctx is taken and the workspace reset, with at most the uploads of the programs before it queued on the stream; every other check comes before the
 * first use of ctx: first those that read neither the key nor the device, then those that read the key.  (The device
 * permutation takes at most 32767 pairs a call; batch * 2 * nl <= 65535 keeps batch * nl within that, so the shape it would
 * refuse is already BZH_E_ARG.)  The uploads that depend on the key and the operand pointers alone are the call's first work on
 * the stream -- the small upload kernels that carry them included --; a BZH_MEM_HOST call's operands are staged up after them. */
typedef struct {
    uint64_t *advice, *instance, *lookup_compressed, *lookup_permuted; /* over the domain */
    uint64_t *advice_polys, *instance_polys, *lookup_polys;            /* coefficients */
    uint64_t *advice_blinds, *lookup_blinds;
    uint64_t *theta, *beta, *gamma;
} bzh_commitments_out;
int bzh_commitments_plan(int curve, const uint8_t* circuit, size_t circuit_len, uint32_t shape8[8]);
int bzh_commitments_batch_device(bzh_ctx* ctx, struct bzh_pk* pk, size_t batch, const uint64_t* advice, const uint64_t* instances,
                                 size_t instance_rows, int form, int mem, const uint8_t* rng, size_t rng_stride,
                                 struct bzh_transcript_batch* transcripts, const bzh_commitments_out* out, uint8_t* status);
int bzh_ipa_verify(bzh_ctx* ctx, const bzh_bases* bases, const uint64_t* commitment_xy, const uint64_t* x3, const uint64_t* v,
                   const uint8_t* proof, size_t proof_len, bzh_transcript* transcript, const uint64_t* g0_u_w);

/* ---- whole proofs (halo2_proofs plonk::{keygen_pk, create_proof}; reference call sites benches/shot.rs:58-71,
 * benches/board.rs:51-71, src/circuits/shot.rs:915-930, src/circuits/board.rs:907-922) ----------------------
 * bzh_pk_create    keygen_pk for a circuit given as data (serialised constraint system + fixed assignment; the
 *                  format is documented at the top of csrc/prove.hip; produced by bzh_circuit_blob for the reference's circuits and by
 *                  bzh2.circuit_data.serialize_circuit for test circuits):
 *                  fixed / permutation polynomials in Lagrange, coefficient and extended-coset form, l_0 / l_last /
 *                  l_blind, resident on the device.  `srs`: n + 2 points G_0..G_(n-1), U, W with a window table
 *                  (bzh_bases_precompute).  LIFETIME: the key BORROWS `srs` (and the table given to
 *                  bzh_pk_set_lagrange): both must outlive the key -- free the key before bzh_params_free / bzh_bases_free.
 * bzh_prove_batch  create_proof for `batch` independent witnesses of that circuit in lockstep (one launch per kernel
 *                  class per protocol phase for all of them); every proof is byte-identical to proving its witness
 *                  alone.  advice: batch x num_advice x n field elements (`form`, `mem`; rows past the usable ones are
 *                  overwritten with blinding values); instances: batch x num_instance x instance_rows canonical
 *                  elements (host); rng: per proof, at offset b * rng_stride, 64 bytes per Field::random draw in
 *                  upstream's draw order (bzh_pk_info reports the byte count); proofs: batch records of
 *                  proof_stride bytes, lengths in proof_lens.  BZH_E_RANGE: a witness does not satisfy the circuit
 *                  (surplus quotient coefficients) or a lookup input is not in its table.
 *                  A key is shared, read-only state (upstream's &ProvingKey): several host threads may prove / verify on
 *                  ONE key concurrently, each through its own ctx -- the per-call workspace lives with the (key, ctx) pair
 *                  inside the library.  Calls through one ctx are serialised as everywhere else.
 *                  bzh_pk_free and bzh_pk_set_quotient_module change what those calls run on (workspaces of every ctx, the
 *                  loaded code object): both return BZH_E_ARG, leaving the key as it was, while a bzh_prove_batch /
 *                  bzh_verify_batch / bzh_vk_from_pk on the key has started on any ctx and not returned -- a call counts from
 *                  its entry into the library, also while it waits for its ctx -- and synchronise every device the key has a
 *                  workspace on before they release anything.  Starting a call on a key after its bzh_pk_free has returned
 *                  BZH_OK is the caller's error: join the proving threads first. */
typedef struct bzh_pk bzh_pk;
/* THE VERIFYING-KEY DIGEST.  The first thing upstream's create_proof and verify_proof absorb is pk.get_vk().hash_into(transcript)
 * (halo2_proofs 0.2.0 plonk.rs, UPSTREAM; the keys come from keygen_vk / keygen_pk at benches/shot.rs:59-61,
 * benches/board.rs:52-54,80-86, src/circuits/shot.rs:915-940, src/circuits/board.rs:907-932): one scalar,
 *     Fp::from_bytes_wide( Blake2b-512(personal = "Halo2-Verify-Key", (s.len() as u64).to_le_bytes() || s) ),
 *     s = format!("{:?}", vk.pinned())
 * -- a digest of Rust's Debug text of the pinned key (moduli, domain, every gate's expression tree as upstream's
 * Expression enum prints it, query lists, fixed + permutation commitments).  That text cannot be produced outside the
 * crate (the tree SHAPES of halo2_gadgets' 19 gates are upstream source, absent here: SURVEY F2), so the digest is an
 * INPUT of this boundary, not something the library derives:
 *   - a circuit blob carries it as 32 canonical little-endian bytes at BZH_CIRCUIT_BLOB_VK_REPR_OFFSET;
 *   - bzh_circuit_create fills in BZH_VK_REPR_PLACEHOLDER (0x1234); proofs made with it verify here (bzh_verify_batch
 *     absorbs the same value) but are REJECTED by the reference's verify_proof, and vice versa;
 *   - bzh_circuit_set_vk_repr installs the real one before bzh_circuit_blob / bzh_pk_create; the Rust-side shim obtains it
 *     once per key (INTEGRATION.md "The verifying-key digest": a 6-line capture transcript around vk.hash_into), or hands
 *     the Debug text to bzh_vk_digest;
 *   - bzh_circuit_vk_repr / bzh_pk_vk_repr report what a circuit / key carries, and whether it is still the placeholder.
 * BZH_E_RANGE: a repr that is not a canonical Fp element (Fp::from_repr(..) is None upstream). */
#define BZH_CIRCUIT_BLOB_VK_REPR_OFFSET 24
#define BZH_VK_REPR_PLACEHOLDER 0x1234
int bzh_vk_digest(const char* pinned_debug, size_t len, uint8_t* out_repr32);
int bzh_pk_vk_repr(const bzh_pk* pk, uint8_t* out_repr32, int* is_placeholder);
int bzh_pk_create(bzh_ctx* ctx, const bzh_bases* srs, const uint8_t* circuit, size_t circuit_len, bzh_pk** out);
int bzh_pk_free(bzh_ctx* ctx, bzh_pk* pk);
/* Params::commit_lagrange: with the table (g_lagrange | u | w) of bzh_params_create set, the instance, advice, permuted-lookup and
 * grand-product columns are committed in the Lagrange basis, as upstream does -- the same group elements (hence the same proof
 * bytes) as committing their coefficients to g, but sparse / small witness columns then cost the MSM almost nothing.
 * NULL returns to coefficient-basis commitments.  The table must outlive the key. */
int bzh_pk_set_lagrange(bzh_pk* pk, const bzh_bases* g_lagrange);
/* the quotient's evaluator program (compiled on the host at bzh_pk_create): instructions, field multiplications per
 * extended-domain row, LDS slots, proof-independent subexpressions hoisted into key-owned coset columns */
int bzh_pk_quotient_stats(bzh_pk* pk, uint32_t* ops, uint32_t* multiplications, uint32_t* lds_slots, uint32_t* hoisted_columns);
/* ... and its memory side: column operands loaded per extended-domain row, and how many of the slots hold column leaves
 * (a (column, rotation) value loaded once and read from its slot over a range of gate groups; BZH_VM2_LEAF, default 3) */
int bzh_pk_quotient_loads(bzh_pk* pk, uint32_t* loads_per_row, uint32_t* leaf_slots);
/* The quotient evaluator as compiled code.  The program depends on the circuit only (not on k, the SRS or a witness), so for
 * the reference's two circuits (ShotCircuit, BoardCircuit) the kernels are generated when the library is BUILT
 * (csrc/gen_quotient.cpp -> quotient_builtin.hip, linked into libbzh2.so) and picked up by bzh_pk_create through the program's
 * hash: no compiler is needed where the library runs.  For any other circuit bzh_pk_quotient_source returns the key's program
 * as straight-line HIP source (*len = its length, copied NUL-terminated into buf when buf != NULL): compile it for gfx950
 * against csrc/field.cuh (`hipcc -O3 -std=c++17 --offload-arch=gfx950 --genco -I <csrc>`, ~5 s; or hiprtc) and hand the code
 * object to bzh_pk_set_quotient_module, which selects it (BoardCircuit, 64 x 2^17 rows: 35.5 ms against the interpreter's 49.5 ms;
 * same proof bytes).  A module generated from another program is refused (BZH_E_ARG: it carries the program's hash); NULL / 0
 * unloads the module and returns to the key's default (the builtin kernel if there is one, else the interpreter).
 * bzh_pk_quotient_select picks explicitly (BZH_E_RANGE when that flavour is not available for this key);
 * bzh_pk_quotient_selected reports the current choice and whether a builtin kernel exists.  Environment: BZH_QUOTIENT=interp
 * makes the interpreter every new key's default. */
typedef enum { BZH_QUOTIENT_INTERPRETER = 0, BZH_QUOTIENT_BUILTIN = 1, BZH_QUOTIENT_MODULE = 2 } bzh_quotient_flavour;
int bzh_pk_quotient_source(bzh_pk* pk, char* buf, size_t cap, size_t* len);
int bzh_pk_set_quotient_module(bzh_ctx* ctx, bzh_pk* pk, const void* code_object, size_t len);
int bzh_pk_quotient_select(bzh_pk* pk, int flavour);
int bzh_pk_quotient_selected(bzh_pk* pk, int* flavour, int* builtin_available);
/* Where bzh_prove_batch permutes the lookup argument's columns: BZH_LOOKUP_DEVICE (every new key's default) runs
 * bzh_permute_expression_pair_batch's kernels on the ctx's stream; the one status word per proof comes back with the lookup's
 * commitments, without a stream synchronisation of its own.  BZH_LOOKUP_HOST moves the compressed columns to pinned host memory
 * and sorts them on host threads (bzh_permute_expression_pair per proof).  Same proof bytes and statuses either way: a lookup
 * input without a table copy is BZH_E_RANGE, and nothing of that batch is written.  A key on which bzh_pk_lookup_select was never
 * called reports BZH_LOOKUP_DEVICE and chooses per call: the device for a batch of 8 proofs or more, the host path below that
 * (a single proof is 0.1 ms slower with the one-workgroup launches the device path makes for it); a call of
 * bzh_pk_lookup_select fixes the choice for every batch size.  BZH_E_ARG: NULL key or an unknown value. */
typedef enum { BZH_LOOKUP_HOST = 0, BZH_LOOKUP_DEVICE = 1 } bzh_lookup_where;
int bzh_pk_lookup_select(bzh_pk* pk, int where);
int bzh_pk_lookup_selected(bzh_pk* pk, int* where);
/* Where the quotient reads the per-proof columns (advice, instance, grand products, permuted lookup columns) in bzh_prove_batch,
 * bzh_prove_batch_seeded, bzh_vanishing_batch_device and everything built on it (bzh_prove_batch_device[_seeded],
 * bzh_prove_shots_device, bzh_prove_boards_device).  BZH_WORKSPACE_EXTENDED (every new key's default): each of them on the whole
 * extended coset, 8 n elements, until the call ends.  BZH_WORKSPACE_COSETWISE: none of them is ever taken there; the extended
 * domain is eight cosets of the n-sized one, and for each coset the coefficient forms go through one n-point transform into
 * n-sized buffers that are reused, followed by one launch of the interpreter for the batch (k_expr_vm2_cosets) that reads the
 * key's columns where they lie and writes its share of the quotient's 8 n values.  Same quotient, same proof bytes, same
 * statuses; an eighth of the memory for these columns (bzh_workspace_plan), eight launches and eight transforms where there was
 * one of each.  COSETWISE OVERRIDES THE QUOTIENT FLAVOUR: the quotient always runs the interpreter in this mode -- the builtin
 * kernels and loaded modules index 8 n columns -- while bzh_pk_quotient_selected keeps reporting the caller's choice, which is
 * in force again after a return to BZH_WORKSPACE_EXTENDED.  A circuit the interpreter does not fit, or an extended domain other
 * than 8 n, makes the prove calls return BZH_E_RANGE in this mode.  BZH_E_ARG: NULL key or an unknown value. */
typedef enum { BZH_WORKSPACE_EXTENDED = 0, BZH_WORKSPACE_COSETWISE = 1 } bzh_workspace_mode;
int bzh_pk_workspace_select(bzh_pk* pk, int mode);
int bzh_pk_workspace_selected(bzh_pk* pk, int* mode);
/* What one prove call of `batch` proofs takes from the key's per-ctx arena in `mode`, in bytes: pure host code (no ctx, no
 * device), like bzh_vanishing_plan.  The figure is the sum of the items below, which count the call's column-sized buffers as
 * the phases allocate them, plus an allowance for what the launches stage; it is not below the arena's high-water mark
 * (bzh_pk_workspace_peak) and above it by no more than the allowance for the batches the tests run; `cosets_bytes` is the term the mode
 * changes, and the prover carves its coset-wise buffers with the sizes this same function computes.  cosets_extended_bytes is
 * that term in BZH_WORKSPACE_EXTENDED whatever `mode` is: the two modes' totals differ by 7/8 of it.  Apart from the coset term
 * the items are a MODEL of the phases' allocations, held against the arena only for the Shot circuit at k = 11, batch 3; for
 * other circuits and sizes nothing has compared it with an arena, and a circuit with more lookups or a larger quotient
 * program can stage more than the allowance: size with a margin, or read bzh_pk_workspace_peak after a first call.  In EXTENDED mode with the
 * builtin quotient kernel in unsaturated limbs the columns take 9/8 of the figure (36 bytes an element).  BZH_E_ARG: a blob
 * that does not parse, batch 0 or above 65535, an unknown mode, a NULL argument. */
typedef struct bzh_workspace_items {
    uint64_t n, extended;             /* rows of the domain | of the extended domain */
    uint64_t columns;                 /* per-proof columns the quotient reads */
    uint64_t column_bytes;            /* one of them where the quotient reads it: 32 * extended | 32 * n */
    uint64_t cosets_bytes;            /* all of them for the batch, in `mode` */
    uint64_t cosets_extended_bytes;   /* ... in BZH_WORKSPACE_EXTENDED */
    uint64_t witness_bytes;           /* the per-proof columns over the domain and as coefficients, the grand products' factors */
    uint64_t quotient_bytes;          /* h: 32 * extended per proof */
    uint64_t tail_bytes;              /* the largest stretch after the quotient: random polynomial, pieces, evaluation gather or multiopen */
    uint64_t staging_bytes;           /* an allowance for what the launches stage (programs, constants, blinds): 1 MiB + 64 KiB a proof */
    uint64_t total_bytes;             /* their sum: what bzh_workspace_plan returns */
} bzh_workspace_items;
int bzh_workspace_plan(int curve, const uint8_t* circuit, size_t circuit_len, size_t batch, int mode, size_t* arena_bytes);
int bzh_workspace_plan_items(int curve, const uint8_t* circuit, size_t circuit_len, size_t batch, int mode, bzh_workspace_items* items);
/* The high-water mark of the key's arenas, in bytes handed out at once, since the start of the LAST call on each ctx (the
 * largest over the ctxs that have used the key; 0 before any call): what bzh_workspace_plan is an estimate of.  Read it when no
 * call is running on the key.  BZH_E_ARG: a NULL argument. */
int bzh_pk_workspace_peak(const bzh_pk* pk, size_t* arena_bytes);
/* Where bzh_verify_batch decompresses the points of the proofs: BZH_VERIFY_POINTS_HOST inside the per-proof host pass, one
 * square root at a time (every new key's default); BZH_VERIFY_POINTS_DEVICE gathers the 32-byte strings of the whole batch --
 * their offsets in a proof depend on the key only --, decompresses them in one bzh_affine_decompress launch on the ctx's
 * stream ahead of the instance commitments, and the host pass replays the transcript over the decoded points.  Same
 * results[] either way.  BZH_E_ARG: NULL key or an unknown value. */
typedef enum { BZH_VERIFY_POINTS_HOST = 0, BZH_VERIFY_POINTS_DEVICE = 1 } bzh_verify_points_where;
int bzh_pk_verify_select(bzh_pk* pk, int where);
int bzh_pk_verify_selected(bzh_pk* pk, int* where);
/* Where bzh_verify_batch runs the per-proof pass between the instance commitments and the IPA check -- the transcript replay,
 * the point decompressions, expected h(x), the multiopen recombination and the IPA scalars: BZH_VERIFY_PASS_HOST on host threads,
 * one proof each (every new key's default); BZH_VERIFY_PASS_DEVICE on the ctx's stream for the whole batch in lockstep -- the
 * proof bytes go up once, one decompression launch, one batch of device transcripts, the key's scalar program one lane per
 * proof (csrc/verify_program.hpp) -- and only two Jacobian sums and one reject byte per proof come back.  It implies device
 * decompression whatever bzh_pk_verify_select says.  Same results[] either way; its speed has not been measured (DESIGN.md
 * section 7).  BZH_E_ARG: NULL key or an unknown value, and the key keeps its selection.  A verify call under
 * BZH_VERIFY_PASS_DEVICE on a key whose shape has no program (a degree no circuit reaches) is BZH_E_RANGE. */
typedef enum { BZH_VERIFY_PASS_HOST = 0, BZH_VERIFY_PASS_DEVICE = 1 } bzh_verify_pass_where;
int bzh_pk_verify_pass_select(bzh_pk* pk, int where);
int bzh_pk_verify_pass_selected(bzh_pk* pk, int* where);
/* Host only (no ctx, no GPU): the quotient program of a circuit blob as the source text of a BUILTIN kernel (namespace
 * bzh_q_<hash> with the kernel bzh_quotient_<hash> and a host function `launch`), and the program hash.  This is what the
 * build-time generator calls; BZH_E_RANGE if the circuit does not fit the evaluator (such circuits use the VM v1 fold). */
int bzh_quotient_source_for_circuit(int curve, const uint8_t* circuit, size_t circuit_len, char* buf, size_t cap, size_t* len,
                                    uint64_t* program_hash);
/* Host only: the quotient program itself, as the interpreter runs it and the kernels are generated from it.  ops: 16-byte
 * instructions {u8 code = form << 4 | operation << 2 | register, u8 a_kind, u8 b_kind, u8 0, i32 a_idx, i32 b_idx, i16 a_rot,
 * i16 b_rot} (forms, operations and operand kinds: csrc/exprvm.hip); consts: 40-byte entries {i32 symbol (< 0: a literal), u32 0,
 * u32 value[8] (the literal, Montgomery form)}.  *nops / *nconsts are the counts; a buffer is filled when it is non-NULL and
 * its capacity in bytes suffices (BZH_E_ARG otherwise).  stats8 (may be NULL): instructions, multiplications per row, slots,
 * column loads per row, slots holding column leaves, the first of those slots, hoisted columns, 0. */
int bzh_quotient_program_for_circuit(int curve, const uint8_t* circuit, size_t circuit_len, void* ops, size_t ops_cap, size_t* nops,
                                     void* consts, size_t consts_cap, size_t* nconsts, uint32_t* stats8);
/* Host only: the terms of a circuit's quotient numerator (gate constraints with their compressed selectors, permutation and
 * lookup argument terms, in protocol order) by polynomial degree -- polys[d] terms of degree d (in units of n - 1, d < 16) and
 * muls[d] field multiplications in their expression trees.  A term of degree d vanishes on the 2^k-row domain by itself, so its
 * share of h(X) could be computed from (d - 1) n evaluations instead of the extended domain's; the histogram says what that
 * would buy (halo2's selector compression pads nearly every gate of the reference's circuits to degree
 * 7 - 9, so for them it buys ~3 %). */
int bzh_quotient_degree_histogram(int curve, const uint8_t* circuit, size_t circuit_len, uint32_t* polys16, uint32_t* muls16);
/* launcher of one builtin kernel, and the table the generated file exports (used inside the library) */
typedef void (*bzh_quotient_launch_fn)(unsigned grid_x, unsigned grid_y, void* hip_stream, const uint32_t* const* cols, const size_t* strides,
                                       const uint32_t* consts, size_t const_stride, size_t size, uint32_t* out);
/* launch29 (may be NULL): the same program in unsaturated 9 x 29-bit limbs (csrc/fe29.cuh: 188-instruction products without carry
 * instructions).  Its columns are fe29 planes (9 * size words per column: limbs 0-3 | limbs 4-7 | limb 8), `strides` in words
 * between proofs, constants 12 words apart (9 used), `out` saturated as for `launch`. */
typedef struct { uint64_t program_hash; bzh_quotient_launch_fn launch; const char* name; bzh_quotient_launch_fn launch29; } bzh_builtin_quotient;
const bzh_builtin_quotient* bzh_builtin_quotients(size_t* count);
int bzh_pk_info(const bzh_pk* pk, size_t* rng_bytes_per_proof, size_t* max_proof_bytes, uint32_t* num_advice, uint32_t* n_rows,
                uint32_t* usable_rows);
/* bzh_verify_batch  plonk::verify_proof (SingleVerifier; benches/board.rs:80-86) for `batch` proofs of the key's circuit:
 *                  results[b] = 1 if proof b verifies against instances b, else 0 (malformed proofs included).
 *                  g0_u_w: G_0, U, W of the SRS as 3 affine canonical points; they are checked against the SRS the key
 *                  was built on (BZH_E_ARG if they differ: a stale copy would otherwise reject every valid proof). */
int bzh_verify_batch(bzh_ctx* ctx, bzh_pk* pk, size_t batch, const uint64_t* instances, size_t instance_rows, const uint8_t* proofs,
                     size_t proof_stride, const size_t* proof_lens, const uint64_t* g0_u_w, int* results);
int bzh_prove_batch(bzh_ctx* ctx, bzh_pk* pk, size_t batch, const uint64_t* advice, int form, int mem, const uint64_t* instances,
                    size_t instance_rows, const uint8_t* rng, size_t rng_stride, uint8_t* proofs, size_t proof_stride,
                    size_t* proof_lens);

/* ---- the verifying key (halo2_proofs plonk::{keygen_vk, VerifyingKey}; the reference's verify_board / verify_shot run keygen_vk
 * only, src/wasm/circuit_wasm.rs:97-111,180-194; benches/board.rs:80-86 verifies through pk.get_vk()) ---------------------------
 * What verify_proof reads of a key and nothing else: curve, k, the verifying-key digest, the constraint system (gates, lookups,
 * query lists, permutation columns -- no fixed assignment), the commitments to the fixed and permutation polynomials, and the
 * multiopen structure derived from those.  A bzh_vk is host memory only, immutable and tied to no device: it owns no device
 * allocation (the per-call workspace of a verification lives with the (key, ctx) pair inside the library, as for bzh_pk), and
 * several host threads may verify on ONE key concurrently, each through its own ctx.
 *   bzh_vk_create        keygen_vk: parses the blob, builds the permutation polynomials, commits the fixed and permutation columns
 *                        (blind 1) against `srs` (n + 2 points, as for bzh_pk_create), keeps the commitments and releases every
 *                        column before it returns.  No quotient program, no cosets, no hoisted or fe29 columns are made.
 *   bzh_vk_from_pk       pk.get_vk(): the same bytes as bzh_vk_create on the pk's blob and SRS (fills the pk's lazy commitments
 *                        if they have not been computed yet).
 *   bzh_vk_write / read  VerifyingKey::write / read in THIS LIBRARY'S OWN FORMAT "BZV1" (layout at the top of
 *                        csrc/verifying_key.hpp; not upstream's, which stores the commitments only and re-derives the constraint
 *                        system from the Circuit type).  out == NULL: size query; a cap below *len is BZH_E_ARG and nothing is
 *                        written.  bzh_vk_read is host only -- no ctx, no device, no keygen -- and validates everything the
 *                        verifier will index with: truncated / corrupt / wrong-magic input is BZH_E_ARG, a coordinate >= p or a
 *                        point off the curve BZH_E_RANGE.
 *   bzh_vk_info          any out pointer may be NULL.
 *   bzh_vk_device_bytes / bzh_pk_device_bytes
 *                        the library's own bookkeeping of device memory held under a key: *key_bytes = allocations that live as
 *                        long as the key (always 0 for a bzh_vk; columns, cosets, hoisted and fe29 columns for a bzh_pk),
 *                        *workspace_bytes = the per-(key, ctx) workspaces calls have grown so far.  Either may be NULL.
 *   bzh_vk_free          BZH_E_ARG, leaving the key as it was, while a bzh_verify_batch_vk on it has started (a call counts from
 *                        its entry into the library, also while it waits for its ctx) and not returned.  Starting a call on a
 *                        key after its bzh_vk_free has returned BZH_OK is the caller's error.
 *   bzh_verify_batch_vk  bzh_verify_batch with the key and the SRS apart.  srs: (g | u | w) with its window table; g_lagrange:
 *                        (g_lagrange | u | w) or NULL; the other arguments and results[] exactly as bzh_verify_batch; g0_u_w is
 *                        checked against `srs`.  With g_lagrange the instance columns are committed as upstream's commit_lagrange
 *                        does -- their instance_rows values against the first instance_rows points of g_lagrange, plus W -- and
 *                        nothing proportional to n is allocated for them; with NULL they go through an inverse NTT and an n-term
 *                        MSM against srs, as in bzh_verify_batch.  The same points, hence the same results[], either way.
 *                        A proof of another circuit or another k is results[b] = 0, not an error. */
typedef struct bzh_vk bzh_vk;
int bzh_vk_create(bzh_ctx* ctx, const bzh_bases* srs, const uint8_t* circuit, size_t circuit_len, bzh_vk** out);
int bzh_vk_from_pk(bzh_ctx* ctx, bzh_pk* pk, bzh_vk** out);
int bzh_vk_write(const bzh_vk* vk, uint8_t* out, size_t cap, size_t* len);
int bzh_vk_read(const uint8_t* bytes, size_t len, bzh_vk** out);
int bzh_vk_info(const bzh_vk* vk, int* curve, unsigned* k, uint32_t* num_instance, uint32_t* num_fixed_commitments,
                uint32_t* num_permutation_commitments, size_t* max_proof_bytes);
int bzh_vk_vk_repr(const bzh_vk* vk, uint8_t* out_repr32, int* is_placeholder);
int bzh_vk_device_bytes(const bzh_vk* vk, size_t* key_bytes, size_t* workspace_bytes);
int bzh_pk_device_bytes(const bzh_pk* pk, size_t* key_bytes, size_t* workspace_bytes);
int bzh_vk_free(bzh_vk* vk);
int bzh_verify_batch_vk(bzh_ctx* ctx, const bzh_vk* vk, const bzh_bases* srs, const bzh_bases* g_lagrange, size_t batch,
                        const uint64_t* instances, size_t instance_rows, const uint8_t* proofs, size_t proof_stride,
                        const size_t* proof_lens, const uint64_t* g0_u_w, int* results);
/* bzh_verify_batch_vk with the choice of bzh_verify_pass_where per call (a bzh_vk is immutable and shared between threads, so
 * it carries no selection): bzh_verify_batch_vk is pass_where = BZH_VERIFY_PASS_HOST.  BZH_E_ARG for an unknown value. */
int bzh_verify_batch_vk_with(bzh_ctx* ctx, const bzh_vk* vk, const bzh_bases* srs, const bzh_bases* g_lagrange, int pass_where,
                             size_t batch, const uint64_t* instances, size_t instance_rows, const uint8_t* proofs, size_t proof_stride,
                             const size_t* proof_lens, const uint64_t* g0_u_w, int* results);

/* create_proof with the randomness drawn inside the library, as the reference does from OsRng (benches/shot.rs:68): proof b's
 * stream is ChaCha20 keyed by seeds[b] (32 bytes; 64-bit block counter from 0, zero nonce), block i being the i-th 64-byte draw
 * (ff::Field::random), expanded on the device -- no rng_bytes_per_proof (2 MB at k = 14) to generate and upload per proof.
 * The proofs are exactly those of bzh_prove_batch fed with bzh_rng_expand(seeds[b], 0, rng_bytes_per_proof / 64, ..).
 * SECURITY: every blinding factor of proof b is a function of seeds[b]; the seeds (and the bytes given to bzh_prove_batch)
 * MUST come from a cryptographically secure generator (getrandom(2), OsRng, os.urandom), fresh per proof -- a predictable or
 * reused seed voids zero-knowledge.  Fixed seeds are for tests and benchmarks only. */
int bzh_prove_batch_seeded(bzh_ctx* ctx, bzh_pk* pk, size_t batch, const uint64_t* advice, int form, int mem, const uint64_t* instances,
                           size_t instance_rows, const uint8_t* seeds, uint8_t* proofs, size_t proof_stride, size_t* proof_lens);
/* host: draws [first_draw, first_draw + draws) of the stream of `seed`, 64 bytes each, into out */
int bzh_rng_expand(const uint8_t* seed, uint64_t first_draw, size_t draws, uint8_t* out);
/* host, no ctx, no device: the weights of an accumulated batch verification (bzh_verify_records_accumulated,
 * bzh_verify_batch_vk_accumulated, bzh_ipa_check_accumulated).  out[b] (4 canonical limbs) = draw b of bzh_rng_expand(seed, b, 1, ..),
 * 64 bytes, reduced into the scalar field of `curve` (BZH_CURVE_VESTA / BZH_CURVE_PALLAS) exactly as bzh_random_field reduces a
 * 64-byte draw (from_bytes_wide).  BZH_E_ARG: a NULL seed, a NULL out with batch != 0, another curve.
 * SECURITY: the weights of a batch are a function of `seed`; the seed MUST come from a cryptographically secure generator
 * (getrandom(2), OsRng, os.urandom), fresh per call and drawn AFTER the records of the batch are fixed.  With a seed the proofs'
 * author can predict, invalid proofs can be made to cancel each other and the batch is accepted.  With an unpredictable seed a batch
 * that contains an invalid included proof passes the accumulated check with probability at most 1/|F|.  Fixed seeds are for tests
 * and benchmarks only. */
int bzh_accumulation_weights(int curve, const uint8_t seed[32], size_t batch, uint64_t* out);

/* THE DEVICE-RESIDENT BATCH PROVER: create_proof as ONE call that runs the five leaves above -- the witness commitments, the grand
 * products, the vanishing argument, the evaluations and the multiopen with its opening -- on one device transcript batch inside the
 * library.  It takes what bzh_prove_batch takes and returns what it returns, and additionally reports failures PER PROOF.
 * advice, form, mem, instances (host, canonical), instance_rows (0 is accepted, `instances` is then not read), rng / rng_stride (or
 * seeds), proofs, proof_stride and proof_lens mean what they mean in bzh_prove_batch / bzh_prove_batch_seeded; with
 * BZH_MEM_DEVICE `rng` may also be a device pointer (16-byte aligned, rng_stride a multiple of 16) -- the chain's natural position:
 * the draws are then read where they lie.  proofs, proof_lens and status are host memory.  The proofs are byte-identical to
 * bzh_prove_batch's for the same key, witness and draws, and bzh_prove_batch_device_seeded's to bzh_prove_batch_seeded's: it
 * expands every proof's stream on the device with the same ChaCha20 expansion (bzh_rng_expand), no draw is generated or uploaded by
 * the host.
 * status, one byte per proof, folds the four leaves' per-proof bytes: bit 0 a lookup input is not in its table, bit 1 a grand product
 * does not close, bit 2 the quotient's degree check failed, bit 3 the multiopen or the opening flagged the proof (coincident points,
 * u_j = 0).  A flagged proof still gets all its bytes and disturbs no other proof.  With status != NULL the call returns BZH_OK and
 * the caller reads the bytes; with status == NULL a batch with any flagged proof returns BZH_E_RANGE and writes nothing, as
 * bzh_prove_batch fails the whole batch, and bzh_last_error names the first flagged proof and its bits.
 * bzh_prove_device_plan is host only (no ctx, no device).  shape8: the draws per proof of the four drawing leaves in chain order
 * (commitments, grand products, vanishing, multiopen with the opening); their sum (= rng_bytes_per_proof / 64 of bzh_pk_info); the
 * proof bytes; nown, the polynomials of a proof that get opened (instance, advice, the random polynomial, grand products, permuted
 * lookup columns, h(X)); the largest batch the call accepts, 65535 / max(na, ni, 2 * nl, nz, npieces): the commitments of a kind
 * are one launch with one row of its grid per commitment.
 * Inside, under the key's guard and in the key's workspace for this ctx: a new device transcript batch absorbs the key's vk_repr;
 * the five leaf bodies run without their entry points' second round of argument checks; the proofs, the status bytes and the
 * lengths are read back once.  The query lists and the rotation list of the evaluations and the multiopen are built from the key's
 * own constraint system in upstream's order when the key first needs them and kept with the key.  The fixed and permutation
 * polynomials are the key's own, with blind 1, read in place.  No copy of size n is made between the leaves: the evaluations and
 * the multiopen read every polynomial where its leaf left it, through a table of (pointer, per-proof stride); one launch
 * (k_pd_blinds) gathers the [batch][nown] blind row of the multiopen, one (k_pd_status) folds the status bytes.  With g_lagrange
 * (bzh_pk_set_lagrange) the grand products are committed in the Lagrange basis as well -- the same bytes.  The digest, the blinds
 * of the key's polynomials and the blind table's sources go up before the first launch, and each leaf body uploads its programs,
 * registries and descriptor tables as its first work on the stream; after that the call only enqueues, makes ONE stream wait at
 * the end for the read-back, and the one-time wait of the call that merges the workspace's blocks.  No challenge, scalar or point
 * comes to the host before that read-back.  Its speed against bzh_prove_batch: DESIGN.md section 5.
 * BZH_E_ARG, nothing written and the key usable: what bzh_prove_batch refuses (a NULL ctx, pk, advice, rng / seeds, proofs or
 * proof_lens; batch == 0; unknown form or mem; BZH_MEM_DEVICE with canonical form; a key on another device than ctx; rng_stride
 * below rng_bytes_per_proof; instance_rows > usable; instance rows without `instances`), a batch above the plan's limit, a
 * misaligned device pointer.  BZH_E_RANGE, likewise: a key without a VM v2 quotient program (or an extended domain below its
 * workgroup), a lookup whose expressions do not fit the expression interpreter, a circuit whose queries the evaluations or the
 * multiopen do not take, a proof_stride below the proof bytes.  Every check but the lookup's (decided when the commitments leaf
 * finds or compiles the key's cached programs) and the alignment of a device `rng` comes before the first use of ctx. */
int bzh_prove_device_plan(int curve, const uint8_t* circuit, size_t circuit_len, uint32_t shape8[8]);
int bzh_prove_batch_device(bzh_ctx* ctx, bzh_pk* pk, size_t batch, const uint64_t* advice, int form, int mem, const uint64_t* instances,
                           size_t instance_rows, const uint8_t* rng, size_t rng_stride, uint8_t* proofs, size_t proof_stride,
                           size_t* proof_lens, uint8_t* status);
int bzh_prove_batch_device_seeded(bzh_ctx* ctx, bzh_pk* pk, size_t batch, const uint64_t* advice, int form, int mem,
                                  const uint64_t* instances, size_t instance_rows, const uint8_t* seeds, uint8_t* proofs, size_t proof_stride,
                                  size_t* proof_lens, uint8_t* status);

/* ---- Params::new (halo2_proofs poly::commitment::Params; benches/shot.rs:58, benches/board.rs:51, and on every call of
 * the wasm exports, src/wasm/circuit_wasm.rs:57,97,145,180) -------------------------------------------------------
 * A pure function of k: g[i] = hash_to_curve("Halo2-Parameters")(0u8 || i as u32 LE), g_lagrange = inverse group FFT of
 * g, w = hash_to_curve(..)([1]), u = hash_to_curve(..)([2]) on Vesta.
 *   bzh_hash_to_curve      pasta_curves' CurveExt::hash_to_curve(domain_prefix)(msg) on Pallas / Vesta (host): the reference's
 *                          own call site is src/utils/pedersen.rs:19-21 ("battlezips:hash2curve", b"v" / b"r").
 *   bzh_params_generators  g (n x 8 canonical limbs), w, u on the host (threads over i; 0 = auto).
 *   bzh_group_ifft         g -> g_lagrange on the device (n/2 log n + n point-by-scalar multiplications).
 *   bzh_params_create      both of the above, cached on disk keyed by (curve, k) under cache_dir (NULL: next to the library
 *                          or $BZH_CACHE_DIR; "": no cache), then the two commitment-base tables (g | u | w) and
 *                          (g_lagrange | u | w) uploaded with fixed-base window tables: what bzh_pk_create /
 *                          bzh_pk_set_lagrange take.  The params own the tables (bzh_params_free releases them). */
typedef struct bzh_params bzh_params;
int bzh_hash_to_curve(int curve, const char* domain_prefix, const uint8_t* msg, size_t len, uint64_t* out_xy);
int bzh_params_generators(unsigned k, uint64_t* g_xy, uint64_t* w_xy, uint64_t* u_xy, unsigned threads);
int bzh_group_ifft(bzh_ctx* ctx, int curve, const uint64_t* g_xy, unsigned k, uint64_t* out_xy);
int bzh_params_create(bzh_ctx* ctx, unsigned k, const char* cache_dir, int window_bits, bzh_params** out);
int bzh_params_free(bzh_ctx* ctx, bzh_params* p);
int bzh_params_bases(const bzh_params* p, bzh_bases** g, bzh_bases** g_lagrange);
int bzh_params_points(const bzh_params* p, uint64_t* g_xy, uint64_t* g_lagrange_xy, uint64_t* w_xy, uint64_t* u_xy, int* from_cache);

/* ---- batched hash-to-curve (csrc/hash_to_curve.hip): one lane per message, two kernels (expand_message_xmd over BLAKE2b,
 * then iso_map(swu(u0) + swu(u1))) around the functions the host path runs ------------------------------------------------
 * The conventions are bzh_affine_decompress's: `mem` applies to msgs / u01, out_xy and status; device buffers are 16-byte
 * aligned; ctx == NULL with BZH_MEM_HOST runs on the host; with BZH_MEM_DEVICE and a status buffer the call only enqueues.
 * out_xy: n affine points x || y in `form`.  status (may be NULL): one bzh_point_status byte per message -- BZH_POINT_IDENTITY
 * (and zeros) for a result at infinity, else BZH_POINT_OK; with status == NULL the call returns BZH_E_RANGE if any result is the
 * identity.  n == 0 returns BZH_OK.
 *   bzh_hash_to_curve_batch       CurveExt::hash_to_curve(domain_prefix)(msg_i) for n messages of msg_len bytes each
 *                                 (contiguous), Pallas or Vesta.  BZH_E_ARG: another curve, msg_len > 128, a DST
 *                                 (prefix + "-" + curve + "_XMD:BLAKE2b_SSWU_RO_") longer than 255 bytes, n > 2^28.
 *   bzh_map_to_curve_batch        the map alone: u01 = n x 2 base-field elements (u0 || u1, `form`).  A u that is not below p:
 *                                 host operands are checked first (BZH_E_RANGE, nothing is written); a lane of device operands
 *                                 gets BZH_POINT_INVALID and zeros (BZH_E_RANGE when status == NULL).
 *   bzh_params_generators_device  g[first .. first + count) of Params::new on the device (Vesta); nothing is uploaded.
 *                                 BZH_E_RANGE if first + count > 2^32 (the message holds the index as a u32).
 *   bzh_params_create_with        bzh_params_create with the maker of g on a cache miss chosen: BZH_GENERATORS_HOST is
 *                                 bzh_params_create itself; BZH_GENERATORS_DEVICE makes g with the kernels above and hands it
 *                                 to the group FFT on the device (g is read back once).  Same points, byte-identical cache file;
 *                                 a cache hit ignores the argument.  BZH_E_ARG for any other value. */
int bzh_hash_to_curve_batch(bzh_ctx* ctx, int curve, const char* domain_prefix, const uint8_t* msgs, size_t msg_len, size_t n, int form,
                            int mem, uint64_t* out_xy, uint8_t* status);
int bzh_map_to_curve_batch(bzh_ctx* ctx, int curve, const uint64_t* u01, size_t n, int form, int mem, uint64_t* out_xy, uint8_t* status);
int bzh_params_generators_device(bzh_ctx* ctx, size_t first, size_t count, int form, int mem, uint64_t* g_xy);
typedef enum { BZH_GENERATORS_HOST = 0, BZH_GENERATORS_DEVICE = 1 } bzh_generators_where;
int bzh_params_create_with(bzh_ctx* ctx, unsigned k, const char* cache_dir, int window_bits, int generators_where, bzh_params** out);

/* ---- Params files in halo2's byte format (csrc/params_file.hpp, csrc/params_file.hip, csrc/params.hip) -----------------
 * halo2_proofs 0.2.0's Params::write / Params::read: k as a u32 little-endian, the n = 2^k points of g, the n points of
 * g_lagrange, w, u -- every point the 32-byte to_bytes string bzh_affine_compress writes; 4 + 32 (2 n + 2) bytes.  The way a
 * Rust caller hands over ITS Params and gets a bzh_params back, and the only SRS file the library reads that
 * is checked.  The field order is stated from upstream's source as remembered and has NOT been compared with a file that Rust
 * wrote; it lives in csrc/params_file.hpp alone.
 *   bzh_params_file_info  host only, no ctx: header and length.  BZH_E_ARG: NULL bytes, len < 4, k above 24 (what
 *                         bzh_params_generators takes), len != 4 + 32 (2 n + 2).  k and n_points may be NULL.
 *   bzh_params_encode     host only, no ctx: canonical affine limbs (g_xy, g_lagrange_xy: n x 8; w_xy, u_xy: 8) -> the byte string.
 *                         *len is always set to the file's size.  out == NULL: the size query, nothing else is read.  BZH_E_ARG
 *                         with nothing written: cap below that size, a NULL point array, k above 24, a NULL len.
 *   bzh_params_write      the same for the points of a bzh_params: they are compressed by bzh_affine_compress_batch on the ctx's
 *                         device.  out == NULL: the size query (ctx may then be NULL).  BZH_E_ARG as above.
 *   bzh_params_read       the byte string -> a bzh_params that cannot be told from bzh_params_create's for the same points: the
 *                         tables (g | u | w) and (g_lagrange | u | w | g_0) with window tables of `window_bits` (0: the planner's),
 *                         the host copies bzh_params_points serves, from_cache = 0.  `check` says how much of the file is believed:
 *       BZH_PARAMS_CHECK_POINTS    every string is a canonical encoding of a point that is not the identity (the status of
 *                                  bzh_affine_decompress).  Upstream's from_bytes accepts 32 zero bytes; a generator at infinity
 *                                  is never a valid SRS, so this library refuses it.
 *       BZH_PARAMS_CHECK_LAGRANGE  and g_lagrange is the inverse group FFT of g.  The matrix M_ji = n^-1 omega^-ij that
 *                                  bzh_group_ifft applies is symmetric, so for any r: sum_j r_j g_lagrange[j] = sum_i intt(r)_i g[i].
 *                                  r is drawn by Fiat-Shamir from the file -- seed = the first 32 bytes of BLAKE2b-512(personal
 *                                  "bzh2-params-file", bytes); r_j = draw j of bzh_rng_expand(seed, ..) reduced as bzh_random_field
 *                                  reduces it --, so the file's author cannot choose it and a wrong g_lagrange passes with
 *                                  probability about 2^-254.  One inverse NTT and two n-term MSMs against the two tables instead
 *                                  of a group FFT.
 *       BZH_PARAMS_CHECK_FULL      and g, w, u are Params::new(k)'s: g is made again by bzh_params_generators_device's kernels and
 *                                  compared limb for limb where it lies, w and u by two bzh_hash_to_curve calls on the host.  The
 *                                  only level that protects soundness against a g whose discrete logarithms somebody knows.
 *                         The 2 n + 2 strings go up in one copy and are decoded by bzh_affine_decompress's kernel; one kernel
 *                         (k_pf_verdict) folds the status bytes, the comparison with the regenerated points and the comparison of
 *                         the two sums into the 16-byte verdict, which is the one read-back the decision needs.  The host copies
 *                         of the points are queued behind the verdict kernel and come back in the same wait.  That wait is the only
 *                         one the call adds; bzh_bases_precompute's own waits, while it swaps a table for its window table, and a
 *                         workspace or pinned buffer that grows on first use stay as they are.
 *                         BZH_E_RANGE: the file is refused.  *out is NULL, everything the call allocated is freed, *verdict
 *                         (may be NULL) says why and bzh_last_error names the section and the index.  bits: BZH_PARAMS_BAD_DECODE
 *                         alone when a string is no point (nothing else is then decided) -- section / first_bad: the lowest such
 *                         string in file order, n_bad: how many; else BZH_PARAMS_BAD_LAGRANGE and / or BZH_PARAMS_BAD_GENERATORS --
 *                         with the latter section / first_bad / n_bad describe the points of g, w, u that are not Params::new's
 *                         (file order again); with BZH_PARAMS_BAD_LAGRANGE alone section is 1 and first_bad and n_bad are 0: the
 *                         check says that g_lagrange is wrong, not where.  An accepted file leaves the verdict all zero.
 *                         BZH_E_ARG, nothing done: a NULL ctx, bytes or out; an unknown check; window_bits < 0; whatever
 *                         bzh_params_file_info refuses; k = 0 (bzh_params_create takes 1 .. 24). */
typedef enum { BZH_PARAMS_CHECK_POINTS = 0, BZH_PARAMS_CHECK_LAGRANGE = 1, BZH_PARAMS_CHECK_FULL = 2 } bzh_params_check;
enum { BZH_PARAMS_BAD_DECODE = 1, BZH_PARAMS_BAD_LAGRANGE = 2, BZH_PARAMS_BAD_GENERATORS = 4 };
typedef struct {
    uint32_t bits;      /* BZH_PARAMS_BAD_* */
    uint32_t section;   /* of first_bad: 0 g, 1 g_lagrange, 2 w, 3 u */
    uint32_t first_bad; /* index inside the section */
    uint32_t n_bad;
} bzh_params_verdict;
int bzh_params_file_info(const uint8_t* bytes, size_t len, unsigned* k, size_t* n_points);
int bzh_params_encode(unsigned k, const uint64_t* g_xy, const uint64_t* g_lagrange_xy, const uint64_t* w_xy, const uint64_t* u_xy, uint8_t* out,
                      size_t cap, size_t* len);
int bzh_params_write(bzh_ctx* ctx, const bzh_params* p, uint8_t* out, size_t cap, size_t* len);
int bzh_params_read(bzh_ctx* ctx, const uint8_t* bytes, size_t len, int window_bits, int check, bzh_params** out, bzh_params_verdict* verdict);

/* ---- circuits: the reference's ShotCircuit / BoardCircuit as data + their witness synthesis -------------------------
 * The reference-side interface this replaces is `impl Circuit<pallas::Base> for {ShotCircuit, BoardCircuit}`
 * (src/circuits/shot.rs:22-53, src/circuits/board.rs:21-51): `configure` -> ShotChip::configure / BoardChip::configure
 * (src/chips/shot.rs:179-297, src/chips/board.rs:194-321) and `synthesize` -> ShotChip::synthesize / BoardChip::synthesize
 * (src/chips/shot.rs:308-354, src/chips/board.rs:331-363), with every chip under them (src/chips/{bitify,placement,
 * transpose,pedersen}.rs and halo2_gadgets' EccChip), laid out by SimpleFloorPlanner.  Host C++, no device needed
 * except for BZH_MEM_DEVICE output.
 *   bzh_circuit_create   configure + the keygen synthesis at 2^k rows (Shot: k >= 11, Board: k >= 12 -- the reference's
 *                        sizes, benches/shot.rs:22, benches/board.rs:22; BZH_E_RANGE if the circuit does not fit) +
 *                        selector compression.  `bits`: B of the two bitify test circuits (src/chips/bitify.rs:255-403),
 *                        ignored otherwise.
 *   bzh_circuit_blob     the serialised constraint system + fixed assignment for bzh_pk_create ("BZC2", csrc/prove.hip);
 *                        out = NULL only reports the length.
 *   bzh_circuit_describe JSON: column counts, gates (names, constraint names, queried cells), regions (name, rows,
 *                        columns), permutation columns, query lists -- what dev::MockProver reports failures against.
 *   bzh_synthesize_shot / bzh_synthesize_board
 *                        `batch` witnesses: fills advice = batch x num_advice x 2^k elements (`form`; BZH_MEM_HOST, or
 *                        BZH_MEM_DEVICE + BZH_FORM_MONTGOMERY: staged compactly through pinned memory and expanded on the
 *                        ctx's stream) -- exactly the tensor bzh_prove_batch consumes -- and instances = batch x
 *                        {4, 2} canonical public inputs (Shot: commitment x, y, shot, hit: src/circuits/shot.rs:125-130;
 *                        Board: commitment x, y: src/circuits/board.rs:113-118).  Inputs are the constructor arguments of
 *                        ShotCircuit::new / BoardCircuit::new: 256-bit BinaryValues as 4 limbs, trapdoors as canonical
 *                        Pallas scalars.  `threads` host threads (0 = auto).  BZH_E_RANGE: an input the reference would
 *                        panic on (H and V share a bit: src/utils/binary.rs:97-108; non-canonical trapdoor).
 *   bzh_board_witness    Board::from(&Deck::from(ships)).{witness, state}(options): ships = 5 x (x, y, z), x < 0 = None;
 *                        options = 5 WitnessOption values (src/utils/ship.rs:315-331) or NULL.  Anything but NULL / all
 *                        BZH_WITNESS_DEFAULT is the reference's TEST-ONLY fault injection (malicious ship commitments for its
 *                        negative MockProver tests): a negative-test aid, never a production input;
 *                        out: 10 ship commitments [H5, V5, H4, V4, H3a, V3a, H3b, V3b, H2, V2] and the board state.
 *   bzh_shot_serialize   shot::serialize (src/utils/shot.rs:12-19).
 *   bzh_pedersen_commit_host   pedersen_commit (src/utils/pedersen.rs:17-28) on the host, from the circuit's window tables.
 *   bzh_fixed_base_tables      Z / U / Lagrange tables of BoardCommitV (0) and BoardCommitR (1), derived from the generators
 *                        (src/utils/constants/fixed_bases/board_commit_{v,r}.rs). */
typedef struct bzh_circuit bzh_circuit;
typedef enum { BZH_CIRCUIT_SHOT = 0, BZH_CIRCUIT_BOARD = 1, BZH_CIRCUIT_NUM2BITS_TEST = 2, BZH_CIRCUIT_BITS2NUM_TEST = 3 } bzh_circuit_kind;
typedef enum {
    BZH_WITNESS_DEFAULT = 0,
    BZH_WITNESS_DUAL_PLACEMENT = 1,
    BZH_WITNESS_NONCONSECUTIVE = 2,
    BZH_WITNESS_EXTRA_BIT = 3,
    BZH_WITNESS_OVERSIZED = 4,
    BZH_WITNESS_UNDERSIZED = 5
} bzh_witness_option;
int bzh_circuit_create(int kind, unsigned k, unsigned bits, bzh_circuit** out);
int bzh_circuit_free(bzh_circuit* c);
const char* bzh_circuit_last_error(void);
int bzh_circuit_blob(const bzh_circuit* c, uint8_t* out, size_t cap, size_t* len);
int bzh_circuit_describe(const bzh_circuit* c, char* out, size_t cap, size_t* len);
int bzh_circuit_info(const bzh_circuit* c, uint32_t* num_advice, uint32_t* num_instance_rows, uint32_t* n_rows, uint32_t* rows_used,
                     uint32_t* num_gates, uint32_t* num_regions);
/* the verifying-key digest of the blob this circuit hands out (see "THE VERIFYING-KEY DIGEST" above): set it BEFORE
 * bzh_circuit_blob / bzh_pk_create; *is_placeholder = 1 until it has been set */
int bzh_circuit_set_vk_repr(bzh_circuit* c, const uint8_t* repr32);
int bzh_circuit_vk_repr(const bzh_circuit* c, uint8_t* out_repr32, int* is_placeholder);
int bzh_synthesize_shot(bzh_ctx* ctx, const bzh_circuit* c, size_t batch, const uint64_t* boards, const uint64_t* trapdoors, const uint64_t* shots,
                        const uint64_t* hits, uint64_t* advice, int form, int mem, uint64_t* instances, unsigned threads);
int bzh_synthesize_board(bzh_ctx* ctx, const bzh_circuit* c, size_t batch, const uint64_t* ship_commitments, const uint64_t* boards,
                         const uint64_t* trapdoors, uint64_t* advice, int form, int mem, uint64_t* instances, unsigned threads);
/* The same two calls with the place of the arithmetic chosen (`where`).  BZH_SYNTH_HOST is bzh_synthesize_shot / _board exactly.
 * BZH_SYNTH_DEVICE computes the witness on the ctx's device, straight into the advice tensor: it needs a ctx, BZH_MEM_DEVICE and
 * BZH_FORM_MONTGOMERY (BZH_E_ARG otherwise); the inputs stay host pointers and `instances` host memory (or NULL).  Same tensor,
 * same instances, same statuses: an input the host path refuses gives BZH_E_RANGE and bzh_circuit_last_error's text.  The call
 * returns after one read-back (status words and commitments), its only stream synchronisation; `threads` is ignored. */
#define BZH_SYNTH_HOST 0
#define BZH_SYNTH_DEVICE 1
int bzh_synthesize_shot_with(bzh_ctx* ctx, const bzh_circuit* c, size_t batch, const uint64_t* boards, const uint64_t* trapdoors, const uint64_t* shots,
                             const uint64_t* hits, uint64_t* advice, int form, int mem, uint64_t* instances, unsigned threads, int where);
int bzh_synthesize_board_with(bzh_ctx* ctx, const bzh_circuit* c, size_t batch, const uint64_t* ship_commitments, const uint64_t* boards,
                              const uint64_t* trapdoors, uint64_t* advice, int form, int mem, uint64_t* instances, unsigned threads, int where);
/* THE GAME-INPUT PROVER: the reference's top-level operation -- game inputs in, {commitment, proof} out (src/wasm/circuit_wasm.rs,
 * benches/{shot,board}.rs) -- for a batch, as ONE device-resident call: bzh_synthesize_*_with(BZH_SYNTH_DEVICE) and
 * bzh_prove_batch_device_seeded joined on the device.  The game inputs are host pointers with the layout of bzh_synthesize_shot /
 * bzh_synthesize_board; `seeds` is 32 bytes per proof, with the ChaCha20 expansion and the SECURITY note of
 * bzh_prove_batch_device_seeded; `instances` (host, may be NULL) receives batch x {4, 2} canonical rows, exactly what
 * bzh_synthesize_* writes; proofs, proof_stride, proof_lens and status are bzh_prove_batch_device's.
 * Proofs, lengths and instances are byte-identical to bzh_synthesize_*_with(BZH_SYNTH_DEVICE) followed by
 * bzh_prove_batch_device_seeded on the same inputs and seeds, and so to host synthesis followed by bzh_prove_batch_seeded.
 * status keeps bits 0 .. 3 of bzh_prove_batch_device and adds the synthesis status at bits 4 .. 6: bit 4 "incomplete addition:
 * exceptional case", bit 5 "fixed-base mul: window point with x = 0", bit 6 "pedersen_commit: message repr is not a canonical
 * scalar" -- the inputs bzh_synthesize_* refuses after running.  A proof flagged by the synthesis still gets all its bytes and
 * disturbs no other proof.  With status == NULL any flagged proof makes the call return BZH_E_RANGE and write nothing;
 * bzh_last_error names the first flagged proof and its bits, and for a synthesis bit ends with the text bzh_synthesize_* gives.
 * Inside: the inputs are checked and packed on the host and go up once (128 bytes a Shot proof, 384 a Board proof, plus the seed);
 * the advice tensor lives in the key's workspace and is filled by the three synthesis kernels; one lane per proof makes the
 * instance rows from the commitment where the synthesis left it (k_pg_instances) and folds the synthesis status (k_pg_status);
 * nothing of size n is uploaded, and neither the status words nor the commitment come to the host between the two halves.  The
 * call makes the one stream wait of bzh_prove_batch_device, for one read-back of the proofs, the status and length slots and the
 * canonical instances (and the one-time wait of the call that merges the workspace's blocks).
 * Refused before anything is launched, with the key and the ctx usable:
 * BZH_E_ARG: a NULL ctx, pk, circuit, input array, seeds, proofs or proof_lens; batch == 0 or above 65536; a circuit of the other
 * kind; a key on another device than ctx; a circuit that does not match the key -- compared are the curve (Vesta), n, the number of
 * advice columns, the number of instance columns (one) and that the circuit's instance rows fit the key's usable rows.
 * BZH_E_RANGE: a batch above bzh_prove_device_plan's limit; what bzh_prove_batch_device answers with BZH_E_RANGE (no VM v2
 * quotient program, a proof_stride below the proof bytes); the inputs bzh_synthesize_* refuses on sight, with its text in
 * bzh_last_error and bzh_circuit_last_error (a non-canonical trapdoor; H and V commitments sharing a bit). */
int bzh_prove_shots_device(bzh_ctx* ctx, bzh_pk* pk, const bzh_circuit* circuit, size_t batch, const uint64_t* boards, const uint64_t* trapdoors,
                           const uint64_t* shots, const uint64_t* hits, const uint8_t* seeds, uint64_t* instances, uint8_t* proofs,
                           size_t proof_stride, size_t* proof_lens, uint8_t* status);
int bzh_prove_boards_device(bzh_ctx* ctx, bzh_pk* pk, const bzh_circuit* circuit, size_t batch, const uint64_t* ship_commitments,
                            const uint64_t* boards, const uint64_t* trapdoors, const uint8_t* seeds, uint64_t* instances, uint8_t* proofs,
                            size_t proof_stride, size_t* proof_lens, uint8_t* status);
int bzh_synthesize_bitify_test(const bzh_circuit* c, const uint64_t* value, const uint64_t* binary, uint64_t* advice);
int bzh_board_witness(const int8_t* ships, const int32_t* options, uint64_t* ship_commitments, uint64_t* state);
int bzh_shot_serialize(const uint8_t* xs, const uint8_t* ys, size_t count, uint64_t* out);
int bzh_pedersen_commit_host(const uint64_t* message, const uint64_t* trapdoor, uint64_t* out_xy);
/* The same commitment for n (message, trapdoor) pairs in ONE launch on the device (the reference calls
 * pedersen_commit once per proof from every frontend and a second time inside ShotChip::synthesize, src/chips/shot.rs:319,
 * re-hashing V and R each time).  messages / trapdoors: n x 4 canonical limbs (host) -- the message is an Fp value re-read as a
 * Pallas scalar through its repr, as pedersen.rs:23-24 does; out_xy: n affine canonical points x || y, (0, 0) = identity.
 * V and R live in a ctx-owned direct-lookup table (d * 2^(8w) * G for 32 signed 8-bit windows, 512 KB, built on the first
 * call): 64 mixed additions + one inversion per commitment, one lane each.  BZH_E_RANGE: a repr that is not a canonical
 * Pallas scalar (from_repr(..).unwrap() panics upstream).  Returns when out_xy is filled. */
int bzh_pedersen_commit_batch(bzh_ctx* ctx, const uint64_t* messages, const uint64_t* trapdoors, size_t n, uint64_t* out_xy);
int bzh_fixed_base_tables(int base, uint64_t* z, uint64_t* u, uint64_t* lagrange);

/* ---- host helpers (CPU, no device needed): what `.to_affine()` / `to_bytes()`
 * do on the Rust side; used by tests and benches to compare canonical bytes. */
int bzh_jacobian_to_affine(int curve, const uint64_t* xyz, size_t n, int form, uint64_t* out_xy);
/* sum of n Jacobian points (host): the combine step of one MSM whose points are split over several GPUs -- every rank
 * holds N/R points, returns one 96-byte partial, the partials are all-gathered and added locally. */
int bzh_jacobian_sum(int curve, const uint64_t* xyz, size_t n, int form, uint64_t* out_xyz);
/* pasta_curves to_bytes: x little-endian, bit 255 = parity of canonical y, identity = 32 zero bytes.
 * xy in `form`; out: n * 32 bytes. */
int bzh_affine_compress(int curve, const uint64_t* xy, size_t n, int form, uint8_t* out32);
/* pasta_curves from_bytes for n points (Blake2bRead::read_point; one lane per point on the device, csrc/sqrt_decompress.hip):
 * in32 = n x 32 bytes, out_xy = n affine points x || y in `form`, (0,0) = identity.
 * status (may be NULL): BZH_POINT_OK = 0, BZH_POINT_IDENTITY = 1, BZH_POINT_INVALID = 2 (x >= p, not on the curve, sign
 * bit on the identity; out = zeros).  Same return convention as bzh_batch_sqrt.  `mem` applies to in32, out_xy, status;
 * ctx == NULL with BZH_MEM_HOST runs on the host. */
typedef enum { BZH_POINT_OK = 0, BZH_POINT_IDENTITY = 1, BZH_POINT_INVALID = 2 } bzh_point_status;
int bzh_affine_decompress(bzh_ctx* ctx, int curve, const uint8_t* in32, size_t n, int form, int mem, uint64_t* out_xy, uint8_t* status);
/* ---- Curve::batch_normalize / to_affine and GroupEncoding::to_bytes on the device (csrc/normalize_compress.hip): the
 * outbound twin of bzh_affine_decompress, for the Jacobian points bzh_msm leaves in HBM -------------------------------
 * The conventions are bzh_affine_decompress's: `mem` applies to every buffer of the call; device buffers are 16-byte
 * aligned; ctx == NULL with BZH_MEM_HOST runs the same chain code on the host; with BZH_MEM_DEVICE and a status buffer the
 * call only enqueues on the ctx's stream, otherwise it returns when the statuses are known.  n == 0 returns BZH_OK.
 *   bzh_batch_normalize        n Jacobian points (X || Y || Z, 12 limbs, `form`) -> out_xy (n x 8 limbs, `form`) and / or
 *                              out32 (n x 32 bytes, the to_bytes encoding bzh_affine_compress writes); either may be NULL, not
 *                              both.  One launch: Montgomery's trick over the chain a lane owns (bzh_batch_normalize_plan),
 *                              one inversion per lane.  status (may be NULL): one bzh_point_status byte per point.  Z = 0 is
 *                              an ordinary value: (0, 0), 32 zero bytes, BZH_POINT_IDENTITY -- never an error.  A canonical
 *                              coordinate that is not below p: host operands are checked first (BZH_E_RANGE, nothing is
 *                              written); a lane of device operands gets BZH_POINT_INVALID and zeros (BZH_E_RANGE when
 *                              status == NULL) and leaves its neighbours alone.  Montgomery operands are taken as given
 *                              (reduced), and points are not checked to be on the curve, as upstream.  The outputs must not
 *                              overlap xyz (they hold the chain's running products while the launch runs).
 *                              BZH_E_ARG: unknown curve, form or mem, both outputs NULL, xyz NULL with n > 0, n > 2^28,
 *                              BZH_MEM_DEVICE without a ctx or with a misaligned buffer.
 *   bzh_affine_compress_batch  to_bytes for n affine points already in `form`, wherever they live: the bytes
 *                              bzh_affine_compress gives.  With BZH_MEM_DEVICE the call only enqueues.
 *   bzh_batch_normalize_plan   host only: the launch shape bzh_batch_normalize uses for n points -- lane t of `lanes` owns the
 *                              points t, t + lanes, ... (at most `chain` of them). */
int bzh_batch_normalize(bzh_ctx* ctx, int curve, const uint64_t* xyz, size_t n, int form, int mem, uint64_t* out_xy, uint8_t* out32,
                        uint8_t* status);
int bzh_affine_compress_batch(bzh_ctx* ctx, int curve, const uint64_t* xy, size_t n, int form, int mem, uint8_t* out32);
int bzh_batch_normalize_plan(size_t n, size_t* lanes, size_t* chain);
/* ---- Batched Fiat-Shamir transcripts on the device (csrc/transcript_batch.hip): `batch` transcripts of
 * transcript::{Blake2bWrite, Challenge255} in lockstep, resident in HBM -- the step the points of bzh_msm are normalised for.
 * They absorb from device memory and squeeze into device memory, one launch per step for the whole batch:
 *     bzh_msm (BZH_MEM_DEVICE output)  ->  bzh_transcript_batch_write_jacobian  ->  bzh_transcript_batch_squeeze
 * with no read-back in between, and on through the opening argument: bzh_ipa_open_batch_device runs its rounds against such a
 * batch.  Not used by bzh_prove_batch or bzh_ipa_open(_batch), which keep their host transcripts; the verifier's opt-in device
 * pass drives a batch of its own.
 * Conventions: those of bzh_batch_normalize.  `mem` applies to every data pointer of a call; device buffers are 16-byte aligned;
 * with BZH_MEM_DEVICE a call only enqueues on the ctx's stream; count == 0 returns BZH_OK.  `curve` (Vesta, Pallas, BN254 G1)
 * fixes both fields: coordinates are in the base field, scalars and challenges in the scalar field.  Every call gives every
 * transcript the same number of items: transcript b reads the items b * stride + i, i < count, stride >= count (in items).
 *   _new             ctx == NULL makes a host-resident batch: it takes BZH_MEM_HOST only and runs the same step code on the host.
 *                    proof_cap: the most proof bytes one transcript may hold.  Free the batch before its ctx.
 *   _common_points   absorb affine points x || y (8 limbs, `form`) as 0x01 || x || y;  _write_points also appends to_bytes
 *   _write_jacobian  the same for Jacobian points X || Y || Z (12 limbs): bzh_batch_normalize's launch into the batch's own
 *                    scratch, then _write_points.  Device operands are normalised as the whole span they lie in, gaps included.
 *   _common_scalars  absorb scalars (4 limbs, `form`) as 0x02 || repr;  _write_scalars also appends the repr
 *   _squeeze         absorb 0x00; out: batch x 4 limbs, the digest of a copy of the state as a 512-bit integer mod the scalar field
 *   _proofs          *len (may be NULL) = the proof bytes per transcript; out (may be NULL): batch rows of out_stride >= *len bytes
 *   _status          host, batch bytes, waits for the stream: per transcript the largest bzh_point_status seen (sticky) --
 *                    BZH_POINT_IDENTITY: a point (0, 0) was absorbed (hashed as 64 zero bytes, as bzh_transcript_common_point
 *                    does; upstream refuses it); BZH_POINT_INVALID: a canonical device operand was not below its modulus
 *                    (hashed as zeros).  Host operands not below the modulus are checked first: BZH_E_RANGE, nothing absorbed.
 *   _from_host       load the state and proof bytes of `batch` bzh_transcript objects (statuses restart at BZH_POINT_OK);
 *                    BZH_E_ARG if their absorbed or proof lengths differ from each other, their challenge field is not the
 *                    curve's scalar field, or a proof is longer than proof_cap.   _to_host  overwrites the objects' state and
 *                    proof bytes: together they let a caller cross between the two kinds in the middle of a proof.
 * BZH_E_RANGE: a write past proof_cap (nothing is absorbed).  BZH_E_ARG: a NULL batch or pointer, unknown curve, form or mem,
 * stride < count, batch == 0, BZH_MEM_DEVICE on a host-resident batch or with a misaligned buffer.  Every argument error
 * leaves the batch as it was. */
typedef struct bzh_transcript_batch bzh_transcript_batch;
int bzh_transcript_batch_new(bzh_ctx* ctx, int curve, size_t batch, size_t proof_cap, bzh_transcript_batch** out);
int bzh_transcript_batch_free(bzh_transcript_batch* tb);
int bzh_transcript_batch_common_points(bzh_transcript_batch* tb, const uint64_t* xy, size_t count, size_t stride, int form, int mem);
int bzh_transcript_batch_write_points(bzh_transcript_batch* tb, const uint64_t* xy, size_t count, size_t stride, int form, int mem);
int bzh_transcript_batch_write_jacobian(bzh_transcript_batch* tb, const uint64_t* xyz, size_t count, size_t stride, int form, int mem);
int bzh_transcript_batch_common_scalars(bzh_transcript_batch* tb, const uint64_t* s, size_t count, size_t stride, int form, int mem);
int bzh_transcript_batch_write_scalars(bzh_transcript_batch* tb, const uint64_t* s, size_t count, size_t stride, int form, int mem);
int bzh_transcript_batch_squeeze(bzh_transcript_batch* tb, int form, int mem, uint64_t* out);
int bzh_transcript_batch_proofs(bzh_transcript_batch* tb, int mem, uint8_t* out, size_t out_stride, size_t* len);
int bzh_transcript_batch_status(bzh_transcript_batch* tb, uint8_t* out);
int bzh_transcript_batch_from_host(bzh_transcript_batch* tb, const bzh_transcript* const* hosts);
int bzh_transcript_batch_to_host(bzh_transcript_batch* tb, bzh_transcript* const* hosts);
/* host only, no ctx: the launch shapes of bzh_batch_invert and bzh_kate_division(_batch), from the functions the drivers call.
 *   bzh_batch_invert_plan    thread t of *nthreads owns the chain of elements t, t + nthreads, ... below count (Montgomery's
 *                            trick over it, one inversion per thread); count == 0 gives 0: nothing is launched.
 *   bzh_kate_division_plan   every polynomial of n coefficients is cut into *S spans, one workgroup of *threads threads each,
 *                            thread t of a span walking *L consecutive quotient coefficients (the last span and its last
 *                            threads may have fewer, or none).  BZH_E_ARG for what is not launched or refused: n < 2,
 *                            batch == 0, batch > 65535.
 * BZH_E_ARG on a NULL output. */
int bzh_batch_invert_plan(size_t count, size_t* nthreads);
int bzh_kate_division_plan(size_t n, size_t batch, unsigned* threads, size_t* L, size_t* S);
/* root of unity of order 2^log_n used by halo2's EvaluationDomain for this field
 * (ROOT_OF_UNITY^(2^(S-log_n))); out: 4 limbs in `form`. */
int bzh_field_omega(int field, unsigned log_n, int form, uint64_t* out);

/* ---- proof / IO record (host) ---------------------------------------------
 * The record the reference's wasm frontend hands to JavaScript, src/wasm/circuit_wasm.rs:27-31:
 *     struct BattleZipsWASM { commitment: Vec<[u8; 32]>, proof: Vec<u8> }
 * commitment = the public inputs (Board: commit.x, commit.y; Shot: commit.x, commit.y, shot, hit) as
 * BinaryValue::from_fp(fp).to_repr() (:75-83, :164-167), proof = Blake2bWrite::finalize().  Two forms:
 *   - the serde JSON text {"commitment":[[32 numbers],...],"proof":[numbers]} (bzh_record_to_json / _from_json), and
 *   - a fixed-stride binary record: what the multi-GPU gather carries (equal-sized records, one all_gather) and what
 *     a batch client stores per proof:
 *         u32 proof_len | u8 n_inputs | u8 kind | u16 0 | u32 index | u32 0 | u8 inputs[4][32] | u8 proof[proof_stride]
 *     `kind` / `index` are the caller's tags (e.g. 0 = Board, 1 = Shot; position in the batch); they are not part of the
 *     JSON form.
 * Reading back (verify_board / verify_shot, :86-116) goes through BinaryValue::from_repr(bin).to_fp(): a public input
 * that is not a canonical Fp element is refused -- BZH_E_RANGE here, from encode, decode and from_json alike.
 * Malformed JSON is BZH_E_ARG; a proof longer than the record's stride, more than 4 inputs, or a corrupt header is
 * BZH_E_RANGE. */
#define BZH_RECORD_HEADER_BYTES 144
#define BZH_RECORD_MAX_INPUTS 4
/* bytes per record for proofs of up to proof_stride bytes (bzh_pk_info's max_proof_bytes) */
size_t bzh_record_stride(size_t proof_stride);
/* public_inputs: n_inputs x 4 canonical limbs */
int bzh_record_encode(const uint64_t* public_inputs, size_t n_inputs, const uint8_t* proof, size_t proof_len, uint32_t kind, uint32_t index,
                      uint8_t* record, size_t record_stride);
/* any out pointer may be NULL; *proof points into `record` */
int bzh_record_decode(const uint8_t* record, size_t record_stride, uint64_t* public_inputs, size_t* n_inputs, const uint8_t** proof,
                      size_t* proof_len, uint32_t* kind, uint32_t* index);
/* out == NULL: size query (*len = strlen of the text); otherwise cap must hold *len + 1 */
int bzh_record_to_json(const uint8_t* record, size_t record_stride, char* out, size_t cap, size_t* len);
int bzh_record_from_json(const char* text, size_t text_len, uint32_t kind, uint32_t index, uint8_t* record, size_t record_stride);

/* ---- verify_board / verify_shot over a batch of records, device-resident (src/wasm/circuit_wasm.rs:86-116, 180-194) -------------
 * bzh_verify_records_device reads `batch` binary records (host memory, the fixed-stride layout above, record_stride bytes apart)
 * and decides accept or reject for each: what bzh_record_decode followed by bzh_verify_batch_vk decides, as ONE call in which
 * nothing crosses the bus between the upload of the record bytes and the read-back of one result and one status byte per record.
 * On the ctx's stream: a kernel checks every header and every public input against the modulus (limb by limb, as
 * BinaryValue::from_repr(..).to_fp()) and unpacks inputs and proofs; the instance commitments are Params::commit_lagrange with
 * blind 1 -- a prefix MSM over the first n_inputs points of g_lagrange, plus W, normalised by bzh_batch_normalize's launch --;
 * the per-proof pass is BZH_VERIFY_PASS_DEVICE's; the two sums of every opening check are compared on the device.  The stream is
 * waited for once, by the read-back (the MSMs' own waits aside, and a workspace that grows on a key's first call).
 *   n_inputs   what every record must carry: 4 for Shot, 2 for Board
 *   g0_u_w     G_0, U, W of srs as 3 affine canonical points, compared with the table on the device (BZH_E_ARG after the call's
 *              one wait if they differ, results[] and status[] untouched), or NULL: no comparison, the table's points are used
 *   results[b] 1 accept, 0 reject: exactly bzh_verify_batch_vk's on the decoded record
 *   status[b]  (status may be NULL) bit 0: the record was refused before verification -- a non-zero reserved header field, an
 *              n_inputs field other than the argument, a proof length other than the key's, or a public input that is not a
 *              canonical Fp element; bits 1 .. 7 zero.  A refused record is results[b] = 0, never an error, and leaves its
 *              neighbours alone.  `kind` and `index` are the caller's tags and are not read.
 * The largest batch a call takes is 4096, bzh_verify_batch's own limit: the pass's launches (one row of a grid per proof, 65535
 * rows) are exercised up to it.  Nothing selects this call: every other entry point keeps its path and its defaults.  Its speed
 * has not been measured (tools/ubench_verify_records.py prints the comparison).
 * BZH_E_ARG: a NULL ctx, vk, srs, g_lagrange, records or results; n_inputs == 0 or > BZH_RECORD_MAX_INPUTS; batch > 4096; a vk
 * whose constraint system does not have exactly one instance column; record_stride < BZH_RECORD_HEADER_BYTES + the key's proof
 * length; tables of another device, curve or size.  batch == 0: BZH_OK, nothing is touched.  BZH_E_RANGE: a key whose shape has
 * no device program, as bzh_verify_batch_vk_with under BZH_VERIFY_PASS_DEVICE. */
int bzh_verify_records_device(bzh_ctx* ctx, const bzh_vk* vk, const bzh_bases* srs, const bzh_bases* g_lagrange, size_t batch, size_t n_inputs,
                              const uint8_t* records, size_t record_stride, const uint64_t* g0_u_w, int* results, uint8_t* status);

/* ---- a batch verified with ONE accumulated opening check ------------------------------------------------------------------------
 * All B opening checks of a batch are linear equations in group elements, so a random linear combination of them is one equation:
 *     sum_b w_b * ( sum_i lc_scal[b][i] * lc_pts[b][i] )  ==  < sum_b w_b * c_b * s(u_b) , G >
 * The right side is ONE n-term MSM against the SRS on a vector a field kernel accumulates ((n + 2) * 32 bytes instead of
 * B * (n + 2) * 32), the left side ONE Pippenger MSM over the B * nl points of the batch.  The weights are
 * bzh_accumulation_weights(curve, seed, B, ..): read its SECURITY paragraph -- `seed` is 32 bytes of a cryptographically secure
 * generator, fresh per call, drawn after the records are fixed.
 * bzh_verify_records_accumulated takes what bzh_verify_records_device takes, bzh_verify_batch_vk_accumulated what
 * bzh_verify_batch_vk_with(.., BZH_VERIFY_PASS_DEVICE, ..) takes, and `seed`; everything up to the opening check is that call's,
 * launch for launch.  Then:
 *   - a record refused before verification, or a proof the pass rejects (a point off the curve, a non-canonical scalar, ..), is
 *     EXCLUDED: weight 0 on both sides.  It is results[b] = 0 and does not make the batch fail.
 *   - the accumulated check runs and its one byte comes back with the reject bytes: the call's one wait.  Accepted: results[b] = 1
 *     for every included record, *path = 0.
 *   - not accepted: the per-proof ending of bzh_verify_records_device (bzh_verify_batch_vk_with) runs on the same device operands
 *     and says exactly which record fails; *path = 1.  A failing batch therefore costs BOTH checks.
 *   - a batch in which every record is refused on the host's reading (header, inputs, proof length) launches no MSM; *path = 0.
 * results[] and status[] equal bzh_verify_records_device's (results[] bzh_verify_batch_vk_with's) on the same input, for every
 * seed -- up to the 1/|F| above.  path may be NULL.  Argument refusals, the 4096 limit, batch == 0 and BZH_E_RANGE are that
 * call's; in addition a NULL seed is BZH_E_ARG.  Nothing selects these calls.  Measured: DESIGN.md section 7,
 * tools/ubench_verify_accumulated.py. */
int bzh_verify_records_accumulated(bzh_ctx* ctx, const bzh_vk* vk, const bzh_bases* srs, const bzh_bases* g_lagrange, size_t batch,
                                   size_t n_inputs, const uint8_t* records, size_t record_stride, const uint64_t* g0_u_w, const uint8_t seed[32],
                                   int* results, uint8_t* status, int* path);
int bzh_verify_batch_vk_accumulated(bzh_ctx* ctx, const bzh_vk* vk, const bzh_bases* srs, const bzh_bases* g_lagrange, size_t batch,
                                    const uint64_t* instances, size_t instance_rows, const uint8_t* proofs, size_t proof_stride,
                                    const size_t* proof_lens, const uint64_t* g0_u_w, const uint8_t seed[32], int* results, int* path);
/* the accumulated check alone, operands in host memory: lc_pts batch x nl affine canonical points ((0,0) = padding, never added),
 * lc_scal batch x nl, cu batch x (k + 1) (c, u_0 .. u_(k-1)) and weights batch x 4 limbs, all canonical; exclude: batch bytes or
 * NULL, a non-zero byte gives the opening weight 0; bases: the n + 2 points (g | u | w).  *ok = 1 when
 * sum_b w'_b (sum_i lc_scal[b][i] lc_pts[b][i]) = < sum_b w'_b c_b s(u_b), g >.  BZH_E_ARG: a NULL pointer but exclude, batch == 0
 * or > 4096, nl == 0 or > 65536, n not a power of two, a table of another device. */
int bzh_ipa_check_accumulated(bzh_ctx* ctx, const bzh_bases* bases, size_t batch, size_t nl, const uint64_t* lc_pts, const uint64_t* lc_scal,
                              const uint64_t* cu, const uint64_t* weights, const uint8_t* exclude, int* ok);

#ifdef __cplusplus
}
#endif
#endif /* BZH2_H */
