// The evaluation phase on device-resident transcripts (bzh_evaluations_batch_device) on gfx950.
//
// Replaces the step of halo2_proofs 0.2.0 `plonk::create_proof` (UPSTREAM, un-vendored) between the quotient commitments and the
// multiopen argument -- squeeze x, write every queried polynomial's value at x * omega^rotation, build h(X) = sum_i x^(n i) h_i(X) --
// for a caller whose Fiat-Shamir transcripts are a bzh_transcript_batch in HBM: x is squeezed into device memory and read from
// there by every launch that needs it, so nothing goes to the host between the first launch and the last.  bzh_prove_batch's
// evaluations() and h_poly() phases (csrc/prover.hpp) do the same arithmetic around host transcripts: x comes down, the points are
// computed on the host, every (polynomial, rotation) job is copied into a gathered buffer and evaluated on its own, the values
// come down and go into host transcripts, and h(X) runs on the expression VM from a constant table made of the host's x^n.  Here:
//   k_ev_scalars     one lane per proof, bodies in evaluations_scalars.hpp: the points x * omega^rotation (omega^rotation depends
//                    on (field, k, rotation) alone and is uploaded before the first launch), x^n by k squarings, h_blind.
//   k_ev_multipoint  the hot kernel: one workgroup per (queried polynomial, proof) evaluates the polynomial at R of its distinct
//                    rotations in ONE pass over its coefficients -- each coefficient is loaded once and feeds R strided-Horner
//                    accumulators, each with its own x^tid and x^T as block_eval_poly (polyops.hip) has them for one point -- and
//                    writes the values into the [proof][query] slots the transcript absorbs from; a repeated query copies.  R is
//                    a template parameter, 1 .. kEvPass; a polynomial at more rotations than kEvPass takes a second pass.  There
//                    is no gathered copy: the sources are read in place through a table of (pointer, per-proof stride).
//   k_ev_export      the values from those slots to the caller's array, in its form.
//   k_mo_combine (multiopen.hip, through mo_combine) builds h(X): the pieces from the top one down, the challenge pointer at x^n.
//   tb_squeeze_locked / tb_absorb_locked do the transcript steps: one squeeze, one absorb launch for the whole run of queries.
#include <algorithm>
#include <cstring>
#include <utility>
#include <vector>

#include "block.cuh"
#include "ctx.hpp"
#include "curve.cuh"
#include "evaluations_scalars.hpp"
#include "host_field.hpp"

static_assert(bzh::kEvMaxRotations == BZH_EVAL_MAX_ROTATIONS, "lane bodies and header disagree");

namespace bzh {

// Points one pass of k_ev_multipoint carries.  hipcc's kernel-resource-usage remarks for gfx950 (Fp and Fq alike), VGPRs and
// waves per SIMD, no scratch in any of them:
//   R = 1: 72, 7   R = 2: 102, 4   R = 3: 164, 3   R = 4: 194, 2   R = 5: 232, 2   (R = 6 and 8: 256 and accumulation registers, 1)
// A workgroup is four waves, one per SIMD, so waves per SIMD is workgroups per CU.  The loop is a chain of 256-bit modular
// multiplications per accumulator with one 32-byte load per R of them: it needs independent chains, which R gives it, far more
// than it needs waves to hide the load.  Five points sit on the same occupancy step as four (two workgroups per CU, up to 256
// registers); six leave one workgroup per CU.  The Board circuit queries one polynomial at 5 rotations and no other at more
// than 3 (tools/ubench_evaluations.py --plan-only), so with 5 none of its polynomials takes a second pass.  (DESIGN.md section
// 4 keeps the table.)
static constexpr int kEvPass = 5;
static constexpr unsigned kEvLanes = 64;

// one workgroup's work on every proof: a polynomial and R of its rotations
struct EvJob {
    MoSrc src;
    uint32_t pt[kEvPass];      // the rotations' indices into a proof's row of the points
    uint32_t qfirst, qcount;   // its entries of the slot table: (point of this pass, query) pairs
};

// f(integral_constant<int, 0>) .. f(integral_constant<int, R - 1>)
template <int... J, class F>
__device__ __forceinline__ void ev_each(std::integer_sequence<int, J...>, F&& f) {
    (f(std::integral_constant<int, J>{}), ...);
}

// evals[b][q] = src_b(points[b][pt]) for every slot (pt, q) of job blockIdx.x; proof b = blockIdx.y.  points: batch x nrot in the
// caller's form, evals: batch x nqueries Montgomery.  n >= 1 coefficients.
template <class P, int R>
__global__ void __launch_bounds__(kVecThreads) k_ev_multipoint(const EvJob* __restrict__ jobs, const uint32_t* __restrict__ slots,
                                                               const uint32_t* __restrict__ points, size_t nrot, int canonical, size_t n,
                                                               size_t nqueries, uint32_t* __restrict__ evals) {
    constexpr int T = kVecThreads;
    __shared__ __align__(16) uint4 sh[2 * T];
    __shared__ uint32_t res[R * 8];
    const int tid = threadIdx.x;
    const size_t b = blockIdx.y;
    const EvJob job = jobs[blockIdx.x];
    const uint32_t* __restrict__ c = job.src.p + b * job.src.stride * 8;
    // per point: x^tid for this thread (binary method over the 8 bits of tid) and y = x^T.  The points are numbered at compile
    // time (ev_each), so that xt, y and acc are registers and not an indexed array in scratch.
    Fe<P> xt[R], y[R], acc[R];
    constexpr std::make_integer_sequence<int, R> each{};
    ev_each(each, [&](auto jc) {
        constexpr int j = decltype(jc)::value;
        Fe<P> pw = fe_load<P>(points + (b * nrot + job.pt[j]) * 8);
        if (canonical) pw = fe_to_mont(pw);
        xt[j] = fe_one<P>();
#pragma unroll
        for (int bit = 0; bit < 8; bit++) {
            if ((tid >> bit) & 1) xt[j] = fe_mul(xt[j], pw);
            pw = fe_sqr(pw);
        }
        y[j] = pw;
        acc[j] = fe_zero<P>();
    });
    if ((size_t)tid < n) {
        const size_t last = tid + ((n - 1 - tid) / T) * T;
        for (size_t i = last;; i -= T) {
            const Fe<P> cf = fe_load<P>(c + i * 8);   // loaded once, used R times
            ev_each(each, [&](auto jc) {
                constexpr int j = decltype(jc)::value;
                acc[j] = fe_add(fe_mul(acc[j], y[j]), cf);
            });
            if (i < (size_t)T) break;
        }
        ev_each(each, [&](auto jc) {
            constexpr int j = decltype(jc)::value;
            acc[j] = fe_mul(acc[j], xt[j]);
        });
    }
    ev_each(each, [&](auto jc) {
        constexpr int j = decltype(jc)::value;
        const Fe<P> s = block_sum(acc[j], sh, T);
        if (tid == 0) fe_store(res + j * 8, s);
    });
    __syncthreads();
    for (uint32_t e = tid; e < job.qcount; e += T) {
        const uint32_t pt = slots[2 * (job.qfirst + e)], q = slots[2 * (job.qfirst + e) + 1];
        uint32_t* out = evals + (b * nqueries + q) * 8;
#pragma unroll
        for (int w = 0; w < 8; w++) out[w] = res[pt * 8 + w];
    }
}

template <class P>
__global__ void __launch_bounds__(kEvLanes) k_ev_scalars(const uint32_t* __restrict__ xs, const uint32_t* __restrict__ omegas, size_t nrot, unsigned k,
                                                         const uint32_t* __restrict__ h_blinds, size_t npieces, size_t batch, int canonical,
                                                         uint32_t* __restrict__ out_points, uint32_t* __restrict__ xn,
                                                         uint32_t* __restrict__ out_h_blind) {
    const size_t b = blockIdx.x * (size_t)kEvLanes + threadIdx.x;
    if (b >= batch) return;
    ev_points_lane<P>(b, xs, omegas, nrot, canonical != 0, out_points);
    if (!npieces) return;
    ev_xn_lane<P>(b, xs, k, xn);
    ev_hblind_lane<P>(b, xn, h_blinds, npieces, canonical != 0, out_h_blind);
}
template <class P>
__global__ void __launch_bounds__(kEvLanes) k_ev_export(const uint32_t* __restrict__ evals, size_t count, int canonical, uint32_t* __restrict__ out) {
    const size_t g = blockIdx.x * (size_t)kEvLanes + threadIdx.x;
    if (g >= count) return;
    ev_export_lane<P>(g, evals, canonical != 0, out);
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
namespace {
// the passes and their slots, from the plan alone: jobs sorted by the number of their points, count[r] of them with r + 1
struct EvPasses {
    std::vector<EvJob> jobs;           // (their sources are filled in by evaluations_t, which knows the addresses)
    std::vector<uint32_t> poly, slots;   // poly[a]: the polynomial of jobs[a]
    size_t count[kEvPass] = {};
    explicit EvPasses(const EvPlan& p) {
        const size_t npolys = p.npolys_own + p.npolys_shared;
        // every queried polynomial's distinct points in first-seen order, and the queries that read it
        std::vector<std::vector<uint32_t>> pts(npolys), qs(npolys);
        for (size_t q = 0; q < p.nqueries; q++) {
            std::vector<uint32_t>& v = pts[p.poly_of_query[q]];
            if (std::find(v.begin(), v.end(), p.point_of_query[q]) == v.end()) v.push_back(p.point_of_query[q]);
            qs[p.poly_of_query[q]].push_back((uint32_t)q);
        }
        std::vector<EvJob> all;
        std::vector<uint32_t> poly_of;
        std::vector<int> size_of;
        std::vector<std::vector<uint32_t>> slots_of;
        for (uint32_t id : p.poly_order) {
            if (id == 0xffffffffu) break;
            for (size_t at = 0; at < pts[id].size(); at += kEvPass) {
                const size_t r = std::min<size_t>(kEvPass, pts[id].size() - at);
                EvJob j{};
                std::vector<uint32_t> sl;
                for (size_t i = 0; i < r; i++) {
                    j.pt[i] = pts[id][at + i];
                    for (uint32_t q : qs[id])
                        if (p.point_of_query[q] == j.pt[i]) sl.push_back((uint32_t)i), sl.push_back(q);
                }
                all.push_back(j), poly_of.push_back(id), size_of.push_back((int)r), slots_of.push_back(std::move(sl));
            }
        }
        for (int r = 1; r <= kEvPass; r++)
            for (size_t a = 0; a < all.size(); a++) {
                if (size_of[a] != r) continue;
                EvJob j = all[a];
                j.qfirst = (uint32_t)(slots.size() / 2), j.qcount = (uint32_t)(slots_of[a].size() / 2);
                slots.insert(slots.end(), slots_of[a].begin(), slots_of[a].end());
                jobs.push_back(j), poly.push_back(poly_of[a]), count[r - 1]++;
            }
    }
};
// scratch layout, in 32-bit words; every piece starts 64-byte aligned
struct EvScratch {
    size_t words = 0;
    size_t take(size_t w) {
        const size_t at = words;
        words += (w + 15) & ~(size_t)15;
        return at;
    }
    size_t x, xn, evals, omegas, jobs, slots, hsrcs, hfirst;
    EvScratch(const EvPlan& p, size_t njobs, size_t B, size_t npieces) {
        x = take(B * 8), xn = take(B * 8);
        evals = take(B * p.nqueries * 8);
        omegas = take(p.nrot * 8);
        jobs = take(njobs * (sizeof(EvJob) / 4)), slots = take(2 * p.nqueries);
        hsrcs = take(npieces * (sizeof(MoSrc) / 4)), hfirst = take(2);
    }
};
}  // namespace

size_t evaluations_scratch_bytes(const EvPlan& plan, size_t batch, size_t npieces) {
    // a polynomial has at most kEvMaxRotations distinct rotations: at most two passes
    const size_t njobs = 2 * std::min(plan.nqueries, plan.npolys_own + plan.npolys_shared);
    return EvScratch(plan, njobs, batch, npieces).words * 4 + 64;
}

template <class C>
static int evaluations_t(bzh_ctx* ctx, size_t B, unsigned k, const EvPlan& plan, const MoSrc* srcs, const uint32_t* d_h, size_t npieces, size_t h_stride, const uint32_t* d_h_blinds, int form, bzh_transcript_batch* tb,
                         uint32_t* d_out_points, uint32_t* d_out_evals, uint32_t* d_out_h, uint32_t* d_out_h_blind, void* d_scratch) {
    using SF = typename CurveInfo<C>::SF;
    const int field = CurveInfo<C>::scalar_field;
    const size_t n = (size_t)1 << k, nq = plan.nqueries, nrot = plan.nrot;
    const int canonical = form == BZH_FORM_CANONICAL ? 1 : 0;
    hipStream_t st = ctx->stream;
    EvPasses passes(plan);
    const EvScratch L(plan, passes.jobs.size(), B, npieces);
    if (L.words * 4 + 64 > evaluations_scratch_bytes(plan, B, npieces)) return BZH_E_ARG;
    uint32_t* base = (uint32_t*)(((uintptr_t)d_scratch + 63) & ~(uintptr_t)63);
    auto at = [&](size_t w) { return base + w; };
    uint32_t *x = at(L.x), *xn = at(L.xn), *evals = at(L.evals);

    // the tables, uploaded before the first launch: omega^rotation (omega has order n, so the exponent is taken mod n and a negative
    // rotation needs no inverse), the passes with their sources' addresses, the slots, and h(X)'s sources from the top piece down
    std::vector<Fe<SF>> omegas(nrot);
    const Fe<SF> omega = h_omega<SF>(k);
    for (size_t j = 0; j < nrot; j++) {
        const int64_t m = (int64_t)n, e = (((int64_t)plan.rotations[j] % m) + m) % m;
        omegas[j] = h_pow_u64(omega, (uint64_t)e);
    }
    for (size_t a = 0; a < passes.jobs.size(); a++) passes.jobs[a].src = srcs[passes.poly[a]];
    std::vector<MoSrc> hsrcs;
    for (size_t i = npieces; i-- > 0;) hsrcs.push_back(MoSrc{d_h + i * n * 8, (uint64_t)h_stride});
    const uint32_t hfirst[2] = {0, (uint32_t)npieces};
    EvJob* d_jobs = (EvJob*)at(L.jobs);
    BZH_TRY(h2d_small(ctx, at(L.omegas), omegas.data(), nrot * 32));
    BZH_TRY(h2d_small(ctx, d_jobs, passes.jobs.data(), passes.jobs.size() * sizeof(EvJob)));
    BZH_TRY(h2d_small(ctx, at(L.slots), passes.slots.data(), passes.slots.size() * 4));
    if (npieces) {
        BZH_TRY(h2d_small(ctx, at(L.hsrcs), hsrcs.data(), hsrcs.size() * sizeof(MoSrc)));
        BZH_TRY(h2d_small(ctx, at(L.hfirst), hfirst, sizeof(hfirst)));
    }

    // x; the points, x^n and h_blind
    BZH_TRY(tb_squeeze_locked(tb, BZH_FORM_MONTGOMERY, x));
    hipLaunchKernelGGL((k_ev_scalars<SF>), dim3((unsigned)((B + kEvLanes - 1) / kEvLanes)), dim3(kEvLanes), 0, st, x, at(L.omegas), nrot, k,
                       d_h_blinds, npieces, B, canonical, d_out_points, xn, d_out_h_blind);
    BZH_HIP_TRY(ctx, hipGetLastError());
    // every queried polynomial at all of its points, the passes of 1, 2, .. kEvPass points in a launch each
    size_t first = 0;
    auto pass = [&](auto r) {
        constexpr int R = decltype(r)::value;
        if (const size_t cnt = passes.count[R - 1]) {
            hipLaunchKernelGGL((k_ev_multipoint<SF, R>), dim3((unsigned)cnt, (unsigned)B), dim3(kVecThreads), 0, st, d_jobs + first, at(L.slots),
                               d_out_points, nrot, canonical, n, nq, evals);
            first += cnt;
        }
    };
    static_assert(kEvPass == 5, "one launch per pass size");
    pass(std::integral_constant<int, 1>{}), pass(std::integral_constant<int, 2>{}), pass(std::integral_constant<int, 3>{}),
        pass(std::integral_constant<int, 4>{}), pass(std::integral_constant<int, 5>{});
    BZH_HIP_TRY(ctx, hipGetLastError());
    // the values into the transcripts, in the order of the queries, and to the caller
    BZH_TRY(tb_absorb_locked(tb, 3, evals, nq, nq, BZH_FORM_MONTGOMERY, nullptr));
    if (d_out_evals) {
        hipLaunchKernelGGL((k_ev_export<SF>), dim3((unsigned)((B * nq + kEvLanes - 1) / kEvLanes)), dim3(kEvLanes), 0, st, evals, B * nq, canonical,
                           d_out_evals);
        BZH_HIP_TRY(ctx, hipGetLastError());
    }
    // h(X) = sum_i x^(n i) h_i(X)
    if (npieces) BZH_TRY(mo_combine(ctx, field, (const MoSrc*)at(L.hsrcs), at(L.hfirst), xn, n, B, 1, d_out_h));
    return BZH_OK;
}

int evaluations_device(bzh_ctx* ctx, int curve, size_t batch, unsigned k, const EvPlan& plan, const uint32_t* d_polys, const uint32_t* d_shared,
                       const uint32_t* d_h, size_t npieces, size_t h_stride, const uint32_t* d_h_blinds, int form, bzh_transcript_batch* tb,
                       uint32_t* d_out_points, uint32_t* d_out_evals, uint32_t* d_out_h, uint32_t* d_out_h_blind, void* d_scratch) {
    // the dense operands as a source table: polynomial id of a proof at d_polys + id * n, npolys_own * n between proofs
    const size_t n = (size_t)1 << k, nown = plan.npolys_own;
    std::vector<MoSrc> srcs(nown + plan.npolys_shared);
    for (size_t id = 0; id < srcs.size(); id++)
        srcs[id] = id < nown ? MoSrc{d_polys + id * n * 8, (uint64_t)(nown * n)} : MoSrc{d_shared + (id - nown) * n * 8, 0};
    return evaluations_device_srcs(ctx, curve, batch, k, plan, srcs.data(), d_h, npieces, h_stride, d_h_blinds, form, tb, d_out_points,
                                   d_out_evals, d_out_h, d_out_h_blind, d_scratch);
}

int evaluations_device_srcs(bzh_ctx* ctx, int curve, size_t batch, unsigned k, const EvPlan& plan, const MoSrc* srcs, const uint32_t* d_h,
                            size_t npieces, size_t h_stride, const uint32_t* d_h_blinds, int form, bzh_transcript_batch* tb,
                            uint32_t* d_out_points, uint32_t* d_out_evals, uint32_t* d_out_h, uint32_t* d_out_h_blind, void* d_scratch) {
    return with_curve(curve, [&](auto c) {
        return evaluations_t<decltype(c)>(ctx, batch, k, plan, srcs, d_h, npieces, h_stride, d_h_blinds, form, tb, d_out_points, d_out_evals,
                                          d_out_h, d_out_h_blind, d_scratch);
    });
}

}  // namespace bzh

// what the evaluation phase needs to know about its queries: pure host code
int bzh_evaluations_plan(const bzh_eval_query* queries, size_t nqueries, size_t npolys, int32_t* rotations, size_t* nrotations,
                         uint32_t* point_of_query, uint32_t* poly_order, uint32_t* rot_count) {
    constexpr uint32_t kNone = 0xffffffffu;
    if (!queries || !nqueries || !rotations || !nrotations || !point_of_query || !poly_order || !rot_count) return BZH_E_ARG;
    if (npolys >= kNone || nqueries >= kNone) return BZH_E_ARG;
    for (size_t q = 0; q < nqueries; q++)
        if (queries[q].poly >= npolys) return BZH_E_ARG;
    std::vector<int32_t> rots;
    std::vector<uint32_t> point(nqueries), order;
    std::vector<std::vector<uint32_t>> pts(npolys);
    for (size_t q = 0; q < nqueries; q++) {
        size_t j = std::find(rots.begin(), rots.end(), queries[q].rotation) - rots.begin();
        if (j == rots.size()) rots.push_back(queries[q].rotation);
        point[q] = (uint32_t)j;
        std::vector<uint32_t>& v = pts[queries[q].poly];
        if (v.empty()) order.push_back(queries[q].poly);
        if (std::find(v.begin(), v.end(), (uint32_t)j) == v.end()) v.push_back((uint32_t)j);
        if (v.size() > BZH_EVAL_MAX_ROTATIONS) return BZH_E_ARG;
    }
    for (size_t j = 0; j < rots.size(); j++) rotations[j] = rots[j];
    *nrotations = rots.size();
    for (size_t q = 0; q < nqueries; q++) point_of_query[q] = point[q];
    for (size_t i = 0; i < npolys; i++) poly_order[i] = i < order.size() ? order[i] : kNone, rot_count[i] = (uint32_t)pts[i].size();
    return BZH_OK;
}
