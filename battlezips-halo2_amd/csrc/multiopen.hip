// The multiopen argument on device-resident transcripts (bzh_multiopen_batch_device) on gfx950.
//
// Replaces halo2_proofs 0.2.0 `poly::multiopen::prover::create_proof` (UPSTREAM, un-vendored) for a caller whose Fiat-Shamir
// transcripts are a bzh_transcript_batch in HBM: x1 .. x4 are squeezed into device memory and read from there by every launch
// that needs them, so nothing goes to the host between the first launch and the last of the opening that ends the call.
// bzh_prove_batch's multiopen() phase (csrc/prover.hpp) does the same arithmetic around host transcripts: its Horner
// combinations run on the expression VM with a constant table built from the host's challenges, its blinds, interpolation and
// batch inversion on the host.  Here:
//   k_mo_combine      the hot kernel: out[z][b][i] = Horner in ch[b] over a source list of (pointer, per-proof stride), one thread
//                     per (proof, coefficient), blockIdx.z over the lists of one launch.  It builds every q_s in one launch
//                     (x1), the dividends q_s - r_s in the division's order, f (x2, over the f_s) and p (x4, over f, q_0, ..).
//   lane kernels      one lane per (proof, set) or per proof, bodies in multiopen_scalars.hpp: the opening points into the
//                     division's order, the blinds' Horner sums, the interpolants r_s with their flags, p_blind, the status byte.
//   poly_eval / poly_kate_division / ipa_commit_blinded / tb_* / ipa_open_device do the rest, all on device operands.
// The sets are ordered by the number of their points, most first ("position"), as the prover's open_quotients orders them: step t
// of the division divides every set that still has a t-th point in one launch, those sets are a prefix of the order, and the
// vectors [position][proof] stay densely packed while they shrink by one coefficient per step.
#include <algorithm>
#include <cstring>
#include <vector>

#include "ctx.hpp"
#include "curve.cuh"
#include "host_field.hpp"
#include "multiopen_scalars.hpp"

static_assert(bzh::kMoMaxPoints == BZH_MULTIOPEN_MAX_POINTS, "lane bodies and header disagree");

namespace bzh {

// (one Horner term, MoSrc: ctx.hpp)
struct MoSteps {
    uint32_t at[kMoMaxPoints];   // entries of the point / evaluation tables before step t
};

static constexpr unsigned kMoBlock = 256;   // a workgroup covers 256 coefficients of ONE proof: the challenge load is wave-uniform
static constexpr unsigned kMoLanes = 64;

// out[(z * out_zstride + b * n + i)] = sum_j src_j[b][i] * x_b^(last - j) over the sources first[z] .. first[z + 1), minus
// sub[z][b][i] for i < kMoMaxPoints when sub is given.  grid (ceil(n / 256), batch, lists)
template <class P>
__global__ void __launch_bounds__(kMoBlock) k_mo_combine(const MoSrc* __restrict__ srcs, const uint32_t* __restrict__ first,
                                                         const uint32_t* __restrict__ ch, size_t n, size_t batch,
                                                         const uint32_t* __restrict__ sub, uint32_t* __restrict__ out, size_t out_zstride) {
    const size_t i = blockIdx.x * (size_t)kMoBlock + threadIdx.x, b = blockIdx.y, z = blockIdx.z;
    if (i >= n) return;
    const Fe<P> x = fe_load<P>(ch + b * 8);
    const uint32_t j0 = first[z], j1 = first[z + 1];
    Fe<P> acc = fe_zero<P>();
    for (uint32_t j = j0; j < j1; j++) {
        const MoSrc s = srcs[j];
        const Fe<P> v = fe_load<P>(s.p + (b * s.stride + i) * 8);
        acc = j == j0 ? v : fe_add(fe_mul(acc, x), v);
    }
    if (sub && i < kMoMaxPoints) acc = fe_sub(acc, fe_load<P>(sub + ((z * batch + b) * kMoMaxPoints + i) * 8));
    fe_store(out + (z * out_zstride + b * n + i) * 8, acc);
}

// entry e = (step, position) of the division's order opens point number pid[e]: xall[e * batch + b] = points[b][pid[e]]
template <class P>
__global__ void __launch_bounds__(kMoLanes) k_mo_points(const uint32_t* __restrict__ points, size_t npoints, const uint32_t* __restrict__ pid,
                                                        size_t entries, size_t batch, int canonical, uint32_t* __restrict__ xall) {
    const size_t g = blockIdx.x * (size_t)kMoLanes + threadIdx.x;
    if (g >= entries * batch) return;
    const size_t e = g / batch, b = g - e * batch;
    mo_point_lane<P>(b, points, npoints, pid[e], canonical != 0, xall, g);
}
// lane (set s, proof b): q_blinds[s * batch + b]
template <class P>
__global__ void __launch_bounds__(kMoLanes) k_mo_blinds(const uint32_t* __restrict__ x1, const uint32_t* __restrict__ blinds, size_t npolys_own,
                                                        const uint32_t* __restrict__ shared_blinds, const uint32_t* __restrict__ grp_first,
                                                        const uint32_t* __restrict__ grp_ids, size_t nsets, size_t batch, int canonical,
                                                        uint32_t* __restrict__ q_blinds) {
    const size_t g = blockIdx.x * (size_t)kMoLanes + threadIdx.x;
    if (g >= nsets * batch) return;
    const size_t s = g / batch, b = g - s * batch;
    mo_blind_lane<P>(b, x1, blinds, npolys_own, shared_blinds, grp_ids + grp_first[s], grp_first[s + 1] - grp_first[s], canonical != 0, q_blinds, g);
}
// lane (position, proof b): r[(pos * batch + b)][8], flags[pos * batch + b]
template <class P>
__global__ void __launch_bounds__(kMoLanes) k_mo_interpolate(const uint32_t* __restrict__ xall, const uint32_t* __restrict__ evals, MoSteps steps,
                                                             const uint32_t* __restrict__ np_of_pos, size_t nsets, size_t batch,
                                                             uint32_t* __restrict__ r, uint8_t* __restrict__ flags) {
    const size_t g = blockIdx.x * (size_t)kMoLanes + threadIdx.x;
    if (g >= nsets * batch) return;
    const size_t pos = g / batch;
    mo_interpolate_lane<P>(xall, evals, g, steps.at, batch, np_of_pos[pos], r + g * kMoMaxPoints * 8, flags + g);
}
// x3 once per (position, proof), for one poly_eval over every q
__global__ void __launch_bounds__(kMoLanes) k_mo_spread(const uint32_t* __restrict__ x3, size_t nsets, size_t batch, uint32_t* __restrict__ out) {
    const size_t g = blockIdx.x * (size_t)kMoLanes + threadIdx.x;
    if (g >= nsets * batch) return;
    const size_t b = g % batch;
    for (int w = 0; w < 8; w++) out[g * 8 + w] = x3[b * 8 + w];
}
// q_s(x3) from the division's order [position][proof] to the transcript's [proof][set]
__global__ void __launch_bounds__(kMoLanes) k_mo_gather(const uint32_t* __restrict__ in, const uint32_t* __restrict__ pos_of_set, size_t nsets,
                                                        size_t batch, uint32_t* __restrict__ out) {
    const size_t g = blockIdx.x * (size_t)kMoLanes + threadIdx.x;
    if (g >= nsets * batch) return;
    const size_t b = g / nsets, s = g - b * nsets;
    for (int w = 0; w < 8; w++) out[g * 8 + w] = in[(pos_of_set[s] * batch + b) * 8 + w];
}
template <class P>
__global__ void __launch_bounds__(kMoLanes) k_mo_final_blind(const uint32_t* __restrict__ x4, const uint32_t* __restrict__ f_blinds,
                                                             const uint32_t* __restrict__ q_blinds, size_t nsets, size_t batch,
                                                             uint32_t* __restrict__ p_blinds) {
    const size_t b = blockIdx.x * (size_t)kMoLanes + threadIdx.x;
    if (b >= batch) return;
    mo_final_blind_lane<P>(b, batch, x4, f_blinds, q_blinds, nsets, p_blinds);
}
__global__ void __launch_bounds__(kMoLanes) k_mo_status(const uint8_t* __restrict__ flags, size_t nsets, const uint8_t* __restrict__ ipa_status,
                                                        size_t batch, uint8_t* __restrict__ status) {
    const size_t b = blockIdx.x * (size_t)kMoLanes + threadIdx.x;
    if (b >= batch) return;
    mo_status_lane(b, batch, flags, nsets, ipa_status, status);
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
namespace {
// the division's order and everything that follows from the plan alone
struct MoOrder {
    size_t nsets = 0, steps = 0, entries = 0, nterms = 0;
    std::vector<uint32_t> order, pos_of_set, np_of_pos, active;   // active[t]: sets with a t-th point
    MoSteps at{};
    explicit MoOrder(const MoPlan& p) : nsets(p.nsets) {
        order.resize(nsets);
        for (size_t s = 0; s < nsets; s++) order[s] = (uint32_t)s;
        std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return p.set_sizes[x] > p.set_sizes[y]; });
        pos_of_set.resize(nsets);
        np_of_pos.resize(nsets);
        for (size_t pos = 0; pos < nsets; pos++) pos_of_set[order[pos]] = (uint32_t)pos, np_of_pos[pos] = p.set_sizes[order[pos]];
        steps = nsets ? np_of_pos[0] : 0;
        active.resize(steps);
        for (size_t t = 0; t < steps; t++) {
            at.at[t] = (uint32_t)entries;
            size_t a = 0;
            while (a < nsets && np_of_pos[a] > t) a++;
            active[t] = (uint32_t)a;
            entries += a;
        }
        for (size_t c = 0; c < p.group_order.size(); c++) nterms += p.group_order[c] != 0xffffffffu;
    }
};
// scratch layout, in 32-bit words; every piece starts 64-byte aligned
struct MoScratch {
    size_t words = 0;
    size_t take(size_t w) {
        const size_t at = words;
        words += (w + 15) & ~(size_t)15;
        return at;
    }
    size_t ch, q, ka, kb, fparts, f, p, commit, out_xyz, raw, fblind, xall, evals, r, qblind, pblind, x3rep, ev3pos, ev3, ipa_v, flags, ipa_st,
        tab, srcs;
    size_t ntab = 0, nsrcs = 0;
    MoScratch(const MoOrder& o, size_t B, size_t n) {
        const size_t big = o.nsets * B * n * 8, ent = std::max<size_t>(o.entries, 1) * B * 8, sb = o.nsets * B * 8;
        ch = take(4 * B * 8);
        q = take(big), ka = take(big), kb = take(big), fparts = take(big);
        f = take(B * n * 8), p = take(B * n * 8);
        commit = take(B * (n + 2) * 8), out_xyz = take(B * 24);
        raw = take(B * 16), fblind = take(B * 8);
        xall = take(ent), evals = take(ent), r = take(sb * kMoMaxPoints);
        qblind = take(sb), pblind = take(B * 8), x3rep = take(sb), ev3pos = take(sb), ev3 = take(sb), ipa_v = take(B * 8);
        flags = take((o.nsets * B + 3) / 4), ipa_st = take((B + 3) / 4);
        // u32 tables: pid | np_of_pos | pos_of_set | grp_first | grp_ids | first_q | first_one (0 .. nsets) | first_f | first_p
        ntab = o.entries + 2 * o.nsets + (o.nsets + 1) + o.nterms + (o.nsets + 1) + (o.nsets + 1) + 2 + 2;
        tab = take(ntab);
        // sources: q (nterms) | dividends (nsets) | f (nsets) | p (1 + nsets)
        nsrcs = o.nterms + 3 * o.nsets + 1;
        srcs = take(nsrcs * (sizeof(MoSrc) / 4));
    }
};
}  // namespace

size_t multiopen_scratch_bytes(const MoPlan& plan, size_t batch, size_t n) {
    const MoOrder o(plan);
    return MoScratch(o, batch, n).words * 4 + 64;
}

template <class C>
static int multiopen_t(bzh_ctx* ctx, const bzh_bases* bases, size_t B, unsigned k, const MoPlan& plan, const MoSrc* poly_srcs,
                       const uint32_t* d_blinds, const uint32_t* d_shared_blinds, const uint32_t* d_points, int form,
                       const uint8_t* d_rng, size_t rng_stride, bzh_transcript_batch* tb, uint8_t* d_status, void* d_scratch) {
    using SF = typename CurveInfo<C>::SF;
    const int field = CurveInfo<C>::scalar_field;
    const size_t n = (size_t)1 << k, nsets = plan.nsets, nown = plan.npolys_own;
    const int canonical = form == BZH_FORM_CANONICAL ? 1 : 0;
    hipStream_t st = ctx->stream;
    const MoOrder o(plan);
    const MoScratch L(o, B, n);
    uint32_t* base = (uint32_t*)(((uintptr_t)d_scratch + 63) & ~(uintptr_t)63);
    auto at = [&](size_t w) { return base + w; };
    uint32_t *x1 = at(L.ch), *x2 = x1 + B * 8, *x3 = x2 + B * 8, *x4 = x3 + B * 8;
    uint32_t *Q = at(L.q), *cur = at(L.ka), *nxt = at(L.kb), *fparts = at(L.fparts), *f = at(L.f), *p = at(L.p);
    uint8_t *flags = (uint8_t*)at(L.flags), *ipa_st = (uint8_t*)at(L.ipa_st);
    const size_t big = B * n * 8;   // words of one set's polynomials

    // the tables: what each launch reads about the plan, in one upload each
    std::vector<uint32_t> tab;
    tab.reserve(L.ntab);
    auto put = [&](const std::vector<uint32_t>& v) {
        const size_t a = tab.size();
        tab.insert(tab.end(), v.begin(), v.end());
        return a;
    };
    std::vector<uint32_t> pid, grp_first(nsets + 1, 0), grp_ids, first_q(nsets + 1, 0), first_one(nsets + 1), first_f{0, (uint32_t)nsets},
        first_p{0, (uint32_t)nsets + 1};
    for (size_t t = 0; t < o.steps; t++)
        for (size_t pos = 0; pos < o.active[t]; pos++) pid.push_back(plan.set_points[o.order[pos] * kMoMaxPoints + t]);
    {   // group_order lists the queried polynomials set by set
        size_t c = 0;
        std::vector<uint32_t> count(nsets, 0);
        for (uint32_t s : plan.set_of_poly)
            if (s != 0xffffffffu) count[s]++;
        for (size_t s = 0; s < nsets; s++) {
            grp_first[s + 1] = grp_first[s] + count[s];
            for (uint32_t i = 0; i < count[s]; i++) grp_ids.push_back(plan.group_order[c++]);
        }
    }
    std::vector<MoSrc> srcs;
    srcs.reserve(L.nsrcs);
    auto src_of = [&](uint32_t id) { return poly_srcs[id]; };
    for (size_t pos = 0; pos < nsets; pos++) {   // q, list z = position
        const size_t s = o.order[pos];
        for (uint32_t c = grp_first[s]; c < grp_first[s + 1]; c++) srcs.push_back(src_of(grp_ids[c]));
        first_q[pos + 1] = (uint32_t)srcs.size();
    }
    const size_t src_div = srcs.size();
    for (size_t pos = 0; pos < nsets; pos++) srcs.push_back(MoSrc{Q + pos * big, (uint64_t)n});
    const size_t src_f = srcs.size();
    for (size_t s = 0; s < nsets; s++) srcs.push_back(MoSrc{fparts + s * big, (uint64_t)n});
    const size_t src_p = srcs.size();
    srcs.push_back(MoSrc{f, (uint64_t)n});
    for (size_t s = 0; s < nsets; s++) srcs.push_back(MoSrc{Q + o.pos_of_set[s] * big, (uint64_t)n});
    for (size_t z = 0; z <= nsets; z++) first_one[z] = (uint32_t)z;
    const size_t t_pid = put(pid), t_np = put(o.np_of_pos), t_pos = put(o.pos_of_set), t_gf = put(grp_first), t_gi = put(grp_ids),
                 t_fq = put(first_q), t_f1 = put(first_one), t_ff = put(first_f), t_fp = put(first_p);
    if (tab.size() != L.ntab || srcs.size() != L.nsrcs) return BZH_E_ARG;
    uint32_t* d_tab = at(L.tab);
    MoSrc* d_srcs = (MoSrc*)at(L.srcs);
    BZH_TRY(h2d_small(ctx, d_tab, tab.data(), tab.size() * 4));
    BZH_TRY(h2d_small(ctx, d_srcs, srcs.data(), srcs.size() * sizeof(MoSrc)));

    const dim3 lanes_sb((unsigned)((nsets * B + kMoLanes - 1) / kMoLanes)), lanes_b((unsigned)((B + kMoLanes - 1) / kMoLanes)), lb(kMoLanes);
    auto combine = [&](const MoSrc* s, const uint32_t* first, const uint32_t* ch, size_t lists, const uint32_t* sub, uint32_t* out) {
        hipLaunchKernelGGL((k_mo_combine<SF>), dim3((unsigned)((n + kMoBlock - 1) / kMoBlock), (unsigned)B, (unsigned)lists), dim3(kMoBlock), 0, st,
                           s, first, ch, n, B, sub, out, B * n);
    };

    // x1, x2; the points in the division's order, the q blinds, every q_s
    BZH_TRY(tb_squeeze_locked(tb, BZH_FORM_MONTGOMERY, x1));
    BZH_TRY(tb_squeeze_locked(tb, BZH_FORM_MONTGOMERY, x2));
    hipLaunchKernelGGL((k_mo_points<SF>), dim3((unsigned)((o.entries * B + kMoLanes - 1) / kMoLanes)), lb, 0, st, d_points, plan.npoints,
                       d_tab + t_pid, o.entries, B, canonical, at(L.xall));
    hipLaunchKernelGGL((k_mo_blinds<SF>), lanes_sb, lb, 0, st, x1, d_blinds, nown, d_shared_blinds, d_tab + t_gf, d_tab + t_gi, nsets, B,
                       canonical, at(L.qblind));
    combine(d_srcs, d_tab + t_fq, x1, nsets, nullptr, Q);
    BZH_HIP_TRY(ctx, hipGetLastError());
    // q_s at its own points (the sets that have a t-th point are the first active[t] positions), the remainders, q_s - r_s
    for (size_t t = 0; t < o.steps; t++)
        BZH_TRY(poly_eval(ctx, field, Q, n, o.active[t] * B, at(L.xall) + o.at.at[t] * B * 8, 1, at(L.evals) + o.at.at[t] * B * 8));
    hipLaunchKernelGGL((k_mo_interpolate<SF>), lanes_sb, lb, 0, st, at(L.xall), at(L.evals), o.at, d_tab + t_np, nsets, B, at(L.r), flags);
    combine(d_srcs + src_div, d_tab + t_f1, x1, nsets, at(L.r), cur);
    BZH_HIP_TRY(ctx, hipGetLastError());
    // f_s = (q_s - r_s) / prod (X - point): one division per step for every set that still has a point, zero-padded to n
    BZH_HIP_TRY(ctx, hipMemsetAsync(fparts, 0, nsets * big * 4, st));
    size_t len = n;
    for (size_t t = 0; t < o.steps; t++) {
        BZH_TRY(poly_kate_division(ctx, field, cur, len, o.active[t] * B, at(L.xall) + o.at.at[t] * B * 8, nxt));
        std::swap(cur, nxt);
        len--;
        for (size_t pos = 0; pos < o.active[t]; pos++)   // the sets whose last point this was
            if (o.np_of_pos[pos] == t + 1 && len)
                BZH_HIP_TRY(ctx, hipMemcpy2DAsync(fparts + o.order[pos] * big, n * 32, cur + pos * B * len * 8, len * 32, len * 32, B,
                                                  hipMemcpyDeviceToDevice, st));
    }
    // f, its blind (the first draw) and its commitment; x3; q_s(x3); x4
    combine(d_srcs + src_f, d_tab + t_ff, x2, 1, nullptr, f);
    BZH_HIP_TRY(ctx, hipGetLastError());
    BZH_HIP_TRY(ctx, hipMemcpy2DAsync(at(L.raw), 64, d_rng, rng_stride, 64, B, hipMemcpyDeviceToDevice, st));
    BZH_TRY(random_field(ctx, field, at(L.raw), B, at(L.fblind)));
    BZH_TRY(ipa_commit_blinded(ctx, bases, f, B, at(L.fblind), at(L.commit), at(L.out_xyz)));
    BZH_TRY(tb_write_jacobian_locked(tb, at(L.out_xyz), 1, 1, BZH_FORM_MONTGOMERY));
    BZH_TRY(tb_squeeze_locked(tb, BZH_FORM_MONTGOMERY, x3));
    hipLaunchKernelGGL(k_mo_spread, lanes_sb, lb, 0, st, x3, nsets, B, at(L.x3rep));
    BZH_HIP_TRY(ctx, hipGetLastError());
    BZH_TRY(poly_eval(ctx, field, Q, n, nsets * B, at(L.x3rep), 1, at(L.ev3pos)));
    hipLaunchKernelGGL(k_mo_gather, lanes_sb, lb, 0, st, at(L.ev3pos), d_tab + t_pos, nsets, B, at(L.ev3));
    BZH_HIP_TRY(ctx, hipGetLastError());
    BZH_TRY(tb_absorb_locked(tb, 3, at(L.ev3), nsets, nsets, BZH_FORM_MONTGOMERY, nullptr));
    BZH_TRY(tb_squeeze_locked(tb, BZH_FORM_MONTGOMERY, x4));
    // p, p_blind, and the opening of p at x3 with the draws after the first
    combine(d_srcs + src_p, d_tab + t_fp, x4, 1, nullptr, p);
    hipLaunchKernelGGL((k_mo_final_blind<SF>), lanes_b, lb, 0, st, x4, at(L.fblind), at(L.qblind), nsets, B, at(L.pblind));
    BZH_HIP_TRY(ctx, hipGetLastError());
    BZH_TRY(ipa_open_device(ctx, bases, p, B, at(L.pblind), x3, BZH_FORM_MONTGOMERY, d_rng + 64, rng_stride, tb, at(L.ipa_v), ipa_st));
    if (d_status) {
        hipLaunchKernelGGL(k_mo_status, lanes_b, lb, 0, st, flags, nsets, ipa_st, B, d_status);
        BZH_HIP_TRY(ctx, hipGetLastError());
    }
    return BZH_OK;
}

int multiopen_device(bzh_ctx* ctx, const bzh_bases* bases, size_t batch, unsigned k, const MoPlan& plan, const uint32_t* d_polys,
                     const uint32_t* d_shared, const uint32_t* d_blinds, const uint32_t* d_shared_blinds, const uint32_t* d_points, int form,
                     const uint8_t* d_rng, size_t rng_stride, bzh_transcript_batch* tb, uint8_t* d_status, void* d_scratch) {
    // the dense operands as a source table: polynomial id of a proof at d_polys + id * n, npolys_own * n between proofs
    const size_t n = (size_t)1 << k, nown = plan.npolys_own;
    std::vector<MoSrc> srcs(nown + plan.npolys_shared);
    for (size_t id = 0; id < srcs.size(); id++)
        srcs[id] = id < nown ? MoSrc{d_polys + id * n * 8, (uint64_t)(nown * n)} : MoSrc{d_shared + (id - nown) * n * 8, 0};
    return multiopen_device_srcs(ctx, bases, batch, k, plan, srcs.data(), d_blinds, d_shared_blinds, d_points, form, d_rng, rng_stride, tb,
                                 d_status, d_scratch);
}

int multiopen_device_srcs(bzh_ctx* ctx, const bzh_bases* bases, size_t batch, unsigned k, const MoPlan& plan, const MoSrc* srcs,
                          const uint32_t* d_blinds, const uint32_t* d_shared_blinds, const uint32_t* d_points, int form, const uint8_t* d_rng,
                          size_t rng_stride, bzh_transcript_batch* tb, uint8_t* d_status, void* d_scratch) {
    return with_curve(bases->curve, [&](auto c) {
        return multiopen_t<decltype(c)>(ctx, bases, batch, k, plan, srcs, d_blinds, d_shared_blinds, d_points, form, d_rng, rng_stride, tb,
                                        d_status, d_scratch);
    });
}

int mo_combine(bzh_ctx* ctx, int field, const MoSrc* d_srcs, const uint32_t* d_first, const uint32_t* d_ch, size_t n, size_t batch,
               size_t lists, uint32_t* d_out) {
    return with_field(field, [&](auto p) {
        hipLaunchKernelGGL((k_mo_combine<decltype(p)>), dim3((unsigned)((n + kMoBlock - 1) / kMoBlock), (unsigned)batch, (unsigned)lists),
                           dim3(kMoBlock), 0, ctx->stream, d_srcs, d_first, d_ch, n, batch, (const uint32_t*)nullptr, d_out, batch * n);
        BZH_HIP_TRY(ctx, hipGetLastError());
        return BZH_OK;
    });
}

}  // namespace bzh

// upstream's construct_intermediate_sets on (polynomial, point number) pairs: pure host code
int bzh_multiopen_plan(const bzh_open_query* queries, size_t nqueries, size_t npolys, size_t npoints, uint32_t* set_of_poly,
                       uint32_t* group_order, uint32_t* set_sizes, uint32_t* set_points, size_t* nsets) {
    constexpr uint32_t kNone = 0xffffffffu;
    constexpr size_t M = BZH_MULTIOPEN_MAX_POINTS;
    if (!queries || !nqueries || !set_of_poly || !group_order || !set_sizes || !set_points || !nsets) return BZH_E_ARG;
    if (npolys >= kNone || npoints >= kNone) return BZH_E_ARG;
    for (size_t i = 0; i < nqueries; i++)
        if (queries[i].poly >= npolys || queries[i].point >= npoints) return BZH_E_ARG;
    // every polynomial's points, ascending and without repeats, in first-seen order of the polynomials
    std::vector<std::vector<uint32_t>> pts(npolys);
    std::vector<uint32_t> seen;
    for (size_t i = 0; i < nqueries; i++) {
        std::vector<uint32_t>& v = pts[queries[i].poly];
        if (v.empty()) seen.push_back(queries[i].poly);
        const auto it = std::lower_bound(v.begin(), v.end(), queries[i].point);
        if (it == v.end() || *it != queries[i].point) v.insert(it, queries[i].point);
    }
    std::vector<std::vector<uint32_t>> sets, members;
    for (uint32_t poly : seen) {
        if (pts[poly].size() > M) return BZH_E_ARG;
        size_t s = 0;
        while (s < sets.size() && sets[s] != pts[poly]) s++;
        if (s == sets.size()) sets.push_back(pts[poly]), members.emplace_back();
        members[s].push_back(poly);
    }
    for (size_t i = 0; i < npolys; i++) set_of_poly[i] = group_order[i] = kNone;
    size_t at = 0;
    for (size_t s = 0; s < sets.size(); s++) {
        set_sizes[s] = (uint32_t)sets[s].size();
        for (size_t j = 0; j < M; j++) set_points[s * M + j] = j < sets[s].size() ? sets[s][j] : kNone;
        for (uint32_t poly : members[s]) set_of_poly[poly] = (uint32_t)s, group_order[at++] = poly;
    }
    *nsets = sets.size();
    return BZH_OK;
}
