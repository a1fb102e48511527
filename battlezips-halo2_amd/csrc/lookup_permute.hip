// lookup::prover::permute_expression_pair on gfx950 (halo2_proofs 0.2.0, UPSTREAM; restated by oracle/pasta.py).
//
// For every (input, table) pair of a batch, over the first `usable` rows:
//   A' = the input sorted ascending by canonical value;
//   S'[i] = A'[i] where A'[i] starts a run of equal values; the table values not consumed that way go, ascending, to the
//   repeated rows from the last repeated row backwards.  An input value without a table copy fails that pair (status word);
//   its run start has no copy to take and is filled like a repeated row, so S' of a failed pair is still a permutation of the
//   table (and A' of the input): the pair's grand product closes and what gives the pair away is its status word.
// Equal keys are indistinguishable in the output, so VALUES are sorted, not indices.
//
// Pipeline (every launch covers the whole batch; nothing is read back to choose a path):
//   k_lp_load        canonical copies of both columns, [pair][side][row]; one flag per pair: some value >= 2^16
//   small keys       k_lp_small_sort: one workgroup per column, LDS histogram over 4096 values at a time (LDS atomics), a
//                    prefix sum over the bins, and every output row finds its bin by a search in LDS
//   general keys     k_lp_tile_sort: bitonic sort of 1024-key tiles in LDS (32 KB, words of a key 1024 apart), then
//                    k_lp_merge passes: every element finds its slot by co-rank -- its index in its own run plus a lower
//                    bound (left run) or an upper bound (right run) in the sibling run.  Any usable < 2^31.
//   k_lp_mark        every run start marks the lower bound of its value in the sorted table as used (or fails the pair and marks
//                    its own row as one without a copy)
//   k_lp_assign      one workgroup per pair, two prefix sums: the rows to fill -- repeated rows and run starts without a copy --
//                    are ranked in row order (sum over their flags); the j-th leftover (sum over the not-used flags) lands on
//                    the row of rank m - 1 - j, m = number of rows to fill.
// Leftovers and rows to fill are equally many, failed pair or not: usable - (run starts with a copy) of either.
#include "ctx.hpp"
#include "field.cuh"
#include "host_field.hpp"

namespace bzh {

static constexpr int kLpTile = 1024;        // keys per LDS tile of the general sort
static constexpr int kLpTileThreads = 256;  // two compare-exchanges per thread and stage
static constexpr int kLpBins = 4096;        // histogram bins per pass of the small-key sort
static constexpr int kLpWide = 1024;        // threads of the one-workgroup-per-vector kernels

struct LpKey {
    uint32_t w[8];
};
static __device__ __forceinline__ LpKey lp_load(const uint32_t* p) {
    const uint4* q = reinterpret_cast<const uint4*>(p);
    const uint4 a = q[0], b = q[1];
    LpKey k;
    k.w[0] = a.x; k.w[1] = a.y; k.w[2] = a.z; k.w[3] = a.w;
    k.w[4] = b.x; k.w[5] = b.y; k.w[6] = b.z; k.w[7] = b.w;
    return k;
}
static __device__ __forceinline__ void lp_store(uint32_t* p, const LpKey& k) {
    uint4* q = reinterpret_cast<uint4*>(p);
    q[0] = make_uint4(k.w[0], k.w[1], k.w[2], k.w[3]);
    q[1] = make_uint4(k.w[4], k.w[5], k.w[6], k.w[7]);
}
// canonical order: the most significant word decides (permute_pair_host::Key, limb 3 down to limb 0)
static __device__ __forceinline__ bool lp_less(const LpKey& a, const LpKey& b) {
#pragma unroll
    for (int i = 7; i >= 0; i--)
        if (a.w[i] != b.w[i]) return a.w[i] < b.w[i];
    return false;
}
static __device__ __forceinline__ bool lp_eq(const LpKey& a, const LpKey& b) {
    uint32_t d = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) d |= a.w[i] ^ b.w[i];
    return d == 0;
}
// first index in [0, len) of the sorted run whose key is not below k (upper = false) or above k (upper = true)
static __device__ __forceinline__ uint32_t lp_bound(const uint32_t* run, uint32_t len, const LpKey& k, bool upper) {
    uint32_t lo = 0, hi = len;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        const LpKey m = lp_load(run + (size_t)mid * 8);
        const bool right = upper ? !lp_less(k, m) : lp_less(m, k);
        if (right) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
// exclusive sum of one word per thread over the workgroup (a multiple of 64 threads); sh: one word per wave
static __device__ __forceinline__ uint32_t lp_block_exscan(uint32_t v, uint32_t* sh, uint32_t* total) {
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(inc, d, 64);
        if (lane >= (unsigned)d) inc += t;
    }
    __syncthreads();  // the previous call's readers are done with sh
    if (lane == 63) sh[wave] = inc;
    __syncthreads();
    uint32_t off = 0, tot = 0;
    for (unsigned w = 0; w < nw; w++) {
        const uint32_t s = sh[w];
        if (w < wave) off += s;
        tot += s;
    }
    *total = tot;
    return off + inc - v;
}

// vector v = 2 * pair + side of the working copies starts at element v * usable
template <class P>
__global__ void __launch_bounds__(256) k_lp_load(const uint32_t* __restrict__ in, const uint32_t* __restrict__ tab, size_t stride,
                                                 uint32_t usable, int mont, uint32_t* __restrict__ work, uint32_t* __restrict__ big) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const size_t v = blockIdx.y, pair = v >> 1;
    int is_big = 0;
    if (i < usable) {
        const uint32_t* src = ((v & 1) ? tab : in) + (pair * stride + i) * 8;
        Fe<P> x = fe_load<P>(src);
        if (mont) x = fe_from_mont(x);
        fe_store(work + (v * usable + i) * 8, x);
        is_big = (x.l[0] >> 16) | x.l[1] | x.l[2] | x.l[3] | x.l[4] | x.l[5] | x.l[6] | x.l[7];
    }
    if (__syncthreads_or(is_big) && threadIdx.x == 0) atomicOr(&big[pair], 1u);
}

__global__ void __launch_bounds__(kLpWide) k_lp_small_sort(const uint32_t* __restrict__ src_all, uint32_t* __restrict__ dst_all,
                                                          uint32_t usable, const uint32_t* __restrict__ big) {
    __shared__ uint32_t hist[kLpBins];
    __shared__ uint32_t wave_sums[kLpWide / 64];
    __shared__ uint32_t top;
    const size_t v = blockIdx.x;
    if (big[v >> 1]) return;
    const uint32_t* src = src_all + v * usable * 8;
    uint32_t* dst = dst_all + v * usable * 8;
    const unsigned tid = threadIdx.x;
    if (tid == 0) top = 0;
    __syncthreads();
    uint32_t mx = 0;
    for (uint32_t i = tid; i < usable; i += kLpWide) mx = max(mx, src[(size_t)i * 8]);
    atomicMax(&top, mx);
    __syncthreads();
    const uint32_t passes = top / kLpBins + 1;  // top < 2^16: at most 16
    uint32_t base = 0;
    for (uint32_t c = 0; c < passes; c++) {
        for (unsigned j = tid; j < kLpBins; j += kLpWide) hist[j] = 0;
        __syncthreads();
        for (uint32_t i = tid; i < usable; i += kLpWide) {
            const uint32_t x = src[(size_t)i * 8];
            if (x / kLpBins == c) atomicAdd(&hist[x % kLpBins], 1u);
        }
        __syncthreads();
        // bins -> exclusive offsets: every thread owns kLpBins / kLpWide consecutive bins
        constexpr int per = kLpBins / kLpWide;
        uint32_t cnt[per], sum = 0;
#pragma unroll
        for (int j = 0; j < per; j++) {
            cnt[j] = hist[tid * per + j];
            sum += cnt[j];
        }
        uint32_t total;
        uint32_t off = lp_block_exscan(sum, wave_sums, &total);
#pragma unroll
        for (int j = 0; j < per; j++) {
            hist[tid * per + j] = off;
            off += cnt[j];
        }
        __syncthreads();
        // row r of this pass holds the value of the last bin whose offset is <= r (empty bins share the offset of the next one)
        for (uint32_t r = tid; r < total; r += kLpWide) {
            uint32_t lo = 0, hi = kLpBins;  // hist[lo] <= r < hist[hi] (hist[kLpBins] = total)
            while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) >> 1;
                if (hist[mid] <= r) lo = mid;
                else hi = mid;
            }
            LpKey k = {{c * kLpBins + lo, 0, 0, 0, 0, 0, 0, 0}};
            lp_store(dst + (size_t)(base + r) * 8, k);
        }
        base += total;
        __syncthreads();
    }
}

// sorts tile blockIdx.x of every vector of a general-key pair from src to dst (which may be the same buffer)
__global__ void __launch_bounds__(kLpTileThreads) k_lp_tile_sort(const uint32_t* __restrict__ src_all, uint32_t* __restrict__ dst_all,
                                                                uint32_t usable, const uint32_t* __restrict__ big) {
    __shared__ uint32_t lds[8 * kLpTile];  // word w of key e at lds[w * kLpTile + e]
    const size_t v = blockIdx.y;
    if (!big[v >> 1]) return;
    const uint32_t first = blockIdx.x * (uint32_t)kLpTile;
    const uint32_t cnt = min((uint32_t)kLpTile, usable - first);
    const uint32_t* src = src_all + (v * usable + first) * 8;
    uint32_t* dst = dst_all + (v * usable + first) * 8;
    const unsigned tid = threadIdx.x;
    for (unsigned e = tid; e < kLpTile; e += kLpTileThreads) {
        LpKey k;
        if (e < cnt) {
            k = lp_load(src + (size_t)e * 8);
        } else {  // padding above every field element (moduli are below 2^255)
#pragma unroll
            for (int w = 0; w < 8; w++) k.w[w] = 0xffffffffu;
        }
#pragma unroll
        for (int w = 0; w < 8; w++) lds[w * kLpTile + e] = k.w[w];
    }
    for (unsigned k = 2; k <= kLpTile; k <<= 1) {
        for (unsigned j = k >> 1; j >= 1; j >>= 1) {
            __syncthreads();
            for (unsigned p = tid; p < kLpTile / 2; p += kLpTileThreads) {
                const unsigned i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), q = i | j;
                LpKey a, b;
#pragma unroll
                for (int w = 0; w < 8; w++) {
                    a.w[w] = lds[w * kLpTile + i];
                    b.w[w] = lds[w * kLpTile + q];
                }
                const bool up = (i & k) == 0;
                if (up ? lp_less(b, a) : lp_less(a, b)) {
#pragma unroll
                    for (int w = 0; w < 8; w++) {
                        lds[w * kLpTile + i] = b.w[w];
                        lds[w * kLpTile + q] = a.w[w];
                    }
                }
            }
        }
    }
    __syncthreads();
    for (unsigned e = tid; e < cnt; e += kLpTileThreads) {
        LpKey k;
#pragma unroll
        for (int w = 0; w < 8; w++) k.w[w] = lds[w * kLpTile + e];
        lp_store(dst + (size_t)e * 8, k);
    }
}

// merges the sorted runs [s, s + width) and [s + width, s + 2 width) of every vector, clipped to `usable`
__global__ void __launch_bounds__(256) k_lp_merge(const uint32_t* __restrict__ src_all, uint32_t* __restrict__ dst_all, uint32_t usable,
                                                  uint32_t width, const uint32_t* __restrict__ big) {
    const size_t v = blockIdx.y;
    if (!big[v >> 1]) return;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= usable) return;
    const uint32_t* src = src_all + v * usable * 8;
    uint32_t* dst = dst_all + v * usable * 8;
    const uint32_t start = i - i % (2 * width);
    const uint32_t mid = min(start + width, usable), end = (uint32_t)min((size_t)start + 2 * (size_t)width, (size_t)usable);
    const LpKey k = lp_load(src + (size_t)i * 8);
    uint32_t pos;
    if (i < mid) pos = i + lp_bound(src + (size_t)mid * 8, end - mid, k, false);
    else pos = start + (i - mid) + lp_bound(src + (size_t)start * 8, mid - start, k, true);
    lp_store(dst + (size_t)pos * 8, k);
}

__global__ void __launch_bounds__(256) k_lp_mark(const uint32_t* __restrict__ sorted, uint32_t usable, uint32_t* __restrict__ used,
                                                 uint32_t* __restrict__ nocopy, int32_t* __restrict__ status) {
    const size_t pair = blockIdx.y;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= usable) return;
    const uint32_t* a = sorted + (2 * pair) * usable * 8;
    const uint32_t* t = a + (size_t)usable * 8;
    const LpKey k = lp_load(a + (size_t)i * 8);
    if (i && lp_eq(k, lp_load(a + (size_t)(i - 1) * 8))) return;
    const uint32_t lb = lp_bound(t, usable, k, false);
    if (lb < usable && lp_eq(k, lp_load(t + (size_t)lb * 8))) used[pair * usable + lb] = 1;  // run starts differ: one writer each
    else status[pair] = BZH_E_RANGE, nocopy[pair * usable + i] = 1;   // (a row of the input: this thread's own)
}

template <class P>
static __device__ __forceinline__ void lp_emit(uint32_t* p, const LpKey& k, int mont) {
    Fe<P> x;
#pragma unroll
    for (int w = 0; w < 8; w++) x.l[w] = k.w[w];
    if (mont) x = fe_to_mont(x);
    fe_store(p, x);
}

template <class P>
__global__ void __launch_bounds__(kLpWide) k_lp_assign(const uint32_t* __restrict__ sorted, uint32_t usable, const uint32_t* __restrict__ used,
                                                      const uint32_t* __restrict__ nocopy, uint32_t* __restrict__ row_of_rank, uint32_t* __restrict__ out_a,
                                                      uint32_t* __restrict__ out_s, size_t out_stride, uint32_t rows, int mont) {
    __shared__ uint32_t wave_sums[kLpWide / 64];
    const size_t pair = blockIdx.x;
    const uint32_t* a = sorted + (2 * pair) * usable * 8;
    const uint32_t* t = a + (size_t)usable * 8;
    used += pair * usable;
    nocopy += pair * usable;
    row_of_rank += pair * usable;
    out_a += pair * out_stride * 8;
    out_s += pair * out_stride * 8;
    const unsigned tid = threadIdx.x;
    uint32_t m = 0;  // rows to fill so far
    for (uint32_t i0 = 0; i0 < usable; i0 += kLpWide) {
        const uint32_t i = i0 + tid;
        LpKey k;
        uint32_t fill = 0;  // a repeated row, or a run start whose value the table does not hold
        if (i < usable) {
            k = lp_load(a + (size_t)i * 8);
            fill = (i && lp_eq(k, lp_load(a + (size_t)(i - 1) * 8))) || nocopy[i];
        }
        uint32_t total;
        const uint32_t q = m + lp_block_exscan(fill, wave_sums, &total);
        if (i < usable) {
            lp_emit<P>(out_a + (size_t)i * 8, k, mont);
            if (fill) row_of_rank[q] = i;
            else lp_emit<P>(out_s + (size_t)i * 8, k, mont);
        }
        m += total;
    }
    __threadfence_block();
    __syncthreads();  // row_of_rank is complete
    uint32_t left = 0;  // leftovers so far
    for (uint32_t i0 = 0; i0 < usable; i0 += kLpWide) {
        const uint32_t i = i0 + tid;
        const uint32_t free_ = i < usable && !used[i];
        uint32_t total;
        const uint32_t j = left + lp_block_exscan(free_, wave_sums, &total);
        if (free_ && j < m)  // (always: as many leftovers as rows to fill)
            lp_emit<P>(out_s + (size_t)row_of_rank[m - 1 - j] * 8, lp_load(t + (size_t)i * 8), mont);
        left += total;
    }
    const uint4 z = make_uint4(0, 0, 0, 0);
    for (uint32_t i = usable + tid; i < rows; i += kLpWide) {
        uint4* pa = reinterpret_cast<uint4*>(out_a + (size_t)i * 8);
        uint4* ps = reinterpret_cast<uint4*>(out_s + (size_t)i * 8);
        pa[0] = z; pa[1] = z;
        ps[0] = z; ps[1] = z;
    }
}

namespace {
inline size_t lp_al(size_t v) { return (v + 255) & ~(size_t)255; }
}  // namespace

size_t lookup_permute_ws_bytes(size_t usable, size_t batch) {
    return 2 * lp_al(2 * batch * usable * 32) + 3 * lp_al(batch * usable * 4) + 2 * lp_al(batch * 4);
}

template <class P>
static int lookup_permute_t(bzh_ctx* ctx, const uint32_t* d_in, const uint32_t* d_tab, size_t stride, size_t usable, size_t batch, int mont,
                            uint32_t* d_out_a, uint32_t* d_out_s, size_t out_stride, size_t rows, void* d_ws, int32_t** d_status) {
    if (!usable || usable > stride || usable > rows || rows > out_stride || rows >> 32 || usable >= ((size_t)1 << 31) || !batch || batch > 32767) return BZH_E_ARG;
    hipStream_t st = ctx->stream;
    const uint32_t U = (uint32_t)usable;
    char* w = (char*)d_ws;
    uint32_t* buf0 = (uint32_t*)w;
    w += lp_al(2 * batch * usable * 32);
    uint32_t* buf1 = (uint32_t*)w;
    w += lp_al(2 * batch * usable * 32);
    uint32_t* row_of_rank = (uint32_t*)w;
    w += lp_al(batch * usable * 4);
    char* zeroed = w;  // used | nocopy | big | status: cleared in one piece
    uint32_t* used = (uint32_t*)w;
    w += lp_al(batch * usable * 4);
    uint32_t* nocopy = (uint32_t*)w;
    w += lp_al(batch * usable * 4);
    uint32_t* big = (uint32_t*)w;
    w += lp_al(batch * 4);
    int32_t* status = (int32_t*)w;
    w += lp_al(batch * 4);
    BZH_HIP_TRY(ctx, hipMemsetAsync(zeroed, 0, (size_t)(w - zeroed), st));
    const dim3 per_elem((unsigned)((usable + 255) / 256), (unsigned)(2 * batch));
    hipLaunchKernelGGL((k_lp_load<P>), per_elem, dim3(256), 0, st, d_in, d_tab, stride, U, mont, buf0, big);
    // both sorts end in buf1: the small-key sort goes there directly, the merge passes alternate and the tile sort starts on
    // the side that makes them end there
    hipLaunchKernelGGL(k_lp_small_sort, dim3((unsigned)(2 * batch)), dim3(kLpWide), 0, st, buf0, buf1, U, big);
    const size_t tiles = (usable + kLpTile - 1) / kLpTile;
    int passes = 0;
    for (size_t width = kLpTile; width < usable; width *= 2) passes++;
    uint32_t* cur = (passes & 1) ? buf0 : buf1;
    hipLaunchKernelGGL(k_lp_tile_sort, dim3((unsigned)tiles, (unsigned)(2 * batch)), dim3(kLpTileThreads), 0, st, buf0, cur, U, big);
    for (size_t width = kLpTile; width < usable; width *= 2) {
        uint32_t* nxt = cur == buf0 ? buf1 : buf0;
        hipLaunchKernelGGL(k_lp_merge, per_elem, dim3(256), 0, st, cur, nxt, U, (uint32_t)width, big);
        cur = nxt;
    }
    hipLaunchKernelGGL(k_lp_mark, dim3((unsigned)((usable + 255) / 256), (unsigned)batch), dim3(256), 0, st, buf1, U, used, nocopy, status);
    hipLaunchKernelGGL((k_lp_assign<P>), dim3((unsigned)batch), dim3(kLpWide), 0, st, buf1, U, used, nocopy, row_of_rank, d_out_a, d_out_s, out_stride,
                       (uint32_t)rows, mont);
    BZH_HIP_TRY(ctx, hipGetLastError());
    *d_status = status;
    return BZH_OK;
}

int lookup_permute(bzh_ctx* ctx, int field, const uint32_t* d_in, const uint32_t* d_tab, size_t stride, size_t usable, size_t batch, int form,
                   uint32_t* d_out_a, uint32_t* d_out_s, size_t out_stride, size_t rows, void* d_ws, int32_t** d_status) {
    return with_field(field, [&](auto p) {
        return lookup_permute_t<decltype(p)>(ctx, d_in, d_tab, stride, usable, batch, form == BZH_FORM_MONTGOMERY, d_out_a, d_out_s, out_stride,
                                             rows, d_ws, d_status);
    });
}

}  // namespace bzh
