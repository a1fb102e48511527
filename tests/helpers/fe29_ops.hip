// Test program (not product code): applies ONE operation of csrc/fe29.cuh / csrc/curve29.cuh to every case of an operand file
// and writes the raw result words, on the host (--host: the BZH_HD functions in a loop) or on the device (--device: one
// __launch_bounds__(64) kernel per operation, one case per lane; the quad operations put one case on each aligned group of four
// lanes, all four loaded with the same data, and every lane writes its own result).  tests/helpers/fe29_model.py writes the
// operand files and judges the results with Python integers; tests/test_fe29_edges_cpu.py and tests/test_gpu_fe29_edges.py run it.
//
// Built with the optimisation and -std flags csrc/Makefile gives msm.hip.  The INLINING CONTEXT still differs from the product
// kernels (k_msm_accumulate and the reductions inline these functions into loops with their own register pressure and
// scheduling): that part stays covered by the MSM parity tests (tests/test_gpu_msm.py, tests/test_gpu_env_paths.py).
//
// usage: fe29_ops --host|--device fp|fq <operand file> <result file>
// Operand file, 32-bit little-endian words: "FE29", version 1, field (0 = Fp, 1 = Fq), number of sections; then per section
// op, cases, words per case in, words per case out, parameter, and cases x words-in operand words.  An Fe29 is its 9 limbs, a
// saturated element its 8 words, an Xyzz29 x, y, zz, zzz (9 limbs each) and the id flag as a word (37 in all).
// Result file: per section cases x lanes x words-out words (lanes = 4 for the quad operations, else 1).
// Every count comes from the header and is checked on the host against the operation's own table and the file's length before
// anything is touched; after every launch the status of the launch and of the synchronisation is checked, and at the first
// error the program returns non-zero and launches nothing more.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <vector>
#include "curve29.cuh"
using namespace bzh;

enum Op : int {
    OP_MUL, OP_SQR, OP_DOT2, OP_ADD_MUL, OP_CARRY, OP_ADD_C, OP_SUB4, OP_SUB8, OP_SUB16, OP_SUB64, OP_SUB_LAZY81, OP_SUB_LAZY41,
    OP_SUB3_4, OP_FOLD, OP_FROM_SAT_X32, OP_FROM_SAT_REDUCED, OP_TO_SAT, OP_TO_SAT_DIV32, OP_PACK_CANONICAL, OP_IS_ZERO,
    OP_MADD_Q29, OP_MADD, OP_DBL, OP_ADD, OP_ADD_NOCALL, OP_FROM_SAT, OP_XTO_SAT, OP_XTO_SAT_FAST,
    OP_ADD_QUAD, OP_FROM_SAT_QUAD, OP_SHFL_DOWN, OP_COUNT
};
constexpr int kF = 9, kS = 8, kX = 37, kXS = 32;
constexpr int op_in(int op) {
    switch (op) {
    case OP_MUL: case OP_ADD_C: case OP_SUB4: case OP_SUB8: case OP_SUB16: case OP_SUB64: case OP_SUB_LAZY81: case OP_SUB_LAZY41: return 2 * kF;
    case OP_SQR: case OP_CARRY: case OP_FOLD: case OP_TO_SAT: case OP_TO_SAT_DIV32: case OP_PACK_CANONICAL: case OP_IS_ZERO: return kF;
    case OP_DOT2: return 4 * kF;
    case OP_ADD_MUL: case OP_SUB3_4: return 3 * kF;
    case OP_FROM_SAT_X32: case OP_FROM_SAT_REDUCED: return kS;
    case OP_MADD_Q29: return kX + 2 * kF;
    case OP_MADD: return kX + 2 * kS;
    case OP_DBL: case OP_XTO_SAT: case OP_XTO_SAT_FAST: case OP_SHFL_DOWN: return kX;
    case OP_ADD: case OP_ADD_NOCALL: case OP_ADD_QUAD: return 2 * kX;
    case OP_FROM_SAT: case OP_FROM_SAT_QUAD: return kXS;
    default: return 0;
    }
}
constexpr int op_out(int op) {
    switch (op) {
    case OP_TO_SAT: case OP_TO_SAT_DIV32: case OP_PACK_CANONICAL: return kS;
    case OP_IS_ZERO: return 1;
    case OP_MADD_Q29: case OP_MADD: case OP_DBL: case OP_ADD: case OP_ADD_NOCALL: case OP_FROM_SAT: case OP_ADD_QUAD: case OP_FROM_SAT_QUAD:
    case OP_SHFL_DOWN: return kX;
    case OP_XTO_SAT: case OP_XTO_SAT_FAST: return kXS;
    default: return op < OP_COUNT ? kF : 0;
    }
}
constexpr bool op_device_only(int op) { return op == OP_ADD_QUAD || op == OP_FROM_SAT_QUAD || op == OP_SHFL_DOWN; }
constexpr int op_lanes(int op) { return op == OP_ADD_QUAD || op == OP_FROM_SAT_QUAD ? 4 : 1; }

template <class P>
BZH_HD Fe29<P> ld29(const uint32_t* w) {
    Fe29<P> r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.l[i] = w[i];
    return r;
}
template <class P>
BZH_HD void st29(uint32_t* w, const Fe29<P>& v) {
#pragma unroll
    for (int i = 0; i < 9; i++) w[i] = v.l[i];
}
template <class P>
BZH_HD Fe<P> ldsat(const uint32_t* w) {
    Fe<P> r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.l[i] = w[i];
    return r;
}
template <class P>
BZH_HD void stsat(uint32_t* w, const Fe<P>& v) {
#pragma unroll
    for (int i = 0; i < 8; i++) w[i] = v.l[i];
}
template <class P>
BZH_HD Xyzz29<P> ldx(const uint32_t* w) {
    Xyzz29<P> r;
    r.x = ld29<P>(w), r.y = ld29<P>(w + 9), r.zz = ld29<P>(w + 18), r.zzz = ld29<P>(w + 27);
    r.id = w[36] != 0u;
    return r;
}
template <class P>
BZH_HD void stx(uint32_t* w, const Xyzz29<P>& v) {
    st29(w, v.x), st29(w + 9, v.y), st29(w + 18, v.zz), st29(w + 27, v.zzz);
    w[36] = v.id ? 1u : 0u;
}
template <class P>
BZH_HD Xyzz<P> ldxs(const uint32_t* w) {
    Xyzz<P> r;
    r.x = ldsat<P>(w), r.y = ldsat<P>(w + 8), r.zz = ldsat<P>(w + 16), r.zzz = ldsat<P>(w + 24);
    return r;
}
template <class P>
BZH_HD void stxs(uint32_t* w, const Xyzz<P>& v) {
    stsat(w, v.x), stsat(w + 8, v.y), stsat(w + 16, v.zz), stsat(w + 24, v.zzz);
}

// one case of an operation that has a host and a device build
template <class P, int OP>
BZH_HD void apply(const uint32_t* in, uint32_t* out) {
    if constexpr (OP == OP_MUL) st29(out, fe29_mul(ld29<P>(in), ld29<P>(in + 9)));
    else if constexpr (OP == OP_SQR) st29(out, fe29_sqr(ld29<P>(in)));
    else if constexpr (OP == OP_DOT2) st29(out, fe29_dot2(ld29<P>(in), ld29<P>(in + 9), ld29<P>(in + 18), ld29<P>(in + 27)));
    else if constexpr (OP == OP_ADD_MUL) st29(out, fe29_mul(fe29_add(ld29<P>(in), ld29<P>(in + 9)), ld29<P>(in + 18)));
    else if constexpr (OP == OP_CARRY) st29(out, fe29_carry(ld29<P>(in)));
    else if constexpr (OP == OP_ADD_C) st29(out, fe29_add_c(ld29<P>(in), ld29<P>(in + 9)));
    else if constexpr (OP == OP_SUB4) st29(out, fe29_sub<P, 4>(ld29<P>(in), ld29<P>(in + 9)));
    else if constexpr (OP == OP_SUB8) st29(out, fe29_sub<P, 8>(ld29<P>(in), ld29<P>(in + 9)));
    else if constexpr (OP == OP_SUB16) st29(out, fe29_sub<P, 16>(ld29<P>(in), ld29<P>(in + 9)));
    else if constexpr (OP == OP_SUB64) st29(out, fe29_sub<P, 64>(ld29<P>(in), ld29<P>(in + 9)));
    else if constexpr (OP == OP_SUB_LAZY81) st29(out, fe29_sub_lazy<P, 8, 1>(ld29<P>(in), ld29<P>(in + 9)));
    else if constexpr (OP == OP_SUB_LAZY41) st29(out, fe29_sub_lazy<P, 4, 1>(ld29<P>(in), ld29<P>(in + 9)));
    else if constexpr (OP == OP_SUB3_4) st29(out, fe29_sub3<P, 4>(ld29<P>(in), ld29<P>(in + 9), ld29<P>(in + 18)));
    else if constexpr (OP == OP_FOLD) st29(out, fe29_fold(ld29<P>(in)));
    else if constexpr (OP == OP_FROM_SAT_X32) st29(out, fe29_from_sat_x32(ldsat<P>(in)));
    else if constexpr (OP == OP_FROM_SAT_REDUCED) st29(out, fe29_from_sat_reduced(ldsat<P>(in)));
    else if constexpr (OP == OP_TO_SAT) stsat(out, fe29_to_sat(ld29<P>(in), fe29_consts<P>().two256));
    else if constexpr (OP == OP_TO_SAT_DIV32) stsat(out, fe29_to_sat_div32(ld29<P>(in)));
    else if constexpr (OP == OP_PACK_CANONICAL) stsat(out, fe29_pack_canonical(ld29<P>(in)));
    else if constexpr (OP == OP_IS_ZERO) out[0] = fe29_is_zero_mod_p(ld29<P>(in), fe29_consts<P>()) ? 1u : 0u;
    else if constexpr (OP == OP_MADD_Q29) {
        Xyzz29<P> acc = ldx<P>(in);
        xyzz29_madd_q29(acc, ld29<P>(in + 37), ld29<P>(in + 46), fe29_consts<P>());
        stx(out, acc);
    } else if constexpr (OP == OP_MADD) {
        Xyzz29<P> acc = ldx<P>(in);
        Affine<P> q;
        q.x = ldsat<P>(in + 37), q.y = ldsat<P>(in + 45);
        xyzz29_madd(acc, q, fe29_consts<P>());
        stx(out, acc);
    } else if constexpr (OP == OP_DBL) stx(out, xyzz29_dbl(ldx<P>(in)));
    else if constexpr (OP == OP_ADD) {
        Xyzz29<P> acc = ldx<P>(in);
        xyzz29_add(acc, ldx<P>(in + 37));
        stx(out, acc);
    } else if constexpr (OP == OP_ADD_NOCALL) {
        Xyzz29<P> acc = ldx<P>(in);
        xyzz29_add_nocall(acc, ldx<P>(in + 37));
        stx(out, acc);
    } else if constexpr (OP == OP_FROM_SAT) stx(out, xyzz29_from_sat(ldxs<P>(in), fe29_consts<P>()));
    else if constexpr (OP == OP_XTO_SAT) stxs(out, xyzz29_to_sat(ldx<P>(in), fe29_consts<P>()));
    else if constexpr (OP == OP_XTO_SAT_FAST) stxs(out, xyzz29_to_sat_fast(ldx<P>(in)));
}

template <class P, int OP>
__global__ __launch_bounds__(64) void k_op(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    apply<P, OP>(in + (size_t)i * op_in(OP), out + (size_t)i * op_out(OP));
}
// one case per aligned group of four lanes; a quad past the last case leaves as a whole
template <class P, int OP>
__global__ __launch_bounds__(64) void k_quad(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n) {
    const uint32_t t = blockIdx.x * 64u + threadIdx.x, c = t >> 2;
    const int ql = (int)(threadIdx.x & 3u);
    if (c >= n) return;
    const uint32_t* src = in + (size_t)c * op_in(OP);
    uint32_t* dst = out + (size_t)t * op_out(OP);
    if constexpr (OP == OP_ADD_QUAD) {
        Xyzz29<P> acc = ldx<P>(src);
        xyzz29_add_quad(acc, ldx<P>(src + 37), ql);
        stx(dst, acc);
    } else {
        stx(dst, xyzz29_from_sat_quad(ldxs<P>(src), ql));
    }
}
// n is a multiple of 64 (checked on the host): every lane of every wave holds a case and takes part in the shuffle
template <class P>
__global__ __launch_bounds__(64) void k_shfl(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n, int d) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    const Xyzz29<P> v = i < n ? ldx<P>(in + (size_t)i * kX) : xyzz29_identity<P>();
    const Xyzz29<P> o = xyzz29_shfl_down(v, d);
    if (i < n) stx(out + (size_t)i * kX, o);
}

static bool hip_ok(hipError_t e, const char* what) {
    if (e == hipSuccess) return true;
    fprintf(stderr, "fe29_ops: %s: %s\n", what, hipGetErrorString(e));
    return false;
}

struct Section {
    int op;
    uint32_t n, param;
    size_t in_off, out_off;   // word offsets into the operand / result buffers
};

template <class P, int OP>
static bool run_host(const Section& s, const uint32_t* in, uint32_t* out) {
    if constexpr (op_device_only(OP)) {
        fprintf(stderr, "fe29_ops: op %d exists on the device only\n", OP);
        return false;
    } else {
        for (uint32_t i = 0; i < s.n; i++) apply<P, OP>(in + s.in_off + (size_t)i * op_in(OP), out + s.out_off + (size_t)i * op_out(OP));
        return true;
    }
}
template <class P, int OP>
static bool run_device(const Section& s, const uint32_t* in, uint32_t* out) {
    const size_t in_words = (size_t)s.n * op_in(OP), out_words = (size_t)s.n * op_lanes(OP) * op_out(OP);
    if (s.n == 0) return true;
    uint32_t *din = nullptr, *dout = nullptr;
    bool ok = hip_ok(hipMalloc(&din, in_words * 4), "hipMalloc") && hip_ok(hipMalloc(&dout, out_words * 4), "hipMalloc") &&
              hip_ok(hipMemcpy(din, in + s.in_off, in_words * 4, hipMemcpyHostToDevice), "copy in") &&
              hip_ok(hipMemset(dout, 0, out_words * 4), "hipMemset");
    if (ok) {
        const uint32_t blocks = (uint32_t)(((size_t)s.n * op_lanes(OP) + 63) / 64);
        if constexpr (OP == OP_SHFL_DOWN) k_shfl<P><<<blocks, 64>>>(din, dout, s.n, (int)s.param);
        else if constexpr (op_lanes(OP) == 4) k_quad<P, OP><<<blocks, 64>>>(din, dout, s.n);
        else k_op<P, OP><<<blocks, 64>>>(din, dout, s.n);
        ok = hip_ok(hipGetLastError(), "launch") && hip_ok(hipDeviceSynchronize(), "synchronize") &&
             hip_ok(hipMemcpy(out + s.out_off, dout, out_words * 4, hipMemcpyDeviceToHost), "copy out");
    }
    if (din) (void)hipFree(din);
    if (dout) (void)hipFree(dout);
    return ok;
}

template <class P>
static bool run_all(bool device, const std::vector<Section>& secs, const uint32_t* in, uint32_t* out) {
    for (const Section& s : secs) {
        bool ok = false;
        static_for<OP_COUNT>([&](auto i) {
            constexpr int OP = decltype(i)::value;
            if (s.op == OP) ok = device ? run_device<P, OP>(s, in, out) : run_host<P, OP>(s, in, out);
        });
        if (!ok) return false;   // nothing more is launched after the first error
    }
    return true;
}

int main(int argc, char** argv) {
    if (argc != 5 || (strcmp(argv[1], "--host") && strcmp(argv[1], "--device")) || (strcmp(argv[2], "fp") && strcmp(argv[2], "fq"))) {
        fprintf(stderr, "usage: fe29_ops --host|--device fp|fq <operand file> <result file>\n");
        return 2;
    }
    const bool device = !strcmp(argv[1], "--device");
    const uint32_t field = !strcmp(argv[2], "fq") ? 1u : 0u;
    FILE* f = fopen(argv[3], "rb");
    if (!f) return fprintf(stderr, "fe29_ops: cannot open %s\n", argv[3]), 2;
    std::vector<uint32_t> in;
    {
        uint32_t buf[4096];
        size_t got;
        while ((got = fread(buf, 4, 4096, f)) > 0) in.insert(in.end(), buf, buf + got);
        fclose(f);
    }
    if (in.size() < 4 || in[0] != 0x39324546u || in[1] != 1u || in[2] != field || in[3] > 4096u)
        return fprintf(stderr, "fe29_ops: bad file header\n"), 2;
    std::vector<Section> secs;
    size_t pos = 4, out_words = 0;
    for (uint32_t k = 0; k < in[3]; k++) {
        if (in.size() - pos < 5) return fprintf(stderr, "fe29_ops: truncated section header\n"), 2;
        Section s;
        const uint32_t op = in[pos], n = in[pos + 1], wi = in[pos + 2], wo = in[pos + 3];
        s.param = in[pos + 4];
        pos += 5;
        if (op >= (uint32_t)OP_COUNT || n > (1u << 20) || wi != (uint32_t)op_in((int)op) || wo != (uint32_t)op_out((int)op))
            return fprintf(stderr, "fe29_ops: section %u: unknown op or wrong word counts\n", k), 2;
        if (op == OP_SHFL_DOWN && (n % 64u != 0u || s.param < 1u || s.param > 63u))
            return fprintf(stderr, "fe29_ops: section %u: the shuffle wants whole waves and a distance in 1..63\n", k), 2;
        if ((in.size() - pos) / wi < n) return fprintf(stderr, "fe29_ops: section %u: truncated operands\n", k), 2;
        s.op = (int)op, s.n = n, s.in_off = pos, s.out_off = out_words;
        pos += (size_t)n * wi;
        out_words += (size_t)n * op_lanes((int)op) * wo;
        secs.push_back(s);
    }
    if (pos != in.size()) return fprintf(stderr, "fe29_ops: trailing words\n"), 2;
    std::vector<uint32_t> out(out_words, 0u);
    const bool ok = field ? run_all<FqParams>(device, secs, in.data(), out.data()) : run_all<FpParams>(device, secs, in.data(), out.data());
    if (!ok) return 1;
    FILE* g = fopen(argv[4], "wb");
    if (!g) return fprintf(stderr, "fe29_ops: cannot write %s\n", argv[4]), 2;
    const bool wrote = fwrite(out.data(), 4, out.size(), g) == out.size();
    return (fclose(g) == 0 && wrote) ? 0 : 2;
}
