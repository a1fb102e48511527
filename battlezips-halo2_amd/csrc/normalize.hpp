// pasta_curves' Curve::batch_normalize / to_affine and GroupEncoding::to_bytes as host/device templates on Fe<P>: what
// csrc/normalize_compress.hip's kernels run one lane per chain is what its host path (ctx == NULL) runs in a loop over the lanes.
//   normalize_plan    the launch shape: lane t of `lanes` owns the points t, t + lanes, ..., at most `chain` of them
//   normalize_chain   one lane: Montgomery's trick over its chain with ONE fe_inv_ct, then x = X / Z^2, y = Y / Z^3, the affine
//                     point in `form`, the 32-byte encoding and a BZH_POINT_* byte, each optional
//   affine_encode     to_bytes of an affine point in `form`
// h_jac_to_affine and h_compress (csrc/host_field.hpp) are separate code and stay the comparators.
#pragma once
#include "hash_to_curve.hpp"

namespace bzh {

// ---------------------------------------------------------------------------
// The launch shape.  A lane that inverts alone pays the whole inversion (330 products for Fp) for one point, and a launch lasts
// as long as one lane's chain whatever n is, so up to kNormLanes points get a lane each.  Above that a lane chains
// ceil(n / kNormLanes) points -- a chained point costs 7 to 9 products, so a chain of kNormMaxChain adds about as much as the
// inversion itself --, and beyond kNormLanes * kNormMaxChain points the chains stay that long and the lanes multiply.
// ---------------------------------------------------------------------------
constexpr size_t kNormLanes = 16384, kNormMaxChain = 32;
inline void normalize_plan(size_t n, size_t* lanes, size_t* chain) {
    size_t c = (n + kNormLanes - 1) / kNormLanes;
    c = c < 1 ? 1 : (c > kNormMaxChain ? kNormMaxChain : c);
    *chain = c;
    *lanes = (n + c - 1) / c;
}

// 32 bytes at p: two 16-byte moves on the device (p is 16-byte aligned there), bytes on the host (any alignment)
template <class P>
BZH_HD Fe<P> norm_load(const void* p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return fe_load<P>((const uint32_t*)p);
#else
    Fe<P> r;
    memcpy(r.l, p, 32);
    return r;
#endif
}
template <class P>
BZH_HD void norm_store(void* p, const Fe<P>& v) {
#if defined(__HIP_DEVICE_COMPILE__)
    fe_store<P>((uint32_t*)p, v);
#else
    memcpy(p, v.l, 32);
#endif
}

// to_bytes from canonical coordinates: x little-endian, bit 255 = parity of y; the identity (0, 0) = zeros
template <class P>
BZH_HD Fe<P> fe_point_encode(const Fe<P>& xc, const Fe<P>& yc) {
    Fe<P> e = xc;
    e.l[7] |= (yc.l[0] & 1u) << 31;
    return e;
}
// to_bytes of an affine point in `form`.  Through Montgomery form whatever the form, as h_compress goes: a canonical coordinate
// that is not below p is reduced the same way, so the bytes are h_compress's on every input.
template <class P>
BZH_HD Fe<P> affine_encode(const Fe<P>& x, const Fe<P>& y, bool canonical) {
    const Fe<P> xm = canonical ? fe_to_mont(x) : x, ym = canonical ? fe_to_mont(y) : y;
    return fe_point_encode(fe_from_mont(xm), fe_from_mont(ym));
}

// ---------------------------------------------------------------------------
// One call's buffers and shape.  xyz: n x 96 bytes X || Y || Z in `form`; out_xy (n x 64 bytes, `form`), out32 (n x 32 bytes)
// and status (n bytes) may each be null, out_xy and out32 not both.  None of them overlaps xyz.
// ---------------------------------------------------------------------------
struct NormIo {
    const void* xyz;
    void* out_xy;
    void* out32;
    uint8_t* status;
    size_t n, lanes, chain;
    int canonical;
};

// Point i's share of the chain and its status.  The identity (Z = 0) and a point with a canonical coordinate that is not below
// p (BZH_POINT_INVALID, whatever its Z) contribute 1, through a select: they cannot poison the lane's other points.
template <class P>
BZH_HD uint8_t norm_z(const NormIo& io, size_t i, Fe<P>& zsel) {
    const char* p = (const char*)io.xyz + i * 96;
    const Fe<P> Z = norm_load<P>(p + 64);
    bool valid = true;
    if (io.canonical) valid = fe_lt_p(norm_load<P>(p)) && fe_lt_p(norm_load<P>(p + 32)) && fe_lt_p(Z);
    const bool inf = fe_is_zero(Z);  // zero is zero in either form
    const Fe<P> zm = io.canonical ? fe_to_mont(Z) : Z;
    zsel = fe_csel(valid && !inf, zm, fe_one<P>());
    return !valid ? (uint8_t)BZH_POINT_INVALID : (inf ? (uint8_t)BZH_POINT_IDENTITY : (uint8_t)BZH_POINT_OK);
}

// Lane t of io.lanes.  Forward: the product of the Z's before point i waits in the output's own slot i -- the x half of out_xy,
// or the 32 bytes of out32 when there is no out_xy -- so the call needs no buffer besides its outputs; a lane reads and writes
// its own slots only.  Backward: zi = inv * prefix, inv *= Z, then the coordinates.  X and Y stay in `form`: a canonical X times
// the Montgomery zi^2 is the canonical x, so only Z changes form.  Products per chained point, Montgomery / canonical operands:
// 1 / 2 forward, 6 / 7 backward, and 2 / 0 more for the encoding's canonical x and y.  No loop bound and no branch depends on a
// lane's data but the tail guard; the chain length and the choice of outputs are constants of the launch.
template <class C>
BZH_HD void normalize_chain(const NormIo& io, size_t t) {
    using P = typename C::Base;
    char* const pre = io.out_xy ? (char*)io.out_xy : (char*)io.out32;
    const size_t pre_stride = io.out_xy ? 64 : 32;
    Fe<P> acc = fe_one<P>();
#pragma unroll 1
    for (size_t j = 0; j < io.chain; j++) {
        const size_t i = t + j * io.lanes;
        if (i >= io.n) break;
        Fe<P> zsel;
        (void)norm_z<P>(io, i, zsel);
        norm_store<P>(pre + i * pre_stride, acc);
        acc = fe_mul(acc, zsel);
    }
    Fe<P> inv = fe_inv_ct(acc);
    const Fe<P> zero = fe_zero<P>();
#pragma unroll 1
    for (size_t j = io.chain; j-- > 0;) {
        const size_t i = t + j * io.lanes;
        if (i >= io.n) continue;
        Fe<P> zsel;
        const uint8_t st = norm_z<P>(io, i, zsel);
        const char* p = (const char*)io.xyz + i * 96;
        const Fe<P> X = norm_load<P>(p), Y = norm_load<P>(p + 32);
        const Fe<P> zi = fe_mul(inv, norm_load<P>(pre + i * pre_stride));
        inv = fe_mul(inv, zsel);
        const Fe<P> zi2 = fe_sqr(zi);
        const bool ok = st == BZH_POINT_OK;
        const Fe<P> x = fe_csel(ok, fe_mul(X, zi2), zero), y = fe_csel(ok, fe_mul(Y, fe_mul(zi2, zi)), zero);
        if (io.out_xy) {
            norm_store<P>((char*)io.out_xy + i * 64, x);
            norm_store<P>((char*)io.out_xy + i * 64 + 32, y);
        }
        if (io.out32) {
            const Fe<P> xc = io.canonical ? x : fe_from_mont(x), yc = io.canonical ? y : fe_from_mont(y);
            norm_store<P>((char*)io.out32 + i * 32, fe_point_encode(xc, yc));
        }
        if (io.status) io.status[i] = st;
    }
}

}  // namespace bzh
