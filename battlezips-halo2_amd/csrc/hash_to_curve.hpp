// pasta_curves 0.4.1's CurveExt::hash_to_curve as two uniform-control-flow stages on Fe<P>, host and device: what
// csrc/hash_to_curve.hip's kernels run one lane per message is what its host path (ctx == NULL) runs in a loop.
//   h2c_hash_to_field  expand_message_xmd over BLAKE2b-512 (len_in_bytes = 128, no personalisation) -> u0, u1 (Montgomery)
//   h2c_map            iso_map(swu(u0) + swu(u1)) -> affine point (Montgomery) and a BZH_POINT_* status
// csrc/params.hip's hash_to_curve_t (bzh_hash_to_curve, bzh_params_generators: one message of any length at a time) streams its
// own expand_message_xmd and then runs h2f_os2ip and h2c_map from here with the same constants (h2c_host): there is one map.
#pragma once
#include <string>

#include "host_field.hpp"

namespace bzh {

// ---------------------------------------------------------------------------
// a^(p - 2) with the exponent's bits as compile-time constants of the field (no table of exponent limbs in private memory);
// 0 -> 0.  254 squarings + popcount(p - 2) - 1 products: 330 for Fp, 327 for Fq.
// ---------------------------------------------------------------------------
template <class P>
struct InvExp {
    struct Limbs {
        uint32_t v[8];
    };
    static constexpr Limbs make() {  // p - 2
        Limbs r{};
        uint64_t br = 2;
        for (int i = 0; i < 8; i++) {
            const uint64_t d = (uint64_t)P::mod(i) - br;
            r.v[i] = (uint32_t)d;
            br = (d >> 63) & 1;
        }
        return r;
    }
    BZH_HD static constexpr unsigned bit(int i) {
        constexpr Limbs e = make();
        return (e.v[i >> 5] >> (i & 31)) & 1u;
    }
    static constexpr int top_bit() {
        int i = 255;
        while (i > 0 && bit(i) == 0) i--;
        return i;
    }
    static constexpr int top = top_bit();
};
template <class P>
BZH_HD Fe<P> fe_inv_ct(const Fe<P>& a) {
    Fe<P> acc = a;
#pragma unroll 1
    for (int i = InvExp<P>::top - 1; i >= 0; i--) {
        acc = fe_sqr(acc);
        if (InvExp<P>::bit(i)) acc = fe_mul(acc, a);
    }
    return acc;
}

// ---------------------------------------------------------------------------
// BLAKE2b compression (RFC 7693) with state and message words in registers: the twelve rounds are unrolled at compile time,
// so every sigma lookup is a constant index.
// ---------------------------------------------------------------------------
BZH_HD constexpr int b2_sigma(int r, int i) {
    constexpr uint8_t S[10][16] = {
        {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
        {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4}, {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
        {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13}, {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
        {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11}, {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
        {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5}, {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0}};
    return S[r % 10][i];
}
BZH_HD constexpr uint64_t b2_iv(int i) {
    constexpr uint64_t IV[8] = {0x6a09e667f3bcc908ULL, 0xbb67ae8584caa73bULL, 0x3c6ef372fe94f82bULL, 0xa54ff53a5f1d36f1ULL,
                                0x510e527fade682d1ULL, 0x9b05688c2b3e6c1fULL, 0x1f83d9abfb41bd6bULL, 0x5be0cd19137e2179ULL};
    return IV[i];
}
BZH_HD uint64_t b2_rotr(uint64_t x, int n) { return (x >> n) | (x << (64 - n)); }
#define BZH_B2_G(a, b, c, d, x, y)   \
    v[a] = v[a] + v[b] + (x);        \
    v[d] = b2_rotr(v[d] ^ v[a], 32); \
    v[c] = v[c] + v[d];              \
    v[b] = b2_rotr(v[b] ^ v[c], 24); \
    v[a] = v[a] + v[b] + (y);        \
    v[d] = b2_rotr(v[d] ^ v[a], 16); \
    v[c] = v[c] + v[d];              \
    v[b] = b2_rotr(v[b] ^ v[c], 63);
// h <- F(h, m, t, last); t < 2^64
BZH_HD void b2_compress(uint64_t (&h)[8], const uint64_t (&m)[16], uint64_t t, bool last) {
    uint64_t v[16];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        v[i] = h[i];
        v[i + 8] = b2_iv(i);
    }
    v[12] ^= t;
    v[14] = last ? ~v[14] : v[14];
    static_for<12>([&](auto R) {
        constexpr int r = decltype(R)::value;
        BZH_B2_G(0, 4, 8, 12, m[b2_sigma(r, 0)], m[b2_sigma(r, 1)])
        BZH_B2_G(1, 5, 9, 13, m[b2_sigma(r, 2)], m[b2_sigma(r, 3)])
        BZH_B2_G(2, 6, 10, 14, m[b2_sigma(r, 4)], m[b2_sigma(r, 5)])
        BZH_B2_G(3, 7, 11, 15, m[b2_sigma(r, 6)], m[b2_sigma(r, 7)])
        BZH_B2_G(0, 5, 10, 15, m[b2_sigma(r, 8)], m[b2_sigma(r, 9)])
        BZH_B2_G(1, 6, 11, 12, m[b2_sigma(r, 10)], m[b2_sigma(r, 11)])
        BZH_B2_G(2, 7, 8, 13, m[b2_sigma(r, 12)], m[b2_sigma(r, 13)])
        BZH_B2_G(3, 4, 9, 14, m[b2_sigma(r, 14)], m[b2_sigma(r, 15)])
    });
#pragma unroll
    for (int i = 0; i < 8; i++) h[i] ^= v[i] ^ v[i + 8];
}
#undef BZH_B2_G

// ---------------------------------------------------------------------------
// hash_to_field.  Every message of a launch has the same length and the same DST, so the block layout is a constant of the
// launch, prepared once on the host (h2f_plan, csrc/hash_to_curve.hip):
//   hash 0  Z_pad (128 zero bytes) | msg | 0, 128, 0 | dst_prime     h0 = the chaining value after Z_pad; t0 = the blocks that
//                                                                    follow it, with zeros where the message goes
//   hash 1  b_0 | 1 | dst_prime,  hash 2  (b_0 ^ b_1) | 2 | dst_prime   t1 = their blocks, zeros in the first 65 bytes
// msg_len <= 128 and len(dst_prime) <= 256: at most 4 and 3 blocks.
// ---------------------------------------------------------------------------
struct H2fPlan {
    uint64_t h0[8];
    uint64_t t0[64];
    uint64_t t1[64];  // three blocks used; as long as t0, so that a select between the two never indexes past either
    uint32_t msg_len, nb0, nb1;
    uint32_t len0, len1;  // bytes hashed by hash 0 (Z_pad included) and by hash 1 / 2
};
// OS2IP of a 64-byte big-endian digest (d = its eight little-endian words) mod p: lo R^2 + (hi R^2) R^2, as the host does
template <class P>
BZH_HD Fe<P> h2f_os2ip(const uint64_t (&d)[8]) {
    Fe<P> lo, hi;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint64_t l = __builtin_bswap64(d[7 - i]), h = __builtin_bswap64(d[3 - i]);
        lo.l[2 * i] = (uint32_t)l, lo.l[2 * i + 1] = (uint32_t)(l >> 32);
        hi.l[2 * i] = (uint32_t)h, hi.l[2 * i + 1] = (uint32_t)(h >> 32);
    }
    const Fe<P> r2 = fe_r2<P>();
    return fe_add(fe_mul(lo, r2), fe_mul(fe_mul(hi, r2), r2));
}
// msg: the lane's msg_len bytes; srs: the message is 0u8 || (index as u32 LE) instead (msg_len = 5) and msg is not read
template <class P>
BZH_HD void h2c_hash_to_field(const H2fPlan& pl, const uint8_t* msg, bool srs, uint32_t index, Fe<P>& u0, Fe<P>& u1) {
    uint64_t h[8], b0[8] = {0, 0, 0, 0, 0, 0, 0, 0}, b1[8] = {0, 0, 0, 0, 0, 0, 0, 0}, m[16];
#pragma unroll 1
    for (uint32_t s = 0; s < 3; s++) {
        const uint32_t nb = s == 0 ? pl.nb0 : pl.nb1;
#pragma unroll
        for (int i = 0; i < 8; i++) h[i] = s == 0 ? pl.h0[i] : b2_iv(i);
        if (s != 0) h[0] ^= 0x01010040ull;  // digest length 64, no key, fanout 1, depth 1
#pragma unroll 1
        for (uint32_t b = 0; b < nb; b++) {
#pragma unroll
            for (int w = 0; w < 16; w++) m[w] = s == 0 ? pl.t0[b * 16 + w] : pl.t1[b * 16 + w];
            if (b == 0) {
                if (s == 0) {
                    if (!srs) {
#pragma unroll
                        for (int w = 0; w < 16; w++) {
                            uint64_t x = 0;
#pragma unroll
                            for (int j = 0; j < 8; j++)
                                if ((uint32_t)(8 * w + j) < pl.msg_len) x |= (uint64_t)msg[8 * w + j] << (8 * j);
                            m[w] |= x;
                        }
                    } else {
                        m[0] |= (uint64_t)index << 8;
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < 8; i++) m[i] = s == 1 ? b0[i] : b0[i] ^ b1[i];
                    m[8] |= s;
                }
            }
            const bool last = b + 1 == nb;
            const uint64_t t = last ? (s == 0 ? pl.len0 : pl.len1) : (uint64_t)128 * (b + 1 + (s == 0 ? 1 : 0));
            b2_compress(h, m, t, last);
        }
        if (s == 0) {
#pragma unroll
            for (int i = 0; i < 8; i++) b0[i] = h[i];
        } else if (s == 1) {
#pragma unroll
            for (int i = 0; i < 8; i++) b1[i] = h[i];
            u0 = h2f_os2ip<P>(h);
        } else {
            u1 = h2f_os2ip<P>(h);
        }
    }
}

// ---------------------------------------------------------------------------
// map_to_curve.  Constants of the iso-curve y^2 = x^3 + A x + B and of the normalised 3-isogeny (csrc/params.hip's Iso<F>, after
// its self-check), Montgomery form:
//   mba = -B / A,  bza = B / (Z A)  (x1 when ta = 0),  t, u (Velu),  s2 = 1/9,  s3 = 1/27,
//   c = sqrt(Z g) with g = gpow[0], the generator of the 2-Sylow subgroup fe_sqrt_ct works with.
// Every `if` of map_to_curve_simple_swu, iso_add and iso_map is a select.  Products per h2c_map: 9 and one inversion for 1 / ta
// of both maps at once; 2 x (9 + one root) for the two maps -- ONE root each: for a non-square gx1 fe_sqrt_ct leaves r with
// r^2 = gx1 / g, so sqrt(gx2) = sqrt(Z^3 u^6 gx1) = Z u^2 * u * r * c costs three products instead of a second root --; 10, one
// inversion and 17 for the addition and the isogeny on fractions, which share that inversion.  54 + 2 inversions + 2 roots:
// 1 884 for Fq (327, 588), 1 896 for Fp (330, 591).
// ---------------------------------------------------------------------------
template <class P>
struct H2cConsts {
    Fe<P> a, b, z, x0, t, u, s2, s3, mba, bza, c;
};
template <class P>
BZH_HD bool fe_lt_p(const Fe<P>& x) {  // the limbs are a canonical encoding, limb by limb from the top
    bool below = false, decided = false;
#pragma unroll
    for (int k = 7; k >= 0; k--) {
        const bool ne = x.l[k] != P::mod(k);
        below = (!decided && ne) ? x.l[k] < P::mod(k) : below;
        decided = decided || ne;
    }
    return below;
}
template <class P>
BZH_HD bool fe_is_odd(const Fe<P>& a) {  // sgn0 of a Montgomery element
    return fe_from_mont(a).l[0] & 1u;
}
// simplified SWU (RFC 9380 6.6.2) for one u; ta_inv = 1 / ta, anything when ta = 0
template <class P>
BZH_HD void h2c_swu(const Fe<P>& u, const Fe<P>& zu2, bool ta_zero, const Fe<P>& ta_inv, const H2cConsts<P>& K, const uint32_t* gpow,
                    Fe<P>& x, Fe<P>& y) {
    const Fe<P> x1 = fe_csel(ta_zero, K.bza, fe_mul(K.mba, fe_add(fe_one<P>(), ta_inv)));
    const Fe<P> gx1 = fe_add(fe_mul(fe_add(fe_sqr(x1), K.a), x1), K.b);
    Fe<P> r;
    const bool sq = fe_sqrt_ct(gx1, gpow, r);
    const Fe<P> y2 = fe_mul(fe_mul(fe_mul(zu2, u), r), K.c);
    x = fe_csel(sq, x1, fe_mul(zu2, x1));
    y = fe_csel(sq, r, y2);
    y = fe_csel(fe_is_odd(u) != fe_is_odd(y), fe_neg(y), y);  // sgn0(u) == sgn0(y)
}
// iso_map(swu(u0) + swu(u1)): BZH_POINT_OK and the point, or BZH_POINT_IDENTITY and zeros
template <class P>
BZH_HD uint8_t h2c_map(const Fe<P>& u0, const Fe<P>& u1, const H2cConsts<P>& K, const uint32_t* gpow, Fe<P>& ox, Fe<P>& oy) {
    const Fe<P> one = fe_one<P>();
    const Fe<P> zu0 = fe_mul(K.z, fe_sqr(u0)), zu1 = fe_mul(K.z, fe_sqr(u1));
    const Fe<P> ta0 = fe_add(fe_sqr(zu0), zu0), ta1 = fe_add(fe_sqr(zu1), zu1);
    const bool z0 = fe_is_zero(ta0), z1 = fe_is_zero(ta1);
    const Fe<P> d0 = fe_csel(z0, one, ta0), d1 = fe_csel(z1, one, ta1);
    const Fe<P> ti = fe_inv_ct(fe_mul(d0, d1));
    Fe<P> px, py, qx, qy;
    h2c_swu(u0, zu0, z0, fe_mul(ti, d1), K, gpow, px, py);
    h2c_swu(u1, zu1, z1, fe_mul(ti, d0), K, gpow, qx, qy);
    // p + q on the iso-curve as fractions: lambda = N / D (the tangent when p = q), x3 = X3 / D^2, y3 = Y3 / D^3;
    // D = 0 exactly when the sum is the identity (opposite points, or doubling a point of order two)
    const bool dbl = fe_eq(px, qx) && fe_eq(py, qy);
    const Fe<P> px2 = fe_sqr(px);
    const Fe<P> N = fe_csel(dbl, fe_add(fe_add(fe_dbl(px2), px2), K.a), fe_sub(qy, py));
    const Fe<P> D = fe_csel(dbl, fe_dbl(py), fe_sub(qx, px));
    const Fe<P> D2 = fe_sqr(D), D3 = fe_mul(D2, D);
    const Fe<P> X3 = fe_sub(fe_sqr(N), fe_mul(fe_add(px, qx), D2));
    const Fe<P> Y3 = fe_sub(fe_mul(N, fe_sub(fe_mul(px, D2), X3)), fe_mul(py, D3));
    // the isogeny: d = x3 - x0 = W / D^2; W = 0 for the kernel points, which map to the identity
    const Fe<P> W = fe_sub(X3, fe_mul(K.x0, D2));
    const bool inf = fe_is_zero(D) || fe_is_zero(W);
    const Fe<P> inv = fe_inv_ct(fe_mul(D, W));
    const Fe<P> Di = fe_mul(inv, W), Wi = fe_mul(inv, D);
    const Fe<P> Di2 = fe_sqr(Di);
    const Fe<P> x3 = fe_mul(X3, Di2), y3 = fe_mul(Y3, fe_mul(Di2, Di));
    const Fe<P> di = fe_mul(D2, Wi), di2 = fe_sqr(di);
    const Fe<P> X = fe_add(x3, fe_add(fe_mul(K.t, di), fe_mul(K.u, di2)));
    const Fe<P> Y = fe_mul(y3, fe_sub(one, fe_add(fe_mul(K.t, di2), fe_mul(fe_dbl(K.u), fe_mul(di2, di)))));
    const Fe<P> zero = fe_zero<P>();
    ox = fe_csel(inf, zero, fe_mul(K.s2, X));
    oy = fe_csel(inf, zero, fe_mul(K.s3, Y));
    return inf ? BZH_POINT_IDENTITY : BZH_POINT_OK;
}

// ---------------------------------------------------------------------------
// host side: the domain separation tag and the map's constants, made once per curve
// ---------------------------------------------------------------------------
template <class C>
inline std::string h2c_dst(const char* prefix) {
    return std::string(prefix) + "-" + (C::id == BZH_CURVE_PALLAS ? "pallas" : "vesta") + "_XMD:BLAKE2b_SSWU_RO_";
}
// the iso-curve and isogeny constants, canonical limbs: A, B, Z, x0, t, u, 1/9, 1/27.  csrc/params.hip derives them and checks
// them (Iso<F>); BZH_E_HIP if that self-check fails
int h2c_iso_constants(int curve, uint64_t out[8][4]);
template <class C>
struct H2cHost {
    H2cConsts<typename C::Base> K;
    bool ok = false;
    H2cHost() {
        using P = typename C::Base;
        uint64_t raw[8][4];
        if (h2c_iso_constants(C::id, raw) != BZH_OK) return;
        Fe<P> v[8];
        for (int i = 0; i < 8; i++) v[i] = fe_from_u64<P>(raw[i], BZH_FORM_CANONICAL);
        K.a = v[0], K.b = v[1], K.z = v[2], K.x0 = v[3], K.t = v[4], K.u = v[5], K.s2 = v[6], K.s3 = v[7];
        const Fe<P> ai = fe_inv(K.a);
        K.mba = fe_mul(fe_neg(K.b), ai);
        K.bza = fe_mul(K.b, fe_mul(fe_inv(K.z), ai));
        // Z and g are non-squares, so Z g has a root; it turns fe_sqrt_ct's r for a non-square gx1 (r^2 = gx1 / g) into sqrt(Z gx1)
        const Fe<P> zg = fe_mul(K.z, fe_sqrt_gpow<P>(h_sqrt_table<P>(), 0));
        ok = h_sqrt(zg, K.c) && fe_eq(fe_sqr(K.c), zg);
    }
};
template <class C>
inline const H2cHost<C>& h2c_host() {
    static const H2cHost<C> v;
    return v;
}

}  // namespace bzh
