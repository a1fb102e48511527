// halo2_proofs 0.2.0's transcript::{Blake2bWrite, Challenge255} for `batch` proofs in lockstep, as host/device functions: what
// csrc/transcript_batch.hip's kernels run one lane per transcript is what its host path (ctx == NULL) runs in a loop over the
// transcripts.  csrc/transcript.hip (one host object per proof, csrc/blake2b.hpp) is separate code and stays the comparator.
//   tb_put            `len` bytes, given as little-endian words, into the block buffer at the byte position `buflen`, with
//                     blake2b.hpp's lazy rule: a full buffer is compressed only when more input follows
//   tb_absorb_point   0x01 || x || y (65 bytes) from an affine point in `form`, its 32 proof bytes and a BZH_POINT_* byte
//   tb_absorb_scalar  0x02 || repr (33 bytes) from a scalar in `form`, and its 32 proof bytes
//   tb_squeeze        absorbs 0x00, finalises a COPY of the state and reduces the digest as a 512-bit little-endian integer
//
// One transcript is h[8], the 128-byte block buffer and one sticky status byte.  The bytes compressed so far (t), the buffer fill
// (buflen) and the proof length are the same for every transcript of a batch at all times -- every operation gives every
// transcript the same number of items --, so they live in the handle on the host, reach the kernels as plain arguments and
// make the control flow uniform; tb_advance is how the host keeps them in step.
//
// The buffer is kept in memory (TbState, word w of transcript b at buf[w * batch + b]: a wave's lanes touch neighbouring
// words), zero past buflen at all times.  An item is built in registers as whole words, shifted by the uniform buflen % 8 with
// funnel shifts and stored at the uniform word offset buflen / 8; only memory is indexed with a runtime value, never a register
// array.  A compression loads the sixteen words back with constant indices (b2_compress, twelve rounds unrolled).
#pragma once
#include "normalize.hpp"

namespace bzh {

struct TbState {
    uint64_t* h;       // 8 x batch words
    uint64_t* buf;     // 16 x batch words, zero past buflen
    uint8_t* status;   // batch bytes, the maximum BZH_POINT_* seen
    uint8_t* proofs;   // batch rows of pstride bytes (a multiple of 32)
    size_t batch, pstride;
};

// the uniform counters after `len` more bytes: what tb_put does to its own copies
inline void tb_advance(uint64_t& t, uint32_t& buflen, uint32_t len) {
    if (!len) return;
    const uint32_t end = buflen + len;
    if (end > 128) {
        t += 128;
        buflen = end - 128;
    } else {
        buflen = end;
    }
}

BZH_HD void tb_load_h(const TbState& S, size_t b, uint64_t (&h)[8]) {
#pragma unroll
    for (int i = 0; i < 8; i++) h[i] = S.h[i * S.batch + b];
}
BZH_HD void tb_store_h(const TbState& S, size_t b, const uint64_t (&h)[8]) {
#pragma unroll
    for (int i = 0; i < 8; i++) S.h[i * S.batch + b] = h[i];
}
BZH_HD void tb_compress_buf(const TbState& S, size_t b, uint64_t (&h)[8], uint64_t t, bool last) {
    uint64_t m[16];
#pragma unroll
    for (int w = 0; w < 16; w++) m[w] = S.buf[w * S.batch + b];
    b2_compress(h, m, t, last);
}

// it: the item's bytes as NW little-endian words, zero past `len` (0 < len <= 8 * NW - 7, so the shifted item fits NW words).
// buflen <= 128 on entry and on exit.  A buffer that is full on entry is the general case with word offset 16: the whole item
// goes to the next block.
template <int NW>
BZH_HD void tb_put(const TbState& S, size_t b, uint64_t (&h)[8], const uint64_t (&it)[NW], uint32_t len, uint64_t& t, uint32_t& buflen) {
    const uint32_t sh = 8 * (buflen & 7), wo = buflen >> 3;
    uint64_t s[NW];
    s[0] = it[0] << sh;
#pragma unroll
    for (int j = 1; j < NW; j++) s[j] = (it[j] << sh) | (sh ? it[j - 1] >> (64 - sh) : 0);
    uint64_t* const buf = S.buf + b;
    if (wo < 16) buf[wo * S.batch] |= s[0];
#pragma unroll
    for (int j = 1; j < NW; j++)
        if (wo + j < 16) buf[(wo + j) * S.batch] = s[j];
    const uint32_t end = buflen + len;
    if (end > 128) {   // the buffer is full and more input follows: not the last block
        t += 128;
        tb_compress_buf(S, b, h, t, false);
#pragma unroll
        for (int w = 0; w < 16; w++) buf[w * S.batch] = 0;
#pragma unroll
        for (int j = 0; j < NW; j++)
            if (wo + j >= 16) buf[(wo + j - 16) * S.batch] = s[j];
        buflen = end - 128;
    } else {
        buflen = end;
    }
}

// tag || v[0 .. NV) as words: NV + 1 of them, the last holds one byte
template <int NV>
BZH_HD void tb_tagged(uint64_t tag, const uint64_t (&v)[NV], uint64_t (&it)[NV + 1]) {
    it[0] = tag | (v[0] << 8);
#pragma unroll
    for (int k = 1; k < NV; k++) it[k] = (v[k - 1] >> 56) | (v[k] << 8);
    it[NV] = v[NV - 1] >> 56;
}
template <class P>
BZH_HD void tb_words(const Fe<P>& a, uint64_t* v) {
#pragma unroll
    for (int k = 0; k < 4; k++) v[k] = (uint64_t)a.l[2 * k] | ((uint64_t)a.l[2 * k + 1] << 32);
}
// the canonical value of an operand in `form`; false (and zero) for a canonical operand that is not below the modulus
template <class P>
BZH_HD bool tb_canonical(const Fe<P>& a, bool canonical, Fe<P>& out) {
    const bool ok = !canonical || fe_lt_p(a);
    out = fe_csel(ok, canonical ? a : fe_from_mont(a), fe_zero<P>());
    return ok;
}
BZH_HD void tb_mark(const TbState& S, size_t b, uint8_t st) {
    if (st > S.status[b]) S.status[b] = st;
}

// xy: 64 bytes x || y in `form` (base field).  pre: a BZH_POINT_* byte the point already carries (bzh_batch_normalize's), or
// BZH_POINT_OK.  (0, 0) is hashed as 64 zero bytes and marked BZH_POINT_IDENTITY; an operand that is not below p is hashed as
// zeros and marked BZH_POINT_INVALID.  proof32: where the to_bytes encoding goes, or null (common_point).
template <class C>
BZH_HD void tb_absorb_point(const TbState& S, size_t b, uint64_t (&h)[8], const void* xy, bool canonical, uint8_t pre, void* proof32,
                            uint64_t& t, uint32_t& buflen) {
    using P = typename C::Base;
    Fe<P> x, y;
    const bool okx = tb_canonical(norm_load<P>(xy), canonical, x), oky = tb_canonical(norm_load<P>((const char*)xy + 32), canonical, y);
    const bool ok = okx && oky;
    x = fe_csel(ok, x, fe_zero<P>());
    y = fe_csel(ok, y, fe_zero<P>());
    const uint8_t st = !ok ? (uint8_t)BZH_POINT_INVALID : ((fe_is_zero(x) && fe_is_zero(y)) ? (uint8_t)BZH_POINT_IDENTITY : (uint8_t)BZH_POINT_OK);
    tb_mark(S, b, st > pre ? st : pre);
    uint64_t v[8], it[9];
    tb_words(x, v);
    tb_words(y, v + 4);
    tb_tagged<8>(1, v, it);
    tb_put<9>(S, b, h, it, 65, t, buflen);
    if (proof32) norm_store<P>(proof32, fe_point_encode(x, y));
}
// s: 32 bytes in `form` (scalar field); an operand that is not below the modulus is hashed as zeros and marked BZH_POINT_INVALID
template <class C>
BZH_HD void tb_absorb_scalar(const TbState& S, size_t b, uint64_t (&h)[8], const void* s, bool canonical, void* proof32, uint64_t& t,
                             uint32_t& buflen) {
    using P = typename CurveInfo<C>::SF;
    Fe<P> a;
    if (!tb_canonical(norm_load<P>(s), canonical, a)) tb_mark(S, b, (uint8_t)BZH_POINT_INVALID);
    uint64_t v[4], it[5];
    tb_words(a, v);
    tb_tagged<4>(2, v, it);
    tb_put<5>(S, b, h, it, 33, t, buflen);
    if (proof32) norm_store<P>(proof32, a);
}

// `count` items of transcript b: item i at base + (b * stride + i) * item bytes.  KIND: 0 common point, 1 write point,
// 2 common scalar, 3 write scalar; a write puts item i's 32 bytes at proof offset proof_len + 32 i.
template <class C, int KIND>
BZH_HD void tb_absorb(const TbState& S, size_t b, const void* base, size_t count, size_t stride, bool canonical, const uint8_t* pre,
                      uint64_t t, uint32_t buflen, size_t proof_len) {
    constexpr bool point = KIND < 2, write = (KIND & 1) != 0;
    constexpr size_t item = point ? 64 : 32;
    uint64_t h[8];
    tb_load_h(S, b, h);
#pragma unroll 1
    for (size_t i = 0; i < count; i++) {
        const size_t at = b * stride + i;
        const void* src = (const char*)base + at * item;
        void* out = write ? (void*)(S.proofs + b * S.pstride + proof_len + 32 * i) : nullptr;
        if constexpr (point)
            tb_absorb_point<C>(S, b, h, src, canonical, pre ? pre[at] : (uint8_t)BZH_POINT_OK, out, t, buflen);
        else
            tb_absorb_scalar<C>(S, b, h, src, canonical, out, t, buflen);
    }
    tb_store_h(S, b, h);
}

// squeeze_challenge: absorbs 0x00, then the digest of a copy of the state -- the buffer is zero past buflen, so it is the padded
// last block as it stands -- as lo + hi 2^256 mod the scalar field (lo R^2 + (hi R^2) R^2, as h_from_u512); 32 bytes in `form`
template <class C>
BZH_HD void tb_squeeze(const TbState& S, size_t b, uint64_t t, uint32_t buflen, bool canonical, void* out32) {
    using P = typename CurveInfo<C>::SF;
    uint64_t h[8];
    tb_load_h(S, b, h);
    const uint64_t zero[1] = {0};
    tb_put<1>(S, b, h, zero, 1, t, buflen);
    tb_store_h(S, b, h);
    tb_compress_buf(S, b, h, t + buflen, true);
    Fe<P> lo, hi;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        lo.l[2 * k] = (uint32_t)h[k], lo.l[2 * k + 1] = (uint32_t)(h[k] >> 32);
        hi.l[2 * k] = (uint32_t)h[4 + k], hi.l[2 * k + 1] = (uint32_t)(h[4 + k] >> 32);
    }
    const Fe<P> r2 = fe_r2<P>();
    const Fe<P> c = fe_add(fe_mul(lo, r2), fe_mul(fe_mul(hi, r2), r2));
    norm_store<P>(out32, canonical ? fe_from_mont(c) : c);
}

}  // namespace bzh
