// The two scalar lane bodies of the grand products on device-resident transcripts (bzh_grand_products_batch_device), as
// host/device functions: what csrc/products.hip's k_gp_finish runs is what tests/helpers/products_scalars_check.hip runs on the
// host against fe_mul (csrc/host_field.hpp).  `raw` is the scanned buffer [product][proof][row], Montgomery: the exclusive
// running product of each product's factors on its own, permutation sets first, then lookups.
//   gp_carry_lane    what upstream chains the permutation sets through: set i starts from the previous set's z[usable], and that
//                    chaining is linear, so z_i = raw_i * carry_i with carry_i = prod_{j < i} raw_j[usable] -- at most nsets - 1
//                    products, formed once per workgroup; 1 for set 0 and for a lookup
//   gp_status_lane   bit 0 of a proof's status: the last permutation set's z[usable] = prod_{j < nsets} raw_j[usable] is not 1, or a
//                    lookup's raw[usable] is not 1 -- a copy constraint or a lookup of that witness does not hold
// The trip counts depend on the key alone (nsets, nl), never on a lane's data; a zero raw_j[usable] (a zero denominator upstream
// of it) makes the carry zero like upstream's last_z, and the status bit is then set.
#pragma once
#include "ipa_scalars.hpp"

namespace bzh {

// one column of a product as k_gp_factors reads it: the column table of a call, built on the host from the key
struct GpCol {
    const uint32_t* v;       // the column's values over the domain, proof 0
    uint64_t stride;         // elements between proofs; 0: a fixed column of the key
    const uint32_t* sigma;   // pk.sigma / pk.ident rows of a permutation column; null for a lookup's columns
    const uint32_t* ident;
};
// product p reads table entries [first, first + count): the columns of its chunk for a permutation set; a_c, s_c, a, s for a lookup
struct GpProd {
    uint32_t first, count;
};

// prod_{j < count} raw_j[usable] of proof b
template <class P>
BZH_HD Fe<P> gp_chain(const void* raw, size_t batch, size_t n, size_t usable, size_t b, size_t count) {
    Fe<P> acc = fe_one<P>();
    for (size_t j = 0; j < count; j++) acc = fe_mul(acc, ipa_at<P>(raw, (j * batch + b) * n + usable));
    return acc;
}

template <class P>
BZH_HD Fe<P> gp_carry_lane(const void* raw, size_t batch, size_t n, size_t usable, size_t p, size_t b, size_t nsets) {
    return gp_chain<P>(raw, batch, n, usable, b, p < nsets ? p : 0);
}

template <class P>
BZH_HD uint8_t gp_status_lane(const void* raw, size_t batch, size_t n, size_t usable, size_t b, size_t nsets, size_t nl) {
    const Fe<P> one = fe_one<P>();
    bool open = !fe_eq(gp_chain<P>(raw, batch, n, usable, b, nsets), one);   // (no permutation: the empty product)
    for (size_t l = 0; l < nl; l++) open |= !fe_eq(ipa_at<P>(raw, ((nsets + l) * batch + b) * n + usable), one);
    return open ? 1 : 0;
}

}  // namespace bzh
