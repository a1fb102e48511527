// The byte layout of halo2_proofs 0.2.0's Params::write / Params::read (src/poly/commitment.rs), in ONE place:
//     k as a u32, little-endian | n = 2^k points of g | n points of g_lagrange | w | u
// every point the 32-byte GroupEncoding::to_bytes string (x little-endian, bit 255 = parity of y).  4 + 32 (2 n + 2) bytes.
// The order is stated from upstream's source as remembered; it has NOT been checked against a file that Rust wrote.  Every reader
// and writer of the format (bzh_params_file_info, bzh_params_encode, bzh_params_write, bzh_params_read, k_pf_verdict) takes
// offsets and lane numbers from the functions below, so another field order is a change of pf_order()'s one line.
//
// Point number `lane` of a file is its position among the 2 n + 2 strings.  The verdict's section codes -- 0 g, 1 g_lagrange,
// 2 w, 3 u -- are the C ABI's (bzh_params_verdict) and do not move with the file order.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define BZH_PF_HD __host__ __device__ inline
#else
#define BZH_PF_HD inline
#endif

namespace bzh {

enum { PF_G = 0, PF_G_LAGRANGE = 1, PF_W = 2, PF_U = 3, kPfSections = 4 };
constexpr size_t kPfHeaderBytes = 4, kPfPointBytes = 32;
constexpr unsigned kPfMaxK = 24;   // what bzh_params_generators and bzh_params_create take

// the section at position `pos` of the file
BZH_PF_HD constexpr int pf_order(int pos) { return pos == 0 ? PF_G : pos == 1 ? PF_G_LAGRANGE : pos == 2 ? PF_W : PF_U; }

BZH_PF_HD constexpr size_t pf_section_len(int section, size_t n) { return section == PF_G || section == PF_G_LAGRANGE ? n : 1; }
BZH_PF_HD constexpr size_t pf_points(size_t n) { return 2 * n + 2; }
BZH_PF_HD constexpr size_t pf_file_bytes(size_t n) { return kPfHeaderBytes + kPfPointBytes * pf_points(n); }
// the lane of a section's first point
BZH_PF_HD constexpr size_t pf_first_lane(int section, size_t n) {
    size_t at = 0;
    for (int pos = 0; pos < kPfSections; pos++) {
        if (pf_order(pos) == section) return at;
        at += pf_section_len(pf_order(pos), n);
    }
    return at;
}
BZH_PF_HD constexpr size_t pf_offset(int section, size_t index, size_t n) {
    return kPfHeaderBytes + kPfPointBytes * (pf_first_lane(section, n) + index);
}
// lane < 2 n + 2 -> its section and its index there
BZH_PF_HD void pf_lane_section(size_t lane, size_t n, uint32_t* section, uint32_t* index) {
    size_t at = 0;
    for (int pos = 0; pos < kPfSections; pos++) {
        const size_t len = pf_section_len(pf_order(pos), n);
        if (lane < at + len || pos == kPfSections - 1) {
            *section = (uint32_t)pf_order(pos);
            *index = (uint32_t)(lane - at);
            return;
        }
        at += len;
    }
}

}  // namespace bzh

struct bzh_ctx;
namespace bzh {
// csrc/params_file.hip: k_pf_verdict's launch.  Device pointers, 16-byte aligned; enqueues only, the caller holds ctx->mu.
//   d_status   2 n + 2 BZH_POINT_* bytes, one per string of the file, as decompress_run leaves them
//   d_points   the 2 n + 2 decoded points, affine Montgomery (zeros where the status is not BZH_POINT_OK)
//   d_gen, d_gen_status   Params::new's g as h2c_generators_run leaves it (n points, n bytes), and
//   d_wu       Params::new's w then u, affine Montgomery: all three null unless the generators are checked
//   d_sums     two Jacobian points, Montgomery: sum_j r_j g_lagrange[j], then sum_i intt(r)_i g[i]; null unless they are compared
//   d_acc      eight words of scratch, zeroed by the launch function
//   d_verdict  the 16-byte bzh_params_verdict
struct PfVerdictArgs {
    const uint8_t* d_status = nullptr;
    const uint32_t* d_points = nullptr;
    const uint32_t* d_gen = nullptr;
    const uint8_t* d_gen_status = nullptr;
    const uint32_t* d_wu = nullptr;
    const uint32_t* d_sums = nullptr;
    uint32_t* d_acc = nullptr;
    uint32_t* d_verdict = nullptr;
    uint32_t n = 0;
};
int params_file_verdict_run(bzh_ctx* ctx, const PfVerdictArgs& a);
}  // namespace bzh
