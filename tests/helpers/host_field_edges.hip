// Test program (not product code): the host twins of csrc/field.cuh on operands chosen by the test.
//   host_field_edges <field id 0..3> <in> <out>
// <in> holds n pairs (a, b) of 8 x 32-bit little-endian limbs (64 bytes a pair); <out> receives, per pair, fe_add(a, b),
// fe_sub(a, b), fe_neg(a), fe_mul(a, b) (128 bytes).  Built once as is (64-bit-limb product) and once with
// -DBZH_NO_HOST_MUL64 (32-bit CIOS); tests/test_host_field_cpu.py compares every result with Python integers.
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "field.cuh"
using namespace bzh;

template <class P>
static void run(const std::vector<uint32_t>& in, std::vector<uint32_t>& out) {
    const size_t n = in.size() / 16;
    out.resize(n * 32);
    for (size_t i = 0; i < n; i++) {
        Fe<P> a, b;
        memcpy(a.l, &in[i * 16], 32);
        memcpy(b.l, &in[i * 16 + 8], 32);
        const Fe<P> r[4] = {fe_add(a, b), fe_sub(a, b), fe_neg(a), fe_mul(a, b)};
        for (int k = 0; k < 4; k++) memcpy(&out[i * 32 + k * 8], r[k].l, 32);
    }
}

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    FILE* f = fopen(argv[2], "rb");
    if (!f) return 3;
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    if (bytes < 0 || bytes % 64) return 4;
    std::vector<uint32_t> in(bytes / 4), out;
    if (bytes && fread(in.data(), 1, bytes, f) != (size_t)bytes) return 5;
    fclose(f);
    switch (atoi(argv[1])) {
        case 0: run<FpParams>(in, out); break;
        case 1: run<FqParams>(in, out); break;
        case 2: run<BnFrParams>(in, out); break;
        case 3: run<BnFqParams>(in, out); break;
        default: return 6;
    }
    f = fopen(argv[3], "wb");
    if (!f) return 7;
    if (!out.empty() && fwrite(out.data(), 4, out.size(), f) != out.size()) return 8;
    fclose(f);
#if defined(BZH_HOST_MUL64)
    printf("64-bit limbs\n");
#else
    printf("32-bit limbs\n");
#endif
    return 0;
}
