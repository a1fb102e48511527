// TEST HELPER (stand-alone host program, no GPU): the reader and the writer of the verifying key's "BZV1" bytes -- csrc/verifying_key.hpp
// over csrc/key_shape.hpp, the code libbzh2.so runs -- replaying a file of well-formed and hostile inputs, each copied into an
// exact-size heap buffer so that a read past its end is caught.  tests/test_vk_cpu.py builds it with the host's address and
// undefined-behaviour sanitizers and runs it.  File: per case i32 expectation, u32 length, bytes (tests/helpers/vk_cases.py).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <vector>

#include "host_field.hpp"
#define BZH_TRY(expr)          \
    do {                       \
        int rc__ = (expr);     \
        if (rc__) return rc__; \
    } while (0)
namespace bzh {
namespace {
#include "key_shape.hpp"
#include "verifying_key.hpp"
}  // namespace
}  // namespace bzh

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int bad = 0;
    size_t cases = 0, accepted = 0;
    for (;;) {
        int32_t expect;
        uint32_t len;
        if (fread(&expect, 4, 1, f) != 1 || fread(&len, 4, 1, f) != 1) break;
        uint8_t* buf = (uint8_t*)malloc(len ? len : 1);
        if (len && fread(buf, 1, len, f) != len) return 2;
        cases++;
        bzh_vk* vk = nullptr;
        const int rc = bzh_vk_read(buf, len, &vk);
        bool ok;
        if (rc == BZH_OK) {
            // a key that was accepted writes the bytes it was read from, the size query agrees, a short buffer is refused
            size_t n = 0;
            ok = vk && bzh_vk_write(vk, nullptr, 0, &n) == BZH_OK && n == len;
            if (ok) {
                uint8_t* out = (uint8_t*)malloc(n);
                memset(out, 0x5a, n);
                size_t m = 0;
                ok = bzh_vk_write(vk, out, n - 1, &m) == BZH_E_ARG && out[0] == 0x5a && out[n - 2] == 0x5a;
                ok = ok && bzh_vk_write(vk, out, n, &m) == BZH_OK && m == n && memcmp(out, buf, n) == 0;
                free(out);
            }
            ok = ok && (expect == 1 || expect == 2);
            accepted++;
            bzh_vk_free(vk);
        } else {
            ok = !vk && rc < 0 && (expect == 0 || expect == 2 || rc == expect);
        }
        if (!ok) {
            printf("FAIL case %zu (length %u): status %d, expected %d\n", cases, len, rc, expect);
            bad++;
        }
        free(buf);
    }
    fclose(f);
    if (bad || !cases) return 1;
    printf("%zu cases, %zu accepted\nvk_check: ok\n", cases, accepted);
    return 0;
}
