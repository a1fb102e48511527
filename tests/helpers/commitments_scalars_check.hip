// TEST HELPER (stand-alone host program, no GPU): the lane bodies of csrc/commitments_scalars.hpp -- what k_cm_consts runs once
// per (proof, constant) (cm_const_lane) and k_cm_lookup_finish once per proof (cm_status_lane) for bzh_commitments_batch_device --
// lane by lane over exact-size heap buffers, against values tests/test_commitments_device_cpu.py computes and hands over in a
// text file of unsigned decimal words (argv[1]).  A case:
//   "consts" field batch canonical ntables | per table: nconsts per_proof | ndescs | per descriptor: table sym index value[8] |
//   theta[batch][8] | per table: the expected rows x nconsts x 8 words
//   "status" nl batch | words[batch * nl] | expected[batch]
// The test builds it with the host's address and undefined-behaviour sanitizers and runs it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "host_field.hpp"
#include "commitments_scalars.hpp"
using namespace bzh;

static FILE* in;
static unsigned long rd() {
    unsigned long v = 0;
    if (fscanf(in, "%lu", &v) != 1) {
        printf("commitments_scalars_check: short input\n");
        exit(2);
    }
    return v;
}

template <class P>
static int consts_case(size_t batch, bool canonical, size_t* lanes) {
    const size_t ntables = rd();
    std::vector<size_t> nc(ntables), rows(ntables);
    std::vector<uint32_t*> tables(ntables);
    std::vector<uint32_t> per_proof(ntables);
    for (size_t t = 0; t < ntables; t++) {
        nc[t] = rd();
        per_proof[t] = rd() ? 1u : 0u;
        rows[t] = per_proof[t] ? batch : 1;
        tables[t] = (uint32_t*)malloc(rows[t] * nc[t] * 32);   // exact size: a lane that writes past its table is caught
        memset(tables[t], 0xa5, rows[t] * nc[t] * 32);
    }
    const size_t nd = rd();
    CmConst* descs = (CmConst*)malloc(nd * sizeof(CmConst));
    for (size_t e = 0; e < nd; e++) {
        const size_t t = rd();
        descs[e].table = tables[t], descs[e].nconsts = (uint32_t)nc[t], descs[e].per_proof = per_proof[t];
        descs[e].sym = rd() ? 0 : -1;
        descs[e].index = (uint32_t)rd();
        for (int w = 0; w < 8; w++) descs[e].value[w] = (uint32_t)rd();
    }
    uint32_t* theta = (uint32_t*)malloc(batch * 32);
    for (size_t i = 0; i < batch * 8; i++) theta[i] = (uint32_t)rd();
    for (size_t g = 0; g < nd * batch; g++, ++*lanes) cm_const_lane<P>(g, descs, nd, theta, canonical);
    int bad = 0;
    for (size_t t = 0; t < ntables; t++) {
        for (size_t i = 0; i < rows[t] * nc[t] * 8; i++)
            if (tables[t][i] != (uint32_t)rd()) bad = 1;
        free(tables[t]);
    }
    free(descs);
    free(theta);
    return bad;
}

static int status_case(size_t* lanes) {
    const size_t nl = rd(), batch = rd();
    int32_t* words = (int32_t*)malloc((batch * nl ? batch * nl : 1) * sizeof(int32_t));
    for (size_t i = 0; i < batch * nl; i++) words[i] = (int32_t)(uint32_t)rd();
    int bad = 0;
    for (size_t b = 0; b < batch; b++, ++*lanes)
        if (cm_status_lane(words, nl, b) != (uint8_t)rd()) bad = 1;
    free(words);
    return bad;
}

int main(int argc, char** argv) {
    if (argc < 2 || !(in = fopen(argv[1], "r"))) return 2;
    int bad = 0, cases = 0;
    size_t lanes = 0;
    char kind[16];
    while (fscanf(in, "%15s", kind) == 1) {
        int rc;
        if (!strcmp(kind, "consts")) {
            const size_t field = rd(), batch = rd(), canonical = rd();
            rc = field == 0 ? consts_case<FpParams>(batch, canonical != 0, &lanes) : consts_case<FqParams>(batch, canonical != 0, &lanes);
        } else {
            rc = status_case(&lanes);
        }
        if (rc) printf("FAIL case %d (%s)\n", cases, kind);
        bad |= rc;
        cases++;
    }
    fclose(in);
    printf("%d cases, %zu lanes\n", cases, lanes);
    printf(bad ? "commitments_scalars_check: FAILED\n" : "commitments_scalars_check: ok\n");
    return bad ? 1 : 0;
}
