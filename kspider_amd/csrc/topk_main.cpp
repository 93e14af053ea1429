// `topk PREFIX DIST K [OUT]` — the K best hits of every source of the pairwise TSV (kspider_topk; DIST min_cont, avg_cont,
// max_cont or ani): PREFIX_kSpider_topk_<DIST>.tsv, or OUT.
#include <cstdio>
#include <cstdlib>

#include "../../include/kspider_amd.h"

int main(int argc, char** argv) {
    if (argc < 4 || argc > 5) {
        std::fprintf(stderr, "usage: %s INDEX_PREFIX DIST K [OUT]\n", argv[0]);
        return 2;
    }
    char* end = nullptr;
    const unsigned long long k = std::strtoull(argv[3], &end, 10);
    if (end == argv[3] || *end || argv[3][0] == '-' || k > 0xFFFFFFFFull) {
        std::fprintf(stderr, "topk: '%s' is not a number of hits\n", argv[3]);
        return 2;
    }
    if (kspider_topk(argv[1], argv[2], (uint32_t)k, argc > 4 ? argv[4] : nullptr) != KSP_OK) {
        std::fprintf(stderr, "topk: %s\n", ksp_last_error());
        return 1;
    }
    return 0;
}
