// `dereplicate PREFIX DIST THRESHOLD [OUT]` — the dereplicated set of the pairwise TSV (kspider_dereplicate; DIST min_cont,
// avg_cont or max_cont): PREFIX_kSpider_dereplicated_<DIST>.tsv, or OUT.
#include <cstdio>
#include <cstdlib>

#include "../../include/kspider_amd.h"

int main(int argc, char** argv) {
    if (argc < 4 || argc > 5) {
        std::fprintf(stderr, "usage: %s INDEX_PREFIX DIST THRESHOLD [OUT]\n", argv[0]);
        return 2;
    }
    char* end = nullptr;
    const double threshold = std::strtod(argv[3], &end);
    if (end == argv[3] || *end) {
        std::fprintf(stderr, "dereplicate: '%s' is not a threshold\n", argv[3]);
        return 2;
    }
    if (kspider_dereplicate(argv[1], argv[2], threshold, argc > 4 ? argv[4] : nullptr) != KSP_OK) {
        std::fprintf(stderr, "dereplicate: %s\n", ksp_last_error());
        return 1;
    }
    return 0;
}
