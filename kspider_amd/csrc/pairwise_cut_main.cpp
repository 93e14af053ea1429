// `pairwise_cut PREFIX THREADS DIST CUTOFF` — `pairwise PREFIX THREADS` with a minimum containment: the pairwise TSV holds
// only the rows `kSpider cluster -d DIST -c CUTOFF` would keep (kspider_pairwise_cut; DIST min_cont, avg_cont or max_cont).
#include <cstdio>
#include <cstdlib>

#include "../../include/kspider_amd.h"

int main(int argc, char** argv) {
    if (argc < 5) {
        std::fprintf(stderr, "usage: %s INDEX_PREFIX THREADS DIST CUTOFF\n", argv[0]);
        return 2;
    }
    char* end = nullptr;
    const double cutoff = std::strtod(argv[4], &end);
    if (end == argv[4] || *end) {
        std::fprintf(stderr, "pairwise_cut: '%s' is not a cut-off\n", argv[4]);
        return 2;
    }
    if (kspider_pairwise_cut(argv[1], std::atoi(argv[2]), argv[3], cutoff) != KSP_OK) {
        std::fprintf(stderr, "pairwise_cut: %s\n", ksp_last_error());
        return 1;
    }
    return 0;
}
