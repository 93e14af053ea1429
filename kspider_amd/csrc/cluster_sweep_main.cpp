// `cluster_sweep PREFIX DIST C1 [C2 ...]` — `kSpider cluster -i PREFIX -d DIST -c C` at every cut-off of the list from one
// reading of the pairwise TSV and one pass on the device (kspider_cluster_sweep; DIST min_cont, avg_cont, max_cont or ani).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/kspider_amd.h"

int main(int argc, char** argv) {
    if (argc < 4) {
        std::fprintf(stderr, "usage: %s INDEX_PREFIX DIST CUTOFF [CUTOFF ...]\n", argv[0]);
        return 2;
    }
    std::vector<double> cutoffs;
    for (int i = 3; i < argc; ++i) {
        char* end = nullptr;
        cutoffs.push_back(std::strtod(argv[i], &end));
        if (end == argv[i] || *end) {
            std::fprintf(stderr, "cluster_sweep: '%s' is not a cut-off\n", argv[i]);
            return 2;
        }
    }
    if (kspider_cluster_sweep(argv[1], argv[2], cutoffs.data(), (uint32_t)cutoffs.size()) != KSP_OK) {
        std::fprintf(stderr, "cluster_sweep: %s\n", ksp_last_error());
        return 1;
    }
    return 0;
}
