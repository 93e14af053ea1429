// `cluster_upgma PREFIX DIST [--newick] [--cut C ...]` — the average-linkage tree (UPGMA) of the pairwise TSV (kspider_upgma; DIST
// min_cont, avg_cont or max_cont), then the clusters of every --cut, from the merge table alone (kspider_cluster_from_upgma):
// PREFIX_kSpider_clusters_upgma_<DIST>_<C*100>%.tsv.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/kspider_amd.h"

int main(int argc, char** argv) {
    if (argc < 3) {
        std::fprintf(stderr, "usage: %s INDEX_PREFIX DIST [--newick] [--cut CUTOFF ...]\n", argv[0]);
        return 2;
    }
    int newick = 0;
    std::vector<double> cuts;
    for (int i = 3; i < argc; ++i) {
        if (!std::strcmp(argv[i], "--newick")) {
            newick = 1;
        } else if (!std::strcmp(argv[i], "--cut") && i + 1 < argc) {
            char* end = nullptr;
            cuts.push_back(std::strtod(argv[++i], &end));
            if (end == argv[i] || *end) {
                std::fprintf(stderr, "cluster_upgma: '%s' is not a cut-off\n", argv[i]);
                return 2;
            }
        } else {
            std::fprintf(stderr, "cluster_upgma: unknown argument '%s'\n", argv[i]);
            return 2;
        }
    }
    if (kspider_upgma(argv[1], argv[2], newick) != KSP_OK) {
        std::fprintf(stderr, "cluster_upgma: %s\n", ksp_last_error());
        return 1;
    }
    for (const double c : cuts)
        if (kspider_cluster_from_upgma(argv[1], argv[2], c) != KSP_OK) {
            std::fprintf(stderr, "cluster_upgma: %s\n", ksp_last_error());
            return 1;
        }
    return 0;
}
