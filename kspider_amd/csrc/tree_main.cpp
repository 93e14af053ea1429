// `cluster_tree PREFIX DIST [--newick] [--cut C ...]` — the single-linkage tree of the pairwise TSV (kspider_tree; DIST min_cont,
// avg_cont, max_cont or ani), then `kSpider cluster -i PREFIX -d DIST -c C` for every --cut, from the tree file alone
// (kspider_cluster_from_tree).
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
                std::fprintf(stderr, "cluster_tree: '%s' is not a cut-off\n", argv[i]);
                return 2;
            }
        } else {
            std::fprintf(stderr, "cluster_tree: unknown argument '%s'\n", argv[i]);
            return 2;
        }
    }
    if (kspider_tree(argv[1], argv[2], newick) != KSP_OK) {
        std::fprintf(stderr, "cluster_tree: %s\n", ksp_last_error());
        return 1;
    }
    for (const double c : cuts)
        if (kspider_cluster_from_tree(argv[1], argv[2], c) != KSP_OK) {
            std::fprintf(stderr, "cluster_tree: %s\n", ksp_last_error());
            return 1;
        }
    return 0;
}
