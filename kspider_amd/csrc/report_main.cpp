// `cluster_report PREFIX DIST CUTOFF` — the report of every cluster of the pairwise TSV at one cut-off (kspider_cluster_report;
// DIST min_cont, avg_cont or max_cont): PREFIX_kSpider_cluster_report_<DIST>_<CUTOFF*100>%.tsv and
// PREFIX_kSpider_cluster_members_<DIST>_<CUTOFF*100>%.tsv.
#include <cstdio>
#include <cstdlib>

#include "../../include/kspider_amd.h"

int main(int argc, char** argv) {
    if (argc != 4) {
        std::fprintf(stderr, "usage: %s INDEX_PREFIX DIST CUTOFF\n", argv[0]);
        return 2;
    }
    char* end = nullptr;
    const double cutoff = std::strtod(argv[3], &end);
    if (end == argv[3] || *end) {
        std::fprintf(stderr, "cluster_report: '%s' is not a cut-off\n", argv[3]);
        return 2;
    }
    if (kspider_cluster_report(argv[1], argv[2], cutoff) != KSP_OK) {
        std::fprintf(stderr, "cluster_report: %s\n", ksp_last_error());
        return 1;
    }
    return 0;
}
