// Driver of the sanitizer build (make asan): runs one host entry point on one input and prints its return code.
//   host_asan_check index PREFIX | info PREFIX | sigs DIR KSIZE OUTPREFIX | bins DIR OUTPREFIX
//                   | cut PREFIX DIST CUTOFF | edges_cut X | host_cut X   (the last two: the entry point with nothing to do)
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/kspider_amd.h"

int main(int argc, char** argv) {
    if (argc < 3) return 64;
    int rc = -1;
    if (!std::strcmp(argv[1], "index")) rc = kspider_pairwise(argv[2], 2);
    else if (!std::strcmp(argv[1], "info")) { uint64_t out[6]; rc = ksp_index_info(argv[2], out); if (!rc) std::printf("info %llu %llu %llu %llu %llu %llu\n", (unsigned long long)out[0], (unsigned long long)out[1], (unsigned long long)out[2], (unsigned long long)out[3], (unsigned long long)out[4], (unsigned long long)out[5]); }
    else if (!std::strcmp(argv[1], "sigs") && argc >= 5) rc = kspider_pairwise_sigs(argv[2], std::atoi(argv[3]), argv[4], 2);
    else if (!std::strcmp(argv[1], "bins") && argc >= 4) rc = kspider_pairwise_bins(argv[2], argv[3], 2);
    else if (!std::strcmp(argv[1], "cut") && argc >= 5) rc = kspider_pairwise_cut(argv[2], 2, argv[3], std::atof(argv[4]));
    else if (!std::strcmp(argv[1], "edges_cut")) { uint64_t kept = 0; rc = ksp_edges_cut(0, nullptr, 0, nullptr, 5, 0.5, nullptr, &kept); }
    else if (!std::strcmp(argv[1], "host_cut")) {
        const uint64_t offsets[1] = {0};
        const int device = 0;
        ksp_edge* out = nullptr;
        uint64_t n = 0, found = 0;
        rc = ksp_pairwise_host_cut(nullptr, nullptr, offsets, 0, nullptr, 5, 0.5, &device, 1, &out, &n, &found, nullptr);
    }
    std::printf("rc %d %s\n", rc, rc ? ksp_last_error() : "");
    return 0;
}
