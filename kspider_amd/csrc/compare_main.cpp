// `compare SAMPLES K OUT_PREFIX THREADS [--against DB] [--matrix]` — cosine, angular similarity and weighted containment of
// counted sketches (kspider_compare): SAMPLES is a directory of .sig / .sig.gz files; without --against every pair of samples is
// compared and --matrix also writes the N x N angular similarities, with --against DB (a directory or a pack file) every database
// source against every sample.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/kspider_amd.h"

static bool number(const char* text, int* out) {
    char* end = nullptr;
    const long v = std::strtol(text, &end, 10);
    if (end == text || *end || v < 0 || v > 1000000) return false;
    *out = (int)v;
    return true;
}

int main(int argc, char** argv) {
    const char* against = nullptr;
    uint64_t flags = 0;
    bool usage = argc < 5;
    for (int i = 5; i < argc && !usage; ++i) {
        if (std::strcmp(argv[i], "--matrix") == 0) flags |= KSP_COMPARE_MATRIX;
        else if (std::strcmp(argv[i], "--against") == 0 && i + 1 < argc) against = argv[++i];
        else usage = true;
    }
    if (usage) {
        std::fprintf(stderr, "usage: %s SAMPLES K OUT_PREFIX THREADS [--against DB] [--matrix]\n", argv[0]);
        return 2;
    }
    int k = 0, threads = 0;
    if (!number(argv[2], &k) || !number(argv[4], &threads)) {
        std::fprintf(stderr, "compare: K and THREADS are numbers\n");
        return 2;
    }
    if (kspider_compare(argv[1], against, k, argv[3], threads, flags) != KSP_OK) {
        std::fprintf(stderr, "compare: %s\n", ksp_last_error());
        return 1;
    }
    return 0;
}
