// `gather DB QUERIES K OUT_PREFIX THREADS MIN_HASHES [--max-matches M] [--abund]` — what every query is made of (kspider_gather): DB and QUERIES
// are each a pack file or a directory of .sig / .gz files (K > 0) or .bin files (K = 0); a database source is reported while it
// still covers MIN_HASHES hashes of what is left of the query; M caps the rows per query (0: no cap).  --abund (kspider_gather_abund):
// QUERIES is a directory of signatures with abundances, and the rows also say how much of the sample's weight a match takes.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/kspider_amd.h"

static bool number(const char* text, const long long max, long long* out) {
    char* end = nullptr;
    const long long v = std::strtoll(text, &end, 10);
    if (end == text || *end || v < 0 || v > max) return false;
    *out = v;
    return true;
}

int main(int argc, char** argv) {
    const bool abund = argc > 7 && std::strcmp(argv[argc - 1], "--abund") == 0;
    if (abund) --argc;
    const bool capped = argc == 9 && std::strcmp(argv[7], "--max-matches") == 0;
    long long k = 0, threads = 0, min_hashes = 0, max_matches = 0;
    if (argc != 7 && !capped) {
        std::fprintf(stderr, "usage: %s DB QUERIES K OUT_PREFIX THREADS MIN_HASHES [--max-matches M] [--abund]\n", argv[0]);
        return 2;
    }
    if (!number(argv[3], 1000000, &k) || !number(argv[5], 1000000, &threads) || !number(argv[6], 0xFFFFFFFFll, &min_hashes) ||
        (capped && !number(argv[8], 0xFFFFFFFFll, &max_matches))) {
        std::fprintf(stderr, "gather: K, THREADS, MIN_HASHES and M are numbers\n");
        return 2;
    }
    const int rc = (abund ? kspider_gather_abund : kspider_gather)(argv[1], argv[2], (int)k, argv[4], (int)threads, (uint32_t)min_hashes, (uint32_t)max_matches);
    if (rc != KSP_OK) {
        std::fprintf(stderr, "gather: %s\n", ksp_last_error());
        return 1;
    }
    return 0;
}
