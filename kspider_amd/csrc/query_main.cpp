// `query DB QUERIES K OUT_PREFIX THREADS [--self]` — the pairwise rows of new sketches against a database (kspider_query): DB and
// QUERIES are each a pack file or a directory of .sig / .gz files (K > 0) or .bin files (K = 0); --self adds the query x query rows.
// `query --pack DIR K OUT_FILE THREADS` — the directory's sketches as one pack file (kspider_pack).
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
    const bool pack = argc > 1 && std::strcmp(argv[1], "--pack") == 0;
    const bool self = !pack && argc == 7 && std::strcmp(argv[6], "--self") == 0;
    int k = 0, threads = 0;
    if (pack ? argc != 6 : (argc != 6 && !self)) {
        std::fprintf(stderr, "usage: %s DB QUERIES K OUT_PREFIX THREADS [--self]\n       %s --pack DIR K OUT_FILE THREADS\n", argv[0], argv[0]);
        return 2;
    }
    if (!number(argv[3], &k) || !number(argv[5], &threads)) {
        std::fprintf(stderr, "query: K and THREADS are numbers\n");
        return 2;
    }
    const int rc = pack ? kspider_pack(argv[2], k, argv[4], threads)
                        : kspider_query(argv[1], argv[2], k, argv[4], threads, self ? KSP_QUERY_CROSS_AND_SELF : KSP_QUERY_CROSS);
    if (rc != KSP_OK) {
        std::fprintf(stderr, "query: %s\n", ksp_last_error());
        return 1;
    }
    return 0;
}
