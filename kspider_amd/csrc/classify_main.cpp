// `classify INPUT K SCALED DB OUT_PREFIX THREADS [--min-hits M]` — every read or contig of FASTA / FASTQ input against a sketch
// database (kspider_classify): INPUT is one file or a directory of .fa .fasta .fna .fq .fastq files (plain or .gz), every record a
// unit; DB is a directory of .sig files or a pack file.  Writes OUT_PREFIX_kSpider_classify.tsv (one row per record) and
// OUT_PREFIX_kSpider_classify_hits.tsv (one row per record and reference with at least M shared hashes; M defaults to 1).
// KSPIDER_CLASSIFY=host: no GPU.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/kspider_amd.h"

static bool number(const char* text, const unsigned long long most, unsigned long long* out) {
    char* end = nullptr;
    if (*text == '-') return false;
    const unsigned long long v = std::strtoull(text, &end, 10);
    if (end == text || *end || v > most) return false;
    *out = v;
    return true;
}

int main(int argc, char** argv) {
    unsigned long long k = 0, scaled = 0, threads = 0, min_hits = 1;
    bool ok = argc >= 7;
    for (int i = 7; ok && i < argc; ++i) {
        if (std::strcmp(argv[i], "--min-hits") == 0 && i + 1 < argc && number(argv[i + 1], 0xFFFFFFFFull, &min_hits)) ++i;
        else ok = false;
    }
    if (!ok) {
        std::fprintf(stderr, "usage: %s INPUT K SCALED DB OUT_PREFIX THREADS [--min-hits M]\n", argv[0]);
        return 2;
    }
    if (!number(argv[2], 64, &k) || !number(argv[3], ~0ull, &scaled) || !number(argv[6], 1000000, &threads)) {
        std::fprintf(stderr, "classify: K, SCALED and THREADS are numbers\n");
        return 2;
    }
    const int rc = kspider_classify(argv[1], (int)k, scaled, argv[4], argv[5], (int)threads, (unsigned)min_hits);
    if (rc != KSP_OK) {
        std::fprintf(stderr, "classify: %s\n", ksp_last_error());
        return 1;
    }
    return 0;
}
