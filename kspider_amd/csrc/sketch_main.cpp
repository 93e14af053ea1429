// `sketch INPUT K SCALED OUT_DIR THREADS [--per-record] [--seed S] [--abund] [--protein | --dayhoff | --hp] [--translate]` —
// sourmash-compatible FracMinHash sketches of FASTA / FASTQ files (kspider_sketch): INPUT is a directory, each of its .fa .fasta
// .fna .fq .fastq files (plain or .gz) one source, or one file; --per-record makes every record of that file a source; --abund
// writes every hash's abundance ("abundances").  --protein, --dayhoff, --hp: K is the residue k and INPUT is protein (a directory's
// .faa .fa .fasta files), or with --translate DNA read in six frames (K <= 21); the signatures say "ksize": 3 K.  Writes
// OUT_DIR/<name>.sig.  KSPIDER_SKETCH=host: no GPU.
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
    unsigned long long k = 0, scaled = 0, threads = 0, seed = 0, flags = 0;
    bool ok = argc >= 6;
    for (int i = 6; ok && i < argc; ++i) {
        if (std::strcmp(argv[i], "--per-record") == 0) flags |= KSP_SKETCH_PER_RECORD;
        else if (std::strcmp(argv[i], "--abund") == 0) flags |= KSP_SKETCH_ABUND;
        else if (std::strcmp(argv[i], "--protein") == 0) flags |= KSP_SKETCH_PROTEIN;
        else if (std::strcmp(argv[i], "--dayhoff") == 0) flags |= KSP_SKETCH_DAYHOFF;
        else if (std::strcmp(argv[i], "--hp") == 0) flags |= KSP_SKETCH_HP;
        else if (std::strcmp(argv[i], "--translate") == 0) flags |= KSP_SKETCH_TRANSLATE;
        else if (std::strcmp(argv[i], "--seed") == 0 && i + 1 < argc && number(argv[i + 1], 0xFFFFFFFFull, &seed)) { flags |= KSP_SKETCH_SEED; ++i; }
        else ok = false;
    }
    if (!ok) {
        std::fprintf(stderr, "usage: %s INPUT K SCALED OUT_DIR THREADS [--per-record] [--seed S] [--abund] [--protein | --dayhoff | --hp] [--translate]\n", argv[0]);
        return 2;
    }
    if (!number(argv[2], 64, &k) || !number(argv[3], ~0ull, &scaled) || !number(argv[5], 1000000, &threads)) {
        std::fprintf(stderr, "sketch: K, SCALED and THREADS are numbers\n");
        return 2;
    }
    const int rc = kspider_sketch(argv[1], (int)k, scaled, argv[4], (int)threads, flags | (seed << 32));
    if (rc != KSP_OK) {
        std::fprintf(stderr, "sketch: %s\n", ksp_last_error());
        return 1;
    }
    return 0;
}
