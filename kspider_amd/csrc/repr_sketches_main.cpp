// `repr_sketches PAIRWISE_TSV` — same command line as the reference's tool (apps/repr_sketches.cpp, CMake target
// `repr_sketches`): "id: count" lines on stdout, ids ranked by their number of neighbours with avg_containment > 0.20.
#include <cstdio>

#include "../../include/kspider_amd.h"

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s PAIRWISE_TSV\n", argv[0]);
        return 2;
    }
    if (kspider_repr_sketches(argv[1], nullptr, 0.20, nullptr) != KSP_OK) {
        std::fprintf(stderr, "repr_sketches: %s\n", ksp_last_error());
        return 1;
    }
    return 0;
}
