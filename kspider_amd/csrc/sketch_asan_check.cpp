// Driver of the sketcher's sanitizer build (make asan-sketch): the host code of fastx_reader.cpp, sketch_files.cpp and
// sketch_cpu.cpp under -fsanitize=address,undefined, linked with the stub instead of the HIP engine.
//   sketch_asan_check read FILE...               every file through ksp_fastx_info and, when that accepts it, ksp_fastx_load into
//                                                buffers of exactly the reported sizes: one line "<rc> <file>" per file
//   sketch_asan_check sketch INPUT K SCALED OUT [--per-record]
//                                                kspider_sketch in host mode with 2 threads (set KSPIDER_SKETCH_BATCH_BYTES for
//                                                small batches), then the rc line
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/kspider_amd.h"

int main(int argc, char** argv) {
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "read" && argc > 2) {
        for (int i = 2; i < argc; ++i) {
            uint64_t info[4] = {0, 0, 0, 0};
            int rc = ksp_fastx_info(argv[i], info);
            if (rc == KSP_OK) {
                // exactly the reported sizes, so that a byte too many is a sanitizer report (an array of 0 gets one element: the
                // entry refuses a NULL pointer)
                const auto n = [](const uint64_t v) { return (size_t)(v ? v : 1); };
                std::vector<uint8_t> seq(n(info[1]));
                std::vector<uint64_t> rec_off(info[0] + 1), name_off(info[0] + 1);
                std::vector<char> names(n(info[2]));
                rc = ksp_fastx_load(argv[i], seq.data(), rec_off.data(), name_off.data(), names.data());
            }
            std::printf("%d %s\n", rc, argv[i]);
        }
        return 0;
    }
    if (cmd == "sketch" && (argc == 6 || (argc == 7 && std::strcmp(argv[6], "--per-record") == 0))) {
        setenv("KSPIDER_SKETCH", "host", 1);
        const int rc = kspider_sketch(argv[2], std::atoi(argv[3]), std::strtoull(argv[4], nullptr, 10), argv[5], 2, argc == 7 ? KSP_SKETCH_PER_RECORD : 0);
        std::printf("rc %d %s\n", rc, rc ? ksp_last_error() : "");
        return 0;
    }
    std::fprintf(stderr, "usage: %s read FILE... | sketch INPUT K SCALED OUT [--per-record]\n", argv[0]);
    return 2;
}
