// Driver of the pack reader's sanitizer build (make asan-pack): the host code of sketch_pack.cpp under
// -fsanitize=address,undefined, linked with the stub instead of the HIP engine.
//   pack_asan_check read FILE...     every file through ksp_pack_info and, when that accepts it, ksp_pack_load into buffers of
//                                    exactly the reported sizes: one line "<rc> <file>" per file
//   pack_asan_check pack DIR K OUT   kspider_pack, then the rc line
//   pack_asan_check query DB Q K OUT kspider_query up to the device call (the stub's ksp_query_host fails), then the rc line
//   pack_asan_check compare SAMPLES K OUT [DB]   kspider_compare (with the matrix unless DB is given) up to the device call, then
//                                    the rc line; and ksp_compare_values on a row at the top of its range, one line of four values
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
            uint64_t info[5] = {0, 0, 0, 0, 0};
            int rc = ksp_pack_info(argv[i], info);
            if (rc == KSP_OK) {
                // exactly the reported sizes, so that a byte too many is a sanitizer report (an array of 0 gets one element: the
                // entry refuses a NULL pointer)
                const auto n = [](const uint64_t v) { return (size_t)(v ? v : 1); };
                std::vector<uint32_t> kmers(n(info[1]));
                std::vector<uint8_t> present(n(info[1]));
                std::vector<uint64_t> offsets(info[2] + 1), keys(n(info[3])), name_off(info[1] + 1);
                std::vector<char> names(n(info[4]));
                rc = ksp_pack_load(argv[i], kmers.data(), present.data(), offsets.data(), keys.data(), name_off.data(), names.data());
            }
            std::printf("%d %s\n", rc, argv[i]);
        }
        return 0;
    }
    if (cmd == "pack" && argc == 5) {
        const int rc = kspider_pack(argv[2], std::atoi(argv[3]), argv[4], 2);
        std::printf("rc %d %s\n", rc, rc ? ksp_last_error() : "");
        return 0;
    }
    if (cmd == "query" && argc == 6) {
        const int rc = kspider_query(argv[2], argv[3], std::atoi(argv[4]), argv[5], 2, KSP_QUERY_CROSS);
        std::printf("rc %d %s\n", rc, rc ? ksp_last_error() : "");
        return 0;
    }
    if (cmd == "compare" && (argc == 5 || argc == 6)) {
        const int rc = kspider_compare(argv[2], argc == 6 ? argv[5] : nullptr, std::atoi(argv[3]), argv[4], 2, argc == 6 ? 0 : KSP_COMPARE_MATRIX);
        std::printf("rc %d %s\n", rc, rc ? ksp_last_error() : "");
        const uint64_t top = ~0ull;
        const ksp_wedge row = {0, 1, 5, top, 10, 9};
        double v[4] = {0, 0, 0, 0};
        const int rv = ksp_compare_values(&row, 5, 10, top, 5, 10, top, v);
        std::printf("values %d %.17g %.17g %.17g %.17g\n", rv, v[0], v[1], v[2], v[3]);
        return 0;
    }
    std::fprintf(stderr, "usage: %s read FILE... | pack DIR K OUT | query DB Q K OUT | compare SAMPLES K OUT [DB]\n", argv[0]);
    return 2;
}
