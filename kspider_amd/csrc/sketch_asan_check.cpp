// Driver of the sketcher's sanitizer build (make asan-sketch): the host code of fastx_reader.cpp, sketch_files.cpp and
// sketch_cpu.cpp under -fsanitize=address,undefined, linked with the stub instead of the HIP engine.
//   sketch_asan_check read FILE...               every file through ksp_fastx_info and, when that accepts it, ksp_fastx_load into
//                                                buffers of exactly the reported sizes: one line "<rc> <file>" per file
//   sketch_asan_check sketch INPUT K SCALED OUT [--per-record]
//                                                kspider_sketch in host mode with 2 threads (set KSPIDER_SKETCH_BATCH_BYTES for
//                                                small batches), then the rc line
//   sketch_asan_check abund INPUT K SCALED OUT [--per-record]
//                                                the same with KSP_SKETCH_ABUND; then every file of OUT back through ksp_sig_read
//                                                into buffers of exactly the reported sizes: "sig <rc> <mins> <sum of the
//                                                abundances> <file>" per file, in the order of the names, then the rc line
//   sketch_asan_check mol FLAGS INPUT K SCALED OUT
//                                                kspider_sketch in host mode with FLAGS, the decimal value of any of its flags
//                                                (KSP_SKETCH_PROTEIN 8, _DAYHOFF 16, _HP 32, _TRANSLATE 64, _ABUND 4, _PER_RECORD 1);
//                                                then the files of OUT back through ksp_sig_read at 3 K, and the rc line
//   sketch_asan_check sigs K FILE...             every file through ksp_sig_read alone, the same lines
#include <dirent.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/kspider_amd.h"

// one signature file through the size query and, when that accepts it, the read into buffers of exactly that size
static void read_sig(const std::string& path, const int k) {
    uint64_t n = 0, sum = 0;
    int has = 0;
    int rc = ksp_sig_read(path.c_str(), k, nullptr, nullptr, 0, &n, &has);
    if (rc == KSP_OK || rc == KSP_E_OVERFLOW) {
        std::vector<uint64_t> mins((size_t)(n ? n : 1));
        std::vector<uint32_t> abunds((size_t)(n ? n : 1));
        rc = ksp_sig_read(path.c_str(), k, mins.data(), abunds.data(), n, &n, &has);
        if (rc == KSP_OK && has)
            for (uint64_t i = 0; i < n; ++i) sum += abunds[(size_t)i];
    }
    std::printf("sig %d %llu %llu %s\n", rc, (unsigned long long)n, (unsigned long long)sum, path.c_str());
}

// the files of a directory through read_sig, in the order of their names
static void read_sigs_of(const char* dir, const int k) {
    std::vector<std::string> names;
    if (DIR* d = opendir(dir)) {
        while (const dirent* e = readdir(d))
            if (e->d_name[0] != '.') names.push_back(e->d_name);
        closedir(d);
    }
    std::sort(names.begin(), names.end());
    for (const std::string& n : names) read_sig(std::string(dir) + "/" + n, k);
}

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
    if (cmd == "abund" && (argc == 6 || (argc == 7 && std::strcmp(argv[6], "--per-record") == 0))) {
        setenv("KSPIDER_SKETCH", "host", 1);
        const int rc = kspider_sketch(argv[2], std::atoi(argv[3]), std::strtoull(argv[4], nullptr, 10), argv[5], 2, KSP_SKETCH_ABUND | (argc == 7 ? KSP_SKETCH_PER_RECORD : 0));
        read_sigs_of(argv[5], std::atoi(argv[3]));
        std::printf("rc %d %s\n", rc, rc ? ksp_last_error() : "");
        return 0;
    }
    if (cmd == "mol" && argc == 7) {
        setenv("KSPIDER_SKETCH", "host", 1);
        const int rc = kspider_sketch(argv[3], std::atoi(argv[4]), std::strtoull(argv[5], nullptr, 10), argv[6], 2, std::strtoull(argv[2], nullptr, 10));
        read_sigs_of(argv[6], 3 * std::atoi(argv[4]));
        std::printf("rc %d %s\n", rc, rc ? ksp_last_error() : "");
        return 0;
    }
    if (cmd == "sigs" && argc > 3) {
        for (int i = 3; i < argc; ++i) read_sig(argv[i], std::atoi(argv[2]));
        return 0;
    }
    std::fprintf(stderr, "usage: %s read FILE... | sketch INPUT K SCALED OUT [--per-record] | abund INPUT K SCALED OUT [--per-record] | mol FLAGS INPUT K SCALED OUT | sigs K FILE...\n", argv[0]);
    return 2;
}
