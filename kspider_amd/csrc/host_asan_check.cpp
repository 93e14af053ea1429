// Driver of the sanitizer build (make asan): runs one host entry point on one input and prints its return code.
//   host_asan_check index PREFIX | info PREFIX | sigs DIR KSIZE OUTPREFIX | bins DIR OUTPREFIX
//                   | cut PREFIX DIST CUTOFF | edges_cut X | host_cut X   (the last two: the entry point with nothing to do)
//                   | partial DIR   (partial_file.h itself in DIR, which holds only the directory d.tsv with a file in it: one
//                                    "ok" / "FAIL" line per case)
//                   | plan sketch N DEVICES | plan postings DEVICES COUNT...   (slice_plan.h with $KSP_SLICES: the slices of N key
//                                    entries, or of an index whose keys have COUNT members each, on the devices "0,1,...": the
//                                    lines "slices S", "devices d0 d1 ...", "cuts c0 c1 ..." and "sliced 0|1", then the rc line)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/kspider_amd.h"
#include "partial_file.h"
#include "slice_plan.h"

namespace {
bool exists(const std::string& path) { return (bool)std::ifstream(path); }
std::string partial_of(const std::string& path) { return path + ".partial"; }   // (spelled out here: the helper's own is what is checked)
bool holds(const std::string& path, const std::string& text) {
    std::ifstream f(path, std::ios::binary);
    std::ostringstream ss;
    ss << f.rdbuf();
    return f && ss.str() == text;
}
void report(const char* name, const bool ok) { std::printf("%s %s\n", ok ? "ok" : "FAIL", name); }

int check_partial_files(const std::string& dir) {
    const std::string a = dir + "/a.tsv", b = dir + "/b.tsv";
    {   // two files opened and committed
        {
            std::ofstream fa, fb;
            ksp::PartialFiles files;
            files.open(a, fa);
            files.open(b, fb);
            fa << "first\n";
            fb << "second\r\n\n";
            files.commit();
        }
        report("committed", holds(a, "first\n") && holds(b, "second\r\n\n") && !exists(partial_of(a)) && !exists(partial_of(b)));
        std::remove(a.c_str());
        std::remove(b.c_str());
    }
    {   // two files opened, an exception before the commit
        bool thrown = false, seen = false;
        try {
            std::ofstream fa, fb;
            ksp::PartialFiles files;
            files.open(a, fa);
            files.open(b, fb);
            fa << "first\n";
            fa.flush();
            seen = exists(partial_of(a)) && exists(partial_of(b));
            throw std::runtime_error("stop");
        } catch (const std::runtime_error&) {
            thrown = true;
        }
        report("abandoned", thrown && seen && !exists(a) && !exists(b) && !exists(partial_of(a)) && !exists(partial_of(b)));
    }
    {   // a directory that does not exist
        const std::string c = dir + "/missing/c.tsv";
        bool thrown = false;
        try {
            std::ofstream f;
            ksp::PartialFiles files;
            files.open(c, f);
            files.commit();
        } catch (const std::runtime_error&) {
            thrown = true;
        }
        report("no directory", thrown && !exists(c) && !exists(partial_of(c)) && !exists(dir + "/missing"));
    }
    {   // a rename that fails: the final name is a directory that is not empty (DIR/d.tsv/keep, made by the caller)
        const std::string d = dir + "/d.tsv";
        bool thrown = false;
        try {
            ksp::write_file_atomically(d, "text\n");
        } catch (const std::runtime_error&) {
            thrown = true;
        }
        report("rename refused", thrown && !exists(partial_of(d)) && exists(d + "/keep"));
    }
    return 0;
}

int print_plan(const int argc, char** argv) {
    const bool postings = !std::strcmp(argv[2], "postings");
    std::vector<int> devices;
    for (const char* p = argv[postings ? 3 : 4]; *p; p += std::strcspn(p, ","), p += *p == ',') devices.push_back(std::atoi(p));
    std::vector<uint64_t> key_off(1, 0);
    for (int a = 4; postings && a < argc; ++a) key_off.push_back(key_off.back() + std::strtoull(argv[a], nullptr, 10));
    const uint64_t n = postings ? key_off.back() : std::strtoull(argv[3], nullptr, 10);
    ksp::SlicePlan plan;
    const uint32_t n_keys = (uint32_t)key_off.size() - 1;   // (no COUNT: an index without keys, whose key_off may be NULL)
    const int rc = ksp::plan_slices(postings, n, n_keys, postings && n_keys ? key_off.data() : nullptr, devices.data(), (int)devices.size(),
                                    std::getenv("KSP_SLICES"), plan);
    if (rc) return rc;
    std::printf("slices %zu\ndevices", plan.devices.size());
    for (const int d : plan.devices) std::printf(" %d", d);
    std::printf("\ncuts");
    for (const uint32_t c : plan.pk_cut) std::printf(" %u", c);
    std::printf("\nsliced %d\n", (int)plan.sliced);
    return rc;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) return 64;
    int rc = -1;
    if (!std::strcmp(argv[1], "partial")) return check_partial_files(argv[2]);
    if (!std::strcmp(argv[1], "plan") && argc >= (std::strcmp(argv[2], "postings") ? 5 : 4)) rc = print_plan(argc, argv);
    else if (!std::strcmp(argv[1], "index")) rc = kspider_pairwise(argv[2], 2);
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
