// Driver of the sanitizer build (make asan): runs one host entry point on one input and prints its return code.
//   host_asan_check index PREFIX | info PREFIX | sigs DIR KSIZE OUTPREFIX | bins DIR OUTPREFIX
//                   | cut PREFIX DIST CUTOFF | edges_cut X | host_cut X   (the last two: the entry point with nothing to do)
//                   | partial DIR   (partial_file.h itself in DIR, which holds only the directory d.tsv with a file in it: one
//                                    "ok" / "FAIL" line per case)
//                   | plan sketch N DEVICES | plan postings DEVICES COUNT...   (slice_plan.h with $KSP_SLICES: the slices of N key
//                                    entries, or of an index whose keys have COUNT members each, on the devices "0,1,...": the
//                                    lines "slices S", "devices d0 d1 ...", "cuts c0 c1 ..." and "sliced 0|1", then the rc line)
//                   | tsv_text STRIDE NMAX   (tsv_text.h, the code of the device's row text, against snprintf on the host: every STRIDE-th
//                                    float of the domain, the quotients s / n up to NMAX, j * 2^k, rows at both length bounds, the
//                                    refusals: one "ok" / "FAIL" line per case)
//                   | tsv_pieces DIR   (index_io.h's PairwiseTsvPieces in DIR: committed in pieces that end inside rows, abandoned)
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/kspider_amd.h"
#include "index_io.h"
#include "partial_file.h"
#include "slice_plan.h"
#include "tsv_text.h"

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

// the text of tsv_text.h for a float, "" when it is refused
std::string tsv_float_text(const float v) {
    uint32_t bits;
    std::memcpy(&bits, &v, 4);
    const ksp_tsv::FloatDigits f = ksp_tsv::float_digits(bits);
    if (f.kind == ksp_tsv::FloatDigits::kRefused) return "";
    ksp_tsv::Counter c;
    ksp_tsv::emit_float(c, f);
    std::string out(c.n, '?');
    ksp_tsv::Writer w{&out[0]};
    ksp_tsv::emit_float(w, f);
    return w.p == out.data() + out.size() ? out : "length mismatch";
}
bool tsv_float_agrees(const float v, uint64_t* bad) {
    char buf[32];
    buf[ksp::format_float(buf, v)] = 0;
    if (tsv_float_text(v) == buf) return true;
    if ((*bad)++ < 5) std::printf("mismatch %.9g: libc '%s' here '%s'\n", (double)v, buf, tsv_float_text(v).c_str());
    return false;
}
std::string tsv_row_text(const uint32_t id1, const uint32_t id2, const uint64_t shared, const float mn, const float av, const float mx) {
    ksp_tsv::RowText r{id1, id2, shared, {}};
    const float col[3] = {mn, av, mx};
    for (int c = 0; c < 3; ++c) {
        uint32_t bits;
        std::memcpy(&bits, &col[c], 4);
        r.col[c] = ksp_tsv::float_digits(bits);
    }
    ksp_tsv::Counter c;
    ksp_tsv::emit_row(c, r);
    std::string out(c.n, '?');
    ksp_tsv::Writer w{&out[0]};
    ksp_tsv::emit_row(w, r);
    return out;
}
int check_tsv_text(const uint32_t stride, const uint32_t n_max) {
    uint64_t bad = 0, n = 0;
    bool est = true;   // the estimate of the decimal exponent: floor(b * log10(2)) for every binary exponent of the domain
    for (int b = -40; b <= 39; ++b) {
        int want = 0;
        const double x = std::ldexp(1.0, b);
        while (std::pow(10.0, want) > x) --want;
        while (std::pow(10.0, want + 1) <= x) ++want;
        est = est && ((b * 1233) >> 12) == want;
    }
    report("exponent estimate", est);
    for (uint64_t bits = (uint64_t)(127 - 40) << 23; bits < (uint64_t)(127 + 40) << 23; bits += stride, ++n) {
        float v;
        const uint32_t b32 = (uint32_t)bits;
        std::memcpy(&v, &b32, 4);
        tsv_float_agrees(v, &bad);
    }
    std::printf("strided %llu\n", (unsigned long long)n);
    report("every STRIDE-th float of the domain", bad == 0);
    bad = 0;
    for (uint32_t d = 1; d <= n_max; ++d)
        for (uint32_t s = 1; s <= d; ++s) tsv_float_agrees((float)s / (float)d, &bad);
    report("quotients", bad == 0);
    bad = 0;
    for (int k = -40; k <= 28; ++k)
        for (uint32_t j = 1; j < 4096; ++j) {
            const float v = std::ldexp((float)j, k);
            if (v >= std::ldexp(1.0f, -40) && v < std::ldexp(1.0f, 40)) tsv_float_agrees(v, &bad);
        }
    report("j * 2^k", bad == 0);
    report("zero and inf", tsv_float_text(0.0f) == "0" && tsv_float_text(INFINITY) == "inf");
    report("ties", tsv_float_text(1.0f / 1024) == "0.000976562" && tsv_float_text(3.0f / 1024) == "0.00292969");
    report("refused", tsv_float_text(-1.0f).empty() && tsv_float_text(-0.0f).empty() && tsv_float_text(NAN).empty() && tsv_float_text(std::ldexp(1.0f, 40)).empty() &&
                          tsv_float_text(std::ldexp(1.0f, -41)).empty() && tsv_float_text(1e-40f).empty() && tsv_float_text(-INFINITY).empty());
    char want[160];
    const float big = 1e19f / 4294967295.0f;
    std::snprintf(want, sizeof want, "%u\t%u\t%llu\t%.6g\t%.6g\t%.6g\n", 4294967295u, 4294967294u, 18446744073709551615ull, (double)big, (double)big, (double)big);
    const std::string longest = tsv_row_text(4294967295u, 4294967294u, 18446744073709551615ull, big, big, big);
    report("longest row", longest == want && longest.size() == KSP_TSV_ROW_MAX);
    const std::string shortest = tsv_row_text(0, 1, 7, 1.0f, 1.0f, 1.0f);
    report("shortest row", shortest == "0\t1\t7\t1\t1\t1\n" && shortest.size() == KSP_TSV_ROW_MIN);
    return 0;
}

int check_tsv_pieces(const std::string& dir) {
    const std::string prefix = dir + "/p", path = prefix + "_kSpider_pairwise.tsv";
    const std::string header = "source_1\tsource_2\tshared_kmers\tmin_containment\tavg_containment\tmax_containment\n";
    const std::string rows = "1\t2\t3\t0.5\t0.75\t1\n10\t20\t30\t0.000976562\t1.5\tinf\n";
    {
        bool partial_seen = false;
        {
            ksp::PairwiseTsvPieces f(prefix);
            for (size_t at = 0; at < rows.size(); at += 7) f.append(rows.data() + at, std::min<size_t>(7, rows.size() - at));   // pieces end inside rows
            f.append(rows.data(), 0);
            partial_seen = exists(partial_of(path)) && !exists(path) && f.bytes() == rows.size();
            f.commit();
        }
        report("pieces committed", partial_seen && holds(path, header + rows) && !exists(partial_of(path)));
        std::remove(path.c_str());
    }
    {
        {
            ksp::PairwiseTsvPieces f(prefix);
            f.append(rows.data(), 5);
        }
        report("pieces abandoned", !exists(path) && !exists(partial_of(path)));
    }
    {
        bool thrown = false;
        try {
            ksp::PairwiseTsvPieces f(dir + "/missing/p");
        } catch (const std::runtime_error&) {
            thrown = true;
        }
        report("pieces without a directory", thrown);
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
    if (!std::strcmp(argv[1], "tsv_text")) return check_tsv_text((uint32_t)std::max(1, std::atoi(argv[2])), argc > 3 ? (uint32_t)std::atoi(argv[3]) : 4096u);
    if (!std::strcmp(argv[1], "tsv_pieces")) return check_tsv_pieces(argv[2]);
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
