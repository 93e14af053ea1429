// `kSpider pairwise --estimate-ani` (pykSpider/kSpider2/ks_pairwise.py:29-84) on the host: the ANI table the device
// looks up (ani.h), the ANI column writer of the fused pairwise calls, and kspider_estimate_ani over existing files.
#include <algorithm>
#include <cctype>
#include <cerrno>
#include <charconv>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <mutex>
#include <sstream>
#include <stdexcept>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/kspider_amd.h"
#include "ani.h"
#include "engine_internal.h"
#include "index_io.h"
#include "partial_file.h"

namespace ksp {

double ani_g(const double c, const int ksize) {
    // containment_to_distance's point estimate, then ANIResult.ani = 1 - dist.  Evaluated in this order, no fused
    // operations (there is no product to fuse), so the double is the one Python computes.
    if (c != c) return c;
    double pe;
    if (c <= 0.0001) pe = 1.0;
    else if (c >= 0.9999) pe = 0.0;
    else pe = 1.0 - std::pow(c, 1.0 / ksize);
    return 1 - pe;
}

std::shared_ptr<const std::vector<double>> ani_table(const int ksize) {
    static std::mutex mu;
    static std::map<int, std::shared_ptr<const std::vector<double>>> cache;
    std::lock_guard<std::mutex> lock(mu);
    auto it = cache.find(ksize);
    if (it != cache.end()) return it->second;
    auto t = std::make_shared<std::vector<double>>(kAniTableSize);
    double* out = t->data();
    static const double p10[4] = {1e9, 1e8, 1e7, 1e6};
    // entry (9 - q) * 900000 + (d - 100000) holds g of the decimal d * 10^-q.  d / 10^q in double is the correctly
    // rounded quotient of two exact doubles: the same double strtod makes of the decimal's text.
    auto work = [&](uint32_t i0, uint32_t i1) {
        for (uint32_t i = i0; i < i1; ++i)
            out[i] = ani_g((double)(100000 + i % kAniDecade) / p10[i / kAniDecade], ksize);
    };
    const unsigned nt = std::max(1u, std::min(32u, std::thread::hardware_concurrency()));
    std::vector<std::thread> th;
    for (unsigned p = 0; p < nt; ++p) th.emplace_back(work, (uint32_t)((uint64_t)kAniTableSize * p / nt), (uint32_t)((uint64_t)kAniTableSize * (p + 1) / nt));
    for (auto& x : th) x.join();
    cache.emplace(ksize, t);
    return t;
}

int format_py_repr(char* buf, const double v) {
    // repr(float): the shortest digits that round-trip; positional notation unless the decimal exponent is < -4 or
    // >= 16; ".0" on an integral value; an exponent with a sign and at least two digits.
    if (v != v) { std::memcpy(buf, "nan", 3); return 3; }
    char sci[40];
    const auto r = std::to_chars(sci, sci + sizeof sci, v, std::chars_format::scientific);
    const char* p = sci;
    int n = 0;
    if (*p == '-') buf[n++] = *p++;
    if (*p == 'i') { std::memcpy(buf + n, "inf", 3); return n + 3; }
    const char* e = std::find(p, (const char*)r.ptr, 'e');
    int exp10 = 0;
    std::from_chars(e + 1 + (e[1] == '+'), r.ptr, exp10);   // (sci is not NUL-terminated)
    if (exp10 < -4 || exp10 >= 16) {   // to_chars already writes the exponent as Python does (e-05, e+16)
        std::memcpy(buf + n, p, (size_t)(r.ptr - p));
        return n + (int)(r.ptr - p);
    }
    char dig[24];
    int nd = 0;
    for (const char* x = p; x < e; ++x)
        if (*x != '.') dig[nd++] = *x;
    if (exp10 < 0) {
        buf[n++] = '0';
        buf[n++] = '.';
        for (int z = 0; z < -exp10 - 1; ++z) buf[n++] = '0';
        for (int i = 0; i < nd; ++i) buf[n++] = dig[i];
        return n;
    }
    for (int i = 0; i <= exp10; ++i) buf[n++] = i < nd ? dig[i] : '0';
    buf[n++] = '.';
    if (nd <= exp10 + 1) buf[n++] = '0';
    for (int i = exp10 + 1; i < nd; ++i) buf[n++] = dig[i];
    return n;
}

namespace {

bool is_blank(char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == '\v' || c == '\f'; }
void strip(const char*& b, const char*& e) {
    while (b < e && is_blank(*b)) ++b;
    while (e > b && is_blank(e[-1])) --e;
}
// Python's number texts allow one '_' between two digits ("1_000"): drop them, refuse any other '_'
bool drop_underscores(char* buf) {
    const auto digit = [](char c) { return c >= '0' && c <= '9'; };
    char* w = buf;
    for (const char* r = buf; *r; ++r) {
        if (*r == '_') {
            if (r == buf || !digit(r[-1]) || !digit(r[1])) return false;
            continue;
        }
        *w++ = *r;
    }
    *w = 0;
    return true;
}
// int(text): surrounding blanks, an optional sign, decimal digits
bool py_int(const char* b, const char* e, long long& v) {
    strip(b, e);
    if (b == e || e - b > 30) return false;
    char buf[32];
    std::memcpy(buf, b, (size_t)(e - b));
    buf[e - b] = 0;
    if (!drop_underscores(buf)) return false;
    const char* d = buf + (buf[0] == '+' || buf[0] == '-');
    if (!*d) return false;
    for (const char* x = d; *x; ++x)
        if (*x < '0' || *x > '9') return false;
    errno = 0;
    char* end = nullptr;
    v = std::strtoll(buf, &end, 10);
    return !errno && *end == 0;
}
// float(text): decimal, inf, nan (strtod's hexadecimal and nan(...) forms are not Python's)
bool py_float(const char* b, const char* e, double& v) {
    strip(b, e);
    if (b == e || e - b > 60) return false;
    char buf[64];
    std::memcpy(buf, b, (size_t)(e - b));
    buf[e - b] = 0;
    if (std::strpbrk(buf, "xX(") || !drop_underscores(buf)) return false;
    char* end = nullptr;
    v = std::strtod(buf, &end);
    return end != buf && *end == 0;
}

std::string read_file(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error("cannot open " + path);
    std::ostringstream ss;
    ss << f.rdbuf();
    return ss.str();
}

// the lines of a text file as Python iterates them ('\n'-terminated; a last line without one counts)
void split_lines(const std::string& s, std::vector<std::pair<size_t, size_t>>& lines) {
    size_t b = 0;
    while (b < s.size()) {
        size_t e = s.find('\n', b);
        if (e == std::string::npos) e = s.size();
        lines.emplace_back(b, e);
        b = e + 1;
    }
}

void write_through_partial(const std::string& path, const std::vector<std::string>& parts) {
    std::ofstream f;
    PartialFiles files;
    files.open(path, f);
    f << "avg_ani\n";
    for (auto& s : parts)
        if (!s.empty() && !f.write(s.data(), (std::streamsize)s.size())) break;
    files.commit();
}

template <class F>
void parallel_chunks(size_t n, int threads, F&& f) {
    const size_t T = (size_t)std::max(1, std::min(threads, 64));
    if (T == 1 || n < 4096) { f(0, (size_t)0, n); return; }
    std::vector<std::thread> th;
    for (size_t t = 0; t < T; ++t) th.emplace_back([&, t] { f(t, n * t / T, n * (t + 1) / T); });
    for (auto& x : th) x.join();
}

}  // namespace

int read_extra_ksize(const std::string& prefix) {
    const std::string path = prefix + ".extra";
    std::ifstream f(path);
    if (!f) throw std::runtime_error("cannot open " + path + " (the k-mer size is read from its first line)");
    std::string line;
    long long k = 0;
    if (!std::getline(f, line) || !py_int(line.data(), line.data() + line.size(), k))
        throw std::runtime_error("the first line of " + path + " is not an integer k-mer size");
    // (k is an int of the C ABI: a first line above 2^31 - 1, which Python would take, is refused)
    if (k < 1 || k > 2147483647LL) throw std::runtime_error("k-mer size " + std::to_string(k) + " in " + path + " is not usable");
    return (int)k;
}

void row_min_max(const uint64_t shared, const uint32_t n1, const uint32_t n2, float* mn, float* mx) {
    // index_io.cpp format_rows = src/pairwise.cpp:260-264, single precision
    const float cont_1_in_2 = (float)shared / n2;
    const float cont_2_in_1 = (float)shared / n1;
    *mn = std::min(cont_1_in_2, cont_2_in_1);
    *mx = std::max(cont_1_in_2, cont_2_in_1);
}

void write_ani_column(const std::string& prefix, const std::vector<EdgeRow>& rows, const std::unordered_map<uint32_t, uint32_t>& kmer_count,
                      const double* table, const int threads) {
    const size_t T = (size_t)std::max(1, std::min(threads, 64));
    std::vector<std::string> parts(T);
    std::vector<char> bad(T, 0);
    parallel_chunks(rows.size(), (int)T, [&](size_t t, size_t lo, size_t hi) {
        std::string& out = parts[t];
        out.reserve((hi - lo) * 20);
        char buf[40];
        for (size_t i = lo; i < hi; ++i) {
            const EdgeRow& e = rows[i];
            uint32_t n1 = 0, n2 = 0;   // operator[] of the reference yields 0 for a missing group
            auto it1 = kmer_count.find(e.source_1);
            if (it1 != kmer_count.end()) n1 = it1->second;
            auto it2 = kmer_count.find(e.source_2);
            if (it2 != kmer_count.end()) n2 = it2->second;
            float mn, mx;
            row_min_max(e.shared, n1, n2, &mn, &mx);
            double v;
            if (!ani_of_row(mn, mx, table, &v)) { bad[t] = 1; return; }
            const int n = format_py_repr(buf, v);
            buf[n] = '\n';
            out.append(buf, (size_t)n + 1);
        }
    });
    for (char b : bad)
        if (b) throw std::runtime_error("a pairwise row has a NaN containment (0 shared k-mers of a source with 0 k-mers): it has no ANI");
    write_through_partial(prefix + "_kSpider_pairwise.ani_col.tsv", parts);
}

namespace {

// ks_pairwise.py:29-84 over the files of any producer, rows in any order
int estimate_ani(const std::string& prefix, const int threads, const int64_t scale) {
    if (scale <= 0) {   // (:41-42; the value itself only feeds sourmash's p_nothing_in_common, which .ani discards)
        ksp::set_error("kspider_estimate_ani: estimating ANI needs the sourmash scale (> 0)");
        return KSP_E_ARG;
    }
    const int k = ksp::read_extra_ksize(prefix);
    std::unordered_map<long long, long long> kmers_of;   // (:52-58) id -> k-mer count; only membership matters
    {
        const std::string path = prefix + "_kSpider_seqToKmersNo.tsv";
        const std::string text = read_file(path);
        std::vector<std::pair<size_t, size_t>> lines;
        split_lines(text, lines);
        if (lines.empty()) throw std::runtime_error(path + " is empty");
        for (size_t i = 1; i < lines.size(); ++i) {
            const char *b = text.data() + lines[i].first, *e = text.data() + lines[i].second;
            strip(b, e);
            const char* t1 = std::find(b, e, '\t');
            const char* t2 = t1 == e ? e : std::find(t1 + 1, e, '\t');
            long long id, n;
            if (t1 == e || t2 == e || std::find(t2 + 1, e, '\t') != e || !py_int(t1 + 1, t2, id) || !py_int(t2 + 1, e, n))
                throw std::runtime_error("malformed row " + std::to_string(i + 1) + " in " + path);
            kmers_of[id] = n;
        }
    }
    const std::string path = prefix + "_kSpider_pairwise.tsv";
    const std::string text = read_file(path);
    std::vector<std::pair<size_t, size_t>> lines;
    split_lines(text, lines);
    if (lines.empty()) throw std::runtime_error(path + " is empty");
    const size_t n = lines.size() - 1;
    const size_t T = (size_t)std::max(1, std::min(threads, 64));
    std::vector<std::string> parts(T);
    std::vector<std::string> errs(T);
    parallel_chunks(n, (int)T, [&](size_t t, size_t lo, size_t hi) {
        std::string& out = parts[t];
        out.reserve((hi - lo) * 20);
        char buf[40];
        const char* f[6];
        const char* fe[6];
        for (size_t r = lo; r < hi; ++r) {
            const char *b = text.data() + lines[r + 1].first, *e = text.data() + lines[r + 1].second;
            strip(b, e);
            int nf = 0;
            for (const char* x = b; nf < 6;) {   // line.strip().split('\t')[0..5]
                const char* y = std::find(x, e, '\t');
                f[nf] = x; fe[nf] = y; ++nf;
                if (y == e) break;
                x = y + 1;
            }
            long long id1, id2, shared;
            double c3, c5;
            if (nf < 6 || !py_int(f[2], fe[2], shared) || !py_int(f[0], fe[0], id1) || !py_int(f[1], fe[1], id2) ||
                !py_float(f[3], fe[3], c3) || !py_float(f[5], fe[5], c5)) {
                errs[t] = "malformed row " + std::to_string(r + 2) + " in " + path;
                return;
            }
            if (!kmers_of.count(id2) || !kmers_of.count(id1)) {   // id_to_kmer_count[id] (:77-78): KeyError
                errs[t] = "row " + std::to_string(r + 2) + " of " + path + " names a source missing from _kSpider_seqToKmersNo.tsv";
                return;
            }
            const double g3 = ksp::ani_g(c3, k), g5 = ksp::ani_g(c5, k);
            if (g3 != g3 || g5 != g5) {   // sourmash rejects a NaN containment
                errs[t] = "row " + std::to_string(r + 2) + " of " + path + " has a NaN containment: it has no ANI";
                return;
            }
            const int m = ksp::format_py_repr(buf, (g3 + g5) / 2.0);
            buf[m] = '\n';
            out.append(buf, (size_t)m + 1);
        }
    });
    for (auto& e : errs)
        if (!e.empty()) { ksp::set_error("kspider_estimate_ani: " + e); return KSP_E_IO; }
    write_through_partial(prefix + "_kSpider_pairwise.ani_col.tsv", parts);
    return KSP_OK;
}

}  // namespace
}  // namespace ksp

extern "C" int kspider_estimate_ani(const char* index_prefix, int user_threads, int64_t scale) {
    if (!index_prefix) { ksp::set_error("kspider_estimate_ani: index_prefix is NULL"); return KSP_E_ARG; }
    try {
        return ksp::estimate_ani(index_prefix, user_threads < 1 ? 1 : user_threads, scale);
    } catch (const std::bad_alloc&) {
        ksp::set_error("kspider_estimate_ani: out of host memory");
        return KSP_E_LIMIT;
    } catch (const std::exception& e) {
        ksp::set_error(std::string("kspider_estimate_ani: ") + e.what());
        return KSP_E_IO;
    }
}

extern "C" int ksp_ani_values(const float* min_c, const float* max_c, uint64_t n, int ksize, int via_table, double* out) {
    if ((n && (!min_c || !max_c || !out)) || ksize < 1) { ksp::set_error("ksp_ani_values: NULL argument or ksize < 1"); return KSP_E_ARG; }
    try {
        std::shared_ptr<const std::vector<double>> table;
        if (via_table) table = ksp::ani_table(ksize);
        std::vector<char> nan(64, 0);
        ksp::parallel_chunks((size_t)n, (int)std::max(1u, std::thread::hardware_concurrency()), [&](size_t t, size_t lo, size_t hi) {
            char buf[40];
            for (size_t i = lo; i < hi; ++i) {
                double v;
                if (via_table) {
                    if (!ksp::ani_of_row(min_c[i], max_c[i], table->data(), &v)) v = std::nan("");
                } else {   // the text definition: "%.6g" -> strtod -> g
                    int m = ksp_format_float(min_c[i], buf);
                    buf[m] = 0;
                    const double g3 = ksp::ani_g(std::strtod(buf, nullptr), ksize);
                    m = ksp_format_float(max_c[i], buf);
                    buf[m] = 0;
                    const double g5 = ksp::ani_g(std::strtod(buf, nullptr), ksize);
                    v = (g3 + g5) / 2.0;
                }
                if (v != v) nan[t] = 1;
                out[i] = v;
            }
        });
        for (char b : nan)
            if (b) { ksp::set_error("ksp_ani_values: a NaN containment has no ANI"); return KSP_E_ARG; }
        return KSP_OK;
    } catch (const std::bad_alloc&) {
        ksp::set_error("ksp_ani_values: out of host memory");
        return KSP_E_LIMIT;
    }
}

extern "C" int ksp_ani_value(float min_c, float max_c, int ksize, int via_table, double* out) {
    if (!out) { ksp::set_error("ksp_ani_value: out is NULL"); return KSP_E_ARG; }
    return ksp_ani_values(&min_c, &max_c, 1, ksize, via_table, out);
}

extern "C" int ksp_format_ani(double value, char* buf) { return buf ? ksp::format_py_repr(buf, value) : 0; }
