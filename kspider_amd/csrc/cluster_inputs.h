// The inputs of `kSpider cluster`, read and validated as ks_clustering.py does (:48-61, :67-105), and the text helpers around
// them.  Shared by the clustering (cluster.hip), the trees (tree.hip, upgma.hip) and their siblings; each includes its own copy.
#ifndef KSPIDER_CLUSTER_INPUTS_H
#define KSPIDER_CLUSTER_INPUTS_H
#include <algorithm>
#include <cctype>
#include <cerrno>
#include <charconv>
#include <cstdint>
#include <cstdlib>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "engine_internal.h"

namespace {

// text of a double as Python's repr() prints it (the reference builds the output file name with an f-string)
std::string py_float_repr(double v) {
    char buf[64];
    auto r = std::to_chars(buf, buf + sizeof buf, v);
    std::string s(buf, r.ptr);
    if (s.find_first_of(".enai") == std::string::npos) s += ".0";
    return s;
}

bool split_tabs(const std::string& line, std::vector<std::string>& out) {
    out.clear();
    size_t b = 0;
    while (true) {
        const size_t e = line.find('\t', b);
        out.emplace_back(line.substr(b, e == std::string::npos ? std::string::npos : e - b));
        if (e == std::string::npos) break;
        b = e + 1;
    }
    return true;
}
std::string strip(const std::string& s) {
    size_t b = 0, e = s.size();
    while (b < e && std::isspace((unsigned char)s[b])) ++b;
    while (e > b && std::isspace((unsigned char)s[e - 1])) --e;
    return s.substr(b, e - b);
}
bool parse_id(const std::string& t, long long& v) {   // int(text): optional sign, digits, surrounding blanks
    const std::string s = strip(t);
    if (s.empty()) return false;
    char* end = nullptr;
    errno = 0;
    v = std::strtoll(s.c_str(), &end, 10);
    return !errno && end && *end == 0;
}
bool parse_float(const std::string& t, double& v) {   // float(text): decimal, inf, nan
    const std::string s = strip(t);
    if (s.empty()) return false;
    char* end = nullptr;
    v = std::strtod(s.c_str(), &end);
    return end && *end == 0;
}

// column of a distance name (6 = the ANI column file), 0 when unknown
int cluster_col(const std::string& dt) { return dt == "min_cont" ? 3 : dt == "avg_cont" ? 4 : dt == "max_cont" ? 5 : dt == "ani" ? 6 : 0; }

// name_of from .namesMap, then row(a, b, d, text) for every pairwise row, a / b its ids, text its column (col 6: its line of
// the ANI column file) as it stands in the file and d that text as a float times 100.
template <class Row>
void read_cluster_inputs(const std::string& prefix, const int col, std::vector<std::string>& name_of, Row&& row) {
    std::string line;
    {   // _kSpider_seqToKmersNo.tsv must be there and well-formed (load_seq_to_kmers, :48-53); its values are not used
        std::ifstream f(prefix + "_kSpider_seqToKmersNo.tsv");
        if (!f) throw std::runtime_error("cannot open " + prefix + "_kSpider_seqToKmersNo.tsv");
        std::getline(f, line);
        std::vector<std::string> p;
        while (std::getline(f, line)) {
            split_tabs(strip(line), p);
            long long a, b;
            if (p.size() != 3 || !parse_id(p[1], a) || !parse_id(p[2], b))
                throw std::runtime_error("malformed row in " + prefix + "_kSpider_seqToKmersNo.tsv");
        }
    }
    ksp::read_names_map(prefix, name_of);
    std::ifstream f(prefix + "_kSpider_pairwise.tsv");
    if (!f) throw std::runtime_error("cannot open " + prefix + "_kSpider_pairwise.tsv");
    std::ifstream ani;
    if (col == 6) {
        ani.open(prefix + "_kSpider_pairwise.ani_col.tsv");
        if (!ani) throw std::runtime_error("ANI was selected, but " + prefix + "_kSpider_pairwise.ani_col.tsv was not found");
        std::getline(ani, line);
    }
    std::getline(f, line);   // header
    std::vector<std::string> p;
    std::string aline;
    while (std::getline(f, line)) {
        split_tabs(strip(line), p);
        long long a, b;
        double d;
        if (p.size() < 2 || !parse_id(p[0], a) || !parse_id(p[1], b)) throw std::runtime_error("malformed row in " + prefix + "_kSpider_pairwise.tsv");
        if (col == 6) {
            if (!std::getline(ani, aline) || !parse_float(aline, d)) throw std::runtime_error("malformed / short " + prefix + "_kSpider_pairwise.ani_col.tsv");
            row(a, b, d * 100.0, strip(aline));
        } else if ((int)p.size() <= col || !parse_float(p[(size_t)col], d)) {
            throw std::runtime_error("malformed row in " + prefix + "_kSpider_pairwise.tsv");
        } else {
            row(a, b, d * 100.0, strip(p[(size_t)col]));
        }
    }
}

}  // namespace
#endif
