// The newick text of a merge table and the union-find the tree writers share (tree.hip, upgma.hip); each includes its own copy.
// Host only.
#ifndef KSPIDER_TREE_NEWICK_H
#define KSPIDER_TREE_NEWICK_H
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <ostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "engine_internal.h"

namespace {

struct TreeDsu {
    std::vector<uint32_t> parent, size;
    explicit TreeDsu(const uint64_t n) : parent((size_t)n), size((size_t)n, 1) { std::iota(parent.begin(), parent.end(), 0u); }
    uint32_t find(uint32_t v) {
        while (parent[v] != v) { parent[v] = parent[parent[v]]; v = parent[v]; }
        return v;
    }
};

std::string fmt_len(const double v) {
    char buf[64];
    std::snprintf(buf, sizeof buf, "%.6g", v);
    return buf;
}

// The newick text of the merges (rows in merge order, node indices): leaves are 0 .. N - 1, merge i makes node N + i out of the
// trees that hold its two ends, the one holding `a` first.  Written with an explicit stack: a chain of 10^6 merges is 10^6 deep.
void write_newick(std::ostream& f, const std::vector<ksp::TreeRow>& rows, const std::vector<std::string>& name_of) {
    const uint64_t N = name_of.size(), M = rows.size();
    if (N + M >= (1ull << 32)) throw std::runtime_error("tree: more than 2^32 tree nodes");
    std::vector<uint32_t> left((size_t)M), right((size_t)M);
    std::vector<double> height((size_t)(N + M), 0.0);
    std::vector<uint32_t> top((size_t)N);   // per union-find root: the tree node that stands for its cluster
    TreeDsu dsu(N);
    std::iota(top.begin(), top.end(), 0u);
    for (uint64_t i = 0; i < M; ++i) {
        const uint32_t ra = dsu.find(rows[(size_t)i].a), rb = dsu.find(rows[(size_t)i].b);
        left[(size_t)i] = top[ra];
        right[(size_t)i] = top[rb];
        double h = 1.0 - rows[(size_t)i].value;
        if (h != h) h = 0.0;
        height[(size_t)(N + i)] = std::min(1.0, std::max(0.0, h));
        const uint32_t r = std::min(ra, rb);   // (the label of a cluster is its smallest node: the roots come out in that order below)
        dsu.parent[std::max(ra, rb)] = r;
        top[r] = (uint32_t)(N + i);
    }
    std::vector<uint32_t> roots;
    for (uint64_t v = 0; v < N; ++v)
        if (dsu.parent[(size_t)v] == v) roots.push_back(top[(size_t)v]);
    if (roots.empty()) { f << ";\n"; return; }
    const bool joint = roots.size() > 1;   // clusters that never join: under one root at height 1, which stands for no shared k-mers
    // one frame per open inner node: (node, children written so far); a leaf is written at once
    struct Frame { uint32_t node; uint32_t done; double up; };   // up: the height of the parent (a branch length = up - own height), < 0: no parent
    std::vector<Frame> stack;
    auto open = [&](const uint32_t node, const double up) {
        if (node < N) {
            f << name_of[node];
            if (up >= 0) f << ':' << fmt_len(up - 0.0);
        } else {
            f << '(';
            stack.push_back(Frame{node, 0, up});
        }
    };
    if (joint) f << '(';
    for (size_t r = 0; r < roots.size(); ++r) {
        if (r) f << ',';
        open(roots[r], joint ? 1.0 : -1.0);
        while (!stack.empty()) {
            Frame& t = stack.back();
            const uint32_t i = t.node - (uint32_t)N;
            if (t.done == 2) {
                f << ')';
                if (t.up >= 0) f << ':' << fmt_len(t.up - height[t.node]);
                stack.pop_back();
                continue;
            }
            const uint32_t child = t.done == 0 ? left[i] : right[i];
            if (t.done == 1) f << ',';
            ++t.done;
            open(child, height[t.node]);   // (may push: t is not used after this)
        }
    }
    if (joint) f << ')';
    f << ";\n";
}

}  // namespace
#endif
