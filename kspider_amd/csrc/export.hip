// kspider_export(): the reference's `kSpider export` — pykSpider/kSpider2/ks_export.py — with the single-linkage tree
// of `--newick` computed on the GPU.
//
// What the reference does (restated, nothing copied):
//   * reads PREFIX_kSpider_seqToKmersNo.tsv (must parse, values unused), PREFIX.namesMap and PREFIX_kSpider_pairwise.tsv;
//     the value of a row is column dist_type (min_cont 3, avg_cont 4, max_cont 5) as a Python float, or for "ani" the
//     same line of PREFIX_kSpider_pairwise.ani_col.tsv;
//   * OUT_pairwise.tsv: the names of both ids and repr() of the value, one line per row;
//   * OUT_distmat.tsv: pandas' to_csv of an N x N DataFrame over the names that occur, sorted, cell (a, b) = (b, a) =
//     1 - value, fillna(0) — a column whose assigned values are all NaN becomes int64 and prints every cell "0",
//     any other column float64 with the fill printed "0.0"; a name holding '"' is quoted CSV-style;
//   * OUT.newick (--newick): the matrix read back by pandas' read_csv (precise_xstrtod: not correctly rounded), then
//     scipy's linkage(M, 'single') — Euclidean distances between the ROWS of M, a plain sequential sum over the
//     columns, and mst_single_linkage (Prim from node 0, ties to the smallest index, a stable sort by height, a
//     union-find relabel) — printed by to_tree + get_newick: "(<right>,<left>):%.2f", the root ends in ");".
// Deliberate differences: everything --newick needs (2 nodes or more, finite values, N <= 65 536, device memory) is
// checked before any file is written, and no file is left behind on an error (the reference writes two files and
// then raises); no recursion limit; a repeated unordered pair or a self pair is refused (the reference's result then
// depends on dict order).
//
// Device side: the dense matrix is scattered into HBM, k_row_dist computes the sums of squares of all row pairs as a
// tiled GEMM-like kernel (column chunks of both row blocks through LDS, a 4 x 4 register micro-tile per lane, columns
// in ascending order, no fused multiply-add), k_dist_sqrt takes the correctly rounded square root, and k_prim_single
// runs scipy's Prim loop step for step in one persistent 1024-thread workgroup.
#include <algorithm>
#include <atomic>
#include <cerrno>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <numeric>
#include <sstream>
#include <stdexcept>
#include <string>
#include <string_view>
#include <thread>
#include <unordered_map>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/kspider_amd.h"
#include "ani.h"
#include "device_call.h"
#include "engine_internal.h"
#include "partial_file.h"

typedef uint32_t u32;
typedef uint64_t u64;

namespace {

constexpr u32 kMaxNodes = 65536;
constexpr int kTile = 64;          // k_row_dist: 64 x 64 row pairs per workgroup
constexpr int kChunk = 16;         // columns per LDS stage
constexpr int kPrimThreads = 1024;
constexpr u32 kPrimLdsNodes = 19456;   // D[] of k_prim_single in LDS up to here (152 KiB), in global memory above

__global__ void k_scatter(const u32* __restrict__ p, const u32* __restrict__ q, const double* __restrict__ m, u64 ne, u32 n,
                          double* __restrict__ M) {
    for (u64 e = (u64)blockIdx.x * blockDim.x + threadIdx.x; e < ne; e += (u64)gridDim.x * blockDim.x) {
        M[(u64)p[e] * n + q[e]] = m[e];
        M[(u64)q[e] * n + p[e]] = m[e];
    }
}

// S[i][j] = sum over c = 0..n-1, in that order, of (M[i][c] - M[j][c])^2 — each operation rounded on its own, exactly
// what scipy's pdist(M, 'euclidean') sums before its sqrt.  Workgroup (bj, bi) with bj >= bi owns rows I0.. x J0..;
// lane (tx, ty) holds the pairs (I0 + ty + 16 r, J0 + tx + 16 q), r, q < 4.  Columns past n and rows past n load as
// 0: a padded column adds (0 - 0)^2 = +0, which leaves every sum as it is.  Both S[i][j] and S[j][i] are written.
__global__ __launch_bounds__(256) void k_row_dist(const double* __restrict__ M, u32 n, double* __restrict__ S) {
#pragma clang fp contract(off)
    const u32 bj = blockIdx.x, bi = blockIdx.y;
    if (bj < bi) return;
    __shared__ double As[kChunk][kTile], Bs[kChunk][kTile];
    const u32 t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const u32 I0 = bi * kTile, J0 = bj * kTile;
    double acc[4][4];
    for (int r = 0; r < 4; ++r)
        for (int q = 0; q < 4; ++q) acc[r][q] = 0.0;
    for (u32 c0 = 0; c0 < n; c0 += kChunk) {
        const u32 c = c0 + (t & 15);
        for (int q = 0; q < 4; ++q) {
            const u32 row = (t >> 4) + 16 * q;
            const u32 gi = I0 + row, gj = J0 + row;
            As[t & 15][row] = (gi < n && c < n) ? M[(u64)gi * n + c] : 0.0;
            Bs[t & 15][row] = (gj < n && c < n) ? M[(u64)gj * n + c] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kChunk; ++k) {
            double a[4], b[4];
            for (int r = 0; r < 4; ++r) a[r] = As[k][ty + 16 * r];
            for (int q = 0; q < 4; ++q) b[q] = Bs[k][tx + 16 * q];
            for (int r = 0; r < 4; ++r)
                for (int q = 0; q < 4; ++q) {
                    const double d = a[r] - b[q];   // (plain operators: the pragma above keeps them unfused;
                    acc[r][q] = acc[r][q] + d * d;   //  __dmul_rn / __dadd_rn are inlined with contraction allowed)
                }
        }
        __syncthreads();
    }
    for (int r = 0; r < 4; ++r)
        for (int q = 0; q < 4; ++q) {
            const u32 i = I0 + ty + 16 * r, j = J0 + tx + 16 * q;
            if (i >= n || j >= n) continue;
            if (bi == bj && i > j) continue;   // (the lane of (j, i) in this tile writes both)
            S[(u64)i * n + j] = acc[r][q];
            S[(u64)j * n + i] = acc[r][q];
        }
}

// kept out of k_row_dist so that its code object has no v_fma_f64 at all: the correctly rounded f64 sqrt uses fma.
// A finite matrix can still have an infinite distance (a cell of 1e200 squares to inf): *not_finite = 1 then, and the
// host refuses the matrix as scipy's linkage does ("must contain only finite values") before Prim runs.
__global__ void k_dist_sqrt(double* __restrict__ S, u64 count, u32* __restrict__ not_finite) {
    bool bad = false;
    for (u64 e = (u64)blockIdx.x * blockDim.x + threadIdx.x; e < count; e += (u64)gridDim.x * blockDim.x) {
        const double r = sqrt(S[e]);
        S[e] = r;
        bad |= !(r <= __DBL_MAX__);
    }
    if (bad) *not_finite = 1;
}

__device__ inline bool lex_less(double v1, u32 i1, double v2, u32 i2) { return v1 < v2 || (v1 == v2 && i1 < i2); }

// scipy's mst_single_linkage loop, step for step: D[] = inf; step k marks x merged, lowers D[i] to dist(x, i) for every
// unmerged i (`if D[i] > d`), takes y = the first index with the smallest D[i] and records (x, y, D[y]).  D[i] of node i
// lives with lane i % 1024 only, so the update needs no barrier; a merged node holds -1 (distances are >= 0).  Each
// lane scans its indices upwards keeping the first minimum, the workgroup then reduces (value, index) pairs: smaller
// value first, smaller index on a tie — the first index of the minimum, as scipy's scan finds it.
// Every live D[i] is finite once step 0 has run (the host has checked every distance), so the minimum always has an
// index; should none be found, *status = 1 and the kernel stops rather than take row 0xFFFFFFFF.  nearest (may be NULL):
// nearest[i] = the merged node whose row last lowered D[i], so that D[i] = dist(nearest[i], i) exactly (tests).
__global__ __launch_bounds__(kPrimThreads) void k_prim_single(const double* __restrict__ dist, u32 n, double* __restrict__ Dglobal,
                                                             int use_lds, double* __restrict__ rows, u32* __restrict__ status,
                                                             u32* __restrict__ nearest) {
    extern __shared__ double Dlds[];
    __shared__ double wv[kPrimThreads / 64];
    __shared__ u32 wi[kPrimThreads / 64];
    __shared__ u32 next_x;
    double* D = use_lds ? Dlds : Dglobal;
    const u32 t = threadIdx.x, lane = t & 63, wave = t >> 6;
    for (u32 i = t; i < n; i += kPrimThreads) D[i] = __builtin_inf();
    u32 x = 0;
    for (u32 k = 0; k + 1 < n; ++k) {
        const double* row = dist + (u64)x * n;
        double best = __builtin_inf();
        u32 bi = 0xFFFFFFFFu;
        for (u32 i = t; i < n; i += kPrimThreads) {
            if (i == x) { D[i] = -1.0; continue; }
            double d = D[i];
            if (d < 0.0) continue;
            const double v = row[i];
            if (d > v) {
                d = v;
                D[i] = d;
                if (nearest) nearest[i] = x;
            }
            if (d < best) { best = d; bi = i; }
        }
        for (int off = 32; off > 0; off >>= 1) {
            const double ov = __shfl_xor(best, off);
            const u32 oi = __shfl_xor(bi, off);
            if (lex_less(ov, oi, best, bi)) { best = ov; bi = oi; }
        }
        if (lane == 0) { wv[wave] = best; wi[wave] = bi; }
        __syncthreads();
        if (wave == 0) {
            best = lane < kPrimThreads / 64 ? wv[lane] : __builtin_inf();
            bi = lane < kPrimThreads / 64 ? wi[lane] : 0xFFFFFFFFu;
            for (int off = 8; off > 0; off >>= 1) {
                const double ov = __shfl_xor(best, off);
                const u32 oi = __shfl_xor(bi, off);
                if (lex_less(ov, oi, best, bi)) { best = ov; bi = oi; }
            }
            if (lane == 0) {
                next_x = bi;
                if (bi >= n) *status = 1;
                rows[3 * (u64)k] = (double)x;
                rows[3 * (u64)k + 1] = (double)bi;
                rows[3 * (u64)k + 2] = best;
            }
        }
        __syncthreads();
        x = next_x;
        if (x >= n) return;   // (uniform: every lane read the same next_x)
    }
}

using Clock = std::chrono::steady_clock;
double ms_since(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }

struct Phases {   // $KSP_EXPORT_TIMES=1: one line of phase times on stderr
    bool on = false;
    std::string text;
    Clock::time_point t = Clock::now();
    void mark(const char* name) {
        if (!on) return;
        char b[64];
        std::snprintf(b, sizeof b, "%s%s %.1f ms", text.empty() ? "" : ", ", name, ms_since(t));
        text += b;
        t = Clock::now();
    }
};

// scipy's linkage after mst_single_linkage's loop: stable sort of the (x, y, height) rows by height, union-find relabel
bool relabel(u32 n, const std::vector<double>& prim, double* Z) {
    std::vector<u32> order(n - 1);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](u32 a, u32 b) { return prim[3 * (u64)a + 2] < prim[3 * (u64)b + 2]; });
    std::vector<u32> parent(2 * (u64)n - 1), size(2 * (u64)n - 1, 1);
    std::iota(parent.begin(), parent.end(), 0u);
    auto find = [&](u32 x) {
        u32 r = x;
        while (parent[r] != r) r = parent[r];
        while (parent[x] != r) { const u32 nx = parent[x]; parent[x] = r; x = nx; }
        return r;
    };
    for (u32 i = 0; i + 1 < n; ++i) {
        const double* row = &prim[3 * (u64)order[i]];
        if (!(row[0] >= 0 && row[0] < n && row[1] >= 0 && row[1] < n)) return false;
        const u32 a = find((u32)row[0]), b = find((u32)row[1]);
        parent[a] = parent[b] = n + i;
        size[n + i] = size[a] + size[b];
        Z[4 * (u64)i] = (double)std::min(a, b);
        Z[4 * (u64)i + 1] = (double)std::max(a, b);
        Z[4 * (u64)i + 2] = row[2];
        Z[4 * (u64)i + 3] = (double)size[n + i];
    }
    return true;
}

// k_row_dist + k_dist_sqrt: the n x n distances between the rows of d_rows into d_dist (device memory of the current
// device), *d_not_finite = 1 when one is not finite.  The export's linkage and ksp_row_distances both launch them here.
hipError_t launch_row_distances(u32 n, const double* d_rows, double* d_dist, u32* d_not_finite) {
    const u64 nn = (u64)n * n;
    const u32 nb = (n + kTile - 1) / kTile;
    hipLaunchKernelGGL(k_row_dist, dim3(nb, nb), dim3(256), 0, nullptr, d_rows, n, d_dist);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(k_dist_sqrt, dim3((unsigned)std::min<u64>((nn + 255) / 256, 8192)), dim3(256), 0, nullptr, d_dist, nn, d_not_finite);
    return hipGetLastError();
}

// linkage of the n x n row matrix d_rows (device memory of the current device) into h_Z and / or Prim's (x, y, height)
// rows before the sort, each with the merged node nearest to y, into h_prim ((n - 1) x 4; either may be NULL); d_rows is
// not changed.  KSP_E_ARG when a distance is not finite.
int single_linkage_on_device(u32 n, const double* d_rows, double* h_Z, double* h_prim, Phases* ph) {
    int rc = KSP_OK;
    ksp::DeviceArena A;
    double *d_dist = nullptr, *d_prim = nullptr, *d_D = nullptr;
    u32* d_near = nullptr;
    std::vector<u32> near(h_prim ? n : 0);
    u32* d_flags = nullptr;   // [0] a distance is not finite, [1] Prim found no minimum
    u32 flags[2] = {0, 0};
    std::vector<double> prim(3 * (u64)(n - 1));
    const u64 nn = (u64)n * n;
    const char* lds_env = std::getenv("KSP_PRIM_LDS");   // "0": keep D[] in global memory at every size (tests)
    const bool use_lds = n <= kPrimLdsNodes && !(lds_env && std::strcmp(lds_env, "0") == 0);
    if ((rc = A.alloc(&d_dist, (size_t)nn)) || (rc = A.alloc(&d_prim, prim.size())) || (rc = A.alloc(&d_flags, 2))) return rc;
    KSP_TRY_HIP(hipMemsetAsync(d_flags, 0, sizeof flags, nullptr));
    if (!use_lds && (rc = A.alloc(&d_D, (size_t)n))) return rc;
    if (h_prim && (rc = A.alloc(&d_near, (size_t)n))) return rc;
    {
        KSP_TRY_HIP(launch_row_distances(n, d_rows, d_dist, d_flags));
        KSP_TRY_HIP(hipMemcpy(flags, d_flags, sizeof flags, hipMemcpyDeviceToHost));
        if (ph) ph->mark("k_row_dist+sqrt");
        if (flags[0]) {
            ksp::set_error("single linkage: a distance between two rows is not finite (scipy's linkage refuses it)");
            rc = KSP_E_ARG;
            goto done;
        }
        const size_t lds = use_lds ? (size_t)n * sizeof(double) : 0;
        if (use_lds) KSP_TRY_HIP(hipFuncSetAttribute((const void*)k_prim_single, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k_prim_single, dim3(1), dim3(kPrimThreads), lds, nullptr, d_dist, n, d_D, use_lds ? 1 : 0, d_prim, d_flags + 1, d_near);
        KSP_TRY_HIP(hipGetLastError());
        KSP_TRY_HIP(hipMemcpy(prim.data(), d_prim, prim.size() * sizeof(double), hipMemcpyDeviceToHost));
        KSP_TRY_HIP(hipMemcpy(flags, d_flags, sizeof flags, hipMemcpyDeviceToHost));
        if (h_prim) KSP_TRY_HIP(hipMemcpy(near.data(), d_near, (u64)n * sizeof(u32), hipMemcpyDeviceToHost));
        if (ph) ph->mark("k_prim_single");
    }
    if (flags[1] || (h_Z && !relabel(n, prim, h_Z))) {
        ksp::set_error("single linkage: Prim found no next node (a distance is not finite)");
        rc = KSP_E_ARG;
        goto done;
    }
    if (h_prim)
        for (u64 k = 0; k + 1 < n; ++k) {
            const u32 y = (u32)prim[3 * k + 1];
            if (y >= n) { ksp::set_error("single linkage: Prim found no next node"); rc = KSP_E_ARG; goto done; }
            for (int c = 0; c < 3; ++c) h_prim[4 * k + c] = prim[3 * k + c];
            h_prim[4 * k + 3] = (double)near[y];
        }
done:
    return rc;
}

// ---- host side ------------------------------------------------------------------------------------------------------

// pandas' precise_xstrtod (the default float parser of read_csv): up to 17 significant digits accumulated as a
// double, then ONE multiplication or division by a correctly rounded power of ten — not correctly rounded.
const double* pow10_table() {
    static const std::vector<double> e = [] {
        std::vector<double> v(309);
        for (int i = 0; i <= 308; ++i) v[i] = std::strtod(("1e" + std::to_string(i)).c_str(), nullptr);
        return v;
    }();
    return e.data();
}

bool csv_float(const char* s, double* out) {
    const double* E = pow10_table();
    const char* p = s;
    if (!std::strcmp(p, "inf") || !std::strcmp(p, "+inf")) { *out = HUGE_VAL; return true; }
    if (!std::strcmp(p, "-inf")) { *out = -HUGE_VAL; return true; }
    if (!std::strcmp(p, "nan")) { *out = std::nan(""); return true; }
    bool neg = false;
    if (*p == '-' || *p == '+') neg = *p++ == '-';
    double num = 0.0;
    int nd = 0, ex = 0;
    while (*p >= '0' && *p <= '9') {
        if (nd < 17) { num = num * 10.0 + (*p - '0'); ++nd; } else ++ex;
        ++p;
    }
    if (*p == '.') {
        ++p;
        int ndec = 0;
        while (nd < 17 && *p >= '0' && *p <= '9') { num = num * 10.0 + (*p - '0'); ++p; ++nd; ++ndec; }
        while (*p >= '0' && *p <= '9') ++p;
        ex -= ndec;
    }
    if (nd == 0) return false;
    if (*p == 'e' || *p == 'E') {
        ++p;
        bool en = false;
        if (*p == '-' || *p == '+') en = *p++ == '-';
        int n = 0, k = 0;
        while (k < 17 && *p >= '0' && *p <= '9') { n = n * 10 + (*p - '0'); ++p; ++k; }
        if (k == 0) return false;
        ex += en ? -n : n;
    }
    if (*p) return false;
    if (ex > 308) num = HUGE_VAL;
    else if (ex > 0) num *= E[ex];
    else if (ex < -308) num = ex < -616 ? 0.0 : num / E[-308 - ex] / E[308];
    else num /= E[-ex];
    *out = neg ? -num : num;
    return true;
}

// the matrix value of a cell: the text to_csv writes for 1 - v, as read_csv reads it back
double cell_value(double v, char* buf) {
    const int n = ksp::format_py_repr(buf, 1 - v);
    buf[n] = 0;
    double m = 0;
    csv_float(buf, &m);
    return m;
}

bool is_blank(char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == '\v' || c == '\f'; }
void strip(const char*& b, const char*& e) {
    while (b < e && is_blank(*b)) ++b;
    while (e > b && is_blank(e[-1])) --e;
}
bool py_int(const char* b, const char* e, long long& v) {   // int(text)
    strip(b, e);
    if (b == e) return false;
    std::string s(b, e);
    char* end = nullptr;
    errno = 0;
    v = std::strtoll(s.c_str(), &end, 10);
    return !errno && end && *end == 0;
}
bool py_float(const char* b, const char* e, double& v) {   // float(text)
    strip(b, e);
    if (b == e) return false;
    std::string s(b, e);
    char* end = nullptr;
    v = std::strtod(s.c_str(), &end);
    return end && *end == 0;
}

std::string read_file(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error("cannot open " + path);
    std::ostringstream ss;
    ss << f.rdbuf();
    return ss.str();
}

int pool_size() { return (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency())); }

// f(t) for t = 0..P-1, one thread each (P <= 16); the first exception is rethrown after all have ended
template <class F>
void run_pieces(size_t P, F&& f) {
    if (P <= 1) { if (P) f((size_t)0); return; }
    std::vector<std::thread> th;
    std::vector<std::exception_ptr> err(P);
    for (size_t t = 0; t < P; ++t)
        th.emplace_back([&, t] {
            try { f(t); } catch (...) { err[t] = std::current_exception(); }
        });
    for (auto& x : th) x.join();
    for (auto& e : err)
        if (e) std::rethrow_exception(e);
}

// f(begin, end) over [0, n) cut into at most 16 ranges
template <class F>
void parallel_for(size_t n, F&& f) {
    const size_t T = std::min<size_t>((size_t)pool_size(), std::max<size_t>(1, n / 1024));
    run_pieces(T, [&](size_t t) { f(n * t / T, n * (t + 1) / T); });
}

// the lines after the first of a text, as [begin, end) offsets (a last line without '\n' counts), cut at line ends
// into pieces parsed on the pool; out[i] is what parse() made of line i
template <class T, class P>
std::vector<T> parse_lines(const std::string& text, P&& parse) {
    const size_t first = text.find('\n');
    const size_t b0 = first == std::string::npos ? text.size() : first + 1;
    const size_t len = text.size() - b0;
    const size_t NP = std::min<size_t>((size_t)pool_size(), std::max<size_t>(1, len / (1 << 20)));
    std::vector<size_t> cut(NP + 1, text.size());
    cut[0] = b0;
    for (size_t t = 1; t < NP; ++t) {
        size_t c = std::max(cut[t - 1], b0 + len * t / NP);
        while (c < text.size() && c > b0 && text[c - 1] != '\n') ++c;
        cut[t] = c;
    }
    std::vector<std::vector<T>> part(NP);
    run_pieces(NP, [&](size_t t) {
        size_t b = cut[t];
        while (b < cut[t + 1]) {
            size_t e = text.find('\n', b);
            if (e == std::string::npos || e > cut[t + 1]) e = cut[t + 1];
            part[t].push_back(parse(text.data() + b, text.data() + e));
            b = e + 1;
        }
    });
    std::vector<T> out;
    size_t total = 0;
    for (auto& p : part) total += p.size();
    out.reserve(total);
    for (auto& p : part) out.insert(out.end(), p.begin(), p.end());
    return out;
}

struct Row {
    u32 id1, id2;   // index into the .namesMap rows (by id text)
    double v;
};

// a field as csv's QUOTE_MINIMAL writes it with sep '\t' (names hold no blanks: .namesMap is split on them)
std::string csv_field(const std::string& s) {
    if (s.find('"') == std::string::npos) return s;
    std::string q = "\"";
    for (char c : s) {
        q += c;
        if (c == '"') q += '"';
    }
    return q + "\"";
}

struct Refusal : std::runtime_error {
    int code;
    Refusal(int c, const std::string& s) : std::runtime_error(s), code(c) {}
};

// the (sorted) tree text of a linkage matrix: to_tree + get_newick of ks_export.py, without recursion
std::string newick_text(u32 n, const double* Z, const std::vector<std::string>& names) {
    std::string out;
    char buf[64];
    struct Op { u32 node; double parent_h; int kind; };   // kind 0: node, 1: "(", 2: ",", 3: tail of node
    const u32 root = 2 * n - 2;
    auto height = [&](u32 v) { return Z[4 * (u64)(v - n) + 2]; };
    std::vector<Op> st{{root, height(root), 0}};
    while (!st.empty()) {
        const Op op = st.back();
        st.pop_back();
        if (op.kind == 1) { out += '('; continue; }
        if (op.kind == 2) { out += ','; continue; }
        if (op.kind == 3) {
            if (op.node == root) out += ");";
            else { std::snprintf(buf, sizeof buf, "):%.2f", op.parent_h - height(op.node)); out += buf; }
            continue;
        }
        if (op.node < n) {
            std::snprintf(buf, sizeof buf, ":%.2f", op.parent_h - 0.0);
            out += names[op.node];
            out += buf;
            continue;
        }
        const double h = height(op.node);
        const u32 left = (u32)Z[4 * (u64)(op.node - n)], right = (u32)Z[4 * (u64)(op.node - n) + 1];
        st.push_back({op.node, op.parent_h, 3});
        st.push_back({left, h, 0});
        st.push_back({0, 0, 2});
        st.push_back({right, h, 0});
        st.push_back({0, 0, 1});
    }
    return out;
}

int export_impl(const std::string& prefix, const std::string& dt, bool newick, const std::string& out_prefix) {
    int col;
    if (dt == "min_cont") col = 3;
    else if (dt == "avg_cont") col = 4;
    else if (dt == "max_cont") col = 5;
    else if (dt == "ani") col = 0;
    else throw Refusal(KSP_E_ARG, "unknown distance '" + dt + "' (min_cont, avg_cont, max_cont, ani)");
    Phases ph;
    if (const char* e = std::getenv("KSP_EXPORT_TIMES")) ph.on = *e && std::strcmp(e, "0") != 0;
    std::string base = prefix;
    if (const size_t sl = base.rfind('/'); sl != std::string::npos) base = base.substr(sl + 1);
    const std::string out_pw = out_prefix.empty() ? "kSpider_" + base + "_pairwise.tsv" : out_prefix + "_pairwise.tsv";
    const std::string out_dm = out_prefix.empty() ? "kSpider_" + base + "_distmat.tsv" : out_prefix + "_distmat.tsv";
    const std::string out_nw = out_prefix.empty() ? "kSpider_" + base + ".newick" : out_prefix + ".newick";

    // ---- parse ----
    {   // _kSpider_seqToKmersNo.tsv: there, and every row "<x>\t<id>\t<int>" (ks_export.py reads it, uses nothing)
        const std::string path = prefix + "_kSpider_seqToKmersNo.tsv";
        const std::string text = read_file(path);
        auto ok = parse_lines<char>(text, [](const char* b, const char* e) -> char {
            strip(b, e);
            const char* t1 = std::find(b, e, '\t');
            const char* t2 = t1 == e ? e : std::find(t1 + 1, e, '\t');
            long long n;
            return t1 != e && t2 != e && std::find(t2 + 1, e, '\t') == e && py_int(t2 + 1, e, n);
        });
        if (text.empty()) throw std::runtime_error(path + " is empty");
        for (char c : ok)
            if (!c) throw std::runtime_error("malformed row in " + path);
    }
    // PREFIX.namesMap: after the count line, "<id> <name>" split on blanks; the reference keys its dict by the id's
    // TEXT, so a pairwise id is looked up as text too ('01' is not '1'); a later row of the same id replaces the name
    std::vector<std::string> id_text, name_of;
    std::unordered_map<std::string_view, u32> id_index;
    {
        const std::string path = prefix + ".namesMap";
        const std::string text = read_file(path);
        std::unordered_map<std::string, u32> seen;
        size_t b = text.find('\n');
        while (b != std::string::npos && b + 1 < text.size()) {   // (a trailing '\n' ends the last line, as in Python)
            size_t e = text.find('\n', b + 1);
            if (e == std::string::npos) e = text.size();
            const char *p = text.data() + b + 1, *q = text.data() + e;
            b = e;
            std::vector<std::string> tok;
            while (p < q) {
                while (p < q && is_blank(*p)) ++p;
                const char* t = p;
                while (p < q && !is_blank(*p)) ++p;
                if (p > t) tok.emplace_back(t, p);
            }
            if (tok.size() < 2) throw std::runtime_error("malformed row in " + path);
            auto it = seen.find(tok[0]);
            if (it != seen.end()) { name_of[it->second] = tok[1]; continue; }
            seen.emplace(tok[0], (u32)id_text.size());
            id_text.push_back(tok[0]);
            name_of.push_back(tok[1]);
        }
        if (id_text.size() >= 0xFFFFFFFFull) throw std::runtime_error(path + ": too many rows");
        for (u32 i = 0; i < id_text.size(); ++i) id_index.emplace(std::string_view(id_text[i]), i);
    }
    std::vector<Row> rows;
    {
        const std::string path = prefix + "_kSpider_pairwise.tsv";
        const std::string text = read_file(path);
        const int c = col;
        rows = parse_lines<Row>(text, [c, &id_index](const char* b, const char* e) -> Row {
            strip(b, e);
            const char* f[7];
            int nf = 0;
            f[nf++] = b;
            for (const char* p = b; p < e && nf < 7; ++p)
                if (*p == '\t') f[nf++] = p + 1;
            auto end_of = [&](int i) { return i + 1 < nf ? f[i + 1] - 1 : e; };
            Row r{0, 0, 0};
            if (nf < 2) throw std::runtime_error("malformed row in _kSpider_pairwise.tsv");
            for (int k = 0; k < 2; ++k) {   // (the ids first, then the value: the reference's order)
                const std::string_view id(f[k], (size_t)(end_of(k) - f[k]));
                const auto it = id_index.find(id);
                if (it == id_index.end())
                    throw Refusal(KSP_E_ARG, "pairwise row names id '" + std::string(id) + "', which .namesMap does not have");
                (k ? r.id2 : r.id1) = it->second;
            }
            if (c && !(nf > c && py_float(f[c], end_of(c), r.v))) throw std::runtime_error("malformed row in _kSpider_pairwise.tsv");
            return r;
        });
        if (col == 0) {
            const std::string apath = prefix + "_kSpider_pairwise.ani_col.tsv";
            std::ifstream probe(apath);
            if (!probe) throw Refusal(KSP_E_IO, "ANI was selected, but " + apath + " was not found");
            probe.close();
            const std::string atext = read_file(apath);
            std::vector<double> ani = parse_lines<double>(atext, [](const char* b, const char* e) -> double {
                double v;
                if (!py_float(b, e, v)) throw std::runtime_error("malformed row in _kSpider_pairwise.ani_col.tsv");
                return v;
            });
            if (ani.size() < rows.size()) throw std::runtime_error(apath + " has fewer rows than the pairwise TSV");
            for (size_t i = 0; i < rows.size(); ++i) rows[i].v = ani[i];
        }
    }
    const u64 E = rows.size();
    // nodes: the names that occur, sorted (byte order = Python's order of str for UTF-8); pos_of[.namesMap row]
    std::vector<u32> pos_of(name_of.size(), 0xFFFFFFFFu);
    std::vector<std::string> nodes;
    {
        std::vector<char> used(name_of.size(), 0);
        for (const Row& r : rows) used[r.id1] = used[r.id2] = 1;
        for (size_t i = 0; i < name_of.size(); ++i)
            if (used[i]) nodes.push_back(name_of[i]);
        std::sort(nodes.begin(), nodes.end());
        nodes.erase(std::unique(nodes.begin(), nodes.end()), nodes.end());
        for (size_t i = 0; i < name_of.size(); ++i)
            if (used[i]) pos_of[i] = (u32)(std::lower_bound(nodes.begin(), nodes.end(), name_of[i]) - nodes.begin());
    }
    const u32 N = (u32)nodes.size();
    // CSR by node position: the other end and the row of every cell, in column order
    std::vector<u64> off((u64)N + 1, 0);
    std::vector<u32> other(2 * E), which(2 * E);
    std::vector<char> real(N, 0);   // the column has an assigned value that is not NaN: float64 (else int64)
    {
        for (const Row& r : rows) {
            const u32 a = pos_of[r.id1], b = pos_of[r.id2];
            if (a == b) throw Refusal(KSP_E_ARG, "pairwise row " + id_text[r.id1] + " " + id_text[r.id2] + " pairs a name with itself");
            ++off[a + 1];
            ++off[b + 1];
            if (r.v == r.v) real[a] = real[b] = 1;
        }
        for (u32 p = 0; p < N; ++p) off[p + 1] += off[p];
        std::vector<u64> cur(off.begin(), off.end() - 1);
        for (u64 e = 0; e < E; ++e) {
            const u32 a = pos_of[rows[e].id1], b = pos_of[rows[e].id2];
            other[cur[a]] = b; which[cur[a]++] = (u32)e;
            other[cur[b]] = a; which[cur[b]++] = (u32)e;
        }
        std::atomic<bool> dup{false};
        parallel_for(N, [&](size_t lo, size_t hi) {
            std::vector<std::pair<u32, u32>> tmp;
            for (size_t p = lo; p < hi; ++p) {
                tmp.clear();
                for (u64 k = off[p]; k < off[p + 1]; ++k) tmp.emplace_back(other[k], which[k]);
                std::sort(tmp.begin(), tmp.end());
                for (size_t k = 0; k < tmp.size(); ++k) {
                    other[off[p] + k] = tmp[k].first;
                    which[off[p] + k] = tmp[k].second;
                    if (k && tmp[k].first == tmp[k - 1].first) dup = true;
                }
            }
        });
        if (dup) throw Refusal(KSP_E_ARG, "the pairwise TSV holds a pair of names twice");
    }
    ph.mark("parse");

    // ---- newick: checks first, then the device ----
    std::vector<double> Z;
    if (newick) {
        if (N < 2) throw Refusal(KSP_E_ARG, "--newick needs at least 2 nodes, the pairwise TSV names " + std::to_string(N));
        if (N > kMaxNodes)
            throw Refusal(KSP_E_LIMIT, "--newick: " + std::to_string(N) + " nodes, above the limit of " + std::to_string(kMaxNodes) +
                                           " (two N x N double matrices on the device)");
        std::vector<double> m(E);
        std::atomic<bool> bad{false};
        parallel_for(E, [&](size_t lo, size_t hi) {
            char buf[40];
            for (size_t e = lo; e < hi; ++e) {
                const double v = rows[e].v;
                m[e] = v == v ? cell_value(v, buf) : 0.0;
                if (!std::isfinite(m[e])) bad = true;
            }
        });
        if (bad) throw Refusal(KSP_E_ARG, "--newick: a distance 1 - value is not finite (scipy's linkage refuses it)");
        if (int rc = ksp::set_device("kspider_export", ksp::device_from_env())) throw Refusal(rc, ksp_last_error());
        const u64 nn = (u64)N * N;
        u64 fr = 0;
        if (ksp::device_fits("kspider_export", 2 * nn * sizeof(double) + E * 16 + ((u64)N * 4 + 64) * sizeof(double), "", &fr))
            throw Refusal(KSP_E_LIMIT, "--newick: the two " + std::to_string(N) + " x " + std::to_string(N) +
                                           " double matrices do not fit the device's free memory (" + std::to_string(fr >> 20) + " MiB)");
        int rc = KSP_OK;
        ksp::DeviceArena A;
        double *d_M = nullptr, *d_m = nullptr;
        u32 *d_p = nullptr, *d_q = nullptr;
        Z.resize(4 * (u64)(N - 1));
        {
            std::vector<u32> p(E), q(E);
            for (u64 e = 0; e < E; ++e) { p[e] = pos_of[rows[e].id1]; q[e] = pos_of[rows[e].id2]; }
            if ((rc = A.alloc(&d_M, (size_t)nn))) goto done;
            KSP_TRY_HIP(hipMemsetAsync(d_M, 0, nn * sizeof(double), nullptr));
            if (E) {
                if ((rc = ksp::upload_pairs(A, p.data(), q.data(), E, &d_p, &d_q)) || (rc = A.alloc(&d_m, (size_t)E))) goto done;
                KSP_TRY_HIP(hipMemcpy(d_m, m.data(), E * 8, hipMemcpyHostToDevice));
                hipLaunchKernelGGL(k_scatter, dim3((unsigned)std::min<u64>((E + 255) / 256, 8192)), dim3(256), 0, nullptr, d_p, d_q, d_m, E, N, d_M);
                KSP_TRY_HIP(hipGetLastError());
                KSP_TRY_HIP(A.release(d_p));   // (the cells are in the matrix: the distance matrix gets their room)
                KSP_TRY_HIP(A.release(d_q));
                KSP_TRY_HIP(A.release(d_m));
            }
            if (ph.on) { KSP_TRY_HIP(hipDeviceSynchronize()); ph.mark("h2d+scatter"); }
            rc = single_linkage_on_device(N, d_M, Z.data(), nullptr, &ph);
        }
    done:
        if (rc) throw Refusal(rc, ksp_last_error());
    }

    // ---- text outputs ----
    std::ofstream f_pw, f_dm, f_nw;
    ksp::PartialFiles files;
    {   // named pairwise TSV, in row order
        std::ofstream& f = f_pw;
        files.open(out_pw, f);
        f << (col == 0 ? std::string("source1\tsource2\tani\n") : "grp1\tgrp2\t" + dt + "\n");
        const u64 B = 1 << 20;
        for (u64 b0 = 0; b0 < E; b0 += B) {
            const u64 b1 = std::min(E, b0 + B);
            std::vector<std::string> part(pool_size());
            const size_t P = part.size();
            run_pieces(P, [&](size_t t) {
                char buf[40];
                std::string& s = part[t];
                for (u64 e = b0 + (b1 - b0) * t / P; e < b0 + (b1 - b0) * (t + 1) / P; ++e) {
                    s += name_of[rows[e].id1];
                    s += '\t';
                    s += name_of[rows[e].id2];
                    s += '\t';
                    s.append(buf, (size_t)ksp::format_py_repr(buf, rows[e].v));
                    s += '\n';
                }
            });
            for (auto& s : part) f.write(s.data(), (std::streamsize)s.size());
        }
    }
    {   // distance matrix, row by row from the CSR
        std::ofstream& f = f_dm;
        files.open(out_dm, f);
        std::string head;
        for (u32 p = 0; p < N; ++p) { head += '\t'; head += csv_field(nodes[p]); }
        head += '\n';
        f.write(head.data(), (std::streamsize)head.size());
        const u32 B = 512;
        std::vector<std::string> text(B);
        for (u32 r0 = 0; r0 < N; r0 += B) {
            const u32 r1 = std::min(N, r0 + B);
            parallel_for((size_t)(r1 - r0) * 1024, [&](size_t lo, size_t hi) {   // (a range of rows per thread)
                char buf[40];
                for (u32 p = r0 + (u32)(lo / 1024); p < r0 + (u32)(hi / 1024); ++p) {
                    std::string& s = text[p - r0];
                    s.clear();
                    s += csv_field(nodes[p]);
                    u64 k = off[p];
                    for (u32 q = 0; q < N; ++q) {
                        s += '\t';
                        double v = NAN;
                        if (k < off[p + 1] && other[k] == q) v = rows[which[k++]].v;
                        if (v == v) s.append(buf, (size_t)ksp::format_py_repr(buf, 1 - v));
                        else if (real[q]) s += "0.0";
                        else s += '0';
                    }
                    s += '\n';
                }
            });
            for (u32 i = 0; i < r1 - r0; ++i) f.write(text[i].data(), (std::streamsize)text[i].size());
        }
    }
    ph.mark("text outputs");
    if (newick) {
        files.open(out_nw, f_nw);
        const std::string t = newick_text(N, Z.data(), nodes);
        f_nw.write(t.data(), (std::streamsize)t.size());
        ph.mark("newick");
    }
    files.commit();
    if (ph.on) std::fprintf(stderr, "kspider_export: N %u, rows %llu: %s\n", N, (unsigned long long)E, ph.text.c_str());
    return KSP_OK;
}

}  // namespace

extern "C" int ksp_csv_float(const char* text, double* out) {
    if (!text || !out) { ksp::set_error("ksp_csv_float: NULL argument"); return KSP_E_ARG; }
    if (!csv_float(text, out)) { ksp::set_error(std::string("ksp_csv_float: not a number: ") + text); return KSP_E_ARG; }
    return KSP_OK;
}

namespace {
// the checks of the device entry points, in this order, then run() on the selected device
template <class F>
int linkage_entry(const char* who, int device, uint32_t n, const double* d_rows, bool has_output, F&& run) {
    if (n > kMaxNodes) { ksp::set_error(std::string(who) + ": n above the limit of 65536"); return KSP_E_LIMIT; }
    if (n < 2 || !d_rows || !has_output) { ksp::set_error(std::string(who) + ": n < 2 or NULL argument"); return KSP_E_ARG; }
    if (int rc = ksp::set_device(who, device)) return rc;
    if (ksp::device_fits(who, (u64)n * n * sizeof(double) + ((u64)n * 4 + 64) * sizeof(double), "")) {
        ksp::set_error(std::string(who) + ": the n x n distance matrix does not fit the device's free memory");
        return KSP_E_LIMIT;
    }
    try {
        return run();
    } catch (const std::bad_alloc&) {
        ksp::set_error(std::string(who) + ": out of host memory");
        return KSP_E_LIMIT;
    }
}

int row_distances_on_device(u32 n, const double* d_rows, double* h_dist) {
    int rc = KSP_OK;
    ksp::DeviceArena A;
    double* d_dist = nullptr;
    u32* d_flag = nullptr;
    u32 flag = 0;
    if ((rc = A.alloc(&d_dist, (size_t)n * n)) || (rc = A.alloc(&d_flag, 1))) return rc;
    KSP_TRY_HIP(hipMemsetAsync(d_flag, 0, sizeof flag, nullptr));
    KSP_TRY_HIP(launch_row_distances(n, d_rows, d_dist, d_flag));
    KSP_TRY_HIP(hipMemcpy(&flag, d_flag, sizeof flag, hipMemcpyDeviceToHost));
    if (flag) {
        ksp::set_error("row distances: a distance between two rows is not finite (scipy's linkage refuses it)");
        rc = KSP_E_ARG;
        goto done;
    }
    KSP_TRY_HIP(hipMemcpy(h_dist, d_dist, (u64)n * n * sizeof(double), hipMemcpyDeviceToHost));
done:
    return rc;
}
}  // namespace

extern "C" int ksp_single_linkage_rows(int device, uint32_t n, const double* d_rows, double* h_Z) {
    return linkage_entry("ksp_single_linkage_rows", device, n, d_rows, h_Z != nullptr,
                         [&] { return single_linkage_on_device(n, d_rows, h_Z, nullptr, nullptr); });
}

extern "C" int ksp_single_linkage_prim(int device, uint32_t n, const double* d_rows, double* h_prim) {
    return linkage_entry("ksp_single_linkage_prim", device, n, d_rows, h_prim != nullptr,
                         [&] { return single_linkage_on_device(n, d_rows, nullptr, h_prim, nullptr); });
}

extern "C" int ksp_row_distances(int device, uint32_t n, const double* d_rows, double* h_dist) {
    return linkage_entry("ksp_row_distances", device, n, d_rows, h_dist != nullptr,
                         [&] { return row_distances_on_device(n, d_rows, h_dist); });
}

extern "C" int kspider_export(const char* index_prefix, const char* dist_type, int newick, const char* out_prefix) {
    if (!index_prefix) { ksp::set_error("kspider_export: index_prefix is NULL"); return KSP_E_ARG; }
    try {
        return export_impl(index_prefix, dist_type && *dist_type ? dist_type : "max_cont", newick != 0, out_prefix ? out_prefix : "");
    } catch (const Refusal& r) {
        ksp::set_error(std::string("kspider_export: ") + r.what());
        return r.code;
    } catch (const std::bad_alloc&) {
        ksp::set_error("kspider_export: out of host memory");
        return KSP_E_LIMIT;
    } catch (const std::exception& e) {
        ksp::set_error(std::string("kspider_export: ") + e.what());
        return KSP_E_IO;
    }
}
