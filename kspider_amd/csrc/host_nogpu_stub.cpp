// Sanitizer build of the HOST side only (make asan): the file parsers and TSV writers are compiled with
// -fsanitize=address,undefined and linked against this stub instead of the HIP engine, so that a CPU test can
// feed them malformed files (tests/test_host_hardening_cpu.py).  Every compute entry fails with KSP_E_HIP —
// there is no CPU implementation of the hot path, here or anywhere else in the product.
#include <cstdlib>
#include <string>

#include "../../include/kspider_amd.h"
#include "engine_internal.h"

namespace ksp {
static thread_local std::string g_error;
void set_error(const std::string& s) { g_error = s; }
}  // namespace ksp

namespace ksp {
int pairwise_postings_multi_cc(const uint64_t*, const uint32_t*, const uint32_t*, uint32_t, uint32_t, const int*, int, ksp_edge**,
                               uint64_t*, ksp_stats*, AfterJoin*) {
    set_error("host-only sanitizer build: no HIP engine");
    return KSP_E_HIP;
}
void cc_critical(double, float* vcrit, int* mode) { *vcrit = 0; *mode = 0; }
void read_names_map(const std::string&, std::vector<std::string>& name_of) { name_of.clear(); }
void write_cluster_file(const std::string&, double, const std::vector<uint32_t>&, const std::vector<std::string>&) {}
bool repr_text_passes(float, double) { return false; }
void write_sweep_outputs(const std::string&, const std::string&, const double*, uint32_t, const uint32_t*, const uint64_t*,
                         const std::vector<std::string>&) {}
void write_tree_files(const std::string&, const std::string&, std::vector<TreeRow>&, const std::vector<std::string>&, bool) {}
void write_repr_file(const std::string&, const std::vector<uint32_t>&, const uint32_t*, const uint32_t*, uint64_t) {}
void write_derep_file(const std::string&, const std::string&, const std::vector<DerepRow>&, const std::vector<std::string>&) {}
void write_topk_file(const std::string&, const std::string&, const std::vector<std::string>&, const std::vector<uint32_t>&, const std::vector<uint32_t>&,
                     const std::vector<std::string>&) {}
void write_report_files(const std::string&, const std::string&, double, const std::vector<ksp_cluster_row>&, const std::vector<ksp_member_row>&,
                        const std::vector<std::string>&, const std::vector<std::string>&) {}
void write_upgma_files(const std::string&, const std::string&, const std::vector<ksp_upgma_row>&, const std::vector<std::string>&, bool) {}
void* pinned_alloc(size_t bytes) { return std::malloc(bytes ? bytes : 1); }
void pinned_free(void* p) { std::free(p); }
}  // namespace ksp

extern "C" {
const char* ksp_last_error(void) { return ksp::g_error.c_str(); }
int ksp_edges_degrees(int, uint32_t, const ksp_edge*, uint64_t, const uint32_t*, int, double, uint32_t*) {
    ksp::set_error("host-only sanitizer build: no HIP engine");
    return KSP_E_HIP;
}
int ksp_edges_repr(int, uint32_t, const ksp_edge*, uint64_t, const uint32_t*, int, double, uint32_t*, uint32_t*, uint32_t*) {
    ksp::set_error("host-only sanitizer build: no HIP engine");
    return KSP_E_HIP;
}
int ksp_repr_critical(double, float*, int*) {
    ksp::set_error("host-only sanitizer build: no HIP engine");
    return KSP_E_HIP;
}
int kspider_repr_sketches(const char*, const char*, double, const char*) {
    ksp::set_error("host-only sanitizer build: no HIP engine");
    return KSP_E_HIP;
}
int ksp_edges_dereplicate(int, uint32_t, const ksp_edge*, uint64_t, const uint32_t*, int, double, uint32_t*, uint32_t*, uint32_t*, uint32_t*, uint32_t*) {
    ksp::set_error("host-only sanitizer build: no HIP engine");
    return KSP_E_HIP;
}
int kspider_dereplicate(const char*, const char*, double, const char*) {
    ksp::set_error("host-only sanitizer build: no HIP engine");
    return KSP_E_HIP;
}
int ksp_edges_topk(int, uint32_t, const ksp_edge*, uint64_t, const uint32_t*, int, uint32_t, uint32_t*, uint32_t*) {
    ksp::set_error("host-only sanitizer build: no HIP engine");
    return KSP_E_HIP;
}
int ksp_topk_ranked(int, uint32_t, const uint32_t*, const uint32_t*, const uint32_t*, uint64_t, uint32_t, uint32_t*, uint32_t*) {
    ksp::set_error("host-only sanitizer build: no HIP engine");
    return KSP_E_HIP;
}
int kspider_topk(const char*, const char*, uint32_t, const char*) {
    ksp::set_error("host-only sanitizer build: no HIP engine");
    return KSP_E_HIP;
}
int ksp_cluster_report_valued(int, uint32_t, const uint32_t*, const uint32_t*, const float*, uint64_t, ksp_cluster_row*, uint32_t*, ksp_member_row*) {
    ksp::set_error("host-only sanitizer build: no HIP engine");
    return KSP_E_HIP;
}
int ksp_edges_cut(int, const ksp_edge*, uint64_t, const uint32_t*, int, double, ksp_edge*, uint64_t*) {
    ksp::set_error("host-only sanitizer build: no HIP engine");
    return KSP_E_HIP;
}
int ksp_pairwise_host_cut(const uint64_t*, const uint32_t*, const uint64_t*, uint32_t, const uint32_t*, int, double, const int*, int, ksp_edge**,
                          uint64_t*, uint64_t*, ksp_stats*) {
    ksp::set_error("host-only sanitizer build: no HIP engine");
    return KSP_E_HIP;
}
int ksp_edges_tsv(int, uint32_t, const ksp_edge*, uint64_t, const uint32_t*, const uint32_t*, char*, uint64_t, uint64_t*) {
    ksp::set_error("host-only sanitizer build: no HIP engine");
    return KSP_E_HIP;
}
int ksp_debug_format_floats(int, const float*, uint64_t, char*, uint32_t*) {
    ksp::set_error("host-only sanitizer build: no HIP engine");
    return KSP_E_HIP;
}
int ksp_debug_tsv_records(int, uint32_t, uint64_t, uint64_t, ksp_edge*, uint32_t*, uint32_t*) {
    ksp::set_error("host-only sanitizer build: no HIP engine");
    return KSP_E_HIP;
}
int ksp_debug_tsv_times(int, uint32_t, const ksp_edge*, uint64_t, const uint32_t*, const uint32_t*, int, int, int, float*) {
    ksp::set_error("host-only sanitizer build: no HIP engine");
    return KSP_E_HIP;
}
int ksp_query_host(const uint64_t*, const uint64_t*, uint32_t, const uint64_t*, const uint64_t*, uint32_t, int, int, ksp_edge**, uint64_t*, ksp_query_stats*) {
    ksp::set_error("host-only sanitizer build: no HIP engine");
    return KSP_E_HIP;
}
int ksp_gather_host(const uint64_t*, const uint64_t*, uint32_t, const uint64_t*, const uint64_t*, uint32_t, uint32_t, uint32_t, int, ksp_gather_row**, uint64_t*,
                    ksp_gather_stats*) {
    ksp::set_error("host-only sanitizer build: no HIP engine");
    return KSP_E_HIP;
}
int ksp_gather_device(int, const uint64_t*, const uint64_t*, uint32_t, const uint64_t*, const uint64_t*, uint32_t, uint32_t, uint32_t, ksp_gather_row*, uint64_t, uint64_t*,
                      ksp_gather_stats*) {
    ksp::set_error("host-only sanitizer build: no HIP engine");
    return KSP_E_HIP;
}
int ksp_sketch_host(int, const uint8_t*, uint64_t, const uint64_t*, uint32_t, int, uint64_t, uint32_t, uint64_t**, uint64_t*, ksp_sketch_stats*) {
    ksp::set_error("host-only sanitizer build: no HIP engine");
    return KSP_E_HIP;
}
int ksp_sketch_host_abund(int, const uint8_t*, uint64_t, const uint64_t*, uint32_t, int, uint64_t, uint32_t, uint64_t**, uint32_t**, uint64_t*, ksp_sketch_stats*) {
    ksp::set_error("host-only sanitizer build: no HIP engine");
    return KSP_E_HIP;
}
int ksp_sketch_host_mol(int, const uint8_t*, uint64_t, const uint64_t*, uint32_t, int, int, uint64_t, uint64_t, uint32_t, uint64_t**, uint32_t**, uint64_t*, ksp_sketch_stats*) {
    ksp::set_error("host-only sanitizer build: no HIP engine");
    return KSP_E_HIP;
}
int ksp_gather_abund_host(const uint64_t*, const uint64_t*, uint32_t, const uint64_t*, const uint32_t*, const uint64_t*, uint32_t, uint32_t, uint32_t, int, ksp_gather_wrow**,
                          uint64_t*, ksp_gather_stats*) {
    ksp::set_error("host-only sanitizer build: no HIP engine");
    return KSP_E_HIP;
}
int ksp_gather_abund_device(int, const uint64_t*, const uint64_t*, uint32_t, const uint64_t*, const uint32_t*, const uint64_t*, uint32_t, uint32_t, uint32_t, ksp_gather_wrow*,
                            uint64_t, uint64_t*, ksp_gather_stats*) {
    ksp::set_error("host-only sanitizer build: no HIP engine");
    return KSP_E_HIP;
}
int ksp_compare_host(const uint64_t*, const uint32_t*, const uint64_t*, uint32_t, const uint64_t*, const uint32_t*, const uint64_t*, uint32_t, int, int, ksp_wedge**, uint64_t*,
                     uint64_t*, uint64_t*, ksp_compare_stats*) {
    ksp::set_error("host-only sanitizer build: no HIP engine");
    return KSP_E_HIP;
}
int ksp_compare_device(int, const uint64_t*, const uint32_t*, const uint64_t*, uint32_t, const uint64_t*, const uint32_t*, const uint64_t*, uint32_t, int, ksp_wedge*, uint64_t,
                       uint64_t*, uint64_t*, uint64_t*, ksp_compare_stats*) {
    ksp::set_error("host-only sanitizer build: no HIP engine");
    return KSP_E_HIP;
}
int ksp_classify_open(int, int, uint64_t, uint32_t, const uint64_t*, const uint64_t*, uint32_t, ksp_classify**) {
    ksp::set_error("host-only sanitizer build: no HIP engine");
    return KSP_E_HIP;
}
int ksp_classify_add(ksp_classify*, const uint8_t*, uint64_t, const uint64_t*, const uint32_t*, uint32_t) {
    ksp::set_error("host-only sanitizer build: no HIP engine");
    return KSP_E_HIP;
}
int ksp_classify_finish(ksp_classify*, uint32_t, uint32_t, ksp_classify_row**, uint64_t*, uint32_t*, uint32_t*, uint32_t*, uint32_t*, uint32_t*, uint32_t*, ksp_classify_stats*) {
    ksp::set_error("host-only sanitizer build: no HIP engine");
    return KSP_E_HIP;
}
void ksp_classify_close(ksp_classify*) {}
void ksp_free(void* p) { std::free(p); }
int ksp_engine_lists_path(const ksp_engine*, int*) {
    ksp::set_error("host-only sanitizer build: no HIP engine");
    return KSP_E_HIP;
}
int ksp_pairwise_host_multi(const uint64_t*, const uint32_t*, const uint64_t*, uint32_t, const int*, int, ksp_edge**,
                            uint64_t*, ksp_stats*) {
    ksp::set_error("host-only sanitizer build: no HIP engine");
    return KSP_E_HIP;
}
int ksp_pairwise_postings_host_multi(const uint64_t*, const uint32_t*, const uint32_t*, uint32_t, uint32_t, const int*, int,
                                     ksp_edge**, uint64_t*, ksp_stats*) {
    ksp::set_error("host-only sanitizer build: no HIP engine");
    return KSP_E_HIP;
}
}
