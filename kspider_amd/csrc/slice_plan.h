// How a multi-device job (run_multi, multi.hip) shares its input out: how many slices, which device builds each, and for an
// inverted index the keys of every slice.  Host arithmetic only, nothing of HIP: the sanitizer build drives it directly
// (host_asan_check plan; tests/test_slice_plan_cpu.py).
#ifndef KSPIDER_SLICE_PLAN_H
#define KSPIDER_SLICE_PLAN_H
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "engine_internal.h"

namespace ksp {

struct SlicePlan {
    std::vector<int> devices;      // the device of every worker: the job's devices, taken round robin when there are more slices
    std::vector<uint32_t> pk_cut;  // postings input in slices: slice s holds the keys [pk_cut[s], pk_cut[s + 1]); empty otherwise
    bool sliced = false;           // stage 1 builds slices that are exchanged and assembled
};

// n entries (sketch input: n_keys and key_off ignored) or memberships (postings input: key_off[n_keys] == n; key_off may be
// NULL without keys) on the nd devices `devices` (1 <= nd <= 64); slices_env: the text of $KSP_SLICES or NULL (it forces a
// slice count: tests).
//
// An input of 2^30 entries or more does not fit one build (32-bit entry positions): it is cut into slices of at most
// ~0.9 * 2^30 entries, more than there are devices if need be (several workers per device).  Sketch input is cut into equal
// shares of the hash range (~equal sizes for hashes), one per device of the job.  An inverted index (the reference's colour ->
// sources map, src/pairwise.cpp:95-111, which has no size limit) is cut into slices of whole keys with fewer than 2^30
// memberships each, one per device of the job, so that every device builds 1 / nd of the colours instead of all of them.
inline int plan_slices(const bool postings, const uint64_t n, const uint32_t n_keys, const uint64_t* key_off, const int* devices,
                       const int nd, const char* slices_env, SlicePlan& plan) {
    const bool big = n >= (1ull << 30);
    plan = SlicePlan();
    plan.devices.assign(devices, devices + nd);
    uint64_t want = big ? n / 900000000ull + 1 : 1;
    if (slices_env) want = std::max<uint64_t>(want, (uint64_t)std::max(1, std::atoi(slices_env)));
    if (postings) {
        want = std::max<uint64_t>(want, (uint64_t)nd);
        if (want > (uint64_t)n_keys && !big) want = 1;   // (fewer colours than slices: every device builds the few there are, the tiles are still shared)
    }
    if (want > 64) {
        set_error(postings ? "pairwise: more than 2^35 colour memberships" : "pairwise_host: more than 2^35 key entries");
        return KSP_E_LIMIT;
    }
    if (want > (uint64_t)nd) {
        plan.devices.clear();
        for (uint64_t i = 0; i < want; ++i) plan.devices.push_back(devices[i % (uint64_t)nd]);
    }
    const uint32_t ns = (uint32_t)plan.devices.size();
    if (!postings) { plan.sliced = ns > 1; return KSP_OK; }
    if (want <= 1) return KSP_OK;   // (without keys always: key_off is not read)
    const char* const too_large = "pairwise: one colour range holds 2^30 memberships or more (a single colour that large?)";
    // More slices than keys happens only from 2^30 memberships on (below, the index is built whole: above).  With one slice
    // more than keys the first slice is empty and every other slice holds one key: two keys of 9 * 10^8 in 3 slices are cut
    // at 0, 0, 1, 2.  With two or more slices too many, the 32-bit "keys left for the later slices" (n_keys - (ns - s)) used to
    // wrap, the clamp did nothing, a later cut fell back to key 0 and the range before it came out negative, that is as 2^64
    // less its size: always refused as too large.  The refusal is spelled out here instead.
    if ((uint64_t)ns > (uint64_t)n_keys + 1) { set_error(too_large); return KSP_E_LIMIT; }
    plan.pk_cut.assign((size_t)ns + 1, 0);
    uint32_t k = 0;
    for (uint32_t s = 1; s < ns; ++s) {   // cut where the memberships reach s / ns of all (whole keys; a key is left for every later slice)
        const uint64_t goal = n / ns * s;
        while (k < n_keys && key_off[k] < goal) ++k;
        k = std::max<uint32_t>(k, plan.pk_cut[(size_t)s - 1] + 1);
        k = std::min<uint32_t>(k, n_keys - (ns - s));   // (ns - s <= ns - 1 <= n_keys: no wrap)
        plan.pk_cut[s] = k;
    }
    plan.pk_cut[ns] = n_keys;
    for (uint32_t s = 0; s < ns; ++s)
        if (key_off[plan.pk_cut[(size_t)s + 1]] - key_off[plan.pk_cut[s]] >= (1ull << 30)) { set_error(too_large); return KSP_E_LIMIT; }
    plan.sliced = true;
    return KSP_OK;
}

}  // namespace ksp
#endif
