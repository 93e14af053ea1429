// Connected components by min-label hooking + pointer jumping over an edge list in device memory (every parent[] only ever
// decreases, parent[v] <= v): when nothing changes any more every tree is a star whose root is the smallest node of its
// component.  Shared by the clustering (cluster.hip) and the cut-off ladder (sweep.hip); each includes its own copy.
#ifndef KSPIDER_CC_KERNELS_HIP_H
#define KSPIDER_CC_KERNELS_HIP_H
#include <cstdint>

#include <hip/hip_runtime.h>

namespace {

__global__ void k_cc_init(uint32_t* __restrict__ parent, uint32_t n) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v < n) parent[v] = v;
}
// one pass over the edges: the larger of the two labels is lowered to the smaller one
__global__ void k_cc_hook(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, uint64_t m, uint32_t* __restrict__ parent,
                          uint32_t* __restrict__ changed) {
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < m; e += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t pu = parent[a[e]], pv = parent[b[e]];
        if (pu == pv) continue;
        const uint32_t hi = pu > pv ? pu : pv, lo = pu > pv ? pv : pu;
        if (atomicMin(&parent[hi], lo) > lo) *changed = 1;
    }
}
__global__ void k_cc_jump(uint32_t* __restrict__ parent, uint32_t n, uint32_t* __restrict__ changed) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    const uint32_t p = parent[v], gp = parent[p];
    if (gp != p) { parent[v] = gp; *changed = 1; }
}

}  // namespace
#endif
