// Wave- and grid-level device helpers shared by the kernel files of librlhip.so: the one copy of every helper that more than one
// .hip file needs.  A kernel file pulls them in with `using namespace rlhip_dev;` inside its anonymous namespace.  Helpers that a
// single file uses stay in that file.  gfx950 only: 64-lane wavefronts.
#pragma once
#include "rlhip_internal.h"

namespace rlhip_dev {

// ---- cross-workgroup traffic uses agent-scope relaxed atomics on 8-byte granules (sc1 write-through stores /
//      L1-bypassing loads): no cache-maintenance fences are needed around the rendezvous (guide section 6, G16:
//      "8-B agent atomics both sides"), which keeps a step's single grid barrier at a few microseconds.
template <typename T>
__device__ __forceinline__ void pub_store(T* p, T v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <typename T>
__device__ __forceinline__ T pub_load(const T* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// rendezvous of all workgroups of a persistent launch: `bar` counts arrivals (zeroed by the host), `target` = gridDim.x * epoch
__device__ __forceinline__ void grid_barrier(unsigned* bar, unsigned target) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's published stores have left
    __syncthreads();
    if (threadIdx.x == 0) {
        __hip_atomic_fetch_add(bar, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        while (__hip_atomic_load(bar, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) __builtin_amdgcn_s_sleep(1);
        // one L1 invalidate per step: everything published before the rendezvous was stored write-through (sc1),
        // so after this acquire it can be read with ordinary wide loads
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
    __syncthreads();
}

// sum over the 64 lanes of a wave, result valid in lane 0
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// the same sum, every lane gets it
template <typename T>
__device__ __forceinline__ T wave_allsum(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// v + (v rotated right by n lanes inside each 16-lane row), n = 8, 4, 2 or 1: one DPP step of a row all-reduce at VALU speed
__device__ __forceinline__ double dpp_ror_add(double v, const int n) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    int lo2, hi2;
    switch (n) {   // row_ror:n  (rotate inside each 16-lane row)
        case 1: lo2 = __builtin_amdgcn_update_dpp(0, lo, 0x121, 0xF, 0xF, false); hi2 = __builtin_amdgcn_update_dpp(0, hi, 0x121, 0xF, 0xF, false); break;
        case 2: lo2 = __builtin_amdgcn_update_dpp(0, lo, 0x122, 0xF, 0xF, false); hi2 = __builtin_amdgcn_update_dpp(0, hi, 0x122, 0xF, 0xF, false); break;
        case 4: lo2 = __builtin_amdgcn_update_dpp(0, lo, 0x124, 0xF, 0xF, false); hi2 = __builtin_amdgcn_update_dpp(0, hi, 0x124, 0xF, 0xF, false); break;
        default: lo2 = __builtin_amdgcn_update_dpp(0, lo, 0x128, 0xF, 0xF, false); hi2 = __builtin_amdgcn_update_dpp(0, hi, 0x128, 0xF, 0xF, false); break;
    }
    return v + __hiloint2double(hi2, lo2);
}

// value held by lane l (wave-uniform l; a compile-time constant after unrolling): v_readlane, a scalar
__device__ __forceinline__ float lane_get(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }
__device__ __forceinline__ double lane_get(double v, int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}

}  // namespace rlhip_dev
