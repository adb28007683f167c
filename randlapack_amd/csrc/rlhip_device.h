// Wave- and grid-level device helpers shared by the kernel files of librlhip.so: the one copy of every helper that more than one
// .hip file needs.  A kernel file pulls them in with `using namespace rlhip_dev;` inside its anonymous namespace.  Helpers that a
// single file uses stay in that file.  gfx950 only: 64-lane wavefronts.  One host-side helper lives here too, beside the IntC it is
// built on: rbf_ks_dispatch, which picks the KS instantiation of the fused two-point-set kernels.
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

// ---- the one DPP move: every lane receives x from the lane that the control word CTRL names (v_mov_b32 with a DPP modifier, VALU speed,
//      no LDS crossbar), all rows and banks enabled; a lane whose source falls outside its row gets 0, with or without BOUND_CTRL.
//      The control is an immediate of the instruction, hence a template argument.  64-bit values move as two words, low half first.
constexpr int DPP_QUAD_PERM = 0x000;         // + a | b << 2 | c << 4 | d << 6: lanes 0..3 of every quad take the quad's lanes a, b, c, d
constexpr int DPP_ROW_SHR = 0x110;           // + n (1..15): from n lanes below, inside each 16-lane row
constexpr int DPP_ROW_ROR = 0x120;           // + n (1..15): the same, wrapping around inside the row
constexpr int DPP_ROW_HALF_MIRROR = 0x141;   // lane l of each 8-lane half row takes lane 7 - l
template <int CTRL, bool BOUND_CTRL = false>
__device__ __forceinline__ int dpp_mov(int x) { return __builtin_amdgcn_update_dpp(0, x, CTRL, 0xF, 0xF, BOUND_CTRL); }
template <int CTRL, bool BOUND_CTRL = false>
__device__ __forceinline__ unsigned dpp_mov(unsigned x) { return (unsigned)dpp_mov<CTRL, BOUND_CTRL>((int)x); }
template <int CTRL, bool BOUND_CTRL = false>
__device__ __forceinline__ float dpp_mov(float x) { return __int_as_float(dpp_mov<CTRL, BOUND_CTRL>(__float_as_int(x))); }
template <int CTRL, bool BOUND_CTRL = false>
__device__ __forceinline__ unsigned long long dpp_mov(unsigned long long x) {
    const unsigned lo = dpp_mov<CTRL, BOUND_CTRL>((unsigned)x), hi = dpp_mov<CTRL, BOUND_CTRL>((unsigned)(x >> 32));
    return ((unsigned long long)hi << 32) | lo;
}
template <int CTRL, bool BOUND_CTRL = false>
__device__ __forceinline__ double dpp_mov(double x) {
    const int lo = dpp_mov<CTRL, BOUND_CTRL>(__double2loint(x)), hi = dpp_mov<CTRL, BOUND_CTRL>(__double2hiint(x));
    return __hiloint2double(hi, lo);
}

// v + (v rotated right by N lanes inside each 16-lane row), N = 8, 4, 2 or 1: one DPP step of a row all-reduce at VALU speed
template <int N>
__device__ __forceinline__ double dpp_ror_add(double v) { return v + dpp_mov<DPP_ROW_ROR + N>(v); }

// value held by lane l (wave-uniform l; a compile-time constant after unrolling): v_readlane, a scalar
__device__ __forceinline__ float lane_get(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }
__device__ __forceinline__ double lane_get(double v, int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}

// ---- the 16 x 16 x 4 MFMA of either precision: accumulator type, the instruction, and where a lane's four accumulator registers sit.
//      Lane `lane` holds index lane & 15 along one dimension of the 16 x 16 tile and, in register r, index
//      drow(lane, r) = CL * (lane >> 4) + CS * r along the other (fp64: (lane >> 4) + 4 r, fp32: 4 (lane >> 4) + r); drow_g is the same for
//      a caller that already holds the lane group g = lane >> 4.
template <typename T> struct Mfma16x4;
template <> struct Mfma16x4<double> {
    typedef double acc_t __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ acc_t mma(double a, double b, acc_t c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
    static constexpr int CS = 4, CL = 1;
    static __device__ __forceinline__ int drow_g(int g, int r) { return CL * g + CS * r; }
    static __device__ __forceinline__ int drow(int lane, int r) { return drow_g(lane >> 4, r); }
};
template <> struct Mfma16x4<float> {
    typedef float acc_t __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ acc_t mma(float a, float b, acc_t c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
    static constexpr int CS = 1, CL = 4;
    static __device__ __forceinline__ int drow_g(int g, int r) { return CL * g + CS * r; }
    static __device__ __forceinline__ int drow(int lane, int r) { return drow_g(lane >> 4, r); }
};

// ---- the Matern 3/2 and 5/2 kernels as a function of the squared distance s (the contract is in include/rlhip.h):
//      (1 + a (1 + a third)) exp(-a), a = c sqrt(s), in Horner form, each step one fused multiply-add.  c = sqrt(3) / l, third = 0 is Matern
//      3/2: fma(a, 0, 1) is exactly 1, so the polynomial is 1 + a rounded once, for every a.  c = sqrt(5) / l, third = 1 / 3 is Matern 5/2.
//      The clamp is a select, not fmax: a NaN s stays NaN.  s == 0 gives exactly 1.
__device__ __forceinline__ double pdk_sqrt(double x) { return sqrt(x); }
__device__ __forceinline__ float pdk_sqrt(float x) { return sqrtf(x); }
__device__ __forceinline__ double pdk_exp(double x) { return exp(x); }
__device__ __forceinline__ float pdk_exp(float x) { return expf(x); }
__device__ __forceinline__ double pdk_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }
__device__ __forceinline__ float pdk_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
template <typename T>
__device__ __forceinline__ T matern_of_s(T s, T c, T third) {
    s = s < T(0) ? T(0) : s;
    const T a = c * pdk_sqrt(s);
    return pdk_fma(a, pdk_fma(a, third, T(1)), T(1)) * pdk_exp(-a);
}
// ---- the gradient weights of the same kernels: grad_z k(z, x) = w(s) (z - x), w(s) = 2 dk/ds = w(0) u(s), and u is what the
//      device kernels evaluate; the caller multiplies by w(0) once, after the sums (PdkFn's weight forms, rlhip_internal.h).
//        squared exponential  w(0) = -1 / l^2        u = exp(scale s): the kernel itself, no function of its own
//        Matern 3/2           w(0) = -3 / l^2        u = exp(-a)              lin = 0: fma(a, 0, 1) is exactly 1
//        Matern 5/2           w(0) = -5 / (3 l^2)    u = (1 + a) exp(-a)      lin = 1: 1 + a rounded once
//      a = c sqrt(s) with matern_of_s's c and its select-clamp; u(0) is exactly 1, and u is smooth in s wherever k is.
template <typename T>
__device__ __forceinline__ T pdk_weight_of_s(T s, T c, T lin) {
    s = s < T(0) ? T(0) : s;
    const T a = c * pdk_sqrt(s);
    return pdk_fma(a, lin, T(1)) * pdk_exp(-a);
}

// ---- the fused two-point-set kernels (rbf.hip rbf_fused_kernel, rbf_var.hip pdk_var_fused_kernel, rbf_grad.hip pdk_grad_fused_kernel):
//      workgroup shape and the layout of the tiles they stage in LDS.  The walk over X itself (the fetch / stash of a tile and the
//      pipelined sub-tile loop; rbf.hip's header has the scheme) stands in each of the three kernels, and a change to it goes into all
//      three: as one inlined function of this header it compiled to other register counts, which crossed occupancy steps and cost the
//      default apply 10 % in fp32 with 64 columns (profiles/rbf_walk_ab.jsonl).
constexpr int RBF_WG = 256;
constexpr int RBF_ZP = 64;                  // points of Z per workgroup
constexpr int RBF_LDS_CAP = 64 * 1024;      // both buffers; no raised dynamic-LDS limit is needed below it

__device__ __forceinline__ double rbf_exp(double x) { return exp(x); }
__device__ __forceinline__ float rbf_exp(float x) { return expf(x); }

// strides of the staged tiles, in elements.  X tile [point][row]: 4 KS + 1 spreads the 16 points x 4 rows of one A-operand read over
// the banks.  B tile [column][point], as B lies in memory: the staging stores are consecutive, and the four X points drow_g(g, 0..3)
// that a lane needs of one column are one 16-byte read in fp32 (4 g + r) and four reads 4 apart in fp64 (g + 4 r); TP + 4 keeps the 16
// columns of one read off each other's banks.
template <typename T, int KS> constexpr int rbf_xs() { return 4 * KS + 1; }
constexpr int rbf_bsp(int tp) { return tp + 4; }
template <typename T, int KS, int NT> constexpr int rbf_tile_elems(int tp) { return tp * rbf_xs<T, KS>() + 16 * NT * rbf_bsp(tp) + tp; }
// points of X per staged tile: the largest of 64, 32, 16 whose two buffers fit RBF_LDS_CAP
template <typename T, int KS, int NT> constexpr int rbf_tp() {
    return 2 * rbf_tile_elems<T, KS, NT>(64) * (int)sizeof(T) <= RBF_LDS_CAP ? 64 : (2 * rbf_tile_elems<T, KS, NT>(32) * (int)sizeof(T) <= RBF_LDS_CAP ? 32 : 16);
}

// an integer as a type: the argument of a generic lambda that needs it at compile time
template <int N> struct IntC { static constexpr int value = N; };

// host side: f(IntC<KS>{}) for KS = rows_x / 4 rounded up to a power of two, at most KS_MAX (zero rows add exactly 0)
template <int KS_MAX = 32, typename F>
int rbf_ks_dispatch(int64_t rows_x, F&& f) {
    if (rows_x <= 4) return f(IntC<1>{});
    if (rows_x <= 8) return f(IntC<2>{});
    if (rows_x <= 16) return f(IntC<4>{});
    if (rows_x <= 32) return f(IntC<8>{});
    if constexpr (KS_MAX >= 32) {
        if (rows_x > 64) return f(IntC<32>{});
    }
    return f(IntC<16>{});
}

}  // namespace rlhip_dev
