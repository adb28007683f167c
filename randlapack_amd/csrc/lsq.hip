// The least-squares layer: the matrix-vector and block products of the sketch-and-precondition solver and the vector
// steps of pcg_saddle and pcg_saddle_block (RandLAPACK/comps/rl_determiter.hh:18-134); the loops are include/RandLAPACK_amd/rl_determiter.hh.
//
//   gemv 'N'          y = alpha A x + beta y: a workgroup owns 64 rows, its four waves a quarter of the columns each; the four sums of a row are
//                     added in wave order.
//   gemv 'T'          y = alpha A^T x + beta y: a fixed grid of G workgroups, workgroup s walks the 512-row slabs s, s + G, ...; a wave owns every
//                     fourth column, sums a column of the slab over its lanes (shuffles) and keeps the running sum of the column in LDS.
//   normal matvec     q = A^T (A d) + delta d with A read ONCE: the same static walk over R-row slabs; a slab is staged in LDS while t = A d is
//                     formed for its rows, then the partial q is advanced from the staged copy (a thread owns columns, registers hold its sums).
//   normal matmat     Q (n x s) = A^T (A D) + delta D.  One-pass route: the slab walk of the normal matvec, with the staged slab used for
//                     every column of a chunk: T_slab (R x SC) = S D, then the partial Q (n x SC) += S^T T_slab; A is read from memory once
//                     per chunk of SC columns.  Composed route: T = A D and Q = A^T T through the library's GEMM.
//   pcg_saddle steps  the n-length updates of one iteration for s columns kept in lockstep: alpha_j, beta_j, delta1_j and d_j^T q_j stay on
//                     the device, a column whose flag active_j is off is not touched.  pcg_saddle's own steps are these with one column and
//                     no flag.
//
// No kernel here waits for another workgroup and none uses a floating-point atomic: every sum over rows ends in one partial per workgroup
// and column in the scratch arena (G x n values per column) and ONE final pass that adds the partials in a fixed order.  The assignment of
// slabs to workgroups is static, so results are bitwise reproducible.  Sums are taken in the precision of the data.  Column j of every
// block output is a function of A, delta and column j of the inputs alone -- no sum ever mixes two columns.
#include "rlhip_internal.h"
#include "rlhip_device.h"

namespace {

using namespace rlhip_dev;

constexpr int GEMV_T_ROWS = 512;                  // rows of a slab of the 'T' kernel: 8 per lane
constexpr int GEMV_T_COLS = 4096;                 // columns a workgroup of the 'T' kernel keeps running sums for (32 KiB of LDS in fp64)
// the slab walk of the two normal-product kernels
constexpr int WALK_MIN_ROWS = 16;                 // shortest slab: a 128-B column segment in fp64
constexpr int WALK_MAX_ROWS = 256;
constexpr int WALK_THREADS = 1024;
constexpr size_t WALK_LDS_BYTES = 160 << 10;
constexpr int FUSED_STAGED = 16;                  // values of a slab a thread of the matvec kernel holds in registers: R n <= FUSED_STAGED *
                                                  // WALK_THREADS (128 KiB in fp64, 64 KiB in fp32); an fp32 slab of 16 rows may take twice that
                                                  // (n up to 2048)
// widest n of the fused kernel; emax = staged values a thread holds in registers (n / NG at R = 16), kmax = columns of the partial q a thread owns
template <typename T> struct FusedLimit;
template <> struct FusedLimit<double> {
    static constexpr int max_n = RLHIP_NORMAL_FUSED_MAX_N_F64, emax = max_n * WALK_MIN_ROWS / WALK_THREADS, kmax = max_n / WALK_THREADS;
    static constexpr int default_max_n = RLHIP_NORMAL_FUSED_DEFAULT_MAX_N_F64;
};
template <> struct FusedLimit<float> {
    static constexpr int max_n = RLHIP_NORMAL_FUSED_MAX_N_F32, emax = max_n * WALK_MIN_ROWS / WALK_THREADS, kmax = max_n / WALK_THREADS;
    static constexpr int default_max_n = RLHIP_NORMAL_FUSED_DEFAULT_MAX_N_F32;
};
static_assert((size_t)RLHIP_NORMAL_FUSED_MAX_N_F64 * WALK_MIN_ROWS * sizeof(double) == (128 << 10) &&
              (size_t)RLHIP_NORMAL_FUSED_MAX_N_F32 * WALK_MIN_ROWS * sizeof(float) == (128 << 10), "the limits in rlhip.h are 16-row slabs of 128 KiB");
static_assert(FusedLimit<double>::emax == FUSED_STAGED && FusedLimit<float>::emax == 2 * FUSED_STAGED, "");
// a slab of the block kernel is half of the matvec kernel's (64 KiB): the other half of the LDS holds D, the shares of T_slab and T_slab
// itself for a chunk of columns.  staged = values of a slab a thread holds in registers (R n <= staged * WALK_THREADS), max_sc = the
// widest chunk
template <typename T> struct BlockLimit;
template <> struct BlockLimit<double> { static constexpr int staged = 8, max_sc = RLHIP_NORMAL_MATMAT_FUSED_SC_F64; };
template <> struct BlockLimit<float> { static constexpr int staged = 16, max_sc = RLHIP_NORMAL_MATMAT_FUSED_SC_F32; };
static_assert(RLHIP_NORMAL_MATMAT_FUSED_MAX_N * WALK_MIN_ROWS == BlockLimit<double>::staged * WALK_THREADS, "the limit in rlhip.h is a 16-row fp64 slab");
static_assert(RLHIP_NORMAL_MATMAT_FUSED_MAX_N * 2 * WALK_MIN_ROWS == BlockLimit<float>::staged * WALK_THREADS, "and a 32-row fp32 slab");
static_assert(BlockLimit<double>::max_sc == 4 && BlockLimit<float>::max_sc == 4, "the widest instantiation: in fp32 a chunk of 8 spills inside the slab loop");
static_assert(2 * RLHIP_NORMAL_MATMAT_FUSED_MAX_N <= WALK_THREADS, "a thread owns one column of the partial Q and at least two threads share a column");

__host__ __device__ inline int64_t imin(int64_t a, int64_t b) { return a < b ? a : b; }

// chunk width of the one-pass normal matmat for (n, s); 0 outside its limits
inline int block_chunk(int64_t n, int64_t s, int elem_bytes) {
    if (n < 1 || n > RLHIP_NORMAL_MATMAT_FUSED_MAX_N || s < 1) return 0;
    const int cap = elem_bytes == 8 ? RLHIP_NORMAL_MATMAT_FUSED_SC_F64 : (elem_bytes == 4 ? RLHIP_NORMAL_MATMAT_FUSED_SC_F32 : 0);
    return (int)imin(s, cap);
}

// where the one-pass matmat is taken unasked: the (precision, n, s) ranges in which it measured faster than both the composed route and s
// single calls of rlhip_normal_matvec by more than the run-to-run spread: 2 <= s <= 8, and n in the slab configurations (R, CW)
// that were measured or lie between two measured ones: 33 .. 256 in fp64 (n = 64 and 256 measured), 129 .. 256 in fp32 (n = 256 measured)
inline int block_default(int64_t n, int64_t s, int elem_bytes) {
    if (!block_chunk(n, s, elem_bytes) || s < 2 || s > 8 || n > 256) return 0;
    return n >= (elem_bytes == 8 ? 33 : 129) ? 1 : 0;
}

// ---- (a) gemv 'N'
template <typename T>
__global__ __launch_bounds__(256) void gemv_n_kernel(int64_t m, int64_t n, T alpha, const T* __restrict__ A, int64_t lda, const T* __restrict__ x,
                                                     T beta, T* __restrict__ y) {
    __shared__ T wsum[4 * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t i = (int64_t)blockIdx.x * 64 + lane;
    const int64_t cq = (n + 3) / 4, j0 = wave * cq, j1 = imin(n, j0 + cq);
    T acc = T(0);
    if (i < m) {
        const T* a = A + i;
        int64_t j = j0;
        for (; j + 8 <= j1; j += 8) {
            T v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = a[(j + u) * lda];
#pragma unroll
            for (int u = 0; u < 8; ++u) acc += v[u] * x[j + u];
        }
        for (; j < j1; ++j) acc += a[j * lda] * x[j];
    }
    wsum[wave * 64 + lane] = acc;
    __syncthreads();
    if (wave == 0 && i < m) {
        const T s = alpha * (((wsum[lane] + wsum[64 + lane]) + wsum[128 + lane]) + wsum[192 + lane]);
        y[i] = beta == T(0) ? s : s + beta * y[i];
    }
}

// ---- (b) gemv 'T': part[g * n + j] = the sum over workgroup g's slabs of A(:, j)^T x.  Dynamic LDS: min(n - c0, GEMV_T_COLS) running sums.
template <typename T>
__global__ __launch_bounds__(256) void gemv_t_partial_kernel(int64_t m, int64_t n, const T* __restrict__ A, int64_t lda, const T* __restrict__ x,
                                                             T* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) char lsq_smem[];
    T* qacc = (T*)lsq_smem;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t c0 = (int64_t)blockIdx.y * GEMV_T_COLS;
    const int nc = (int)imin(n - c0, GEMV_T_COLS);
    for (int t = tid; t < nc; t += 256) qacc[t] = T(0);
    __syncthreads();
    constexpr int PER = GEMV_T_ROWS / 64;
    const int64_t nslab = (m + GEMV_T_ROWS - 1) / GEMV_T_ROWS;
    for (int64_t s = blockIdx.x; s < nslab; s += gridDim.x) {
        const int64_t r0 = s * GEMV_T_ROWS + lane;
        const bool full = (s + 1) * GEMV_T_ROWS <= m;
        T xr[PER];
#pragma unroll
        for (int k = 0; k < PER; ++k) xr[k] = (r0 + 64 * k < m) ? x[r0 + 64 * k] : T(0);
        for (int jc = wave; jc < nc; jc += 4) {                                   // only this wave ever touches qacc[jc]
            const T* a = A + (c0 + jc) * lda + r0;
            T v[PER];
            if (full) {
#pragma unroll
                for (int k = 0; k < PER; ++k) v[k] = a[64 * k];
            } else {
#pragma unroll
                for (int k = 0; k < PER; ++k) v[k] = (r0 + 64 * k < m) ? a[64 * k] : T(0);
            }
            T acc = T(0);
#pragma unroll
            for (int k = 0; k < PER; ++k) acc += v[k] * xr[k];
            acc = wave_sum(acc);
            if (lane == 0) qacc[jc] += acc;
        }
    }
    __syncthreads();
    for (int t = tid; t < nc; t += 256) part[(int64_t)blockIdx.x * n + c0 + t] = qacc[t];
}

// ---- (c) the final pass of every sum over rows: Out(j, c) = alpha * sum_g part[(c G + g) n + j] + coef * X(j, c); coef == 0 does not read X,
// Out may be X, G == 0 gives coef * X.  blockIdx.y = c; a workgroup owns 64 entries of the column, wave w adds the w-th quarter of the
// partials in order, the four quarters are added in wave order.  The product with alpha is rounded before coef * X is added.
template <typename T>
__global__ __launch_bounds__(256) void reduce_partials_kernel(int64_t G, int64_t n, const T* __restrict__ part, T alpha, T coef, const T* X, int64_t ldx,
                                                              T* Out, int64_t ldo) {
    __shared__ T wsum[4 * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t c = blockIdx.y;
    const int64_t j = (int64_t)blockIdx.x * 64 + lane;
    const int64_t gq = (G + 3) / 4, g0 = wave * gq, g1 = imin(G, g0 + gq);
    T acc = T(0);
    if (j < n) {
        const T* p = part + c * G * n + j;
#pragma unroll 8
        for (int64_t g = g0; g < g1; ++g) acc += p[g * n];
    }
    wsum[wave * 64 + lane] = acc;
    __syncthreads();
    if (wave == 0 && j < n) {
        const T s = alpha * (((wsum[lane] + wsum[64 + lane]) + wsum[128 + lane]) + wsum[192 + lane]);
        Out[j + c * ldo] = coef == T(0) ? s : s + coef * X[j + c * ldx];
    }
}

// x^T y by ONE workgroup of 256 threads, every thread gets it: thread t adds the entries t, t + 256, ... in order, the 64 lanes of a wave are
// added by shuffles, the four waves in order.  ws: 4 values of LDS, free again on return.
template <typename T>
__device__ __forceinline__ T block_dot(int64_t n, const T* __restrict__ x, const T* __restrict__ y, T* ws) {
    T acc = T(0);
    for (int64_t i = threadIdx.x; i < n; i += 256) acc += x[i] * y[i];
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = acc;
    __syncthreads();
    const T s = ((ws[0] + ws[1]) + ws[2]) + ws[3];
    __syncthreads();
    return s;
}

// out[c] = X(:, c)^T Y(:, c), one workgroup per column
template <typename T>
__global__ __launch_bounds__(256) void coldot_kernel(int64_t n, const T* __restrict__ X, int64_t ldx, const T* __restrict__ Y, int64_t ldy, T* __restrict__ out) {
    __shared__ T ws[4];
    const int64_t c = blockIdx.x;
    const T s = block_dot(n, X + c * ldx, Y + c * ldy, ws);
    if (threadIdx.x == 0) out[c] = s;
}

// ---- (d) the fused normal matvec: WALK_THREADS threads, one workgroup per CU.  Dynamic LDS: S (n columns of R + 1), dS (n), tp (one per
// thread), ts (R).
// Staging: thread tid owns row r = tid % R of the slab and the columns g, g + NG, ... (g = tid / R, NG = WALK_THREADS / R; at most EMAX of
// them), so a wave reads 64 / R column segments of R contiguous values.  The values of a slab wait in registers: they are loaded while the
// workgroup still works on the slab before (the loads are issued right after the staged copy of that slab is complete), then go to LDS and
// into the thread's share of t[r].  The NG shares of a row are added in order.
// Partial q: thread tid owns the columns jj, jj + CW, ... (jj = tid % CW) and the rows h, h + RH, ... of the slab (h = tid / CW,
// RH = WALK_THREADS / CW; CW = WALK_THREADS unless n is smaller); its sums stay in registers over all slabs of the workgroup, and the RH
// shares of a column are added in order at the end.
// The staging (cnt, step, fetch) stands in this kernel AND in normal_block_kernel, and a change to it goes into both: as one inlined device
// function every instantiation compiled to another instruction stream, which nobody has measured (the RBF walk of 4.22).
template <typename T, int EMAX, int KMAX>
__global__ __launch_bounds__(WALK_THREADS) void normal_fused_kernel(int64_t m, int n, int R, int CW, const T* __restrict__ A, int64_t lda,
                                                                    const T* __restrict__ d, T* __restrict__ t_out, T* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) char lsq_smem[];
    const int LDR = R + 1;
    T* S = (T*)lsq_smem;
    T* dS = S + (size_t)n * LDR;
    T* tp = dS + n;
    T* ts = tp + WALK_THREADS;
    const int tid = threadIdx.x;
    const int r = tid & (R - 1), g = tid / R, NG = WALK_THREADS / R;
    const int jj = tid & (CW - 1), h = tid / CW, RH = WALK_THREADS / CW;
    for (int j = tid; j < n; j += WALK_THREADS) dS[j] = d[j];
    T acc[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) acc[k] = T(0);
    T v[EMAX];
    const int64_t nslab = (m + R - 1) / R;
    // every load is in bounds and unconditional: a row beyond m reads row m - 1, a column beyond n the thread's last column (or column
    // n - 1 when it owns none); neither value is used.  The address walks from column to column, so that no address outlives its load.
    const int cnt = g < n ? (n - g + NG - 1) / NG : 0;                            // columns this thread stages
    const int64_t step = (int64_t)NG * lda;
    auto fetch = [&](int64_t s) {
        const int64_t row = s * R + r;
        const T* p = A + (row < m ? row : m - 1) + (int64_t)(g < n ? g : n - 1) * lda;
#pragma unroll
        for (int u = 0; u < EMAX; ++u) {
            v[u] = *p;
            if (u + 1 < cnt) p += step;
        }
    };
    int64_t s = blockIdx.x;
    if (s < nslab) fetch(s);
    __syncthreads();
    for (; s < nslab; s += gridDim.x) {
        T tacc = T(0);
        const bool live = s * R + r < m;
#pragma unroll
        for (int u = 0; u < EMAX; ++u) {
            const int j = g + u * NG;
            if (j < n) {
                const T w = live ? v[u] : T(0);
                S[j * LDR + r] = w;
                tacc += w * dS[j];
            }
        }
        tp[tid] = tacc;                                                           // = tp[g * R + r]
        __syncthreads();
        if (s + gridDim.x < nslab) fetch(s + gridDim.x);                          // in flight while this slab is worked on
        if (tid < R) {
            T sum = T(0);
#pragma unroll 16
            for (int gg = 0; gg < NG; ++gg) sum += tp[gg * R + tid];
            ts[tid] = sum;
            if (t_out && s * R + tid < m) t_out[s * R + tid] = sum;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            const int jc = jj + k * CW;
            if (jc < n) {
                const T* col = S + jc * LDR;
                T a2 = acc[k];
#pragma unroll 8
                for (int i = h; i < R; i += RH) a2 += col[i] * ts[i];
                acc[k] = a2;
            }
        }
        __syncthreads();
    }
    T* mine = part + (int64_t)blockIdx.x * n;
    if (RH == 1) {
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
            if (jj + k * CW < n) mine[jj + k * CW] = acc[k];
    } else {                                                                      // CW >= n: one column per thread, RH * n <= WALK_THREADS shares
        if (jj < n) tp[h * n + jj] = acc[0];
        __syncthreads();
        if (tid < n) {
            T sum = T(0);
            for (int hh = 0; hh < RH; ++hh) sum += tp[hh * n + tid];
            mine[tid] = sum;
        }
    }
}

// ---- (e) the one-pass normal matmat for w <= SC columns of D.  WALK_THREADS threads, one workgroup per CU.  Dynamic LDS: S (n columns of
// R + 1), dS (n x SC, column index fastest; columns w .. SC - 1 are zero), tp (SC x WALK_THREADS shares), ts (R x SC, column index fastest).
// The staging is written out here as in normal_fused_kernel, and a change to it goes into both kernels (the note there):
// thread tid owns row r = tid % R of the slab and the columns g, g + NG, ... (at most EMAX of them); the values of the next slab wait in
// registers while this one is worked on.  A thread adds its share of T_slab(r, c) for every c; the NG shares are added in order of g.
// Partial Q: thread tid owns column jj = tid % CW and the rows h, h + RH, ... of the slab (h = tid / CW, RH = WALK_THREADS / CW >= 2, CW the
// least power of two >= n); its SC sums stay in registers over all slabs of the workgroup, and the RH shares of a column are added in order
// at the end.
// part: w blocks of gridDim.x x n values, block c = column c.
template <typename T, int EMAX, int SC>
__global__ __launch_bounds__(WALK_THREADS) void normal_block_kernel(int64_t m, int n, int w, int R, int CW, const T* __restrict__ A, int64_t lda,
                                                                    const T* __restrict__ D, int64_t ldd, T* __restrict__ t_out, int64_t ldt,
                                                                    T* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) char lsq_smem[];
    const int LDR = R + 1;
    T* S = (T*)lsq_smem;
    T* dS = S + (((size_t)n * LDR + 3) & ~(size_t)3);
    T* tp = dS + (size_t)n * SC;
    T* ts = tp + (size_t)WALK_THREADS * SC;
    const int tid = threadIdx.x;
    const int r = tid & (R - 1), g = tid / R, NG = WALK_THREADS / R;
    const int jj = tid & (CW - 1), h = tid / CW, RH = WALK_THREADS / CW;
    for (int o = tid; o < n * SC; o += WALK_THREADS) {
        const int j = o / SC, c = o - j * SC;
        dS[o] = c < w ? D[j + (int64_t)c * ldd] : T(0);
    }
    T acc[SC];
#pragma unroll
    for (int c = 0; c < SC; ++c) acc[c] = T(0);
    T v[EMAX];
    const int64_t nslab = (m + R - 1) / R;
    // every load is in bounds and unconditional: a row beyond m reads row m - 1, a column beyond n the thread's last column (or column
    // n - 1 when it owns none); neither value is used
    const int cnt = g < n ? (n - g + NG - 1) / NG : 0;                            // columns this thread stages
    const int64_t step = (int64_t)NG * lda;
    auto fetch = [&](int64_t s) {
        const int64_t row = s * R + r;
        const T* p = A + (row < m ? row : m - 1) + (int64_t)(g < n ? g : n - 1) * lda;
#pragma unroll
        for (int u = 0; u < EMAX; ++u) {
            v[u] = *p;
            if (u + 1 < cnt) p += step;
        }
    };
    int64_t s = blockIdx.x;
    if (s < nslab) fetch(s);
    __syncthreads();
    for (; s < nslab; s += gridDim.x) {
        T tacc[SC];
#pragma unroll
        for (int c = 0; c < SC; ++c) tacc[c] = T(0);
        const bool live = s * R + r < m;
#pragma unroll
        for (int u = 0; u < EMAX; ++u) {
            const int j = g + u * NG;
            if (j < n) {
                const T a = live ? v[u] : T(0);
                S[j * LDR + r] = a;
                const T* dj = dS + j * SC;
#pragma unroll
                for (int c = 0; c < SC; ++c) tacc[c] += a * dj[c];
            }
        }
#pragma unroll
        for (int c = 0; c < SC; ++c) tp[c * WALK_THREADS + tid] = tacc[c];        // = tp[(c * NG + g) * R + r]
        __syncthreads();
        if (s + gridDim.x < nslab) fetch(s + gridDim.x);                          // in flight while this slab is worked on
        for (int o = tid; o < R * SC; o += WALK_THREADS) {
            const int c = o / R, row = o - c * R;
            const T* sh = tp + c * WALK_THREADS + row;
            T sum = T(0);
#pragma unroll 16
            for (int gg = 0; gg < NG; ++gg) sum += sh[gg * R];
            const bool in = s * R + row < m;                                      // a row beyond m is zero whatever D holds
            ts[row * SC + c] = in ? sum : T(0);
            if (t_out && in && c < w) t_out[s * R + row + (int64_t)c * ldt] = sum;
        }
        __syncthreads();
        if (jj < n) {
            const T* col = S + jj * LDR;
#pragma unroll 4
            for (int i = h; i < R; i += RH) {
                const T a = col[i];
                const T* ti = ts + i * SC;
#pragma unroll
                for (int c = 0; c < SC; ++c) acc[c] += a * ti[c];
            }
        }
        __syncthreads();
    }
    // RH * n <= WALK_THREADS shares of every column
    if (jj < n) {
#pragma unroll
        for (int c = 0; c < SC; ++c) tp[c * WALK_THREADS + h * n + jj] = acc[c];
    }
    __syncthreads();
    for (int o = tid; o < n * w; o += WALK_THREADS) {
        const int c = o / n, j = o - c * n;
        const T* sh = tp + c * WALK_THREADS + j;
        T sum = T(0);
        for (int hh = 0; hh < RH; ++hh) sum += sh[hh * n];
        part[((int64_t)c * gridDim.x + blockIdx.x) * n + j] = sum;
    }
}

// Q += delta D on an n x s block (the composed matmat's last step)
template <typename T>
__global__ __launch_bounds__(256) void add_delta_kernel(int64_t n, int64_t s, T delta, const T* __restrict__ D, int64_t ldd, T* __restrict__ Q, int64_t ldq) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    for (int64_t c = blockIdx.y; c < s; c += gridDim.y) Q[j + c * ldq] += delta * D[j + c * ldd];
}

// ---- (f) the vector steps of pcg_saddle and pcg_saddle_block; one column per grid row (step_d: per workgroup).  A column whose flag is
// off is left alone; active == nullptr: every column is active.
template <typename T>
__global__ __launch_bounds__(256) void block_step_xr_kernel(int64_t n, const T* __restrict__ D, int64_t ldd, const T* __restrict__ Q, int64_t ldq,
                                                            const T* __restrict__ dq, const T* __restrict__ delta1, int64_t ldh, T* __restrict__ X,
                                                            int64_t ldx, T* __restrict__ Rm, int64_t ldr, const int* __restrict__ active) {
    const int64_t c = blockIdx.y;
    if (active && !active[c]) return;
    const T alpha = delta1[c * ldh] / dq[c];                                                              // rl_determiter.hh:86
    const T* d = D + c * ldd;
    T* x = X + c * ldx;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        x[i] += alpha * d[i];                                                                             // :89
        if (Q) Rm[i + c * ldr] -= alpha * Q[i + c * ldq];                                                 // :106
    }
}

template <typename T>
__global__ __launch_bounds__(256) void block_step_refresh_kernel(int64_t n, const T* __restrict__ B1, int64_t ldb1, const T* __restrict__ QX, int64_t ldqx,
                                                                 T delta, const T* __restrict__ X, int64_t ldx, T* __restrict__ Rm, int64_t ldr,
                                                                 const int* __restrict__ active) {
    const int64_t c = blockIdx.y;
    if (active && !active[c]) return;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        T v = B1[i + c * ldb1] - QX[i + c * ldqx];                                                        // :101-102
        if (delta > T(0)) v -= delta * X[i + c * ldx];                                                    // :103
        Rm[i + c * ldr] = v;
    }
}

// delta1_old == nullptr: the first call; it forms rel_sq_tol and sets the flag whatever it held.  rel_sq_tol == nullptr (pcg_saddle, whose
// host loop tests delta1 itself): no tolerance is formed and no flag written.
template <typename T>
__global__ __launch_bounds__(256) void block_step_d_kernel(int64_t n, const T* __restrict__ Rm, int64_t ldr, const T* __restrict__ Sm, int64_t lds,
                                                           const T* delta1_old, T* delta1_new, int64_t ldh, T* __restrict__ D, int64_t ldd, T tol,
                                                           T* __restrict__ rel_sq_tol, int* __restrict__ active) {
    __shared__ T ws[4];
    const int64_t c = blockIdx.x;
    if (delta1_old && active && !active[c]) return;                               // uniform over the workgroup
    const T* s = Sm + c * lds;
    const T dnew = block_dot(n, Rm + c * ldr, s, ws);                                                     // :118 (:69)
    if (delta1_old) {
        const T beta = dnew / delta1_old[c * ldh];                                                        // :119
        T* d = D + c * ldd;
        for (int64_t i = threadIdx.x; i < n; i += 256) d[i] = beta * d[i] + s[i];                         // :120-122
    }
    if (threadIdx.x == 0) {
        delta1_new[c * ldh] = dnew;
        if (rel_sq_tol) {
            T lim;
            if (delta1_old) lim = rel_sq_tol[c];
            else rel_sq_tol[c] = lim = (dnew * tol) * tol;                                                // :71
            active[c] = dnew > lim ? 1 : 0;                                       // false for a NaN: the column stops (:76)
        }
    }
}

inline unsigned stream_grid(rlhip_ctx* c, int64_t n) {
    const int64_t want = (n + 255) / 256, cap = c->num_cu;
    return (unsigned)(want < 1 ? 1 : (want < cap ? want : cap));
}
constexpr int64_t GRID_Y_MAX = 65535;

// The slab rule of both normal-product kernels: R rows per slab, the largest power of two in [WALK_MIN_ROWS, WALK_MAX_ROWS] with
// R n <= staged * WALK_THREADS (at WALK_MIN_ROWS the caller's own limit on n decides) and no taller than m needs; CW = the least power of two
// >= n, at most cw_max; one workgroup per CU (or max_wg) and never more than there are slabs.
struct SlabPlan {
    int R, CW;
    int64_t G;
};
inline SlabPlan slab_plan(int64_t m, int64_t n, int staged, int cw_max, int64_t max_wg, int num_cu) {
    SlabPlan p{WALK_MAX_ROWS, cw_max, 0};
    while (p.R > WALK_MIN_ROWS && (int64_t)p.R * n > (int64_t)staged * WALK_THREADS) p.R >>= 1;
    while (p.R > WALK_MIN_ROWS && p.R / 2 >= m) p.R >>= 1;
    while (p.CW / 2 >= n) p.CW >>= 1;
    p.G = imin((m + p.R - 1) / p.R, max_wg > 0 ? max_wg : (int64_t)num_cu);
    return p;
}

template <typename T, int EMAX, int KMAX>
int launch_fused(rlhip_ctx* c, int64_t G, size_t lds, int64_t m, int n, int R, int CW, const T* A, int64_t lda, const T* d, T* t, T* part) {
    RLHIP_FUNC_LDS(c, (normal_fused_kernel<T, EMAX, KMAX>), WALK_LDS_BYTES);
    hipLaunchKernelGGL((normal_fused_kernel<T, EMAX, KMAX>), dim3((unsigned)G), dim3(WALK_THREADS), lds, c->stream, m, n, R, CW, A, lda, d, t, part);
    return 0;
}

template <typename T, int SC>
int launch_block(rlhip_ctx* c, int64_t G, size_t lds, int64_t m, int n, int w, int R, int CW, const T* A, int64_t lda, const T* D, int64_t ldd, T* t,
                 int64_t ldt, T* part) {
    constexpr int EMAX = BlockLimit<T>::staged;
    RLHIP_FUNC_LDS(c, (normal_block_kernel<T, EMAX, SC>), WALK_LDS_BYTES);
    hipLaunchKernelGGL((normal_block_kernel<T, EMAX, SC>), dim3((unsigned)G), dim3(WALK_THREADS), lds, c->stream, m, n, w, R, CW, A, lda, D, ldd, t, ldt,
                       part);
    return 0;
}

// Out (n x w) = alpha * (the sum of the G partials of every column) + coef X; not followed by a launch check
template <typename T>
void launch_reduce(rlhip_ctx* c, int64_t G, int64_t n, int64_t w, const T* part, T alpha, T coef, const T* X, int64_t ldx, T* Out, int64_t ldo) {
    hipLaunchKernelGGL(reduce_partials_kernel<T>, dim3((unsigned)((n + 63) / 64), (unsigned)w), dim3(256), 0, c->stream, G, n, part, alpha, coef, X, ldx, Out,
                       ldo);
}

// out = alpha A^T x + coef xvec (m >= 0, n > 0)
template <typename T>
int gemv_t(rlhip_ctx* c, int64_t m, int64_t n, const T* A, int64_t lda, const T* x, T alpha, T coef, const T* xvec, T* out) {
    const int64_t nslab = (m + GEMV_T_ROWS - 1) / GEMV_T_ROWS;
    const int64_t G = alpha == T(0) ? 0 : imin(nslab, (int64_t)c->num_cu * 4);
    ws_scope ws(c);
    T* part = nullptr;
    if (G > 0) {
        part = ws.alloc<T>((size_t)(G * n));
        if (!part) return RLHIP_ERR_HIP(hipErrorOutOfMemory);
        const dim3 grid((unsigned)G, (unsigned)((n + GEMV_T_COLS - 1) / GEMV_T_COLS));
        hipLaunchKernelGGL(gemv_t_partial_kernel<T>, grid, dim3(256), (size_t)imin(n, GEMV_T_COLS) * sizeof(T), c->stream, m, n, A, lda, x, part);
    }
    launch_reduce<T>(c, G, n, 1, part, alpha, coef, xvec, n, out, n);
    RLHIP_LAUNCH_CHECK();
    return 0;
}

template <typename T>
int normal_matvec(rlhip_ctx* c, int64_t m, int64_t n, const T* A, int64_t lda, const T* d, T delta, T* q, T* t, T* dq_dev, int64_t max_wg) {
    if (m < 0) return -2;
    if (n < 0) return -3;
    if (m > 0 && n > 0 && !A) return -4;
    if (lda < (m > 1 ? m : 1)) return -5;
    if (n > 0 && !d) return -6;
    if (n > 0 && !q) return -8;
    if (n == 0) return 0;
    const int64_t route = c->opt[RLHIP_OPT_LSQ_NORMAL_FUSED];
    const bool fused = n <= FusedLimit<T>::max_n && route != 0 && (route > 0 || n <= FusedLimit<T>::default_max_n);
    if (fused) {
        c->lsq_path_count[0]++;
        const SlabPlan p = slab_plan(m, n, FUSED_STAGED, WALK_THREADS, max_wg, c->num_cu);
        // S, dS, tp, ts: at most 17/16 of the slab budget + (max_n + WALK_THREADS + WALK_MAX_ROWS) values
        const size_t lds = ((size_t)n * (p.R + 1) + n + WALK_THREADS + p.R) * sizeof(T);
        if (lds > WALK_LDS_BYTES) return RLHIP_ERR_HIP(hipErrorInvalidValue);
        ws_scope ws(c);
        T* part = nullptr;
        if (p.G > 0) {
            part = ws.alloc<T>((size_t)(p.G * n));
            if (!part) return RLHIP_ERR_HIP(hipErrorOutOfMemory);
            int rc;
            if ((int64_t)p.R * n > (int64_t)FUSED_STAGED * WALK_THREADS)          // fp32, n > 1024: 32 staged values and two columns of q per thread
                rc = launch_fused<T, FusedLimit<T>::emax, FusedLimit<T>::kmax>(c, p.G, lds, m, (int)n, p.R, p.CW, A, lda, d, t, part);
            else
                rc = launch_fused<T, FUSED_STAGED, 1>(c, p.G, lds, m, (int)n, p.R, p.CW, A, lda, d, t, part);
            if (rc) return rc;
        }
        launch_reduce<T>(c, p.G, n, 1, part, T(1), delta, d, n, q, n);
    } else {
        c->lsq_path_count[1]++;
        ws_scope ws(c);
        T* tt = t;
        if (!tt && m > 0) {
            tt = ws.alloc<T>((size_t)m);
            if (!tt) return RLHIP_ERR_HIP(hipErrorOutOfMemory);
        }
        int rc = m > 0 ? rlhip::gemv<T>(c, rlhip::NoTrans, m, n, T(1), A, lda, d, T(0), tt) : 0;
        if (rc) return rc;
        if (m > 0) c->lsq_path_count[3]++;
        rc = gemv_t<T>(c, m, n, A, lda, tt, T(1), delta, d, q);
        if (rc) return rc;
    }
    if (dq_dev) hipLaunchKernelGGL(coldot_kernel<T>, dim3(1), dim3(256), 0, c->stream, n, d, n, q, n, dq_dev);
    RLHIP_LAUNCH_CHECK();
    return 0;
}

// the one-pass matmat for w <= max_sc columns (m, n > 0)
template <typename T>
int block_chunk_pass(rlhip_ctx* c, int64_t m, int n, int w, const T* A, int64_t lda, const T* D, int64_t ldd, T delta, T* Q, int64_t ldq, T* t, int64_t ldt,
                     int64_t max_wg) {
    const int SC = w <= 1 ? 1 : (w <= 2 ? 2 : 4);
    const SlabPlan p = slab_plan(m, n, BlockLimit<T>::staged, WALK_THREADS / 2, max_wg, c->num_cu);
    const size_t lds = ((((size_t)n * (p.R + 1) + 3) & ~(size_t)3) + (size_t)n * SC + (size_t)WALK_THREADS * SC + (size_t)p.R * SC) * sizeof(T);
    if ((int64_t)p.R * n > (int64_t)BlockLimit<T>::staged * WALK_THREADS || lds > WALK_LDS_BYTES || w > BlockLimit<T>::max_sc)
        return RLHIP_ERR_HIP(hipErrorInvalidValue);
    ws_scope ws(c);
    T* part = ws.alloc<T>((size_t)(p.G * n * w));
    if (!part) return RLHIP_ERR_HIP(hipErrorOutOfMemory);
    int rc;
    if (SC == 1) rc = launch_block<T, 1>(c, p.G, lds, m, n, w, p.R, p.CW, A, lda, D, ldd, t, ldt, part);
    else if (SC == 2) rc = launch_block<T, 2>(c, p.G, lds, m, n, w, p.R, p.CW, A, lda, D, ldd, t, ldt, part);
    else rc = launch_block<T, 4>(c, p.G, lds, m, n, w, p.R, p.CW, A, lda, D, ldd, t, ldt, part);
    if (rc) return rc;
    launch_reduce<T>(c, p.G, n, w, part, T(1), delta, D, ldd, Q, ldq);
    RLHIP_LAUNCH_CHECK();
    return 0;
}

template <typename T>
int normal_matmat(rlhip_ctx* c, int64_t m, int64_t n, int64_t s, const T* A, int64_t lda, const T* D, int64_t ldd, T delta, T* Q, int64_t ldq, T* t,
                  int64_t ldt, T* dq_dev, int64_t max_wg) {
    if (!c) return -1;
    if (m < 0) return -2;
    if (n < 0) return -3;
    if (s < 0) return -4;
    const bool work = n > 0 && s > 0;
    if (m > 0 && work && !A) return -5;
    if (lda < (m > 1 ? m : 1)) return -6;
    if (work && !D) return -7;
    if (ldd < (n > 1 ? n : 1)) return -8;
    if (work && !Q) return -10;
    if (ldq < (n > 1 ? n : 1)) return -11;
    if (t && ldt < (m > 1 ? m : 1)) return -13;
    if (!work) return 0;
    if (m == 0) {                                                                 // Q = delta D
        for (int64_t c0 = 0; c0 < s; c0 += GRID_Y_MAX)
            launch_reduce<T>(c, 0, n, imin(s - c0, GRID_Y_MAX), nullptr, T(1), delta, D + c0 * ldd, ldd, Q + c0 * ldq, ldq);
    } else {
        const int sc = c->matmat_route == 0 ? 0 : block_chunk(n, s, (int)sizeof(T));
        if (sc > 0 && (c->matmat_route > 0 || block_default(n, s, (int)sizeof(T)))) {
            c->lsq_block_path_count[0]++;
            for (int64_t c0 = 0; c0 < s; c0 += sc) {
                const int rc = block_chunk_pass<T>(c, m, (int)n, (int)imin(s - c0, sc), A, lda, D + c0 * ldd, ldd, delta, Q + c0 * ldq, ldq,
                                                   t ? t + c0 * ldt : nullptr, ldt, max_wg);
                if (rc) return rc;
            }
        } else {
            c->lsq_block_path_count[1]++;
            ws_scope ws(c);
            T* tt = t;
            int64_t ldtt = ldt;
            if (!tt) {
                tt = ws.alloc<T>((size_t)(m * s));
                ldtt = m;
                if (!tt) return RLHIP_ERR_HIP(hipErrorOutOfMemory);
            }
            int rc = rlhip::gemm<T>(c, rlhip::NoTrans, rlhip::NoTrans, m, s, n, T(1), A, lda, D, ldd, T(0), tt, ldtt);
            if (rc) return rc;
            rc = rlhip::gemm<T>(c, rlhip::Trans, rlhip::NoTrans, n, s, m, T(1), A, lda, tt, ldtt, T(0), Q, ldq);
            if (rc) return rc;
            if (delta != T(0))
                hipLaunchKernelGGL(add_delta_kernel<T>, dim3((unsigned)((n + 255) / 256), (unsigned)imin(s, GRID_Y_MAX)), dim3(256), 0, c->stream, n, s, delta, D,
                                   ldd, Q, ldq);
        }
    }
    if (dq_dev) hipLaunchKernelGGL(coldot_kernel<T>, dim3((unsigned)s), dim3(256), 0, c->stream, n, D, ldd, Q, ldq, dq_dev);
    RLHIP_LAUNCH_CHECK();
    return 0;
}

// pcg_saddle's steps: one column, leading dimensions n, scalars one apart, no flag and no tolerance
template <typename T>
int step_xr(rlhip_ctx* c, int64_t n, const T* d, const T* q, const T* dq_dev, const T* delta1_dev, T* x, T* r) {
    if (n < 0) return -2;
    if (n > 0 && !d) return -3;
    if (!dq_dev) return -5;
    if (!delta1_dev) return -6;
    if (n > 0 && !x) return -7;
    if (n > 0 && q && !r) return -8;
    if (n == 0) return 0;
    hipLaunchKernelGGL(block_step_xr_kernel<T>, dim3(stream_grid(c, n), 1), dim3(256), 0, c->stream, n, d, n, q, n, dq_dev, delta1_dev, (int64_t)1, x, n, r, n,
                       (const int*)nullptr);
    RLHIP_LAUNCH_CHECK();
    return 0;
}

template <typename T>
int step_refresh(rlhip_ctx* c, int64_t n, const T* b1, const T* qx, T delta, const T* x, T* r) {
    if (n < 0) return -2;
    if (n > 0 && !b1) return -3;
    if (n > 0 && !qx) return -4;
    if (n > 0 && !x) return -6;
    if (n > 0 && !r) return -7;
    if (n == 0) return 0;
    hipLaunchKernelGGL(block_step_refresh_kernel<T>, dim3(stream_grid(c, n), 1), dim3(256), 0, c->stream, n, b1, n, qx, n, delta, x, n, r, n,
                       (const int*)nullptr);
    RLHIP_LAUNCH_CHECK();
    return 0;
}

template <typename T>
int step_d(rlhip_ctx* c, int64_t n, const T* r, const T* s, const T* delta1_old_dev, T* delta1_new_dev, T* d) {
    if (n < 0) return -2;
    if (n > 0 && !r) return -3;
    if (n > 0 && !s) return -4;
    if (!delta1_new_dev) return -6;
    if (n > 0 && delta1_old_dev && !d) return -7;
    if (n == 0) return 0;
    hipLaunchKernelGGL(block_step_d_kernel<T>, dim3(1), dim3(256), 0, c->stream, n, r, n, s, n, delta1_old_dev, delta1_new_dev, (int64_t)1, d, n, T(0),
                       (T*)nullptr, (int*)nullptr);
    RLHIP_LAUNCH_CHECK();
    return 0;
}

template <typename T>
int block_step_xr(rlhip_ctx* c, int64_t n, int64_t s, const T* D, int64_t ldd, const T* Q, int64_t ldq, const T* dq_dev, const T* delta1_dev, int64_t ldh,
                  T* X, int64_t ldx, T* R, int64_t ldr, const int* active_dev) {
    if (!c) return -1;
    if (n < 0) return -2;
    if (s < 0 || s > GRID_Y_MAX) return -3;
    const bool work = n > 0 && s > 0;
    const int64_t nn = n > 1 ? n : 1;
    if (work && !D) return -4;
    if (ldd < nn) return -5;
    if (Q && ldq < nn) return -7;
    if (work && !dq_dev) return -8;
    if (work && !delta1_dev) return -9;
    if (ldh < 1) return -10;
    if (work && !X) return -11;
    if (ldx < nn) return -12;
    if (work && Q && !R) return -13;
    if (Q && ldr < nn) return -14;
    if (work && !active_dev) return -15;
    if (!work) return 0;
    hipLaunchKernelGGL(block_step_xr_kernel<T>, dim3(stream_grid(c, n), (unsigned)s), dim3(256), 0, c->stream, n, D, ldd, Q, ldq, dq_dev, delta1_dev, ldh, X,
                       ldx, R, ldr, active_dev);
    RLHIP_LAUNCH_CHECK();
    return 0;
}

template <typename T>
int block_step_refresh(rlhip_ctx* c, int64_t n, int64_t s, const T* B1, int64_t ldb1, const T* QX, int64_t ldqx, T delta, const T* X, int64_t ldx, T* R,
                       int64_t ldr, const int* active_dev) {
    if (!c) return -1;
    if (n < 0) return -2;
    if (s < 0 || s > GRID_Y_MAX) return -3;
    const bool work = n > 0 && s > 0;
    const int64_t nn = n > 1 ? n : 1;
    if (work && !B1) return -4;
    if (ldb1 < nn) return -5;
    if (work && !QX) return -6;
    if (ldqx < nn) return -7;
    if (work && !X) return -9;
    if (ldx < nn) return -10;
    if (work && !R) return -11;
    if (ldr < nn) return -12;
    if (work && !active_dev) return -13;
    if (!work) return 0;
    hipLaunchKernelGGL(block_step_refresh_kernel<T>, dim3(stream_grid(c, n), (unsigned)s), dim3(256), 0, c->stream, n, B1, ldb1, QX, ldqx, delta, X, ldx, R, ldr,
                       active_dev);
    RLHIP_LAUNCH_CHECK();
    return 0;
}

template <typename T>
int block_step_d(rlhip_ctx* c, int64_t n, int64_t s, const T* R, int64_t ldr, const T* S, int64_t lds, const T* delta1_old_dev, T* delta1_new_dev,
                 int64_t ldh, T* D, int64_t ldd, T tol, T* rel_sq_tol_dev, int* active_dev) {
    if (!c) return -1;
    if (n < 0) return -2;
    if (s < 0) return -3;
    const bool work = n > 0 && s > 0;
    const int64_t nn = n > 1 ? n : 1;
    if (work && !R) return -4;
    if (ldr < nn) return -5;
    if (work && !S) return -6;
    if (lds < nn) return -7;
    if (work && !delta1_new_dev) return -9;
    if (ldh < 1) return -10;
    if (work && delta1_old_dev && !D) return -11;
    if (delta1_old_dev && ldd < nn) return -12;
    if (work && !rel_sq_tol_dev) return -14;
    if (work && !active_dev) return -15;
    if (!work) return 0;
    if (delta1_old_dev) c->lsq_block_path_count[2]++;                             // one such call per iteration of pcg_saddle_block
    hipLaunchKernelGGL(block_step_d_kernel<T>, dim3((unsigned)s), dim3(256), 0, c->stream, n, R, ldr, S, lds, delta1_old_dev, delta1_new_dev, ldh, D, ldd, tol,
                       rel_sq_tol_dev, active_dev);
    RLHIP_LAUNCH_CHECK();
    return 0;
}

inline int trans_of(char t) { return (t == 'N' || t == 'n') ? rlhip::NoTrans : ((t == 'T' || t == 't') ? rlhip::Trans : -1); }

}  // namespace

namespace rlhip {

template <typename T>
int gemv(rlhip_ctx* c, int trans, int64_t m, int64_t n, T alpha, const T* A, int64_t lda, const T* x, T beta, T* y) {
    if (trans != NoTrans && trans != Trans) return -2;
    if (m < 0) return -3;
    if (n < 0) return -4;
    const bool work = m > 0 && n > 0;
    if (work && !A) return -6;
    if (lda < (m > 1 ? m : 1)) return -7;
    if (work && !x) return -8;
    if (work && !y) return -10;
    if (!work || (alpha == T(0) && beta == T(1))) return 0;                       // BLAS's quick return
    if (trans == Trans) {
        c->lsq_path_count[3]++;
        return gemv_t<T>(c, m, n, A, lda, x, alpha, beta, y, y);
    }
    c->lsq_path_count[2]++;
    if (alpha == T(0))
        launch_reduce<T>(c, 0, m, 1, nullptr, T(0), beta, y, m, y, m);
    else
        hipLaunchKernelGGL(gemv_n_kernel<T>, dim3((unsigned)((m + 63) / 64)), dim3(256), 0, c->stream, m, n, alpha, A, lda, x, beta, y);
    RLHIP_LAUNCH_CHECK();
    return 0;
}
template int gemv<double>(rlhip_ctx*, int, int64_t, int64_t, double, const double*, int64_t, const double*, double, double*);
template int gemv<float>(rlhip_ctx*, int, int64_t, int64_t, float, const float*, int64_t, const float*, float, float*);

template <typename T>
int dot_dev(rlhip_ctx* c, int64_t n, const T* x, const T* y, T* out_dev) {
    hipLaunchKernelGGL(coldot_kernel<T>, dim3(1), dim3(256), 0, c->stream, n, x, n, y, n, out_dev);
    RLHIP_LAUNCH_CHECK();
    return 0;
}
template int dot_dev<double>(rlhip_ctx*, int64_t, const double*, const double*, double*);
template int dot_dev<float>(rlhip_ctx*, int64_t, const float*, const float*, float*);

}  // namespace rlhip

extern "C" {

int64_t rlhip_lsq_path_count(rlhip_ctx* c, int which) { return (c && which >= 46 && which <= 49) ? c->lsq_path_count[which - 46] : -1; }

int64_t rlhip_lsq_block_path_count(rlhip_ctx* c, int which) { return (c && which >= 76 && which <= 78) ? c->lsq_block_path_count[which - 76] : -1; }

int rlhip_normal_matmat_fused(int64_t n, int64_t s, int elem_bytes) { return block_chunk(n, s, elem_bytes); }

int rlhip_normal_matmat_default(int64_t n, int64_t s, int elem_bytes) { return block_default(n, s, elem_bytes); }

int rlhip_normal_matmat_set_route(rlhip_ctx* c, int route) {
    if (!c) return -1;
    const int was = c->matmat_route;
    c->matmat_route = route < 0 ? -1 : (route > 0 ? 1 : 0);
    return was;
}

#define RLHIP_DEFINE_LSQ(SUF, T)                                                                                                                       \
    int rlhip_gemv_##SUF(rlhip_ctx* c, char trans, int64_t m, int64_t n, T alpha, const T* A, int64_t lda, const T* x, T beta, T* y) {                 \
        return rlhip::gemv<T>(c, trans_of(trans), m, n, alpha, A, lda, x, beta, y);                                                                    \
    }                                                                                                                                                  \
    int rlhip_normal_matvec_##SUF(rlhip_ctx* c, int64_t m, int64_t n, const T* A, int64_t lda, const T* d, T delta, T* q, T* t, T* dq_dev,             \
                                  int64_t max_wg) {                                                                                                    \
        return normal_matvec<T>(c, m, n, A, lda, d, delta, q, t, dq_dev, max_wg);                                                                      \
    }                                                                                                                                                  \
    int rlhip_pcg_saddle_step_xr_##SUF(rlhip_ctx* c, int64_t n, const T* d, const T* q, const T* dq_dev, const T* delta1_dev, T* x, T* r) {            \
        return step_xr<T>(c, n, d, q, dq_dev, delta1_dev, x, r);                                                                                       \
    }                                                                                                                                                  \
    int rlhip_pcg_saddle_step_refresh_##SUF(rlhip_ctx* c, int64_t n, const T* b1, const T* qx, T delta, const T* x, T* r) {                            \
        return step_refresh<T>(c, n, b1, qx, delta, x, r);                                                                                             \
    }                                                                                                                                                  \
    int rlhip_pcg_saddle_step_d_##SUF(rlhip_ctx* c, int64_t n, const T* r, const T* s, const T* delta1_old_dev, T* delta1_new_dev, T* d) {             \
        return step_d<T>(c, n, r, s, delta1_old_dev, delta1_new_dev, d);                                                                               \
    }                                                                                                                                                  \
    int rlhip_normal_matmat_##SUF(rlhip_ctx* c, int64_t m, int64_t n, int64_t s, const T* A, int64_t lda, const T* D, int64_t ldd, T delta, T* Q,      \
                                  int64_t ldq, T* t, int64_t ldt, T* dq_dev, int64_t max_wg) {                                                         \
        return normal_matmat<T>(c, m, n, s, A, lda, D, ldd, delta, Q, ldq, t, ldt, dq_dev, max_wg);                                                    \
    }                                                                                                                                                  \
    int rlhip_pcg_saddle_block_step_xr_##SUF(rlhip_ctx* c, int64_t n, int64_t s, const T* D, int64_t ldd, const T* Q, int64_t ldq, const T* dq_dev,    \
                                             const T* delta1_dev, int64_t ldh, T* X, int64_t ldx, T* R, int64_t ldr, const int* active_dev) {          \
        return block_step_xr<T>(c, n, s, D, ldd, Q, ldq, dq_dev, delta1_dev, ldh, X, ldx, R, ldr, active_dev);                                         \
    }                                                                                                                                                  \
    int rlhip_pcg_saddle_block_step_refresh_##SUF(rlhip_ctx* c, int64_t n, int64_t s, const T* B1, int64_t ldb1, const T* QX, int64_t ldqx, T delta,   \
                                                  const T* X, int64_t ldx, T* R, int64_t ldr, const int* active_dev) {                                 \
        return block_step_refresh<T>(c, n, s, B1, ldb1, QX, ldqx, delta, X, ldx, R, ldr, active_dev);                                                  \
    }                                                                                                                                                  \
    int rlhip_pcg_saddle_block_step_d_##SUF(rlhip_ctx* c, int64_t n, int64_t s, const T* R, int64_t ldr, const T* S, int64_t lds,                      \
                                            const T* delta1_old_dev, T* delta1_new_dev, int64_t ldh, T* D, int64_t ldd, T tol, T* rel_sq_tol_dev,      \
                                            int* active_dev) {                                                                                         \
        return block_step_d<T>(c, n, s, R, ldr, S, lds, delta1_old_dev, delta1_new_dev, ldh, D, ldd, tol, rel_sq_tol_dev, active_dev);                 \
    }
RLHIP_DEFINE_LSQ(f64, double)
RLHIP_DEFINE_LSQ(f32, float)

}  // extern "C"
