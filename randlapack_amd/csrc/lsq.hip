// The matrix-vector layer of the sketch-and-precondition least-squares solver and the vector steps of pcg_saddle
// (RandLAPACK/comps/rl_determiter.hh:18-134); the loop itself is include/RandLAPACK_amd/rl_determiter.hh.
//
//   gemv 'N'          y = alpha A x + beta y: a workgroup owns 64 rows, its four waves a quarter of the columns each; the four sums of a row are
//                     added in wave order.
//   gemv 'T'          y = alpha A^T x + beta y: a fixed grid of G workgroups, workgroup s walks the 512-row slabs s, s + G, ...; a wave owns every
//                     fourth column, sums a column of the slab over its lanes (shuffles) and keeps the running sum of the column in LDS.
//   normal matvec     q = A^T (A d) + delta d with A read ONCE: the same static walk over R-row slabs; a slab is staged in LDS while t = A d is
//                     formed for its rows, then the partial q is advanced from the staged copy (a thread owns columns, registers hold its sums).
//   pcg_saddle steps  the n-length updates of one iteration with alpha, beta and delta_1 kept on the device.
//
// No kernel here waits for another workgroup and none uses a floating-point atomic: every sum over rows ends in one partial per workgroup
// and column in the scratch arena (G x n values) and a final pass that adds the partials in a fixed order.  The assignment of slabs to
// workgroups is static, so results are bitwise reproducible.  Sums are taken in the precision of the data.
#include "rlhip_internal.h"
#include "rlhip_device.h"

namespace {

using namespace rlhip_dev;

constexpr int GEMV_T_ROWS = 512;                  // rows of a slab of the 'T' kernel: 8 per lane
constexpr int GEMV_T_COLS = 4096;                 // columns a workgroup of the 'T' kernel keeps running sums for (32 KiB of LDS in fp64)
constexpr int FUSED_MIN_ROWS = 16;                // shortest slab of the fused kernel: a 128-B column segment in fp64
constexpr int FUSED_MAX_ROWS = 256;
constexpr int FUSED_THREADS = 1024;
constexpr int FUSED_STAGED = 16;                  // values of a slab a thread holds in registers: R n <= FUSED_STAGED * FUSED_THREADS (128 KiB in
                                                  // fp64, 64 KiB in fp32); an fp32 slab of 16 rows may take twice that (n up to 2048)
constexpr size_t FUSED_LDS_BYTES = 160 << 10;
// widest n of the fused kernel; emax = staged values a thread holds in registers (n / NG at R = 16), kmax = columns of the partial q a thread owns
template <typename T> struct FusedLimit;
template <> struct FusedLimit<double> {
    static constexpr int max_n = RLHIP_NORMAL_FUSED_MAX_N_F64, emax = max_n * FUSED_MIN_ROWS / FUSED_THREADS, kmax = max_n / FUSED_THREADS;
    static constexpr int default_max_n = RLHIP_NORMAL_FUSED_DEFAULT_MAX_N_F64;
};
template <> struct FusedLimit<float> {
    static constexpr int max_n = RLHIP_NORMAL_FUSED_MAX_N_F32, emax = max_n * FUSED_MIN_ROWS / FUSED_THREADS, kmax = max_n / FUSED_THREADS;
    static constexpr int default_max_n = RLHIP_NORMAL_FUSED_DEFAULT_MAX_N_F32;
};
static_assert((size_t)RLHIP_NORMAL_FUSED_MAX_N_F64 * FUSED_MIN_ROWS * sizeof(double) == (128 << 10) &&
              (size_t)RLHIP_NORMAL_FUSED_MAX_N_F32 * FUSED_MIN_ROWS * sizeof(float) == (128 << 10), "the limits in rlhip.h are 16-row slabs of 128 KiB");
static_assert(FusedLimit<double>::emax == FUSED_STAGED && FusedLimit<float>::emax == 2 * FUSED_STAGED, "");

__host__ __device__ inline int64_t imin(int64_t a, int64_t b) { return a < b ? a : b; }

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

// ---- (c) the final pass: out[j] = alpha * sum_g part[g * n + j] + coef * xvec[j] (coef == 0 does not read xvec; out may be xvec).  A workgroup
// owns 64 columns; wave w adds the w-th quarter of the partials in order, the four quarters are added in wave order.
template <typename T>
__global__ __launch_bounds__(256) void reduce_partials_kernel(int64_t G, int64_t n, const T* __restrict__ part, T alpha, T coef, const T* xvec, T* out) {
    __shared__ T wsum[4 * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t j = (int64_t)blockIdx.x * 64 + lane;
    const int64_t gq = (G + 3) / 4, g0 = wave * gq, g1 = imin(G, g0 + gq);
    T acc = T(0);
    if (j < n) {
#pragma unroll 8
        for (int64_t g = g0; g < g1; ++g) acc += part[g * n + j];
    }
    wsum[wave * 64 + lane] = acc;
    __syncthreads();
    if (wave == 0 && j < n) {
        const T s = alpha * (((wsum[lane] + wsum[64 + lane]) + wsum[128 + lane]) + wsum[192 + lane]);
        out[j] = coef == T(0) ? s : s + coef * xvec[j];
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

template <typename T>
__global__ __launch_bounds__(256) void dot_kernel(int64_t n, const T* __restrict__ x, const T* __restrict__ y, T* __restrict__ out) {
    __shared__ T ws[4];
    const T s = block_dot(n, x, y, ws);
    if (threadIdx.x == 0) *out = s;
}

// ---- (d) the fused normal matvec: FUSED_THREADS threads, one workgroup per CU.  Dynamic LDS: S (n columns of R + 1), dS (n), tp (one per
// thread), ts (R).
// Staging: thread tid owns row r = tid % R of the slab and the columns g, g + NG, ... (g = tid / R, NG = FUSED_THREADS / R; at most EMAX of
// them), so a wave reads 64 / R column segments of R contiguous values.  The values of a slab wait in registers: they are loaded while the
// workgroup still works on the slab before (the loads are issued right after the staged copy of that slab is complete), then go to LDS and
// into the thread's share of t[r].  The NG shares of a row are added in order.
// Partial q: thread tid owns the columns jj, jj + CW, ... (jj = tid % CW) and the rows h, h + RH, ... of the slab (h = tid / CW,
// RH = FUSED_THREADS / CW; CW = FUSED_THREADS unless n is smaller); its sums stay in registers over all slabs of the workgroup, and the RH
// shares of a column are added in order at the end.
template <typename T, int EMAX, int KMAX>
__global__ __launch_bounds__(FUSED_THREADS) void normal_fused_kernel(int64_t m, int n, int R, int CW, const T* __restrict__ A, int64_t lda,
                                                                     const T* __restrict__ d, T* __restrict__ t_out, T* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) char lsq_smem[];
    const int LDR = R + 1;
    T* S = (T*)lsq_smem;
    T* dS = S + (size_t)n * LDR;
    T* tp = dS + n;
    T* ts = tp + FUSED_THREADS;
    const int tid = threadIdx.x;
    const int r = tid & (R - 1), g = tid / R, NG = FUSED_THREADS / R;
    const int jj = tid & (CW - 1), h = tid / CW, RH = FUSED_THREADS / CW;
    for (int j = tid; j < n; j += FUSED_THREADS) dS[j] = d[j];
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
    } else {                                                                      // CW >= n: one column per thread, RH * n <= FUSED_THREADS shares
        if (jj < n) tp[h * n + jj] = acc[0];
        __syncthreads();
        if (tid < n) {
            T sum = T(0);
            for (int hh = 0; hh < RH; ++hh) sum += tp[hh * n + tid];
            mine[tid] = sum;
        }
    }
}

// ---- (e) the vector steps of pcg_saddle
template <typename T>
__global__ __launch_bounds__(256) void step_xr_kernel(int64_t n, const T* __restrict__ d, const T* __restrict__ q, const T* __restrict__ dq,
                                                      const T* __restrict__ delta1, T* __restrict__ x, T* __restrict__ r) {
    const T alpha = *delta1 / *dq;                                                                        // rl_determiter.hh:86
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        x[i] += alpha * d[i];                                                                             // :89
        if (q) r[i] -= alpha * q[i];                                                                      // :106
    }
}

template <typename T>
__global__ __launch_bounds__(256) void step_refresh_kernel(int64_t n, const T* __restrict__ b1, const T* __restrict__ qx, T delta, const T* __restrict__ x,
                                                           T* __restrict__ r) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        T v = b1[i] - qx[i];                                                                              // :101-102
        if (delta > T(0)) v -= delta * x[i];                                                              // :103
        r[i] = v;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void step_d_kernel(int64_t n, const T* __restrict__ r, const T* __restrict__ s, const T* delta1_old, T* delta1_new,
                                                     T* __restrict__ d) {
    __shared__ T ws[4];
    const T dnew = block_dot(n, r, s, ws);                                                                // :118
    if (delta1_old) {
        const T beta = dnew / *delta1_old;                                                                // :119
        for (int64_t i = threadIdx.x; i < n; i += 256) d[i] = beta * d[i] + s[i];                         // :120-122
    }
    if (threadIdx.x == 0) *delta1_new = dnew;
}

inline unsigned stream_grid(rlhip_ctx* c, int64_t n) {
    const int64_t want = (n + 255) / 256, cap = c->num_cu;
    return (unsigned)(want < 1 ? 1 : (want < cap ? want : cap));
}

template <typename T, int EMAX, int KMAX>
int launch_fused(rlhip_ctx* c, int64_t G, size_t lds, int64_t m, int n, int R, int CW, const T* A, int64_t lda, const T* d, T* t, T* part) {
    RLHIP_FUNC_LDS(c, (normal_fused_kernel<T, EMAX, KMAX>), FUSED_LDS_BYTES);
    hipLaunchKernelGGL((normal_fused_kernel<T, EMAX, KMAX>), dim3((unsigned)G), dim3(FUSED_THREADS), lds, c->stream, m, n, R, CW, A, lda, d, t, part);
    return 0;
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
    hipLaunchKernelGGL(reduce_partials_kernel<T>, dim3((unsigned)((n + 63) / 64)), dim3(256), 0, c->stream, G, n, part, alpha, coef, xvec, out);
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
        int R = FUSED_MAX_ROWS;
        while (R > FUSED_MIN_ROWS && (int64_t)R * n > (int64_t)FUSED_STAGED * FUSED_THREADS) R >>= 1;
        while (R > FUSED_MIN_ROWS && R / 2 >= m) R >>= 1;
        int CW = FUSED_THREADS;
        while (CW / 2 >= n) CW >>= 1;
        const int64_t nslab = (m + R - 1) / R;
        const int64_t G = imin(nslab, max_wg > 0 ? max_wg : (int64_t)c->num_cu);
        // S, dS, tp, ts: at most 17/16 of the slab budget + (max_n + FUSED_THREADS + FUSED_MAX_ROWS) values
        const size_t lds = ((size_t)n * (R + 1) + n + FUSED_THREADS + R) * sizeof(T);
        if (lds > FUSED_LDS_BYTES) return RLHIP_ERR_HIP(hipErrorInvalidValue);
        ws_scope ws(c);
        T* part = nullptr;
        if (G > 0) {
            part = ws.alloc<T>((size_t)(G * n));
            if (!part) return RLHIP_ERR_HIP(hipErrorOutOfMemory);
            int rc;
            if ((int64_t)R * n > (int64_t)FUSED_STAGED * FUSED_THREADS)           // fp32, n > 1024: 32 staged values and two columns of q per thread
                rc = launch_fused<T, FusedLimit<T>::emax, FusedLimit<T>::kmax>(c, G, lds, m, (int)n, R, CW, A, lda, d, t, part);
            else
                rc = launch_fused<T, FUSED_STAGED, 1>(c, G, lds, m, (int)n, R, CW, A, lda, d, t, part);
            if (rc) return rc;
        }
        hipLaunchKernelGGL(reduce_partials_kernel<T>, dim3((unsigned)((n + 63) / 64)), dim3(256), 0, c->stream, G, n, part, T(1), delta, d, q);
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
    if (dq_dev) hipLaunchKernelGGL(dot_kernel<T>, dim3(1), dim3(256), 0, c->stream, n, d, q, dq_dev);
    RLHIP_LAUNCH_CHECK();
    return 0;
}

template <typename T>
int step_xr(rlhip_ctx* c, int64_t n, const T* d, const T* q, const T* dq_dev, const T* delta1_dev, T* x, T* r) {
    if (n < 0) return -2;
    if (n > 0 && !d) return -3;
    if (!dq_dev) return -5;
    if (!delta1_dev) return -6;
    if (n > 0 && !x) return -7;
    if (n > 0 && q && !r) return -8;
    if (n == 0) return 0;
    hipLaunchKernelGGL(step_xr_kernel<T>, dim3(stream_grid(c, n)), dim3(256), 0, c->stream, n, d, q, dq_dev, delta1_dev, x, r);
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
    hipLaunchKernelGGL(step_refresh_kernel<T>, dim3(stream_grid(c, n)), dim3(256), 0, c->stream, n, b1, qx, delta, x, r);
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
    hipLaunchKernelGGL(step_d_kernel<T>, dim3(1), dim3(256), 0, c->stream, n, r, s, delta1_old_dev, delta1_new_dev, d);
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
    const int64_t leny = trans == NoTrans ? m : n;
    if (trans == Trans) {
        c->lsq_path_count[3]++;
        return gemv_t<T>(c, m, n, A, lda, x, alpha, beta, y, y);
    }
    c->lsq_path_count[2]++;
    if (alpha == T(0))
        hipLaunchKernelGGL(reduce_partials_kernel<T>, dim3((unsigned)((leny + 63) / 64)), dim3(256), 0, c->stream, (int64_t)0, leny, (const T*)nullptr,
                           T(0), beta, y, y);
    else
        hipLaunchKernelGGL(gemv_n_kernel<T>, dim3((unsigned)((m + 63) / 64)), dim3(256), 0, c->stream, m, n, alpha, A, lda, x, beta, y);
    RLHIP_LAUNCH_CHECK();
    return 0;
}
template int gemv<double>(rlhip_ctx*, int, int64_t, int64_t, double, const double*, int64_t, const double*, double, double*);
template int gemv<float>(rlhip_ctx*, int, int64_t, int64_t, float, const float*, int64_t, const float*, float, float*);

template <typename T>
int dot_dev(rlhip_ctx* c, int64_t n, const T* x, const T* y, T* out_dev) {
    hipLaunchKernelGGL(dot_kernel<T>, dim3(1), dim3(256), 0, c->stream, n, x, y, out_dev);
    RLHIP_LAUNCH_CHECK();
    return 0;
}
template int dot_dev<double>(rlhip_ctx*, int64_t, const double*, const double*, double*);
template int dot_dev<float>(rlhip_ctx*, int64_t, const float*, const float*, float*);

}  // namespace rlhip

extern "C" {

int64_t rlhip_lsq_path_count(rlhip_ctx* c, int which) { return (c && which >= 46 && which <= 49) ? c->lsq_path_count[which - 46] : -1; }

#define RLHIP_DEFINE_LSQ(SUF, T)                                                                                                             \
    int rlhip_gemv_##SUF(rlhip_ctx* c, char trans, int64_t m, int64_t n, T alpha, const T* A, int64_t lda, const T* x, T beta, T* y) {       \
        return rlhip::gemv<T>(c, trans_of(trans), m, n, alpha, A, lda, x, beta, y);                                                          \
    }                                                                                                                                        \
    int rlhip_normal_matvec_##SUF(rlhip_ctx* c, int64_t m, int64_t n, const T* A, int64_t lda, const T* d, T delta, T* q, T* t, T* dq_dev,   \
                                  int64_t max_wg) {                                                                                          \
        return normal_matvec<T>(c, m, n, A, lda, d, delta, q, t, dq_dev, max_wg);                                                            \
    }                                                                                                                                        \
    int rlhip_pcg_saddle_step_xr_##SUF(rlhip_ctx* c, int64_t n, const T* d, const T* q, const T* dq_dev, const T* delta1_dev, T* x, T* r) {  \
        return step_xr<T>(c, n, d, q, dq_dev, delta1_dev, x, r);                                                                             \
    }                                                                                                                                        \
    int rlhip_pcg_saddle_step_refresh_##SUF(rlhip_ctx* c, int64_t n, const T* b1, const T* qx, T delta, const T* x, T* r) {                  \
        return step_refresh<T>(c, n, b1, qx, delta, x, r);                                                                                   \
    }                                                                                                                                        \
    int rlhip_pcg_saddle_step_d_##SUF(rlhip_ctx* c, int64_t n, const T* r, const T* s, const T* delta1_old_dev, T* delta1_new_dev, T* d) {   \
        return step_d<T>(c, n, r, s, delta1_old_dev, delta1_new_dev, d);                                                                     \
    }
RLHIP_DEFINE_LSQ(f64, double)
RLHIP_DEFINE_LSQ(f32, float)

}  // extern "C"
