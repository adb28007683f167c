// Least squares with several right-hand sides: the normal product on a block of columns and the lockstep vector steps of
// pcg_saddle_block (include/RandLAPACK_amd/rl_determiter.hh).
//
//   normal matmat     Q (n x s) = A^T (A D) + delta D.  One-pass route: the static slab walk of lsq.hip's fused normal matvec, with the staged
//                     slab used for every column of a chunk: T_slab (R x SC) = S D, then the partial Q (n x SC) += S^T T_slab; A is read
//                     from memory once per chunk of SC columns.  Composed route: T = A D and Q = A^T T through the library's GEMM.
//   block steps       the n-length updates of one iteration for s columns kept in lockstep: alpha_j, beta_j, delta1_j and d_j^T q_j stay on
//                     the device, a column whose flag active_j is off is not touched.
//
// The rules are lsq.hip's: no kernel waits for another workgroup, none uses a floating-point atomic, slabs are assigned statically, every
// sum over rows ends in one partial per workgroup and column in the scratch arena and a final pass in a fixed order.  On top of them: column
// j of every output is a function of A, delta and column j of the inputs alone -- no sum ever mixes two columns.
#include "rlhip_internal.h"
#include "rlhip_device.h"

namespace {

using namespace rlhip_dev;

constexpr int BLK_THREADS = 1024;
constexpr int BLK_MIN_ROWS = 16;
constexpr int BLK_MAX_ROWS = 256;
constexpr size_t BLK_LDS_BYTES = 160 << 10;
// a slab is half of lsq.hip's (64 KiB): the other half of the LDS holds D, the shares of T_slab and T_slab itself for a chunk of columns.
// staged = values of a slab a thread holds in registers (R n <= staged * BLK_THREADS), max_sc = the widest chunk
template <typename T> struct BlockLimit;
template <> struct BlockLimit<double> { static constexpr int staged = 8, max_sc = RLHIP_NORMAL_MATMAT_FUSED_SC_F64; };
template <> struct BlockLimit<float> { static constexpr int staged = 16, max_sc = RLHIP_NORMAL_MATMAT_FUSED_SC_F32; };
static_assert(RLHIP_NORMAL_MATMAT_FUSED_MAX_N * BLK_MIN_ROWS == BlockLimit<double>::staged * BLK_THREADS, "the limit in rlhip.h is a 16-row fp64 slab");
static_assert(RLHIP_NORMAL_MATMAT_FUSED_MAX_N * 2 * BLK_MIN_ROWS == BlockLimit<float>::staged * BLK_THREADS, "and a 32-row fp32 slab");
static_assert(BlockLimit<double>::max_sc == 4 && BlockLimit<float>::max_sc == 4, "the widest instantiation: in fp32 a chunk of 8 spills inside the slab loop");
static_assert(2 * RLHIP_NORMAL_MATMAT_FUSED_MAX_N <= BLK_THREADS, "a thread owns one column of the partial Q and at least two threads share a column");

__host__ __device__ inline int64_t imin(int64_t a, int64_t b) { return a < b ? a : b; }

// chunk width of the one-pass route for (n, s); 0 outside its limits
inline int block_chunk(int64_t n, int64_t s, int elem_bytes) {
    if (n < 1 || n > RLHIP_NORMAL_MATMAT_FUSED_MAX_N || s < 1) return 0;
    const int cap = elem_bytes == 8 ? RLHIP_NORMAL_MATMAT_FUSED_SC_F64 : (elem_bytes == 4 ? RLHIP_NORMAL_MATMAT_FUSED_SC_F32 : 0);
    return (int)imin(s, cap);
}

// where the one-pass route is taken unasked: the (precision, n, s) ranges in which it measured faster than both the composed route and s
// single calls of rlhip_normal_matvec by more than the run-to-run spread: 2 <= s <= 8, and n in the slab configurations (R, CW)
// that were measured or lie between two measured ones: 33 .. 256 in fp64 (n = 64 and 256 measured), 129 .. 256 in fp32 (n = 256 measured)
inline int block_default(int64_t n, int64_t s, int elem_bytes) {
    if (!block_chunk(n, s, elem_bytes) || s < 2 || s > 8 || n > 256) return 0;
    return n >= (elem_bytes == 8 ? 33 : 129) ? 1 : 0;
}

// ---- (a) the one-pass kernel for w <= SC columns of D.  BLK_THREADS threads, one workgroup per CU.  Dynamic LDS: S (n columns of R + 1),
// dS (n x SC, column index fastest; columns w .. SC - 1 are zero), tp (SC x BLK_THREADS shares), ts (R x SC, column index fastest).
// Staging is normal_fused_kernel's (lsq.hip): thread tid owns row r = tid % R of the slab and the columns g, g + NG, ... (g = tid / R,
// NG = BLK_THREADS / R, at most EMAX of them); the values of the next slab wait in registers while this one is worked on.  A thread adds its
// share of T_slab(r, c) for every c; the NG shares are added in order of g.  Partial Q: thread tid owns column jj = tid % CW and the rows
// h, h + RH, ... of the slab (h = tid / CW, RH = BLK_THREADS / CW >= 2, CW the least power of two >= n); its SC sums stay in registers
// over all slabs of the workgroup, and the RH shares of a column are added in order at the end.
// part: w blocks of gridDim.x x n values, block c = column c.
template <typename T, int EMAX, int SC>
__global__ __launch_bounds__(BLK_THREADS) void normal_block_kernel(int64_t m, int n, int w, int R, int CW, const T* __restrict__ A, int64_t lda,
                                                                   const T* __restrict__ D, int64_t ldd, T* __restrict__ t_out, int64_t ldt,
                                                                   T* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) char lsqb_smem[];
    const int LDR = R + 1;
    T* S = (T*)lsqb_smem;
    T* dS = S + (((size_t)n * LDR + 3) & ~(size_t)3);
    T* tp = dS + (size_t)n * SC;
    T* ts = tp + (size_t)BLK_THREADS * SC;
    const int tid = threadIdx.x;
    const int r = tid & (R - 1), g = tid / R, NG = BLK_THREADS / R;
    const int jj = tid & (CW - 1), h = tid / CW, RH = BLK_THREADS / CW;
    for (int o = tid; o < n * SC; o += BLK_THREADS) {
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
        for (int c = 0; c < SC; ++c) tp[c * BLK_THREADS + tid] = tacc[c];         // = tp[(c * NG + g) * R + r]
        __syncthreads();
        if (s + gridDim.x < nslab) fetch(s + gridDim.x);                          // in flight while this slab is worked on
        for (int o = tid; o < R * SC; o += BLK_THREADS) {
            const int c = o / R, row = o - c * R;
            const T* sh = tp + c * BLK_THREADS + row;
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
    // RH * n <= BLK_THREADS shares of every column
    if (jj < n) {
#pragma unroll
        for (int c = 0; c < SC; ++c) tp[c * BLK_THREADS + h * n + jj] = acc[c];
    }
    __syncthreads();
    for (int o = tid; o < n * w; o += BLK_THREADS) {
        const int c = o / n, j = o - c * n;
        const T* sh = tp + c * BLK_THREADS + j;
        T sum = T(0);
        for (int hh = 0; hh < RH; ++hh) sum += sh[hh * n];
        part[((int64_t)c * gridDim.x + blockIdx.x) * n + j] = sum;
    }
}

// ---- (b) the final pass for w columns: Q(j, c) = sum_g part[(c G + g) n + j] + delta D(j, c) (delta == 0 does not read D).  blockIdx.y = c; a
// workgroup owns 64 rows of Q, wave v adds the v-th quarter of the partials in order, the four quarters are added in wave order.  G == 0
// (m == 0): Q = delta D.
template <typename T>
__global__ __launch_bounds__(256) void reduce_block_kernel(int64_t G, int64_t n, const T* __restrict__ part, T delta, const T* __restrict__ D, int64_t ldd,
                                                           T* __restrict__ Q, int64_t ldq) {
    __shared__ T wsum[4 * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t c = blockIdx.y;
    const int64_t j = (int64_t)blockIdx.x * 64 + lane;
    const int64_t gq = (G + 3) / 4, g0 = wave * gq, g1 = imin(G, g0 + gq);
    T acc = T(0);
    if (j < n) {
        const T* p = part + c * G * n + j;
#pragma unroll 8
        for (int64_t gi = g0; gi < g1; ++gi) acc += p[gi * n];
    }
    wsum[wave * 64 + lane] = acc;
    __syncthreads();
    if (wave == 0 && j < n) {
        const T sum = ((wsum[lane] + wsum[64 + lane]) + wsum[128 + lane]) + wsum[192 + lane];
        Q[j + c * ldq] = delta == T(0) ? sum : sum + delta * D[j + c * ldd];
    }
}

// Q += delta D on an n x s block (the composed route's last step)
template <typename T>
__global__ __launch_bounds__(256) void add_delta_kernel(int64_t n, int64_t s, T delta, const T* __restrict__ D, int64_t ldd, T* __restrict__ Q, int64_t ldq) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    for (int64_t c = blockIdx.y; c < s; c += gridDim.y) Q[j + c * ldq] += delta * D[j + c * ldd];
}

// x^T y by ONE workgroup of 256 threads, every thread gets it, in the order of lsq.hip's block_dot: thread t adds the entries t, t + 256,
// ... in order, the 64 lanes of a wave are added by shuffles, the four waves in order.  ws: 4 values of LDS, free again on return.
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

// ---- (c) the lockstep vector steps; blockIdx.y = column.  A column whose flag is off is left alone.
template <typename T>
__global__ __launch_bounds__(256) void block_step_xr_kernel(int64_t n, const T* __restrict__ D, int64_t ldd, const T* __restrict__ Q, int64_t ldq,
                                                            const T* __restrict__ dq, const T* __restrict__ delta1, int64_t ldh, T* __restrict__ X,
                                                            int64_t ldx, T* __restrict__ Rm, int64_t ldr, const int* __restrict__ active) {
    const int64_t c = blockIdx.y;
    if (!active[c]) return;
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
    if (!active[c]) return;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        T v = B1[i + c * ldb1] - QX[i + c * ldqx];                                                        // :101-102
        if (delta > T(0)) v -= delta * X[i + c * ldx];                                                    // :103
        Rm[i + c * ldr] = v;
    }
}

// one workgroup per column.  delta1_old == nullptr: the first call; it forms rel_sq_tol and sets the flag whatever it held.
template <typename T>
__global__ __launch_bounds__(256) void block_step_d_kernel(int64_t n, const T* __restrict__ Rm, int64_t ldr, const T* __restrict__ Sm, int64_t lds,
                                                           const T* delta1_old, T* delta1_new, int64_t ldh, T* __restrict__ D, int64_t ldd, T tol,
                                                           T* __restrict__ rel_sq_tol, int* __restrict__ active) {
    __shared__ T ws[4];
    const int64_t c = blockIdx.x;
    if (delta1_old && !active[c]) return;                                         // uniform over the workgroup
    const T* s = Sm + c * lds;
    const T dnew = block_dot(n, Rm + c * ldr, s, ws);                                                     // :118 (:69)
    if (delta1_old) {
        const T beta = dnew / delta1_old[c * ldh];                                                        // :119
        T* d = D + c * ldd;
        for (int64_t i = threadIdx.x; i < n; i += 256) d[i] = beta * d[i] + s[i];                         // :120-122
    }
    if (threadIdx.x == 0) {
        delta1_new[c * ldh] = dnew;
        T lim;
        if (delta1_old) lim = rel_sq_tol[c];
        else rel_sq_tol[c] = lim = (dnew * tol) * tol;                                                    // :71
        active[c] = dnew > lim ? 1 : 0;                                           // false for a NaN: the column stops (:76)
    }
}

inline unsigned stream_grid(rlhip_ctx* c, int64_t n) {
    const int64_t want = (n + 255) / 256, cap = c->num_cu;
    return (unsigned)(want < 1 ? 1 : (want < cap ? want : cap));
}
constexpr int64_t GRID_Y_MAX = 65535;

template <typename T, int SC>
int launch_block(rlhip_ctx* c, int64_t G, size_t lds, int64_t m, int n, int w, int R, int CW, const T* A, int64_t lda, const T* D, int64_t ldd, T* t,
                 int64_t ldt, T* part) {
    constexpr int EMAX = BlockLimit<T>::staged;
    RLHIP_FUNC_LDS(c, (normal_block_kernel<T, EMAX, SC>), BLK_LDS_BYTES);
    hipLaunchKernelGGL((normal_block_kernel<T, EMAX, SC>), dim3((unsigned)G), dim3(BLK_THREADS), lds, c->stream, m, n, w, R, CW, A, lda, D, ldd, t, ldt,
                       part);
    return 0;
}

// the one-pass route for w <= max_sc columns (m, n > 0)
template <typename T>
int block_chunk_pass(rlhip_ctx* c, int64_t m, int n, int w, const T* A, int64_t lda, const T* D, int64_t ldd, T delta, T* Q, int64_t ldq, T* t, int64_t ldt,
                     int64_t max_wg) {
    const int SC = w <= 1 ? 1 : (w <= 2 ? 2 : 4);
    int R = BLK_MAX_ROWS;
    while (R > BLK_MIN_ROWS && (int64_t)R * n > (int64_t)BlockLimit<T>::staged * BLK_THREADS) R >>= 1;
    while (R > BLK_MIN_ROWS && R / 2 >= m) R >>= 1;
    int CW = BLK_THREADS / 2;
    while (CW / 2 >= n) CW >>= 1;
    const int64_t nslab = (m + R - 1) / R;
    const int64_t G = imin(nslab, max_wg > 0 ? max_wg : (int64_t)c->num_cu);
    const size_t lds = ((((size_t)n * (R + 1) + 3) & ~(size_t)3) + (size_t)n * SC + (size_t)BLK_THREADS * SC + (size_t)R * SC) * sizeof(T);
    if ((int64_t)R * n > (int64_t)BlockLimit<T>::staged * BLK_THREADS || lds > BLK_LDS_BYTES || w > BlockLimit<T>::max_sc)
        return RLHIP_ERR_HIP(hipErrorInvalidValue);
    ws_scope ws(c);
    T* part = ws.alloc<T>((size_t)(G * n * w));
    if (!part) return RLHIP_ERR_HIP(hipErrorOutOfMemory);
    int rc;
    if (SC == 1) rc = launch_block<T, 1>(c, G, lds, m, n, w, R, CW, A, lda, D, ldd, t, ldt, part);
    else if (SC == 2) rc = launch_block<T, 2>(c, G, lds, m, n, w, R, CW, A, lda, D, ldd, t, ldt, part);
    else rc = launch_block<T, 4>(c, G, lds, m, n, w, R, CW, A, lda, D, ldd, t, ldt, part);
    if (rc) return rc;
    hipLaunchKernelGGL(reduce_block_kernel<T>, dim3((unsigned)((n + 63) / 64), (unsigned)w), dim3(256), 0, c->stream, G, (int64_t)n, part, delta, D, ldd, Q,
                       ldq);
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
            hipLaunchKernelGGL(reduce_block_kernel<T>, dim3((unsigned)((n + 63) / 64), (unsigned)imin(s - c0, GRID_Y_MAX)), dim3(256), 0, c->stream, (int64_t)0, n,
                               (const T*)nullptr, delta, D + c0 * ldd, ldd, Q + c0 * ldq, ldq);
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

}  // namespace

extern "C" {

int rlhip_normal_matmat_fused(int64_t n, int64_t s, int elem_bytes) { return block_chunk(n, s, elem_bytes); }

int rlhip_normal_matmat_default(int64_t n, int64_t s, int elem_bytes) { return block_default(n, s, elem_bytes); }

int rlhip_normal_matmat_set_route(rlhip_ctx* c, int route) {
    if (!c) return -1;
    const int was = c->matmat_route;
    c->matmat_route = route < 0 ? -1 : (route > 0 ? 1 : 0);
    return was;
}

int64_t rlhip_lsq_block_path_count(rlhip_ctx* c, int which) { return (c && which >= 76 && which <= 78) ? c->lsq_block_path_count[which - 76] : -1; }

#define RLHIP_DEFINE_LSQ_BLOCK(SUF, T)                                                                                                                 \
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
RLHIP_DEFINE_LSQ_BLOCK(f64, double)
RLHIP_DEFINE_LSQ_BLOCK(f32, float)

}  // extern "C"
