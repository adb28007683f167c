// Randomly pivoted Cholesky (RandLAPACK/comps/rl_rpchol.hh) and the squared-exponential kernel matrix
// (RandLAPACK/misc/rl_pdkernels.hh) on the device.
//
//   sqexp_columns      out(i, l) = exp(-sum_r (X(r,i) - X(r,idx[l]))^2 / (2 h^2)) [+ reg where i == idx[l]]: the reference's
//                      A_stateless(i, j) (squared_exp_kernel, rl_pdkernels.hh:102) evaluated as compute_columns does (rl_rpchol.hh:19).
//                      Differences, not the norm expansion, so the diagonal is exactly 1.
//   sqexp_submatrix    squared_exp_kernel_submatrix (rl_pdkernels.hh:133): MFMA GEMM for -2 X_rows^T X_cols, then one epilogue kernel
//                      adds the squared column norms and takes exp.
//   rbf_apply          linops::RBFKernelMatrix::operator() (rl_pdkernels.hh:255-283) by full row blocks of K.
//   pdk_*              the three routines above with the kernel function as an argument: the squared exponential or Matern
//                      3/2, 5/2.  The two device kernels that evaluate it take it as a template flag; the squared exponential's code is
//                      the one it always was.
//   sample_indices_iid RandBLAS::weights_to_cdf + sample_indices_iid (rl_rpchol.hh:64, 131, 141); the stream is this library's own and
//                      is specified in include/rlhip.h.
//   rpchol_panel_finish the trsm of rl_rpchol.hh:174 followed by the downdate of :47-62 (d -= row norms^2, d[S'] = 0).
#include <cmath>
#include <cfloat>
#include <cstring>
#include "rlhip_internal.h"
#include "rlhip_device.h"

namespace {
using rlhip::PdkFn;

constexpr int COL_TILE_L = 64;      // kernel columns per workgroup (accumulators per thread)
constexpr int COL_TILE_R = 64;      // feature rows staged per LDS chunk
constexpr int SAMPLE_CHUNK = 256;   // weights per chunk of the blocked prefix sum
constexpr int SORT_MAX = 4096;      // largest block the sampler sorts / de-duplicates in LDS

__host__ __device__ inline void philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
    const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
    uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3];
    uint32_t k0 = key[0], k1 = key[1];
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        uint64_t p0 = (uint64_t)M0 * c0;
        uint64_t p1 = (uint64_t)M1 * c2;
        uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        uint32_t n1 = (uint32_t)p1;
        uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        uint32_t n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += W0; k1 += W1;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

__host__ __device__ inline void ctr_add(const uint32_t base[4], uint64_t inc, uint32_t out[4]) {
    uint64_t lo = ((uint64_t)base[1] << 32) | base[0];
    uint64_t hi = ((uint64_t)base[3] << 32) | base[2];
    uint64_t nlo = lo + inc;
    if (nlo < lo) hi += 1;
    out[0] = (uint32_t)nlo; out[1] = (uint32_t)(nlo >> 32);
    out[2] = (uint32_t)hi;  out[3] = (uint32_t)(hi >> 32);
}

struct RngState {
    uint32_t ctr[4];
    uint32_t key[2];
};

__device__ inline double dexp(double x) { return exp(x); }
__device__ inline float dexp(float x) { return expf(x); }

// ---- (a) kernel columns.  Workgroup: 256 points x COL_TILE_L indices; X(:, idx tile) is staged in LDS COL_TILE_R rows at a time, each
// thread keeps COL_TILE_L accumulators and reads its own point's features once per index tile.  MATERN: the squared distance goes through
// matern_of_s(s, cs, third) instead of exp(-s * cs), cs = 1 / (2 h^2) there and sqrt(3) / l, sqrt(5) / l here; s = 0 gives exactly 1 in both.
template <typename T, bool MATERN>
__global__ __launch_bounds__(256) void sqexp_columns_kernel(int64_t rows_x, int64_t n, const T* __restrict__ X, int64_t ldx, int64_t nidx,
                                                            const int64_t* __restrict__ idx, T cs, T third, T reg, T* __restrict__ out,
                                                            int64_t ldo) {
    __shared__ T xs[COL_TILE_R * COL_TILE_L];
    __shared__ int64_t js[COL_TILE_L];
    const int tid = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * 256 + tid;
    const int64_t l0 = (int64_t)blockIdx.y * COL_TILE_L;
    const int lcnt = (int)((nidx - l0) < COL_TILE_L ? (nidx - l0) : COL_TILE_L);
    if (tid < COL_TILE_L) js[tid] = tid < lcnt ? idx[l0 + tid] : -1;
    T acc[COL_TILE_L];
#pragma unroll
    for (int l = 0; l < COL_TILE_L; ++l) acc[l] = T(0);
    const T* xi = X + (i < n ? i : 0) * ldx;
    for (int64_t r0 = 0; r0 < rows_x; r0 += COL_TILE_R) {
        const int rc = (int)((rows_x - r0) < COL_TILE_R ? (rows_x - r0) : COL_TILE_R);
        __syncthreads();
        for (int t = tid; t < COL_TILE_R * COL_TILE_L; t += 256) {
            const int r = t % COL_TILE_R, l = t / COL_TILE_R;
            xs[r * COL_TILE_L + l] = (r < rc && l < lcnt) ? X[(r0 + r) + js[l] * ldx] : T(0);
        }
        __syncthreads();
        if (i < n) {
            for (int r = 0; r < rc; ++r) {
                const T xv = xi[r0 + r];
#pragma unroll
                for (int l = 0; l < COL_TILE_L; ++l) {
                    const T df = xv - xs[r * COL_TILE_L + l];
                    acc[l] += df * df;
                }
            }
        }
    }
    if (i >= n) return;
#pragma unroll
    for (int l = 0; l < COL_TILE_L; ++l) {
        if (l < lcnt) {
            T v;
            if constexpr (MATERN) v = rlhip_dev::matern_of_s(acc[l], cs, third);
            else v = dexp(-(acc[l] * cs));
            if (i == js[l]) v += reg;
            out[i + (l0 + l) * ldo] = v;
        }
    }
}

// ---- (b) norm-expansion submatrix: squared column norms, then the epilogue over the GEMM's -2 X_rows^T X_cols
template <typename T>
__global__ void sq_colnorms_kernel(int64_t rows_x, int64_t cols, const T* __restrict__ X, int64_t ldx, T* __restrict__ nr) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= cols) return;
    T s = T(0);
    for (int64_t r = 0; r < rows_x; ++r) { const T v = X[r + j * ldx]; s += v * v; }
    nr[j] = s;
}

template <typename T, bool MATERN, bool WEIGHT = false>
__global__ void sqexp_epilogue_kernel(int64_t rows, int64_t cols, const T* __restrict__ nr_rows, const T* __restrict__ nr_cols, T scale, T third,
                                      T* __restrict__ K, int64_t ldk) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t j = blockIdx.y;
    if (i >= rows) return;
    T* p = K + i + j * ldk;
    const T s = (nr_rows[i] + nr_cols[j]) + *p;
    if constexpr (WEIGHT) *p = rlhip_dev::pdk_weight_of_s(s, scale, third);
    else if constexpr (MATERN) *p = rlhip_dev::matern_of_s(s, scale, third);
    else *p = dexp(scale * s);
}

// ---- (c) sampler.  Chunk c holds weights [c*256, c*256 + 256); w_i = max(d_i, 0).  All sums in double:
//   loc_i   = sequential inclusive sum of w inside i's chunk, from 0
//   S_c     = loc of the chunk's last element;  off_0 = 0, off_{c+1} = off_c + S_c (sequential)
//   prefix_i = off_c + loc_i   (one rounding; prefix of a chunk's last element == off_{c+1}, so prefix is non-decreasing)
struct SampleHdr {
    double total;
    int64_t lastpos;     // last index with w > 0, -1 if none
    int64_t status;      // 0 / 1 / 2
    int64_t count;       // indices written by the draw kernel
};
static_assert(sizeof(SampleHdr) == MAIL_SAMPLE_HDR_WORDS * sizeof(int64_t), "the header is read back through its mailbox slot");

template <typename T>
__global__ void sample_partial_kernel(int64_t n, const T* __restrict__ d, double* __restrict__ S, int64_t* __restrict__ lastpos,
                                      int* __restrict__ bad, int64_t nchunks, double neg_eps) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nchunks) return;
    const int64_t i0 = c * SAMPLE_CHUNK;
    const int64_t i1 = (i0 + SAMPLE_CHUNK) < n ? (i0 + SAMPLE_CHUNK) : n;
    double s = 0.0;
    int64_t lp = -1;
    int b = 0;
    for (int64_t i = i0; i < i1; ++i) {
        const double v = (double)d[i];
        if (v != v || v < neg_eps) b = 1;
        const double w = v > 0.0 ? v : 0.0;
        s += w;
        if (w > 0.0) lp = i;
    }
    S[c] = s;
    lastpos[c] = lp;
    bad[c] = b;
}

__global__ __launch_bounds__(1024) void sample_scan_kernel(int64_t n, int64_t nchunks, const double* __restrict__ S,
                                                           const int64_t* __restrict__ lastpos, const int* __restrict__ bad,
                                                           double* __restrict__ off, double status1_below, SampleHdr* __restrict__ hdr) {
    __shared__ double buf[4096];
    __shared__ int64_t red_lp[1024];
    __shared__ int red_bad[1024];
    const int tid = threadIdx.x;
    int64_t lp = -1;
    int b = 0;
    for (int64_t c = tid; c < nchunks; c += 1024) {
        lp = lastpos[c] > lp ? lastpos[c] : lp;
        b |= bad[c];
    }
    red_lp[tid] = lp;
    red_bad[tid] = b;
    double run = 0.0;                       // held by thread 0 only
    if (tid == 0) off[0] = 0.0;
    for (int64_t c0 = 0; c0 < nchunks; c0 += 4096) {
        const int cnt = (int)((nchunks - c0) < 4096 ? (nchunks - c0) : 4096);
        __syncthreads();
        for (int t = tid; t < cnt; t += 1024) buf[t] = S[c0 + t];
        __syncthreads();
        if (tid == 0) {
            for (int t = 0; t < cnt; ++t) {
                run += buf[t];
                off[c0 + t + 1] = run;
            }
        }
    }
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if (tid < s) {
            red_lp[tid] = red_lp[tid + s] > red_lp[tid] ? red_lp[tid + s] : red_lp[tid];
            red_bad[tid] |= red_bad[tid + s];
        }
        __syncthreads();
    }
    if (tid == 0) {
        hdr->total = run;
        hdr->lastpos = red_lp[0];
        hdr->status = red_bad[0] ? 2 : (run < status1_below ? 1 : 0);
        hdr->count = 0;
    }
}

template <typename T>
__device__ int64_t sample_one(int64_t n, const T* __restrict__ d, const double* __restrict__ off, int64_t nchunks, double total,
                              int64_t lastpos, RngState st, int64_t j) {
    uint32_t c[4], r[4];
    ctr_add(st.ctr, (uint64_t)(j >> 1), c);
    philox4x32_10(c, st.key, r);
    const int h = (int)(j & 1) * 2;
    const uint64_t w = (uint64_t)r[h] | ((uint64_t)r[h + 1] << 32);
    const double u = ((double)(w >> 11) + 0.5) * 0x1.0p-53;
    const double t = u * total;
    // first chunk c with off[c+1] > t
    int64_t lo = 0, hi = nchunks;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (off[mid + 1] > t) hi = mid; else lo = mid + 1;
    }
    if (lo >= nchunks) return lastpos;
    const double base = off[lo];
    const int64_t i0 = lo * SAMPLE_CHUNK;
    const int64_t i1 = (i0 + SAMPLE_CHUNK) < n ? (i0 + SAMPLE_CHUNK) : n;
    double s = 0.0;
    for (int64_t i = i0; i < i1; ++i) {
        const double v = (double)d[i];
        s += v > 0.0 ? v : 0.0;
        if (base + s > t) return i < lastpos ? i : lastpos;
    }
    return lastpos;
}

// raw draws in draw order; any k
template <typename T>
__global__ void sample_draw_kernel(int64_t n, const T* __restrict__ d, const double* __restrict__ off, int64_t nchunks,
                                   const SampleHdr* __restrict__ hdr, RngState st, int64_t k, int64_t* __restrict__ out) {
    if (hdr->status != 0) return;
    const double total = hdr->total;
    const int64_t lastpos = hdr->lastpos;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < k; j += (int64_t)gridDim.x * blockDim.x)
        out[j] = sample_one(n, d, off, nchunks, total, lastpos, st, j);
}

// k <= SORT_MAX draws, then bitonic sort + de-duplication in LDS (rl_rpchol.hh:142-143); one workgroup
template <typename T>
__global__ __launch_bounds__(1024) void sample_draw_unique_kernel(int64_t n, const T* __restrict__ d, const double* __restrict__ off,
                                                                  int64_t nchunks, SampleHdr* __restrict__ hdr, RngState st, int64_t k,
                                                                  int64_t* __restrict__ out) {
    __shared__ int64_t keys[SORT_MAX];
    const int tid = threadIdx.x;
    if (hdr->status != 0) return;           // uniform across the workgroup
    const double total = hdr->total;
    const int64_t lastpos = hdr->lastpos;
    int P = 1;
    while (P < k) P <<= 1;
    for (int j = tid; j < P; j += 1024) keys[j] = j < k ? sample_one(n, d, off, nchunks, total, lastpos, st, j) : INT64_MAX;
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < P; t += 1024) {
                const int partner = t ^ stride;
                if (partner > t) {
                    const bool up = (t & size) == 0;
                    const int64_t a = keys[t], b = keys[partner];
                    if ((a > b) == up) { keys[t] = b; keys[partner] = a; }
                }
            }
            __syncthreads();
        }
    }
    if (tid == 0) {
        int64_t cnt = 0;
        for (int j = 0; j < k; ++j)
            if (j == 0 || keys[j] != keys[j - 1]) out[cnt++] = keys[j];
        hdr->count = cnt;
    }
}

// ---- (d) panel finish, fused (cols <= 64): thread i reads row i of G once, solves x U = G(i,:) by forward substitution in registers with U
// in LDS, writes F(i,:) = x once, and downdates d[i] -= sum_j x_j^2 (j in order, as rl_rpchol.hh:51-56); d[S'] = 0 by a binary search in
// the sorted S'.  One read and one write of the panel, where trsm + downdate take three passes.
__device__ inline bool in_sorted(const int64_t* __restrict__ s, int64_t cnt, int64_t i) {
    int64_t lo = 0, hi = cnt;
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (s[mid] < i) lo = mid + 1; else hi = mid; }
    return lo < cnt && s[lo] == i;
}

template <typename T, int MAXC>
__global__ __launch_bounds__(256) void rpchol_panel_fused_kernel(int64_t n, int cols, const T* __restrict__ U, int64_t ldu, T* __restrict__ F,
                                                                 int64_t ldf, T* __restrict__ d, const int64_t* __restrict__ sidx) {
    __shared__ T Us[MAXC * MAXC];
    for (int t = threadIdx.x; t < cols * cols; t += 256) {
        const int r = t % cols, cc = t / cols;
        Us[r + cc * MAXC] = r <= cc ? U[r + cc * ldu] : T(0);
    }
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    T x[MAXC];
#pragma unroll
    for (int j = 0; j < MAXC; ++j) x[j] = j < cols ? F[i + j * ldf] : T(0);
    T v = d[i];
#pragma unroll
    for (int j = 0; j < MAXC; ++j) {
        if (j < cols) {
            T s = x[j];
#pragma unroll
            for (int l = 0; l < j; ++l) s -= x[l] * Us[l + j * MAXC];
            s = s / Us[j + j * MAXC];
            x[j] = s;
            F[i + j * ldf] = s;
            v -= s * s;
        }
    }
    d[i] = in_sorted(sidx, cols, i) ? T(0) : v;
}

// panel finish for cols > 64 (U does not fit the fused kernel's registers): after rlhip_trsm, d[i] -= sum_j F(i, j)^2 and d[S'] = 0
template <typename T>
__global__ void rpchol_downdate_kernel(int64_t n, int64_t cols, const T* __restrict__ F, int64_t ldf, T* __restrict__ d,
                                       const int64_t* __restrict__ sidx, int64_t scnt) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    T v = d[i];
    for (int64_t j = 0; j < cols; ++j) { const T f = F[i + j * ldf]; v -= f * f; }
    int64_t lo = 0, hi = scnt;                // S' is sorted
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (sidx[mid] < i) lo = mid + 1; else hi = mid; }
    if (lo < scnt && sidx[lo] == i) v = T(0);
    d[i] = v;
}

template <typename T>
__global__ void gather_rows_kernel(int64_t cnt, const int64_t* __restrict__ idx, int64_t ncols, const T* __restrict__ A, int64_t lda,
                                   T* __restrict__ out, int64_t ldo) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= cnt * ncols) return;
    const int64_t r = t % cnt, c = t / cnt;
    out[r + c * ldo] = A[idx[r] + c * lda];
}

template <typename T>
__global__ void gather_cols_kernel(int64_t m, const int64_t* __restrict__ idx, const T* __restrict__ A, int64_t lda, T* __restrict__ out,
                                   int64_t ldo) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t c = blockIdx.y;
    if (r >= m) return;
    out[r + c * ldo] = A[r + idx[c] * lda];
}

// The three routines below serve the rlhip_sqexp_* / rlhip_rbf_apply_* entries (kernel = RLHIP_PDK_SQEXP, sh = 0) and the rlhip_pdk_* entries,
// whose argument lists have `kernel` in front of the bandwidth: sh = 1 moves the codes of the arguments from there on by one.
template <typename T>
int pdk_columns(rlhip_ctx* c, int64_t rows_x, int64_t n, const T* X, int64_t ldx, int64_t nidx, const int64_t* idx, int kernel, int sh, T bandwidth,
                T reg, T* out, int64_t ldo) {
    if (rows_x < 1) return -2;
    if (n < 0) return -3;
    if (ldx < rows_x) return -5;
    if (nidx < 0) return -6;
    if (!rlhip::pdk_kind_ok(kernel)) return -8;
    if (!(bandwidth > T(0))) return -(8 + sh);
    if (ldo < (n > 1 ? n : 1)) return -(11 + sh);
    if (n == 0 || nidx == 0) return 0;
    const int64_t ltiles = (nidx + COL_TILE_L - 1) / COL_TILE_L;
    if (ltiles > 65535) return -6;
    const dim3 grid(grid1(n, 256), (unsigned)ltiles);
    if (kernel == RLHIP_PDK_SQEXP) {
        const T inv2h2 = (T)(1.0 / (2.0 * (double)bandwidth * (double)bandwidth));
        hipLaunchKernelGGL((sqexp_columns_kernel<T, false>), grid, dim3(256), 0, c->stream, rows_x, n, X, ldx, nidx, idx, inv2h2, T(0), reg, out, ldo);
    } else {
        const PdkFn<T> f = rlhip::pdk_fn<T>(kernel, bandwidth);
        hipLaunchKernelGGL((sqexp_columns_kernel<T, true>), grid, dim3(256), 0, c->stream, rows_x, n, X, ldx, nidx, idx, f.scale, f.third, reg, out,
                           ldo);
    }
    RLHIP_LAUNCH_CHECK();
    return 0;
}

template <typename T>
int launch_epilogue(rlhip_ctx* c, int64_t rows, int64_t cols, const T* nr_rows, const T* nr_cols, PdkFn<T> f, T* K, int64_t ldk) {
    const dim3 grid(grid1(rows, 256), (unsigned)cols);
    if (f.weight)
        hipLaunchKernelGGL((sqexp_epilogue_kernel<T, true, true>), grid, dim3(256), 0, c->stream, rows, cols, nr_rows, nr_cols, f.scale, f.third, K, ldk);
    else if (f.matern)
        hipLaunchKernelGGL((sqexp_epilogue_kernel<T, true>), grid, dim3(256), 0, c->stream, rows, cols, nr_rows, nr_cols, f.scale, f.third, K, ldk);
    else
        hipLaunchKernelGGL((sqexp_epilogue_kernel<T, false>), grid, dim3(256), 0, c->stream, rows, cols, nr_rows, nr_cols, f.scale, f.third, K, ldk);
    RLHIP_LAUNCH_CHECK();
    return 0;
}

template <typename T>
int sq_colnorms(rlhip_ctx* c, int64_t rows_x, int64_t cols, const T* X, int64_t ldx, T* nr) {
    if (cols <= 0) return 0;
    hipLaunchKernelGGL(sq_colnorms_kernel<T>, dim3(grid1(cols, 256)), dim3(256), 0, c->stream, rows_x, cols, X, ldx, nr);
    RLHIP_LAUNCH_CHECK();
    return 0;
}

template <typename T>
int pdk_submatrix(rlhip_ctx* c, int64_t rows_x, int64_t cols_x, const T* X, int64_t ldx, const T* sq_colnorms_x, int64_t rows_k,
                  int64_t cols_k, T* K, int64_t ldk, int64_t ro, int64_t co, int kernel, int sh, T bandwidth) {
    if (rows_x < 1) return -2;
    if (cols_x < 0) return -3;
    if (ldx < rows_x) return -5;
    if (rows_k < 0 || ro < 0 || ro + rows_k > cols_x) return -7;
    if (cols_k < 0 || co < 0 || co + cols_k > cols_x) return -8;
    if (ldk < (rows_k > 1 ? rows_k : 1)) return -10;
    if (!rlhip::pdk_kind_ok(kernel)) return -13;
    if (!(bandwidth > T(0))) return -(13 + sh);
    if (rows_k == 0 || cols_k == 0) return 0;
    if (cols_k > 65535) return -8;
    ws_scope ws(c);
    const T* nr = sq_colnorms_x;
    if (!nr) {
        T* tmp = ws.alloc<T>((size_t)cols_x);
        if (!tmp) return RLHIP_ERR_HIP(hipErrorOutOfMemory);
        int rc = sq_colnorms(c, rows_x, cols_x, X, ldx, tmp);
        if (rc) return rc;
        nr = tmp;
    }
    int rc = rlhip::gemm<T>(c, rlhip::Trans, rlhip::NoTrans, rows_k, cols_k, rows_x, T(-2), X + ro * ldx, ldx, X + co * ldx, ldx, T(0), K, ldk);
    if (rc == 0) rc = launch_epilogue<T>(c, rows_k, cols_k, nr + ro, nr + co, rlhip::pdk_fn<T>(kernel, bandwidth), K, ldk);
    return rc;
}

template <typename T>
int axpby_dev(rlhip_ctx* c, int64_t n, T a, const T* x, T b, T* y);
template <>
int axpby_dev<double>(rlhip_ctx* c, int64_t n, double a, const double* x, double b, double* y) { return rlhip_axpby_f64(c, n, a, x, b, y); }
template <>
int axpby_dev<float>(rlhip_ctx* c, int64_t n, float a, const float* x, float b, float* y) { return rlhip_axpby_f32(c, n, a, x, b, y); }

// C (dim x n) = alpha * (K [+ regs]) * B + beta * C, K evaluated in full row blocks of at most max(2^26, dim) entries of scratch
template <typename T>
int pdk_apply(rlhip_ctx* c, int64_t rows_x, int64_t dim, const T* X, int64_t ldx, int kernel, int sh, T bandwidth, const T* regs_host,
              int64_t num_ops, int eval_includes_reg, int64_t n, T alpha, const T* B, int64_t ldb, T beta, T* C, int64_t ldc) {
    if (rows_x < 1) return -2;
    if (dim < 0) return -3;
    if (ldx < rows_x) return -5;
    if (!rlhip::pdk_kind_ok(kernel)) return -6;
    if (!(bandwidth > T(0))) return -(6 + sh);
    if (eval_includes_reg && (!regs_host || num_ops < 1)) return -(7 + sh);
    if (eval_includes_reg && num_ops != 1 && n != num_ops) return -(10 + sh);
    if (n < 0) return -(10 + sh);
    if (ldb < (dim > 1 ? dim : 1)) return -(13 + sh);
    if (ldc < (dim > 1 ? dim : 1)) return -(16 + sh);
    if (dim == 0 || n == 0) return 0;
    ws_scope ws(c);
    int rc = 0;
    T* nr = ws.alloc<T>((size_t)dim);
    const int64_t rb = rlhip::pdk_row_block(dim, dim);     // rows of a block of K
    T* Kb = ws.alloc<T>((size_t)(rb * dim));
    if (!nr || !Kb) return RLHIP_ERR_HIP(hipErrorOutOfMemory);
    rc = sq_colnorms(c, rows_x, dim, X, ldx, nr);
    for (int64_t r0 = 0; rc == 0 && r0 < dim; r0 += rb) {
        const int64_t rows = (dim - r0) < rb ? (dim - r0) : rb;
        // K(r0 : r0+rows, :) -- the transpose of the column block, which is what the MFMA GEMM's row operand wants
        for (int64_t c0 = 0; rc == 0 && c0 < dim; c0 += 65535) {
            const int64_t cc = (dim - c0) < 65535 ? (dim - c0) : 65535;
            rc = pdk_submatrix<T>(c, rows_x, dim, X, ldx, nr, rows, cc, Kb + c0 * rows, rows, r0, c0, kernel, 0, bandwidth);
        }
        if (rc == 0) rc = rlhip::gemm<T>(c, rlhip::NoTrans, rlhip::NoTrans, rows, n, dim, alpha, Kb, rows, B, ldb, beta, C + r0, ldc);
    }
    if (rc == 0 && eval_includes_reg) {
        for (int64_t i = 0; rc == 0 && i < n; ++i) {
            const T coeff = alpha * regs_host[i < num_ops - 1 ? i : num_ops - 1];
            rc = axpby_dev<T>(c, dim, coeff, B + i * ldb, T(1), C + i * ldc);
        }
    }
    return rc;
}

template <typename T>
int sample_indices_iid(rlhip_ctx* c, int64_t n, const T* d, int64_t k, int unique, const uint32_t ctr[4], const uint32_t key[2],
                       uint32_t next_ctr[4], int64_t* out_dev, int64_t* out_host, int64_t* count, int* status) {
    if (n < 1) return -2;
    if (!d) return -3;
    if (k < 0) return -4;
    if (unique && k > SORT_MAX) return -4;
    if (unique != 0 && unique != 1) return -5;
    if (!ctr) return -6;
    if (!key) return -7;
    if (!count) return -11;
    if (!status) return -12;
    const int64_t nchunks = (n + SAMPLE_CHUNK - 1) / SAMPLE_CHUNK;
    ws_scope ws(c);
    double* S = ws.alloc<double>((size_t)nchunks);
    double* off = ws.alloc<double>((size_t)nchunks + 1);
    int64_t* lp = ws.alloc<int64_t>((size_t)nchunks);
    int* bad = ws.alloc<int>((size_t)nchunks);
    SampleHdr* hdr = ws.alloc<SampleHdr>(1);
    int64_t* out = out_dev ? out_dev : ws.alloc<int64_t>((size_t)(k > 0 ? k : 1));
    if (!S || !off || !lp || !bad || !hdr || !out) return RLHIP_ERR_HIP(hipErrorOutOfMemory);
    const double eps = sizeof(T) == 8 ? (double)DBL_EPSILON : (double)FLT_EPSILON;
    hipLaunchKernelGGL(sample_partial_kernel<T>, dim3(grid1(nchunks, 256)), dim3(256), 0, c->stream, n, d, S, lp, bad, nchunks, -eps);
    hipLaunchKernelGGL(sample_scan_kernel, dim3(1), dim3(1024), 0, c->stream, n, nchunks, S, lp, bad, off, std::sqrt((double)n) * eps, hdr);
    RngState st;
    for (int i = 0; i < 4; ++i) st.ctr[i] = ctr[i];
    st.key[0] = key[0]; st.key[1] = key[1];
    if (k > 0) {
        if (unique) {
            hipLaunchKernelGGL(sample_draw_unique_kernel<T>, dim3(1), dim3(1024), 0, c->stream, n, d, off, nchunks, hdr, st, k, out);
        } else {
            const int64_t g = (k + 255) / 256;
            hipLaunchKernelGGL(sample_draw_kernel<T>, dim3((unsigned)(g < 1024 ? g : 1024)), dim3(256), 0, c->stream, n, d, off, nchunks, hdr,
                               st, k, out);
        }
    }
    hipError_t e = hipGetLastError();
    // the one host read: status (and the unique count) ride in the pinned mailbox, the indices go straight to the caller's buffer
    if (e == hipSuccess) e = hipMemcpyAsync(c->h_mail + MAIL_SAMPLE_HDR, hdr, sizeof(SampleHdr), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess && out_host && k > 0) e = hipMemcpyAsync(out_host, out, (size_t)k * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = rlhip_stream_sync(c);
    if (e != hipSuccess) return RLHIP_ERR_HIP(e);
    SampleHdr h;
    memcpy(&h, c->h_mail + MAIL_SAMPLE_HDR, sizeof(SampleHdr));
    *status = (int)h.status;
    *count = h.status != 0 ? 0 : (unique ? h.count : k);
    if (next_ctr) ctr_add(ctr, h.status != 0 ? 0 : (uint64_t)((k + 1) / 2), next_ctr);
    return 0;
}

template <typename T>
int trsm_dev(rlhip_ctx* c, int64_t m, int64_t n, const T* U, int64_t ldu, T* B, int64_t ldb);
template <>
int trsm_dev<double>(rlhip_ctx* c, int64_t m, int64_t n, const double* U, int64_t ldu, double* B, int64_t ldb) {
    return rlhip_trsm_f64(c, 'R', 'U', 'N', 'N', m, n, 1.0, U, ldu, B, ldb);
}
template <>
int trsm_dev<float>(rlhip_ctx* c, int64_t m, int64_t n, const float* U, int64_t ldu, float* B, int64_t ldb) {
    return rlhip_trsm_f32(c, 'R', 'U', 'N', 'N', m, n, 1.0f, U, ldu, B, ldb);
}

template <typename T>
int rpchol_panel_finish(rlhip_ctx* c, int64_t n, int64_t cols, const T* U, int64_t ldu, T* F, int64_t ldf, T* d, const int64_t* sidx) {
    if (n < 0) return -2;
    if (cols < 0) return -3;
    if (cols > 0 && ldu < cols) return -5;
    if (ldf < (n > 1 ? n : 1)) return -7;
    if (n == 0) return 0;
    if (cols <= 64) {
        const dim3 g(grid1(n, 256)), blk(256);
        if (cols <= 16) hipLaunchKernelGGL((rpchol_panel_fused_kernel<T, 16>), g, blk, 0, c->stream, n, (int)cols, U, ldu, F, ldf, d, sidx);
        else if (cols <= 32) hipLaunchKernelGGL((rpchol_panel_fused_kernel<T, 32>), g, blk, 0, c->stream, n, (int)cols, U, ldu, F, ldf, d, sidx);
        else hipLaunchKernelGGL((rpchol_panel_fused_kernel<T, 64>), g, blk, 0, c->stream, n, (int)cols, U, ldu, F, ldf, d, sidx);
        RLHIP_LAUNCH_CHECK();
        return 0;
    }
    {
        const int rc = trsm_dev<T>(c, n, cols, U, ldu, F, ldf);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(rpchol_downdate_kernel<T>, dim3(grid1(n, 256)), dim3(256), 0, c->stream, n, cols, F, ldf, d, sidx, cols);
    RLHIP_LAUNCH_CHECK();
    return 0;
}

template <typename T>
int gather_rows(rlhip_ctx* c, int64_t cnt, const int64_t* idx, int64_t ncols, const T* A, int64_t lda, T* out, int64_t ldo) {
    if (cnt < 0) return -2;
    if (ncols < 0) return -4;
    if (ldo < (cnt > 1 ? cnt : 1)) return -8;
    if (cnt == 0 || ncols == 0) return 0;
    hipLaunchKernelGGL(gather_rows_kernel<T>, dim3(grid1(cnt * ncols, 256)), dim3(256), 0, c->stream, cnt, idx, ncols, A, lda, out, ldo);
    RLHIP_LAUNCH_CHECK();
    return 0;
}

template <typename T>
int gather_cols(rlhip_ctx* c, int64_t m, int64_t cnt, const int64_t* idx, const T* A, int64_t lda, T* out, int64_t ldo) {
    if (m < 0) return -2;
    if (cnt < 0 || cnt > 65535) return -3;
    if (lda < (m > 1 ? m : 1)) return -6;
    if (ldo < (m > 1 ? m : 1)) return -8;
    if (m == 0 || cnt == 0) return 0;
    hipLaunchKernelGGL(gather_cols_kernel<T>, dim3(grid1(m, 256), (unsigned)cnt), dim3(256), 0, c->stream, m, idx, A, lda, out, ldo);
    RLHIP_LAUNCH_CHECK();
    return 0;
}

}  // namespace

// the two pieces of pdk_submatrix that the two-point-set kernels of rbf.hip are composed from as well
namespace rlhip {
template <typename T>
int sqexp_colnorms(rlhip_ctx* c, int64_t rows_x, int64_t cols, const T* X, int64_t ldx, T* nr) { return sq_colnorms<T>(c, rows_x, cols, X, ldx, nr); }
template <typename T>
int pdk_epilogue(rlhip_ctx* c, int64_t rows, int64_t cols, const T* nr_rows, const T* nr_cols, PdkFn<T> f, T* K, int64_t ldk) {
    if (rows <= 0 || cols <= 0) return 0;
    if (cols > 65535) return -3;
    return launch_epilogue<T>(c, rows, cols, nr_rows, nr_cols, f, K, ldk);
}
template int sqexp_colnorms<double>(rlhip_ctx*, int64_t, int64_t, const double*, int64_t, double*);
template int sqexp_colnorms<float>(rlhip_ctx*, int64_t, int64_t, const float*, int64_t, float*);
template int pdk_epilogue<double>(rlhip_ctx*, int64_t, int64_t, const double*, const double*, PdkFn<double>, double*, int64_t);
template int pdk_epilogue<float>(rlhip_ctx*, int64_t, int64_t, const float*, const float*, PdkFn<float>, float*, int64_t);
}  // namespace rlhip

extern "C" {

int rlhip_sqexp_columns_f64(rlhip_ctx* c, int64_t rows_x, int64_t n, const double* X, int64_t ldx, int64_t nidx, const int64_t* idx_dev,
                            double bandwidth, double reg, double* out, int64_t ldo) {
    return pdk_columns<double>(c, rows_x, n, X, ldx, nidx, idx_dev, RLHIP_PDK_SQEXP, 0, bandwidth, reg, out, ldo);
}
int rlhip_sqexp_columns_f32(rlhip_ctx* c, int64_t rows_x, int64_t n, const float* X, int64_t ldx, int64_t nidx, const int64_t* idx_dev,
                            float bandwidth, float reg, float* out, int64_t ldo) {
    return pdk_columns<float>(c, rows_x, n, X, ldx, nidx, idx_dev, RLHIP_PDK_SQEXP, 0, bandwidth, reg, out, ldo);
}
int rlhip_sqexp_submatrix_f64(rlhip_ctx* c, int64_t rows_x, int64_t cols_x, const double* X, int64_t ldx, const double* sq_colnorms_x,
                              int64_t rows_ksub, int64_t cols_ksub, double* Ksub, int64_t ldk, int64_t ro_ksub, int64_t co_ksub, double bandwidth) {
    return pdk_submatrix<double>(c, rows_x, cols_x, X, ldx, sq_colnorms_x, rows_ksub, cols_ksub, Ksub, ldk, ro_ksub, co_ksub, RLHIP_PDK_SQEXP, 0, bandwidth);
}
int rlhip_sqexp_submatrix_f32(rlhip_ctx* c, int64_t rows_x, int64_t cols_x, const float* X, int64_t ldx, const float* sq_colnorms_x,
                              int64_t rows_ksub, int64_t cols_ksub, float* Ksub, int64_t ldk, int64_t ro_ksub, int64_t co_ksub, float bandwidth) {
    return pdk_submatrix<float>(c, rows_x, cols_x, X, ldx, sq_colnorms_x, rows_ksub, cols_ksub, Ksub, ldk, ro_ksub, co_ksub, RLHIP_PDK_SQEXP, 0, bandwidth);
}
int rlhip_sq_colnorms_f64(rlhip_ctx* c, int64_t rows_x, int64_t cols_x, const double* X, int64_t ldx, double* nr) {
    return rows_x < 1 ? -2 : ldx < rows_x ? -5 : sq_colnorms<double>(c, rows_x, cols_x, X, ldx, nr);
}
int rlhip_sq_colnorms_f32(rlhip_ctx* c, int64_t rows_x, int64_t cols_x, const float* X, int64_t ldx, float* nr) {
    return rows_x < 1 ? -2 : ldx < rows_x ? -5 : sq_colnorms<float>(c, rows_x, cols_x, X, ldx, nr);
}
int rlhip_rbf_apply_f64(rlhip_ctx* c, int64_t rows_x, int64_t dim, const double* X, int64_t ldx, double bandwidth, const double* regs_host,
                        int64_t num_ops, int eval_includes_reg, int64_t n, double alpha, const double* B, int64_t ldb, double beta, double* C,
                        int64_t ldc) {
    return pdk_apply<double>(c, rows_x, dim, X, ldx, RLHIP_PDK_SQEXP, 0, bandwidth, regs_host, num_ops, eval_includes_reg, n, alpha, B, ldb, beta, C, ldc);
}
int rlhip_rbf_apply_f32(rlhip_ctx* c, int64_t rows_x, int64_t dim, const float* X, int64_t ldx, float bandwidth, const float* regs_host,
                        int64_t num_ops, int eval_includes_reg, int64_t n, float alpha, const float* B, int64_t ldb, float beta, float* C,
                        int64_t ldc) {
    return pdk_apply<float>(c, rows_x, dim, X, ldx, RLHIP_PDK_SQEXP, 0, bandwidth, regs_host, num_ops, eval_includes_reg, n, alpha, B, ldb, beta, C, ldc);
}
// the same three routines with the kernel function as an argument
#define RLHIP_DEFINE_PDK_SQUARE(SUF, T)                                                                                                           \
    int rlhip_pdk_columns_##SUF(rlhip_ctx* c, int64_t rows_x, int64_t n, const T* X, int64_t ldx, int64_t nidx, const int64_t* idx_dev, int kernel, \
                                T bandwidth, T reg, T* out, int64_t ldo) {                                                                        \
        return pdk_columns<T>(c, rows_x, n, X, ldx, nidx, idx_dev, kernel, 1, bandwidth, reg, out, ldo);                                          \
    }                                                                                                                                             \
    int rlhip_pdk_submatrix_##SUF(rlhip_ctx* c, int64_t rows_x, int64_t cols_x, const T* X, int64_t ldx, const T* sq_colnorms_x, int64_t rows_ksub, \
                                  int64_t cols_ksub, T* Ksub, int64_t ldk, int64_t ro_ksub, int64_t co_ksub, int kernel, T bandwidth) {           \
        return pdk_submatrix<T>(c, rows_x, cols_x, X, ldx, sq_colnorms_x, rows_ksub, cols_ksub, Ksub, ldk, ro_ksub, co_ksub, kernel, 1, bandwidth); \
    }                                                                                                                                             \
    int rlhip_pdk_apply_##SUF(rlhip_ctx* c, int64_t rows_x, int64_t dim, const T* X, int64_t ldx, int kernel, T bandwidth, const T* regs_host,    \
                              int64_t num_ops, int eval_includes_reg, int64_t n, T alpha, const T* B, int64_t ldb, T beta, T* C, int64_t ldc) {   \
        return pdk_apply<T>(c, rows_x, dim, X, ldx, kernel, 1, bandwidth, regs_host, num_ops, eval_includes_reg, n, alpha, B, ldb, beta, C, ldc); \
    }
RLHIP_DEFINE_PDK_SQUARE(f64, double)
RLHIP_DEFINE_PDK_SQUARE(f32, float)
int rlhip_sample_indices_iid_f64(rlhip_ctx* c, int64_t n, const double* d, int64_t k, int unique, const uint32_t ctr[4], const uint32_t key[2],
                                 uint32_t next_ctr[4], int64_t* out_dev, int64_t* out_host, int64_t* count, int* status) {
    return sample_indices_iid<double>(c, n, d, k, unique, ctr, key, next_ctr, out_dev, out_host, count, status);
}
int rlhip_sample_indices_iid_f32(rlhip_ctx* c, int64_t n, const float* d, int64_t k, int unique, const uint32_t ctr[4], const uint32_t key[2],
                                 uint32_t next_ctr[4], int64_t* out_dev, int64_t* out_host, int64_t* count, int* status) {
    return sample_indices_iid<float>(c, n, d, k, unique, ctr, key, next_ctr, out_dev, out_host, count, status);
}
int rlhip_rpchol_panel_finish_f64(rlhip_ctx* c, int64_t n, int64_t cols, const double* U, int64_t ldu, double* F, int64_t ldf, double* d,
                                  const int64_t* sidx_dev) {
    return rpchol_panel_finish<double>(c, n, cols, U, ldu, F, ldf, d, sidx_dev);
}
int rlhip_rpchol_panel_finish_f32(rlhip_ctx* c, int64_t n, int64_t cols, const float* U, int64_t ldu, float* F, int64_t ldf, float* d,
                                  const int64_t* sidx_dev) {
    return rpchol_panel_finish<float>(c, n, cols, U, ldu, F, ldf, d, sidx_dev);
}
int rlhip_gather_rows_f64(rlhip_ctx* c, int64_t cnt, const int64_t* idx_dev, int64_t ncols, const double* A, int64_t lda, double* out, int64_t ldo) {
    return gather_rows<double>(c, cnt, idx_dev, ncols, A, lda, out, ldo);
}
int rlhip_gather_rows_f32(rlhip_ctx* c, int64_t cnt, const int64_t* idx_dev, int64_t ncols, const float* A, int64_t lda, float* out, int64_t ldo) {
    return gather_rows<float>(c, cnt, idx_dev, ncols, A, lda, out, ldo);
}
int rlhip_gather_cols_f64(rlhip_ctx* c, int64_t m, int64_t cnt, const int64_t* idx_dev, const double* A, int64_t lda, double* out, int64_t ldo) {
    return gather_cols<double>(c, m, cnt, idx_dev, A, lda, out, ldo);
}
int rlhip_gather_cols_f32(rlhip_ctx* c, int64_t m, int64_t cnt, const int64_t* idx_dev, const float* A, int64_t lda, float* out, int64_t ldo) {
    return gather_cols<float>(c, m, cnt, idx_dev, A, lda, out, ldo);
}

}  // extern "C"
