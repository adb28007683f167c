// Sparse matrix-VECTOR products: the hot path of pcg_saddle on a linops::SparseLinOp (include/RandLAPACK_amd/rl_determiter.hh), where one
// iteration is one normal matvec q = A^T (A d) + delta d plus O(n k) small work.  The operator is a CSR together with the CSR of its
// transpose (sparse.hip), so both halves are a gather over the rows of one of the two structures: y = alpha A x + beta y.
//
//   rows route    W = 4, 16 or 64 lanes own a row, a wave takes 64 / W rows.  Lane s of a group walks the entries p0 + s, p0 + s + W, ...
//                 of its row in storage order (consecutive lanes read consecutive (column, value) pairs: every load of a group is one
//                 contiguous run), four entries in flight; the W sums are added in a fixed tree (shuffles of width W).  When x fits
//                 RLHIP_SPMV_X_LDS_BYTES it is staged in LDS once per workgroup and the workgroup walks several row groups.
//   split route   long rows, i.e. the transposed product of a tall operator: rows are cut into chunks of SPMV_CH entries (a compile-time
//                 constant: the sums do not depend on the device), one wave sums one chunk (lane l walks p0 + l, p0 + l + 64, ..., the 64
//                 sums added in a fixed tree), the chunk sums go to the scratch arena (at most nnz / SPMV_CH + nrows values) and a final
//                 pass adds the sums of a row: 16 lanes per row, lane s the chunks s, s + 16, ... in order, then a fixed tree.  The
//                 chunk -> row map is built on the device: one workgroup scans ceil(len / SPMV_CH) over the rows, a wave finds the row of
//                 its chunk by bisection.
//
// The rules are those of lsq.hip: no workgroup waits for another, no floating-point atomic, every result bitwise reproducible and
// independent of the grid, sums in the precision of the data, no host read (nnz is an argument), nothing written beyond an output's
// length, int64 indices.  Row pointers are clamped to [0, nnz]; column indices are trusted, as in sparse.hip.
#include "rlhip_internal.h"
#include "rlhip_device.h"

namespace {

using namespace rlhip_dev;

constexpr int SPMV_CH = RLHIP_SPMV_CHUNK;         // entries of a chunk of the split route: 8 per lane
// The default route, from the shape alone (DESIGN 4.21 holds the measurements behind the figures):
constexpr int64_t SPMV_SPLIT_MAX_ROWS = 512;      // the split route when there are at most this many rows (a wave per row cannot fill the device) ...
constexpr int64_t SPMV_SPLIT_MIN_MEAN = 2 * SPMV_CH;   // ... of at least this mean length (below it a row is one or two chunks anyway)
constexpr int64_t SPMV_W4_MAX_MEAN = 64;          // otherwise 4 lanes per row up to this mean row length,
constexpr int64_t SPMV_W16_MAX_MEAN = 1023;       // 16 up to this one, 64 beyond
static_assert(SPMV_CH % 64 == 0, "a chunk is a whole number of wave-wide steps");

__host__ __device__ inline int64_t clamp_ptr(int64_t p, int64_t nnz) { return p < 0 ? 0 : (p > nnz ? nnz : p); }

// sum over the entries p0 + s, p0 + s + STEP, ... < p1 of vals[p] * xv[colidx[p]], in that order
template <typename T, int STEP>
__device__ __forceinline__ T strided_row_sum(int64_t p0, int64_t p1, int s, const int64_t* __restrict__ colidx, const T* __restrict__ vals, const T* xv) {
    T acc = T(0);
    int64_t p = p0 + s;
    for (; p + 3 * STEP < p1; p += 4 * STEP) {
        const int64_t c0 = colidx[p], c1 = colidx[p + STEP], c2 = colidx[p + 2 * STEP], c3 = colidx[p + 3 * STEP];
        const T v0 = vals[p], v1 = vals[p + STEP], v2 = vals[p + 2 * STEP], v3 = vals[p + 3 * STEP];
        const T x0 = xv[c0], x1 = xv[c1], x2 = xv[c2], x3 = xv[c3];
        acc += v0 * x0;
        acc += v1 * x1;
        acc += v2 * x2;
        acc += v3 * x3;
    }
    for (; p < p1; p += STEP) acc += vals[p] * xv[colidx[p]];
    return acc;
}

// yout[i] = alpha * s + beta * yin[i]; beta == 0 does not read yin (yout may be yin)
template <typename T>
__device__ __forceinline__ void store_row(T alpha, T s, T beta, const T* yin, T* yout, int64_t i) {
    const T a = alpha * s;
    yout[i] = beta == T(0) ? a : a + beta * yin[i];
}

// ---- (a) the rows route.  Dynamic LDS: ncols values when STAGE.
template <typename T, int W, bool STAGE>
__global__ __launch_bounds__(256) void spmv_rows_kernel(int64_t nrows, int64_t ncols, int64_t nnz, const int64_t* __restrict__ rowptr,
                                                        const int64_t* __restrict__ colidx, const T* __restrict__ vals, T alpha,
                                                        const T* __restrict__ x, T beta, const T* yin, T* yout) {
    extern __shared__ __attribute__((aligned(16))) char spmv_smem[];
    const T* xv = x;
    if (STAGE) {
        T* xs = (T*)spmv_smem;
        for (int64_t j = threadIdx.x; j < ncols; j += 256) xs[j] = x[j];
        __syncthreads();
        xv = xs;
    }
    constexpr int RPW = 64 / W, RPB = 4 * RPW;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane % W, sr = lane / W;
    const int64_t ngroups = (nrows + RPB - 1) / RPB;
    for (int64_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
        const int64_t row = g * RPB + wave * RPW + sr;
        const bool valid = row < nrows;
        const int64_t p0 = valid ? clamp_ptr(rowptr[row], nnz) : 0, p1 = valid ? clamp_ptr(rowptr[row + 1], nnz) : 0;
        T acc = strided_row_sum<T, W>(p0, p1, sub, colidx, vals, xv);
#pragma unroll
        for (int off = W / 2; off > 0; off >>= 1) acc += __shfl_down(acc, off, W);
        if (valid && sub == 0) store_row(alpha, acc, beta, yin, yout, row);
    }
}

// ---- (b) the split route
// cstart[r] = chunks of the rows before r, cstart[nrows] = all chunks: ONE workgroup of 1024 threads; thread t owns the rows
// [t per, (t + 1) per), the 1024 sums are scanned in LDS.
__global__ __launch_bounds__(1024) void spmv_chunk_scan_kernel(int64_t nrows, int64_t nnz, const int64_t* __restrict__ rowptr, int64_t* __restrict__ cstart) {
    __shared__ int64_t part[1024];
    const int t = threadIdx.x;
    const int64_t per = (nrows + 1023) / 1024;
    const int64_t r0 = t * per < nrows ? t * per : nrows, r1 = r0 + per < nrows ? r0 + per : nrows;
    auto chunks_of = [&](int64_t r) {
        const int64_t len = clamp_ptr(rowptr[r + 1], nnz) - clamp_ptr(rowptr[r], nnz);
        return len > 0 ? (len + SPMV_CH - 1) / SPMV_CH : (int64_t)0;
    };
    int64_t mine = 0;
    for (int64_t r = r0; r < r1; ++r) mine += chunks_of(r);
    part[t] = mine;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int64_t a = t >= off ? part[t - off] : 0;
        __syncthreads();
        part[t] += a;
        __syncthreads();
    }
    int64_t run = part[t] - mine;
    for (int64_t r = r0; r < r1; ++r) {
        cstart[r] = run;
        run += chunks_of(r);
    }
    if (t == 1023) cstart[nrows] = part[1023];
}

// part[c] = the sum of chunk c; cap = the length of part
template <typename T>
__global__ __launch_bounds__(256) void spmv_chunk_kernel(int64_t nrows, int64_t nnz, int64_t cap, const int64_t* __restrict__ rowptr,
                                                         const int64_t* __restrict__ colidx, const T* __restrict__ vals, const T* __restrict__ x,
                                                         const int64_t* __restrict__ cstart, T* __restrict__ part) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t total = cstart[nrows];
    if (total > cap) total = cap;
    for (int64_t c = (int64_t)blockIdx.x * 4 + wave; c < total; c += (int64_t)gridDim.x * 4) {
        int64_t lo = 0, hi = nrows;                                               // the first index in (0, nrows] with cstart[index] > c
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (cstart[mid] > c) hi = mid;
            else lo = mid + 1;
        }
        const int64_t r = lo - 1;                                                 // cstart[0] = 0 <= c: lo >= 1
        const int64_t b0 = clamp_ptr(rowptr[r], nnz) + (c - cstart[r]) * SPMV_CH, e = clamp_ptr(rowptr[r + 1], nnz);
        const int64_t p0 = b0 < e ? b0 : e, p1 = b0 + SPMV_CH < e ? b0 + SPMV_CH : e;
        T acc = strided_row_sum<T, 64>(p0, p1, lane, colidx, vals, x);
        acc = wave_sum(acc);
        if (lane == 0) part[c] = acc;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void spmv_chunk_final_kernel(int64_t nrows, int64_t cap, const int64_t* __restrict__ cstart, const T* __restrict__ part,
                                                               T alpha, T beta, const T* yin, T* yout) {
    const int sub = threadIdx.x & 15;
    const int64_t row = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
    const bool valid = row < nrows;
    int64_t c0 = valid ? cstart[row] : 0, c1 = valid ? cstart[row + 1] : 0;
    if (c0 > cap) c0 = cap;
    if (c1 > cap) c1 = cap;
    T acc = T(0);
    for (int64_t c = c0 + sub; c < c1; c += 16) acc += part[c];
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) acc += __shfl_down(acc, off, 16);
    if (valid && sub == 0) store_row(alpha, acc, beta, yin, yout, row);
}

// yout = beta * yin (beta == 0: zeros, yin not read)
template <typename T>
__global__ __launch_bounds__(256) void spmv_scale_kernel(int64_t n, T beta, const T* yin, T* yout) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) yout[i] = beta == T(0) ? T(0) : beta * yin[i];
}

template <typename T, int W>
void launch_rows(rlhip_ctx* c, int64_t max_wg, int64_t nrows, int64_t ncols, int64_t nnz, const int64_t* rowptr, const int64_t* colidx, const T* vals,
                 T alpha, const T* x, T beta, const T* yin, T* yout) {
    constexpr int RPB = 4 * (64 / W);
    const int64_t ngroups = (nrows + RPB - 1) / RPB;
    const bool stage = (size_t)ncols * sizeof(T) <= (size_t)RLHIP_SPMV_X_LDS_BYTES;
    // a staging workgroup walks several row groups (four workgroups of 32 KiB share a CU's LDS); otherwise one group each
    int64_t grid = stage ? (int64_t)c->num_cu * 4 : (int64_t)1 << 30;
    if (max_wg > 0 && max_wg < grid) grid = max_wg;
    if (ngroups < grid) grid = ngroups;
    if (stage)
        hipLaunchKernelGGL((spmv_rows_kernel<T, W, true>), dim3((unsigned)grid), dim3(256), (size_t)ncols * sizeof(T), c->stream, nrows, ncols, nnz, rowptr,
                           colidx, vals, alpha, x, beta, yin, yout);
    else
        hipLaunchKernelGGL((spmv_rows_kernel<T, W, false>), dim3((unsigned)grid), dim3(256), 0, c->stream, nrows, ncols, nnz, rowptr, colidx, vals, alpha,
                           x, beta, yin, yout);
}

// yout = alpha A x + beta yin for an nrows x ncols CSR with nnz entries (nrows > 0); yout may be yin
template <typename T>
int spmv(rlhip_ctx* c, int64_t nrows, int64_t ncols, int64_t nnz, const int64_t* rowptr, const int64_t* colidx, const T* vals, T alpha, const T* x,
         T beta, const T* yin, T* yout, int64_t max_wg) {
    if (nnz == 0) {
        hipLaunchKernelGGL(spmv_scale_kernel<T>, dim3((unsigned)((nrows + 255) / 256)), dim3(256), 0, c->stream, nrows, beta, yin, yout);
        RLHIP_LAUNCH_CHECK();
        return 0;
    }
    const int64_t mean = nnz / nrows;
    int64_t lanes = c->opt[RLHIP_OPT_SPMV_LANES];
    if (lanes != 0 && lanes != 4 && lanes != 16 && lanes != 64)
        lanes = (nrows <= SPMV_SPLIT_MAX_ROWS && mean >= SPMV_SPLIT_MIN_MEAN) ? 0 : (mean <= SPMV_W4_MAX_MEAN ? 4 : (mean <= SPMV_W16_MAX_MEAN ? 16 : 64));
    if (lanes == 0) {
        const int64_t cap = nnz / SPMV_CH + nrows;
        ws_scope ws(c);
        int64_t* cstart = ws.alloc<int64_t>((size_t)nrows + 1);
        T* part = ws.alloc<T>((size_t)cap);
        if (!cstart || !part) return RLHIP_ERR_HIP(hipErrorOutOfMemory);
        int64_t grid = (cap + 3) / 4;
        const int64_t most = max_wg > 0 ? max_wg : (int64_t)c->num_cu * 32;
        if (grid > most) grid = most;
        hipLaunchKernelGGL(spmv_chunk_scan_kernel, dim3(1), dim3(1024), 0, c->stream, nrows, nnz, rowptr, cstart);
        hipLaunchKernelGGL(spmv_chunk_kernel<T>, dim3((unsigned)grid), dim3(256), 0, c->stream, nrows, nnz, cap, rowptr, colidx, vals, x,
                           (const int64_t*)cstart, part);
        hipLaunchKernelGGL(spmv_chunk_final_kernel<T>, dim3((unsigned)((nrows + 15) / 16)), dim3(256), 0, c->stream, nrows, cap, (const int64_t*)cstart,
                           (const T*)part, alpha, beta, yin, yout);
        RLHIP_LAUNCH_CHECK();
        c->spmv_path_count[3]++;
        return 0;
    }
    if (lanes == 4) launch_rows<T, 4>(c, max_wg, nrows, ncols, nnz, rowptr, colidx, vals, alpha, x, beta, yin, yout);
    else if (lanes == 16) launch_rows<T, 16>(c, max_wg, nrows, ncols, nnz, rowptr, colidx, vals, alpha, x, beta, yin, yout);
    else launch_rows<T, 64>(c, max_wg, nrows, ncols, nnz, rowptr, colidx, vals, alpha, x, beta, yin, yout);
    RLHIP_LAUNCH_CHECK();
    c->spmv_path_count[lanes == 4 ? 0 : (lanes == 16 ? 1 : 2)]++;
    return 0;
}

template <typename T>
int csr_spmv(rlhip_ctx* c, int64_t nrows, int64_t ncols, int64_t nnz, const int64_t* rowptr, const int64_t* colidx, const T* vals, T alpha, const T* x,
             T beta, T* y) {
    if (!c || nrows < 0 || ncols < 0 || nnz < 0) return -2;
    if (nrows > 0 && (!rowptr || !y)) return -2;
    if (nnz > 0 && (nrows == 0 || ncols == 0 || !colidx || !vals || !x)) return -2;
    if (nrows == 0) return 0;
    return spmv<T>(c, nrows, ncols, nnz, rowptr, colidx, vals, alpha, x, beta, y, y, 0);
}

template <typename T>
int csr_normal_matvec(rlhip_ctx* c, int64_t m, int64_t n, int64_t nnz, const int64_t* rowptr, const int64_t* colidx, const T* vals, const int64_t* rowptrT,
                      const int64_t* colidxT, const T* valsT, const T* d, T delta, T* q, T* t, T* dq_dev, int64_t max_wg) {
    if (!c || m < 0 || n < 0 || nnz < 0) return -2;
    if ((m > 0 && !rowptr) || (n > 0 && (!rowptrT || !d || !q))) return -2;
    if (nnz > 0 && (m == 0 || n == 0 || !colidx || !vals || !colidxT || !valsT)) return -2;
    if (n == 0) return 0;
    c->spmv_path_count[4]++;
    ws_scope ws(c);
    T* tt = t;
    if (!tt && m > 0) {
        tt = ws.alloc<T>((size_t)m);
        if (!tt) return RLHIP_ERR_HIP(hipErrorOutOfMemory);
    }
    int rc = m > 0 ? spmv<T>(c, m, n, nnz, rowptr, colidx, vals, T(1), d, T(0), tt, tt, max_wg) : 0;
    if (rc) return rc;
    rc = spmv<T>(c, n, m, nnz, rowptrT, colidxT, valsT, T(1), tt, delta, d, q, max_wg);        // + delta d in the pass that writes q
    if (rc) return rc;
    return dq_dev ? rlhip::dot_dev<T>(c, n, d, q, dq_dev) : 0;
}

}  // namespace

extern "C" {

int64_t rlhip_spmv_path_count(rlhip_ctx* c, int which) { return (c && which >= 50 && which <= 54) ? c->spmv_path_count[which - 50] : -1; }

#define RLHIP_DEFINE_SPMV(SUF, T)                                                                                                                  \
    int rlhip_csr_spmv_##SUF(rlhip_ctx* c, int64_t nrows, int64_t ncols, int64_t nnz, const int64_t* rowptr, const int64_t* colidx, const T* vals, \
                             T alpha, const T* x, T beta, T* y) {                                                                                  \
        return csr_spmv<T>(c, nrows, ncols, nnz, rowptr, colidx, vals, alpha, x, beta, y);                                                         \
    }                                                                                                                                              \
    int rlhip_csr_normal_matvec_##SUF(rlhip_ctx* c, int64_t m, int64_t n, int64_t nnz, const int64_t* rowptr, const int64_t* colidx, const T* vals, \
                                      const int64_t* rowptrT, const int64_t* colidxT, const T* valsT, const T* d, T delta, T* q, T* t, T* dq_dev,  \
                                      int64_t max_wg) {                                                                                            \
        return csr_normal_matvec<T>(c, m, n, nnz, rowptr, colidx, vals, rowptrT, colidxT, valsT, d, delta, q, t, dq_dev, max_wg);                  \
    }
RLHIP_DEFINE_SPMV(f64, double)
RLHIP_DEFINE_SPMV(f32, float)

}  // extern "C"
