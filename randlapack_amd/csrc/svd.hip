// Thin SVD of a tall factor, drop-in for lapack::gesdd(Job::SomeVec, m, n, A, lda, S, U, ldu, VT, ldvt) at
// RandLAPACK/drivers/rl_rsvd.hh:146 (m = n_cols(A) of the data matrix, n = target rank k there).
//
// Pipeline (all on device):
//   1. Cholesky-QR twice:  A = Q1 R1, Q1 = Q2 R2  ->  A = Q (R2 R1)      [MFMA syrk + potrf + trsm]
//   2. X = (R2 R1)^T  (n x n, lower triangular)                          [LDS-tiled transpose]
//   3. one-sided Jacobi on X:  X = Ux S Vx^T   (converges in ~11 sweeps on R^T; 30+ on R itself)
//   4. A = Q R = Q X^T = (Q Vx) S Ux^T   ->   U_out = Q Vx [MFMA gemm],  VT_out = Ux^T [transpose]
// If either Cholesky fails or diag(R1) spans more than 1e7 (CholQR2 no longer guaranteed orthonormal)
// the routine falls back to Jacobi on A itself (slower, unconditionally accurate).
#include "rlhip_internal.h"
#include <cstdlib>
#include <limits>

namespace {

// out[j + i*ldo] = in[i + j*ldi]; 64x64 tiles through LDS, both sides coalesced
template <typename T>
__global__ __launch_bounds__(256) void transpose_kernel(int64_t m, int64_t n, const T* __restrict__ in, int64_t ldi,
                                                        T* __restrict__ out, int64_t ldo, int upper_only) {
    __shared__ T tile[64][65];
    const int64_t i0 = (int64_t)blockIdx.x * 64, j0 = (int64_t)blockIdx.y * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int jj = ty; jj < 64; jj += 4) {
        int64_t i = i0 + tx, j = j0 + jj;
        T v = 0;
        if (i < m && j < n && (!upper_only || i <= j)) v = in[i + j * ldi];
        tile[jj][tx] = v;
    }
    __syncthreads();
    for (int ii = ty; ii < 64; ii += 4) {
        int64_t i = i0 + ii, j = j0 + tx;
        if (i < m && j < n && (!upper_only || i <= j)) out[j + i * ldo] = tile[tx][ii];
    }
}

// A[:, j] /= s[j]
template <typename T>
__global__ void scale_cols_inv_kernel(int64_t m, int64_t n, T* __restrict__ A, int64_t lda, const T* __restrict__ s) {
    int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= m * n) return;
    int64_t i = idx % m, j = idx / m;
    A[i + j * lda] /= s[j];
}

// max|d_i| / min|d_i| over the diagonal of an n x n matrix -> out[0] (one workgroup)
template <typename T>
__global__ __launch_bounds__(256) void diag_ratio_kernel(int n, const T* __restrict__ R, int64_t ldr,
                                                         double* __restrict__ out) {
    __shared__ double smax[256], smin[256];
    double mx = 0, mn = 1e300;
    for (int i = threadIdx.x; i < n; i += 256) {
        double v = fabs((double)R[i + (int64_t)i * ldr]);
        mx = v > mx ? v : mx;
        mn = v < mn ? v : mn;
    }
    smax[threadIdx.x] = mx; smin[threadIdx.x] = mn;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            smax[threadIdx.x] = smax[threadIdx.x] > smax[threadIdx.x + s] ? smax[threadIdx.x] : smax[threadIdx.x + s];
            smin[threadIdx.x] = smin[threadIdx.x] < smin[threadIdx.x + s] ? smin[threadIdx.x] : smin[threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = (smin[0] > 0) ? smax[0] / smin[0] : 1e300;
}

// out[0] = max over the upper triangle of |G - I| (one workgroup): how far the columns behind G = Q^T Q are from orthonormal
template <typename T>
__global__ __launch_bounds__(1024) void gram_identity_dev_kernel(int n, const T* __restrict__ G, int64_t ldg, double* __restrict__ out) {
    __shared__ double red[1024];
    double v = 0;
    for (int e = threadIdx.x; e < n * n; e += 1024) {
        const int i = e % n, j = e / n;
        if (i <= j) { const double dv = fabs((double)G[i + (int64_t)j * ldg] - (i == j ? 1.0 : 0.0)); v = (dv > v || dv != dv) ? dv : v; }
    }
    red[threadIdx.x] = v;
    __syncthreads();
    for (int st = 512; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) { const double o = red[threadIdx.x + st]; if (o > red[threadIdx.x] || o != o) red[threadIdx.x] = o; }
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = red[0];
}

// ---- kernels of the Gram route (gesdd_tall_gram below) ----
// Gf = the full symmetric matrix whose upper triangle is G (syrk's output)
template <typename T>
__global__ void symmetrize_kernel(int n, const T* __restrict__ G, int64_t ldg, T* __restrict__ Gf) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * n) return;
    const int i = idx % n, j = idx / n;
    Gf[idx] = (i <= j) ? G[i + (int64_t)j * ldg] : G[j + (int64_t)i * ldg];
}

// column norms of the swept matrix X (n x n, ld n) -> sig[j]
template <typename T>
__global__ __launch_bounds__(256) void gram_colnorm_kernel(int n, const T* __restrict__ X, T* __restrict__ sig) {
    __shared__ double red[4];
    const T* col = X + (int64_t)blockIdx.x * n;
    double acc = 0;
    for (int i = threadIdx.x; i < n; i += 256) acc += (double)col[i] * (double)col[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) sig[blockIdx.x] = (T)sqrt(red[0] + red[1] + red[2] + red[3]);
}

// column j of X = G J (norm sigma^2) goes to its place r in the descending order of the norms (stable): with u = x / ||x||,
// W[:, r] = u / sigma (so that A W = the left vectors), VT[r, :] = u^T, S[r] = sigma = sqrt(||x||).  One workgroup per column; the rank
// is counted in place (n <= 1024 values).
template <typename T>
__global__ __launch_bounds__(256) void gram_finalize_kernel(int n, const T* __restrict__ X, const T* __restrict__ sig, T* __restrict__ W, T* __restrict__ S,
                                                            T* __restrict__ VT, int64_t ldvt) {
    __shared__ int cnt[4];
    const int j = blockIdx.x;
    const T sj = sig[j];
    int mine = 0;
    for (int i = threadIdx.x; i < n; i += 256) { const T si = sig[i]; mine += (si > sj) || (si == sj && i < j); }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_down(mine, off, 64);
    if ((threadIdx.x & 63) == 0) cnt[threadIdx.x >> 6] = mine;
    __syncthreads();
    const int r = cnt[0] + cnt[1] + cnt[2] + cnt[3];
    const T inv = (sj > T(0)) ? T(1) / sj : T(0);
    const T sigma = sqrt(sj);
    const T isig = (sj > T(0)) ? T(1) / sigma : T(0);
    const T* col = X + (int64_t)j * n;
    for (int i = threadIdx.x; i < n; i += 256) {
        const T u = col[i] * inv;
        W[i + (int64_t)r * n] = u * isig;
        VT[r + (int64_t)i * ldvt] = u;
    }
    if (threadIdx.x == 0) S[r] = sigma;
}

// out[0] = max(out[0], max |M - I|) over the n x n matrix M (NaN counts as infinite); out[0] must start at 0.  Non-negative doubles order
// like their bit patterns, so the workgroups combine with an integer atomic max.
template <typename T>
__global__ __launch_bounds__(256) void identity_defect_kernel(int n, const T* __restrict__ M, double* __restrict__ out) {
    __shared__ double red[4];
    const int idx = blockIdx.x * 256 + threadIdx.x;
    double v = 0;
    if (idx < n * n) {
        const int i = idx % n, j = idx / n;
        v = fabs((double)M[idx] - (i == j ? 1.0 : 0.0));
        if (v != v) v = 1e300;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const double o = __shfl_down(v, off, 64); v = (o > v) ? o : v; }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double w = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
        atomicMax(reinterpret_cast<unsigned long long*>(out), (unsigned long long)__double_as_longlong(w));
    }
}

}  // namespace

namespace rlhip {

template <typename T>
int transpose(rlhip_ctx* c, int64_t m, int64_t n, const T* A, int64_t lda, T* AT, int64_t ldat, int upper_only) {
    if (m <= 0 || n <= 0) return 0;
    dim3 grid((unsigned)((m + 63) / 64), (unsigned)((n + 63) / 64));
    hipLaunchKernelGGL(transpose_kernel<T>, grid, dim3(256), 0, c->stream, m, n, A, lda, AT, ldat, upper_only);
    RLHIP_LAUNCH_CHECK();
    return 0;
}

// The Gram route: the thin SVD of a WELL-CONDITIONED tall factor (the B^T of an RSVD of a matrix without a gap: cond ~ 1..30) as one
// stream of kernels with ONE host read at the end.  With G = A^T A = Ux S^2 Ux^T, the one-sided Jacobi sweeps of G itself (G J = Ux S^2:
// the columns of G J are orthogonal, their norms are sigma^2) give
//     A = (A Ux S^-1) S Ux^T,     i.e.  U = A W with W = Ux S^-1 (one tall GEMM),  VT = Ux^T
// -- no Cholesky factorization, no triangular solve, no explicit Q, no accumulated rotations, A is only READ.  Forming G costs
// eps * cond(A)^2 in the small singular values and in the orthogonality of U, exactly what one pass of Cholesky-QR costs; it is MEASURED
// at the end on k x k matrices: U^T U = W^T G W must equal I to 1e-13 (the orthogonality the two-pass route verifies on its Q) -- the
// same number also certifies that the sweeps converged.  The sweeps watch the range of the column norms (-> cond(A)^2) and stop as soon
// as it exceeds 1e3 (eps cond^2 = 1e-13): such an input cannot pass.  Returns 0 when U, S, VT are final, 1 when the caller must take the classic route
// (A untouched), < 0 on error.
template <typename T>
int gesdd_tall_gram(rlhip_ctx* c, int64_t m, int64_t n, const T* A, int64_t lda, T* S, T* U, int64_t ldu, T* VT, int64_t ldvt, int* sweeps_host) {
    if constexpr (sizeof(T) != 8) { return 1; }
    else {
        if (c->opt[RLHIP_OPT_GESDD_GRAM] == 0 || n <= 32 || n > 256 || m < n) return 1;
        const int nn = (int)n;
        ws_scope ws(c);
        T* G = ws.alloc<T>((size_t)n * n);
        T* Gf = ws.alloc<T>((size_t)n * n);
        T* W = ws.alloc<T>((size_t)n * n);
        T* M1 = ws.alloc<T>((size_t)n * n);
        T* sig = ws.alloc<T>((size_t)n);
        int64_t* mb = ws.alloc<int64_t>(8);       // [0..3] the Jacobi launch's 8 ints, [4] defect (double); the launch clears all of it
        if (!G || !Gf || !W || !M1 || !sig || !mb) return 1;
        int* jout = (int*)mb;
        double* defect = (double*)(mb + 4);
        const unsigned g2 = (unsigned)((n * n + 255) / 256);
        int rc = laset<T>(c, 2, n, n, T(0), T(0), G, n);
        if (!rc) rc = syrk<T>(c, Upper, 1, n, m, T(1), A, lda, T(0), G, n);
        if (rc) return rc < 0 ? rc : 1;
        hipLaunchKernelGGL(symmetrize_kernel<T>, dim3(g2), dim3(256), 0, c->stream, nn, G, n, Gf);
        const T* X = nullptr;
        rc = jacobi_enqueue_rt<T>(c, nn, Gf, n, 0, 1e6f, nullptr, jout, &X);     // squared norms of G J's columns = sigma^4: 1e6 <-> cond(A)^2 = 1e3
        if (rc) return rc < 0 ? rc : 1;
        hipLaunchKernelGGL(gram_colnorm_kernel<T>, dim3((unsigned)n), dim3(256), 0, c->stream, nn, X, sig);
        hipLaunchKernelGGL(gram_finalize_kernel<T>, dim3((unsigned)n), dim3(256), 0, c->stream, nn, X, sig, W, S, VT, ldvt);
        RLHIP_LAUNCH_CHECK();
        rc = gemm<T>(c, 0, 0, m, n, n, T(1), A, lda, W, n, T(0), U, ldu);                 // U = A W
        if (!rc) rc = gemm<T>(c, 0, 0, n, n, n, T(1), Gf, n, W, n, T(0), M1, n);          // U^T U = W^T (G W)
        if (!rc) rc = gemm<T>(c, 1, 0, n, n, n, T(1), W, n, M1, n, T(0), G, n);
        if (rc) return rc < 0 ? rc : 1;
        hipLaunchKernelGGL(identity_defect_kernel<T>, dim3(g2), dim3(256), 0, c->stream, nn, G, defect);            // (defect starts at 0: the Jacobi launch cleared the mailbox)
        RLHIP_LAUNCH_CHECK();
        hipError_t e = hipMemcpyAsync(c->h_mail + MAIL_SVD_GRAM, mb, MAIL_SVD_GRAM_WORDS * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = rlhip_stream_sync(c);
        if (e != hipSuccess) return RLHIP_ERR_HIP(e);
        const int* jo = (const int*)(c->h_mail + MAIL_SVD_GRAM);
        const double dv = *(const double*)(c->h_mail + MAIL_SVD_GRAM_DEFECT);
        const bool ok = (jo[0] == 1 || jo[0] == 2) && jo[2] == 0 && dv <= 1e-13;
        if (getenv("RLHIP_GESDD_TRACE")) fprintf(stderr, "[gesdd gram] jacobi status %d sweeps %d lost %d defect %.3e -> %s\n", jo[0], jo[1], jo[2], dv, ok ? "taken" : "classic route");
        if (jo[3] == 1) c->path_count[15]++;       // same-XCD hand-over taken by the Jacobi launch (jacobi.hip)
        if (!ok) return 1;
        if (sweeps_host) *sweeps_host = jo[1];
        c->path_count[10]++;
        return 0;
    }
}

// the routes behind gesdd_tall's argument checks and exponent-range guard.  Path counters (include/rlhip.h), one per call on the branch
// taken: 10 Gram route; 16 Cholesky-QR twice; 17 one pass; 18 V recovered instead of accumulated (beside 16 or 17); 19 Jacobi on A after
// the first factorization failed or its diagonal ratio reached the limit; 20 Jacobi on A after the second one failed and pass 1 was undone.
template <typename T>
static int gesdd_tall_core(rlhip_ctx* c, int64_t m, int64_t n, T* A, int64_t lda, T* S, T* U, int64_t ldu, T* VT, int64_t ldvt,
                           int* sweeps_host) {
    {
        const int grc = gesdd_tall_gram<T>(c, m, n, A, lda, S, U, ldu, VT, ldvt, sweeps_host);
        if (grc <= 0) return grc;
    }
    ws_scope ws(c);
    T* R1 = ws.alloc<T>((size_t)n * n);
    T* R2 = ws.alloc<T>((size_t)n * n);
    T* X = ws.alloc<T>((size_t)n * n);
    T* VTx = ws.alloc<T>((size_t)n * n);
    if (!R1 || !R2 || !X || !VTx) return RLHIP_ERR_HIP(hipErrorOutOfMemory);
    int rc = 0, info = 0;
    bool fallback = false;
    double ratio = 0;
    // ---- pass 1
    rc = laset<T>(c, 2, n, n, T(0), T(0), R1, n);
    if (!rc) rc = syrk<T>(c, Upper, 1, n, m, T(1), A, lda, T(0), R1, n);
    if (!rc) rc = potrf_upper<T>(c, n, R1, n, &info);
    if (rc) return rc;
    if (info) fallback = true;
    if (!fallback) {
        double* d_ratio = (double*)(c->d_mail + MAIL_SVD_RATIO);
        hipLaunchKernelGGL(diag_ratio_kernel<T>, dim3(1), dim3(256), 0, c->stream, (int)n, R1, (int64_t)n, d_ratio);
        RLHIP_CHECK(hipMemcpyAsync(c->h_mail + MAIL_SVD_RATIO, d_ratio, sizeof(double), hipMemcpyDeviceToHost, c->stream));
        RLHIP_CHECK(rlhip_stream_sync(c));
        ratio = *(double*)(c->h_mail + MAIL_SVD_RATIO);
        const double lim = (sizeof(T) == 8) ? 1e7 : 1e3;
        if (!(ratio < lim)) fallback = true;
    }
    if (fallback) c->path_count[19]++;
    bool one_pass = false;
    if (!fallback) {
        rc = trsm_right_upper<T>(c, NonUnit, m, n, T(1), R1, n, A, lda);
        // ---- pass 2
        if (!rc) rc = laset<T>(c, 2, n, n, T(0), T(0), R2, n);
        if (!rc) rc = syrk<T>(c, Upper, 1, n, m, T(1), A, lda, T(0), R2, n);
        if (rc) return rc;
        // The Gram matrix of the first pass's Q says how orthonormal it already is.  A well-conditioned input (cond ~ 2 for the
        // B^T of an RSVD of a Gaussian matrix) leaves max |Q^T Q - I| at a few eps: the second factorization would multiply by a
        // triangle that equals the identity to rounding, so it is skipped (one k x k Cholesky + one m x k triangular solve +
        // the R2 R1 product per call).  Threshold 1e-13 (fp64) keeps ||Q^T Q - I||_F below k * 1e-13.
        {
            double* d_dev = (double*)(c->d_mail + MAIL_SVD_GRAM_DEV);
            hipLaunchKernelGGL(gram_identity_dev_kernel<T>, dim3(1), dim3(1024), 0, c->stream, (int)n, R2, (int64_t)n, d_dev);
            RLHIP_CHECK(hipMemcpyAsync(c->h_mail + MAIL_SVD_GRAM_DEV, d_dev, sizeof(double), hipMemcpyDeviceToHost, c->stream));
            RLHIP_CHECK(rlhip_stream_sync(c));
            const double dev = *(double*)(c->h_mail + MAIL_SVD_GRAM_DEV);
            one_pass = (dev <= ((sizeof(T) == 8) ? 1e-13 : 5e-6));
        }
        if (one_pass) {
            rc = lacpy<T>(c, 0, n, n, R1, n, R2, n);        // R = R1 (upper triangle; the strictly lower part of R2 is reset below)
            if (rc) return rc;
            info = 0;
        } else {
            rc = potrf_upper<T>(c, n, R2, n, &info);
            if (rc) return rc;
        }
        if (info) {
            // undo pass 1 on A (A = Q1 R1) and take the robust route
            rc = trmm_right_upper<T>(c, NonUnit, m, n, T(1), R1, n, A, lda);
            if (rc) return rc;
            fallback = true;
            c->path_count[20]++;
        }
    }
    if (fallback) {
        // Jacobi on A directly: A -> U_A, then copy out
        int sw = 0;
        int jinfo = gesvdj_core<T>(c, m, n, A, lda, S, VT, ldvt, &sw);
        if (sweeps_host) *sweeps_host = sw;
        if (jinfo < 0) return jinfo;
        rc = lacpy<T>(c, 2, m, n, A, lda, U, ldu);
        return rc ? rc : jinfo;
    }
    if (!one_pass) rc = trsm_right_upper<T>(c, NonUnit, m, n, T(1), R2, n, A, lda);   // A now holds Q (orthonormal)
    // R = R2 * R1 (upper triangles only): zero the strictly lower parts first, then R2 <- R2 * R1
    if (!rc) rc = laset<T>(c, 1, n - 1, n, T(0), T(0), R2 + 1, n);      // 'L' incl. diag of the (n-1) x n block below row 0
    if (!rc && !one_pass) rc = trmm_right_upper<T>(c, NonUnit, n, n, T(1), R1, n, R2, n);
    if (!rc) rc = laset<T>(c, 2, n, n, T(0), T(0), X, n);
    if (!rc) rc = transpose<T>(c, n, n, R2, n, X, n, 1);               // X = R^T (lower triangular)
    if (rc) return rc;
    int sw = 0;
    // Well-conditioned R (diag ratio < 1e3): the rotations need not be accumulated -- R Ux = Vx S gives Vx = (R Ux) S^-1 to
    // eps * cond(R); that removes the V-panel update (a quarter of every Jacobi launch).  Otherwise accumulate as usual.
    // The diagonal ratio is only a LOWER bound on cond(R); the decision uses a rigorous upper bound instead:
    // cond_2(R) <= ||R||_F ||R^-1||_F, with R^-1 from one k x k substitution (I R^-1).
    bool recover_v = false;
    if (ratio < 1e3) {
        T nr = 0, ni = 0;
        rc = laset<T>(c, 2, n, n, T(0), T(1), VTx, n);
        if (!rc) rc = trsm_right_upper<T>(c, NonUnit, n, n, T(1), R2, n, VTx, n);
        if (!rc) rc = lange_fro<T>(c, n, n, R2, n, &nr);
        if (!rc) rc = lange_fro<T>(c, n, n, VTx, n, &ni);
        if (rc) return rc;
        recover_v = ((double)nr * (double)ni < ((sizeof(T) == 8) ? 1e3 : 30.0));
    }
    c->path_count[one_pass ? 17 : 16]++;
    if (recover_v) c->path_count[18]++;
    int jinfo = gesvdj_core<T>(c, n, n, X, n, S, recover_v ? (T*)nullptr : VTx, n, &sw);   // X = Ux S VTx
    if (sweeps_host) *sweeps_host = sw;
    if (jinfo < 0) return jinfo;
    if (recover_v) {
        // VTx (used as scratch for Vx, NOT transposed here) = R * Ux, columns scaled by 1 / sigma;  U_out = Q * Vx
        rc = gemm<T>(c, 0, 0, n, n, n, T(1), R2, n, X, n, T(0), VTx, n);
        if (!rc) {
            hipLaunchKernelGGL(scale_cols_inv_kernel<T>, dim3((unsigned)((n * n + 255) / 256)), dim3(256), 0, c->stream, n, n, VTx, (int64_t)n, S);
            RLHIP_LAUNCH_CHECK();
            rc = gemm<T>(c, 0, 0, m, n, n, T(1), A, lda, VTx, n, T(0), U, ldu);
        }
    } else {
        // U_out = Q * Vx = Q * VTx^T
        rc = gemm<T>(c, 0, 1, m, n, n, T(1), A, lda, VTx, n, T(0), U, ldu);
    }
    // VT_out = Ux^T
    if (!rc) rc = transpose<T>(c, n, n, X, n, VT, ldvt, 0);
    return rc ? rc : jinfo;
}

// the public entry: LAPACK's argument positions of gesdd(jobz, m, n, A, lda, S, U, ldu, VT, ldvt) for the codes -- nothing is enqueued before
// they pass -- then the exponent-range guard (qrcp.hip: svd_guard_begin): A is scaled by a power of two when max |a_ij| lies outside the
// window, every route below then sees entries of order 1, and S gets the scale back exactly; U and VT do not depend on it.
template <typename T>
int gesdd_tall(rlhip_ctx* c, int64_t m, int64_t n, T* A, int64_t lda, T* S, T* U, int64_t ldu, T* VT, int64_t ldvt,
               int* sweeps_host) {
    if (m < 0) return -2;
    if (n < 0) return -3;
    if (m < n) return -2;
    if (lda < (m > 1 ? m : 1)) return -5;
    if (ldu < (m > 1 ? m : 1)) return -8;
    if (ldvt < (n > 1 ? n : 1)) return -10;
    if (sweeps_host) *sweeps_host = 0;
    if (n == 0) return 0;
    ws_scope ws(c);
    unsigned long long* w = ws.alloc<unsigned long long>(4);
    if (!w) return RLHIP_ERR_HIP(hipErrorOutOfMemory);
    int rc = svd_guard_begin<T>(c, m, n, A, lda, w);
    int info = 0;
    if (!rc) info = gesdd_tall_core<T>(c, m, n, A, lda, S, U, ldu, VT, ldvt, sweeps_host);
    if (!rc && info >= 0) rc = svd_guard_end<T>(c, n, S, w);
    return rc ? rc : info;
}

template int transpose<double>(rlhip_ctx*, int64_t, int64_t, const double*, int64_t, double*, int64_t, int);
template int transpose<float>(rlhip_ctx*, int64_t, int64_t, const float*, int64_t, float*, int64_t, int);
template int gesdd_tall<double>(rlhip_ctx*, int64_t, int64_t, double*, int64_t, double*, double*, int64_t, double*, int64_t, int*);
template int gesdd_tall<float>(rlhip_ctx*, int64_t, int64_t, float*, int64_t, float*, float*, int64_t, float*, int64_t, int*);

}  // namespace rlhip
