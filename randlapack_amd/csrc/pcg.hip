// Device pieces of block / lockstep preconditioned conjugate gradients (RandLAPACK/comps/rl_determiter.hh:181-493) and of the spectral
// preconditioner (RandLAPACK/linops/rl_sym_linops.hh:204-379); the loop itself is include/RandLAPACK_amd/rl_determiter.hh.
//
//   posm_square            the Cholesky half of posm_square (rl_determiter.hh:244-257): one workgroup, LHS and RHS in LDS (s <= 64); wider
//                          problems go through potrf_upper, one triangular solve and two products on a scratch copy.
//   pcg_update_xr          X += P alpha, R -= GP alpha (:450-453) and the squared column norms of the new R in one pass: a thread owns a row.
//   pcg_update_p           P <- NR + P beta (:485-488) in place, a thread owns a row.
//   spectral_precond_apply SpectralPrecond::operator() (rl_sym_linops.hh:328-378): two products of the library's GEMM around one scaling
//                          kernel and one axpby kernel, then the squared column norms of the result.
//   ridge_filter           the filter of restricted kernel ridge regression (include/RandLAPACK_amd/rl_krill.hh, restricted_tail): one
//                          element-wise kernel between the two small products of that tail.
//   ridge_loo              the leave-one-out and residual sums of that fit for a grid of regularizations (rl_krill.hh, ridge_path; DESIGN
//                          4.26): one pass over the U of the thin SVD, a thread owns a row, every sum in double.
//
// No kernel here waits for another workgroup and none uses a floating-point atomic: a sum over rows goes through one partial per
// workgroup and column in the scratch arena (wave sums by shuffles, the four waves added in order) and a one-workgroup kernel that adds the
// partials in a fixed order, in double for both precisions.  Results are bitwise reproducible.
#include <cmath>
#include "rlhip_internal.h"
#include "rlhip_device.h"

namespace {

using namespace rlhip_dev;

constexpr int FUSED_MAX = 64;       // widest block the row-per-thread kernels and the one-workgroup solve serve

__device__ inline double dsqrt(double x) { return sqrt(x); }
__device__ inline float dsqrt(float x) { return sqrtf(x); }

// ---- (a) posm_square, s <= 64.  Dynamic LDS: L (s x s, ld s + 1), then B (s x s, ld s + 1).  Unblocked right-looking Cholesky of the lower
// triangle; every thread reads the pivot after the barrier that ends the previous step, so the failure test is uniform and a failing
// workgroup leaves without having written anything but the status.
template <typename T>
__global__ __launch_bounds__(256) void posm_square_kernel(int s, const T* __restrict__ LHS, T* __restrict__ RHS, int diag_only,
                                                          int64_t* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) char posm_smem[];
    const int ld = s + 1;
    T* L = (T*)posm_smem;
    T* B = L + (size_t)s * ld;
    const int tid = threadIdx.x;
    for (int t = tid; t < s * s; t += 256) {
        const int i = t % s, j = t / s;
        const bool keep = !diag_only || i == j;                                              // zero_off_diagonal (:154-161) on both
        L[i + j * ld] = (i >= j && keep) ? LHS[t] : T(0);
        B[i + j * ld] = keep ? RHS[t] : T(0);
    }
    __syncthreads();
    for (int k = 0; k < s; ++k) {
        const T p = L[k + k * ld];
        if (!(p > T(0))) {                                                                   // dpotrf's test: <= 0 or NaN
            if (tid == 0) *status = -1;
            return;
        }
        const T d = dsqrt(p);
        __syncthreads();
        for (int i = k + tid; i < s; i += 256) L[i + k * ld] = i == k ? d : L[i + k * ld] / d;
        __syncthreads();
        const int m = s - k - 1;
        if (!diag_only) {
            for (int t = tid; t < m * m; t += 256) {
                const int ii = t % m, jj = t / m;
                if (ii >= jj) L[(k + 1 + ii) + (k + 1 + jj) * ld] -= L[(k + 1 + ii) + k * ld] * L[(k + 1 + jj) + k * ld];
            }
        }
        __syncthreads();
    }
    if (tid < s) {                                                                           // L y = b, then L^T x = y (:248-255): a thread owns a column
        T* b = B + tid * ld;
        for (int i = 0; i < s; ++i) {
            T acc = b[i];
            for (int l = 0; l < i; ++l) acc -= L[i + l * ld] * b[l];
            b[i] = acc / L[i + i * ld];
        }
        for (int i = s - 1; i >= 0; --i) {
            T acc = b[i];
            for (int l = i + 1; l < s; ++l) acc -= L[l + i * ld] * b[l];
            b[i] = acc / L[i + i * ld];
        }
    }
    __syncthreads();
    for (int t = tid; t < s * s; t += 256) {
        const int i = t % s, j = t / s;
        RHS[t] = (diag_only && i != j) ? T(0) : B[i + j * ld];
    }
    if (tid == 0) *status = s;
}

// lockstep mode for s > 64: s independent pivots, no LDS copy
template <typename T>
__global__ __launch_bounds__(256) void posm_diag_kernel(int64_t s, const T* __restrict__ LHS, T* __restrict__ RHS, int64_t* __restrict__ status) {
    int bad = 0;
    for (int64_t i = threadIdx.x; i < s; i += 256) bad |= !(LHS[i + i * s] > T(0));
    if (__syncthreads_or(bad)) {
        if (threadIdx.x == 0) *status = -1;
        return;
    }
    for (int64_t t = threadIdx.x; t < s * s; t += 256) {
        const int64_t i = t % s, j = t / s;
        if (i != j) { RHS[t] = T(0); continue; }
        const T d = dsqrt(LHS[t]);
        RHS[t] = (RHS[t] / d) / d;
    }
    if (threadIdx.x == 0) *status = s;
}

__global__ void set_status_kernel(int64_t* status, int64_t v) { *status = v; }

// ---- (b) sums over rows.  part is nblk x s (partial b of column j at part[b * s + j]).
// squared column norms of A (n x s): one partial per workgroup of 256 rows
template <typename T>
__global__ __launch_bounds__(256) void colnorm2_partial_kernel(int64_t n, int64_t s, const T* __restrict__ A, int64_t lda, double* __restrict__ part) {
    __shared__ double wsum[4 * FUSED_MAX];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t i = (int64_t)blockIdx.x * 256 + tid;
    for (int64_t j0 = 0; j0 < s; j0 += FUSED_MAX) {
        const int cnt = (int)((s - j0) < FUSED_MAX ? (s - j0) : FUSED_MAX);
        for (int j = 0; j < cnt; ++j) {
            const double v = i < n ? (double)A[i + (j0 + j) * lda] : 0.0;
            const double w = wave_sum(v * v);
            if (lane == 0) wsum[wave * FUSED_MAX + j] = w;
        }
        __syncthreads();
        if (tid < cnt)
            part[(int64_t)blockIdx.x * s + j0 + tid] = ((wsum[tid] + wsum[FUSED_MAX + tid]) + wsum[2 * FUSED_MAX + tid]) + wsum[3 * FUSED_MAX + tid];
        __syncthreads();
    }
}

// out[j] = sum_b part[b * s + j]: lane l of a wave adds the partials l, l + 64, ... in order, then the 64 lanes are added by shuffles
__global__ __launch_bounds__(256) void colnorm2_final_kernel(int64_t nblk, int64_t s, const double* __restrict__ part, double* __restrict__ out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t j = wave; j < s; j += 4) {
        double acc = 0.0;
        for (int64_t b = lane; b < nblk; b += 64) acc += part[b * s + j];
        acc = wave_sum(acc);
        if (lane == 0) out[j] = acc;
    }
}

// ---- (c) the two updates, s <= MAXS <= 64.  The coefficient matrix (s x s, ld s) is staged once in LDS, zero-padded to MAXS rows; a thread
// reads its row of P (or GP) into registers and forms one entry of the result per column against the LDS copy, which every lane reads at
// the same address.
template <typename T, int MAXS>
__device__ __forceinline__ void stage_coeff(T* cs, const T* __restrict__ coef, int s) {
    for (int t = threadIdx.x; t < MAXS * MAXS; t += 256) {
        const int l = t % MAXS, j = t / MAXS;
        cs[t] = (l < s && j < s) ? coef[l + j * s] : T(0);
    }
}

template <typename T, int MAXS>
__global__ __launch_bounds__(256) void pcg_update_xr_kernel(int64_t n, int s, const T* __restrict__ alpha, const T* __restrict__ P, int64_t ldp,
                                                            const T* __restrict__ GP, int64_t ldgp, T* __restrict__ X, int64_t ldx,
                                                            T* __restrict__ R, int64_t ldr, double* __restrict__ part) {
    __shared__ T cs[MAXS * MAXS];
    __shared__ double wsum[4 * MAXS];
    stage_coeff<T, MAXS>(cs, alpha, s);
    __syncthreads();
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t i = (int64_t)blockIdx.x * 256 + tid;
    const bool live = i < n;
    T v[MAXS];
#pragma unroll
    for (int l = 0; l < MAXS; ++l) v[l] = (live && l < s) ? P[i + l * ldp] : T(0);
    if (live) {
        for (int j = 0; j < s; ++j) {                                                        // X <- X + P alpha           (:450)
            T acc = X[i + j * ldx];
#pragma unroll
            for (int l = 0; l < MAXS; ++l) acc += v[l] * cs[l + j * MAXS];
            X[i + j * ldx] = acc;
        }
    }
#pragma unroll
    for (int l = 0; l < MAXS; ++l) v[l] = (live && l < s) ? GP[i + l * ldgp] : T(0);
    for (int j = 0; j < s; ++j) {                                                            // R <- R - GP alpha          (:452)
        T acc = T(0);
        if (live) {
            acc = R[i + j * ldr];
#pragma unroll
            for (int l = 0; l < MAXS; ++l) acc -= v[l] * cs[l + j * MAXS];
            R[i + j * ldr] = acc;
        }
        if (part) {
            const double w = wave_sum((double)acc * (double)acc);
            if (lane == 0) wsum[wave * MAXS + j] = w;
        }
    }
    if (part) {
        __syncthreads();
        if (tid < s) part[(int64_t)blockIdx.x * s + tid] = ((wsum[tid] + wsum[MAXS + tid]) + wsum[2 * MAXS + tid]) + wsum[3 * MAXS + tid];
    }
}

template <typename T, int MAXS>
__global__ __launch_bounds__(256) void pcg_update_p_kernel(int64_t n, int s, const T* __restrict__ beta, const T* __restrict__ NR, int64_t ldnr,
                                                           T* __restrict__ P, int64_t ldp) {
    __shared__ T cs[MAXS * MAXS];
    stage_coeff<T, MAXS>(cs, beta, s);
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    T v[MAXS];
#pragma unroll
    for (int l = 0; l < MAXS; ++l) v[l] = l < s ? P[i + l * ldp] : T(0);
    for (int j = 0; j < s; ++j) {                                                            // P <- NR + P beta           (:485-488)
        T acc = NR[i + j * ldnr];
#pragma unroll
        for (int l = 0; l < MAXS; ++l) acc += v[l] * cs[l + j * MAXS];
        P[i + j * ldp] = acc;
    }
}

// ---- (d) the preconditioner's two element-wise steps
template <typename T>
__global__ void precond_scale_kernel(int64_t dim_pre, int64_t n, const T* __restrict__ D, int64_t num_ops, T* __restrict__ W) {
    const int64_t total = dim_pre * n;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = t % dim_pre, j = t / dim_pre;
        W[t] *= D[i + (num_ops == 1 ? 0 : j) * dim_pre];                                     // mat_D (rl_sym_linops.hh:347)
    }
}

// C = beta C + alpha B; beta == 0 does not read C
template <typename T>
__global__ void precond_axpby_kernel(int64_t dim, int64_t n, T alpha, const T* __restrict__ B, int64_t ldb, T beta, T* __restrict__ C, int64_t ldc) {
    const int64_t total = dim * n;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = t % dim, j = t / dim;
        const T b = alpha * B[i + j * ldb];
        C[i + j * ldc] = beta == T(0) ? b : beta * C[i + j * ldc] + b;
    }
}

// ---- (e) C(j, i) *= sigma[j] / (sigma[j]^2 + mu_i), the factor in double for both precisions and rounded once to T.  mu_i == 0: the
// pseudo-inverse, factor 0 where sigma[j] <= rcond sigma[0].  A thread owns an entry; beyond the grid's cap it strides.
template <typename T>
__global__ __launch_bounds__(256) void ridge_filter_kernel(int64_t k, int64_t s, const T* __restrict__ sigma, const T* __restrict__ mus,
                                                           int64_t num_mus, T rcond, T* __restrict__ C, int64_t ldc) {
    const int64_t total = k * s;
    const double cut = (double)rcond * (double)sigma[0];
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t j = t % k, i = t / k;
        const double sg = (double)sigma[j], mu = (double)mus[num_mus == 1 ? 0 : i];
        const double f = (mu == 0.0 && sg <= cut) ? 0.0 : sg / fma(sg, sg, mu);
        C[j + i * ldc] *= (T)f;
    }
}

// ---- (f) the leave-one-out table of restricted kernel ridge regression.  With d_jm = sigma_j^2 / (sigma_j^2 + mu_m), row i has
// the leverage s_im = sum_j U_ij^2 d_jm and the fitted value yhat_imc = sum_j U_ij d_jm C_jc; its leave-one-out residual is
// (h_ic - yhat_imc) / (1 - s_im).  A thread owns a row of U and walks its k columns once per (grid chunk, column chunk): LOO_GC grid values
// and LC columns, so LOO_GC (1 + LC) sums in registers, all in double.  The tables d_jm and d_jm C_jc of a slab of LOO_JS columns sit in
// LDS, where every lane reads the same address.  One partial per workgroup and entry goes to scratch (wave sums by shuffles, the four waves
// added in order); ridge_loo_final_kernel adds the partials in a fixed order.  A workgroup always owns LOO_ROWS rows, so the bits depend on
// the shapes alone.
constexpr int LOO_ROWS = 256, LOO_JS = 64, LOO_GC = 8, LOO_LC = 4;

template <typename T, int LC>
__global__ __launch_bounds__(LOO_ROWS) void ridge_loo_partial_kernel(int64_t n, int64_t k, int64_t ell, int64_t g, const T* __restrict__ U, int64_t ldu,
                                                                     const T* __restrict__ sigma, const T* __restrict__ C, int64_t ldc,
                                                                     const T* __restrict__ H, int64_t ldh, const T* __restrict__ mus, T rcond,
                                                                     double* __restrict__ part) {
    constexpr int NQ = LOO_GC * LC;
    __shared__ double dt[LOO_JS * LOO_GC];
    __shared__ double ct[LOO_JS * NQ];
    __shared__ double wsum[4 * 2 * NQ];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t i = (int64_t)blockIdx.x * LOO_ROWS + tid;
    const bool live = i < n;
    const int64_t m0 = (int64_t)blockIdx.y * LOO_GC, c0 = (int64_t)blockIdx.z * LC;
    const double cut = (double)rcond * (double)sigma[0];
    double sa[LOO_GC], ya[NQ];
#pragma unroll
    for (int m = 0; m < LOO_GC; ++m) sa[m] = 0.0;
#pragma unroll
    for (int q = 0; q < NQ; ++q) ya[q] = 0.0;
    for (int64_t j0 = 0; j0 < k; j0 += LOO_JS) {
        const int cnt = (int)((k - j0) < LOO_JS ? (k - j0) : LOO_JS);
        __syncthreads();                                                                     // the previous slab has been read
        for (int t = tid; t < LOO_JS * LOO_GC; t += LOO_ROWS) {
            const int jj = t / LOO_GC, m = t % LOO_GC;
            double d = 0.0;
            if (jj < cnt && m0 + m < g) {                                                    // beyond the slab or the grid: 0, which adds nothing
                const double sg = (double)sigma[j0 + jj], mu = (double)mus[m0 + m];
                d = mu == 0.0 ? (sg <= cut ? 0.0 : 1.0) : (sg * sg) / fma(sg, sg, mu);
            }
            dt[t] = d;
#pragma unroll
            for (int c = 0; c < LC; ++c) ct[t * LC + c] = (jj < cnt && c0 + c < ell) ? d * (double)C[(j0 + jj) + (c0 + c) * ldc] : 0.0;
        }
        __syncthreads();
        const T* up = U + (live ? i : 0) + j0 * ldu;
#pragma unroll 4
        for (int jj = 0; jj < cnt; ++jj) {
            const double u = live ? (double)up[(int64_t)jj * ldu] : 0.0;
            const double u2 = u * u;
#pragma unroll
            for (int m = 0; m < LOO_GC; ++m) sa[m] = fma(u2, dt[jj * LOO_GC + m], sa[m]);
#pragma unroll
            for (int q = 0; q < NQ; ++q) ya[q] = fma(u, ct[jj * NQ + q], ya[q]);
        }
    }
#pragma unroll
    for (int c = 0; c < LC; ++c) {
        const bool col = live && c0 + c < ell;
        const double h = col ? (double)H[i + (c0 + c) * ldh] : 0.0;
#pragma unroll
        for (int m = 0; m < LOO_GC; ++m) {
            const bool on = col && m0 + m < g;
            const double r = h - ya[m * LC + c];
            const double e = r / (1.0 - sa[m]);                                              // 1 - s == 0: inf or NaN, reported as it is
            const double lo = wave_sum(on ? e * e : 0.0), rs = wave_sum(on ? r * r : 0.0);
            if (lane == 0) {
                wsum[(wave * 2 + 0) * NQ + m * LC + c] = lo;
                wsum[(wave * 2 + 1) * NQ + m * LC + c] = rs;
            }
        }
    }
    __syncthreads();
    if (tid < 2 * NQ) {
        const int which = tid / NQ, q = tid % NQ, m = q / LC, c = q % LC;
        if (m0 + m < g && c0 + c < ell) {
            const double v = ((wsum[which * NQ + q] + wsum[(2 + which) * NQ + q]) + wsum[(4 + which) * NQ + q]) + wsum[(6 + which) * NQ + q];
            part[((int64_t)which * gridDim.x + blockIdx.x) * (g * ell) + (m0 + m) + (c0 + c) * g] = v;
        }
    }
}

// entry e of (loo | rss), each g x ell: lane l of the wave that owns it adds the partials l, l + 64, ... in order, then the 64 lanes are
// added by shuffles
__global__ __launch_bounds__(256) void ridge_loo_final_kernel(int64_t nblk, int64_t ge, const double* __restrict__ part, double* __restrict__ loo,
                                                              double* __restrict__ rss) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t e = (int64_t)blockIdx.x * 4 + wave;
    if (e >= 2 * ge) return;
    const int64_t which = e / ge, q = e % ge;
    double acc = 0.0;
    for (int64_t b = lane; b < nblk; b += 64) acc += part[(which * nblk + b) * ge + q];
    acc = wave_sum(acc);
    if (lane == 0) (which ? rss : loo)[q] = acc;
}

inline unsigned stream_grid(rlhip_ctx* c, int64_t total) {
    const int64_t want = (total + 255) / 256, cap = (int64_t)c->num_cu * 8;
    return (unsigned)(want < 1 ? 1 : (want < cap ? want : cap));
}

template <typename T>
int colnorm2(rlhip_ctx* c, int64_t n, int64_t s, const T* A, int64_t lda, double* out) {
    if (n < 0) return -2;
    if (s < 0) return -3;
    if (lda < (n > 1 ? n : 1)) return -5;
    if (!out) return -6;
    if (s == 0) return 0;
    const int64_t nblk = (n + 255) / 256;
    ws_scope ws(c);
    double* part = ws.alloc<double>((size_t)((nblk > 0 ? nblk : 1) * s));
    if (!part) return RLHIP_ERR_HIP(hipErrorOutOfMemory);
    if (nblk > 0) hipLaunchKernelGGL(colnorm2_partial_kernel<T>, dim3((unsigned)nblk), dim3(256), 0, c->stream, n, s, A, lda, part);
    hipLaunchKernelGGL(colnorm2_final_kernel, dim3(1), dim3(256), 0, c->stream, nblk, s, part, out);
    RLHIP_LAUNCH_CHECK();
    return 0;
}

template <typename T>
int posm_square(rlhip_ctx* c, int64_t s, const T* LHS, T* RHS, int diag_only, int64_t* status) {
    if (s < 0) return -2;
    if (!status) return -6;
    if (s > 0 && !LHS) return -3;
    if (s > 0 && !RHS) return -4;
    if (s == 0) {
        hipLaunchKernelGGL(set_status_kernel, dim3(1), dim3(1), 0, c->stream, status, (int64_t)0);
        RLHIP_LAUNCH_CHECK();
        return 0;
    }
    if (s <= FUSED_MAX) {
        const size_t lds = 2 * (size_t)FUSED_MAX * (FUSED_MAX + 1) * sizeof(T);
        RLHIP_FUNC_LDS(c, posm_square_kernel<T>, lds);
        hipLaunchKernelGGL(posm_square_kernel<T>, dim3(1), dim3(256), 2 * (size_t)s * (s + 1) * sizeof(T), c->stream, (int)s, LHS, RHS, diag_only,
                           status);
        RLHIP_LAUNCH_CHECK();
        return 0;
    }
    if (diag_only) {
        hipLaunchKernelGGL(posm_diag_kernel<T>, dim3(1), dim3(256), 0, c->stream, s, LHS, RHS, status);
        RLHIP_LAUNCH_CHECK();
        return 0;
    }
    // composed route: the upper triangle of A = LHS^T is LHS's lower one; A = U^T U, RHS <- U^-1 (U^-T RHS) with U^-1 = I U^-1 formed once
    ws_scope ws(c);
    T* A = ws.alloc<T>((size_t)(s * s));
    T* Ui = ws.alloc<T>((size_t)(s * s));
    T* W = ws.alloc<T>((size_t)(s * s));
    if (!A || !Ui || !W) return RLHIP_ERR_HIP(hipErrorOutOfMemory);
    int rc = rlhip::transpose<T>(c, s, s, LHS, s, A, s, 0);
    if (rc) return rc;
    int info = 0;
    rc = rlhip::potrf_upper<T>(c, s, A, s, &info);
    if (rc) return rc;
    if (info == 0) {
        rc = rlhip::laset<T>(c, 2, s, s, T(0), T(1), Ui, s);
        if (rc == 0) rc = rlhip::trsm_right_upper<T>(c, rlhip::NonUnit, s, s, T(1), A, s, Ui, s);
        if (rc == 0) rc = rlhip::gemm<T>(c, rlhip::Trans, rlhip::NoTrans, s, s, s, T(1), Ui, s, RHS, s, T(0), W, s);
        if (rc == 0) rc = rlhip::gemm<T>(c, rlhip::NoTrans, rlhip::NoTrans, s, s, s, T(1), Ui, s, W, s, T(0), RHS, s);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(set_status_kernel, dim3(1), dim3(1), 0, c->stream, status, info == 0 ? s : (int64_t)-1);
    RLHIP_LAUNCH_CHECK();
    return 0;
}

template <typename T>
int pcg_update_xr(rlhip_ctx* c, int64_t n, int64_t s, const T* alpha, const T* P, int64_t ldp, const T* GP, int64_t ldgp, T* X, int64_t ldx,
                  T* R, int64_t ldr, double* colnorm2_out) {
    const int64_t ldmin = n > 1 ? n : 1;
    if (n < 0) return -2;
    if (s < 0) return -3;
    if (ldp < ldmin) return -6;
    if (ldgp < ldmin) return -8;
    if (ldx < ldmin) return -10;
    if (ldr < ldmin) return -12;
    if (s == 0) return 0;
    if (s > FUSED_MAX) {
        c->pcg_path_count[2]++;
        int rc = rlhip::gemm<T>(c, rlhip::NoTrans, rlhip::NoTrans, n, s, s, T(1), P, ldp, alpha, s, T(1), X, ldx);
        if (rc == 0) rc = rlhip::gemm<T>(c, rlhip::NoTrans, rlhip::NoTrans, n, s, s, T(-1), GP, ldgp, alpha, s, T(1), R, ldr);
        if (rc == 0 && colnorm2_out) rc = colnorm2<T>(c, n, s, R, ldr, colnorm2_out);
        return rc;
    }
    c->pcg_path_count[0]++;
    const int64_t nblk = (n + 255) / 256;
    ws_scope ws(c);
    double* part = nullptr;
    if (colnorm2_out) {
        part = ws.alloc<double>((size_t)((nblk > 0 ? nblk : 1) * s));
        if (!part) return RLHIP_ERR_HIP(hipErrorOutOfMemory);
    }
    if (nblk > 0) {
        const dim3 g((unsigned)nblk), blk(256);
        if (s <= 8) hipLaunchKernelGGL((pcg_update_xr_kernel<T, 8>), g, blk, 0, c->stream, n, (int)s, alpha, P, ldp, GP, ldgp, X, ldx, R, ldr, part);
        else if (s <= 16) hipLaunchKernelGGL((pcg_update_xr_kernel<T, 16>), g, blk, 0, c->stream, n, (int)s, alpha, P, ldp, GP, ldgp, X, ldx, R, ldr, part);
        else if (s <= 32) hipLaunchKernelGGL((pcg_update_xr_kernel<T, 32>), g, blk, 0, c->stream, n, (int)s, alpha, P, ldp, GP, ldgp, X, ldx, R, ldr, part);
        else hipLaunchKernelGGL((pcg_update_xr_kernel<T, 64>), g, blk, 0, c->stream, n, (int)s, alpha, P, ldp, GP, ldgp, X, ldx, R, ldr, part);
    }
    if (colnorm2_out) hipLaunchKernelGGL(colnorm2_final_kernel, dim3(1), dim3(256), 0, c->stream, nblk, s, part, colnorm2_out);
    RLHIP_LAUNCH_CHECK();
    return 0;
}

template <typename T>
int pcg_update_p(rlhip_ctx* c, int64_t n, int64_t s, const T* beta, const T* NR, int64_t ldnr, T* P, int64_t ldp) {
    const int64_t ldmin = n > 1 ? n : 1;
    if (n < 0) return -2;
    if (s < 0) return -3;
    if (ldnr < ldmin) return -6;
    if (ldp < ldmin) return -8;
    if (s == 0 || n == 0) return 0;
    if (s > FUSED_MAX) {                       // the product cannot run in place: NR is copied, P beta added to the copy, the copy moved into P
        c->pcg_path_count[2]++;
        ws_scope ws(c);
        T* tmp = ws.alloc<T>((size_t)(n * s));
        if (!tmp) return RLHIP_ERR_HIP(hipErrorOutOfMemory);
        int rc = rlhip::lacpy<T>(c, 2, n, s, NR, ldnr, tmp, n);
        if (rc == 0) rc = rlhip::gemm<T>(c, rlhip::NoTrans, rlhip::NoTrans, n, s, s, T(1), P, ldp, beta, s, T(1), tmp, n);
        if (rc == 0) rc = rlhip::lacpy<T>(c, 2, n, s, tmp, n, P, ldp);
        return rc;
    }
    c->pcg_path_count[1]++;
    const dim3 g(grid1(n, 256)), blk(256);
    if (s <= 8) hipLaunchKernelGGL((pcg_update_p_kernel<T, 8>), g, blk, 0, c->stream, n, (int)s, beta, NR, ldnr, P, ldp);
    else if (s <= 16) hipLaunchKernelGGL((pcg_update_p_kernel<T, 16>), g, blk, 0, c->stream, n, (int)s, beta, NR, ldnr, P, ldp);
    else if (s <= 32) hipLaunchKernelGGL((pcg_update_p_kernel<T, 32>), g, blk, 0, c->stream, n, (int)s, beta, NR, ldnr, P, ldp);
    else hipLaunchKernelGGL((pcg_update_p_kernel<T, 64>), g, blk, 0, c->stream, n, (int)s, beta, NR, ldnr, P, ldp);
    RLHIP_LAUNCH_CHECK();
    return 0;
}

template <typename T>
int spectral_precond_apply(rlhip_ctx* c, int64_t dim, int64_t dim_pre, const T* V, int64_t ldv, const T* D, int64_t num_ops, int64_t n, T alpha,
                           const T* B, int64_t ldb, T beta, T* C, int64_t ldc, T* W, double* colnorm2_out) {
    const int64_t ldmin = dim > 1 ? dim : 1;
    if (dim < 0) return -2;
    if (dim_pre < 0) return -3;
    if (ldv < ldmin) return -5;
    if (num_ops < 1) return -7;
    if (n < 0 || (num_ops != 1 && n != num_ops)) return -8;
    if (ldb < ldmin) return -11;
    if (ldc < ldmin) return -14;
    if (dim_pre > 0 && n > 0 && !W) return -15;
    if (n == 0) return 0;
    int rc = 0;
    if (dim_pre > 0 && dim > 0) {
        rc = rlhip::gemm<T>(c, rlhip::Trans, rlhip::NoTrans, dim_pre, n, dim, T(1), V, ldv, B, ldb, T(0), W, dim_pre);        // :344
        if (rc) return rc;
        hipLaunchKernelGGL(precond_scale_kernel<T>, dim3(stream_grid(c, dim_pre * n)), dim3(256), 0, c->stream, dim_pre, n, D, num_ops, W);   // :349-353
    }
    if (dim > 0)
        hipLaunchKernelGGL(precond_axpby_kernel<T>, dim3(stream_grid(c, dim * n)), dim3(256), 0, c->stream, dim, n, alpha, B, ldb, beta, C, ldc);   // :362-371
    RLHIP_LAUNCH_CHECK();
    if (dim_pre > 0 && dim > 0) {
        rc = rlhip::gemm<T>(c, rlhip::NoTrans, rlhip::NoTrans, dim, n, dim_pre, alpha, V, ldv, W, dim_pre, T(1), C, ldc);     // :376
        if (rc) return rc;
    }
    if (colnorm2_out) rc = colnorm2<T>(c, dim, n, C, ldc, colnorm2_out);
    return rc;
}

template <typename T>
int ridge_filter(rlhip_ctx* c, int64_t k, int64_t s, const T* sigma, const T* mus, int64_t num_mus, T rcond, T* C, int64_t ldc) {
    if (!c) return -1;
    if (k < 0) return -2;
    if (s < 0) return -3;
    if (ldc < (k > 1 ? k : 1)) return -9;
    if (k == 0 || s == 0) return 0;
    if (!sigma) return -4;
    if (!mus) return -5;
    if (num_mus != 1 && num_mus != s) return -100;
    if (!(rcond >= T(0))) return -7;
    if (!C) return -8;
    hipLaunchKernelGGL(ridge_filter_kernel<T>, dim3(stream_grid(c, k * s)), dim3(256), 0, c->stream, k, s, sigma, mus, num_mus, rcond, C, ldc);
    RLHIP_LAUNCH_CHECK();
    return 0;
}

template <typename T>
int ridge_loo(rlhip_ctx* c, int64_t n, int64_t k, int64_t ell, int64_t g, const T* U, int64_t ldu, const T* sigma, const T* C, int64_t ldc, const T* H,
              int64_t ldh, const T* mus, T rcond, double* loo, double* rss) {
    if (!c) return -1;
    if (n < 0) return -2;
    if (k < 0) return -3;
    if (ell < 0) return -4;
    if (g < 0) return -5;
    if (ldu < (n > 1 ? n : 1)) return -7;
    if (ldc < (k > 1 ? k : 1)) return -10;
    if (ldh < (n > 1 ? n : 1)) return -12;
    if (n == 0 || k == 0 || ell == 0 || g == 0) return 0;
    if (!U) return -6;
    if (!sigma) return -8;
    if (!C) return -9;
    if (!H) return -11;
    if (!mus) return -13;
    if (!(rcond >= T(0))) return -14;
    if (!loo) return -15;
    if (!rss) return -16;
    const int64_t nblk = (n + LOO_ROWS - 1) / LOO_ROWS, gchunks = (g + LOO_GC - 1) / LOO_GC;
    const int lc = ell == 1 ? 1 : LOO_LC;
    const int64_t cchunks = (ell + lc - 1) / lc;
    if (nblk > 0x7fffffff || gchunks > 65535 || cchunks > 65535) return -100;
    ws_scope ws(c);
    double* part = ws.alloc<double>((size_t)(2 * nblk * g * ell));
    if (!part) return RLHIP_ERR_HIP(hipErrorOutOfMemory);
    const dim3 grid((unsigned)nblk, (unsigned)gchunks, (unsigned)cchunks), blk(LOO_ROWS);
    if (lc == 1)
        hipLaunchKernelGGL((ridge_loo_partial_kernel<T, 1>), grid, blk, 0, c->stream, n, k, ell, g, U, ldu, sigma, C, ldc, H, ldh, mus, rcond, part);
    else
        hipLaunchKernelGGL((ridge_loo_partial_kernel<T, LOO_LC>), grid, blk, 0, c->stream, n, k, ell, g, U, ldu, sigma, C, ldc, H, ldh, mus, rcond, part);
    hipLaunchKernelGGL(ridge_loo_final_kernel, dim3(grid1(2 * g * ell, 4)), dim3(256), 0, c->stream, nblk, g * ell, part, loo, rss);
    RLHIP_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" {

int64_t rlhip_pcg_path_count(rlhip_ctx* c, int which) { return (c && which >= 43 && which <= 45) ? c->pcg_path_count[which - 43] : -1; }

#define RLHIP_DEFINE_PCG(SUF, T)                                                                                                             \
    int rlhip_posm_square_##SUF(rlhip_ctx* c, int64_t s, const T* LHS, T* RHS, int diag_only, int64_t* status_dev) {                         \
        return posm_square<T>(c, s, LHS, RHS, diag_only, status_dev);                                                                        \
    }                                                                                                                                        \
    int rlhip_pcg_update_xr_##SUF(rlhip_ctx* c, int64_t n, int64_t s, const T* alpha_dev, const T* P, int64_t ldp, const T* GP, int64_t ldgp, \
                                  T* X, int64_t ldx, T* R, int64_t ldr, double* colnorm2_dev) {                                              \
        return pcg_update_xr<T>(c, n, s, alpha_dev, P, ldp, GP, ldgp, X, ldx, R, ldr, colnorm2_dev);                                         \
    }                                                                                                                                        \
    int rlhip_pcg_update_p_##SUF(rlhip_ctx* c, int64_t n, int64_t s, const T* beta_dev, const T* NR, int64_t ldnr, T* P, int64_t ldp) {      \
        return pcg_update_p<T>(c, n, s, beta_dev, NR, ldnr, P, ldp);                                                                         \
    }                                                                                                                                        \
    int rlhip_pcg_colnorm2_##SUF(rlhip_ctx* c, int64_t n, int64_t s, const T* A, int64_t lda, double* colnorm2_dev) {                        \
        return colnorm2<T>(c, n, s, A, lda, colnorm2_dev);                                                                                   \
    }                                                                                                                                        \
    int rlhip_spectral_precond_apply_##SUF(rlhip_ctx* c, int64_t dim, int64_t dim_pre, const T* V, int64_t ldv, const T* D_dev,              \
                                           int64_t num_ops, int64_t n, T alpha, const T* B, int64_t ldb, T beta, T* C, int64_t ldc,          \
                                           T* W_dev, double* colnorm2_dev) {                                                                 \
        return spectral_precond_apply<T>(c, dim, dim_pre, V, ldv, D_dev, num_ops, n, alpha, B, ldb, beta, C, ldc, W_dev, colnorm2_dev);      \
    }                                                                                                                                        \
    int rlhip_ridge_filter_##SUF(rlhip_ctx* c, int64_t k, int64_t s, const T* sigma_dev, const T* mus_dev, int64_t num_mus, T rcond, T* C,   \
                                 int64_t ldc) {                                                                                              \
        return ridge_filter<T>(c, k, s, sigma_dev, mus_dev, num_mus, rcond, C, ldc);                                                         \
    }                                                                                                                                        \
    int rlhip_ridge_loo_##SUF(rlhip_ctx* c, int64_t n, int64_t k, int64_t ell, int64_t g, const T* U, int64_t ldu, const T* sigma_dev,       \
                              const T* C, int64_t ldc, const T* H, int64_t ldh, const T* mus_dev, T rcond, double* loo_dev, double* rss_dev) { \
        return ridge_loo<T>(c, n, k, ell, g, U, ldu, sigma_dev, C, ldc, H, ldh, mus_dev, rcond, loo_dev, rss_dev);                           \
    }
RLHIP_DEFINE_PCG(f64, double)
RLHIP_DEFINE_PCG(f32, float)

}  // extern "C"
