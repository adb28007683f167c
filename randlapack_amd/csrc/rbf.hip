// Squared-exponential (RBF) kernel between TWO point sets:
//   K(Z, X)(i, j) = exp(-|Z(:, i) - X(:, j)|^2 / (2 h^2)),  Z rows_x x mz,  X rows_x x nx, one column per point
//   rlhip_sqexp_cross_submatrix_*   a block of K(Z, X) written to memory: MFMA GEMM for -2 Z^T X + the epilogue of rpchol.hip
//   rlhip_rbf_cross_apply_*         C (mz x n) = alpha * K(Z, X) * B + beta * C
//       fused route    (n <= RLHIP_RBF_FUSED_MAX_N, rows_x <= RLHIP_RBF_FUSED_MAX_ROWS_X): ONE launch, K never in memory;
//       composed route (every other shape, or RLHIP_OPT_RBF_FUSED = 0): row blocks of K of at most max(2^26, nx) entries in the scratch
//                      arena, cross submatrix + GEMM with B per block -- rbf_apply's scheme for two point sets.
// Both routes evaluate an entry by the same formula, exp(scale * ((|z_i|^2 + |x_j|^2) - 2 z_i.x_j)), scale = -1 / (2 h^2) rounded from
// double, the accurate exp / expf, no clamp; they differ in the order of the sums only.
//   rlhip_pdk_cross_submatrix_*, rlhip_pdk_cross_apply_*: the same two routines with the kernel function as an argument.  The
//       Matern kinds evaluate matern_of_s (rlhip_device.h) where the squared exponential evaluates exp, on both routes: the squared distance
//       clamped at 0, a sqrt, two fused multiply-adds, an exp.
//   rlhip::pdk_cross_apply_fn: the apply behind its argument checks with the scalar function as a PdkFn, for rbf_grad.hip, whose gradient
//       weights run through the same two routes: the Matern weights as WEIGHT instantiations of the kernels, never split over X.
//
// The fused kernel.  A 256-thread workgroup owns 64 points of Z, 16 per wave; lane (g = lane >> 4, c = lane & 15) of a wave holds, for
// its wave's point c, the Z rows 4 kk + g (times -2, exact) in registers for the whole loop.  X is walked in tiles of TP points that are
// staged in LDS together with the matching TP x n tile of B and the TP norms, two buffers: the next tile's global loads are issued before
// the arithmetic on the current one and stored to the other buffer after it, one __syncthreads per tile.  Per sub-tile of 16 X points:
//   S^T (16 X points x 16 Z points) = X_sub^T * (-2 Z_frag)       KS MFMAs 16x16x4;  register r of lane (g, c) = X point drow_g(g, r), Z point c
//   P^T = exp(scale * ((zn + xn) + S^T))                          4 exp per lane, in the accumulator registers
//   C^T (n x 16 Z points) += B_sub^T * P^T                        4 NT MFMAs: register r IS the B operand of k-step r (k index g <-> X point
//                                                                 drow_g(g, r)), the A operand reads rows drow_g(g, r) of the B tile
// so P never goes through LDS.  The first product of sub-tile s + 1 is issued in front of the exps of sub-tile s: the matrix pipe works
// beside the VALU instead of in front of it.  X points past nx are never read: the staging stores zeros for them (rows of X, rows of B,
// norm), so such a point contributes exp(scale * zn) * 0 = 0 exactly.  The sums over j run in the order of j, sixteen at a time, whatever
// mz, the grid or the device: row i of the result is a function of Z(:, i), X, B, alpha, beta and C(i, :) alone.
//
// The split over X (RLHIP_OPT_RBF_FUSED = 2 only).  With few points of Z the grid above is a few workgroups that each walk
// all of X.  rlhip_rbf_split_chunks(mz, nx) = g is a function of the shape alone; where g > 1 the same kernel (SPLIT = true) runs on a grid
// of ztiles x g: workgroup (i, b) walks the points [b CH, min(nx, (b + 1) CH)) of X, CH a multiple of 64 and so of every TP, with the
// pipeline above -- the staging zero-fills behind the chunk's end -- and stores its raw accumulators to part[b][column][row] in the scratch
// arena (row stride: mz rounded up to 64, so every lane stores).  rbf_reduce_kernel, one thread per entry of C, adds the g partials in the
// order of b and applies alpha and beta.  No atomics, two launches; row i is a function of the same arguments and of g.
#include <cmath>
#include "rlhip_internal.h"
#include "rlhip_device.h"

namespace {
using namespace rlhip_dev;
using rlhip::PdkFn;

// RBF_WG, RBF_ZP, RBF_LDS_CAP, rbf_exp and the layout of the staged tiles (rbf_xs, rbf_bsp, rbf_tile_elems, rbf_tp) are in rlhip_device.h:
// rbf_var.hip stages its tiles the same way.

template <typename T>
struct RbfArgs {
    int64_t rows_x, mz, nx, n;
    const T* Z; int64_t ldz;
    const T* X; int64_t ldx;
    const T* zn; const T* xn;      // |Z(:, i)|^2, |X(:, j)|^2
    const T* B; int64_t ldb;
    T* C; int64_t ldc;
    T alpha, beta, scale, third;      // scale, third: PdkFn's constants
    T* part; int64_t ch, mzp;         // SPLIT only: the partials [chunk][column][row], points of X per chunk, rows of a partial (64 ztiles)
};

// MATERN = false is the squared exponential, true the two Matern kinds (told apart by a.third alone, matern_of_s): the squared exponential
// keeps an instantiation of its own, so the sqrt and the polynomial cost it no register.
// SPLIT = false walks all of X and writes C; SPLIT = true walks chunk blockIdx.y of X and writes its partial (see the header comment).
// WEIGHT = true (MATERN = true, SPLIT = false only): pdk_weight_of_s in place of matern_of_s, the gradient weight of DESIGN 4.30.
template <typename T, int KS, int NT, bool MATERN, bool SPLIT, bool WEIGHT = false>
__global__ __launch_bounds__(RBF_WG) void rbf_fused_kernel(const RbfArgs<T> a) {
    using M = Mfma16x4<T>;
    using acc_t = typename M::acc_t;
    constexpr int TP = rbf_tp<T, KS, NT>();
    constexpr int XS = rbf_xs<T, KS>(), BSP = rbf_bsp(TP);
    constexpr int XE = TP * 4 * KS, BE = TP * 16 * NT;                        // staged elements of one tile
    constexpr int XPT = (XE + RBF_WG - 1) / RBF_WG, BPT = (BE + RBF_WG - 1) / RBF_WG;
    constexpr int BUF = rbf_tile_elems<T, KS, NT>(TP);
    extern __shared__ __align__(16) unsigned char rbf_lds_raw[];
    T* const lds = reinterpret_cast<T*>(rbf_lds_raw);

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, c = lane & 15;
    const int64_t zp = (int64_t)blockIdx.x * RBF_ZP + 16 * w + c;
    const bool zok = zp < a.mz;

    T zreg[KS];
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) {
        const int row = 4 * kk + g;
        zreg[kk] = (zok && row < a.rows_x) ? T(-2) * a.Z[zp * a.ldz + row] : T(0);
    }
    const T znorm = zok ? a.zn[zp] : T(0);
    const int64_t xbeg = SPLIT ? (int64_t)blockIdx.y * a.ch : 0;                                     // this workgroup's points of X
    const int64_t xend = SPLIT ? (xbeg + a.ch < a.nx ? xbeg + a.ch : a.nx) : a.nx;

    acc_t acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[nt] = acc_t{0, 0, 0, 0};

    T xpre[XPT], bpre[BPT], npre = T(0);
    auto fetch = [&](int64_t x0) {      // global -> registers; nothing past point xend - 1, row rows_x - 1 or column n - 1 is read
#pragma unroll
        for (int e = 0; e < XPT; ++e) {
            const int idx = tid + RBF_WG * e, p = idx / (4 * KS), r = idx % (4 * KS);
            xpre[e] = (idx < XE && x0 + p < xend && r < a.rows_x) ? a.X[(x0 + p) * a.ldx + r] : T(0);
        }
#pragma unroll
        for (int e = 0; e < BPT; ++e) {
            const int idx = tid + RBF_WG * e, col = idx / TP, p = idx % TP;
            bpre[e] = (idx < BE && x0 + p < xend && col < a.n) ? a.B[(x0 + p) + (int64_t)col * a.ldb] : T(0);
        }
        npre = (tid < TP && x0 + tid < xend) ? a.xn[x0 + tid] : T(0);
    };
    auto stash = [&](T* buf) {          // registers -> LDS
        T* Xs = buf; T* Bs = buf + TP * XS; T* Ns = Bs + 16 * NT * BSP;
#pragma unroll
        for (int e = 0; e < XPT; ++e) {
            const int idx = tid + RBF_WG * e;
            if (idx < XE) Xs[(idx / (4 * KS)) * XS + idx % (4 * KS)] = xpre[e];
        }
#pragma unroll
        for (int e = 0; e < BPT; ++e) {
            const int idx = tid + RBF_WG * e;
            if (idx < BE) Bs[(idx / TP) * BSP + idx % TP] = bpre[e];
        }
        if (tid < TP) Ns[tid] = npre;
    };

    const int64_t ntiles = (xend - xbeg + TP - 1) / TP;
    fetch(xbeg);
    stash(lds);
    __syncthreads();
    for (int64_t t = 0; t < ntiles; ++t) {
        const T* buf = lds + (t & 1) * BUF;
        const T* Xs = buf; const T* Bs = buf + TP * XS; const T* Ns = Bs + 16 * NT * BSP;
        const bool more = t + 1 < ntiles;
        if (more) fetch(xbeg + (t + 1) * TP);

        auto first = [&](int st) {      // S^T of sub-tile st
            acc_t s = acc_t{0, 0, 0, 0};
            const T* xr = Xs + (16 * st + c) * XS + g;
#pragma unroll
            for (int kk = 0; kk < KS; ++kk) s = M::mma(xr[4 * kk], zreg[kk], s);
            return s;
        };
        acc_t s = first(0);
#pragma unroll
        for (int st = 0; st < TP / 16; ++st) {
            acc_t snext = acc_t{0, 0, 0, 0};
            if (st + 1 < TP / 16) snext = first(st + 1);      // the matrix pipe runs this beside the exps below
            T p[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const T sq = (znorm + Ns[16 * st + M::drow_g(g, r)]) + s[r];
                if constexpr (WEIGHT) p[r] = pdk_weight_of_s(sq, a.scale, a.third);
                else if constexpr (MATERN) p[r] = matern_of_s(sq, a.scale, a.third);
                else p[r] = rbf_exp(a.scale * sq);
            }
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const T* bc = Bs + (16 * nt + c) * BSP + 16 * st;      // column 16 nt + c of the B tile, this sub-tile's points
                T bv[4];
                if constexpr (sizeof(T) == 4) {
                    const float4 v = *reinterpret_cast<const float4*>(bc + 4 * g);      // drow_g(g, r) = 4 g + r; 16-byte aligned by construction
                    bv[0] = v.x; bv[1] = v.y; bv[2] = v.z; bv[3] = v.w;
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) bv[r] = bc[M::drow_g(g, r)];
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[nt] = M::mma(bv[r], p[r], acc[nt]);
            }
            s = snext;
        }
        if (more) stash(lds + ((t + 1) & 1) * BUF);
        __syncthreads();
    }

    if constexpr (SPLIT) {      // raw sums; the rows past mz of the last Z tile are stored too (mzp covers them) and never read
        T* const pr = a.part + (int64_t)blockIdx.y * a.n * a.mzp + zp;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int col = 16 * nt + M::drow_g(g, r);
                if (col < a.n) pr[(int64_t)col * a.mzp] = acc[nt][r];
            }
        }
        return;
    }
    if (!zok) return;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int col = 16 * nt + M::drow_g(g, r);
            if (col < a.n) {
                T* q = a.C + zp + (int64_t)col * a.ldc;
                const T v = a.alpha * acc[nt][r];
                *q = a.beta == T(0) ? v : v + a.beta * *q;      // beta == 0 never reads C
            }
        }
    }
}

// C (m x n) *= beta, beta == 0 stores zeros without reading: the whole result when alpha == 0 or nx == 0
template <typename T>
__global__ void rbf_scale_kernel(int64_t m, int64_t n, T beta, T* __restrict__ C, int64_t ldc) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= m * n) return;
    T* q = C + t % m + (t / m) * ldc;
    *q = beta == T(0) ? T(0) : beta * *q;
}

// C (mz x n) = alpha * (part[0] + part[1] + ... + part[g - 1]) + beta * C, the sum in that order; beta == 0 never reads C
template <typename T>
__global__ void rbf_reduce_kernel(int64_t mz, int64_t n, int64_t g, int64_t mzp, const T* __restrict__ part, T alpha, T beta, T* __restrict__ C,
                                  int64_t ldc) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= mz * n) return;
    const int64_t row = t % mz, col = t / mz;
    const T* p = part + col * mzp + row;
    const int64_t step = n * mzp;
    T s = p[0];
#pragma unroll 8
    for (int64_t b = 1; b < g; ++b) s += p[b * step];
    T* q = C + row + col * ldc;
    const T v = alpha * s;
    *q = beta == T(0) ? v : v + beta * *q;
}

// the split rule (include/rlhip.h), a function of the shape alone: the number of chunks, and in *ch the points of X per chunk -- a multiple
// of 64, hence of every staged tile length (nx when there is one chunk)
inline int64_t rbf_split_chunks(int64_t mz, int64_t nx, int64_t* ch) {
    *ch = nx;
    if (mz < 0 || nx < 0) return -1;
    if (mz == 0 || nx == 0) return 1;
    const int64_t ztiles = (mz + RBF_ZP - 1) / RBF_ZP;
    const int64_t by_work = (RLHIP_RBF_SPLIT_W + ztiles - 1) / ztiles, by_len = nx / RLHIP_RBF_SPLIT_CH_MIN;
    const int64_t g = by_work < by_len ? by_work : by_len;
    if (g < 2) return 1;
    *ch = 64 * ((nx + 64 * g - 1) / (64 * g));
    return (nx + *ch - 1) / *ch;      // no chunk is empty
}

template <typename T, int KS, int NT, bool MATERN, bool WEIGHT = false>
int launch_fused(rlhip_ctx* c, const RbfArgs<T>& a) {
    constexpr size_t bytes = 2 * (size_t)rbf_tile_elems<T, KS, NT>(rbf_tp<T, KS, NT>()) * sizeof(T);
    static_assert(bytes <= (size_t)RBF_LDS_CAP, "fused RBF kernel: the two staging buffers exceed the LDS budget");
    const int64_t wgs = (a.mz + RBF_ZP - 1) / RBF_ZP;
    if constexpr (WEIGHT) {
        hipLaunchKernelGGL((rbf_fused_kernel<T, KS, NT, true, false, true>), dim3((unsigned)wgs), dim3(RBF_WG), bytes, c->stream, a);
        RLHIP_LAUNCH_CHECK();
        return 0;
    }
    if (a.part) {      // split: a.ch points of X per workgroup, then the ordered sum of the partials
        const int64_t g = (a.nx + a.ch - 1) / a.ch;
        hipLaunchKernelGGL((rbf_fused_kernel<T, KS, NT, MATERN, true>), dim3((unsigned)wgs, (unsigned)g), dim3(RBF_WG), bytes, c->stream, a);
        RLHIP_LAUNCH_CHECK();
        hipLaunchKernelGGL(rbf_reduce_kernel<T>, dim3((unsigned)((a.mz * a.n + 255) / 256)), dim3(256), 0, c->stream, a.mz, a.n, g, a.mzp, a.part,
                           a.alpha, a.beta, a.C, a.ldc);
        RLHIP_LAUNCH_CHECK();
        return 0;
    }
    hipLaunchKernelGGL((rbf_fused_kernel<T, KS, NT, MATERN, false>), dim3((unsigned)wgs), dim3(RBF_WG), bytes, c->stream, a);
    RLHIP_LAUNCH_CHECK();
    return 0;
}
template <typename T, int KS, bool MATERN, bool WEIGHT = false>
int launch_fused_n(rlhip_ctx* c, const RbfArgs<T>& a) {
    if (a.n <= 16) return launch_fused<T, KS, 1, MATERN, WEIGHT>(c, a);
    if (a.n <= 32) return launch_fused<T, KS, 2, MATERN, WEIGHT>(c, a);
    return launch_fused<T, KS, 4, MATERN, WEIGHT>(c, a);
}
template <typename T, bool MATERN, bool WEIGHT = false>
int launch_fused_rows(rlhip_ctx* c, const RbfArgs<T>& a) {
    return rbf_ks_dispatch(a.rows_x, [&](auto ks) { return launch_fused_n<T, decltype(ks)::value, MATERN, WEIGHT>(c, a); });
}

// K (rows_k x cols_k, ldk) = K(Zb, Xb) for rows_k points Zb and cols_k points Xb with their norms: no argument checks, no counter
template <typename T>
int cross_block(rlhip_ctx* c, int64_t rows_x, int64_t rows_k, const T* Zb, int64_t ldz, const T* nz, int64_t cols_k, const T* Xb, int64_t ldx,
                const T* nx, PdkFn<T> f, T* K, int64_t ldk) {
    for (int64_t c0 = 0; c0 < cols_k; c0 += 65535) {      // the epilogue's grid has one column per blockIdx.y
        const int64_t cc = (cols_k - c0) < 65535 ? (cols_k - c0) : 65535;
        int rc = rlhip::gemm<T>(c, rlhip::Trans, rlhip::NoTrans, rows_k, cc, rows_x, T(-2), Zb, ldz, Xb + c0 * ldx, ldx, T(0), K + c0 * ldk, ldk);
        if (rc == 0) rc = rlhip::pdk_epilogue<T>(c, rows_k, cc, nz, nx + c0, f, K + c0 * ldk, ldk);
        if (rc) return rc;
    }
    return 0;
}

// The two routines below serve the squared-exponential entries (kernel = RLHIP_PDK_SQEXP, sh = 0) and the rlhip_pdk_* entries, whose argument
// lists have `kernel` in front of the bandwidth: sh = 1 moves the codes of the arguments from there on by one.
template <typename T>
int pdk_cross_submatrix(rlhip_ctx* c, int64_t rows_x, int64_t mz, const T* Z, int64_t ldz, const T* sq_colnorms_z, int64_t nx, const T* X,
                        int64_t ldx, const T* sq_colnorms_x, int64_t rows_k, int64_t cols_k, T* K, int64_t ldk, int64_t ro, int64_t co,
                        int kernel, int sh, T bandwidth) {
    if (!c) return -1;
    if (rows_x < 1) return -2;
    if (mz < 0) return -3;
    const bool work = rows_k > 0 && cols_k > 0;
    if (!Z && work) return -4;
    if (ldz < rows_x) return -5;
    if (nx < 0) return -7;
    if (!X && work) return -8;
    if (ldx < rows_x) return -9;
    if (rows_k < 0 || ro < 0 || ro + rows_k > mz) return -11;
    if (cols_k < 0 || co < 0 || co + cols_k > nx) return -12;
    if (!K && work) return -13;
    if (ldk < (rows_k > 1 ? rows_k : 1)) return -14;
    if (!rlhip::pdk_kind_ok(kernel)) return -17;
    if (!(bandwidth > T(0))) return -(17 + sh);
    c->rbf_path_count[2]++;
    if (!work) return 0;
    ws_scope ws(c);
    const T* nz = sq_colnorms_z ? sq_colnorms_z + ro : nullptr;
    const T* nxr = sq_colnorms_x ? sq_colnorms_x + co : nullptr;
    if (!nz) {
        T* tmp = ws.alloc<T>((size_t)rows_k);
        if (!tmp) return RLHIP_ERR_HIP(hipErrorOutOfMemory);
        const int rc = rlhip::sqexp_colnorms<T>(c, rows_x, rows_k, Z + ro * ldz, ldz, tmp);
        if (rc) return rc;
        nz = tmp;
    }
    if (!nxr) {
        T* tmp = ws.alloc<T>((size_t)cols_k);
        if (!tmp) return RLHIP_ERR_HIP(hipErrorOutOfMemory);
        const int rc = rlhip::sqexp_colnorms<T>(c, rows_x, cols_k, X + co * ldx, ldx, tmp);
        if (rc) return rc;
        nxr = tmp;
    }
    return cross_block<T>(c, rows_x, rows_k, Z + ro * ldz, ldz, nz, cols_k, X + co * ldx, ldx, nxr, rlhip::pdk_fn<T>(kernel, bandwidth), K, ldk);
}

template <typename T>
int pdk_cross_apply(rlhip_ctx* c, int64_t rows_x, int64_t mz, const T* Z, int64_t ldz, int64_t nx, const T* X, int64_t ldx, int kernel, int sh,
                    T bandwidth, int64_t n, T alpha, const T* B, int64_t ldb, T beta, T* C, int64_t ldc) {
    if (!c) return -1;
    if (rows_x < 1) return -2;
    if (mz < 0) return -3;
    const bool out = mz > 0 && n > 0;                          // C is written
    const bool product = out && nx > 0 && alpha != T(0);       // Z, X and B are read
    if (!Z && product) return -4;
    if (ldz < rows_x) return -5;
    if (nx < 0) return -6;
    if (!X && product) return -7;
    if (ldx < rows_x) return -8;
    if (!rlhip::pdk_kind_ok(kernel)) return -9;
    if (!(bandwidth > T(0))) return -(9 + sh);
    if (n < 0) return -(10 + sh);
    if (!B && product) return -(12 + sh);
    if (ldb < (nx > 1 ? nx : 1)) return -(13 + sh);
    if (!C && out) return -(15 + sh);
    if (ldc < (mz > 1 ? mz : 1)) return -(16 + sh);
    if (!out) return 0;
    if (!product) {
        if (beta != T(1)) {
            hipLaunchKernelGGL(rbf_scale_kernel<T>, dim3(grid1(mz * n, 256)), dim3(256), 0, c->stream, mz, n, beta, C, ldc);
            RLHIP_LAUNCH_CHECK();
        }
        return 0;
    }
    return rlhip::pdk_cross_apply_fn<T>(c, rows_x, mz, Z, ldz, nx, X, ldx, rlhip::pdk_fn<T>(kernel, bandwidth), n, alpha, B, ldb, beta, C, ldc);
}

}  // namespace

namespace rlhip {
template <typename T>
int pdk_cross_apply_fn(rlhip_ctx* c, int64_t rows_x, int64_t mz, const T* Z, int64_t ldz, int64_t nx, const T* X, int64_t ldx, PdkFn<T> f, int64_t n,
                       T alpha, const T* B, int64_t ldb, T beta, T* C, int64_t ldc) {
    const int64_t route = c->opt[RLHIP_OPT_RBF_FUSED];
    const bool fused = route != 0 && n <= RLHIP_RBF_FUSED_MAX_N && rows_x <= RLHIP_RBF_FUSED_MAX_ROWS_X;
    ws_scope ws(c);
    T* nr;                                                     // the fused route's whole scratch
    int rc = pdk_pair_norms<T>(c, ws, rows_x, mz, Z, ldz, nx, X, ldx, &nr);
    if (rc) return rc;
    if (fused) {
        c->rbf_path_count[0]++;
        RbfArgs<T> a{rows_x, mz, nx, n, Z, ldz, X, ldx, nr, nr + mz, B, ldb, C, ldc, alpha, beta, f.scale, f.third, nullptr, 0, 0};
        int64_t ch = nx;
        const int64_t g = route == 2 && !f.weight ? rbf_split_chunks(mz, nx, &ch) : 1;
        if (g > 1) {
            a.ch = ch;
            a.mzp = (mz + RBF_ZP - 1) / RBF_ZP * RBF_ZP;
            a.part = ws.alloc<T>((size_t)(g * a.n * a.mzp));
            if (!a.part) return RLHIP_ERR_HIP(hipErrorOutOfMemory);
            c->rbf_split_count++;
        }
        if (f.weight) return launch_fused_rows<T, true, true>(c, a);
        return f.matern ? launch_fused_rows<T, true>(c, a) : launch_fused_rows<T, false>(c, a);
    }
    c->rbf_path_count[1]++;
    const int64_t rb = pdk_row_block(nx, mz);                  // rows of a block of K
    T* Kb = ws.alloc<T>((size_t)(rb * nx));
    if (!Kb) return RLHIP_ERR_HIP(hipErrorOutOfMemory);
    for (int64_t r0 = 0; rc == 0 && r0 < mz; r0 += rb) {
        const int64_t rows = (mz - r0) < rb ? (mz - r0) : rb;
        rc = cross_block<T>(c, rows_x, rows, Z + r0 * ldz, ldz, nr + r0, nx, X, ldx, nr + mz, f, Kb, rows);
        if (rc == 0) rc = rlhip::gemm<T>(c, rlhip::NoTrans, rlhip::NoTrans, rows, n, nx, alpha, Kb, rows, B, ldb, beta, C + r0, ldc);
    }
    return rc;
}
template int pdk_cross_apply_fn<double>(rlhip_ctx*, int64_t, int64_t, const double*, int64_t, int64_t, const double*, int64_t, PdkFn<double>, int64_t,
                                        double, const double*, int64_t, double, double*, int64_t);
template int pdk_cross_apply_fn<float>(rlhip_ctx*, int64_t, int64_t, const float*, int64_t, int64_t, const float*, int64_t, PdkFn<float>, int64_t, float,
                                       const float*, int64_t, float, float*, int64_t);
}  // namespace rlhip

extern "C" {

int rlhip_sqexp_cross_submatrix_f64(rlhip_ctx* c, int64_t rows_x, int64_t mz, const double* Z, int64_t ldz, const double* sq_colnorms_z, int64_t nx,
                                    const double* X, int64_t ldx, const double* sq_colnorms_x, int64_t rows_ksub, int64_t cols_ksub, double* Ksub,
                                    int64_t ldk, int64_t ro_ksub, int64_t co_ksub, double bandwidth) {
    return pdk_cross_submatrix<double>(c, rows_x, mz, Z, ldz, sq_colnorms_z, nx, X, ldx, sq_colnorms_x, rows_ksub, cols_ksub, Ksub, ldk, ro_ksub, co_ksub,
                                    RLHIP_PDK_SQEXP, 0, bandwidth);
}
int rlhip_sqexp_cross_submatrix_f32(rlhip_ctx* c, int64_t rows_x, int64_t mz, const float* Z, int64_t ldz, const float* sq_colnorms_z, int64_t nx,
                                    const float* X, int64_t ldx, const float* sq_colnorms_x, int64_t rows_ksub, int64_t cols_ksub, float* Ksub,
                                    int64_t ldk, int64_t ro_ksub, int64_t co_ksub, float bandwidth) {
    return pdk_cross_submatrix<float>(c, rows_x, mz, Z, ldz, sq_colnorms_z, nx, X, ldx, sq_colnorms_x, rows_ksub, cols_ksub, Ksub, ldk, ro_ksub, co_ksub,
                                    RLHIP_PDK_SQEXP, 0, bandwidth);
}
int rlhip_rbf_cross_apply_f64(rlhip_ctx* c, int64_t rows_x, int64_t mz, const double* Z, int64_t ldz, int64_t nx, const double* X, int64_t ldx,
                              double bandwidth, int64_t n, double alpha, const double* B, int64_t ldb, double beta, double* C, int64_t ldc) {
    return pdk_cross_apply<double>(c, rows_x, mz, Z, ldz, nx, X, ldx, RLHIP_PDK_SQEXP, 0, bandwidth, n, alpha, B, ldb, beta, C, ldc);
}
int rlhip_rbf_cross_apply_f32(rlhip_ctx* c, int64_t rows_x, int64_t mz, const float* Z, int64_t ldz, int64_t nx, const float* X, int64_t ldx,
                              float bandwidth, int64_t n, float alpha, const float* B, int64_t ldb, float beta, float* C, int64_t ldc) {
    return pdk_cross_apply<float>(c, rows_x, mz, Z, ldz, nx, X, ldx, RLHIP_PDK_SQEXP, 0, bandwidth, n, alpha, B, ldb, beta, C, ldc);
}
// the same two routines with the kernel function as an argument
#define RLHIP_DEFINE_PDK_CROSS(SUF, T)                                                                                                            \
    int rlhip_pdk_cross_submatrix_##SUF(rlhip_ctx* c, int64_t rows_x, int64_t mz, const T* Z, int64_t ldz, const T* sq_colnorms_z, int64_t nx,    \
                                        const T* X, int64_t ldx, const T* sq_colnorms_x, int64_t rows_ksub, int64_t cols_ksub, T* Ksub,           \
                                        int64_t ldk, int64_t ro_ksub, int64_t co_ksub, int kernel, T bandwidth) {                                 \
        return pdk_cross_submatrix<T>(c, rows_x, mz, Z, ldz, sq_colnorms_z, nx, X, ldx, sq_colnorms_x, rows_ksub, cols_ksub, Ksub, ldk, ro_ksub,  \
                                      co_ksub, kernel, 1, bandwidth);                                                                             \
    }                                                                                                                                             \
    int rlhip_pdk_cross_apply_##SUF(rlhip_ctx* c, int64_t rows_x, int64_t mz, const T* Z, int64_t ldz, int64_t nx, const T* X, int64_t ldx,       \
                                    int kernel, T bandwidth, int64_t n, T alpha, const T* B, int64_t ldb, T beta, T* C, int64_t ldc) {            \
        return pdk_cross_apply<T>(c, rows_x, mz, Z, ldz, nx, X, ldx, kernel, 1, bandwidth, n, alpha, B, ldb, beta, C, ldc);                       \
    }
RLHIP_DEFINE_PDK_CROSS(f64, double)
RLHIP_DEFINE_PDK_CROSS(f32, float)
int64_t rlhip_rbf_split_count(rlhip_ctx* c) { return c ? c->rbf_split_count : -1; }
int64_t rlhip_rbf_split_chunks(int64_t mz, int64_t nx) {
    int64_t ch;
    return rbf_split_chunks(mz, nx, &ch);
}
int64_t rlhip_rbf_path_count(rlhip_ctx* c, int which) { return (c && which >= 55 && which <= 57) ? c->rbf_path_count[which - 55] : -1; }

}  // extern "C"
