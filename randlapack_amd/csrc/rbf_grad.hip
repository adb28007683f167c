// The gradient of a kernel expansion with respect to the evaluation point:
//   G(:, r mz + i) = alpha * sum_j w(s_ij) (Z(:, i) - X(:, j)) B(j, r),   s_ij = |Z(:, i) - X(:, j)|^2,   w = 2 dk/ds = w(0) u(s)
//   rlhip_pdk_cross_grad_*   Z rows_x x mz, X rows_x x nx, B nx x n, G rows_x x (mz n), laid out like Z per right-hand side
// Coordinate c is z_c (U B) - U (x_c o B) with U = u(s): a cross apply with d + 1 = rows_x + 1 columns per right-hand side,
//   B' = [B(:, r), x_1 o B(:, r), ..., x_d o B(:, r)]_r   (column r (d + 1) + cc),   T = U B',
//   G(c, r mz + i) = alpha * (w(0) * fma(z_c, T(i, r (d + 1)), -T(i, r (d + 1) + 1 + c))).
//       composed route (the default): B' in the scratch arena, rbf.hip's cross apply with the weight form of the kernel function
//                      (rlhip::pdk_cross_apply_fn; it picks its own fused or row-block route) into row blocks of T, one thread per entry of G;
//       fused route    (opt-in: rlhip_pdk_grad_set_fused(ctx, 1), and rlhip_pdk_grad_fused(rows_x, n)): ONE launch beside the norms; neither
//                      B' nor T reaches memory; column r mz + i of G is a function of Z(:, i), X, B and alpha alone, bit for bit.
// Both routes form an entry of B' as one product in T and an entry of U by the cross apply's formula with pdk_weight_of_s (rlhip_device.h);
// they differ in the order of the sums over j only.
//
// The fused kernel is rbf.hip's rbf_fused_kernel with another second operand: a 256-thread workgroup owns 64 points of Z, 16 per wave, and
// lane (g, c) keeps the Z rows 4 kk + g of its wave's point c (times -2) in registers.  X is walked in tiles of TP points; a tile of X, the
// TP norms and the TP x n tile of B are staged in LDS (X and the norms in two buffers, the raw B tile in one), and after a barrier the
// workgroup forms the tile of B' ([column][point], the cross apply's layout of its B tile) from the staged X and B: one product per entry,
// columns past n (d + 1) and points past nx zero.  Per sub-tile of 16 points S^T by KS MFMAs, u in the accumulator registers, and the
// second product from those registers into acc[nt][r] = T(point c, column 16 nt + drow_g(g, r)).  The epilogue passes the accumulators
// through LDS ([column][point]) so that one thread holds T_0 and T_c of an entry of G, and stores G with the coordinate running fastest.
#include <cmath>
#include "rlhip_internal.h"
#include "rlhip_device.h"

namespace {
using namespace rlhip_dev;
using rlhip::PdkFn;

template <typename T>
struct GradArgs {
    int64_t rows_x, mz, nx, n;
    const T* Z; int64_t ldz;
    const T* X; int64_t ldx;
    const T* zn; const T* xn;      // |Z(:, i)|^2, |X(:, j)|^2
    const T* B; int64_t ldb;
    T* G; int64_t ldg;
    T alpha, w0, scale, lin;       // w0 = w(0); scale, lin: the weight form's constants (pdk_weight_fn)
};

// staged elements: two buffers of the cross apply's tile (X, B', norms) and one raw tile of B, at most 8 NT columns (n (d + 1) <= 16 NT, d >= 1)
constexpr int GRAD_TS = RBF_ZP + 1;      // stride of the epilogue's T tile [column][point]
template <typename T, int KS, int NT> constexpr int grad_stage_elems(int tp) { return 2 * rbf_tile_elems<T, KS, NT>(tp) + 8 * NT * tp; }
template <typename T, int KS, int NT> constexpr int grad_tp() {
    return grad_stage_elems<T, KS, NT>(64) * (int)sizeof(T) <= RBF_LDS_CAP ? 64 : (grad_stage_elems<T, KS, NT>(32) * (int)sizeof(T) <= RBF_LDS_CAP ? 32 : 16);
}
template <typename T, int KS, int NT> constexpr int grad_lds_elems() {
    return grad_stage_elems<T, KS, NT>(grad_tp<T, KS, NT>()) > 16 * NT * GRAD_TS ? grad_stage_elems<T, KS, NT>(grad_tp<T, KS, NT>()) : 16 * NT * GRAD_TS;
}

template <typename T, int KS, int NT, bool MATERN>
__global__ __launch_bounds__(RBF_WG) void pdk_grad_fused_kernel(const GradArgs<T> a) {
    using M = Mfma16x4<T>;
    using acc_t = typename M::acc_t;
    constexpr int TP = grad_tp<T, KS, NT>();
    constexpr int XS = rbf_xs<T, KS>(), BSP = rbf_bsp(TP);
    constexpr int XE = TP * 4 * KS, BE = TP * 16 * NT, RE = TP * 8 * NT;      // staged X, formed B', staged raw B
    constexpr int XPT = (XE + RBF_WG - 1) / RBF_WG, BPT = (BE + RBF_WG - 1) / RBF_WG, RPT = (RE + RBF_WG - 1) / RBF_WG;
    constexpr int BUF = rbf_tile_elems<T, KS, NT>(TP);
    extern __shared__ __align__(16) unsigned char grad_lds_raw[];
    T* const lds = reinterpret_cast<T*>(grad_lds_raw);
    T* const Br = lds + 2 * BUF;      // raw B tile [column][point], stride TP

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, c = lane & 15;
    const int64_t zp = (int64_t)blockIdx.x * RBF_ZP + 16 * w + c;
    const bool zok = zp < a.mz;
    const int d1 = (int)a.rows_x + 1, ncols = (int)a.n * d1;

    T zreg[KS];
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) {
        const int row = 4 * kk + g;
        zreg[kk] = (zok && row < a.rows_x) ? T(-2) * a.Z[zp * a.ldz + row] : T(0);
    }
    const T znorm = zok ? a.zn[zp] : T(0);

    // the entries of B' this thread forms are the same in every tile: column q = r d1 + cc as (r << 8) | cc, -1 past the last column
    int pk[BPT];
#pragma unroll
    for (int e = 0; e < BPT; ++e) {
        const int q = (tid + RBF_WG * e) / TP;
        pk[e] = q < ncols ? (((q / d1) << 8) | (q % d1)) : -1;
    }

    acc_t acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[nt] = acc_t{0, 0, 0, 0};

    T xpre[XPT], bpre[RPT], npre = T(0);
    auto fetch = [&](int64_t x0) {      // global -> registers; nothing past point nx - 1, row rows_x - 1 or column n - 1 is read
#pragma unroll
        for (int e = 0; e < XPT; ++e) {
            const int idx = tid + RBF_WG * e, p = idx / (4 * KS), r = idx % (4 * KS);
            xpre[e] = (idx < XE && x0 + p < a.nx && r < a.rows_x) ? a.X[(x0 + p) * a.ldx + r] : T(0);
        }
#pragma unroll
        for (int e = 0; e < RPT; ++e) {
            const int idx = tid + RBF_WG * e, col = idx / TP, p = idx % TP;
            bpre[e] = (idx < RE && x0 + p < a.nx && col < a.n) ? a.B[(x0 + p) + (int64_t)col * a.ldb] : T(0);
        }
        npre = (tid < TP && x0 + tid < a.nx) ? a.xn[x0 + tid] : T(0);
    };
    auto stash = [&](T* buf) {          // registers -> LDS: X and the norms of the tile, the raw B tile
        T* Xs = buf; T* Ns = buf + TP * XS + 16 * NT * BSP;
#pragma unroll
        for (int e = 0; e < XPT; ++e) {
            const int idx = tid + RBF_WG * e;
            if (idx < XE) Xs[(idx / (4 * KS)) * XS + idx % (4 * KS)] = xpre[e];
        }
#pragma unroll
        for (int e = 0; e < RPT; ++e) {
            const int idx = tid + RBF_WG * e;
            if (idx < RE) Br[idx] = bpre[e];
        }
        if (tid < TP) Ns[tid] = npre;
    };
    auto form = [&](T* buf) {           // B' of the tile from its staged X and B; behind the barrier that follows stash
        const T* Xs = buf; T* Bs = buf + TP * XS;
#pragma unroll
        for (int e = 0; e < BPT; ++e) {
            const int idx = tid + RBF_WG * e;
            if (idx < BE) {
                const int p = idx % TP, r = pk[e] >> 8, cc = pk[e] & 255;
                T v = T(0);
                if (pk[e] >= 0) {
                    v = Br[r * TP + p];
                    if (cc) v = v * Xs[p * XS + cc - 1];
                }
                Bs[(idx / TP) * BSP + p] = v;
            }
        }
    };

    const int64_t ntiles = (a.nx + TP - 1) / TP;
    fetch(0);
    stash(lds);
    __syncthreads();
    form(lds);
    __syncthreads();
    for (int64_t t = 0; t < ntiles; ++t) {
        const T* buf = lds + (t & 1) * BUF;
        const T* Xs = buf; const T* Bs = buf + TP * XS; const T* Ns = Bs + 16 * NT * BSP;
        const bool more = t + 1 < ntiles;
        if (more) fetch((t + 1) * TP);

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
                if constexpr (MATERN) p[r] = pdk_weight_of_s(sq, a.scale, a.lin);
                else p[r] = rbf_exp(a.scale * sq);
            }
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const T* bc = Bs + (16 * nt + c) * BSP + 16 * st;      // column 16 nt + c of the B' tile, this sub-tile's points
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
        if (more) {      // the raw B tile was last read by the form of this tile, in front of a barrier
            stash(lds + ((t + 1) & 1) * BUF);
            __syncthreads();
            form(lds + ((t + 1) & 1) * BUF);
        }
        __syncthreads();
    }

    // epilogue: every read of the staged tiles lies in front of the loop's last barrier.  T(point, column) -> LDS [column][point]
    T* const Tl = lds;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) Tl[(16 * nt + M::drow_g(g, r)) * GRAD_TS + 16 * w + c] = acc[nt][r];
    }
    __syncthreads();
    const int d = (int)a.rows_x, total = RBF_ZP * (int)a.n * d;      // <= 64 * 64
    const T aw = a.w0;
    for (int o = tid; o < total; o += RBF_WG) {                      // coordinate fastest: consecutive threads store consecutive entries of G
        const int cc = o % d, t2 = o / d, pt = t2 & (RBF_ZP - 1), r = t2 / RBF_ZP;
        const int64_t zi = (int64_t)blockIdx.x * RBF_ZP + pt;
        if (zi < a.mz) {
            const T t0 = Tl[(r * d1) * GRAD_TS + pt], tc = Tl[(r * d1 + 1 + cc) * GRAD_TS + pt];
            a.G[((int64_t)r * a.mz + zi) * a.ldg + cc] = a.alpha * (aw * pdk_fma(a.Z[zi * a.ldz + cc], t0, -tc));
        }
    }
}

// ---- the composed route's kernels, one thread per entry
// Bp (nx x n d1, ld nx): column r d1 of it is B(:, r), column r d1 + 1 + c is X(c, :)^T o B(:, r)
template <typename T>
__global__ __launch_bounds__(256) void grad_bprime_kernel(int64_t d1, int64_t nx, int64_t n, const T* __restrict__ X, int64_t ldx, const T* __restrict__ B,
                                                          int64_t ldb, T* __restrict__ Bp) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nx * n * d1) return;
    const int64_t j = t % nx, q = t / nx, r = q / d1, cc = q % d1;
    const T b = B[j + r * ldb];
    Bp[t] = cc ? b * X[j * ldx + cc - 1] : b;
}
// G of the points [r0, r0 + rows) from their block of T (rows x n d1, ld rows); the coordinate runs fastest
template <typename T>
__global__ __launch_bounds__(256) void grad_combine_kernel(int64_t d, int64_t mz, int64_t r0, int64_t rows, int64_t n, const T* __restrict__ Z, int64_t ldz,
                                                           const T* __restrict__ Tm, T alpha, T w0, T* __restrict__ G, int64_t ldg) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= d * rows * n) return;
    const int64_t cc = t % d, t2 = t / d, i = t2 % rows, r = t2 / rows, d1 = d + 1;
    const T t0 = Tm[i + (r * d1) * rows], tc = Tm[i + (r * d1 + 1 + cc) * rows];
    G[(r * mz + r0 + i) * ldg + cc] = alpha * (w0 * pdk_fma(Z[(r0 + i) * ldz + cc], t0, -tc));
}
template <typename T>
__global__ __launch_bounds__(256) void grad_zero_kernel(int64_t d, int64_t cols, T* __restrict__ G, int64_t ldg) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < d * cols) G[(t / d) * ldg + t % d] = T(0);
}

template <typename T, int KS, int NT, bool MATERN>
int launch_grad(rlhip_ctx* c, const GradArgs<T>& a) {
    constexpr size_t bytes = (size_t)grad_lds_elems<T, KS, NT>() * sizeof(T);
    static_assert(bytes <= (size_t)RBF_LDS_CAP, "fused gradient kernel: the staging buffers exceed the LDS budget");
    const int64_t wgs = (a.mz + RBF_ZP - 1) / RBF_ZP;
    hipLaunchKernelGGL((pdk_grad_fused_kernel<T, KS, NT, MATERN>), dim3((unsigned)wgs), dim3(RBF_WG), bytes, c->stream, a);
    RLHIP_LAUNCH_CHECK();
    return 0;
}
template <typename T, int KS, bool MATERN>
int launch_grad_n(rlhip_ctx* c, const GradArgs<T>& a) {
    const int64_t ncols = a.n * (a.rows_x + 1);
    if (ncols <= 16) return launch_grad<T, KS, 1, MATERN>(c, a);
    if (ncols <= 32) return launch_grad<T, KS, 2, MATERN>(c, a);
    return launch_grad<T, KS, 4, MATERN>(c, a);
}
template <typename T, bool MATERN>
int launch_grad_rows(rlhip_ctx* c, const GradArgs<T>& a) {      // n (rows_x + 1) <= 64 leaves rows_x <= 63: KS stops at 16
    return rbf_ks_dispatch<16>(a.rows_x, [&](auto ks) { return launch_grad_n<T, decltype(ks)::value, MATERN>(c, a); });
}

// the shape rule of the fused route (include/rlhip.h)
inline bool grad_fused_shape(int64_t rows_x, int64_t n) {
    return rows_x >= 1 && rows_x <= RLHIP_RBF_FUSED_MAX_ROWS_X && n >= 1 && n <= RLHIP_PDK_GRAD_FUSED_MAX_COLS &&
           n * (rows_x + 1) <= RLHIP_PDK_GRAD_FUSED_MAX_COLS;
}

template <typename T>
int pdk_cross_grad(rlhip_ctx* c, int64_t rows_x, int64_t mz, const T* Z, int64_t ldz, int64_t nx, const T* X, int64_t ldx, int kernel, T bandwidth,
                   int64_t n, T alpha, const T* B, int64_t ldb, T* G, int64_t ldg) {
    if (!c) return -1;
    if (rows_x < 1) return -2;
    if (mz < 0) return -3;
    const bool out = mz > 0 && n > 0;                          // G is written
    const bool product = out && nx > 0 && alpha != T(0);       // Z, X and B are read
    if (!Z && product) return -4;
    if (ldz < rows_x) return -5;
    if (nx < 0) return -6;
    if (!X && product) return -7;
    if (ldx < rows_x) return -8;
    if (!rlhip::pdk_kind_ok(kernel)) return -9;
    if (!(bandwidth > T(0))) return -10;
    if (n < 0) return -11;
    if (!B && product) return -13;
    if (ldb < (nx > 1 ? nx : 1)) return -14;
    if (!G && out) return -15;
    if (ldg < rows_x) return -16;
    if (!out) return 0;
    if (!product) {
        hipLaunchKernelGGL(grad_zero_kernel<T>, dim3(grid1(rows_x * mz * n, 256)), dim3(256), 0, c->stream, rows_x, mz * n, G, ldg);
        RLHIP_LAUNCH_CHECK();
        return 0;
    }
    T w0;
    const PdkFn<T> f = rlhip::pdk_weight_fn<T>(kernel, bandwidth, &w0);
    ws_scope ws(c);
    // the fused kernel is opt-in: DESIGN 4.30 has the measurements behind the default
    if (c->grad_fused && grad_fused_shape(rows_x, n)) {
        c->grad_path_count[0]++;
        T* nr;
        const int rc = rlhip::pdk_pair_norms<T>(c, ws, rows_x, mz, Z, ldz, nx, X, ldx, &nr);
        if (rc) return rc;
        const GradArgs<T> a{rows_x, mz, nx, n, Z, ldz, X, ldx, nr, nr + mz, B, ldb, G, ldg, alpha, w0, f.scale, f.third};
        return f.matern ? launch_grad_rows<T, true>(c, a) : launch_grad_rows<T, false>(c, a);
    }
    c->grad_path_count[1]++;
    const int64_t d1 = rows_x + 1, ncols = n * d1;
    T* Bp = ws.alloc<T>((size_t)(nx * ncols));
    if (!Bp) return RLHIP_ERR_HIP(hipErrorOutOfMemory);
    hipLaunchKernelGGL(grad_bprime_kernel<T>, dim3(grid1(nx * ncols, 256)), dim3(256), 0, c->stream, d1, nx, n, X, ldx, B, ldb, Bp);
    RLHIP_LAUNCH_CHECK();
    const int64_t rb = rlhip::pdk_row_block(ncols, mz);        // rows of a block of T
    T* Tm = ws.alloc<T>((size_t)(rb * ncols));
    if (!Tm) return RLHIP_ERR_HIP(hipErrorOutOfMemory);
    for (int64_t r0 = 0; r0 < mz; r0 += rb) {
        const int64_t rows = (mz - r0) < rb ? (mz - r0) : rb;
        const int rc = rlhip::pdk_cross_apply_fn<T>(c, rows_x, rows, Z + r0 * ldz, ldz, nx, X, ldx, f, ncols, T(1), Bp, nx, T(0), Tm, rows);
        if (rc) return rc;
        hipLaunchKernelGGL(grad_combine_kernel<T>, dim3(grid1(rows_x * rows * n, 256)), dim3(256), 0, c->stream, rows_x, mz, r0, rows, n, Z, ldz, Tm,
                           alpha, w0, G, ldg);
        RLHIP_LAUNCH_CHECK();
    }
    return 0;
}

}  // namespace

extern "C" {

int rlhip_pdk_cross_grad_f64(rlhip_ctx* c, int64_t rows_x, int64_t mz, const double* Z, int64_t ldz, int64_t nx, const double* X, int64_t ldx,
                             int kernel, double bandwidth, int64_t n, double alpha, const double* B, int64_t ldb, double* G, int64_t ldg) {
    return pdk_cross_grad<double>(c, rows_x, mz, Z, ldz, nx, X, ldx, kernel, bandwidth, n, alpha, B, ldb, G, ldg);
}
int rlhip_pdk_cross_grad_f32(rlhip_ctx* c, int64_t rows_x, int64_t mz, const float* Z, int64_t ldz, int64_t nx, const float* X, int64_t ldx,
                             int kernel, float bandwidth, int64_t n, float alpha, const float* B, int64_t ldb, float* G, int64_t ldg) {
    return pdk_cross_grad<float>(c, rows_x, mz, Z, ldz, nx, X, ldx, kernel, bandwidth, n, alpha, B, ldb, G, ldg);
}
int rlhip_pdk_grad_fused(int64_t rows_x, int64_t n) { return grad_fused_shape(rows_x, n) ? 1 : 0; }
int rlhip_pdk_grad_set_fused(rlhip_ctx* c, int on) {
    if (!c) return -1;
    const int was = c->grad_fused;
    c->grad_fused = on != 0;
    return was;
}
int64_t rlhip_pdk_grad_path_count(rlhip_ctx* c, int which) { return (c && which >= 74 && which <= 75) ? c->grad_path_count[which - 74] : -1; }

}  // extern "C"
