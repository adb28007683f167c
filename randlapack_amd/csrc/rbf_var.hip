// The predictive variance of restricted kernel ridge regression as a row-wise weighted quadratic form of the cross kernel:
//   t_i = K(Z(:, i), Xs) * G  (k numbers),   V(i, c) = max(0, 1 - sum_j t_ij^2) + sum_j e_jc t_ij^2,   e_jc = mu_c / (sigma_j^2 + mu_c)
//   rlhip_pdk_cross_var_*   Z rows_x x mz, Xs rows_x x k the centres, G k x k and sigma the basis of the fit, V mz x s
//       fused route    (opt-in: rlhip_pdk_var_set_fused(ctx, 1), and rlhip_pdk_var_fused(rows_x, k, s)): ONE launch beside the norms and the
//                      table of e; neither K nor t reaches memory; row i of V is a function of row i of the inputs alone, bit for bit;
//       composed route (the default, and every other shape): row blocks of t in the scratch arena by rlhip_pdk_cross_apply_*, sized as that
//                      routine sizes its own blocks, then one thread per row.  Its bits are those of the GEMMs behind the cross apply, which
//                      choose their kernels by the shape: no per-row bit contract here.
// Both routes evaluate a kernel entry by the cross apply's formula (rbf.hip) and take the squares and both sums in double.
//
// The fused kernel is rbf.hip's rbf_fused_kernel with NT = 4 and a loop of panels around its walk: a 256-thread workgroup owns 64 points of
// Z, 16 per wave, and lane (g, c) keeps the Z rows 4 kk + g of its wave's point c (times -2) in registers.  For panel P = columns
// [64 P, 64 P + 64) of G it walks the k centres in tiles of TP, staged in two LDS buffers with the matching TP x 64 tile of G and the TP
// norms; per sub-tile of 16 centres S^T by KS MFMAs, the kernel function in the accumulator registers, and the second product from those
// registers into acc[nt][r] = t(point c, column 64 P + 16 nt + drow_g(g, r)).  At the end of the panel the lane squares its 16 accumulators
// in double and adds them -- nt ascending, r ascending, so j ascending -- to u (unweighted) and to w[c] (times e_jc, read from the table);
// the accumulators start the next panel from zero.  After the last panel the four lane groups of a point are added in the order 0, 1, 2, 3
// (every lane forms the same sum from four shuffles) and lane group c mod 4 stores column c.  Centres past k and columns past k are staged
// as zeros: they add exp(.) * 0 = 0 to an accumulator, and a column past k keeps an accumulator of exactly 0.  The table of e has
// 64 ceil(k / 64) rows, zero behind k.  Nothing depends on mz or the grid: row i is a function of Z(:, i), Xs, G, sigma, mus, rcond.
#include <cmath>
#include "rlhip_internal.h"
#include "rlhip_device.h"

namespace {
using namespace rlhip_dev;
using rlhip::PdkFn;

constexpr int VAR_NT = 4;                               // accumulator tiles: a panel is 16 VAR_NT = 64 columns of G
constexpr int VAR_PANEL = 16 * VAR_NT;
constexpr int VAR_MAXS = RLHIP_PDK_VAR_FUSED_MAX_S;     // weighted sums a lane carries

template <typename T>
struct VarArgs {
    int64_t rows_x, mz, k, kp, s;      // kp = 64 ceil(k / 64): the rows of the table of e
    const T* Z; int64_t ldz;
    const T* X; int64_t ldx;
    const T* zn; const T* xn;          // |Z(:, i)|^2, |Xs(:, j)|^2
    const T* G; int64_t ldg;
    const double* E;                   // e_jc at E[j + c kp]
    T* V; int64_t ldv;
    T scale, third;                    // PdkFn's constants
};

// E[j + c kp] = e_jc for j < k, 0 for k <= j < kp; one thread per entry
template <typename T>
__global__ __launch_bounds__(256) void var_weights_kernel(int64_t k, int64_t kp, int64_t s, const T* __restrict__ sigma, const T* __restrict__ mus,
                                                          int64_t num_mus, T rcond, double* __restrict__ E) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= kp * s) return;
    const int64_t j = t % kp, c = t / kp;
    double e = 0.0;
    if (j < k) {
        const double cut = (double)rcond * (double)sigma[0];
        const double sg = (double)sigma[j], mu = (double)mus[num_mus == 1 ? 0 : c];
        e = mu == 0.0 ? (sg <= cut ? 1.0 : 0.0) : mu / fma(sg, sg, mu);
    }
    E[t] = e;
}

template <typename T>
__global__ __launch_bounds__(256) void var_ones_kernel(int64_t m, int64_t s, T* __restrict__ V, int64_t ldv) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < m * s) V[t % m + (t / m) * ldv] = T(1);
}

template <typename T, int KS, bool MATERN>
__global__ __launch_bounds__(RBF_WG) void pdk_var_fused_kernel(const VarArgs<T> a) {
    using M = Mfma16x4<T>;
    using acc_t = typename M::acc_t;
    constexpr int NT = VAR_NT;
    constexpr int TP = rbf_tp<T, KS, NT>();
    constexpr int XS = rbf_xs<T, KS>(), BSP = rbf_bsp(TP);
    constexpr int XE = TP * 4 * KS, BE = TP * 16 * NT;                        // staged elements of one tile
    constexpr int XPT = (XE + RBF_WG - 1) / RBF_WG, BPT = (BE + RBF_WG - 1) / RBF_WG;
    constexpr int BUF = rbf_tile_elems<T, KS, NT>(TP);
    extern __shared__ __align__(16) unsigned char var_lds_raw[];
    T* const lds = reinterpret_cast<T*>(var_lds_raw);

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

    double usum = 0.0, wsum[VAR_MAXS];
#pragma unroll
    for (int cc = 0; cc < VAR_MAXS; ++cc) wsum[cc] = 0.0;

    const int64_t ntiles = (a.k + TP - 1) / TP, npanels = (a.k + VAR_PANEL - 1) / VAR_PANEL;
    for (int64_t P = 0; P < npanels; ++P) {
        const int64_t col0 = P * VAR_PANEL;
        const T* const Gp = a.G + col0 * a.ldg;      // the panel's first column
        const int64_t ncol = a.k - col0;             // columns of G from col0 on (>= 1); the panel holds min(64, ncol) of them

        acc_t acc[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[nt] = acc_t{0, 0, 0, 0};

        T xpre[XPT], bpre[BPT], npre = T(0);
        auto fetch = [&](int64_t x0) {      // global -> registers; nothing past centre k - 1, row rows_x - 1 or column k - 1 of G is read
#pragma unroll
            for (int e = 0; e < XPT; ++e) {
                const int idx = tid + RBF_WG * e, p = idx / (4 * KS), r = idx % (4 * KS);
                xpre[e] = (idx < XE && x0 + p < a.k && r < a.rows_x) ? a.X[(x0 + p) * a.ldx + r] : T(0);
            }
#pragma unroll
            for (int e = 0; e < BPT; ++e) {
                const int idx = tid + RBF_WG * e, col = idx / TP, p = idx % TP;
                bpre[e] = (idx < BE && x0 + p < a.k && col < ncol) ? Gp[(x0 + p) + (int64_t)col * a.ldg] : T(0);
            }
            npre = (tid < TP && x0 + tid < a.k) ? a.xn[x0 + tid] : T(0);
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

        // every read of the previous panel's last tile lies in front of that panel's closing __syncthreads
        fetch(0);
        stash(lds);
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
                    if constexpr (MATERN) p[r] = matern_of_s(sq, a.scale, a.third);
                    else p[r] = rbf_exp(a.scale * sq);
                }
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    const T* bc = Bs + (16 * nt + c) * BSP + 16 * st;      // column 16 nt + c of the G tile, this sub-tile's centres
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

        // the panel's epilogue: squares in double, j = col0 + 16 nt + drow_g(g, r) ascending; j < kp always, and E is 0 behind k
        const double* const Ep = a.E + col0;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int jl = 16 * nt + M::drow_g(g, r);
                const double d = (double)acc[nt][r], q = d * d;
                usum += q;
#pragma unroll
                for (int cc = 0; cc < VAR_MAXS; ++cc)
                    if (cc < a.s) wsum[cc] += Ep[jl + cc * a.kp] * q;
            }
        }
    }

    // the four lane groups of a point in the order 0, 1, 2, 3: every lane of the wave takes part in the shuffles
    auto combine = [&](double v) {
        const double p0 = __shfl(v, c), p1 = __shfl(v, 16 + c), p2 = __shfl(v, 32 + c), p3 = __shfl(v, 48 + c);
        return ((p0 + p1) + p2) + p3;
    };
    double prior = 1.0 - combine(usum);
    prior = prior < 0.0 ? 0.0 : prior;      // a select: NaN stays NaN
#pragma unroll
    for (int cc = 0; cc < VAR_MAXS; ++cc) {
        if (cc < a.s) {
            const double wt = combine(wsum[cc]);
            if (zok && (cc & 3) == g) a.V[zp + (int64_t)cc * a.ldv] = (T)(prior + wt);
        }
    }
}

// the composed route's second step: one thread per row of t (rows x k, ldt), j ascending, VAR_MAXS regularizations per pass over the row
template <typename T>
__global__ __launch_bounds__(256) void var_rows_kernel(int64_t rows, int64_t k, int64_t kp, int64_t s, const T* __restrict__ t, int64_t ldt,
                                                       const double* __restrict__ E, T* __restrict__ V, int64_t ldv) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    for (int64_t c0 = 0; c0 < s; c0 += VAR_MAXS) {
        double usum = 0.0, wsum[VAR_MAXS];
#pragma unroll
        for (int cc = 0; cc < VAR_MAXS; ++cc) wsum[cc] = 0.0;
#pragma unroll 8
        for (int64_t j = 0; j < k; ++j) {      // unrolled for loads in flight; the additions stay in the order of j
            const double d = (double)t[i + j * ldt], q = d * d;
            usum += q;
#pragma unroll
            for (int cc = 0; cc < VAR_MAXS; ++cc)
                if (c0 + cc < s) wsum[cc] += E[j + (c0 + cc) * kp] * q;
        }
        double prior = 1.0 - usum;
        prior = prior < 0.0 ? 0.0 : prior;
#pragma unroll
        for (int cc = 0; cc < VAR_MAXS; ++cc)
            if (c0 + cc < s) V[i + (c0 + cc) * ldv] = (T)(prior + wsum[cc]);
    }
}

template <typename T, int KS, bool MATERN>
int launch_var(rlhip_ctx* c, const VarArgs<T>& a) {
    constexpr size_t bytes = 2 * (size_t)rbf_tile_elems<T, KS, VAR_NT>(rbf_tp<T, KS, VAR_NT>()) * sizeof(T);
    static_assert(bytes <= (size_t)RBF_LDS_CAP, "fused variance kernel: the two staging buffers exceed the LDS budget");
    const int64_t wgs = (a.mz + RBF_ZP - 1) / RBF_ZP;
    hipLaunchKernelGGL((pdk_var_fused_kernel<T, KS, MATERN>), dim3((unsigned)wgs), dim3(RBF_WG), bytes, c->stream, a);
    RLHIP_LAUNCH_CHECK();
    return 0;
}
template <typename T, bool MATERN>
int launch_var_rows(rlhip_ctx* c, const VarArgs<T>& a) {
    return rbf_ks_dispatch(a.rows_x, [&](auto ks) { return launch_var<T, decltype(ks)::value, MATERN>(c, a); });
}

inline int cross_apply(rlhip_ctx* c, int64_t rows_x, int64_t mz, const double* Z, int64_t ldz, int64_t nx, const double* X, int64_t ldx, int kernel,
                       double bandwidth, int64_t n, const double* B, int64_t ldb, double* C, int64_t ldc) {
    return rlhip_pdk_cross_apply_f64(c, rows_x, mz, Z, ldz, nx, X, ldx, kernel, bandwidth, n, 1.0, B, ldb, 0.0, C, ldc);
}
inline int cross_apply(rlhip_ctx* c, int64_t rows_x, int64_t mz, const float* Z, int64_t ldz, int64_t nx, const float* X, int64_t ldx, int kernel,
                       float bandwidth, int64_t n, const float* B, int64_t ldb, float* C, int64_t ldc) {
    return rlhip_pdk_cross_apply_f32(c, rows_x, mz, Z, ldz, nx, X, ldx, kernel, bandwidth, n, 1.0f, B, ldb, 0.0f, C, ldc);
}

// the shape rule of the fused route (include/rlhip.h)
inline bool var_fused_shape(int64_t rows_x, int64_t k, int64_t s) {
    return rows_x >= 1 && rows_x <= RLHIP_RBF_FUSED_MAX_ROWS_X && k >= 1 && s >= 1 && s <= VAR_MAXS;
}

template <typename T>
int pdk_cross_var(rlhip_ctx* c, int64_t rows_x, int64_t mz, const T* Z, int64_t ldz, int64_t k, const T* Xs, int64_t ldx, int kernel, T bandwidth,
                  const T* G, int64_t ldg, const T* sigma, int64_t s, const T* mus, int64_t num_mus, T rcond, T* V, int64_t ldv) {
    if (!c) return -1;
    if (rows_x < 1) return -2;
    if (mz < 0) return -3;
    if (ldz < rows_x) return -5;
    if (k < 0) return -6;
    if (ldx < rows_x) return -8;
    if (!rlhip::pdk_kind_ok(kernel)) return -9;
    if (!(bandwidth > T(0))) return -10;
    if (ldg < (k > 1 ? k : 1)) return -12;
    if (s < 0) return -14;
    if (ldv < (mz > 1 ? mz : 1)) return -19;
    if (mz == 0 || s == 0) return 0;
    if (num_mus != 1 && num_mus != s) return -100;
    if (!(rcond >= T(0))) return -17;
    if (!V) return -18;
    if (k == 0) {      // no centre: the prior variance
        hipLaunchKernelGGL(var_ones_kernel<T>, dim3(grid1(mz * s, 256)), dim3(256), 0, c->stream, mz, s, V, ldv);
        RLHIP_LAUNCH_CHECK();
        return 0;
    }
    if (!Z) return -4;
    if (!Xs) return -7;
    if (!G) return -11;
    if (!sigma) return -13;
    if (!mus) return -15;

    const int64_t kp = (k + VAR_PANEL - 1) / VAR_PANEL * VAR_PANEL;
    const PdkFn<T> f = rlhip::pdk_fn<T>(kernel, bandwidth);
    ws_scope ws(c);
    double* E = ws.alloc<double>((size_t)(kp * s));
    if (!E) return RLHIP_ERR_HIP(hipErrorOutOfMemory);
    hipLaunchKernelGGL(var_weights_kernel<T>, dim3(grid1(kp * s, 256)), dim3(256), 0, c->stream, k, kp, s, sigma, mus, num_mus, rcond, E);
    RLHIP_LAUNCH_CHECK();

    // the fused kernel is opt-in: it measured slower than the product-based route on every shape of DESIGN 4.27
    if (c->var_fused && var_fused_shape(rows_x, k, s)) {
        c->var_path_count[0]++;
        T* nr;
        const int rc = rlhip::pdk_pair_norms<T>(c, ws, rows_x, mz, Z, ldz, k, Xs, ldx, &nr);
        if (rc) return rc;
        const VarArgs<T> a{rows_x, mz, k, kp, s, Z, ldz, Xs, ldx, nr, nr + mz, G, ldg, E, V, ldv, f.scale, f.third};
        return f.matern ? launch_var_rows<T, true>(c, a) : launch_var_rows<T, false>(c, a);
    }
    c->var_path_count[1]++;
    const int64_t rb = rlhip::pdk_row_block(k, mz);            // rows of a block of t, as the cross apply sizes its block of K
    T* tb = ws.alloc<T>((size_t)(rb * k));
    if (!tb) return RLHIP_ERR_HIP(hipErrorOutOfMemory);
    int rc = 0;
    for (int64_t r0 = 0; rc == 0 && r0 < mz; r0 += rb) {
        const int64_t rows = (mz - r0) < rb ? (mz - r0) : rb;
        rc = cross_apply(c, rows_x, rows, Z + r0 * ldz, ldz, k, Xs, ldx, kernel, bandwidth, k, G, ldg, tb, rows);
        if (rc) break;
        hipLaunchKernelGGL(var_rows_kernel<T>, dim3(grid1(rows, 256)), dim3(256), 0, c->stream, rows, k, kp, s, tb, rows, E, V + r0, ldv);
        RLHIP_LAUNCH_CHECK();
    }
    return rc;
}

}  // namespace

extern "C" {

int rlhip_pdk_cross_var_f64(rlhip_ctx* c, int64_t rows_x, int64_t mz, const double* Z, int64_t ldz, int64_t k, const double* Xs, int64_t ldx,
                            int kernel, double bandwidth, const double* G, int64_t ldg, const double* sigma_dev, int64_t s, const double* mus_dev,
                            int64_t num_mus, double rcond, double* V, int64_t ldv) {
    return pdk_cross_var<double>(c, rows_x, mz, Z, ldz, k, Xs, ldx, kernel, bandwidth, G, ldg, sigma_dev, s, mus_dev, num_mus, rcond, V, ldv);
}
int rlhip_pdk_cross_var_f32(rlhip_ctx* c, int64_t rows_x, int64_t mz, const float* Z, int64_t ldz, int64_t k, const float* Xs, int64_t ldx,
                            int kernel, float bandwidth, const float* G, int64_t ldg, const float* sigma_dev, int64_t s, const float* mus_dev,
                            int64_t num_mus, float rcond, float* V, int64_t ldv) {
    return pdk_cross_var<float>(c, rows_x, mz, Z, ldz, k, Xs, ldx, kernel, bandwidth, G, ldg, sigma_dev, s, mus_dev, num_mus, rcond, V, ldv);
}
int rlhip_pdk_var_fused(int64_t rows_x, int64_t k, int64_t s) { return var_fused_shape(rows_x, k, s) ? 1 : 0; }
int rlhip_pdk_var_set_fused(rlhip_ctx* c, int on) {
    if (!c) return -1;
    const int was = c->var_fused;
    c->var_fused = on != 0;
    return was;
}
int64_t rlhip_pdk_var_path_count(rlhip_ctx* c, int which) { return (c && which >= 58 && which <= 59) ? c->var_path_count[which - 58] : -1; }

}  // extern "C"
