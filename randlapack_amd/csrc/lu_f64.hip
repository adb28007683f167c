// fp64 panel step of the row-pivoted LU: the design of lu_f32.hip (rows published by the lanes of the owner's wave, per-wave decision,
// interchanges by row label, two workgroup barriers per column) with what fp64 changes:
//   * a value is two tagged words, so a row of 32 values is ONE store instruction of all 64 lanes (lane l <- word l);
//   * (|value|, row) do not fit one 64-bit key: the first maximum is found in two DPP reductions -- the maximal |value|, then the smallest
//     row among the lanes that hold it;
//   * 2 rows per thread (128 VGPRs of panel), 512 rows per workgroup, G <= 64 workgroups: up to 32768 rows below the diagonal (taller
//     panels keep the general step of lu.hip).
// BQRRP in fp64 (16384^2, b = 512) spends half its time in these panels (rl_bqrrp.hh:341-352); PLUL (rl_orth.hh:212-230) uses them too.
#include "rlhip_device.h"
#include "lu_common.h"

namespace rlhip_lu {
namespace {

using namespace rlhip_dev;   // dpp_mov

template <int N>   // max / min with the value N lanes to the right inside each 16-lane row (row_ror)
__device__ __forceinline__ double ld_dpp_max_step(double k) {
    const double o = dpp_mov<DPP_ROW_ROR + N>(k);
    return o > k ? o : k;
}
template <int N>
__device__ __forceinline__ unsigned ld_dpp_min_step(unsigned k) {
    const unsigned o = dpp_mov<DPP_ROW_ROR + N>(k);
    return o < k ? o : k;
}
// first maximum over the wave: (v, r) with v = -1 for "nothing to offer" (NaNs are offered as -1 too: LAPACK's strict '>' never selects them)
__device__ __forceinline__ void ld_wave_best(double& v, unsigned& r) {
    double k = v;
    k = ld_dpp_max_step<8>(k); k = ld_dpp_max_step<4>(k); k = ld_dpp_max_step<2>(k); k = ld_dpp_max_step<1>(k);
    const int lo = __double2loint(k), hi = __double2hiint(k);
    double vmax = -1.0;
#pragma unroll
    for (int l = 0; l < 64; l += 16) {
        const double t = __hiloint2double(__builtin_amdgcn_readlane(hi, l), __builtin_amdgcn_readlane(lo, l));
        vmax = t > vmax ? t : vmax;
    }
    unsigned rr = (v == vmax && vmax >= 0.0) ? r : 0xffffffffu;
    rr = ld_dpp_min_step<8>(rr); rr = ld_dpp_min_step<4>(rr); rr = ld_dpp_min_step<2>(rr); rr = ld_dpp_min_step<1>(rr);
    unsigned rmin = 0xffffffffu;
#pragma unroll
    for (int l = 0; l < 64; l += 16) {
        const unsigned t = (unsigned)__builtin_amdgcn_readlane((int)rr, l);
        rmin = t < rmin ? t : rmin;
    }
    v = vmax; r = rmin;
}

constexpr int LD_RPT = 2;                 // rows per thread: 512 rows per workgroup
struct LuF64Shared {
    unsigned rb[4][2 * PB];               // wave-private hand-over lines (owner lane -> the wave): word 2 c = low half of value c
    double bv[4]; unsigned br[4];
    double piv[2][PB];                    // by column parity
};

struct LuF64Step {   // (a type: lu_panel_steps<Step> calls Step::run<C> for every column)
    template <int C>
    static __device__ __forceinline__ void run(const LuArgs<double>& g, LuRegState<double, LD_RPT>& st, LuF64Shared& sh) {
        const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
        const int G = (int)gridDim.x, me = (int)blockIdx.x;
        const unsigned m = (unsigned)g.m;
        const unsigned j = (unsigned)g.j0 + C;
        constexpr int par = C & 1;
        const unsigned tag = g.tag_base + C + 1;
        unsigned long long* base = g.tw + (size_t)par * (size_t)(2 * G + G + 2 * G * PB + 2 * PB);
        unsigned long long* cw0 = base, *cw1 = cw0 + 2 * G, *rw = cw1 + G;
        LU_MARK(0)
        // ---- local candidate
        double bv = -1.0; unsigned br = 0xffffffffu;
#pragma unroll
        for (int q = 0; q < LD_RPT; ++q) {
            const unsigned r = (unsigned)st.gr[q];
            const double a = fabs(st.x[q][C]);
            if (r >= j && r < m && (a > bv || (a == bv && r < br))) { bv = a; br = r; }      // (a != a fails both tests)
        }
        ld_wave_best(bv, br);
        if (lane == 0) { sh.bv[wid] = bv; sh.br[wid] = br; }
        __syncthreads();
        {
            double v1 = sh.bv[0]; unsigned r1 = sh.br[0];
#pragma unroll
            for (int w = 1; w < 4; ++w) {
                const double v2 = sh.bv[w]; const unsigned r2 = sh.br[w];
                if (v2 > v1 || (v2 == v1 && r2 < r1)) { v1 = v2; r1 = r2; }
            }
            bv = v1; br = r1;
        }
        const unsigned lrow = (bv >= 0.0 && br < m) ? br : m;
        if (tid == 0) {
            const unsigned long long bits = (unsigned long long)__double_as_longlong(bv);
            lu_tag_put(cw0 + 2 * me, tag, (unsigned)bits); lu_tag_put(cw0 + 2 * me + 1, tag, (unsigned)(bits >> 32)); lu_tag_put(cw1 + me, tag, lrow);
        }
        if (lrow >= m) { if (tid < 2 * PB) lu_tag_put(rw + (size_t)me * 2 * PB + tid, tag, 0u); }     // nothing to offer: a dummy row, readers never wait for one
        else {
#pragma unroll
            for (int q = 0; q < LD_RPT; ++q) {
                const bool own = ((unsigned)st.gr[q] == lrow);
                if (__builtin_amdgcn_ballot_w64(own)) {                       // wave-uniform
                    if (own) {
#pragma unroll
                        for (int c2 = 0; c2 < PB; ++c2) {
                            sh.rb[wid][2 * c2] = (unsigned)__double2loint(st.x[q][c2]);
                            sh.rb[wid][2 * c2 + 1] = (unsigned)__double2hiint(st.x[q][c2]);
                        }
                    }
                    __builtin_amdgcn_s_waitcnt(0xc07f);                        // lgkmcnt(0): the line is written (same wave)
                    __builtin_amdgcn_wave_barrier();
                    lu_tag_put(rw + (size_t)me * 2 * PB + lane, tag, sh.rb[wid][lane]);
                    __builtin_amdgcn_wave_barrier();
                }
            }
        }
        LU_MARK(1)
        // ---- one batch of loads: record of workgroup `lane` (every wave reads all G <= 64 records) and element tid % 32 of the candidate
        //      rows of workgroups tid / 32 + 8 u
        constexpr int PF = 8, NWD = 3 + 2 * PF;
        const unsigned long long* ad[NWD]; bool need[NWD]; unsigned got[NWD];
        {
            const int wl = lane < G ? lane : 0;
            ad[0] = cw0 + 2 * wl; need[0] = lane < G;
            ad[1] = cw0 + 2 * wl + 1; need[1] = lane < G;
            ad[2] = cw1 + wl; need[2] = lane < G;
#pragma unroll
            for (int u = 0; u < PF; ++u) {
                const int wu = (tid >> 5) + 8 * u;
                const unsigned long long* q = rw + ((size_t)(wu < G ? wu : 0) * PB + (tid & 31)) * 2;
                ad[3 + 2 * u] = q; ad[4 + 2 * u] = q + 1;
                need[3 + 2 * u] = wu < G; need[4 + 2 * u] = wu < G;
            }
        }
        lu_tag_get_n<NWD>(ad, need, tag, got, g.info);
        LU_MARK(2)
        // ---- decision, per wave
        double gv = -1.0; unsigned gr = 0xffffffffu;
        if (lane < G && got[2] < m) { gv = __longlong_as_double((long long)(((unsigned long long)got[1] << 32) | got[0])); gr = got[2]; }
        const double myv = gv; const unsigned myr = gr;
        ld_wave_best(gv, gr);
        const bool any = (gv >= 0.0 && gr < m);
        const unsigned p = any ? gr : j;                                        // empty / NaN column: no exchange, (dummy) zero pivot row
        const unsigned long long whob = __builtin_amdgcn_ballot_w64(any && myv == gv && myr == gr);
        const int wstar = whob ? (int)__builtin_ctzll(whob) : 0;
        if ((tid >> 5) == (wstar & 7)) {
            unsigned lo = got[3], hi = got[4];
#pragma unroll
            for (int u = 1; u < PF; ++u) { const bool s = ((wstar >> 3) == u); lo = s ? got[3 + 2 * u] : lo; hi = s ? got[4 + 2 * u] : hi; }
            sh.piv[par][tid & 31] = __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
        }
        if (me == 0 && tid == 0) g.ipiv[j] = (int64_t)p + 1;
        __syncthreads();
        LU_MARK(3)
        // ---- interchange j <-> p by LABEL, then eliminate the rows below j.  (The same text in lu_f32.hip and lu_f64.hip: as one shared
        //      function template it gave both kernels another instruction schedule.)
        const double* s_piv = sh.piv[par];
        const double piv = s_piv[C];
        const double rp = 1.0 / piv;
#pragma unroll
        for (int q = 0; q < LD_RPT; ++q) {
            unsigned r = (unsigned)st.gr[q];
            if (p != j) { r = (r == j) ? p : (r == p) ? j : r; st.gr[q] = (int64_t)r; }
            if (piv != 0.0 && r > j && r < m) {
                const double l = st.x[q][C] * rp;
                st.x[q][C] = l;
#pragma unroll
                for (int c2 = C + 1; c2 < PB; ++c2) st.x[q][c2] -= l * s_piv[c2];
            }
        }
        if (piv == 0.0 && me == 0 && tid == 0 && *g.info == 0) *g.info = (int)(j + 1);
        LU_MARK(4)
    }
};
__global__ __launch_bounds__(256) void getrf_panel_f64_kernel(LuArgs<double> g) {
    __builtin_amdgcn_s_setprio(3);          // latency-bound: when a look-ahead runs this beside a GEMM on the same CUs, its waves issue first
    __shared__ LuF64Shared sh;
    LuRegState<double, LD_RPT> st;
    LU_PANEL_LOAD(double, LD_RPT, g, st)
    lu_panel_steps<LuF64Step>(g, st, sh);
    LU_PANEL_STORE(LD_RPT, g, st)
}

}  // namespace

void launch_getrf_panel_f64(const LuArgs<double>& g, unsigned G, hipStream_t stream) {
    hipLaunchKernelGGL(getrf_panel_f64_kernel, dim3(G), dim3(256), 0, stream, g);
}

}  // namespace rlhip_lu
