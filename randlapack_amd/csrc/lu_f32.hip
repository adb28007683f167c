// fp32 panel step of the row-pivoted LU (see lu.hip for the algorithm and the host driver, lu_common.h for the shared pieces)
#include "rlhip_device.h"
#include "lu_common.h"

namespace rlhip_lu {
namespace {

using namespace rlhip_dev;   // dpp_mov

// ---- fp32 panels of up to 65536 rows (BQRRP's transposed sketch, rl_bqrrp.hh:341-352): the column step rewritten around what the per-phase
// profile of the general step showed (us per column at 65536 x 2048: candidate 1.2, publish 1.3, exchange 1.8, decision 1.1, eliminate
// 1.7 -- the hand-off itself is a quarter; the rest is LOCAL work with one workgroup per CU and nothing to hide latencies behind):
//   * a row is published by 32 lanes with ONE store instruction (the owner lane hands its 32 registers to its own wave through a
//     wave-private LDS line; no workgroup barrier) instead of 32 store instructions from one lane;
//   * (|value|, row) travel as ONE 64-bit key {float bits : 2^32 - 1 - row}: a maximum over keys is LAPACK's first maximum, the wave
//     reduction is four DPP row rotations + four readlanes instead of six dependent cross-lane shuffles of three values;
//   * G <= 64 workgroups, so every WAVE reads all records itself (lane l <- workgroup l) and decides without a workgroup barrier;
//   * two workgroup barriers per column (candidate combine, pivot row staged) instead of four;
//   * rows are never moved between registers: an interchange j <-> p only swaps the two ROW LABELS (st.gr) -- the slot that held row p
//     now is row j (final, no longer eliminated), the slot that held row j carries on as row p -- and every slot is written to the row
//     its label names when the panel is done.  The old diagonal row is therefore never published or fetched, and the 256 conditional
//     moves + 64 LDS reads per thread and column of the value swap are gone (the step was VALU-issue bound: ~500 instructions per thread).
// Same decisions and the same arithmetic per row as the general step: identical pivots and factors.
template <int N>   // max with the key N lanes to the right inside each 16-lane row (row_ror)
__device__ __forceinline__ unsigned long long lu_dpp_max_step(unsigned long long k) {
    const unsigned long long o = dpp_mov<DPP_ROW_ROR + N>(k);
    return o > k ? o : k;
}
__device__ __forceinline__ unsigned long long lu_wave_max_u64(unsigned long long k) {
    k = lu_dpp_max_step<8>(k); k = lu_dpp_max_step<4>(k); k = lu_dpp_max_step<2>(k); k = lu_dpp_max_step<1>(k);
    const int lo = (int)(unsigned)k, hi = (int)(unsigned)(k >> 32);
    unsigned long long r = 0;
#pragma unroll
    for (int l = 0; l < 64; l += 16) {
        const unsigned long long v = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane(hi, l) << 32) | (unsigned)__builtin_amdgcn_readlane(lo, l);
        r = v > r ? v : r;
    }
    return r;
}
// key of a candidate: larger value wins, equal values -> smaller row wins; 0 = nothing to offer (also for NaN, which LAPACK's
// strict '>' search never selects either)
__device__ __forceinline__ unsigned long long lu_key(float absval, unsigned row) {
    return (absval == absval) ? (((unsigned long long)__float_as_uint(absval) << 32) | (0xffffffffu - row)) : 0ull;
}

constexpr int LF_RPT = 4;                 // rows per thread: 1024 rows per workgroup
struct LuF32Shared {
    float rb[4][PB];                      // wave-private hand-over lines (owner lane -> 32 lanes)
    unsigned long long key[4];
    float piv[2][PB];                     // by column parity: no barrier needed before the next column rewrites it
};

struct LuF32Step {   // (a type: lu_panel_steps<Step> calls Step::run<C> for every column)
    template <int C>
    static __device__ __forceinline__ void run(const LuArgs<float>& g, LuRegState<float, LF_RPT>& st, LuF32Shared& sh) {
        const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
        const int G = (int)gridDim.x, me = (int)blockIdx.x;
        const unsigned m = (unsigned)g.m;
        const unsigned j = (unsigned)g.j0 + C;
        constexpr int par = C & 1;
        const unsigned tag = g.tag_base + C + 1;
        unsigned long long* base = g.tw + (size_t)par * (size_t)(2 * G + G * PB + PB);
        unsigned long long* cw0 = base, *cw1 = cw0 + G, *rw = cw1 + G;
        // owner lane (row `want`) -> its wave's 32 low lanes -> one store instruction into dst[0..31]
        auto publish_row = [&](unsigned want, unsigned long long* dst) {
#pragma unroll
            for (int q = 0; q < LF_RPT; ++q) {
                const bool own = ((unsigned)st.gr[q] == want);
                if (__builtin_amdgcn_ballot_w64(own)) {                       // wave-uniform
                    if (own) {
#pragma unroll
                        for (int c2 = 0; c2 < PB; ++c2) sh.rb[wid][c2] = st.x[q][c2];
                    }
                    __builtin_amdgcn_s_waitcnt(0xc07f);                        // lgkmcnt(0): the line is written (same wave)
                    __builtin_amdgcn_wave_barrier();
                    if (lane < PB) lu_tag_put(dst + lane, tag, __float_as_uint(sh.rb[wid][lane]));
                    __builtin_amdgcn_wave_barrier();
                }
            }
        };
        LU_MARK(0)
        // ---- local candidate
        unsigned long long key = 0;
#pragma unroll
        for (int q = 0; q < LF_RPT; ++q) {
            const unsigned r = (unsigned)st.gr[q];
            const unsigned long long k2 = (r >= j && r < m) ? lu_key(fabsf(st.x[q][C]), r) : 0ull;
            key = k2 > key ? k2 : key;
        }
        key = lu_wave_max_u64(key);
        if (lane == 0) sh.key[wid] = key;
        __syncthreads();
        {
            unsigned long long k1 = sh.key[0];
#pragma unroll
            for (int w = 1; w < 4; ++w) k1 = sh.key[w] > k1 ? sh.key[w] : k1;
            key = k1;
        }
        const unsigned lrow = key ? 0xffffffffu - (unsigned)key : m;
        if (tid == 0) { lu_tag_put(cw0 + me, tag, (unsigned)(key >> 32)); lu_tag_put(cw1 + me, tag, lrow); }
        if (lrow >= m) { if (tid < PB) lu_tag_put(rw + (size_t)me * PB + tid, tag, 0u); }        // nothing to offer: a dummy row, readers never wait for one
        else publish_row(lrow, rw + (size_t)me * PB);
        LU_MARK(1)
        // ---- one batch of loads: record of workgroup `lane` (every wave reads all G <= 64 records), element tid % 32 of the diagonal row and
        //      of the candidate rows of workgroups tid / 32 + 8 u
        constexpr int PF = 8, NWD = 2 + PF;
        const unsigned long long* ad[NWD]; bool need[NWD]; unsigned got[NWD];
        {
            const int wl = lane < G ? lane : 0;
            ad[0] = cw0 + wl; need[0] = lane < G;
            ad[1] = cw1 + wl; need[1] = lane < G;
#pragma unroll
            for (int u = 0; u < PF; ++u) {
                const int wu = (tid >> 5) + 8 * u;
                ad[2 + u] = rw + (size_t)(wu < G ? wu : 0) * PB + (tid & 31); need[2 + u] = wu < G;
            }
        }
        lu_tag_get_n<NWD>(ad, need, tag, got, g.info);
        LU_MARK(2)
        // ---- decision, per wave
        const unsigned long long myk = (lane < G && got[1] < m) ? (((unsigned long long)got[0] << 32) | (0xffffffffu - got[1])) : 0ull;
        const unsigned long long gk = lu_wave_max_u64(myk);
        const unsigned p = gk ? 0xffffffffu - (unsigned)gk : j;                 // empty / NaN column: no exchange, (dummy) zero pivot row
        // the winner is the workgroup whose record carries the maximal key (keys are unique: rows are).  NOT (p - j0) / 1024: with
        // interchanges done by label a row lives wherever the slot that received its label is
        const unsigned long long whob = __builtin_amdgcn_ballot_w64(gk != 0ull && myk == gk);
        const int wstar = whob ? (int)__builtin_ctzll(whob) : 0;
        if ((tid >> 5) == (wstar & 7)) {
            unsigned pv = got[2];
#pragma unroll
            for (int u = 1; u < PF; ++u) pv = ((wstar >> 3) == u) ? got[2 + u] : pv;
            sh.piv[par][tid & 31] = __uint_as_float(pv);                        // (p == j: the winner's candidate row IS row j)
        }
        if (me == 0 && tid == 0) g.ipiv[j] = (int64_t)p + 1;
        __syncthreads();
        LU_MARK(3)
        // ---- interchange j <-> p by LABEL, then eliminate the rows below j.  (The same text in lu_f32.hip and lu_f64.hip: as one shared
        //      function template it gave both kernels another instruction schedule.)
        const float* s_piv = sh.piv[par];
        const float piv = s_piv[C];
        const float rp = 1.0f / piv;
#pragma unroll
        for (int q = 0; q < LF_RPT; ++q) {
            unsigned r = (unsigned)st.gr[q];
            if (p != j) { r = (r == j) ? p : (r == p) ? j : r; st.gr[q] = (int64_t)r; }
            if (piv != 0.0f && r > j && r < m) {
                const float l = st.x[q][C] * rp;
                st.x[q][C] = l;
#pragma unroll
                for (int c2 = C + 1; c2 < PB; ++c2) st.x[q][c2] -= l * s_piv[c2];
            }
        }
        if (piv == 0.0f && me == 0 && tid == 0 && *g.info == 0) *g.info = (int)(j + 1);
        LU_MARK(4)
    }
};
__global__ __launch_bounds__(256) void getrf_panel_f32_kernel(LuArgs<float> g) {
    __builtin_amdgcn_s_setprio(3);          // latency-bound: when a look-ahead runs this beside a GEMM on the same CUs, its waves issue first
    __shared__ LuF32Shared sh;
    LuRegState<float, LF_RPT> st;
    LU_PANEL_LOAD(float, LF_RPT, g, st)
    lu_panel_steps<LuF32Step>(g, st, sh);
    LU_PANEL_STORE(LF_RPT, g, st)
}

}  // namespace

void launch_getrf_panel_f32(const LuArgs<float>& g, unsigned G, hipStream_t stream) {
    hipLaunchKernelGGL(getrf_panel_f32_kernel, dim3(G), dim3(256), 0, stream, g);
}

}  // namespace rlhip_lu
