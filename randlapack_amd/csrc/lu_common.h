// Shared by lu.hip (LDS and general register panel kernels, host driver), lu_f32.hip and lu_f64.hip (the fp32 / fp64 fast panel steps):
// the argument block, the tagged-word store and batched fetch, and the frame of a register panel kernel, which does not depend on how a
// column step finds and hands over the pivot -- register state, panel load and store, the unrolled walk over the columns.  Three
// translation units because each unrolls 32 column steps and takes minutes to compile: side by side the build is as long as the
// longest one.
#pragma once
#include "rlhip_internal.h"

namespace rlhip_lu {

constexpr int PB = 32;

// The field order is the kernels' argument layout.  [LDS]: read by the LDS kernel (getrf_panel_kernel) only, the exchange through a grid
// rendezvous with slots by column parity.  [reg]: read by the register kernels (getrf_panel_reg_kernel, getrf_panel_f32_kernel,
// getrf_panel_f64_kernel) only, the flag-less exchange.  Everything else is read by all of them.
template <typename T>
struct LuArgs {
    int64_t m, n;             // full matrix
    T* A; int64_t lda;
    int64_t j0; int pb;       // panel [j0, j0+pb)
    int64_t* ipiv;            // 1-based, device
    T* cand_val; int64_t* cand_row;   // [LDS] 2 x G
    T* cand_data;             // [LDS] 2 x G x PB  : candidate row contents
    T* diag_data;             // [LDS] 2 x PB      : contents of the current diagonal row ([reg]: the RLHIP_LU_PROF counters behind them)
    unsigned* bar;            // [LDS] arrival counter of grid_barrier
    int* info;                // first zero pivot (1-based), 0 if none; -7: a tagged word never arrived
    int64_t rpw;              // [LDS] rows per workgroup
    unsigned long long* tw;   // [reg] tagged 8-byte words, W = sizeof(T) / 4 per value: 2 x (W G + G + W G PB + W PB)
    unsigned tag_base;        // [reg] tags of this launch are tag_base + 1 .. tag_base + PB (unique across launches)
};

// a 32-bit payload under `tag`: one 8-byte store, so a reader sees both or neither
__device__ __forceinline__ void lu_tag_put(unsigned long long* q, unsigned tag, unsigned payload) {
    __hip_atomic_store(q, ((unsigned long long)tag << 32) | payload, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// N tagged words in ONE batch of loads (re-read together until every needed word carries the tag): data that is already there costs
// a single round trip however many words a thread needs
template <int N>
__device__ __forceinline__ void lu_tag_get_n(const unsigned long long* const (&ad)[N], const bool (&need)[N], unsigned tag, unsigned (&out)[N], int* info) {
    for (int spins = 0;; ++spins) {
        unsigned long long w[N];
#pragma unroll
        for (int i = 0; i < N; ++i) w[i] = need[i] ? __hip_atomic_load(ad[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : ((unsigned long long)tag << 32);
        bool ok = true;
#pragma unroll
        for (int i = 0; i < N; ++i) ok = ok && ((unsigned)(w[i] >> 32) == tag);
        if (ok || spins > (1 << 22)) {
            if (!ok) atomicExch(info, -7);
#pragma unroll
            for (int i = 0; i < N; ++i) out[i] = (unsigned)w[i];
            return;
        }
        __builtin_amdgcn_s_sleep(1);
    }
}

template <typename T, int RPT>
struct LuRegState {
    T x[RPT][PB];
    int64_t gr[RPT];
#ifdef RLHIP_LU_PROF
    long long pf[5], pt;
#endif
};
#ifdef RLHIP_LU_PROF
#define LU_MARK(i) { const long long now_ = wall_clock64(); st.pf[i] += now_ - st.pt; st.pt = now_; }
#else
#define LU_MARK(i)
#endif

// ---- the frame of a register panel kernel: workgroup `me` owns rows j0 + 256 RPT me + tid + 256 q, q < RPT, as RPT x 32 registers.
// Load and store are macros, not functions: the compiler simplifies a function of its own before it inlines it, and the kernels then
// come out with another instruction schedule.
// (The selects of the load come after ALL loads: written as `cond ? load : 0` per entry, hipcc sinks every load into its own branch with
// an s_waitcnt vmcnt(0) behind it -- 128 dependent L2 round trips = ~30 us per panel launch.)
#define LU_PANEL_LOAD(T, RPT, g, st)                                                                                                  \
    {                                                                                                                                 \
        const int tid = threadIdx.x;                                                                                                  \
        const int64_t me = blockIdx.x;                                                                                                \
        const int pb = g.pb;                                                                                                          \
        const int64_t j0 = g.j0, m = g.m;                                                                                             \
        const int64_t lo = j0 + me * (256 * RPT);                                                                                     \
        _Pragma("unroll") for (int q = 0; q < RPT; ++q) {                                                                             \
            st.gr[q] = lo + tid + 256 * q;                                                                                            \
            const int64_t rr = st.gr[q] < m ? st.gr[q] : m - 1;           /* clamped row and column: unconditional coalesced */       \
            _Pragma("unroll") for (int c = 0; c < PB; ++c)                /* loads, all in flight together                   */       \
                st.x[q][c] = g.A[rr + (j0 + (c < pb ? c : pb - 1)) * g.lda];                                                          \
        }                                                                                                                             \
        __builtin_amdgcn_sched_barrier(0);                                                                                            \
        _Pragma("unroll") for (int q = 0; q < RPT; ++q) {                                                                             \
            _Pragma("unroll") for (int c = 0; c < PB; ++c) st.x[q][c] = (st.gr[q] < m && c < pb) ? st.x[q][c] : T(0);                 \
        }                                                                                                                             \
        lu_prof_begin(st);                                                                                                            \
    }
// every slot goes to the row its label names (the fast steps interchange labels, not values)
#define LU_PANEL_STORE(RPT, g, st)                                                                                                    \
    {                                                                                                                                 \
        lu_prof_end(g, st);                                                                                                           \
        const int pb = g.pb;                                                                                                          \
        const int64_t j0 = g.j0, m = g.m;                                                                                             \
        _Pragma("unroll") for (int q = 0; q < RPT; ++q) {                                                                             \
            if (st.gr[q] < m) {                                                                                                       \
                _Pragma("unroll") for (int c = 0; c < PB; ++c)                                                                        \
                    if (c < pb) g.A[st.gr[q] + (j0 + c) * g.lda] = st.x[q][c];                                                        \
            }                                                                                                                         \
        }                                                                                                                             \
    }
// RLHIP_LU_PROF: the phase clocks of LU_MARK start after the load; the middle workgroup adds its totals to the counters behind diag_data
template <typename T, int RPT>
__device__ __forceinline__ void lu_prof_begin(LuRegState<T, RPT>& st) {
#ifdef RLHIP_LU_PROF
    for (int i = 0; i < 5; ++i) st.pf[i] = 0;
    st.pt = wall_clock64();
#endif
}
template <typename T, int RPT>
__device__ __forceinline__ void lu_prof_end(const LuArgs<T>& g, const LuRegState<T, RPT>& st) {
#ifdef RLHIP_LU_PROF
    if (blockIdx.x == gridDim.x / 2 && threadIdx.x == 0) for (int i = 0; i < 5; ++i) atomicAdd((unsigned long long*)(g.diag_data + 2 * PB) + i, (unsigned long long)st.pf[i]);
#endif
}
// Step::run<C>(g, st, sh...) for C = 0 .. g.pb - 1.  The column index is a template parameter so that every x[q][c] index is a compile-time
// constant and the panel really stays in registers (a runtime-indexed loop put it in scratch).
template <typename Step, int C = 0, typename T, int RPT, typename... Sh>
__device__ __forceinline__ void lu_panel_steps(const LuArgs<T>& g, LuRegState<T, RPT>& st, Sh&... sh) {
    if constexpr (C < PB) {
        if (C < g.pb) {                                           // uniform: pb is a kernel argument
            Step::template run<C>(g, st, sh...);
            lu_panel_steps<Step, C + 1>(g, st, sh...);
        }
    }
}

// launcher of the fp32 panel step (lu_f32.hip): grid G <= 64 workgroups of 256 threads, 1024 rows each
void launch_getrf_panel_f32(const LuArgs<float>& g, unsigned G, hipStream_t stream);
// launcher of the fp64 panel step (lu_f64.hip): G <= 64 workgroups of 256 threads, 512 rows each
void launch_getrf_panel_f64(const LuArgs<double>& g, unsigned G, hipStream_t stream);

}  // namespace rlhip_lu
