// Internal (non-ABI) declarations shared by the HIP translation units of librlhip.so: the error / LDS-limit macros, the execution
// context with its scratch arena, and THE declaration of every namespace rlhip host function that one .hip file defines and another
// calls (grouped by defining file, at the end).  A .hip file declares no function of another file itself; forward declarations of
// functions local to one file stay in that file.  The device-side helpers shared between kernel files are in rlhip_device.h.
// Everything here is MI355X / gfx950 only: 64-lane wavefronts, MFMA, 160 KiB LDS.
#pragma once
#include <mutex>
#include <utility>
#include <vector>
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstddef>
#include <cstdio>
#include "rlhip.h"

#define RLHIP_ERR_HIP(e) (-1000 - (int)(e))

#define RLHIP_CHECK(expr)                                                     \
    do {                                                                      \
        hipError_t _e = (expr);                                               \
        if (_e != hipSuccess) {                                               \
            fprintf(stderr, "[rlhip] %s:%d: %s -> %s\n", __FILE__, __LINE__,  \
                    #expr, hipGetErrorString(_e));                            \
            return RLHIP_ERR_HIP(_e);                                         \
        }                                                                     \
    } while (0)

#define RLHIP_LAUNCH_CHECK() RLHIP_CHECK(hipGetLastError())

// Raise a kernel's dynamic-LDS limit once PER DEVICE (kernel function attributes are per device: a process-wide flag would leave
// the second device of a process at the 64 KiB default).  `func` must be the kernel's address; the flag array lives at the call site.
#define RLHIP_FUNC_LDS(c, func, bytes)                                                                                     \
    do {                                                                                                                   \
        static bool _rlhip_lds_done[64] = {};                                                                              \
        const int _d = (c)->device & 63;                                                                                   \
        if (!_rlhip_lds_done[_d]) {                                                                                        \
            RLHIP_CHECK(hipSetDevice((c)->device));                                                                        \
            RLHIP_CHECK(hipFuncSetAttribute((const void*)(func), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(bytes))); \
            _rlhip_lds_done[_d] = true;                                                                                    \
        }                                                                                                                  \
    } while (0)

// The same for call sites where the kernel is a RUN-TIME value (a generic lambda over several instantiations shares one static per
// function-pointer TYPE, so the macro above would raise the limit of the first variant only): one flag per (device, kernel address).
#define RLHIP_FUNC_LDS_DYN(c, func, bytes)                                                                                 \
    do {                                                                                                                   \
        static std::mutex _rlhip_lds_mu;                                                                                   \
        static std::vector<std::pair<int, const void*>> _rlhip_lds_seen;                                                   \
        std::lock_guard<std::mutex> _rlhip_lds_lock(_rlhip_lds_mu);                                                        \
        const std::pair<int, const void*> _key((c)->device, (const void*)(func));                                          \
        bool _found = false;                                                                                               \
        for (auto const& _e : _rlhip_lds_seen) _found = _found || (_e == _key);                                            \
        if (!_found) {                                                                                                     \
            RLHIP_CHECK(hipSetDevice((c)->device));                                                                        \
            RLHIP_CHECK(hipFuncSetAttribute(_key.second, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(bytes)));       \
            _rlhip_lds_seen.push_back(_key);                                                                               \
        }                                                                                                                  \
    } while (0)

// ---- the mailbox slots (c->h_mail / c->d_mail: MAIL_WORDS 8-byte words each; a slot index holds in both unless a line says otherwise).
// Owner file, extent in words, lifetime.  "transient": written, waited for and read inside ONE call of the owner (copy, wait, read), so
// two transient ranges may overlap -- several do, each noted below; "across calls": the value waits in the slot for a LATER call.
constexpr int MAIL_WORDS = 64;
constexpr int MAIL_SCALAR = 0;              // aux.hip lange_fro: sum of squares; capi.hip peak probes: their never-taken store.  1, transient
constexpr int MAIL_ABSMAX = 1;              // aux.hip lange_fro: largest |entry| of the rescaled pass.  1, transient
constexpr int MAIL_POTRF_INFO = 8;          // chol.hip potrf_upper: LAPACK's info.  1, transient
constexpr int MAIL_JACOBI = 16;             // jacobi.hip: rotation counters on the device (4 unsigned), up to 8 ints read back.  4, transient
constexpr int MAIL_TRSM_VERDICT = 16;       // tri.hip (h_mail only): block verdicts + pivot verdict, 33 ints.  17 (reaches MAIL_SVD_RATIO,
constexpr int MAIL_TRSM_VERDICT_WORDS = 17; //   MAIL_SVD_GRAM_DEV and the first word of MAIL_SVD_GRAM), transient
constexpr int MAIL_SVD_RATIO = 24;          // svd.hip gesdd_tall_core: diagonal ratio of the first Cholesky factor.  1, transient
constexpr int MAIL_SVD_GRAM_DEV = 25;       // svd.hip gesdd_tall_core: max |Q^T Q - I| after pass 1.  1, transient
constexpr int MAIL_SVD_GRAM = 32;           // svd.hip gesdd_tall_gram (h_mail only): the Jacobi launch's 8 ints, then the defect (double) in
constexpr int MAIL_SVD_GRAM_WORDS = 5;      //   word MAIL_SVD_GRAM_DEFECT.  5, transient
constexpr int MAIL_SVD_GRAM_DEFECT = MAIL_SVD_GRAM + 4;
constexpr int MAIL_HOST_REDUCE = 32;        // comm.hip rlhip_allreduce_sum_host_f64 (d_mail only): up to 16 doubles.  16, transient -- but from
constexpr int MAIL_HOST_REDUCE_WORDS = 16;  //   the 9th double on it OVERWRITES d_mail's MAIL_NORMA_SSQ (across calls): see the note below
constexpr int MAIL_DVFS_SINK = 32;          // capi.hip rlhip_dvfs_burn (d_mail only): the burn kernel's never-taken store.  1, transient
constexpr int MAIL_NORMA_SSQ = 40;          // capi.hip rlhip_gemm_norma_f64: ||A||_F^2 fused into a product.  1, ACROSS CALLS while norma_state == 1:
                                            //   h_mail for rlhip_norma_collect_f64, d_mail for tri.hip cholqrq (rides on the Gram all-reduce)
constexpr int MAIL_NORMA_SSQ_RANKS = 41;    // tri.hip cholqrq -> capi.hip rlhip_norma_collect_f64 (h_mail only): that sum over the row shards.
                                            //   1, ACROSS CALLS while norma_reduced == 1
constexpr int MAIL_GEQRF_CHOLQR = 44;       // house.hip geqrf_cholqr (h_mail only): two potrf infos (words 0, 1), |R2 - I| (word 2).  3, transient
constexpr int MAIL_CHOLQRQ = 44;            // tri.hip cholqrq (h_mail only): potrf info + block verdicts, 40 ints.  20 (to the mailbox's end: covers
constexpr int MAIL_CHOLQRQ_WORDS = 20;      //   every slot from MAIL_GEQRF_CHOLQR to MAIL_SAMPLE_HDR), transient
constexpr int MAIL_ANY_FLAG = 48;           // house.hip any_abs_gt: the flag.  1, transient
constexpr int MAIL_CSR_NNZ = 50;            // sparse.hip csr_transpose (h_mail only): rowptr[m].  1, transient
constexpr int MAIL_CSR_BAD = 51;            // sparse.hip csr_transpose: index-check flag, then the longest transposed row in word
constexpr int MAIL_CSR_MAXLEN = MAIL_CSR_BAD + 1;   //   MAIL_CSR_MAXLEN; cleared and read back together.  2, transient
constexpr int MAIL_PANEL_INFO = 56;         // lu.hip getrf, qrcp.hip (h_mail only): the panel kernel's info word.  1, transient
constexpr int MAIL_SAMPLE_HDR = 60;         // rpchol.hip (h_mail only): SampleHdr.  4, transient
constexpr int MAIL_SAMPLE_HDR_WORDS = 4;
constexpr bool mail_disjoint(int a, int na, int b, int nb) { return a + na <= b || b + nb <= a; }
static_assert(MAIL_TRSM_VERDICT + MAIL_TRSM_VERDICT_WORDS <= MAIL_WORDS && MAIL_SVD_GRAM + MAIL_SVD_GRAM_WORDS <= MAIL_WORDS &&
              MAIL_HOST_REDUCE + MAIL_HOST_REDUCE_WORDS <= MAIL_WORDS && MAIL_CHOLQRQ + MAIL_CHOLQRQ_WORDS <= MAIL_WORDS &&
              MAIL_CSR_BAD + 2 <= MAIL_WORDS && MAIL_SAMPLE_HDR + MAIL_SAMPLE_HDR_WORDS <= MAIL_WORDS, "a mailbox extent ends within the mailbox");
// no transient range of h_mail covers the two across-call slots
static_assert(mail_disjoint(MAIL_TRSM_VERDICT, MAIL_TRSM_VERDICT_WORDS, MAIL_NORMA_SSQ, 2) && mail_disjoint(MAIL_SVD_GRAM, MAIL_SVD_GRAM_WORDS, MAIL_NORMA_SSQ, 2) &&
              mail_disjoint(MAIL_JACOBI, 4, MAIL_NORMA_SSQ, 2) && mail_disjoint(MAIL_CHOLQRQ, MAIL_CHOLQRQ_WORDS, MAIL_NORMA_SSQ, 2),
              "a transient h_mail range covers the deferred norm");
// The same does NOT hold in d_mail: MAIL_HOST_REDUCE's 16 doubles span words 32 .. 47 and MAIL_NORMA_SSQ is word 40.  A host all-reduce of
// more than 8 doubles issued between a product that deferred its norm (norma_state == 1) and the cholqrq(reduce_gram) that reads
// d_mail + MAIL_NORMA_SSQ replaces the sum of squares by the all-reduce's 9th value.  Such a caller exists: blas::Queue::shard_extent
// (include/RandLAPACK_amd/rl_blaspp.hh) reduces one double per rank, n = world size, so from nine ranks on it writes d_mail words 40 .. 47.
// It is called from rl_rs.hh, rl_linops.hh (twice), rl_cqrrpt.hh (twice), rl_cqrrt.hh, rl_bqrrp.hh, rl_abrik.hh, rl_qr_linops.hh and
// rl_sharded_panel.hh.  Whether one of those calls can fall between a product that defers its norm and the cholqrq(reduce_gram) behind
// it has NOT been established for any of them; until it has, treat the overlap as reachable with more than eight ranks.

// Execution context: one HIP stream + a growable device scratch arena + a small
// pinned host mailbox for info codes / scalars coming back from the device.
constexpr int RLHIP_NPATH = 43;          // slots of rlhip_path_count (indices: include/rlhip.h)
struct rlhip_ctx {
    int device = 0;
    int num_cu = 256;            // compute units of THIS context's device (persistent kernels size their grids with it)
    hipStream_t stream = nullptr;
    bool owns_stream = false;
    // scratch arena: stack-disciplined bump allocator over a short list of device segments.  Marks are virtual
    // offsets (segment k starts where segment k-1's full size ends); when a request does not fit, a new, larger
    // segment is appended (hipMalloc once); when the stack returns to empty the segments are merged into one so
    // that steady-state calls never allocate.  Library code opens and closes a marked region with ws_scope (below), never by hand.
    struct Seg { char* base; size_t size; };
    Seg segs[32];
    int nsegs = 0;
    int cur_seg = 0;          // segment currently bumped
    size_t cur_used = 0;      // bytes used inside segs[cur_seg]
    size_t ws_highwater = 0;  // largest virtual offset ever reached
    // pinned mailbox
    int64_t* h_mail = nullptr;   // MAIL_WORDS x int64 host-pinned (slots: the MAIL_ table above)
    int64_t* d_mail = nullptr;   // MAIL_WORDS x int64 device
    void* xchg = nullptr;        // exchange words of the persistent panel kernels (see rlhip_xchg_buffer)
    size_t xchg_bytes = 0;
    void* xloc = nullptr;        // ordinary (cached) twin of the exchange buffer: same-XCD hand-overs of the persistent Jacobi launch (rlhip_xloc_buffer)
    size_t xloc_bytes = 0;
    // timing of the most recent GEMM-family launch set (bench.py roofline leg)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t ev_flag = nullptr;   // marks a flag read-back INSIDE a stream of launches: the host waits for the flags only, the device runs on (tri.hip)
    // ||A||_F fused into a product and not yet collected (rlhip_gemm_norma_f64 with a null result pointer): 0 nothing, 1 the sum of squares
    // is on its way to h_mail[MAIL_NORMA_SSQ] behind the stream, 2 norma_value holds the norm
    int norma_state = 0;
    double norma_value = 0;
    int norma_reduced = 0;           // 1: the sum over the row shards is on its way to h_mail[MAIL_NORMA_SSQ_RANKS] as well (rode on the Gram matrix's all-reduce, tri.hip::cholqrq)
    unsigned long norma_epoch = 0;   // sync_epoch when the deferred copy was enqueued
    unsigned long sync_epoch = 0;    // completed host waits on the stream (rlhip_stream_sync): anything enqueued before the last one has landed
    // != 0: products take the tiled kernel whose workgroups come and go, not the persistent stream-K kernel that holds every CU for its whole
    // duration (set around a product that is meant to share the device with another stream: house.hip::gemqrt_lt_tail)
    int avoid_persistent = 0;
    // > 0: columns per workgroup of the tag-exchange pivoted QR (default 4; a caller that overlaps the factorization with another kernel packs
    // the columns into fewer workgroups so that it occupies fewer CUs)
    int qrcp_cols_per_wg = 0;
    int64_t opt[RLHIP_OPT_COUNT] = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1};   // rlhip_set_option; -1 = default
    rlhip_ctx* side_ctx = nullptr;   // cached side context (rlhip_side_of): created on first use, destroyed with this one
    hipStream_t side = nullptr;  // second stream, created on first use (rlhip_dvfs_burn: load beside the main stream's latency-bound kernels)
    // row-sharding communicator (comm.hip), nullptr = single GPU
    void* comm = nullptr;
    // caching pool behind rlhip_malloc/rlhip_free (outputs the drivers allocate for the caller: Q, BT, U, S, V).
    // Blocks are recycled by exact size; reuse is ordered by the context's stream, so freeing does not synchronise.
    struct PoolBlk { void* p; size_t bytes; bool in_use; unsigned long stamp; };
    PoolBlk pool[256];
    int npool = 0;
    size_t pool_idle_bytes = 0, pool_cap_bytes = 0;
    unsigned long pool_clock = 0;
    // diagnostics: how often each specialised kernel path was taken (rlhip_path_count; tests assert the path under test ran)
    //   0 stream-K f64 GEMM, 1 stream-K f32 GEMM, 2 fused trsm block kernel, 3 substitution trsm sub-block, 4 fused out-of-place trsm
    //   (rlhip_trsm_gather), 5 sketch-preconditioned Cholesky-QR panel inside geqrf -- the list in include/rlhip.h is the contract
    int64_t path_count[RLHIP_NPATH] = {};
    // the routes of the PCG update kernels (pcg.hip), read through rlhip_pcg_path_count: [0] = 43 fused update_xr, [1] = 44 fused update_p,
    // [2] = 45 either one composed from products
    int64_t pcg_path_count[3] = {};
    // the routes of the matrix-vector layer (lsq.hip), read through rlhip_lsq_path_count: [0] = 46 fused normal matvec, [1] = 47 composed
    // normal matvec, [2] = 48 gemv 'N', [3] = 49 gemv 'T'
    int64_t lsq_path_count[4] = {};
    // the routes of the sparse matrix-vector layer (spmv.hip), read through rlhip_spmv_path_count: [0] = 50 four lanes per row, [1] = 51
    // sixteen, [2] = 52 sixty-four, [3] = 53 split long rows, [4] = 54 csr_normal_matvec calls
    int64_t spmv_path_count[5] = {};
    // the routes of the two-point-set RBF kernels (rbf.hip), read through rlhip_rbf_path_count: [0] = 55 fused cross apply, [1] = 56 composed
    // cross apply, [2] = 57 sqexp_cross_submatrix calls
    int64_t rbf_path_count[3] = {};
    int64_t rbf_split_count = 0;     // fused cross applies that ran split over X (RLHIP_OPT_RBF_FUSED = 2, rlhip_rbf_split_count)
    // the routes of the kernel quadratic form (rbf_var.hip), read through rlhip_pdk_var_path_count: [0] = 58 fused, [1] = 59 composed
    int64_t var_path_count[2] = {};
    // the routes of the LU layer (lu.hip), read through rlhip_lu_path_count: [0] = 60 a panel on the LDS kernel, [1] = 61 on the fast step,
    // [2] = 62 on the general register kernel, [3] = 63 getrf calls with an outer block wider than a panel, [4] = 64 launches of
    // unit_lower_solve_kernel, [5] = 65 luqrcp_piv on the LDS walk, [6] = 66 on the serial kernel
    int64_t lu_path_count[7] = {};
    // the routes of the triangular layer (tri.hip) that path_count 2, 3, 4 and 11 do not tell apart, read through rlhip_tri_path_count:
    // [0] = 67 a 256-block on trsm_blk_kernel<T, 1>, [1] = 68 on trsm_blk_kernel<T, 2>, [2] = 69 a fused launch of the twelve-wavefront
    // instantiation, [3] = 70 a fused out-of-place solve on the identity twin (OOP = 2), [4] = 71 a trsm_gather call served by gather-copy +
    // the in-place solver, [5] = 72 trmm_right_upper calls, [6] = 73 trmm_left_upper calls
    int64_t tri_path_count[7] = {};
    int var_fused = 0;               // rlhip_pdk_var_set_fused: 1 = rlhip_pdk_cross_var_* takes its fused kernel where the shape allows
    // the routes of the kernel-gradient apply (rbf_grad.hip), read through rlhip_pdk_grad_path_count: [0] = 74 fused, [1] = 75 composed
    int64_t grad_path_count[2] = {};
    int grad_fused = 0;              // rlhip_pdk_grad_set_fused: 1 = rlhip_pdk_cross_grad_* takes its fused kernel where the shape allows
    // the routes of the block least-squares layer (lsq.hip), read through rlhip_lsq_block_path_count: [0] = 76 one-pass normal matmat,
    // [1] = 77 composed normal matmat, [2] = 78 iterations of pcg_saddle_block (block step_d calls that update d)
    int64_t lsq_block_path_count[3] = {};
    int matmat_route = -1;           // rlhip_normal_matmat_set_route: -1 the default, 0 always composed, 1 one-pass wherever the shape allows
};

// every host wait of the library goes through here: the epoch lets deferred read-backs know that an earlier wait already covered them
static inline hipError_t rlhip_stream_sync(rlhip_ctx* c) {
    const hipError_t e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) ++c->sync_epoch;
    return e;
}

// scratch arena helpers (capi.hip).  Library code takes and returns marks through ws_scope only; the bare mark / release pair is for
// the scratch ABI entry points and rlhip_reserve_workspace in capi.hip.
void* rlhip_ws_alloc(rlhip_ctx* c, size_t bytes);           // 256-B aligned, never fails softly (nullptr on OOM)
size_t rlhip_ws_mark(rlhip_ctx* c);
void rlhip_ws_release(rlhip_ctx* c, size_t mark);

template <typename T>
static inline T* ws_alloc(rlhip_ctx* c, size_t n) { return (T*)rlhip_ws_alloc(c, n * sizeof(T)); }

// One marked region of the arena: everything allocated after the constructor goes back when the scope ends, on every way out of it
// (a plain return and the return inside RLHIP_CHECK included).  A region that ends before its function does is a { } block.
struct ws_scope {
    rlhip_ctx* const c;
    const size_t mark;
    explicit ws_scope(rlhip_ctx* ctx) : c(ctx), mark(rlhip_ws_mark(ctx)) {}
    ~ws_scope() { rlhip_ws_release(c, mark); }
    ws_scope(const ws_scope&) = delete;
    ws_scope& operator=(const ws_scope&) = delete;
    template <typename T>
    T* alloc(size_t n) { return ws_alloc<T>(c, n); }   // nullptr when the arena cannot grow
};
// workgroups of `per` threads for `work` threads' worth of it
static inline unsigned grid1(int64_t work, int per) { return (unsigned)((work + per - 1) / per); }
// device buffer for the tagged-word exchanges between workgroups (QRCP / LU panel kernels); grows, lives with the context.
// RLHIP_XCHG = 0: ordinary device memory, 1: fine-grained, 2: uncached (default)
void* rlhip_xchg_buffer(rlhip_ctx* c, size_t bytes);
void* rlhip_xloc_buffer(rlhip_ctx* c, size_t bytes);

// ---- typed internal entry points (implemented in the .hip files; the extern "C" ABI wraps them): each one is declared here and nowhere else ----
namespace rlhip {

enum Op : int { NoTrans = 0, Trans = 1 };
enum Uplo : int { Upper = 0, Lower = 1 };
enum Diag : int { NonUnit = 0, Unit = 1 };
enum Dist : int { Gaussian = 0, UniformPM1 = 1 };

template <typename T>
int gemm(rlhip_ctx* c, int transA, int transB, int64_t m, int64_t n, int64_t k, T alpha, const T* A,
         int64_t lda, const T* B, int64_t ldb, T beta, T* C, int64_t ldc);

// C(upper or lower) = alpha * op(A)^T-style Gram + beta*C, LAPACK syrk semantics (only `uplo` part referenced/written)
template <typename T>
int syrk(rlhip_ctx* c, int uplo, int trans, int64_t n, int64_t k, T alpha, const T* A, int64_t lda,
         T beta, T* C, int64_t ldc);

template <typename T>
int potrf_upper(rlhip_ctx* c, int64_t n, T* A, int64_t lda, int* info_host);

// B <- alpha * B * inv(op(A)),  A upper triangular n x n (Side::Right, Uplo::Upper, NoTrans)
template <typename T>
int trsm_right_upper_oop(rlhip_ctx* c, int diag, int64_t m, int64_t n, T alpha, const T* A, int64_t lda, const T* Bsrc, int64_t ldsrc,
                         const int64_t* perm_dev, T* B, int64_t ldb);
template <typename T>
int trsm_right_upper_oop_range(rlhip_ctx* c, int diag, int64_t m, int64_t nsrc, T alpha, const T* A, int64_t lda, const T* Bsrc, int64_t ldsrc,
                               const int64_t* perm_dev, T* B, int64_t ldb, int64_t col0, int64_t col1);
template <typename T>
int trsm_right_upper(rlhip_ctx* c, int diag, int64_t m, int64_t n, T alpha, const T* A, int64_t lda,
                     T* B, int64_t ldb);

// B <- alpha * B * A,  A upper triangular n x n (Side::Right, Uplo::Upper, NoTrans); B is m x n
template <typename T>
int trmm_right_upper(rlhip_ctx* c, int diag, int64_t m, int64_t n, T alpha, const T* A, int64_t lda,
                     T* B, int64_t ldb);

template <typename T>
int trmm_left_upper(rlhip_ctx* c, int trans, int diag, int64_t m, int64_t n, T alpha, const T* A, int64_t lda, T* B, int64_t ldb);

template <typename T>
int fill_dense(rlhip_ctx* c, int dist, int64_t rows, int64_t cols, T* buf, const uint32_t ctr[4],
               const uint32_t key[2], uint32_t next_ctr[4]);

template <typename T>
int lange_fro(rlhip_ctx* c, int64_t m, int64_t n, const T* A, int64_t lda, T* result_host);

template <typename T>
int lacpy(rlhip_ctx* c, int uplo /*0 upper,1 lower,2 general*/, int64_t m, int64_t n, const T* A,
          int64_t lda, T* B, int64_t ldb);

template <typename T>
int laset(rlhip_ctx* c, int uplo /*0 upper,1 lower,2 general*/, int64_t m, int64_t n, T offdiag, T diag,
          T* A, int64_t lda);

// one-sided Jacobi SVD of a tall m x n (m >= n) matrix: A = U diag(S) VT.
// On exit A holds U (m x n), S descending, VT n x n (ld ldvt).
template <typename T>
int gesvdj(rlhip_ctx* c, int64_t m, int64_t n, T* A, int64_t lda, T* S, T* VT, int64_t ldvt,
           int* sweeps_host);


// gesvdj without the argument checks and the exponent-range guard (the caller has done both): what gesdd_tall runs on its own factors
template <typename T>
int gesvdj_core(rlhip_ctx* c, int64_t m, int64_t n, T* A, int64_t lda, T* S, T* VT, int64_t ldvt, int* sweeps_host);
// exponent-range guard of the SVDs (qrcp.hip, beside geqrf's): begin scales A by a power of two when max |a_ij| lies outside the safe
// window and leaves the measurement in w (4 device words); end gives the n singular values their scale back.  No host read.
template <typename T>
int svd_guard_begin(rlhip_ctx* c, int64_t m, int64_t n, T* A, int64_t lda, unsigned long long* w);
template <typename T>
int svd_guard_end(rlhip_ctx* c, int64_t n, T* S, const unsigned long long* w);

// A[i,i] += alpha
template <typename T>
int add_diag(rlhip_ctx* c, int64_t n, T alpha, T* A, int64_t lda);

// AT (n x m, ld ldat) = A^T (A m x n); upper_only: only entries i <= j of A are moved
template <typename T>
int transpose(rlhip_ctx* c, int64_t m, int64_t n, const T* A, int64_t lda, T* AT, int64_t ldat, int upper_only);

// thin SVD of a tall matrix with separate outputs (LAPACK gesdd 'S' contract); A is destroyed
template <typename T>
int gesdd_tall(rlhip_ctx* c, int64_t m, int64_t n, T* A, int64_t lda, T* S, T* U, int64_t ldu, T* VT,
               int64_t ldvt, int* sweeps_host);

// ---- gemm.hip
// the router behind gemm (tri = 0) and syrk (tri = 1).  ssqA_dev / ssq_done: the sum of squares of A fused into the product
// (rlhip_gemm_norma_f64); *ssq_done says how much of A the route taken covered, see the definition
template <typename T>
int gemm_impl(rlhip_ctx* c, int transA, int transB, int64_t m, int64_t n, int64_t k, T alpha, const T* A, int64_t lda,
              const T* B, int64_t ldb, T beta, T* C, int64_t ldc, int tri, double* ssqA_dev = nullptr, int* ssq_done = nullptr);

// ---- gemm_sk.hip
// returns 1 if the problem was handled here, 0 if the caller should use the generic kernel, <0 on error
template <typename T>
int gemm_streamk(rlhip_ctx* c, int transA, int transB, int64_t m, int64_t n, int64_t k, T alpha, const T* A, int64_t lda, const T* B,
                 int64_t ldb, T beta, T* C, int64_t ldc, double* ssqA_dev, int tri);

// ---- fill.hip
// rows [row0, row0 + loc_rows) of the glob_rows x cols matrix that fill_dense draws from the same counter / key
template <typename T>
int fill_dense_rows(rlhip_ctx* c, int dist, int64_t glob_rows, int64_t cols, int64_t row0, int64_t loc_rows, T* buf, int64_t ld,
                    const uint32_t ctr[4], const uint32_t key[2], uint32_t next_ctr[4]);
int philox_raw(rlhip_ctx* c, int64_t nblk, uint32_t* out_dev, const uint32_t ctr[4], const uint32_t key[2]);

// ---- chol.hip
// The one-workgroup factorization ENQUEUED only: LAPACK's info (0, or the 1-based index of the first non-positive pivot) goes to the DEVICE
// word `info_dev`, which later kernels of the stream may test; nothing is read back.  n <= 448 only (returns 1 otherwise: not available).
template <typename T>
int potrf_upper_enqueue(rlhip_ctx* c, int64_t n, T* A, int64_t lda, int* info_dev);

// ---- tri.hip
// Cholesky-QR, Q factor only: R (k x k, ld k) = chol(A^T A), A <- A R^-1, *info_host = LAPACK's potrf info, one host read.  `reduce_gram`:
// row-sharded input, the Gram matrix is summed over the ranks first.  Returns 1 when the shape is not served here: the caller runs the three calls.
template <typename T>
int cholqrq(rlhip_ctx* c, int64_t m, int64_t k, T* A, int64_t lda, T* R, int reduce_gram, int* info_host);

// ---- jacobi.hip
// ENQUEUES the one-launch Jacobi sweeps of an n x n matrix (trans_upper = 0: the matrix stored in R, 1: R^T of the upper triangle in R) and
// returns without touching the host; the contract is at the definition.  Returns 0 when enqueued, 1 when the path is not available, < 0 on error.
template <typename T>
int jacobi_enqueue_rt(rlhip_ctx* c, int n, const T* R, int64_t ldr, int trans_upper, float norm_ratio_lim, const int* skip_dev, int* out_dev,
                      const T** X_out);

// ---- sketch.hip
struct SasoOp;   // sparse sign operator S (d x m); the ABI's rlhip_saso is this type
int saso_build(rlhip_ctx* c, int64_t d, int64_t m, int nnz, int mode, const uint32_t ctr[4], const uint32_t key[2],
               uint32_t next_ctr[4], SasoOp** out);
int saso_destroy(rlhip_ctx* c, SasoOp* op);
template <typename T>
int saso_dense(rlhip_ctx* c, const SasoOp* op, T* S /* d x m, zeroed here */);
// B (d x n, ldb) = alpha * S[:, row0 : row0 + mloc] * A_loc (mloc x n, lda) + beta * B : the contribution of one row shard
// (the whole product when row0 = 0, mloc = m)
template <typename T>
int saso_apply_rows(rlhip_ctx* c, const SasoOp* op, int64_t n, T alpha, const T* A, int64_t lda, int64_t row0, int64_t mloc, T beta,
                    T* B, int64_t ldb);
template <typename T>
int saso_apply(rlhip_ctx* c, const SasoOp* op, int64_t n, T alpha, const T* A, int64_t lda, T beta, T* B, int64_t ldb);
// B (d x n, ldb) = alpha * S * A + beta * B for a sparse A (m x n) given by the CSR of its transpose
template <typename T>
int saso_apply_csr(rlhip_ctx* c, const SasoOp* op, int64_t n, T alpha, const int64_t* rowptrT, const int64_t* colidxT, const T* valsT, T beta,
                   T* B, int64_t ldb, int64_t row0);
// the same product with the sums of saso_apply on the densified operand (lda = m), bit for bit; 1: not served, take saso_apply_csr
template <typename T>
int saso_apply_csr_ordered(rlhip_ctx* c, const SasoOp* op, int64_t n, T alpha, const int64_t* rowptrT, const int64_t* colidxT, const T* valsT, T beta,
                           T* B, int64_t ldb);
template <typename T>
int col_swap(rlhip_ctx* c, int64_t m, int64_t n, int64_t k, T* A, int64_t lda, const int64_t* idx_dev);
int col_swap_i64(rlhip_ctx* c, int64_t n, int64_t k, int64_t* A, const int64_t* idx_dev);

// ---- qrcp.hip
template <typename T>
int geqp3(rlhip_ctx* c, int64_t m, int64_t n, T* A, int64_t lda, int64_t* jpvt_dev, T* tau_dev);
// pivoted Householder QR restricted to the first `steps` columns, norm down-date in HQRRP's form; jpvt returns the whole permutation (1-based)
template <typename T>
int qrp_partial(rlhip_ctx* c, int64_t m, int64_t n, int64_t steps, T* A, int64_t lda, int64_t* jpvt_dev, T* tau_dev);
// the first `steps` steps of geqp3 itself (LAPACK's norm down-date form)
template <typename T>
int geqp3_steps(rlhip_ctx* c, int64_t m, int64_t n, int64_t steps, T* A, int64_t lda, int64_t* jpvt_dev, T* tau_dev);
template <typename T>
int geqrf(rlhip_ctx* c, int64_t m, int64_t n, T* A, int64_t lda, T* tau_dev);
// lapack::ungqr(m, n, k = n, A, lda, tau): A (m x n, reflectors below the diagonal) <- Q[:, 0:n]
template <typename T>
int ungqr(rlhip_ctx* c, int64_t m, int64_t n, T* A, int64_t lda, const T* tau_dev);

// ---- qr_blk.hip
// Householder QR of the leading n <= m columns of A (m x n, column-major) in the geqrf output format.  Returns 1 when the problem was
// factored here, 0 when it does not fit this kernel (the caller carries on with its other routes), < 0 on error.
template <typename T>
int geqrf_blk(rlhip_ctx* c, int64_t m, int64_t n, T* A, int64_t lda, T* tau_dev);
// Sign-modified LU without pivoting of the n x n matrix A (what lapack::orhr_col runs on the top block of Q): L (unit lower) and U in
// place, D(i) = -sign of the i-th pivot before its modification.  Returns 1 when done here, 0 when the problem does not fit the kernel.
template <typename T>
int lunp_blk(rlhip_ctx* c, int64_t n, T* A, int64_t lda, T* D);

// ---- house.hip
// A (m x n, orthonormal columns) -> V (unit lower trapezoidal, in place), T (nb x n), D (n)
template <typename T>
int orhr_col(rlhip_ctx* c, int64_t m, int64_t n, int64_t nb, T* A, int64_t lda, T* Tm, int64_t ldt, T* D);
// C (m x n) <- Q^T C,  Q = H_1 ... H_k in compact-WY blocks of width nb: V (m x k, unit lower trapezoidal, only the
// strictly lower part is read), T (nb x k).  Side::Left, Op::Trans.
template <typename T>
int gemqrt_lt(rlhip_ctx* c, int64_t m, int64_t n, int64_t k, int64_t nb, const T* V, int64_t ldv, const T* Tm, int64_t ldt,
              T* C, int64_t ldc);
// the same apply for ONE compact-WY block (k reflectors), cut where the first k rows of C are final:
//   head:  W2 = T^T (V1^T C1 + V2^T C2),  C1 -= V1 W2;   tail:  C2 -= V2 W2.   W2 is the caller's k x n buffer (ld k)
template <typename T>
int gemqrt_lt_head(rlhip_ctx* c, int64_t m, int64_t n, int64_t k, const T* V, int64_t ldv, const T* Tm, int64_t ldt, T* C, int64_t ldc, T* W2);
template <typename T>
int gemqrt_lt_tail(rlhip_ctx* c, int64_t m, int64_t n, int64_t k, const T* V, int64_t ldv, const T* W2, T* C, int64_t ldc);
// C (m x n) <- C Q,  Q = I - V T V^T one compact-WY block (V: n x k unit lower trapezoidal, T: k x k upper).  Side::Right, Op::NoTrans
template <typename T>
int gemqrt_rn(rlhip_ctx* c, int64_t m, int64_t n, int64_t k, const T* V, int64_t ldv, const T* Tm, int64_t ldt, T* C, int64_t ldc);
// T (k x k upper, ldt) from V (m x k unit lower trapezoidal) and tau (k): one compact-WY block for all k reflectors
template <typename T>
int larft_gram(rlhip_ctx* c, int64_t m, int64_t k, const T* V, int64_t ldv, const T* tau, T* Tm, int64_t ldt);
// R <- diag(D) R
template <typename T>
int row_sign(rlhip_ctx* c, int64_t n, T* R, int64_t ldr, const T* D);
template <typename T>
int tau_from_t(rlhip_ctx* c, int64_t k, int64_t nb, const T* Tm, int64_t ldt, T* tau);
// returns 1 in *any_host if some |x[i]| > thr
template <typename T>
int any_abs_gt(rlhip_ctx* c, int64_t n, const T* x, T thr, int* any_host);
// geqrf of a tall panel by Cholesky-QR twice + Householder reconstruction (orhr_col); *done = 0: not taken, the caller takes the Householder route
template <typename T>
int geqrf_cholqr(rlhip_ctx* c, int64_t m, int64_t n, T* A, int64_t lda, T* tau, int* done);
// geqrf followed by ungqr(m, n, n) in ONE pass for a tall panel: A <- the first n columns of the Householder Q, R (n x n, ld ldr) <- the
// triangle geqrf would have left (zero below).  *done = 0: not taken (A as geqrf_cholqr leaves it), the caller runs geqrf + ungqr.
template <typename T>
int geqrf_q(rlhip_ctx* c, int64_t m, int64_t n, T* A, int64_t lda, T* R, int64_t ldr, int* done);
template <typename T>
int vrows_explicit(rlhip_ctx* c, int64_t br, int64_t toff, int64_t tcnt, const T* Vtop, int64_t ldv, T* out, int64_t ldo);

// ---- lu.hip
// row-pivoted LU (lapack::getrf) of a tall-skinny matrix on the device
template <typename T>
int getrf(rlhip_ctx* c, int64_t m, int64_t n, T* A, int64_t lda, int64_t* ipiv_dev, int* info_host, int pivots_only);
// lapack::laswp(n, A, lda, k1, k2, ipiv, incx = 1) with 1-based k1..k2
template <typename T>
int laswp(rlhip_ctx* c, int64_t n, T* A, int64_t lda, int64_t k1, int64_t k2, const int64_t* ipiv_dev);
// the pivot post-processing of BQRRP's LU-based qrcp_wide
int luqrcp_piv(rlhip_ctx* c, int64_t sd, int64_t cols, const int64_t* ipiv_dev, int64_t* J_dev);

// ---- lsq.hip
// y = alpha op(A) x + beta y (trans: NoTrans / Trans); the contract is rlhip_gemv_* in include/rlhip.h
template <typename T>
int gemv(rlhip_ctx* c, int trans, int64_t m, int64_t n, T alpha, const T* A, int64_t lda, const T* x, T beta, T* y);
// *out_dev = x^T y by one workgroup in the fixed order of rlhip_normal_matvec_*'s d^T q (n > 0)
template <typename T>
int dot_dev(rlhip_ctx* c, int64_t n, const T* x, const T* y, T* out_dev);

// ---- rpchol.hip
// The kernel function of a positive-definite kernel matrix as the device kernels take it (RLHIP_PDK_*): whether it is a Matern
// kind, and two constants, each computed in double and rounded once to T.  scale = -1 / (2 l^2) for the squared exponential, sqrt(3) / l
// and sqrt(5) / l for Matern 3/2 and 5/2; third = 1 / 3 for Matern 5/2 and 0 otherwise (matern_of_s, rlhip_device.h).
// weight = true (pdk_weight_fn alone): the Matern kinds' gradient weight u(s) in place of the kernel, pdk_weight_of_s(s, scale, third) with
// third = lin; the squared exponential's u is its kernel, so its weight form is its value form.
template <typename T>
struct PdkFn {
    bool matern;
    T scale, third;
    bool weight = false;
};
inline bool pdk_kind_ok(int kernel) { return kernel >= RLHIP_PDK_SQEXP && kernel <= RLHIP_PDK_MATERN52; }
template <typename T>
PdkFn<T> pdk_fn(int kernel, T bandwidth) {
    const double l = (double)bandwidth;
    if (kernel == RLHIP_PDK_SQEXP) return {false, (T)(-1.0 / (2.0 * l * l)), T(0)};
    if (kernel == RLHIP_PDK_MATERN32) return {true, (T)(1.7320508075688772 / l), T(0)};             // sqrt(3), correctly rounded
    return {true, (T)(2.23606797749979 / l), (T)(1.0 / 3.0)};                                         // sqrt(5), correctly rounded
}
// the gradient weight of a kernel function: u(s) as a PdkFn, and in *w0 the factor w(0) = -1 / l^2, -3 / l^2, -5 / (3 l^2)
template <typename T>
PdkFn<T> pdk_weight_fn(int kernel, T bandwidth, T* w0) {
    const double l = (double)bandwidth;
    if (kernel == RLHIP_PDK_SQEXP) { *w0 = (T)(-1.0 / (l * l)); return {false, (T)(-1.0 / (2.0 * l * l)), T(0), false}; }
    if (kernel == RLHIP_PDK_MATERN32) { *w0 = (T)(-3.0 / (l * l)); return {true, (T)(1.7320508075688772 / l), T(0), true}; }
    *w0 = (T)(-5.0 / (3.0 * l * l));
    return {true, (T)(2.23606797749979 / l), T(1), true};
}
// nr[j] = |X(:, j)|^2 for cols points, and K(i, j) <- f((nr_rows[i] + nr_cols[j]) + K(i, j)) on a rows x cols block that holds -2 z_i^T x_j
// (cols <= 65535), f the kernel function: the two kernels of the norm-expansion submatrix, for the two-point-set routines of rbf.hip
template <typename T>
int sqexp_colnorms(rlhip_ctx* c, int64_t rows_x, int64_t cols, const T* X, int64_t ldx, T* nr);
template <typename T>
int pdk_epilogue(rlhip_ctx* c, int64_t rows, int64_t cols, const T* nr_rows, const T* nr_cols, PdkFn<T> f, T* K, int64_t ldk);
// the norms of two point sets in one block of ws: (*nr)[i] = |Z(:, i)|^2 for i < mz, (*nr)[mz + j] = |X(:, j)|^2 for j < nx
template <typename T>
int pdk_pair_norms(rlhip_ctx* c, ws_scope& ws, int64_t rows_x, int64_t mz, const T* Z, int64_t ldz, int64_t nx, const T* X, int64_t ldx, T** nr) {
    *nr = ws.alloc<T>((size_t)(mz + nx));
    if (!*nr) return RLHIP_ERR_HIP(hipErrorOutOfMemory);
    const int rc = sqexp_colnorms<T>(c, rows_x, mz, Z, ldz, *nr);
    return rc ? rc : sqexp_colnorms<T>(c, rows_x, nx, X, ldx, *nr + mz);
}
// rows per block of a product that goes through the scratch arena one row block (rows x cols) at a time: a block holds at most 2^26
// entries (one row when cols > 2^26), a multiple of 256 rows where that is at least 256, and no more than the mz rows there are
inline int64_t pdk_row_block(int64_t cols, int64_t mz) {
    const int64_t rb = ((int64_t)1 << 26) / cols;
    const int64_t r = rb < 1 ? 1 : (rb >= 256 ? (rb / 256) * 256 : rb);
    return r > mz ? mz : r;
}

// ---- rbf.hip
// rlhip_pdk_cross_apply_* behind its argument checks, for mz, n, nx > 0 and alpha != 0, with the scalar function as a PdkFn: the kernel
// functions for the public entries, a gradient weight for rbf_grad.hip.  It picks its fused or row-block route and counts it as they do;
// a weight form is never split over X.
template <typename T>
int pdk_cross_apply_fn(rlhip_ctx* c, int64_t rows_x, int64_t mz, const T* Z, int64_t ldz, int64_t nx, const T* X, int64_t ldx, PdkFn<T> f, int64_t n,
                       T alpha, const T* B, int64_t ldb, T beta, T* C, int64_t ldc);

}  // namespace rlhip
