"""Cases of test_gpu_sketch_sparse.py and a plain-Python replay of the host-side route decisions of sketch.hip and sparse.hip.

Routes and their counters (rlhip_path_count; one count per call, on the host where the launch is enqueued):

  saso_build (mode 1)   lds      T > 0, nnz <= 8 and 4 d (3 + 2 nnz) <= 144 KiB: saso_ind_block_kernel                          36
                        chain    otherwise, T > 0: generate / scan / scatter / sort                                           37
  saso_apply_rows       dma      mode 1 with 16-bit lists, n % 4 == 0, d <= 1280, d, lda, A and the first whole block 16-byte
                                 aligned, at least 8 whole blocks: saso_apply_dma_kernel<T, 5, NJ, DD>                        14
                        staged   everything else, and the ragged first / last block of a dma call: saso_apply_kernel<T, CT, mode, NR>
                                 33; CT = 2: + 34; CT = 1: + 35 (CT = 4 / 2 / 1 columns per slab while d x CT fits 160 KiB)
                        refused  a one-column slab does not fit: -2, nothing counted
                        empty    the shard holds no rows: B = beta B, nothing counted
  csr_spmm              wide     nc > 32: csr_spmm_rm_kernel<T, 1 / 2 / 4> (layout 'C' through two transposes)                38
                        narrow   nc <= 32: layout 'R' csr_spmm_rm_narrow_kernel<T, 16 / 32>                                   39
                                           layout 'C' csr_spmm_cmout_narrow_kernel<T, 16 / 32>                                40
  csr_transpose         sort     no transposed row longer than 512 entries: scatter by entry number + per-row sort            41
                        count    otherwise: stable counting sort over chunks                                                  42

Exact cases: operands hold integers |x| <= 8, alpha = 2 (alpha is one of 2, -1, 0.5), beta is one of 0, 1, -0.5 and the entries of S are
+-1.  Every product is an integer, every partial sum of any subset of them an integer bounded by |S| |A| (resp. |A_csr| |B|), and the
result a multiple of 1/2 bounded by |alpha| (|S| |A|) + |beta| |B0|.  test_sketch_sparse_cases.py checks on the reference alone that this
bound stays below 2^24 (fp32) / 2^53 (fp64) -- the largest here is below 2^14, so the halves fit too -- hence EVERY order of summation
gives the bits of the float64 reference and the GPU comparison needs no tolerance."""
import functools
from dataclasses import dataclass, field

import numpy as np
import scipy.sparse as sp

SIZEOF = {"f64": 8, "f32": 4}
NPDT = {"f64": np.float64, "f32": np.float32}
UINT = {"f64": np.uint64, "f32": np.uint32}
PRECS = ("f64", "f32")
BITS = {"f64": 53, "f32": 24}
DMA, STAGED, SLAB2, SLAB1, BUILD_LDS, BUILD_CHAIN, SPMM_WIDE, SPMM_NARROW_RM, SPMM_NARROW_CM, CT_SORT, CT_COUNT = 14, 33, 34, 35, 36, 37, 38, 39, 40, 41, 42
COUNTERS = (DMA, STAGED, SLAB2, SLAB1, BUILD_LDS, BUILD_CHAIN, SPMM_WIDE, SPMM_NARROW_RM, SPMM_NARROW_CM, CT_SORT, CT_COUNT)
ENTRY_MAX = 8
ALPHAS, BETAS = (2.0, -1.0, 0.5), (0.0, 1.0, -0.5)
ALPHA, BETA = 2.0, -0.5
CTR, KEY = (0xFFFFFFF0, 3, 0, 0), (5, 9)          # (the low counter word carries into the next one inside every operator)
LDS_CAP = 160 * 1024


def _cdiv(a, b):
    return -(-a // b)


def ints(rng, *shape):
    return rng.integers(-ENTRY_MAX, ENTRY_MAX + 1, shape).astype(np.float64)


def nonzero_ints(rng, n):
    return (rng.integers(1, ENTRY_MAX + 1, n) * rng.choice((-1, 1), n)).astype(np.float64)


def gauss(rng, prec, *shape):
    return rng.standard_normal(shape).astype(NPDT[prec]).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------------------------------
# replay of the host-side decisions
# ---------------------------------------------------------------------------------------------------------------------------------------
def build_replay(d, m, nnz, mode):
    """saso_build -> (route name, counter deltas, the operator keeps 16-bit lists)"""
    T = _cdiv(m, d)
    if mode == 0:
        return "affine", {}, False
    has16 = d <= 32768
    if T == 0:
        return "none", {}, has16
    if nnz <= 8 and 4 * d * (3 + 2 * nnz) <= 144 * 1024:
        return "lds", {BUILD_LDS: 1}, has16
    return f"chain:{8 if nnz <= 8 else 128}", {BUILD_CHAIN: 1}, has16


@dataclass
class ApplyRoute:
    rc: int = 0
    sig: str = ""
    counts: dict = field(default_factory=dict)
    CT: int = 0                  # columns per slab
    NR: int = 0                  # sketch rows per thread and pass
    passes: int = 0              # row passes (launches) of the register-staged kernel
    NJ: object = None            # pieces per wave of the LDS-DMA kernel: 5, 10 or "1280" (the specialised instantiation)
    head: int = 0
    tail: int = 0


def apply_replay(prec, mode, d, m, n, row0=0, mloc=None, lda=None, ldb=None, a_off=0):
    """saso_apply_rows.  a_off: elements between a 16-byte aligned address and the operand pointer."""
    sz = SIZEOF[prec]
    mloc = m if mloc is None else mloc
    lda = max(mloc, 1) if lda is None else lda
    ldb = d if ldb is None else ldb
    r = ApplyRoute()
    if n <= 0:
        r.sig = "nothing"
        return r
    if row0 < 0 or mloc < 0 or row0 + mloc > m or lda < max(mloc, 1):
        r.rc, r.sig = -6, "argument"
        return r
    if ldb < d:
        r.rc, r.sig = -9, "argument"
        return r
    tb0, tb1 = (row0 // d, _cdiv(row0 + mloc, d)) if mloc > 0 else (0, 0)
    CT = 4 if sz * d * 4 <= LDS_CAP else 2 if sz * d * 2 <= LDS_CAP else 1
    if sz * d * CT > LDS_CAP:
        r.rc, r.sig = -2, "refused"
        return r
    r.CT = CT
    if tb1 == tb0:
        r.sig = "empty"
        return r
    fb0 = _cdiv(row0, d)
    fb1 = max((row0 + mloc) // d, fb0)
    nfb = fb1 - fb0
    slab2 = 2 * ((4 * d * sz + 1023) // 1024 * 1024)
    has16 = mode == 1 and d <= 32768
    dma = (has16 and CT == 4 and n % 4 == 0 and d <= 1280 and (d * sz) % 16 == 0 and (lda * sz) % 16 == 0 and (a_off * sz) % 16 == 0
           and ((fb0 * d - row0) * sz) % 16 == 0 and slab2 <= LDS_CAP and sz * (4 * lda + d) < 2 ** 32 and nfb >= 8)
    r.NR = 5 if d <= 1280 else 8
    r.passes = _cdiv(d, 256 * r.NR)
    if dma:
        r.head, r.tail = fb0 - tb0, tb1 - fb1
        nchunks = _cdiv(4 * d * sz // 16, 64)
        nj = _cdiv(nchunks, 4)
        r.NJ = "1280" if d == 1280 and sz == 8 else 5 if nj <= 5 else 10
        r.counts = {DMA: 1}
        if r.head or r.tail:
            r.counts[STAGED] = 1
        r.sig = f"dma:{r.NJ}" + ("+head" if r.head else "") + ("+tail" if r.tail else "")
        return r
    r.counts = {STAGED: 1}
    if CT == 2:
        r.counts[SLAB2] = 1
    if CT == 1:
        r.counts[SLAB1] = 1
    r.sig = f"staged:ct{CT}:nr{r.NR}x{r.passes}"
    return r


def apply_csr_replay(d, m, n, row0=0, ldb=None):
    """saso_apply_csr -> return code (it has one kernel and no counter)"""
    if row0 < 0 or row0 > m:
        return -6
    if n <= 0:
        return 0
    if (d if ldb is None else ldb) < d:
        return -9
    return -2 if 8 * d > 150 * 1024 else 0


def spmm_replay(layout, nrows, nc):
    if nrows <= 0 or nc <= 0:
        return "nothing", {}
    if nc <= 32:
        w = 16 if nc <= 16 else 32
        return (f"narrow-cm:{w}", {SPMM_NARROW_CM: 1}) if layout == "C" else (f"narrow-rm:{w}", {SPMM_NARROW_RM: 1})
    return f"wide:{4 if nc > 128 else 2 if nc > 64 else 1}", {SPMM_WIDE: 1}


def transpose_replay(k, colidx):
    """-> (route, counter deltas, the longest transposed row)"""
    if len(colidx) == 0 or k == 0:
        return "nothing", {}, 0
    longest = int(np.bincount(colidx, minlength=k).max())
    return ("sort", {CT_SORT: 1}, longest) if longest <= 512 else ("count", {CT_COUNT: 1}, longest)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the sketching operator
# ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=6)
def sketch_operator(d, m, nnz, mode):
    """the oracle's restatement of the stream (oracle.saso_dense) as a scipy CSR matrix (d x m, entries +-1) and the state after it"""
    import oracle

    S, nxt = oracle.saso_dense(d, m, nnz, CTR, KEY, mode)
    return sp.csr_matrix(S), tuple(nxt)


@dataclass
class Gen:
    name: str
    d: int
    m: int
    nnz: int
    route: str                   # mode 1; mode 0 builds its closed-form tables (no counter)


GEN = [
    Gen("maxnz-8", 64, 300, 8, "lds"),                    # MAXNZ 8 / 128 and the LDS-build / chain split
    Gen("maxnz-9", 64, 300, 9, "chain:128"),
    Gen("lds-gate-3351", 3351, 3351 + 50, 4, "lds"),      # 4 d (3 + 2 nnz) = 147444 <= 147456
    Gen("lds-gate-3352", 3352, 3352 + 50, 4, "chain:8"),  # 147488
    Gen("all-rows", 128, 300, 128, "chain:128"),          # d = nnz: every column is full
    Gen("no-16-bit-lists", 40960, 37, 2, "chain:8"),
    Gen("m0", 64, 0, 4, "none"),
]
GEN_BY_NAME = {g.name: g for g in GEN}


@dataclass
class Apply:
    name: str
    prec: str
    mode: int
    d: int
    m: int
    n: int
    nnz: int
    sig: str                     # the route the whole-operand call is listed under (apply_replay(...).sig)
    lda_pad: int = 3             # guard rows of NaN under A (lda = m + lda_pad) and under B
    ldb_pad: int = 2
    a_off: int = 0               # the operand pointer sits this many elements behind a 16-byte aligned address
    cuts: tuple = ()             # row shards [cuts[i], cuts[i + 1]) through rlhip_saso_apply_rows_*, each holding only its rows
    shard_sigs: tuple = ()
    whole: bool = True           # run the whole-operand call
    kind: str = "exact"          # "exact" | "rounded"
    seed: int = 0

    def lda(self, rows=None):
        return max((self.m if rows is None else rows) + self.lda_pad, 1)

    def ldb(self):
        return self.d + self.ldb_pad

    def route(self, r0=None, r1=None):
        if r0 is None:
            return apply_replay(self.prec, self.mode, self.d, self.m, self.n, 0, self.m, self.lda(), self.ldb(), self.a_off)
        return apply_replay(self.prec, self.mode, self.d, self.m, self.n, r0, r1 - r0, self.lda(r1 - r0), self.ldb(), self.a_off)

    def operands(self):
        """-> A (m x n), B0 (d x n) in float64, representable in the case's type"""
        rng = np.random.default_rng(self.seed)
        if self.kind == "exact":
            return ints(rng, self.m, self.n), ints(rng, self.d, self.n)
        return gauss(rng, self.prec, self.m, self.n), gauss(rng, self.prec, self.d, self.n)


def _thirds(m, align=2):
    """three shards with cuts inside blocks, multiples of `align`"""
    return (0, (m // 3) // align * align, (2 * m // 3 + 2) // align * align, m)


def _build_apply():
    cs = []

    def add(name, prec, mode, d, m, n, nnz, sig, **kw):
        cs.append(Apply(f"{name}-{prec}-mode{mode}", prec, mode, d, m, n, nnz, sig, seed=len(cs) + 1, **kw))

    for p in PRECS:
        for mode in (1, 0):
            # ---- small shapes (guard rows: lda = m + 4, a multiple of 16 bytes where m is; the first one reaches the LDS-DMA kernel in mode 1)
            add("small-40x1000x16", p, mode, 40, 1000, 16, 4, "dma:5" if mode == 1 else "staged:ct4:nr5x1", lda_pad=4)
            add("small-25x333x9", p, mode, 25, 333, 9, 2, "staged:ct4:nr5x1")
            add("small-1x5x2", p, mode, 1, 5, 2, 1, "staged:ct4:nr5x1")
            add("small-7x50x3", p, mode, 7, 50, 3, 7, "staged:ct4:nr5x1")
            add("small-48x300x4", p, mode, 48, 300, 4, 12, "staged:ct4:nr5x1")
            add("small-2600-two-passes", p, mode, 2600, 3 * 2600 + 11, 5, 3, "staged:ct4:nr8x2")
            # ---- slab thresholds: 4 / 2 / 1 columns while d x CT elements fit 160 KiB, then -2
            e = 1 if p == "f64" else 2
            for d, ct in ((5120 * e, 4), (5120 * e + 1, 2), (10240 * e, 2), (10240 * e + 1, 1), (20480 * e, 1), (20480 * e + 1, 0)):
                add(f"slab-d{d}", p, mode, d, 37, 5, 2, f"staged:ct{ct}:nr8x{_cdiv(d, 2048)}" if ct else "refused")
            # ---- row shards off the LDS-DMA route, cuts inside blocks
            if mode == 0:
                m = 96 * 12 + 10
                add("shards-d96", p, 0, 96, m, 12, 3, "staged:ct4:nr5x1", cuts=_thirds(m), shard_sigs=("staged:ct4:nr5x1",) * 3)
            else:
                m = 3 * 2600 + 11
                add("shards-d2600", p, 1, 2600, m, 5, 3, "staged:ct4:nr8x2", cuts=_thirds(m), shard_sigs=("staged:ct4:nr8x2",) * 3)
            # ---- an operator without columns: B = beta B
            add("m0", p, mode, 40, 0, 5, 4, "empty")

        # ---- the LDS-DMA route: whole operand (nine whole blocks and a ragged one), and three shards with even cuts inside blocks (two or
        #      three whole blocks each: below the route's gate of eight, so the shards take the register-staged kernel)
        nj = {640: 5, 642: 10, 1278: 10, 1280: "1280"} if p == "f64" else {44: 5, 1276: 5, 1280: 5}
        for d, NJ in nj.items():
            for n in (4, 12):
                m = 9 * d + 6
                add(f"dma-d{d}-n{n}", p, 1, d, m, n, 8 if d < 1000 else 4, f"dma:{NJ}+tail", lda_pad=2, cuts=_thirds(m),
                    shard_sigs=(f"staged:ct4:nr5x{_cdiv(d, 1280)}",) * 3)
        # shards long enough to take the route themselves, with a ragged head and a ragged tail (cuts: multiples of 16 bytes)
        if p == "f64":
            add("dma-shards", p, 1, 96, 30 * 96 + 6, 4, 4, "dma:5+tail", lda_pad=2, cuts=(0, 1000, 1924, 30 * 96 + 6),
                shard_sigs=("dma:5+tail", "dma:5+head+tail", "dma:5+head+tail"))
        else:
            add("dma-shards", p, 1, 44, 30 * 44 + 8, 4, 4, "dma:5+tail", lda_pad=4, cuts=(0, 444, 888, 30 * 44 + 8),
                shard_sigs=("dma:5+tail", "dma:5+head+tail", "dma:5+head+tail"))

        # ---- each gate of the route missed alone, next to dma-d640-n4 / dma-d44-n4
        d = 640 if p == "f64" else 44
        m = 9 * d + 6
        G = dict(lda_pad=2)
        add("gate-n6", p, 1, d, m, 6, 8, "staged:ct4:nr5x1", **G)
        add("gate-7-blocks", p, 1, d, 7 * d, 4, 8, "staged:ct4:nr5x1", lda_pad=4)
        add("gate-8-blocks", p, 1, d, 8 * d, 4, 8, "dma:5", lda_pad=4)                       # (the other side: exactly eight, no ragged block)
        add("gate-pointer-offset", p, 1, d, m, 4, 8, "staged:ct4:nr5x1", a_off=1, **G)
        add("gate-mode0", p, 0, d, m, 4, 8, "staged:ct4:nr5x1", **G)
        if p == "f64":
            add("gate-lda-odd", p, 1, d, m, 4, 8, "staged:ct4:nr5x1", lda_pad=1)
            add("gate-d641", p, 1, 641, 9 * 641 + 6, 4, 8, "staged:ct4:nr5x1", lda_pad=3)      # (lda = 9 * 641 + 9: even)
            add("gate-d1282", p, 1, 1282, 9 * 1282 + 6, 4, 4, "staged:ct4:nr8x1", **G)
            # a shard whose first whole block starts an odd number of elements into it: row 1 .. m
            add("gate-odd-block-start", p, 1, d, m, 4, 8, "staged:ct4:nr5x1", whole=False, lda_pad=3, cuts=(1, m), shard_sigs=("staged:ct4:nr5x1",))
            add("gate-even-block-start", p, 1, d, m, 4, 8, "dma:5+tail", whole=False, cuts=(2, m), shard_sigs=("dma:5+head+tail",), **G)
        else:
            add("gate-lda-2-mod-4", p, 1, d, m, 4, 8, "staged:ct4:nr5x1", lda_pad=0)
            add("gate-d1284", p, 1, 1284, 9 * 1284 + 6, 4, 4, "staged:ct4:nr8x1", **G)
            add("gate-d46", p, 1, 46, 9 * 46 + 6, 4, 8, "staged:ct4:nr5x1", lda_pad=0)        # (46 * 4 bytes is no multiple of 16; lda = 420 is)
    # ---- one rounded case: Gaussian operands in fp32 against the entrywise bound
    add("rounded-1280", "f32", 1, 1280, 9 * 1280 + 6, 8, 4, "dma:5+tail", lda_pad=2, kind="rounded")
    return cs


APPLY = _build_apply()
APPLY_BY_NAME = {c.name: c for c in APPLY}
assert len(APPLY_BY_NAME) == len(APPLY)


# ---------------------------------------------------------------------------------------------------------------------------------------
# S * A for a sparse A
# ---------------------------------------------------------------------------------------------------------------------------------------
@dataclass
class ApplyCsr:
    name: str
    prec: str
    mode: int
    d: int
    m: int = 1500
    n: int = 40
    nnz: int = 4
    rc: int = 0
    ldb_pad: int = 3
    seed: int = 0

    def matrix(self):
        """integer-valued sparse A (m x n) as the CSR of its transpose: columns 10 .. 12 empty, column 20 with 300 entries (more than the
        256 threads of its workgroup), about 30 in the others; source rows ascending inside a column -> (rowptrT, colidxT, valsT, dense A)"""
        rng = np.random.default_rng(1000 + self.seed)
        m, n = self.m, self.n
        lens = rng.integers(20, 41, n)
        if n > 20:
            lens[10:13] = 0
            lens[20] = 300
        lens = np.minimum(lens, m)
        rowptr = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
        colidx = np.concatenate([np.sort(rng.choice(m, int(L), replace=False)) for L in lens] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
        vals = nonzero_ints(rng, int(rowptr[-1]))
        A = np.zeros((m, n))
        A[colidx, np.repeat(np.arange(n), lens)] = vals
        return rowptr, colidx, vals, A

    def b0(self):
        return ints(np.random.default_rng(2000 + self.seed), self.d, self.n)


def _build_apply_csr():
    cs = []
    for p in PRECS:
        for mode in (1, 0):
            for d in (120, 2000):
                cs.append(ApplyCsr(f"d{d}-{p}-mode{mode}", p, mode, d, seed=len(cs)))
            cs.append(ApplyCsr(f"d19200-{p}-mode{mode}", p, mode, 19200, m=37, n=3, nnz=2, seed=len(cs)))
            cs.append(ApplyCsr(f"d19201-{p}-mode{mode}", p, mode, 19201, m=37, n=3, nnz=2, rc=-2, seed=len(cs)))
    return cs


APPLY_CSR = _build_apply_csr()
APPLY_CSR_BY_NAME = {c.name: c for c in APPLY_CSR}


# ---------------------------------------------------------------------------------------------------------------------------------------
# CSR products
# ---------------------------------------------------------------------------------------------------------------------------------------
ROW_LENGTHS = (0, 1, 2, 3, 4, 5, 7, 63, 64, 65, 127, 128, 129, 200)
SPMM_NC = (1, 16, 17, 32, 33, 64, 65, 128, 129, 257)


@dataclass
class Spmm:
    name: str
    prec: str
    layout: str
    nc: int
    sig: str
    shape: str = "std"           # "std" 150 x 40 | "k1" 150 x 1 | "nnz0" 150 x 40 without entries | "tall" 70001 x 40, one entry per row
    kind: str = "exact"
    seed: int = 0

    def matrix(self):
        """-> m, k, rowptr, colidx, vals (float64, representable in the case's type).  "std": rows of ROW_LENGTHS entries, once in that order,
        122 rows of 0 .. 9 entries, once reversed; columns drawn with replacement and left unsorted (k = 40 forces duplicates in the long rows)"""
        rng = np.random.default_rng(3000 + self.seed)
        k = 1 if self.shape == "k1" else 40
        if self.shape == "tall":
            lens = np.ones(70001, dtype=np.int64)
        else:
            lens = np.concatenate((ROW_LENGTHS, rng.integers(0, 10, 122), ROW_LENGTHS[::-1])).astype(np.int64)
            if self.shape == "nnz0":
                lens[:] = 0
        m, nnz = len(lens), int(lens.sum())
        rowptr = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
        colidx = rng.integers(0, k, nnz).astype(np.int64)
        vals = nonzero_ints(rng, nnz) if self.kind == "exact" else gauss(rng, self.prec, nnz)
        return m, k, rowptr, colidx, vals

    def operands(self, m, k):
        rng = np.random.default_rng(4000 + self.seed)
        if self.kind == "exact":
            return ints(rng, k, self.nc), ints(rng, m, self.nc)
        return gauss(rng, self.prec, k, self.nc), gauss(rng, self.prec, m, self.nc)


def csr_dense(m, k, rowptr, colidx, vals):
    """dense copy, duplicates summed"""
    A = np.zeros((m, k))
    np.add.at(A, (np.repeat(np.arange(m), np.diff(rowptr)), colidx), vals)
    return A


def _build_spmm():
    cs = []
    for p in PRECS:
        for layout in "CR":
            for nc in SPMM_NC:
                cs.append(Spmm(f"std-{layout}-nc{nc}-{p}", p, layout, nc, "", seed=len(cs)))
            cs.append(Spmm(f"k1-{layout}-nc17-{p}", p, layout, 17, "", shape="k1", seed=len(cs)))
            cs.append(Spmm(f"k1-{layout}-nc65-{p}", p, layout, 65, "", shape="k1", seed=len(cs)))
            cs.append(Spmm(f"nnz0-{layout}-nc16-{p}", p, layout, 16, "", shape="nnz0", seed=len(cs)))
            cs.append(Spmm(f"nnz0-{layout}-nc33-{p}", p, layout, 33, "", shape="nnz0", seed=len(cs)))
        cs.append(Spmm(f"tall-R-nc33-{p}", p, "R", 33, "", shape="tall", seed=len(cs)))
    cs.append(Spmm("rounded-C-nc33-f32", "f32", "C", 33, "", kind="rounded", seed=len(cs)))
    cs.append(Spmm("rounded-R-nc33-f32", "f32", "R", 33, "", kind="rounded", seed=len(cs)))
    # the routes the cases are listed under, written out: by layout and width
    listed = {("C", 1): "narrow-cm:16", ("C", 16): "narrow-cm:16", ("C", 17): "narrow-cm:32", ("C", 32): "narrow-cm:32",
              ("R", 1): "narrow-rm:16", ("R", 16): "narrow-rm:16", ("R", 17): "narrow-rm:32", ("R", 32): "narrow-rm:32"}
    for lay in "CR":
        listed.update({(lay, 33): "wide:1", (lay, 64): "wide:1", (lay, 65): "wide:2", (lay, 128): "wide:2", (lay, 129): "wide:4", (lay, 257): "wide:4"})
    for c in cs:
        c.sig = listed[(c.layout, c.nc)]
    return cs


SPMM = _build_spmm()
SPMM_BY_NAME = {c.name: c for c in SPMM}
assert len(SPMM_BY_NAME) == len(SPMM)


# ---------------------------------------------------------------------------------------------------------------------------------------
# CSR transposes and dense column blocks
# ---------------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Transpose:
    name: str
    m: int
    k: int
    route: str
    long_cols: dict              # column -> exact number of entries
    fill: int = 10               # the other columns hold 0 .. fill entries
    seed: int = 0

    def matrix(self):
        """-> rowptr, colidx, vals (1, 2, 3, ... in entry order: distinct, so the order of duplicates shows).  Entries are dealt to random
        rows (with replacement: duplicate (row, column) pairs), column indices inside a row stay unsorted."""
        rng = np.random.default_rng(5000 + self.seed)
        clen = rng.integers(0, self.fill + 1, self.k)
        for j, L in self.long_cols.items():
            clen[j] = L
        cols = rng.permutation(np.repeat(np.arange(self.k), clen))
        rows = np.sort(rng.integers(0, self.m, len(cols)))
        rowptr = np.concatenate(([0], np.cumsum(np.bincount(rows, minlength=self.m)))).astype(np.int64)
        return rowptr, cols.astype(np.int64), np.arange(1, len(cols) + 1, dtype=np.float64)


def transpose_reference(m, k, rowptr, colidx, vals):
    """the stable sort of the entries by column: source rows ascending inside a transposed row, duplicates in source-entry order"""
    rowid = np.repeat(np.arange(m, dtype=np.int64), np.diff(rowptr))
    perm = np.argsort(colidx, kind="stable")
    rowptrT = np.concatenate(([0], np.cumsum(np.bincount(colidx, minlength=k)))).astype(np.int64)
    return rowptrT, rowid[perm], vals[perm]


TRANSPOSE = [
    Transpose("rows-16-17", 60, 40, "sort", {3: 16, 4: 17, 39: 16, 0: 17}),                     # LDS strip / in place
    Transpose("row-512", 600, 30, "sort", {7: 512}),
    Transpose("row-513", 600, 30, "count", {7: 513}),
    Transpose("m1", 1, 700, "sort", {}, fill=14),                                               # ~5000 entries, one source row
    Transpose("m1-long", 1, 5, "count", {j: 1000 for j in range(5)}),
    Transpose("k1", 50, 1, "sort", {0: 75}),
    Transpose("k1-long", 600, 1, "count", {0: 600}),
]
for _i, _t in enumerate(TRANSPOSE):
    _t.seed = _i
TRANSPOSE_BY_NAME = {t.name: t for t in TRANSPOSE}


def densify_matrix():
    """the CSR of a 12 x 70 transpose (columns of a 70 x 12 matrix): empty columns, one of 300 entries (duplicates forced, more than one trip
    of the kernel's 256 threads), duplicates elsewhere -> rowptrT, colidxT, valsT, m"""
    rng = np.random.default_rng(6000)
    m, lens = 70, np.array([0, 5, 0, 300, 3, 0, 17, 64, 1, 0, 130, 9])
    rowptr = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    colidx = rng.integers(0, m, int(lens.sum())).astype(np.int64)
    return rowptr, colidx, nonzero_ints(rng, int(lens.sum())), m


# ---------------------------------------------------------------------------------------------------------------------------------------
# rounded cases
# ---------------------------------------------------------------------------------------------------------------------------------------
def rounded_bound(L, alpha, abs_terms, beta, c0):
    """(L + 3) 2^-24 (|alpha| sum |terms| + |beta c0|): L products of one output element summed in any order (L - 1 additions), alpha, beta c0
    and the last addition, in fp32 (unit round-off 2^-24), to first order with one unit to spare for the higher-order terms"""
    return (L + 3) * 2.0 ** -24 * (abs(alpha) * abs_terms + np.abs(beta * c0))
