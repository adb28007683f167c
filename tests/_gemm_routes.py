"""Cases of test_gpu_gemm.py and a plain-Python replay of the route decisions gemm.hip::gemm_impl takes on them.

gemm_impl picks a kernel from the shapes, the transposes, the alignment of the operands and the context's avoid_persistent switch alone:

  scale    k == 0 or alpha == 0                                             C = beta C                    counter 30
  skinny   op(A) = A^T, op(B) = B, m, n <= 64, k >= 8192                    gemm_tn_skinny_kernel         counter 29
  cut      the contraction is cut by gemm_impl itself and the pieces come back through it                 counter 31
             k-remainder peel: k % 16 (fp64) / k % 32 (fp32) != 0, k >= 1024, n % 256 == 0
             fp32 chunks of 16384 (k > 16384, n % 256 == 0) and their Gram twin
  sk       the persistent stream-K kernel (gemm_sk.hip::gemm_streamk)                                     counter 0 (fp64) / 1 (fp32)
  mpeel    sk on the first (m / 128) * 128 rows, the other rows back through gemm_impl                    counter 32
  small    m, n <= 512, k <= 2048, m n >= 1024, no tri                      gemm_small_kernel             counter 28
  tiled    everything else: gemm_kernel in one of four tile shapes          (+ split-K slabs: 27)         counter 26

`replay` returns the counter deltas, a signature string that names the kernels in launch order (tile shape, vector or scalar loads,
split-K), and the smallest factor by which a CONTINUOUS gate on the way was cleared: the stream-K work gate ntiles * ktiles >= 64 * 256 and
the split-K time model.  test_gemm_routes.py holds every case to the signature it is listed under with a factor >= 2; the integer gates
are hit on both sides on purpose.

Exact cases: A, B, C0 hold integers |x| <= 4, alpha = 2 and beta is 0, 1 or -0.5.  Every product is an integer <= 16, every partial sum
of any subset of them an integer <= 16 k, and the result a multiple of 1/2 below 32 k + 2: with k < 2^17 all of these fit the 24-bit
significand of fp32 (and the 53 bits of fp64), so EVERY order of summation -- split-K slabs, stream-K fix-up, chunk accumulation, fused or
unfused multiply-add -- gives the same bits as the float64 reference, and the comparison needs no tolerance."""
import math
from dataclasses import dataclass, field

import numpy as np

NUM_CU = 256
SIZEOF = {"f64": 8, "f32": 4}
NPDT = {"f64": np.float64, "f32": np.float32}
SK = {"f64": 0, "f32": 1}
TILED, SPLITK, SMALL, SKINNY, SCALE, CUT, MPEEL = 26, 27, 28, 29, 30, 31, 32
COUNTERS = (0, 1, TILED, SPLITK, SMALL, SKINNY, SCALE, CUT, MPEEL)
ENTRY_MAX = 4                    # |a_ij|, |b_ij|, |c_ij| of the exact cases


def _cdiv(a, b):
    return -(-a // b)


@dataclass
class Route:
    counts: dict = field(default_factory=dict)
    margin: float = math.inf
    leaves: list = field(default_factory=list)
    sig: str = ""

    def count(self, which):
        self.counts[which] = self.counts.get(which, 0) + 1

    def gate(self, factor):
        self.margin = min(self.margin, factor)


def tiled_plan(prec, m, n, k, tri):
    """gemm_dispatch: -> (bm, bn, splitk, margin of the split / no split decision)"""
    sz, BK = SIZEOF[prec], 16
    if n > 128 and not tri:
        bm, bn = 128, 128
    elif n > 64 or tri:
        bm, bn = 128, 128
    elif n > 32:
        bm, bn = 256, 64
    elif n > 16:
        bm, bn = 256, 32
    else:
        bm, bn = 256, 16
    tiles = _cdiv(m, bm) * _cdiv(n, bn)
    if tri:
        tn = _cdiv(n, bn)
        tiles = tn * (tn + 1) // 2
    ktiles = _cdiv(k, BK)
    slots = NUM_CU * 2
    flops_cu = 78.6e12 / slots * (2.0 if sz == 4 else 1.0)
    t_tile_k = 2.0 * bm * bn * BK / flops_cu
    maxs = min(ktiles // (8 if tiles <= 8 else 32), 256)
    best, splitk, t1, t_split = 1e300, 1, None, math.inf
    for s in range(1, max(maxs, 1) + 1):
        kc = _cdiv(ktiles, s)
        se = _cdiv(ktiles, kc)
        rounds = _cdiv(tiles * se, slots)
        t = rounds * (kc * t_tile_k + 2e-6)
        if se > 1:
            t += 2.0 * se * float(m) * n * sz / 4.0e12 + 3e-6
        if float(se) * m * n * sz > 8e9:
            continue
        if se == 1:
            t1 = t if t1 is None else t1
        else:
            t_split = min(t_split, t)
        if t < best * 0.97:
            best, splitk = t, se
    kchunk = _cdiv(ktiles, splitk) * BK
    splitk = max(_cdiv(k, kchunk), 1)
    margin = (t1 / best) if splitk > 1 else (t_split / t1)
    return bm, bn, splitk, margin


def _sk_takes(r, prec, tb, m, n, k, tri, aligned, lda, ldb, avoid):
    """gemm_sk.hip::gemm_streamk's gates"""
    BK, EPP = (16, 2) if prec == "f64" else (32, 4)
    if tb or avoid:
        return False
    if prec == "f32" and k > 16384:
        return False
    if n % 256 or k % BK or m < 128 or n <= 0 or k <= 0:
        return False
    if m % 128 and (tri or (m % 128) % EPP):
        return False
    if not aligned or lda % EPP or ldb % EPP:
        return False
    tiles_m, tiles_n, ktiles = _cdiv(m, 128), n // 256, k // BK
    ntiles = tiles_m * tiles_n
    if tri:
        if m != n:
            return False
        ntiles = sum((tiles_m - i) // 2 for i in range(tiles_m)) + (tiles_m // 2 + 1) // 2
    W, need = ntiles * ktiles, NUM_CU * 64
    if W < need:
        r.gate(need / W)
        return False
    r.gate(W / need)
    if tri and ntiles < 8:
        return False
    return True


def _impl(r, prec, ta, tb, m, n, k, tri, lda, ldb, a_al, b_al, avoid, same, scale_only, norma):
    """gemm_impl after its argument checks; returns the signature of what it launches"""
    SKK = 16 if prec == "f64" else 32
    V = 16 // SIZEOF[prec]
    if m == 0 or n == 0:
        return "nothing"
    if scale_only or k == 0:
        r.count(SCALE)
        r.leaves.append(dict(kind="scale"))
        return "scale"
    rec = lambda m_, k_, tri_, same_: _impl(r, prec, ta, tb, m_, n, k_, tri_, lda, ldb, a_al, b_al, avoid, same_, False, False)
    if ta and not tb and not norma and m <= 64 and n <= 64 and k >= 8192:
        is_same = same and lda == ldb and m == n
        if not (tri and not is_same):
            r.count(SKINNY)
            nta, ntb = (2 if m <= 32 else 4), (2 if n <= 32 else 4)
            name = f"skinny:{nta}{'=' if is_same else 'x' + str(ntb)}"
            r.leaves.append(dict(kind="skinny", nta=nta, ntb=ntb, same=is_same))
            return name
    if not tb and k % SKK and k >= 1024 and n % 256 == 0 and not norma and ((m == n) if tri else (m >= 128)):
        r.count(CUT)
        k_main = (k // SKK) * SKK
        return "cut(" + rec(m, k_main, tri, same and ta) + "," + rec(m, k - k_main, tri, same and ta) + ")"
    if prec == "f32" and not tb and k > 16384 and k % SKK == 0 and n % 256 == 0 and not norma and ((m == n) if tri else (m >= 128)):
        r.count(CUT)
        return "cut(" + ",".join(rec(m, min(16384, k - k0), tri, same and ta) for k0 in range(0, k, 16384)) + ")"
    aligned = a_al and b_al
    if tri and not tb and m == n and n % 256 == 0 and k % SKK == 0:
        if _sk_takes(r, prec, tb, m, n, k, 1, aligned, lda, ldb, avoid):
            r.count(SK[prec])
            r.leaves.append(dict(kind="sk"))
            return "sk"
    if not tri and not tb and m >= 128 and n % 256 == 0 and k % SKK == 0:
        m_main = m if (m % 128) % V == 0 else (m // 128) * 128
        if _sk_takes(r, prec, tb, m_main, n, k, 0, aligned, lda, ldb, avoid):
            r.count(SK[prec])
            r.leaves.append(dict(kind="sk"))
            if m_main == m:
                return "sk"
            r.count(MPEEL)
            return "mpeel(sk," + rec(m - m_main, k, 0, False) + ")"
    if not tri and m <= 512 and n <= 512 and k <= 2048 and m * n >= 1024 and _cdiv(m, 128) * _cdiv(n, 128) <= 16:
        r.count(SMALL)
        r.leaves.append(dict(kind="small"))
        return "small"
    vec = aligned and lda % V == 0 and ldb % V == 0
    bm, bn, splitk, margin = tiled_plan(prec, m, n, k, tri)
    r.gate(margin)
    r.count(TILED)
    if splitk > 1:
        r.count(SPLITK)
    r.leaves.append(dict(kind="tiled", bm=bm, bn=bn, vec=vec, splitk=splitk))
    return f"tiled:{bm}x{bn}:{'v' if vec else 's'}" + ("+split" if splitk > 1 else "")


def replay(prec, ta, tb, m, n, k, tri=0, lda=None, ldb=None, a_aligned=True, b_aligned=True, avoid=False, same=False, alpha_zero=False,
           norma=False):
    """ta, tb: 0 / 1.  a_aligned / b_aligned: the base pointer is a multiple of 16 bytes.  same: B is the pointer A.  -> Route"""
    lda = lda if lda is not None else (k if ta else m)
    ldb = ldb if ldb is not None else (n if tb else k)
    r = Route()
    r.sig = _impl(r, prec, ta, tb, m, n, k, tri, lda, ldb, a_aligned, b_aligned, avoid, same, alpha_zero, norma)
    return r


# ---------------------------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    prec: str
    sig: str                     # the route the case is listed under (replay(...).sig)
    op: str                      # "gemm" | "syrk"
    ta: str
    tb: str
    m: int
    n: int
    k: int
    alpha: float = 2.0
    beta: float = -0.5
    kind: str = "exact"          # "exact" | "rounded"
    amode: str = "vec"           # leading dimension / base of A: "vec" (multiple of 4 elements, aligned base), "odd" (odd leading dimension),
    bmode: str = "vec"           # "off" (multiple of 4, base one element into the allocation)
    same: bool = False           # B is A (the same pointer and leading dimension); syrk always
    avoid: bool = False          # under rlhip_avoid_persistent(1)
    roomy: bool = False          # 272 guard rows and 272 guard columns of NaN: a whole 256 x 16 tile read from any in-range origin stays inside
    seed: int = 0

    def __post_init__(self):
        if self.op == "syrk":
            self.same = True

    @property
    def tri(self):
        return 1 if self.op == "syrk" else 0

    def a_shape(self):           # stored shape of A
        return (self.k, self.m) if self.ta == "T" else (self.m, self.k)

    def b_shape(self):
        return (self.n, self.k) if self.tb == "T" else (self.k, self.n)

    def ld(self, which):
        rows, mode = (self.a_shape()[0], self.amode) if which == "a" else (self.b_shape()[0], self.bmode)
        if self.same and which == "b":
            return self.ld("a")
        if mode == "odd":
            L = rows + 1
            return L if L % 2 else L + 1
        return rows + 4 - rows % 4 + (272 if self.roomy else 0)      # 1 .. 4 guard rows (roomy: 273 .. 276), a multiple of 4

    def guard_cols(self):
        return 272 if self.roomy else 2

    def ldc(self):
        return self.m + (4 if self.m % 4 == 0 else 3)

    def route(self):
        return replay(self.prec, self.ta == "T", self.tb == "T", self.m, self.n, self.k, self.tri, self.ld("a"), self.ld("b"),
                      self.amode != "off", (self.amode if self.same else self.bmode) != "off", self.avoid, self.same, self.alpha == 0.0)

    def operands(self):
        """-> op(A) (m x k), op(B) (k x n), C0 (m x n) in float64, entries representable in the case's type"""
        rng = np.random.default_rng(self.seed)
        m, n, k = self.m, self.n, self.k
        if self.kind == "exact":
            g = lambda *s: rng.integers(-ENTRY_MAX, ENTRY_MAX + 1, s).astype(NPDT[self.prec]).astype(np.float64)
        else:
            g = lambda *s: rng.standard_normal(s).astype(NPDT[self.prec]).astype(np.float64)
        A = g(m, k)
        if self.same:
            assert self.ta != self.tb and (self.op == "syrk" or self.n <= self.m)
            B = A.T[:, :n]                 # B is the pointer A: op(B) is made of op(A)'s first n rows
        else:
            B = g(k, n)
        return A, B, g(m, n)


PRECS = ("f64", "f32")
TT = [(a, b) for a in "NT" for b in "NT"]


def _v(mode_a, mode_b):
    return "v" if mode_a == "vec" and mode_b == "vec" else "s"


def _build():
    cs = []

    def add(name, prec, sig, op, ta, tb, m, n, k, **kw):
        cs.append(Case(f"{name}-{prec}", prec, sig, op, ta, tb, m, n, k, seed=len(cs) + 1, **kw))

    for p in PRECS:
        # ---- scale only: k == 0 and alpha == 0, beta in {0, 1, other}; through gemm and through syrk
        for k, alpha in ((0, 2.0), (7, 0.0)):
            for beta in (0.0, 1.0, -0.5):
                add(f"scale-gemm-k{k}-b{beta}", p, "scale", "gemm", "N", "T", 37, 21, k, alpha=alpha, beta=beta)
                add(f"scale-syrkT-k{k}-b{beta}", p, "scale", "syrk", "T", "N", 37, 37, k, alpha=alpha, beta=beta)
                add(f"scale-syrkN-k{k}-b{beta}", p, "scale", "syrk", "N", "T", 130, 130, k, alpha=alpha, beta=beta)

        # ---- small kernel: four transposes x K in {1, 3, 4, 31, 32, 33, 2047, 2048}, M and N at and off multiples of 16 and 32
        shapes = [(32, 32), (33, 47), (64, 16), (17, 100), (96, 65), (31, 34), (48, 80), (130, 20)]
        for i, k in enumerate((1, 3, 4, 31, 32, 33, 2047, 2048)):
            for j, (ta, tb) in enumerate(TT):
                m, n = shapes[(i + 3 * j) % 8]
                add(f"small-{ta}{tb}-{m}x{n}x{k}", p, "small", "gemm", ta, tb, m, n, k, beta=(0.0 if (i + j) % 3 == 0 else -0.5))
        for ta, tb in TT:                                        # scalar addressing needs no alignment: odd leading dimensions, offset bases
            add(f"small-odd-{ta}{tb}", p, "small", "gemm", ta, tb, 47, 33, 37, amode="odd", bmode="off")
        # both sides of its gates
        add("small-mn1024", p, "small", "gemm", "N", "N", 32, 32, 17)
        add("small-mn1023", p, "tiled:256x64:v", "gemm", "N", "N", 31, 33, 17)
        add("small-k2048", p, "small", "gemm", "T", "N", 64, 64, 2048, beta=0.0)
        add("small-k2049", p, "tiled:256x64:v+split", "gemm", "T", "N", 64, 64, 2049, beta=0.0)
        add("small-m512", p, "small", "gemm", "N", "T", 512, 16, 33)
        add("small-m513", p, "tiled:256x16:v", "gemm", "N", "T", 513, 16, 33)
        add("small-n512", p, "small", "gemm", "T", "T", 16, 512, 33)
        add("small-n513", p, "tiled:128x128:v", "gemm", "T", "T", 16, 513, 33)
        add("small-16tiles", p, "small", "gemm", "N", "N", 512, 512, 33)        # (17 tiles of 128 cannot be had with m, n <= 512: that gate is dead)

        # ---- tiled kernel: every tile shape (N), four transposes, ragged M against 128 and 256, K in {1, 15, 16, 17} and longer
        tile_of = {1: "256x16", 16: "256x16", 17: "256x32", 32: "256x32", 33: "256x64", 64: "256x64", 65: "128x128", 128: "128x128",
                   129: "128x128", 300: "128x128"}
        Ms = [513, 640, 767, 768, 769, 1000]
        Ks = [1, 15, 16, 17, 100]
        for i, (n, tile) in enumerate(tile_of.items()):
            for j, (ta, tb) in enumerate(TT):
                m = [1, 255, 257, 1000][j] if n == 1 else Ms[(i + j) % 6]
                k = Ks[(i + 2 * j) % 5]
                add(f"tiled-{ta}{tb}-{m}x{n}x{k}", p, f"tiled:{tile}:v", "gemm", ta, tb, m, n, k, beta=(0.0 if (i + j) % 2 else -0.5))
        # the scalar-load path, reached both ways, on every tile shape and operand layout
        for i, n in enumerate((16, 32, 64, 129)):
            for j, (ta, tb) in enumerate(TT):
                for am, bm_ in (("odd", "vec"), ("vec", "odd"), ("off", "vec"), ("vec", "off")):
                    add(f"tiled-{am}A-{bm_}B-{ta}{tb}-n{n}", p, f"tiled:{tile_of[n]}:s", "gemm", ta, tb, Ms[(i + j + 1) % 6], n, Ks[(i + j) % 5],
                        amode=am, bmode=bm_, beta=(0.0 if (i + j) % 2 else -0.5))
        # ragged edges inside parents with room for a whole tile of NaN beyond every edge: an edge load that is not masked reads poison
        for ta, tb in TT:
            add(f"tiled-roomy-{ta}{tb}-128x128", p, "tiled:128x128:v", "gemm", ta, tb, 515, 70, 17, roomy=True)
            add(f"tiled-roomy-{ta}{tb}-256x32", p, "tiled:256x32:v", "gemm", ta, tb, 600, 20, 15, roomy=True, beta=0.0)
        # split-K taken and not taken, beta == 0 and != 0 in each
        for beta in (0.0, -0.5):
            add(f"tiled-split-b{beta}", p, "tiled:128x128:v+split", "gemm", "T", "N", 300, 129, 12000, beta=beta)
            add(f"tiled-split-NT-b{beta}", p, "tiled:256x32:v+split", "gemm", "N", "T", 515, 20, 6001, beta=beta)
            add(f"tiled-split-scalar-b{beta}", p, "tiled:256x64:s+split", "gemm", "T", "T", 257, 40, 4099, beta=beta, amode="off", bmode="odd")
            add(f"tiled-nosplit-b{beta}", p, "tiled:128x128:v", "gemm", "N", "N", 700, 129, 500, beta=beta)
        # at a shape the persistent kernel takes: op(B) = B^T, and under avoid_persistent
        M_, N_, K_ = 1024, 2048, (8192 if p == "f64" else 16384)
        add("persistent-shape", p, "sk", "gemm", "N", "N", M_, N_, K_)
        add("persistent-shape-transb", p, "tiled:128x128:v+split", "gemm", "N", "T", M_, N_, K_)
        add("persistent-shape-avoid", p, "tiled:128x128:v+split", "gemm", "T", "N", M_, N_, K_, avoid=True, beta=0.0)

        # ---- syrk: both forms, n in {1, 100, 128, 130, 256, 300}
        for i, n in enumerate((1, 100, 128, 130, 256, 300)):
            for tr in "TN":
                k = (37, 64, 16, 129)[(i + (tr == "N")) % 4]
                add(f"syrk{tr}-n{n}-k{k}", p, "tiled:128x128:v", "syrk", tr, "NT"[tr == "N"], n, n, k, beta=(0.0 if i % 2 else -0.5))
        add("syrkT-odd-ld", p, "tiled:128x128:s", "syrk", "T", "N", 130, 130, 77, amode="odd")
        add("syrkN-offset", p, "tiled:128x128:s", "syrk", "N", "T", 130, 130, 77, amode="off")
        for beta in (0.0, -0.5):
            add(f"syrkT-split-b{beta}", p, "tiled:128x128:v+split", "syrk", "T", "N", 256, 256, 8000, beta=beta)
            add(f"syrkN-split-b{beta}", p, "tiled:128x128:v+split", "syrk", "N", "T", 130, 130, 5000, beta=beta)
        add("syrkT-persistent", p, "sk" if p == "f64" else "cut(sk,sk)", "syrk", "T", "N", 2048, 2048, 8192 if p == "f64" else 32768)
        if p == "f32":
            add("syrkT-chunks-tiled", p, "cut(tiled:128x128:v+split,tiled:128x128:v)", "syrk", "T", "N", 256, 256, 16384 + 32, beta=0.0)

        # ---- narrow-panel kernel: the four widths, B identical to A with and without tri, both sides of its gates
        for m, n in ((16, 16), (32, 48), (48, 32), (64, 64), (33, 7)):
            nta, ntb = (2 if m <= 32 else 4), (2 if n <= 32 else 4)
            add(f"skinny-{m}x{n}", p, f"skinny:{nta}x{ntb}", "gemm", "T", "N", m, n, 8192 + 77 * (m % 3), beta=(0.0 if m == 32 else -0.5))
        add("skinny-same-32", p, "skinny:2=", "gemm", "T", "N", 32, 32, 9000, same=True)
        add("skinny-same-48", p, "skinny:4=", "gemm", "T", "N", 48, 48, 8192, same=True, beta=0.0)
        add("skinny-syrk-20", p, "skinny:2=", "syrk", "T", "N", 20, 20, 10000)
        add("skinny-syrk-64", p, "skinny:4=", "syrk", "T", "N", 64, 64, 8192, beta=0.0)
        add("skinny-alias-not-same", p, "skinny:4x2", "gemm", "T", "N", 48, 16, 8200, same=True)     # the same pointer, m != n
        add("skinny-k8191", p, "tiled:256x32:v+split", "gemm", "T", "N", 32, 32, 8191)
        add("skinny-m64", p, "skinny:4x2", "gemm", "T", "N", 64, 8, 8192)
        add("skinny-m65", p, "tiled:256x16:v+split", "gemm", "T", "N", 65, 8, 8192)
        add("skinny-syrkN", p, "tiled:128x128:v+split", "syrk", "N", "T", 32, 32, 8192)            # A A^T is not its product

        # ---- contraction cut by gemm_impl: k-remainder peel at a small and at a persistent shape, beta = 0 with NaN in C
        add("kpeel-small", p, "cut(small,small)", "gemm", "N", "N", 200, 256, 1024 + 5, beta=0.0)
        add("kpeel-small-TN", p, "cut(small,small)", "gemm", "T", "N", 129, 512, 1024 + 31, beta=-0.5)
        add("kpeel-k1023", p, "small", "gemm", "N", "N", 200, 256, 1023, beta=0.0)
        add("kpeel-persistent", p, "cut(sk,tiled:128x128:v)", "gemm", "T", "N", M_, N_, K_ + 5, beta=0.0)
        add("kpeel-syrk", p, "cut(tiled:128x128:v+split,tiled:128x128:v)", "syrk", "T", "N", 256, 256, 4096 + 3, beta=0.0)
        # m-peel: (m % 128) % (16 bytes) != 0 at a persistent shape
        add("mpeel", p, "mpeel(sk,tiled:128x128:v+split)", "gemm", "N", "N", M_ + (1 if p == "f64" else 2), N_, K_)
        if p == "f32":
            add("chunks-16416", p, "cut(tiled:128x128:v+split,small)", "gemm", "N", "N", 128, 256, 16384 + 32, beta=0.0)
            add("chunks-3x16384", p, "cut(tiled:128x128:v+split,tiled:128x128:v+split,tiled:128x128:v+split)", "gemm", "T", "N", 128, 256,
                3 * 16384, beta=0.0)
            add("chunks-16384-not-cut", p, "tiled:128x128:v+split", "gemm", "N", "N", 128, 256, 16384, beta=0.0)
            add("chunks-persistent-16416", p, "cut(sk,tiled:128x128:v)", "gemm", "N", "N", M_, N_, 16384 + 32, beta=0.0)
            add("chunks-persistent-2x16384", p, "cut(sk,sk)", "gemm", "T", "N", M_, N_, 2 * 16384, beta=-0.5)

        # ---- rounded cases: Gaussian operands against the componentwise bound, a few per route
        R = dict(kind="rounded", alpha=1.5, beta=-0.75)
        add("r-small-NN", p, "small", "gemm", "N", "N", 100, 70, 300, **R)
        add("r-small-TT", p, "small", "gemm", "T", "T", 65, 33, 2047, **R)
        add("r-tiled-NT", p, "tiled:128x128:v", "gemm", "N", "T", 513, 65, 100, **R)
        add("r-tiled-TN-scalar", p, "tiled:256x32:s", "gemm", "T", "N", 600, 20, 100, amode="odd", **R)
        add("r-tiled-split", p, "tiled:128x128:v+split", "gemm", "T", "N", 130, 129, 6000, **R)
        add("r-syrkT", p, "tiled:128x128:v", "syrk", "T", "N", 130, 130, 100, **R)
        add("r-syrkN-split", p, "tiled:128x128:v+split", "syrk", "N", "T", 100, 100, 5000, **R)
        add("r-skinny", p, "skinny:4x2", "gemm", "T", "N", 48, 32, 10000, **R)
        add("r-skinny-syrk", p, "skinny:2=", "syrk", "T", "N", 32, 32, 9001, **R)
        add("r-kpeel", p, "cut(small,small)", "gemm", "N", "N", 130, 256, 1029, **R)
        if p == "f32":
            add("r-chunks", p, "cut(tiled:128x128:v+split,small)", "gemm", "N", "N", 128, 256, 16384 + 32, **R)
            add("r-persistent", p, "sk", "gemm", "N", "N", M_, N_, K_, **R)
    return cs


CASES = _build()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def unit_roundoff(prec):
    return float(np.finfo(NPDT[prec]).eps) / 2


def gamma(n, prec):
    nu = n * unit_roundoff(prec)
    return nu / (1 - nu)
