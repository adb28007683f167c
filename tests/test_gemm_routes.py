"""CPU half of test_gpu_gemm.py: every case of the GPU table is replayed through the plain-Python copy of gemm.hip::gemm_impl's decisions
(tests/_gemm_routes.py) and must land on the route it is listed under, a factor 2 away from every continuous gate; the exact cases must be
exact: their float64 reference is representable in the type of the call."""
import math

import numpy as np
import pytest

import _gemm_routes as gr

IDS = [c.name for c in gr.CASES]


@pytest.mark.parametrize("name", IDS)
def test_case_predicts_the_route_it_is_listed_under(name):
    c = gr.BY_NAME[name]
    r = c.route()
    print(name, r.sig, r.counts, r.margin)
    assert r.sig == c.sig
    assert r.margin >= 2.0, "too close to the stream-K work gate or to the split-K model's break-even"


@pytest.mark.parametrize("name", [c.name for c in gr.CASES if c.kind == "exact" and c.m * c.n * c.k <= 2 ** 28])
def test_exact_case_reference_is_representable(name):
    c = gr.BY_NAME[name]
    A, B, C0 = c.operands()
    ref = c.alpha * (A @ B) + c.beta * C0
    assert np.array_equal(ref, ref.astype(gr.NPDT[c.prec]).astype(np.float64))
    assert np.all(ref == np.round(2 * ref) / 2)


@pytest.mark.parametrize("name", [c.name for c in gr.CASES if c.kind == "exact"])
def test_exact_case_fits_the_bit_budget(name):
    """every partial sum of products (<= 16 k), its multiple by alpha and the result with beta C0 added: multiples of |beta|'s last bit
    below 2^(bits - 1), whatever the order of summation (covers the cases too large to multiply here)"""
    c = gr.BY_NAME[name]
    bits = 24 if c.prec == "f32" else 53
    assert c.alpha in (0.0, 2.0) and c.beta in (0.0, 1.0, -0.5)
    top = gr.ENTRY_MAX ** 2 * c.k * abs(c.alpha) + abs(c.beta) * gr.ENTRY_MAX
    assert max(top, gr.ENTRY_MAX ** 2 * c.k) * 2 < 2 ** (bits - 1)          # (x 2: halves are the unit)


def _routes(prec):
    seen = {}
    for c in gr.CASES:
        if c.prec == prec:
            r = c.route()
            for which in r.counts:
                seen.setdefault(which, set()).add(c.kind)
    return seen


@pytest.mark.parametrize("prec", gr.PRECS)
def test_every_route_has_a_case(prec):
    seen = _routes(prec)
    for which in (gr.SK[prec], gr.TILED, gr.SPLITK, gr.SMALL, gr.SKINNY, gr.SCALE, gr.CUT, gr.MPEEL):
        assert "exact" in seen.get(which, ()), which
    assert gr.SK["f32" if prec == "f64" else "f64"] not in seen


@pytest.mark.parametrize("prec", gr.PRECS)
def test_every_tile_shape_and_load_path_has_a_case(prec):
    got = set()
    for c in gr.CASES:
        if c.prec == prec and c.kind == "exact":
            for leaf in c.route().leaves:
                if leaf["kind"] == "tiled":
                    got.add((leaf["bm"], leaf["bn"], leaf["vec"], leaf["splitk"] > 1, c.tri, c.ta + c.tb))
    for tile in ((256, 16), (256, 32), (256, 64), (128, 128)):
        for tt in ("NN", "NT", "TN", "TT"):
            for vec in (True, False):
                assert any(g[:3] == tile + (vec,) and g[5] == tt and not g[4] for g in got), (tile, tt, vec)
    for tt in ("TN", "NT"):
        for split in (True, False):
            assert any(g[4] and g[3] == split and g[5] == tt for g in got), (tt, split)
    skinny = {(l["nta"], l["ntb"], l["same"]) for c in gr.CASES if c.prec == prec for l in c.route().leaves if l["kind"] == "skinny"}
    assert skinny >= {(2, 2, False), (2, 4, False), (4, 2, False), (4, 4, False), (2, 2, True), (4, 4, True)}


def test_integer_gates_are_hit_on_both_sides():
    sig = lambda *a, **k: gr.replay(*a, **k).sig
    for p in gr.PRECS:
        assert sig(p, 0, 0, 32, 32, 17) == "small" and sig(p, 0, 0, 31, 33, 17).startswith("tiled")
        assert sig(p, 1, 0, 64, 64, 2048) == "small" and sig(p, 1, 0, 64, 64, 2049).startswith("tiled")
        assert sig(p, 0, 1, 512, 16, 33) == "small" and sig(p, 0, 1, 513, 16, 33).startswith("tiled")
        assert sig(p, 1, 0, 32, 32, 8192).startswith("skinny") and sig(p, 1, 0, 32, 32, 8191).startswith("tiled")
        assert sig(p, 1, 0, 64, 8, 8192).startswith("skinny") and sig(p, 1, 0, 65, 8, 8192).startswith("tiled")
        assert sig(p, 0, 0, 200, 256, 1029) == "cut(small,small)" and sig(p, 0, 0, 200, 256, 1023) == "small"
        assert sig(p, 0, 0, 200, 255, 1029) == "small"                                  # n % 256
        assert sig(p, 0, 0, 200, 256, 1024) == "small"                                  # k % 16 / k % 32
    assert sig("f32", 0, 0, 128, 256, 16384).startswith("tiled") and sig("f32", 0, 0, 128, 256, 16416).startswith("cut(")
    assert sig("f64", 0, 0, 128, 256, 16416).startswith("tiled")
    assert sig("f64", 0, 0, 1024, 2048, 8192) == "sk" and sig("f64", 0, 0, 1024, 2048, 8192, avoid=True).startswith("tiled")
    assert sig("f64", 0, 0, 1024, 2048, 8192, a_aligned=False).startswith("tiled")
    assert sig("f64", 0, 0, 1025, 2048, 8192, lda=2048).startswith("mpeel(sk,") and sig("f64", 0, 0, 1026, 2048, 8192) == "sk"
    assert sig("f32", 0, 0, 1026, 2048, 16384, lda=2048).startswith("mpeel(sk,") and sig("f32", 0, 0, 1028, 2048, 16384) == "sk"


def test_split_k_model_matches_hand_worked_points():
    """the replay of gemm_dispatch's time model at two points worked by hand: one K-tile never splits; 750 K-tiles over 6 tiles do"""
    assert gr.tiled_plan("f64", 513, 16, 16, 0)[:3] == (256, 16, 1)
    bm, bn, s, margin = gr.tiled_plan("f64", 300, 129, 12000, 0)
    assert (bm, bn) == (128, 128) and s > 1 and margin >= 2.0
    assert gr.tiled_plan("f32", 256, 256, 32, 1)[2] == 1 and math.isinf(gr.tiled_plan("f32", 256, 256, 32, 1)[3])


def test_gamma():
    assert gr.gamma(10, "f64") == pytest.approx(10 * 2.0 ** -53, rel=1e-12) and gr.unit_roundoff("f32") == 2.0 ** -24
