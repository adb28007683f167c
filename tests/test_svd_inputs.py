"""CPU half of test_gpu_svd.py: every input that is meant to send the device SVD down one particular route is replayed here in numpy, in
the precision of the call, and must clear each threshold of that route by a factor of 10 (tests/_svd_inputs.py)."""
import numpy as np
import pytest

import _svd_inputs as si

CASES = [(name, prec) for name, spec in si.ROUTE_CASES.items() for prec in spec[1]]


@pytest.mark.parametrize("name,prec", CASES)
def test_route_inputs_clear_their_thresholds_tenfold(name, prec):
    build, _, gram, want = si.ROUTE_CASES[name]
    routes, margin, numbers = si.replay(build(), prec, gram)
    print(name, prec, routes, margin, numbers)
    assert routes == want, numbers
    assert margin >= 10.0, numbers


def test_every_reachable_route_has_an_input_in_both_precisions():
    got = {p: set() for p in ("f64", "f32")}
    for name, (_, precs, _, want) in si.ROUTE_CASES.items():
        for p in precs:
            got[p] |= set(want)
    assert got["f64"] == set("abcde") and got["f32"] == set("bcde")      # a is fp64 only; f: see _svd_inputs.py


def test_replay_recognises_the_routes_it_cannot_reach_with_margin():
    """the replay itself: a cond-95 pair lands on b + d or c + d by rounding (margin below 10 either way, which is why no GPU case uses
    it), and a zero matrix fails the first factorization"""
    routes, margin, _ = si.replay(si.with_spectrum(20000, 2, np.array([1.0, 1.0 / 90]), 21), "f64", False)
    assert routes in ("bd", "cd") and margin < 10.0
    assert si.replay(np.zeros((10, 3)), "f64")[0] == "e"


def test_kahan_matches_its_definition():
    K = si.kahan(5, 1.2)
    assert np.allclose(np.diag(K), np.sin(1.2) ** np.arange(5)) and np.allclose(K[1, 3], -np.cos(1.2) * np.sin(1.2)) and np.all(np.tril(K, -1) == 0)


def test_rank_deficient_is_exact_in_fp32():
    A = si.rank_deficient(300, 20, 5, 3)
    assert np.array_equal(A, A.astype(np.float32).astype(np.float64)) and np.linalg.matrix_rank(A) == 5
