"""Per-sweep relaxation weights, the host side (no GPU): the Chebyshev helper against its closed form, the GS_OMEGAS
parser, and tests/weights_ref.py — the weighted V-cycle the GPU tests compare against — held to oracle.Grid.vcycle()
with equal weights, plus the convergence the weights buy on the CPU."""
import math

import numpy as np
import pytest

import gpusolve as gsv
import oracle as O
import weights_ref as W


def closed_form(nu, lo=1.0 / 3.0, hi=2.0):
    return [1.0 / ((hi + lo) / 2 + (hi - lo) / 2 * math.cos(math.pi * (2 * k - 1) / (2 * nu))) for k in range(1, nu + 1)]


def test_chebyshev_pair():
    w = gsv.chebyshev_weights(2)
    assert len(w) == 2
    # the closed form on [1/3, 2]: 1 / (7/6 +- (5/6) / sqrt(2))
    want = [1.0 / (7.0 / 6.0 + 5.0 / 6.0 / math.sqrt(2.0)), 1.0 / (7.0 / 6.0 - 5.0 / 6.0 / math.sqrt(2.0))]
    for a, b, c in zip(w, want, closed_form(2)):
        assert abs(a - b) <= 1e-15 and abs(a - c) <= 1e-15, (a, b, c)
    assert round(w[0], 4) == 0.5695 and round(w[1], 4) == 1.7319
    # the error polynomial's maximum on the band: 0.342 for nu = 2 against 0.733^2 = 0.538 for omega = 0.8
    lam = np.linspace(1.0 / 3.0, 2.0, 20001)
    assert abs(np.abs((1 - w[0] * lam) * (1 - w[1] * lam)).max() - 0.342) < 1e-3
    assert abs(np.abs((1 - 0.8 * lam) ** 2).max() - 0.538) < 1e-3


def test_chebyshev_triple_and_other_intervals():
    w = gsv.chebyshev_weights(3)
    for a, b in zip(w, closed_form(3)):
        assert abs(a - b) <= 1e-15
    assert round(w[0], 4) == 0.5296 and abs(w[1] - 6.0 / 7.0) <= 1e-15 and round(w[2], 4) == 2.2473
    assert abs(gsv.chebyshev_weights(1)[0] - 6.0 / 7.0) <= 1e-15  # one sweep: the band's centre
    for nu, lo, hi in ((4, 0.25, 1.75), (8, 0.1, 2.0), (5, 1.0, 1.5)):
        got = gsv.chebyshev_weights(nu, lo, hi)
        assert len(got) == nu
        for a, b in zip(got, closed_form(nu, lo, hi)):
            assert abs(a - b) <= 4e-16 * abs(b) + 1e-15


@pytest.mark.parametrize("args", [(0,), (-1,), (2, 0.0, 2.0), (2, -0.5, 2.0), (2, 1.0, 1.0), (2, 2.0, 1.0),
                                  (2, float("nan"), 2.0), (2, 1.0, float("inf"))])
def test_chebyshev_errors(args):
    with pytest.raises(gsv.GpuSolveError, match="chebyshev"):
        gsv.chebyshev_weights(*args)


def test_omegas_parser():
    assert gsv.parse_omegas("0.57,1.73/0.5,2", 2, 2) == ((0.57, 1.73), (0.5, 2.0))
    assert gsv.parse_omegas("1e-1,2.5e0,3/4", 3, 1) == ((0.1, 2.5, 3.0), (4.0,))
    assert gsv.parse_omegas("1,2,3,4,5/", 5, 0) == ((1.0, 2.0, 3.0, 4.0, 5.0), ())
    assert gsv.parse_omegas("/-0.25", 0, 1) == ((), (-0.25,))
    cheb = gsv.parse_omegas("cheb", 2, 3)
    assert cheb == (gsv.chebyshev_weights(2), gsv.chebyshev_weights(3))
    assert gsv.parse_omegas("cheb", 5, 0) == (gsv.chebyshev_weights(5), ())


@pytest.mark.parametrize("text,pre,post", [
    ("", 2, 2), ("0.8", 1, 0), ("1,2", 2, 2), ("1,2/3", 2, 2), ("1/2,3", 2, 2), ("1,2/3,4/5,6", 2, 2),
    ("1,,2/3,4", 2, 2), ("1,2,/3,4", 2, 2), ("1,x/3,4", 2, 2), ("1,2 /3,4", 2, 2), ("1,nan/3,4", 2, 2),
    ("1,inf/3,4", 2, 2), ("1,2/3,-inf", 2, 2), ("/", 0, 0), ("chebyshev", 2, 2), ("Cheb", 2, 2),
    ("cheb", gsv.GS_MAX_WEIGHTS + 1, 2), ("cheb", 2, gsv.GS_MAX_WEIGHTS + 1),
    (",".join(["1"] * (gsv.GS_MAX_WEIGHTS + 1)) + "/1", gsv.GS_MAX_WEIGHTS + 1, 1)])
def test_omegas_parser_errors(text, pre, post):
    with pytest.raises(gsv.GpuSolveError):
        gsv.parse_omegas(text, pre, post)


def test_max_weights_constant():
    assert gsv.GS_MAX_WEIGHTS >= 8
    assert gsv.kernels().gs_max_weights() == gsv.GS_MAX_WEIGHTS


@pytest.mark.parametrize("dims", [(15, 15, 15), (31, 15, 23)])
@pytest.mark.parametrize("mode", [O.LINEAR, O.NONLINEAR])
def test_ref_with_equal_weights_is_the_oracle_vcycle(dims, mode):
    g = O.Grid(dims, mode=mode, maxiter=3)
    c = W.Cycle(dims, mode, pre=(0.8, 0.8), post=(0.8, 0.8))
    for _ in range(3):
        want, got = g.vcycle(), c.vcycle()
        v = g.field(0, "v")
        if mode == O.LINEAR:
            np.testing.assert_array_equal(c.v[0], v)
            assert got == want
        else:
            assert np.abs(c.v[0] - v).max() <= 1e-12 * np.abs(v).max()
            assert abs(got - want) <= 1e-12 * want


def test_ref_three_plus_three_and_unequal_counts():
    """pre != post and three sweeps per leg: still the oracle's cycle with equal weights."""
    for pre, post in ((3, 3), (1, 2), (5, 0)):
        g = O.Grid((15, 15, 15), maxiter=2, pre=pre, post=post)
        c = W.Cycle((15, 15, 15), pre=[0.8] * pre, post=[0.8] * post)
        for _ in range(2):
            assert c.vcycle() == g.vcycle()
            np.testing.assert_array_equal(c.v[0], g.field(0, "v"))


def test_ref_fmg_with_equal_weights_is_fmg_ref():
    import fmg_ref
    _, want_v, want_res = fmg_ref.fmg((15, 15, 15))
    v, res = W.fmg((15, 15, 15))
    np.testing.assert_array_equal(v, want_v)
    assert res == want_res


def test_chebyshev_pair_converges_faster_at_63():
    """63^3 LINEAR 2+2, six cycles: the Chebyshev pair leaves a residual below 1/8 of uniform 0.8's (1/12 measured:
    0.0179 against 0.214)."""
    w = gsv.chebyshev_weights(2)
    uniform = W.Cycle((63, 63, 63)).solve(6)
    cheb = W.Cycle((63, 63, 63), pre=w, post=w).solve(6)
    print("uniform", uniform)
    print("cheb", cheb)
    assert uniform[0] == cheb[0]
    assert all(b < a for a, b in zip(cheb, cheb[1:]))
    assert cheb[6] < uniform[6] / 8
    assert abs(uniform[6] - 0.214) < 0.001 and abs(cheb[6] - 0.0179) < 0.0001
    # the order of the two weights within a leg makes no difference to speak of
    swapped = W.Cycle((63, 63, 63), pre=w[::-1], post=w[::-1]).solve(6)
    assert abs(swapped[6] - cheb[6]) < 0.02 * cheb[6]
