"""CPU checks of full multigrid's prolongation by position: gs_fmg_axis (pure host code of libgpusolve_transfer.so)
against the closed form of include/gpusolve_transfer.h, the operator's numpy restatement (tests/fmg_pa_ref.py) for
exactness and against the aligned cubic, and the FMG start composed of it, tests/xfer_ref.py's POSITION V-cycle and the
CPU oracle on even sizes. No GPU is touched.

Bounds. Polynomial exactness 4 * 2^-52 and weight sums 2^-52: a cubic through exact nodes, values in [1, 1.4], four
products and three sums (measured with the restatement: at most 6.7e-16). Aligned axes against fmg_ref.prolong: 1e-14
of the field's maximum, the same cubic with about twenty roundings of difference per point (measured 6.7e-16). The
convergence claims are DESIGN.md §4.7's CPU table: FMG(1) on an even cube is worth a little more than four plain
POSITION cycles from zero (asserted: more than three; 40 x 32 x 24: more than two)."""
import ctypes as C
import functools

import numpy as np
import pytest

import fmg_pa_ref as PA
import fmg_ref
import gpusolve as gsv
import oracle as O
import xfer_ref as X
from conftest import rel

SIZES = list(range(2, 201)) + [511, 512, 1000, 1023, 1024]
EPS = 2.0 ** -52


def test_axis_tables_equal_the_closed_form():
    for n in SIZES:
        got, want = gsv.fmg_axis(n), PA.axis_tables(n)
        for key in ("cj", "cw"):
            a, b = got[key], want[key]
            assert a.dtype == b.dtype and a.shape == b.shape, (n, key)
            assert a.tobytes() == b.tobytes(), (n, key)
        assert not got["cj"][[0, n + 1]].any() and not got["cw"][[0, n + 1]].any()


def test_windows_stay_inside_the_padded_coarse_axis():
    for n in SIZES:
        T = gsv.fmg_axis(n)
        P = n // 2 + 2
        K = 4 if P >= 4 else 3
        cj = T["cj"][1:n + 1].astype(np.int64)
        assert cj.min() >= 0 and cj.max() + K - 1 <= P - 1, n
        d = np.diff(cj)
        assert d.min() >= 0 and d.max() <= 1, n  # the kernel's z window advances by 0 or 1 per fine plane
        if K == 3:
            assert not T["cw"][:, 3].any()


def test_weights_sum_to_one():
    for n in SIZES:
        s = gsv.fmg_axis(n)["cw"][1:n + 1]
        total = ((s[:, 0] + s[:, 1]) + s[:, 2]) + s[:, 3]
        assert np.abs(total - 1.0).max() <= EPS, (n, np.abs(total - 1.0).max())


def test_bad_axes_are_refused():
    t = gsv.transfer()
    cj, cw = np.full(64, 77, np.int32), np.full(256, 7.5)
    pj, pw = cj.ctypes.data_as(C.POINTER(C.c_int32)), cw.ctypes.data_as(C.POINTER(C.c_double))
    for nf, nc in ((1, 0), (0, 0), (-4, -2), (8, 3), (8, 5), (9, 5), (7, 4)):
        assert t.gs_fmg_axis(nf, nc, pj, pw) == gsv._abi.GS_EINVAL, (nf, nc)
    assert t.gs_fmg_axis(8, 4, None, pw) == gsv._abi.GS_EINVAL
    assert t.gs_fmg_axis(8, 4, pj, None) == gsv._abi.GS_EINVAL
    assert np.all(cj == 77) and np.all(cw == 7.5)  # nothing was written
    assert t.gs_fmg_axis(8, 4, pj, pw) == 0
    with pytest.raises(ValueError):
        gsv.fmg_axis(1)


def _poly(x, cubic):
    p = (1.0 + 2.0 * x) - 3.0 * x * x
    return p + x * x * x if cubic else p


@pytest.mark.parametrize("n", [2, 3, 4, 6, 32, 33])
def test_polynomial_exactness_per_axis(n):
    """K = 4 reproduces 1 + 2x - 3x^2 + x^3, K = 3 (n = 2, 3) its quadratic part; node J of the coarse axis sits at
    J / (m + 1), fine point i at i / (n + 1)."""
    m, cubic = n // 2, n >= 4
    xc = np.arange(m + 2) / np.float64(m + 1)
    xf = np.arange(n + 2) / np.float64(n + 1)
    for axis in range(3):
        shape = [1, 1, 1]
        shape[axis] = m + 2
        got = PA.prolong_axis(_poly(xc, cubic).reshape(shape), axis, n).reshape(-1)
        err = np.abs(got[1:n + 1] - _poly(xf, cubic)[1:n + 1]).max()
        print(f"n = {n}, axis {axis}: max error {err:.3g}")
        assert err <= 4 * EPS
        assert got[0] == 0.0 and got[n + 1] == 0.0


@pytest.mark.parametrize("cd", [(1, 1, 1), (2, 2, 2), (3, 3, 3), (7, 3, 15), (16, 9, 5)], ids=str)
def test_aligned_axes_agree_with_the_aligned_cubic(cd):
    fd = tuple(2 * n + 1 for n in cd)
    rng = np.random.default_rng(sum(cd))
    c = np.zeros(tuple(n + 2 for n in cd))
    c[1:-1, 1:-1, 1:-1] = rng.standard_normal(cd)
    got, want = PA.prolong(c, fd), fmg_ref.prolong(c)
    d = np.abs(got - want)[1:-1, 1:-1, 1:-1].max()
    print(f"{cd}: max difference {d:.3g} of {np.abs(want).max():.3g}")
    assert d <= 1e-14 * np.abs(want).max()
    ring = got.copy()
    ring[1:-1, 1:-1, 1:-1] = 0.0
    assert not ring.any()


# ---- convergence (LINEAR, 2+2 smoothing, omega 0.8, the reference's right-hand side) ---------------------------------
@functools.lru_cache(maxsize=None)
def plain(dims, cycles):
    return X.Cycle(dims, O.LINEAR).solve(cycles)


@functools.lru_cache(maxsize=None)
def fmg_res(dims, k, cubic=True):
    return PA.fmg(dims, cycles_per_level=k, cubic=cubic)[1]


@pytest.mark.parametrize("dims,cycles", [((32, 32, 32), 3), ((64, 64, 64), 3), ((46, 46, 46), 3), ((40, 32, 24), 2)],
                         ids=str)
def test_fmg_on_even_sizes(dims, cycles):
    hist, f1, f2, tri = plain(dims, cycles), fmg_res(dims, 1), fmg_res(dims, 2), fmg_res(dims, 1, False)
    print(f"{dims}: plain {hist}, FMG(1) {f1!r}, FMG(2) {f2!r}, FMG(1) trilinear {tri!r}")
    assert f1 < hist[cycles]
    assert f1 < tri
    assert f2 < f1


def test_aligned_grid_is_the_aligned_fmg():
    dims = (63, 63, 63)
    _, _, want = fmg_ref.fmg(dims)
    got = fmg_res(dims, 1)
    print(f"63^3: {got!r} against fmg_ref.fmg's {want!r}")
    assert rel(got, want) <= 1e-12
