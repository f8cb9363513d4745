"""CPU checks of the position-aware grid transfers: gs_transfer_axis (pure host code of libgpusolve_transfer.so)
against the closed form of include/gpusolve_transfer.h, and the V-cycle composed of the operators' numpy restatement
(tests/xfer_ref.py) and the CPU oracle — that it is the reference's V-cycle on aligned sizes and converges on even
ones, where the reference's does not. No GPU is touched."""
import ctypes as C

import numpy as np
import pytest

import gpusolve as gsv
import oracle as O
import xfer_ref as X

SIZES = list(range(2, 201)) + [511, 512, 1000, 1023, 1024]
# Convergence cap of a position-aware V-cycle (LINEAR / NONLINEAR, 2+2 sweeps, omega 0.8): each of cycles 3.. must
# reduce the residual norm by at least 2.5x. A cap, not a measurement: the factors measured with this composition on
# the reference's right-hand side are 0.31 .. 0.35, 0.25 with the Chebyshev pair.
CAP = 0.4


def test_axis_tables_equal_the_closed_form():
    for n in SIZES:
        got, want = gsv.transfer_axis(n), X.axis_tables(n)
        for key in ("pj", "pt", "rlo", "rcnt", "rw"):
            a, b = got[key], want[key]
            assert a.dtype == b.dtype and a.shape == b.shape, (n, key)
            assert a.tobytes() == b.tobytes(), (n, key)


def test_aligned_axis_is_the_reference_operator():
    for n in (3, 5, 7, 31, 63, 199, 511, 1023):
        T = gsv.transfer_axis(n)
        i = np.arange(1, n + 1)
        assert np.array_equal(T["pj"][1:n + 1], i // 2)
        assert np.array_equal(T["pt"][1:n + 1], (i % 2) / 2.0)
        m = n // 2
        assert np.array_equal(T["rlo"][1:m + 1], 2 * np.arange(1, m + 1) - 1)
        assert np.all(T["rcnt"][1:m + 1] == 3)
        assert np.array_equal(T["rw"][1:m + 1], np.tile([0.25, 0.5, 0.25, 0.0], (m, 1)))


def test_restriction_is_the_scaled_transpose():
    """rcnt <= 4 consecutive interior indices, and rw is s * P transposed, element for element."""
    for n in SIZES:
        T = gsv.transfer_axis(n)
        m, D = n // 2, n + 1
        s = np.float64(m + 1) / np.float64(D)
        P = np.zeros((n + 2, m + 2))  # P[i, J]: coarse J's weight in fine i
        for i in range(1, n + 1):
            j, t = int(T["pj"][i]), T["pt"][i]
            assert 0 <= j <= m
            P[i, j] = 1.0 - t
            if t > 0.0:
                P[i, j + 1] = t
        for J in range(1, m + 1):
            lo, cnt = int(T["rlo"][J]), int(T["rcnt"][J])
            assert 1 <= cnt <= 4 and lo >= 1 and lo + cnt - 1 <= n, (n, J)
            assert [i for i in range(1, n + 1) if P[i, J] != 0.0] == list(range(lo, lo + cnt)), (n, J)
            assert np.array_equal(T["rw"][J, :cnt], s * P[lo:lo + cnt, J]), (n, J)
            assert np.all(T["rw"][J, cnt:] == 0.0)
        rows = T["rw"][1:m + 1].sum(axis=1)
        assert np.all(rows <= 1.0 + 1e-15) and np.all(rows >= 1.0 - 4.0 / (n * n) - 1e-15), (n, rows.min())


def test_bad_axes_are_refused():
    t = gsv.transfer()
    i32, dbl = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    bufs = [np.zeros(64, np.int32), np.zeros(64), np.zeros(64, np.int32), np.zeros(64, np.int32), np.zeros(256)]
    ptrs = [b.ctypes.data_as(i32 if b.dtype == np.int32 else dbl) for b in bufs]
    for nf, nc in ((1, 0), (0, 0), (-4, -2), (8, 3), (8, 5), (9, 5), (7, 4)):
        assert t.gs_transfer_axis(nf, nc, *ptrs) == gsv._abi.GS_EINVAL, (nf, nc)
    assert all(not b.any() for b in bufs)  # nothing was written
    assert t.gs_transfer_axis(8, 4, *ptrs) == 0
    assert t.gs_transfer_axis(8, 4, None, *ptrs[1:]) == gsv._abi.GS_EINVAL
    with pytest.raises(ValueError):
        gsv.transfer_axis(1)


def test_aligned_grid_composition_is_the_oracle_vcycle():
    ref = O.Grid((31, 31, 31), mode=O.LINEAR, maxiter=6).solve()
    got = X.Cycle((31, 31, 31), O.LINEAR, transfer="position").solve(6)
    assert len(got) == len(ref)
    for a, b in zip(got, ref):
        assert abs(a - b) <= 1e-12 * abs(b), (a, b)


@pytest.fixture(scope="module")
def factors():
    """Per-cycle residual reduction factors of eight cycles, computed once per case."""
    cache = {}

    def get(dims, mode):
        if (dims, mode) not in cache:
            h = X.Cycle(dims, mode, transfer="position").solve(8)
            print(dims, mode, " ".join(f"{b / a:.3f}" for a, b in zip(h, h[1:])))
            cache[dims, mode] = [b / a for a, b in zip(h, h[1:])]
        return cache[dims, mode]
    return get


@pytest.mark.parametrize("dims", [(32, 32, 32), (40, 32, 24)])
def test_linear_converges_on_even_sizes(factors, dims):
    f = factors(dims, O.LINEAR)
    assert all(x <= CAP for x in f[2:]), f  # cycles 3-8


def test_nonlinear_converges_on_32(factors):
    f = factors((32, 32, 32), O.NONLINEAR)
    assert all(x <= CAP for x in f[2:]), f


def test_reference_transfers_do_not_converge_on_64():
    """SURVEY §0.3's finding, at the smallest power of two that shows it in ten cycles."""
    h = X.Cycle((64, 64, 64), O.LINEAR, transfer="reference").solve(10)
    ref = O.Grid((64, 64, 64), mode=O.LINEAR, maxiter=10).solve()
    assert len(h) == len(ref) and all(abs(a - b) <= 1e-12 * b for a, b in zip(h, ref))  # the oracle's V-cycle
    assert h[10] > h[3], h
