"""Per-sweep relaxation weights through the driver (gs_grid_set_weights, GS_OMEGAS): whole solves
against tests/weights_ref.py, the V-cycle composed of the CPU oracle's operators with one weight per Jacobi sweep.

Tolerances are the suite's own for the same comparisons: LINEAR level-0 fields bit for bit and LINEAR histories to
1e-9 relative (tests/test_gpu_solver.py: only the norm's summation order differs); NONLINEAR fields to 1e-10 of the
field's maximum (ocml's exp against glibc's); the default NEWTON path against the unfused GS_NEWTON one to 1e-11
(tests/test_gpu_newton_b.py: GS_NEWTON_B re-associates one product); paths that only regroup launches (Z-slabs,
equal weights, cleared weights) bit for bit."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import gpusolve as gsv  # noqa: E402
import oracle as O  # noqa: E402
import weights_ref as W  # noqa: E402
from conftest import REPO, rel  # noqa: E402

W2 = (0.57, 1.73)
W3 = (0.53, 0.86, 2.25)
SWITCHES = ("GS_OMEGAS", "GS_FMG", "GS_SWEEP3_MIN_POINTS", "GS_NO_SWEEP3", "GS_NO_SPECULATION", "GS_NO_FUSED_SWEEPS",
            "GS_NO_FUSED_PROLONG", "GS_NO_FUSED_RR", "GS_NO_NEWTON_B", "GS_COARSE_POINTS", "GS_ZSLAB_MIN_POINTS")


def weights_for(n, scale=1.0):
    """n distinct weights (none of them the grid's omega)."""
    table = {0: (), 1: (1.2,), 2: W2, 3: W3}
    w = table[n] if n in table else gsv.chebyshev_weights(n)
    return tuple(scale * x for x in w)


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    assert torch.cuda.is_available(), "GPU tests need a GPU (no CPU fallback exists)"


def params(dims, mode=gsv.GS_LINEAR, cycles=3, pre=2, post=2):
    return gsv.GridParams(maxiter=cycles, tol=0.0, gridDim=dims, mode=mode, preSmoothing=pre, postSmoothing=post)


def solve(p, pre=None, post=None):
    """(history, level-0 v, level 0 smooths in pairs, triples launched on level 0)."""
    with gsv.HipGridData(p) as g:
        if pre is not None:
            g.set_weights(pre, post)
            assert g.weights == (tuple(pre), tuple(post))
        hist = gsv.HipSolver.solve(g)
        d = gsv.driver()
        return hist, g.field(0, "v"), bool(d.gs_grid_level_fused(g.handle, 0)), d.gs_grid_level_triples(g.handle, 0)


@functools.lru_cache(maxsize=None)
def ref_solve(dims, mode, pre, post, cycles):
    c = W.Cycle(dims, mode, pre=pre, post=post)
    hist = c.solve(cycles)
    c.v[0].setflags(write=False)
    return hist, c.v[0]


def assert_hist(got, want, tol):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert rel(a, b) < tol, (got, want)


# 63^3 and 127x63x71 smooth level 0 in fused pairs (the speculative pair, the prolongation pair); 31^3 and 130x40x36
# in single sweeps; every one runs the tiled small levels and the one-workgroup coarse end
LINEAR_SHAPES = [(31, 31, 31), (63, 63, 63), (127, 63, 71), (130, 40, 36)]


@pytest.mark.parametrize("pre,post", [(2, 2), (3, 3), (1, 2), (5, 0)])
@pytest.mark.parametrize("dims", LINEAR_SHAPES)
def test_linear_vcycles_match_the_reference(dims, pre, post):
    wpre, wpost = weights_for(pre), weights_for(post, 0.9)
    hist, v, fused, _ = solve(params(dims, pre=pre, post=post), wpre, wpost)
    want_h, want_v = ref_solve(dims, O.LINEAR, wpre, wpost, 3)
    print("history", hist, "reference", want_h, "fused pairs on level 0:", fused)
    np.testing.assert_array_equal(v, want_v)
    assert_hist(hist, want_h, 1e-9)
    assert fused == (dims in ((63, 63, 63), (127, 63, 71)))


def test_some_shape_smooths_level_0_in_pairs():
    fused = []
    for dims in LINEAR_SHAPES:
        with gsv.HipGridData(params(dims)) as g:
            fused.append(bool(gsv.driver().gs_grid_level_fused(g.handle, 0)))
    assert any(fused) and not all(fused), fused


def test_linear_triples(monkeypatch):
    """3+3 at 64^3 with the triple's threshold lowered and no speculation: the three pre-smoothing sweeps of each
    cycle are one gs_jacobi_sweep3_w launch with pre[0..2]."""
    monkeypatch.setenv("GS_SWEEP3_MIN_POINTS", "1")
    monkeypatch.setenv("GS_NO_SPECULATION", "1")
    hist, v, _, triples = solve(params((64, 64, 64), pre=3, post=3), W3, weights_for(3, 0.9))
    assert triples > 0
    want_h, want_v = ref_solve((64, 64, 64), O.LINEAR, W3, weights_for(3, 0.9), 3)
    np.testing.assert_array_equal(v, want_v)
    assert_hist(hist, want_h, 1e-9)


@pytest.mark.parametrize("dims", [(31, 31, 31), (63, 63, 63)])
def test_nonlinear_vcycles_match_the_reference(dims):
    hist, v, _, _ = solve(params(dims, mode=gsv.GS_NONLINEAR), W2, weights_for(2, 0.9))
    want_h, want_v = ref_solve(dims, O.NONLINEAR, W2, weights_for(2, 0.9), 3)
    d = np.abs(v - want_v).max()
    print("max field difference", d, "of", np.abs(want_v).max(), "history", hist, want_h)
    assert d <= 1e-10 * np.abs(want_v).max()
    assert_hist(hist, want_h, 1e-9)


def test_newton_default_path_against_unfused(monkeypatch):
    """NEWTON at 31^3 with non-uniform weights: the default path (fused pairs, prolongation pair, fused residual +
    restriction, GS_NEWTON_B inner solves) against the one-operator-per-launch GS_NEWTON path."""
    p = params((31, 31, 31), mode=gsv.GS_NEWTON, cycles=3)

    def run():
        with gsv.HipGridData(p) as g:
            g.set_weights(W2, weights_for(2, 0.9))
            hist = gsv.NewtonSolver.solve(g)
            return hist, g.field(0, "v"), g.field(0, "newtonV")

    got = run()
    for name in ("GS_NO_FUSED_SWEEPS", "GS_NO_FUSED_PROLONG", "GS_NO_FUSED_RR", "GS_NO_NEWTON_B"):
        monkeypatch.setenv(name, "1")
    want = run()
    print("histories", got[0], want[0])
    assert len(got[0]) == len(want[0]) == 4
    assert all(b < a for a, b in zip(got[0], got[0][1:])), got[0]
    for a, b in zip(got[0], want[0]):
        assert abs(a - b) <= 1e-11 * abs(b)
    for a, b in zip(got[1:], want[1:]):
        assert np.abs(a - b).max() <= 1e-11 * np.abs(b).max()
    # and the weights are in force: the uniform solve's history is another one
    with gsv.HipGridData(p) as g:
        uniform = gsv.NewtonSolver.solve(g)
    assert uniform != got[0]


@pytest.mark.parametrize("mode,dims", [(gsv.GS_LINEAR, (63, 63, 63)), (gsv.GS_NEWTON, (31, 31, 31))])
def test_equal_weights_and_clearing_are_the_unweighted_solve(mode, dims):
    p = params(dims, mode=mode, cycles=2)
    names = ("v", "newtonV") if mode == gsv.GS_NEWTON else ("v",)

    def run(prepare):
        with gsv.HipGridData(p) as g:
            prepare(g)
            hist = gsv.HipSolver.solve(g)
            return hist, [g.field(0, n) for n in names]

    def set_then_clear(g):
        g.set_weights(W2, W2)
        g.clear_weights()
        assert g.weights is None

    want = run(lambda g: None)
    for prepare in (lambda g: g.set_weights([p.omega] * 2, [p.omega] * 2), set_then_clear):
        got = run(prepare)
        assert got[0] == want[0]
        for a, b in zip(got[1], want[1]):
            np.testing.assert_array_equal(a, b)
    other = run(lambda g: g.set_weights(W2, W2))
    assert other[0] != want[0]


def test_standalone_jacobi_keeps_omega():
    rng = np.random.default_rng(3)
    v0 = np.zeros((66, 66, 66))
    v0[1:-1, 1:-1, 1:-1] = rng.uniform(-1, 1, (64, 64, 64))

    def swept(weighted):
        with gsv.HipGridData(params((64, 64, 64))) as g:
            g.set_field(0, "v", v0)
            if weighted:
                g.set_weights(W2, W2)
            gsv.HipSolver.jacobi(g, 0, 5)
            g.sync()
            return g.field(0, "v")

    np.testing.assert_array_equal(swept(True), swept(False))


def test_errors_leave_the_grid_unchanged(monkeypatch):
    mx = gsv.GS_MAX_WEIGHTS
    with gsv.HipGridData(params((31, 31, 31))) as g:
        assert g.weights is None
        g.set_weights(W2, (0.9, 1.1))
        for pre, post in (((0.8,), W2), (W3, W2), (W2, ()), ((), ()), (W2, (1.0, float("nan"))),
                          ((float("inf"), 1.0), W2), (W2, (1.0, -float("inf"))), ([0.8] * (mx + 1), W2)):
            with pytest.raises(gsv.GpuSolveError, match="weights"):
                g.set_weights(pre, post)
            assert g.weights == (W2, (0.9, 1.1))
        d = gsv.driver()
        two = (C.c_double * 2)(*W2)
        assert d.gs_grid_set_weights(g.handle, None, 2, two, 2) == 1  # a count without its array
        assert d.gs_grid_set_weights(g.handle, two, -1, two, 2) == 1
        assert b"weights" in d.gs_last_error()
        assert g.weights == (W2, (0.9, 1.1))
    with gsv.HipGridData(params((31, 31, 31), pre=mx + 1, post=2)) as g:  # counts above the cap: no weights at all
        with pytest.raises(gsv.GpuSolveError, match="at most"):
            g.set_weights([0.8] * (mx + 1), W2)
        assert g.weights is None
        assert len(gsv.HipSolver.solve(g)) == 4  # larger counts without weights keep working
    for text in ("0.5,1.5", "0.5,1.5/1", "a,b/c,d", "0.5,nan/1,1", "0.5,,1.5/1,1", "chebyshev"):
        monkeypatch.setenv("GS_OMEGAS", text)
        with pytest.raises(gsv.GpuSolveError, match="GS_OMEGAS|weights"):
            gsv.HipGridData(params((31, 31, 31)))
    monkeypatch.setenv("GS_OMEGAS", "0.57,1.73/0.5,1.5")
    with gsv.HipGridData(params((31, 31, 31))) as g:
        assert g.weights == (W2, (0.5, 1.5))
    monkeypatch.setenv("GS_OMEGAS", "cheb")
    with gsv.HipGridData(params((31, 31, 31), pre=3, post=1)) as g:
        assert g.weights == (gsv.chebyshev_weights(3), gsv.chebyshev_weights(1))


@pytest.mark.parametrize("mode", [gsv.GS_LINEAR, gsv.GS_NONLINEAR])
def test_fmg_with_weights(mode):
    dims = (63, 63, 63)
    wpost = weights_for(2, 0.9)
    with gsv.HipGridData(params(dims, mode=mode)) as g:
        g.set_weights(W2, wpost)
        res = gsv.HipSolver.fmg(g, 1)
        v = g.field(0, "v")
    want_v, want_res = W.fmg(dims, mode, 1, W2, wpost)
    if mode == gsv.GS_LINEAR:
        np.testing.assert_array_equal(v, want_v)
    else:
        assert np.abs(v - want_v).max() <= 1e-10 * np.abs(want_v).max()
    assert rel(res, want_res) < 1e-9


def loopback(p, nranks, min_points):
    nx, ny, nz = p.gridDim
    v = np.zeros((nz + 2, ny + 2, nx + 2))
    cap = 4 * (p.maxiter + 2)
    hist, cnt, ap = (C.c_double * cap)(), C.c_int(0), p.to_abi()
    rc = gsv.driver().gs_zslab_loopback_run(C.byref(ap), nranks, min_points, 0, 1, hist, cap, C.byref(cnt),
                                            v.ctypes.data_as(gsv._abi.dptr))
    assert rc == 0, gsv.driver().gs_last_error().decode()
    return list(hist[:cnt.value]), v.transpose(2, 1, 0)


# 70x33x41: slabs of single sweeps; 64x64x128: two 64^3 slabs that smooth in pairs (two ghost planes)
@pytest.mark.parametrize("dims,nranks", [((70, 33, 41), 2), ((70, 33, 41), 3), ((64, 64, 128), 2)])
def test_zslab_loopback_with_omegas(monkeypatch, dims, nranks):
    monkeypatch.setenv("GS_OMEGAS", "0.57,1.73/0.5,1.6")
    p = params(dims, cycles=2)
    want_h, want_v, _, _ = solve(p)  # (GS_OMEGAS sets the single-GPU grid's weights too)
    ref_h, ref_v = ref_solve(dims, O.LINEAR, W2, (0.5, 1.6), 2)
    np.testing.assert_array_equal(want_v, ref_v)
    hist, v = loopback(p, nranks, 1000)
    np.testing.assert_array_equal(v[1:-1, 1:-1, 1:-1], want_v[1:-1, 1:-1, 1:-1])
    assert_hist(hist, want_h, 1e-12)  # (the slabs' partial sums regroup the norm's summation)


def test_chebyshev_convergence_at_127(monkeypatch):
    """127^3 LINEAR 2+2, six cycles with GS_OMEGAS=cheb: the CPU numbers (last residual 0.0534 against uniform
    0.8's 0.686), the history within 1e-9 relative of the reference's."""
    dims = (127, 127, 127)
    uniform, _, _, _ = solve(params(dims, cycles=6))
    monkeypatch.setenv("GS_OMEGAS", "cheb")
    hist, _, fused, _ = solve(params(dims, cycles=6))
    w = gsv.chebyshev_weights(2)
    want, _ = ref_solve(dims, O.LINEAR, w, w, 6)
    print("cheb", hist, "reference", want, "uniform", uniform)
    assert fused
    assert_hist(hist, want, 1e-9)
    assert abs(hist[-1] - 0.0534) < 0.0001
    assert hist[-1] < uniform[-1] / 8


def test_executable_with_omegas(monkeypatch):
    ex = os.path.join(REPO, "tests", "golden", "data-2nd_order.conf")
    env = dict(os.environ, GS_OMEGAS="cheb")
    out = subprocess.run([gsv._abi.EXECUTABLE, ex], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert lines[1] == "Solving newton problem"
    first = re.fullmatch(r"Inital newton residual: ([\d\.e+-]+)", lines[2])
    assert first, lines[2]
    res = [float(first.group(1))]
    assert len(lines) > 3
    for i, l in enumerate(lines[3:]):
        m = re.fullmatch(r"newton iter: (\d+) residual: ([\d\.e+-]+) Took (\d+)ms", l)
        assert m and int(m.group(1)) == i, l
        res.append(float(m.group(2)))
    assert all(b < a for a, b in zip(res, res[1:])), res
    # a count mismatch (the config smooths 3+3) is a backend error at grid creation, before any solve line:
    # "Exception: ..." on stderr and exit 0, as every backend error (src/main.cpp:96-111)
    bad = subprocess.run([gsv._abi.EXECUTABLE, ex], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, GS_OMEGAS="1,2/3"))
    assert bad.returncode == 0 and bad.stderr.startswith("Exception: weights"), bad.stderr
    assert bad.stdout.splitlines()[1:] == ["Solving newton problem"]
