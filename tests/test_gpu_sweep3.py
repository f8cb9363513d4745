"""The fused three-sweep kernel (gs_jacobi_sweep3, LINEAR, k_tb3y) against three single sweeps (gs_jacobi_sweep)
— bit for bit: the kernel evaluates the same expressions in the same order — on shapes that hit every tile edge,
with a general stencil and with extreme magnitudes; and the driver's triple schedule (HipSolver::jacobi with
GS_SWEEP3_MIN_POINTS / GS_NO_SWEEP3) against the pair schedule."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import gpusolve as gsv  # noqa: E402
from gpusolve.devfield import DevField  # noqa: E402


def k():
    assert torch.cuda.is_available()
    return gsv.kernels()


def st():
    return torch.cuda.current_stream().cuda_stream


def ok(rc):
    assert rc == 0, k().gs_strerror(rc).decode()


UNIT = gsv.Stencil().to_abi()
# non-unit weights in canonical order: the UN = false instances
GENERAL = gsv.Stencil([4, -1, -1, -0.5, -0.5, -0.5, -0.5], list(gsv.CANONICAL_OFFSETS)).to_abi()


def rand_full(rng, nx, ny, nz, scale=1.0):
    a = np.zeros((nx + 2, ny + 2, nz + 2))
    a[1:nx + 1, 1:ny + 1, 1:nz + 1] = rng.uniform(-scale, scale, (nx, ny, nz))
    return a


def three_sweeps(S, v0, f0, h, omega, gamma):
    nx, ny, nz = (s - 2 for s in v0.shape)
    v, f, alt = DevField(nx, ny, nz).from_xyz(v0), DevField(nx, ny, nz).from_xyz(f0), DevField(nx, ny, nz)
    L = v.level(h)
    for _ in range(3):
        ok(k().gs_jacobi_sweep(C.byref(S), C.byref(L), 0, omega, gamma, v.ptr, alt.ptr, f.ptr, None, st()))
        v, alt = alt, v
    return v.to_xyz()


def triple(S, v0, f0, h, omega, gamma):
    nx, ny, nz = (s - 2 for s in v0.shape)
    v, f, out = DevField(nx, ny, nz).from_xyz(v0), DevField(nx, ny, nz).from_xyz(f0), DevField(nx, ny, nz)
    L = v.level(h)
    assert k().gs_jacobi_sweep3_supported(C.byref(S), C.byref(L)) >= 1
    ok(k().gs_jacobi_sweep3(C.byref(S), C.byref(L), omega, gamma, v.ptr, out.ptr, f.ptr, st()))
    got = out.to_xyz()
    np.testing.assert_array_equal(v.to_xyz(), v0)  # the input iterate is left as it was
    return got


SHAPES = [(1, 1, 1), (2, 5, 3), (3, 2, 2),  # nz shorter than the pipeline
          (5, 4, 33),  # many 4-plane chunks
          (127, 9, 17), (128, 8, 8), (256, 12, 9),  # FX rows, several y-tiles
          (129, 13, 40), (257, 6, 10), (500, 7, 9),
          (512, 4, 5), (512, 7, 13),  # a ragged last tile whose mirrored wave is partly outside
          (64, 64, 64), (200, 33, 70),
          (130, 1, 6), (130, 2, 6), (130, 3, 6)]


@pytest.mark.parametrize("shape", SHAPES)
def test_sweep3_equals_three_sweeps(shape):
    rng = np.random.default_rng(sum(s * 1000 ** i for i, s in enumerate(shape)) % 2**32)
    h = 1.0 / (shape[1] + 1)
    v0, f0 = rand_full(rng, *shape), rand_full(rng, *shape, 100.0)
    ref = three_sweeps(UNIT, v0, f0, h, 0.8, 1.0)
    np.testing.assert_array_equal(triple(UNIT, v0, f0, h, 0.8, 1.0), ref)


def test_sweep3_rejects_unsupported():
    shape = (513, 5, 6)  # rows of more than 512 points: no triple
    v, f, out = DevField(*shape), DevField(*shape), DevField(*shape)
    L = v.level(1.0 / 6)
    assert k().gs_jacobi_sweep3_supported(C.byref(UNIT), C.byref(L)) == 0
    assert k().gs_jacobi_sweep3(C.byref(UNIT), C.byref(L), 0.8, 1.0, v.ptr, out.ptr, f.ptr, st()) == gsv._abi.GS_EINVAL
    # plane ranges past a level's first plane, a non-canonical stencil order, a missing or aliased iterate
    ok_shape = (64, 8, 8)
    v, f, out = DevField(*ok_shape), DevField(*ok_shape), DevField(*ok_shape)
    assert k().gs_jacobi_sweep3_supported(C.byref(UNIT), C.byref(v.level(1.0 / 9, 2))) == 0
    perm = gsv.Stencil([6, -1, -1, -1, -1, -1, -1], [gsv.CANONICAL_OFFSETS[i] for i in (0, 2, 1, 3, 4, 5, 6)]).to_abi()
    L = v.level(1.0 / 9)
    assert k().gs_jacobi_sweep3_supported(C.byref(perm), C.byref(L)) == 0
    assert k().gs_jacobi_sweep3_supported(C.byref(UNIT), C.byref(L)) == 1
    assert k().gs_jacobi_sweep3(C.byref(UNIT), C.byref(L), 0.8, 1.0, None, out.ptr, f.ptr, st()) == gsv._abi.GS_EINVAL
    assert k().gs_jacobi_sweep3(C.byref(UNIT), C.byref(L), 0.8, 1.0, v.ptr, v.ptr, f.ptr, st()) == gsv._abi.GS_EINVAL
    big = DevField(512, 512, 64)
    assert k().gs_jacobi_sweep3_supported(C.byref(UNIT), C.byref(big.level(1 / 513))) == 2


@pytest.mark.parametrize("shape", [(129, 13, 40), (128, 8, 8)])
def test_sweep3_general_stencil(shape):
    rng = np.random.default_rng(7 + shape[0])
    h = 1.0 / (shape[1] + 1)
    v0, f0 = rand_full(rng, *shape), rand_full(rng, *shape, 100.0)
    ref = three_sweeps(GENERAL, v0, f0, h, 0.7, 0.5)
    np.testing.assert_array_equal(triple(GENERAL, v0, f0, h, 0.7, 0.5), ref)


@pytest.mark.parametrize("nx", [128, 512])
def test_sweep3_extreme_magnitudes(nx):
    """The pair's extreme-magnitude fields (tests/test_gpu_sweep2.py): zeros, denormals, values straddling both ends
    of the fast h^2 division's range, overflow — bit for bit, NaNs as NaNs."""
    rng = np.random.default_rng(nx)
    shape = (nx, 6, 7)
    mags = np.array([0.0, 5e-324, 1e-310, 1e-280, 1e-272, 1.3e-271, 1e-270, 1e-200, 1.0, 1e100, 1e180, 4e180, 5e180,
                     1e200, 1e300])

    def field():
        a = rand_full(rng, *shape)
        inner = a[1:nx + 1, 1:7, 1:8]
        inner[...] = np.sign(inner) * rng.choice(mags, inner.shape) * rng.uniform(0.5, 2.0, inner.shape)
        return a

    h = 1.0 / 7
    v0, f0 = field(), field()
    ref = three_sweeps(UNIT, v0, f0, h, 0.8, 1.0)
    got = triple(UNIT, v0, f0, h, 0.8, 1.0)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
    m = ~np.isnan(ref)
    assert np.array_equal(got[m].view(np.int64), ref[m].view(np.int64))


# ---- the driver's schedule -------------------------------------------------------------------------------------

def lin(dims, **kw):
    return gsv.GridParams(gridDim=dims, mode=gsv.GS_LINEAR, **kw)


def seeded(g, dims, seed):
    """A non-trivial level-0 iterate (the fresh grid's is zero)."""
    v0 = rand_full(np.random.default_rng(seed), *dims)
    g.set_field(0, "v", v0)


def swept(monkeypatch, env, dims, sweeps):
    for name in ("GS_SWEEP3_MIN_POINTS", "GS_NO_SWEEP3"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv(*env)
    with gsv.HipGridData(lin(dims, maxiter=1, tol=0.0)) as g:
        seeded(g, dims, 3)
        gsv.HipSolver.jacobi(g, 0, sweeps)
        g.sync()
        return g.field(0, "v"), gsv.driver().gs_grid_level_triples(g.handle, 0)


@pytest.mark.parametrize("dims", [(64, 64, 64), (33, 31, 29)])
def test_driver_triples_equal_the_pair_schedule(monkeypatch, dims):
    if dims == (64, 64, 64):  # the level the triple really runs on once the threshold allows
        L = DevField(*dims).level(1.0 / 65)
        assert k().gs_jacobi_sweep3_supported(C.byref(UNIT), C.byref(L)) == 2
    # the schedule: 3: T, 4: P P, 5: T P, 6: T T, 7: T P P, 10: T T P P; (33, 31, 29) is too small for triples
    # (and for pairs), so the same calls launch none there
    triples = {3: 1, 4: 0, 5: 1, 6: 2, 7: 1, 10: 2}
    for sweeps in (3, 4, 5, 6, 7, 10):
        want, n_off = swept(monkeypatch, ("GS_NO_SWEEP3", "1"), dims, sweeps)
        got, n_on = swept(monkeypatch, ("GS_SWEEP3_MIN_POINTS", "1"), dims, sweeps)
        assert n_off == 0
        assert n_on == (triples[sweeps] if dims == (64, 64, 64) else 0), (sweeps, n_on)
        assert np.any(want[1:-1, 1:-1, 1:-1] != 0.0)
        np.testing.assert_array_equal(got, want, err_msg=f"{sweeps} sweeps")


def test_default_threshold_keeps_small_levels_on_pairs():
    """Without the switches a 64^3 level is below GS_SWEEP3_MIN_POINTS' default (2^26): no triple."""
    with gsv.HipGridData(lin((64, 64, 64), maxiter=1, tol=0.0)) as g:
        gsv.HipSolver.jacobi(g, 0, 6)
        g.sync()
        assert gsv.driver().gs_grid_level_triples(g.handle, 0) == 0


@pytest.mark.parametrize("speculation", [True, False])
def test_solve_with_three_sweep_smoothing(monkeypatch, speculation):
    """A 3+3 LINEAR solve of 3 cycles at 64^3; histories and level-0 fields identical with and without triples.
    With the default speculation the cycle's first two pre-smoothing sweeps are the pair that also reports the
    norm, so one sweep is left for HipSolver::jacobi and no triple runs; with GS_NO_SPECULATION the three
    pre-smoothing sweeps go through it as one triple per cycle (post-smoothing keeps its prolongation pair)."""
    def solve(env):
        for name in ("GS_SWEEP3_MIN_POINTS", "GS_NO_SWEEP3", "GS_NO_SPECULATION"):
            monkeypatch.delenv(name, raising=False)
        monkeypatch.setenv(*env)
        if not speculation:
            monkeypatch.setenv("GS_NO_SPECULATION", "1")
        with gsv.HipGridData(lin((64, 64, 64), maxiter=3, tol=0.0, preSmoothing=3, postSmoothing=3)) as g:
            hist = gsv.HipSolver.solve(g)
            return hist, g.field(0, "v"), gsv.driver().gs_grid_level_triples(g.handle, 0)

    want_h, want_v, n_off = solve(("GS_NO_SWEEP3", "1"))
    got_h, got_v, n_on = solve(("GS_SWEEP3_MIN_POINTS", "1"))
    assert n_off == 0
    assert n_on == 0 if speculation else n_on >= 1, n_on
    assert len(want_h) >= 3 and all(np.isfinite(want_h))
    assert got_h == want_h
    np.testing.assert_array_equal(got_v, want_v)


def test_slabs_keep_the_pair_schedule(monkeypatch):
    """Two loopback Z-slabs: triples are not taken on distributed levels, so the switch changes nothing."""
    p = lin((64, 256, 64), maxiter=0)

    def loopback(params, nranks, sweeps):
        nx, ny, nz = params.gridDim
        v = np.zeros((nz + 2, ny + 2, nx + 2))
        hist, cnt, ap = (C.c_double * 8)(), C.c_int(0), params.to_abi()
        rc = gsv.driver().gs_zslab_loopback_run(C.byref(ap), nranks, 0, sweeps, 0, hist, 8, C.byref(cnt),
                                                v.ctypes.data_as(gsv._abi.dptr))
        assert rc == 0, gsv.driver().gs_last_error().decode()
        return v.transpose(2, 1, 0)

    def run(env):
        for name in ("GS_SWEEP3_MIN_POINTS", "GS_NO_SWEEP3"):
            monkeypatch.delenv(name, raising=False)
        monkeypatch.setenv(*env)
        return loopback(p, 2, 6)

    want = run(("GS_NO_SWEEP3", "1"))
    got = run(("GS_SWEEP3_MIN_POINTS", "1"))
    assert np.any(want[1:-1, 1:-1, 1:-1] != 0.0)
    np.testing.assert_array_equal(got, want)
