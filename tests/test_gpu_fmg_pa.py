"""Full multigrid on every grid size, on the GPU (DESIGN.md §4.7 "FMG on every size"): the tricubic prolongation by
position, gs_fmg_prolong_pa of libgpusolve_transfer.so, against tests/fmg_pa_ref.py and under the kernel ABI's layout
contract, and the driver's POSITION prolongation (gs_grid_set_fmg_prolong, GS_FMG_PROLONG) against the FMG start
composed of fmg_pa_ref's operator, tests/xfer_ref.py's POSITION V-cycle and the CPU oracle.

Tolerances. The kernel and every LINEAR field are bit for bit: the numpy restatement rounds every product and sum as
the kernel does. LINEAR norms to 1e-12 (only the summation order differs). NONLINEAR: the field to 1e-10 of its maximum
and the norm to 1e-9, tests/test_gpu_fuzz.py's bounds for that mode (ocml's exp against glibc's)."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import gpusolve as gsv  # noqa: E402
import oracle as O  # noqa: E402
import fmg_pa_ref as PA  # noqa: E402
from conftest import REPO, rel  # noqa: E402
from fmg_ref import level_dims  # noqa: E402
from layout_field import LAYOUT_IDS, POISON_IN, LayoutField, layouts  # noqa: E402

EINVAL = gsv._abi.GS_EINVAL
SWITCHES = ("GS_TRANSFER", "GS_FMG_PROLONG", "GS_OMEGAS", "GS_FMG", "GS_FMG_NT", "GS_NO_FUSED_SWEEPS",
            "GS_COARSE_POINTS", "GS_TILE_POINTS", "GS_NO_SPECULATION", "GS_ZSLAB_MIN_POINTS")
# A block owns 128 fine x-points by 8 fine rows and marches 16 fine planes on levels that do not fill the chip. K = 3
# (one coarse point); aligned with K = 3; P = 4, both clamps on one window; mixed aligned and non-aligned axes (twice);
# a row crossing a 128-point segment; two segment seams; a y-block seam (2 * 8 + 2 rows); a z-chunk seam with the
# window carried across it (16 + 3 planes); one aligned axis; four z-chunk seams; two y-block seams
SHAPES = [(2, 2, 2), (3, 3, 3), (4, 4, 4), (5, 4, 6), (7, 6, 2), (130, 6, 4), (258, 3, 2), (6, 18, 4), (4, 4, 19),
          (63, 64, 6), (4, 4, 70), (6, 20, 4)]


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    assert torch.cuda.is_available(), "GPU tests need a GPU (no CPU fallback exists)"


def st():
    return torch.cuda.current_stream().cuda_stream


def sid(shape):
    return "x".join(str(n) for n in shape)


def half(shape):
    return tuple(n // 2 for n in shape)


def inner(a):
    return a[1:-1, 1:-1, 1:-1]


def same(a, b, what):
    ne = np.ascontiguousarray(a).view(np.int64) != np.ascontiguousarray(b).view(np.int64)
    assert a.shape == b.shape and not ne.any(), f"{what}: {int(ne.sum())} words differ, first at {tuple(np.argwhere(ne)[0])}"


class Tables:
    """Device copies of one transition's tables and the gs_fmg_tables that describes them."""

    def __init__(self, fine, coarse=None):
        coarse = half(fine) if coarse is None else coarse
        self.keep, self.abi = [], gsv.gs_fmg_tables()
        for a in range(3):
            T = gsv.fmg_axis(fine[a])
            self.abi.nf[a], self.abi.nc[a] = fine[a], coarse[a]
            for key in ("cj", "cw"):
                t = torch.from_numpy(np.ascontiguousarray(T[key]).reshape(-1)).cuda()
                self.keep.append(t)
                getattr(self.abi, key)[a] = t.data_ptr()


@functools.lru_cache(maxsize=None)
def coarse_input(shape):
    """Seeded noise on the coarse interior, zero ring; read-only."""
    rng = np.random.default_rng(shape[0] + 1000 * shape[1] + 1000003 * shape[2])
    a = np.zeros(tuple(n + 2 for n in half(shape)))
    inner(a)[...] = rng.uniform(-1.0, 1.0, half(shape))
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def reference(shape):
    r = PA.prolong(coarse_input(shape), shape)
    r.setflags(write=False)
    return r


def ring_noise(shape):
    """A padded fine array: finite non-zero noise in the ring, NaN in the interior."""
    rng = np.random.default_rng(sum(shape))
    a = np.where(rng.random(tuple(n + 2 for n in shape)) < 0.5, -1.0, 1.0) * rng.uniform(0.5, 50.0, tuple(n + 2 for n in shape))
    inner(a)[...] = np.nan
    return a


class Run:
    """gs_fmg_prolong_pa on one shape in one layout with every contract check: the coarse input NaN-poisoned outside
    its padded box and unchanged word for word afterwards; the fine output NaN everywhere but its ring of noise, of
    which exactly the interior is written."""

    def __init__(self, shape, lid="default"):
        self.shape, self.cshape, self.lid = shape, half(shape), lid
        self.T = Tables(shape)
        self.hf, self.hc = 1.0 / (shape[1] + 1), 1.0 / (self.cshape[1] + 1)

    def fld(self, dims, role):
        lay = layouts(*dims)[self.lid]
        return LayoutField(*dims, lay.ldy, lay.ldz, lay.phase_in if role == "in" else lay.phase_out)

    def fields(self):
        cf = self.fld(self.cshape, "in")
        cf.poison_all(POISON_IN).from_xyz(coarse_input(self.shape))
        cf.snapshot()
        ff = self.fld(self.shape, "out")
        ff.poison_all().from_xyz(ring_noise(self.shape))
        ff.snapshot()
        return cf, ff

    def prolong(self):
        cf, ff = self.fields()
        rc = gsv.transfer().gs_fmg_prolong_pa(cf.ptr, C.byref(cf.level(self.hc)), ff.ptr, C.byref(ff.level(self.hf)),
                                              C.byref(self.T.abi), st())
        assert rc == 0, rc
        ff.assert_unchanged(~ff.interior_mask(), "gs_fmg_prolong_pa: outside the fine interior")
        cf.assert_unchanged(what="gs_fmg_prolong_pa: the coarse input")
        got = ff.to_xyz()
        assert not np.isnan(inner(got)).any(), "an interior fine point was not written"
        return got


# ---- kernel level -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_prolong_pa_bitwise(shape):
    same(inner(Run(shape).prolong()), inner(reference(shape)), "fine interior")


LAYOUT_SHAPES = [(6, 5, 4), (130, 6, 4)]


@pytest.mark.parametrize("lid", LAYOUT_IDS)
@pytest.mark.parametrize("shape", LAYOUT_SHAPES, ids=sid)
def test_layout_contract(shape, lid):
    same(inner(Run(shape, lid).prolong()), inner(reference(shape)), f"fine interior, layout {lid}")


@pytest.mark.parametrize("lid", ["default", "tight_odd"])
def test_einval_writes_nothing(lid):
    shape, t = (6, 5, 4), gsv.transfer()
    r = Run(shape, lid)
    cf, ff = r.fields()
    fl, cl = ff.level(r.hf), cf.level(r.hc)
    T, other = r.T.abi, Tables((8, 5, 4)).abi
    nullp = gsv.gs_fmg_tables()
    C.memmove(C.byref(nullp), C.byref(T), C.sizeof(T))
    nullp.cw[1] = None

    def lvl(base, **kw):
        L = gsv.gs_level(base.nx, base.ny, base.nz, base.ldy, base.ldz, base.z0, base.h)
        for k, val in kw.items():
            setattr(L, k, val)
        return L

    cases = [(fl, cl, other), (fl, cl, nullp), (fl, cl, None), (lvl(fl, ldy=fl.nx + 1), cl, T),
             (fl, lvl(cl, ldz=cl.ldy * (cl.ny + 2) - 1), T), (fl, lvl(cl, nx=cl.nx + 1, ldy=cl.ldy + 1), T),
             (lvl(fl, z0=2), cl, T), (fl, lvl(cl, z0=1), T), (fl, lvl(cl, nz=-1), T), (None, cl, T), (fl, None, T)]
    for i, (a, b, tab) in enumerate(cases):
        pa, pb = (C.byref(a) if a is not None else None), (C.byref(b) if b is not None else None)
        pt = C.byref(tab) if tab is not None else None
        assert t.gs_fmg_prolong_pa(cf.ptr, pb, ff.ptr, pa, pt, st()) == EINVAL, i
    assert t.gs_fmg_prolong_pa(None, C.byref(cl), ff.ptr, C.byref(fl), C.byref(T), st()) == EINVAL
    assert t.gs_fmg_prolong_pa(cf.ptr, C.byref(cl), None, C.byref(fl), C.byref(T), st()) == EINVAL
    ff.assert_unchanged(what="fine output after EINVAL")
    cf.assert_unchanged(what="coarse input after EINVAL")


# ---- driver -------------------------------------------------------------------------------------------------------
def params(dims, mode=gsv.GS_LINEAR, cycles=1):
    return gsv.GridParams(maxiter=cycles, tol=0.0, gridDim=dims, mode=mode)


def gpu_fmg(dims, mode=gsv.GS_LINEAR, k=1, prolong="position", transfer="position", weights=None):
    with gsv.HipGridData(params(dims, mode)) as g:
        g.set_transfer(transfer)
        g.set_fmg_prolong(prolong)
        assert g.fmg_prolong == prolong
        if weights is not None:
            g.set_weights(weights, weights)
        res = gsv.HipSolver.fmg(g, k)
        return g.field(0, "v"), res, g.fmg_start_level()


@functools.lru_cache(maxsize=None)
def ref_fmg(dims, mode, k, weights=(0.8, 0.8)):
    v, res = PA.fmg(dims, mode, k, pre=weights, post=weights)
    v.setflags(write=False)
    return v, res


FUSED = (46, 46, 46)  # tests/test_gpu_transfer.py: the smallest cube whose level 0 smooths in fused pairs across a
# non-aligned transition


@pytest.mark.parametrize("dims,k", [((32, 32, 32), 1), ((32, 32, 32), 2), ((40, 32, 24), 1), ("fused", 1)], ids=str)
def test_linear_fmg_matches_the_composition(dims, k):
    if dims == "fused":
        dims = FUSED
        with gsv.HipGridData(params(dims)) as g:
            assert bool(gsv.driver().gs_grid_level_fused(g.handle, 0)) and not g.level_aligned(0)
    v, res, s = gpu_fmg(dims, k=k)
    want_v, want_res = ref_fmg(dims, O.LINEAR, k)
    print(f"{dims} FMG({k}): residual {res!r}, composition {want_res!r}")
    assert s == len(level_dims(dims)) - 1
    same(v, want_v, "level-0 v")
    assert rel(res, want_res) <= 1e-12


def test_mixed_transitions_start_at_the_coarsest_level():
    """95 -> 47 -> 23 -> 11 -> 5 -> 2 are aligned, 2 -> 1 is not: the ALIGNED prolongation starts at the 2^3 level
    (tests/test_gpu_fmg.py), POSITION at the 1^3 level below it."""
    dims = (95, 95, 95)
    ld = level_dims(dims)
    v, res, s = gpu_fmg(dims)
    want_v, want_res = ref_fmg(dims, O.LINEAR, 1)
    print(f"95^3 FMG(1): residual {res!r}, composition {want_res!r}")
    assert s == len(ld) - 1 == 6 and ld[s] == (1, 1, 1)
    same(v, want_v, "level-0 v")
    assert rel(res, want_res) <= 1e-12


def test_linear_fmg_with_chebyshev_weights():
    dims, w = (32, 32, 32), gsv.chebyshev_weights(2)
    v, res, _ = gpu_fmg(dims, weights=w)
    want_v, want_res = ref_fmg(dims, O.LINEAR, 1, tuple(w))
    same(v, want_v, "level-0 v")
    assert rel(res, want_res) <= 1e-12


def test_nonlinear_fmg_matches_the_composition():
    dims = (32, 32, 32)
    v, res, _ = gpu_fmg(dims, gsv.GS_NONLINEAR)
    want_v, want_res = ref_fmg(dims, O.NONLINEAR, 1)
    d = np.abs(v - want_v).max()
    print(f"max field difference {d} of {np.abs(want_v).max()}, residual {res!r}, composition {want_res!r}")
    assert d <= 1e-10 * np.abs(want_v).max()
    assert rel(res, want_res) <= 1e-9


@pytest.mark.parametrize("transfer", ["reference", "position"])
def test_aligned_grid_is_unchanged(transfer):
    dims = (63, 63, 63)
    v0, r0, s0 = gpu_fmg(dims, prolong="aligned", transfer=transfer)
    v1, r1, s1 = gpu_fmg(dims, prolong="position", transfer=transfer)
    assert s0 == s1 == len(level_dims(dims)) - 1
    same(v1, v0, "level-0 v")
    assert r1 == r0


def test_fmg_beats_three_position_cycles_at_64():
    dims = (64, 64, 64)
    with gsv.HipGridData(params(dims, cycles=3)) as g:
        g.set_transfer("position")
        plain = gsv.HipSolver.solve(g)
    _, res, _ = gpu_fmg(dims)
    print("FMG(1)", res, "plain POSITION history", plain)
    assert res < plain[3]


# ---- refusals and switches ----------------------------------------------------------------------------------------
def test_position_prolong_needs_position_transfers():
    dims = (32, 32, 32)
    rng = np.random.default_rng(3)
    v0 = np.zeros(tuple(n + 2 for n in dims))
    inner(v0)[...] = rng.standard_normal(dims)
    with gsv.HipGridData(params(dims)) as g:
        g.set_fmg_prolong("position")
        g.set_field(0, "v", v0)
        before, f1 = g.field(0, "v"), g.field(1, "f")
        assert g.transfer == "reference"
        with pytest.raises(gsv.GpuSolveError, match="gs_grid_set_transfer") as e:
            gsv.HipSolver.fmg(g, 1)
        assert "GS_TRANSFER=position" in str(e.value)
        same(g.field(0, "v"), before, "level-0 v after the refusal")
        same(g.field(1, "f"), f1, "level-1 f after the refusal")
        g.set_transfer("position")
        assert gsv.HipSolver.fmg(g, 1) > 0.0
        with pytest.raises(gsv.GpuSolveError, match="at least 1"):
            gsv.HipSolver.fmg(g, 0)
        with pytest.raises(ValueError):
            g.set_fmg_prolong("nonsense")
        assert gsv.driver().gs_grid_set_fmg_prolong(g.handle, 7) == 1 and b"fmg prolong" in gsv.driver().gs_last_error()
        assert g.fmg_prolong == "position"


def test_newton_is_refused():
    with gsv.HipGridData(params((32, 32, 32), gsv.GS_NEWTON)) as g:
        g.set_transfer("position")
        g.set_fmg_prolong("position")
        assert g.fmg_start_level() == 0
        with pytest.raises(gsv.GpuSolveError, match="NEWTON"):
            gsv.HipSolver.fmg(g, 1)


def test_zslab_grid_is_refused(monkeypatch):
    """A Z-slab grid (the loopback emulation: two ranks on one device) under GS_FMG with the POSITION prolongation:
    the solve fails with FMG's single-GPU message before any work."""
    p = params((70, 33, 41))
    cap = 16
    hist, cnt, ap = (C.c_double * cap)(*([-1.0] * cap)), C.c_int(-1), p.to_abi()
    monkeypatch.setenv("GS_FMG", "1")
    monkeypatch.setenv("GS_FMG_PROLONG", "position")
    rc = gsv.driver().gs_zslab_loopback_run(C.byref(ap), 2, 1000, 0, 1, hist, cap, C.byref(cnt), None)
    assert rc == 1
    msg = gsv.driver().gs_last_error().decode()
    assert "FMG" in msg and "single-GPU" in msg, msg
    assert cnt.value == -1 and all(x == -1.0 for x in hist)


def test_default_keeps_the_alignment_requirement():
    with gsv.HipGridData(params((32, 32, 32))) as g:
        assert g.fmg_prolong == "aligned"
        for mode in ("reference", "position"):
            g.set_transfer(mode)
            assert g.fmg_start_level() == 0
        g.set_fmg_prolong("position")
        assert g.fmg_start_level() == g.numLevels() - 1
        g.set_fmg_prolong("aligned")
        assert g.fmg_start_level() == 0


CHILD = """
import sys
sys.path[:0] = {paths!r}
import gpusolve as gsv
p = gsv.GridParams(maxiter=1, tol=0.0, gridDim=(32, 32, 32))
with gsv.HipGridData(p) as g:
    hist = gsv.HipSolver.solve(g)
    print(g.fmg_prolong, g.transfer, " ".join(x.hex() for x in hist), g.field(0, "v").tobytes().hex()[-64:])
"""


def test_environment_switch(monkeypatch):
    """GS_FMG=1 GS_TRANSFER=position GS_FMG_PROLONG=position through gs_grid_solve: the history's FMG entry is the
    direct call's residual, and the V-cycle after it starts from the direct call's field — also with the fine stores
    forced non-temporal (GS_FMG_NT=1: the path levels of 2^25 points and more take)."""
    dims = (32, 32, 32)
    with gsv.HipGridData(params(dims)) as g:
        g.set_transfer("position")
        g.set_fmg_prolong("position")
        res = gsv.HipSolver.fmg(g, 1)
        after = gsv.HipSolver.vcycle(g)
        v = g.field(0, "v")
    paths = [os.path.join(REPO, "gpu-solve_amd")]
    for extra in ({}, {"GS_FMG_NT": "1"}):
        env = dict(os.environ, GS_FMG="1", GS_TRANSFER="position", GS_FMG_PROLONG="position", **extra)
        out = subprocess.run([sys.executable, "-c", CHILD.format(paths=paths)], capture_output=True, text=True,
                             timeout=120, env=env)
        assert out.returncode == 0, out.stderr
        prolong, transfer, *rest = out.stdout.split()
        assert (prolong, transfer) == ("position", "position")
        hist = [float.fromhex(x) for x in rest[:-1]]
        assert len(hist) == 3 and rel(hist[1], res) <= 1e-12 and rel(hist[2], after) <= 1e-12, (hist, res, after)
        assert rest[-1] == v.tobytes().hex()[-64:]
    monkeypatch.setenv("GS_FMG_PROLONG", "aligned")
    with gsv.HipGridData(params(dims)) as g:
        assert g.fmg_prolong == "aligned"
    monkeypatch.setenv("GS_FMG_PROLONG", "position")
    with gsv.HipGridData(params(dims)) as g:
        assert g.fmg_prolong == "position"
    monkeypatch.setenv("GS_FMG_PROLONG", "nonsense")
    with pytest.raises(gsv.GpuSolveError, match="GS_FMG_PROLONG=nonsense"):
        gsv.HipGridData(params(dims))
