"""The position-aware grid transfers on the GPU (include/gpusolve_transfer.h): the three launchers of
libgpusolve_transfer.so against tests/xfer_ref.py and under the kernel ABI's layout contract, and POSITION mode
through the driver (gs_grid_set_transfer, GS_TRANSFER) against the V-cycle composed of xfer_ref's operators and the
CPU oracle's.

Tolerances. The two transfer kernels, and everything LINEAR, are bit for bit: the numpy restatement rounds every
product and sum as the kernels do. The fused residual + restriction outside LINEAR mode is within 1e-12 of the coarse
field's maximum (ocml's exp against glibc's, GS_NEWTON_B's re-associated product: an ulp of one term of the residual).
Driver fields outside LINEAR mode to 1e-10 of the field's maximum and histories inside the 1e-6 contract, as the rest
of the suite. The convergence cap 0.4 per cycle is tests/test_transfer_cpu.py's (measured there: at most 0.35)."""
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
import xfer_ref as X  # noqa: E402
from conftest import REPO, rel  # noqa: E402
from layout_field import LAYOUT_IDS, POISON_IN, LayoutField, layouts  # noqa: E402

EINVAL = gsv._abi.GS_EINVAL
GAMMA = 1.0
CAP = 0.4
SWITCHES = ("GS_TRANSFER", "GS_OMEGAS", "GS_FMG", "GS_NO_FUSED_RR", "GS_NO_FUSED_SWEEPS", "GS_COARSE_POINTS",
            "GS_TILE_POINTS", "GS_NO_SPECULATION", "GS_ZSLAB_MIN_POINTS")
UNIT = gsv.Stencil().to_abi()
# the smallest shapes that reach each edge of the kernels: one coarse point; every axis non-aligned; mixed aligned and
# non-aligned axes; rows crossing one and two x-tiles with a ragged last one (coarse 65 and 129 columns); two y-blocks
# with a ragged last one; z-chunks (4 coarse planes) crossed twice with a last chunk of one plane (coarse 9) and eight
# times with one of three (coarse 35); an odd and an even axis of >= 129 points
SHAPES = [(2, 2, 2), (4, 4, 4), (6, 5, 4), (3, 2, 9), (130, 6, 4), (258, 3, 2), (66, 10, 9), (8, 8, 18), (8, 8, 70),
          (130, 129, 2)]


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


def rand_full(rng, dims, scale=1.0):
    a = np.zeros(tuple(n + 2 for n in dims))
    inner(a)[...] = rng.uniform(-scale, scale, dims)
    return a


def noisy(a):
    """`a` with its ring replaced by finite non-zero noise (no path may read the rings of f and w)."""
    rng = np.random.default_rng(a.size)
    out = np.where(rng.random(a.shape) < 0.5, -1.0, 1.0) * rng.uniform(0.5, 50.0, a.shape)
    inner(out)[...] = inner(a)
    return out


class Tables:
    """Device copies of one transition's tables and the gs_transfer_tables that describes them."""

    def __init__(self, fine, coarse=None):
        coarse = half(fine) if coarse is None else coarse
        self.keep, self.abi = [], gsv.gs_transfer_tables()
        for a in range(3):
            T = gsv.transfer_axis(fine[a])
            self.abi.nf[a], self.abi.nc[a] = fine[a], coarse[a]
            for key in ("pj", "pt", "rlo", "rcnt", "rw"):
                t = torch.from_numpy(np.ascontiguousarray(T[key]).reshape(-1)).cuda()
                self.keep.append(t)
                getattr(self.abi, key)[a] = t.data_ptr()


@functools.lru_cache(maxsize=None)
def inputs(shape):
    """Fine v (+-1), f (+-100), w (+-0.8), coarse c and sub (+-1), all with zero rings; read-only."""
    rng = np.random.default_rng(shape[0] + 1000 * shape[1] + 1000003 * shape[2])
    out = [rand_full(rng, shape), rand_full(rng, shape, 100.0), rand_full(rng, shape, 0.8),
           rand_full(rng, half(shape)), rand_full(rng, half(shape))]
    for a in out:
        a.setflags(write=False)
    return out


def w_of(shape, mode):
    w = inputs(shape)[2]
    return {0: None, 1: None, 2: w, 3: GAMMA * (1.0 + w) * np.exp(w), 4: np.full_like(w, GAMMA)}[mode]


class Run:
    """The three launchers on one shape in one layout, with every contract check: outputs NaN-poisoned, exactly the
    documented set written, every input unchanged word for word (its poison outside the box included)."""

    def __init__(self, shape, lid="default"):
        self.shape, self.cshape, self.lid = shape, half(shape), lid
        self.t = gsv.transfer()
        self.T = Tables(shape)
        self.hf, self.hc = 1.0 / (shape[1] + 1), 1.0 / (self.cshape[1] + 1)
        self.inputs = []

    def fld(self, dims, role):
        lay = layouts(*dims)[self.lid]
        return LayoutField(*dims, lay.ldy, lay.ldz, lay.phase_in if role == "in" else lay.phase_out)

    def inp(self, box, ring_noise=False, role="in"):
        f = self.fld(tuple(n - 2 for n in box.shape), role)
        f.poison_all(POISON_IN).from_xyz(noisy(box) if ring_noise else box)
        f.snapshot()
        self.inputs.append(f)
        return f

    def out(self, dims):
        return self.fld(dims, "out").poison_all()

    def done(self, what):
        for i, f in enumerate(self.inputs):
            f.assert_unchanged(what=f"{what}: input {i}")

    def levels(self, fine, coarse):
        return C.byref(fine.level(self.hf)), C.byref(coarse.level(self.hc))

    def restrict(self, two):
        src = self.inp(inputs(self.shape)[0])
        a, b = self.out(self.cshape), self.out(self.cshape) if two else None
        fl, cl = self.levels(src, a)
        rc = self.t.gs_restrict_pa(src.ptr, fl, a.ptr, b.ptr if two else None, cl, C.byref(self.T.abi), st())
        assert rc == 0, rc
        for o in (a, b) if two else (a,):
            o.assert_written_exactly(o.interior_mask(), "gs_restrict_pa")
        self.done("gs_restrict_pa")
        return [inner(o.to_xyz()) for o in ((a, b) if two else (a,))]

    def prolong(self, sub):
        v, _, _, c, s = inputs(self.shape)
        cf, sf = self.inp(c), self.inp(s) if sub else None
        fv = self.fld(self.shape, "out")
        fv.poison_all(POISON_IN).from_xyz(v)
        fv.snapshot()
        cl, fl = C.byref(cf.level(self.hc)), C.byref(fv.level(self.hf))
        rc = self.t.gs_prolong_add_pa(cf.ptr, sf.ptr if sub else None, cl, fv.ptr, fl, C.byref(self.T.abi), st())
        assert rc == 0, rc
        fv.assert_unchanged(~fv.interior_mask(), "gs_prolong_add_pa: outside the fine interior")
        self.done("gs_prolong_add_pa")
        return fv.to_xyz()

    def fused(self, mode, stencil=UNIT):
        v, f, _, _, _ = inputs(self.shape)
        w = w_of(self.shape, mode)
        vf, ff = self.inp(v), self.inp(f, ring_noise=True, role="out")
        wf = self.inp(w, ring_noise=True) if w is not None else None
        o = self.out(self.cshape)
        fl, cl = self.levels(vf, o)
        rc = self.t.gs_residual_restrict_pa(C.byref(stencil), fl, mode, GAMMA, vf.ptr, ff.ptr,
                                            wf.ptr if wf is not None else None, o.ptr, cl, C.byref(self.T.abi), st())
        assert rc == 0, rc
        o.assert_written_exactly(o.interior_mask(), "gs_residual_restrict_pa")
        self.done("gs_residual_restrict_pa")
        return inner(o.to_xyz())

    def two_pass(self, mode):
        """gs_residual with a stored r, then gs_restrict_pa: the composition the fused kernel replaces."""
        v, f, _, _, _ = inputs(self.shape)
        w = w_of(self.shape, mode)
        vf, ff = self.inp(v), self.inp(f, ring_noise=True, role="out")
        wf = self.inp(w, ring_noise=True) if w is not None else None
        r = self.fld(self.shape, "out")
        r.buf.zero_()
        o = self.out(self.cshape)
        fl, cl = self.levels(vf, o)
        rc = gsv.kernels().gs_residual(C.byref(UNIT), fl, mode, GAMMA, vf.ptr, ff.ptr, wf.ptr if wf is not None else None,
                                       r.ptr, None, st())
        assert rc == 0, rc
        rc = self.t.gs_restrict_pa(r.ptr, C.byref(r.level(self.hf)), o.ptr, None, cl, C.byref(self.T.abi), st())
        assert rc == 0, rc
        return inner(o.to_xyz())


def ref_fused(shape, mode):
    v, f, w, _, _ = inputs(shape)
    h = 1.0 / (shape[1] + 1)
    if mode in (0, 1):
        r, _ = O.residual(v, f, h, mode, GAMMA)
    else:  # 2 / 3: the Newton operator at w; 4: B = gamma everywhere, the operator at w = 0
        r, _ = O.residual(v, f, h, O.NEWTON, GAMMA, w=np.zeros_like(w) if mode == 4 else np.ascontiguousarray(w))
    return inner(X.restrict(r, shape))


# ---- kernel level -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_restrict_pa(shape):
    want = inner(X.restrict(inputs(shape)[0], shape))
    a, b = Run(shape).restrict(two=True)
    same(a, want, "coarse_a")
    same(b, want, "coarse_b")
    same(Run(shape).restrict(two=False)[0], want, "one output")


@pytest.mark.parametrize("sub", [False, True], ids=["plain", "fas"])
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_prolong_add_pa(shape, sub):
    v, _, _, c, s = inputs(shape)
    d = c - s if sub else c
    want = v + X.prolong(d, shape)
    got = Run(shape).prolong(sub)
    same(inner(got), inner(want), "fine interior")


@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_residual_restrict_pa(shape, mode):
    got, want = Run(shape).fused(mode), ref_fused(shape, mode)
    if mode == 0:
        same(got, want, "coarse f")
        same(got, Run(shape).two_pass(0), "fused against gs_residual + gs_restrict_pa")
    else:
        d = np.abs(got - want).max()
        print("max difference", d, "of", np.abs(want).max())
        assert d <= 1e-12 * np.abs(want).max()


def test_residual_restrict_pa_general_stencil():
    """A stencil outside the canonical order and with non-unit weights takes the same kernel (the general sum)."""
    shape = (66, 10, 9)
    values = (-1, -1.25, 6.5, -1, -0.75, -1, -1)
    offsets = [(0, 0, 1), (-1, 0, 0), (0, 0, 0), (0, 0, -1), (1, 0, 0), (0, 1, 0), (0, -1, 0)]
    v, f, _, _, _ = inputs(shape)
    r, _ = O.residual(v, f, 1.0 / (shape[1] + 1), O.LINEAR, GAMMA, stencil=O.Stencil.make(values, offsets))
    got = Run(shape).fused(0, gsv.Stencil(list(values), offsets).to_abi())
    same(got, inner(X.restrict(r, shape)), "general stencil")


# ---- layout contract ----------------------------------------------------------------------------------------------
LAYOUT_SHAPES = [(6, 5, 4), (130, 6, 4), (66, 10, 9)]


@functools.lru_cache(maxsize=None)
def default_results(shape):
    r = Run(shape)
    return {"restrict": r.restrict(True), "plain": r.prolong(False), "fas": r.prolong(True),
            **{m: r.fused(m) for m in (0, 1, 3)}}


@pytest.mark.parametrize("lid", [l for l in LAYOUT_IDS if l != "default"])
@pytest.mark.parametrize("shape", LAYOUT_SHAPES, ids=sid)
def test_layout_contract(shape, lid):
    """Every launcher in every layout: Run makes the contract's checks (NaN outside every input's box, noise in the
    rings of f and w, the written set, the inputs); the values equal the default-layout call's bit for bit."""
    want, r = default_results(shape), Run(shape, lid)
    for got, ref in zip(r.restrict(True), want["restrict"]):
        same(got, ref, "gs_restrict_pa")
    same(r.prolong(False), want["plain"], "gs_prolong_add_pa")
    same(r.prolong(True), want["fas"], "gs_prolong_add_pa (sub)")
    for m in (0, 1, 3):
        same(r.fused(m), want[m], f"gs_residual_restrict_pa mode {m}")


@pytest.mark.parametrize("lid", ["default", "tight_odd"])
def test_einval_writes_nothing(lid):
    shape, t = (6, 5, 4), gsv.transfer()
    r = Run(shape, lid)
    v, f, _, c, _ = inputs(shape)
    fine, ff, coarse = r.inp(v), r.inp(f), r.inp(c)
    fo, co = r.fld(shape, "out").poison_all().snapshot(), r.out(half(shape)).snapshot()
    fl, cl = fine.level(r.hf), coarse.level(r.hc)
    T, other = r.T.abi, Tables((8, 5, 4)).abi
    nullp = gsv.gs_transfer_tables()
    C.memmove(C.byref(nullp), C.byref(T), C.sizeof(T))
    nullp.rw[1] = None

    def lvl(base, **kw):
        L = gsv.gs_level(base.nx, base.ny, base.nz, base.ldy, base.ldz, base.z0, base.h)
        for k, val in kw.items():
            setattr(L, k, val)
        return L

    cases = [(fl, cl, other), (fl, cl, nullp), (fl, cl, None), (lvl(fl, ldy=fl.nx + 1), cl, T),
             (fl, lvl(cl, ldz=cl.ldy * (cl.ny + 2) - 1), T), (fl, lvl(cl, nx=cl.nx + 1, ldy=cl.ldy + 1), T),
             (lvl(fl, z0=2), cl, T), (fl, lvl(cl, nz=-1), T), (None, cl, T)]
    for i, (a, b, tab) in enumerate(cases):
        pa, pb = (C.byref(a) if a is not None else None), C.byref(b)
        pt = C.byref(tab) if tab is not None else None
        assert t.gs_restrict_pa(fine.ptr, pa, co.ptr, co.ptr, pb, pt, st()) == EINVAL, i
        assert t.gs_prolong_add_pa(coarse.ptr, None, pb, fo.ptr, pa, pt, st()) == EINVAL, i
        for mode in (0, 3):
            assert t.gs_residual_restrict_pa(C.byref(UNIT), pa, mode, GAMMA, fine.ptr, ff.ptr, fine.ptr, co.ptr, pb, pt,
                                             st()) == EINVAL, i
    ok_f, ok_c, ok_t = C.byref(fl), C.byref(cl), C.byref(T)
    assert t.gs_restrict_pa(None, ok_f, co.ptr, None, ok_c, ok_t, st()) == EINVAL
    assert t.gs_restrict_pa(fine.ptr, ok_f, None, co.ptr, ok_c, ok_t, st()) == EINVAL
    assert t.gs_prolong_add_pa(None, None, ok_c, fo.ptr, ok_f, ok_t, st()) == EINVAL
    assert t.gs_prolong_add_pa(coarse.ptr, None, ok_c, None, ok_f, ok_t, st()) == EINVAL
    for mode, w in ((5, fine.ptr), (-1, fine.ptr), (2, None), (3, None), (4, None)):
        assert t.gs_residual_restrict_pa(C.byref(UNIT), ok_f, mode, GAMMA, fine.ptr, ff.ptr, w, co.ptr, ok_c, ok_t,
                                         st()) == EINVAL, mode
    assert t.gs_residual_restrict_pa(None, ok_f, 0, GAMMA, fine.ptr, ff.ptr, None, co.ptr, ok_c, ok_t, st()) == EINVAL
    assert t.gs_residual_restrict_pa(C.byref(UNIT), ok_f, 0, GAMMA, fine.ptr, ff.ptr, None, None, ok_c, ok_t, st()) == EINVAL
    bad = gsv.Stencil([6, -1, -1, -1, -1, -1, -1], [(0, 0, 0), (2, 0, 0)] + list(gsv.CANONICAL_OFFSETS[2:])).to_abi()
    assert t.gs_residual_restrict_pa(C.byref(bad), ok_f, 0, GAMMA, fine.ptr, ff.ptr, None, co.ptr, ok_c, ok_t, st()) == EINVAL
    fo.assert_unchanged(what="fine output after EINVAL")
    co.assert_unchanged(what="coarse output after EINVAL")
    r.done("EINVAL")


# ---- driver -------------------------------------------------------------------------------------------------------
def params(dims, mode=gsv.GS_LINEAR, cycles=3):
    return gsv.GridParams(maxiter=cycles, tol=0.0, gridDim=dims, mode=mode)


def solve(p, transfer=None, fields=("v",)):
    with gsv.HipGridData(p) as g:
        if transfer is not None:
            g.set_transfer(transfer)
            assert g.transfer == transfer
        hist = gsv.HipSolver.solve(g)
        return hist, [g.field(0, n) for n in fields]


@functools.lru_cache(maxsize=None)
def ref_solve(dims, mode, cycles, transfer="position", weights=None):
    w = weights or (0.8, 0.8)
    c = X.Cycle(dims, mode, pre=w, post=w, transfer=transfer)
    hist = c.solve(cycles)
    c.v[0].setflags(write=False)
    return hist, c.v[0]


def assert_hist(got, want, tol):
    assert len(got) == len(want), (got, want)
    for a, b in zip(got, want):
        assert rel(a, b) < tol, (got, want)


def level0_fused_nonaligned(n):
    with gsv.HipGridData(params((n, n, n))) as g:
        return bool(gsv.driver().gs_grid_level_fused(g.handle, 0)) and not g.level_aligned(0)


@functools.lru_cache(maxsize=None)
def smallest_fused_nonaligned_cube():
    """The smallest cube whose level 0 smooths in fused pairs and whose first transition is not aligned."""
    return next(n for n in range(2, 129) if level0_fused_nonaligned(n))


def test_smallest_fused_nonaligned_cube():
    n = smallest_fused_nonaligned_cube()
    # 4-row blocks of 4-plane chunks: the pair takes a level from 128 such blocks, 12 x 12 at 45 and 46; 45 is aligned
    assert n == 46
    assert level0_fused_nonaligned(n) and not level0_fused_nonaligned(n - 2)


@pytest.mark.parametrize("dims", [(6, 5, 4), (12, 10, 8), (32, 32, 32), (64, 64, 64), "fused"], ids=str)
def test_linear_vcycles_match_the_composition(dims):
    """6x5x4 ... 32^3: single sweeps; 64^3: levels 1.. would otherwise run the tiled steps; the last shape smooths
    level 0 in fused pairs (with the speculative pair) around the position-aware transfers."""
    if dims == "fused":
        dims = (smallest_fused_nonaligned_cube(),) * 3
    hist, (v,) = solve(params(dims), "position")
    want_h, want_v = ref_solve(dims, O.LINEAR, 3)
    print("history", hist, "composition", want_h)
    same(v, want_v, "level-0 v")
    assert_hist(hist, want_h, 1e-9)


def test_linear_vcycles_with_chebyshev_weights(monkeypatch):
    monkeypatch.setenv("GS_OMEGAS", "cheb")
    dims = (32, 32, 32)
    hist, (v,) = solve(params(dims), "position")
    want_h, want_v = ref_solve(dims, O.LINEAR, 3, weights=gsv.chebyshev_weights(2))
    same(v, want_v, "level-0 v")
    assert_hist(hist, want_h, 1e-9)


@pytest.mark.parametrize("dims", [(32, 32, 32), (40, 32, 24)], ids=sid)
def test_nonlinear_vcycles_match_the_composition(dims):
    hist, (v,) = solve(params(dims, gsv.GS_NONLINEAR), "position")
    want_h, want_v = ref_solve(dims, O.NONLINEAR, 3)
    d = np.abs(v - want_v).max()
    print("max field difference", d, "of", np.abs(want_v).max(), "history", hist, want_h)
    assert d <= 1e-10 * np.abs(want_v).max()
    assert_hist(hist, want_h, 1e-6)


@pytest.mark.parametrize("dims", [(32, 32, 32), (40, 32, 24)], ids=sid)
def test_newton_matches_the_composition(dims):
    """Four Newton iterations. The position-aware history decreases monotonically and ends below the default
    mode's. (Measured with the CPU composition, 32^3: position 36.7, 1.30, 0.0476, 0.00180, 6.9e-5; default 36.7,
    2.95, 0.275, 0.0265, 0.00257 — at these sizes the default history decreases too, more slowly: its inner solves
    stop at their ten-cycle limit, not at their tolerance.)"""
    p = params(dims, gsv.GS_NEWTON, cycles=4)
    hist, (w,) = solve(p, "position", fields=("newtonV",))
    default, _ = solve(p)
    want_h, want_w = X.newton_solve(dims, 4)
    d = np.abs(w - want_w).max()
    print("max newtonV difference", d, "of", np.abs(want_w).max(), "history", hist, want_h, "default", default)
    assert d <= 1e-10 * np.abs(want_w).max()
    assert_hist(hist, want_h, 1e-6)
    assert all(b < a for a, b in zip(hist, hist[1:])), hist
    assert hist[-1] < default[-1]


@pytest.mark.parametrize("mode", [gsv.GS_LINEAR, gsv.GS_NONLINEAR, gsv.GS_NEWTON])
@pytest.mark.parametrize("dims", [(31, 31, 31), (63, 31, 15)], ids=sid)
def test_aligned_grids_are_unchanged(dims, mode):
    p = params(dims, mode, cycles=2)
    names = ("v", "newtonV") if mode == gsv.GS_NEWTON else ("v",)
    want = solve(p, fields=names)
    with gsv.HipGridData(p) as g:
        g.set_transfer("position")
        assert all(g.level_aligned(l) for l in range(g.numLevels() - 1))
        with pytest.raises(IndexError):
            g.level_aligned(g.numLevels() - 1)
        hist = gsv.HipSolver.solve(g)
        got = [g.field(0, n) for n in names]
    assert hist == want[0]
    for a, b in zip(got, want[1]):
        same(a, b, "aligned grid")


def test_convergence_at_64():
    """64^3 LINEAR, ten cycles: the default transfers' residual grows again, the position-aware ones
    reduce it by at least 2.5x in every one of cycles 3-10."""
    p = params((64, 64, 64), cycles=10)
    default, _ = solve(p)
    hist, _ = solve(p, "position")
    f = [b / a for a, b in zip(hist, hist[1:])]
    print("default", default, "position", hist, "factors", f)
    assert default[10] > default[3]
    assert all(x <= CAP for x in f[2:]), f


def test_switching_reproduces_the_bits():
    dims = (12, 10, 8)
    p = params(dims, cycles=2)
    want_pos, want_ref = solve(p, "position"), solve(p)
    zero = np.zeros(tuple(n + 2 for n in dims))
    with gsv.HipGridData(p) as g:
        assert g.transfer == "reference" and not g.level_aligned(0)
        for mode, want in (("position", want_pos), ("reference", want_ref), ("position", want_pos)):
            g.set_transfer(mode)
            g.set_field(0, "v", zero)
            assert gsv.HipSolver.solve(g) == want[0], mode
            same(g.field(0, "v"), want[1][0], mode)
        with pytest.raises(ValueError):
            g.set_transfer("nonsense")
        assert gsv.driver().gs_grid_set_transfer(g.handle, 7) == 1 and b"transfer" in gsv.driver().gs_last_error()
        assert g.transfer == "position"
    assert want_pos[0] != want_ref[0]


CHILD = """
import sys
sys.path[:0] = {paths!r}
import gpusolve as gsv
p = gsv.GridParams(maxiter=2, tol=0.0, gridDim=(12, 10, 8))
with gsv.HipGridData(p) as g:
    print(g.transfer, " ".join(x.hex() for x in gsv.HipSolver.solve(g)), g.field(0, "v").tobytes().hex()[-64:])
"""


def test_environment_switch(monkeypatch):
    hist, (v,) = solve(params((12, 10, 8), cycles=2), "position")
    paths = [os.path.join(REPO, "gpu-solve_amd")]
    env = dict(os.environ, GS_TRANSFER="position")
    out = subprocess.run([sys.executable, "-c", CHILD.format(paths=paths)], capture_output=True, text=True, timeout=120,
                         env=env)
    assert out.returncode == 0, out.stderr
    mode, *rest = out.stdout.split()
    assert mode == "position"
    assert rest[:-1] == [x.hex() for x in hist] and rest[-1] == v.tobytes().hex()[-64:]
    monkeypatch.setenv("GS_TRANSFER", "reference")
    with gsv.HipGridData(params((12, 10, 8))) as g:
        assert g.transfer == "reference"
    monkeypatch.setenv("GS_TRANSFER", "nonsense")
    with pytest.raises(gsv.GpuSolveError, match="GS_TRANSFER=nonsense"):
        gsv.HipGridData(params((12, 10, 8)))


def test_zslab_grid_refuses_position(monkeypatch):
    """A Z-slab grid (the loopback emulation: two ranks on one device) cannot take POSITION mode: its creation fails
    with the reason, before any work, and the caller's buffers are untouched."""
    p = params((70, 33, 41), cycles=1)
    nx, ny, nz = p.gridDim
    v = np.full((nz + 2, ny + 2, nx + 2), np.nan)
    cap = 16
    hist, cnt, ap = (C.c_double * cap)(*([-1.0] * cap)), C.c_int(-1), p.to_abi()
    monkeypatch.setenv("GS_TRANSFER", "position")
    rc = gsv.driver().gs_zslab_loopback_run(C.byref(ap), 2, 1000, 0, 1, hist, cap, C.byref(cnt),
                                            v.ctypes.data_as(gsv._abi.dptr))
    assert rc == 1
    msg = gsv.driver().gs_last_error().decode()
    assert "POSITION" in msg and "Z-slab" in msg, msg
    assert np.isnan(v).all() and cnt.value == -1 and all(x == -1.0 for x in hist)
    monkeypatch.delenv("GS_TRANSFER")
    rc = gsv.driver().gs_zslab_loopback_run(C.byref(ap), 2, 1000, 0, 1, hist, cap, C.byref(cnt),
                                            v.ctypes.data_as(gsv._abi.dptr))
    assert rc == 0 and cnt.value == 2


def test_fmg_keeps_its_alignment_requirement():
    with gsv.HipGridData(params((32, 32, 32))) as g:
        for mode in ("reference", "position"):
            g.set_transfer(mode)
            assert g.fmg_start_level() == 0
            with pytest.raises(gsv.GpuSolveError, match="do not align with the fine grid"):
                gsv.HipSolver.fmg(g, 1)
