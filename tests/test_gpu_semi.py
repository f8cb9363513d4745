"""XY semi-coarsening on the GPU (include/gpusolve_semi.h): the three launchers of
libgpusolve_semi.so against tests/semi_ref.py under the kernel ABI's layout contract, and XY grids through the driver
(gs_grid_create_coarsen, GS_COARSEN, GS_SMOOTHER_AUTO) against semi_ref.Cycle.

Tolerances. Everything here is LINEAR, and the numpy restatement rounds every product, sum and quotient as the kernels
do: fields are compared word for word, on every level. Norms (histories) to 1e-12 relative: the device's fixed-order
sum of squares against the oracle's. The cycle counts of the 63^3 solves come from the model, computed once."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import gpusolve as gsv  # noqa: E402
import oracle as O  # noqa: E402
import pcg_ref as P  # noqa: E402
import semi_ref as S  # noqa: E402
import zline_ref as Z  # noqa: E402
from gpusolve import _abi as A  # noqa: E402
from layout_field import LAYOUT_IDS, POISON_IN, LayoutField, layouts  # noqa: E402

EINVAL = A.GS_EINVAL
SWITCHES = ("GS_COARSEN", "GS_SMOOTHER", "GS_TRANSFER", "GS_OMEGAS", "GS_FMG", "GS_SOLVER", "GS_NO_FUSED_RR",
            "GS_NO_FUSED_SWEEPS", "GS_NO_SPECULATION", "GS_NO_PIPELINE")
# one coarse point; x odd, y even, z-chunks (8 planes) crossed once with a last chunk of one plane; aligned; even x and
# y; nz = 1; a fine row crossing one and two wave boundaries (coarse 64 and 128 columns: one and two full x-tiles);
# a ragged second x-tile (coarse 65) with two y-blocks, the last ragged (coarse 5 rows), and 17 planes (two full
# chunks and one plane). Every launcher has one kernel instance (gs_semi_kernel), so no shape selects another.
SHAPES = [(2, 2, 1), (3, 2, 9), (7, 7, 5), (8, 6, 3), (9, 8, 1), (129, 5, 3), (257, 3, 2), (131, 10, 17)]
LAYOUT_SHAPES = [(3, 2, 9), (8, 6, 3), (131, 10, 17)]
WEAKZ_ABI = gsv.Stencil(list(Z.WEAKZ)).to_abi()


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
    return (shape[0] // 2, shape[1] // 2, shape[2])


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
    """`a` with its ring replaced by finite non-zero noise (no path may read the ring of f or of a restricted field)."""
    rng = np.random.default_rng(a.size)
    out = np.where(rng.random(a.shape) < 0.5, -1.0, 1.0) * rng.uniform(0.5, 50.0, a.shape)
    inner(out)[...] = inner(a)
    return out


class Tables:
    """Device copies of an XY transition's tables and the gs_transfer_tables that describes them."""

    def __init__(self, fine):
        coarse = half(fine)
        self.keep, self.abi = [], gsv.gs_transfer_tables()
        for a in range(2):
            T = gsv.transfer_axis(fine[a])
            self.abi.nf[a], self.abi.nc[a] = fine[a], coarse[a]
            for key in ("pj", "pt", "rlo", "rcnt", "rw"):
                t = torch.from_numpy(np.ascontiguousarray(T[key]).reshape(-1)).cuda()
                self.keep.append(t)
                getattr(self.abi, key)[a] = t.data_ptr()
        self.abi.nf[2] = self.abi.nc[2] = fine[2]


@functools.lru_cache(maxsize=None)
def inputs(shape):
    """Fine v (+-1), f (+-100), coarse c (+-1 with a NON-zero ring: the prolongation takes it as data); read-only."""
    rng = np.random.default_rng(shape[0] + 1000 * shape[1] + 1000003 * shape[2])
    c = rng.uniform(-1.0, 1.0, tuple(n + 2 for n in half(shape)))
    out = [rand_full(rng, shape), rand_full(rng, shape, 100.0), c]
    for a in out:
        a.setflags(write=False)
    return out


def taken(lib):
    buf = C.create_string_buffer(4096)
    lib.gs_semi_launch_record(buf, 4096)
    return buf.value.decode().split()


class Run:
    """The three launchers on one shape in one layout, with every contract check: outputs NaN-poisoned, exactly the
    documented set written, every input unchanged word for word (its poison outside the box included), the kernel
    named by gs_semi_kernel the one the launch record reports."""

    def __init__(self, shape, lid="default"):
        self.shape, self.cshape, self.lid = shape, half(shape), lid
        self.t = gsv.semi()
        self.T = Tables(shape)
        self.hf, self.hc = 1.0 / (shape[1] + 1), 1.0 / (self.cshape[1] + 1)
        self.inputs = []
        taken(self.t)

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

    def done(self, what, op, fl, cl):
        for i, f in enumerate(self.inputs):
            f.assert_unchanged(what=f"{what}: input {i}")
        assert taken(self.t) == [self.t.gs_semi_kernel(op, fl, cl).decode()] != [""], what

    def restrict(self):
        src = self.inp(inputs(self.shape)[0], ring_noise=True)
        o = self.out(self.cshape)
        fl, cl = C.byref(src.level(self.hf)), C.byref(o.level(self.hc))
        assert self.t.gs_restrict_xy(src.ptr, fl, o.ptr, cl, C.byref(self.T.abi), st()) == 0
        o.assert_written_exactly(o.interior_mask(), "gs_restrict_xy")
        self.done("gs_restrict_xy", A.GS_SEMI_RESTRICT, fl, cl)
        return inner(o.to_xyz())

    def prolong(self):
        v, _, c = inputs(self.shape)
        cf = self.inp(c)
        fv = self.fld(self.shape, "out")
        fv.poison_all(POISON_IN).from_xyz(v)
        fv.snapshot()
        cl, fl = C.byref(cf.level(self.hc)), C.byref(fv.level(self.hf))
        assert self.t.gs_prolong_add_xy(cf.ptr, cl, fv.ptr, fl, C.byref(self.T.abi), st()) == 0
        fv.assert_unchanged(~fv.interior_mask(), "gs_prolong_add_xy: outside the fine interior")
        self.done("gs_prolong_add_xy", A.GS_SEMI_PROLONG_ADD, fl, cl)
        return fv.to_xyz()

    def fused(self, stencil=WEAKZ_ABI):
        v, f, _ = inputs(self.shape)
        vf, ff = self.inp(v), self.inp(f, ring_noise=True, role="out")
        o = self.out(self.cshape)
        fl, cl = C.byref(vf.level(self.hf)), C.byref(o.level(self.hc))
        assert self.t.gs_residual_restrict_xy(C.byref(stencil), fl, vf.ptr, ff.ptr, o.ptr, cl, C.byref(self.T.abi),
                                              st()) == 0
        o.assert_written_exactly(o.interior_mask(), "gs_residual_restrict_xy")
        self.done("gs_residual_restrict_xy", A.GS_SEMI_RESIDUAL_RESTRICT, fl, cl)
        return inner(o.to_xyz())

    def two_pass(self, stencil=WEAKZ_ABI):
        """gs_residual with a stored r, then gs_restrict_xy: the composition the fused kernel replaces."""
        v, f, _ = inputs(self.shape)
        vf, ff = self.inp(v), self.inp(f, ring_noise=True, role="out")
        r = self.fld(self.shape, "out")
        r.buf.zero_()
        o = self.out(self.cshape)
        fl, cl = C.byref(vf.level(self.hf)), C.byref(o.level(self.hc))
        assert gsv.kernels().gs_residual(C.byref(stencil), fl, 0, 1.0, vf.ptr, ff.ptr, None, r.ptr, None, st()) == 0
        assert self.t.gs_restrict_xy(r.ptr, C.byref(r.level(self.hf)), o.ptr, cl, C.byref(self.T.abi), st()) == 0
        return inner(o.to_xyz())


def ref_fused(shape, values=Z.WEAKZ, offsets=O.CANONICAL):
    v, f, _ = inputs(shape)
    r, _ = O.residual(v, f, 1.0 / (shape[1] + 1), O.LINEAR, stencil=O.Stencil.make(values, offsets))
    return inner(S.restrict_xy(r, shape))


# ---- kernel level -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_restrict_xy(shape):
    same(Run(shape).restrict(), inner(S.restrict_xy(inputs(shape)[0], shape)), "coarse field")


@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_prolong_add_xy(shape):
    v, _, c = inputs(shape)
    want = v + S.prolong_xy(c, shape)
    same(inner(Run(shape).prolong()), inner(want), "fine interior")


@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_residual_restrict_xy(shape):
    got = Run(shape).fused()
    same(got, ref_fused(shape), "coarse f")
    same(got, Run(shape).two_pass(), "fused against gs_residual + gs_restrict_xy")


def test_residual_restrict_xy_stencils():
    """The unit stencil (the unit-neighbour sum) and a permuted general one take the same kernel."""
    shape = (131, 10, 17)
    same(Run(shape).fused(gsv.Stencil().to_abi()), ref_fused(shape, Z.ISO), "unit stencil")
    values, offsets = Z.permuted(Z.UPLO)
    same(Run(shape).fused(gsv.Stencil(list(values), [tuple(o) for o in offsets]).to_abi()),
         ref_fused(shape, values, offsets), "permuted stencil")


@functools.lru_cache(maxsize=None)
def default_results(shape):
    r = Run(shape)
    return r.restrict(), r.prolong(), r.fused()


@pytest.mark.parametrize("lid", [l for l in LAYOUT_IDS if l != "default"])
@pytest.mark.parametrize("shape", LAYOUT_SHAPES, ids=sid)
def test_layout_contract(shape, lid):
    """Every launcher in every layout: Run makes the contract's checks; the values equal the default-layout call's."""
    want, r = default_results(shape), Run(shape, lid)
    same(r.restrict(), want[0], "gs_restrict_xy")
    same(r.prolong(), want[1], "gs_prolong_add_xy")
    same(r.fused(), want[2], "gs_residual_restrict_xy")


@pytest.mark.parametrize("lid", ["default", "tight_odd"])
def test_einval_writes_nothing(lid):
    shape, t = (8, 6, 3), gsv.semi()
    r = Run(shape, lid)
    v, f, c = inputs(shape)
    fine, ff, coarse = r.inp(v), r.inp(f), r.inp(c)
    fo, co = r.fld(shape, "out").poison_all().snapshot(), r.out(half(shape)).snapshot()
    fl, cl = fine.level(r.hf), coarse.level(r.hc)
    T, other = r.T.abi, Tables((10, 6, 3)).abi
    nullp, withz, nz1 = gsv.gs_transfer_tables(), gsv.gs_transfer_tables(), gsv.gs_transfer_tables()
    for x in (nullp, withz, nz1):
        C.memmove(C.byref(x), C.byref(T), C.sizeof(T))
    nullp.rw[1] = None
    withz.pt[2] = T.pt[0]
    nz1.nc[2] = 1

    def lvl(base, **kw):
        L = gsv.gs_level(base.nx, base.ny, base.nz, base.ldy, base.ldz, base.z0, base.h)
        for k, val in kw.items():
            setattr(L, k, val)
        return L

    cases = [(fl, cl, other), (fl, cl, nullp), (fl, cl, withz), (fl, cl, nz1), (fl, cl, None),
             (lvl(fl, ldy=fl.nx + 1), cl, T), (fl, lvl(cl, ldz=cl.ldy * (cl.ny + 2) - 1), T),
             (fl, lvl(cl, nx=cl.nx + 1, ldy=cl.ldy + 1), T), (fl, lvl(cl, nz=1), T), (lvl(fl, z0=2), cl, T),
             (fl, lvl(cl, nz=-1), T), (None, cl, T)]
    for i, (a, b, tab) in enumerate(cases):
        pa, pb = (C.byref(a) if a is not None else None), C.byref(b)
        pt = C.byref(tab) if tab is not None else None
        assert t.gs_restrict_xy(fine.ptr, pa, co.ptr, pb, pt, st()) == EINVAL, i
        assert t.gs_prolong_add_xy(coarse.ptr, pb, fo.ptr, pa, pt, st()) == EINVAL, i
        assert t.gs_residual_restrict_xy(C.byref(WEAKZ_ABI), pa, fine.ptr, ff.ptr, co.ptr, pb, pt, st()) == EINVAL, i
    ok_f, ok_c, ok_t = C.byref(fl), C.byref(cl), C.byref(T)
    assert t.gs_restrict_xy(None, ok_f, co.ptr, ok_c, ok_t, st()) == EINVAL
    assert t.gs_restrict_xy(fine.ptr, ok_f, None, ok_c, ok_t, st()) == EINVAL
    assert t.gs_prolong_add_xy(None, ok_c, fo.ptr, ok_f, ok_t, st()) == EINVAL
    assert t.gs_prolong_add_xy(coarse.ptr, ok_c, None, ok_f, ok_t, st()) == EINVAL
    assert t.gs_residual_restrict_xy(None, ok_f, fine.ptr, ff.ptr, co.ptr, ok_c, ok_t, st()) == EINVAL
    assert t.gs_residual_restrict_xy(C.byref(WEAKZ_ABI), ok_f, fine.ptr, ff.ptr, None, ok_c, ok_t, st()) == EINVAL
    assert t.gs_residual_restrict_xy(C.byref(WEAKZ_ABI), ok_f, None, ff.ptr, co.ptr, ok_c, ok_t, st()) == EINVAL
    bad = gsv.Stencil([6, -1, -1, -1, -1, -1, -1], [(0, 0, 0), (2, 0, 0)] + list(gsv.CANONICAL_OFFSETS[2:])).to_abi()
    assert t.gs_residual_restrict_xy(C.byref(bad), ok_f, fine.ptr, ff.ptr, co.ptr, ok_c, ok_t, st()) == EINVAL
    fo.assert_unchanged(what="fine output after EINVAL")
    co.assert_unchanged(what="coarse output after EINVAL")
    for i, f in enumerate(r.inputs):
        f.assert_unchanged(what=f"EINVAL: input {i}")
    assert taken(t) == []


# ---- driver -------------------------------------------------------------------------------------------------------
STENCILS = {"WEAKZ": (Z.WEAKZ, list(O.CANONICAL)), "ISO": (Z.ISO, list(O.CANONICAL)),
            "UPLO": (Z.UPLO, list(O.CANONICAL)), "PERM": Z.permuted(Z.UPLO)}


def make_grid(dims, sname="WEAKZ", coarsen="xy", pre=2, post=2, maxiter=3, tol=0.0, f=None, mode=gsv.GS_LINEAR):
    values, offsets = STENCILS[sname]
    stc = gsv.Stencil(list(values), [tuple(o) for o in offsets])
    g = gsv.HipGridData(gsv.GridParams(maxiter=maxiter, tol=tol, gridDim=dims, mode=mode, preSmoothing=pre,
                                       postSmoothing=post, stencil=stc), coarsen=coarsen)
    if f is not None:
        g.set_field(0, "f", f)
    return g


def assert_levels(g, c, what):
    for l in range(len(c.ld)):
        same(g.field(l, "v"), c.v[l], f"{what}: level {l}'s v")
        same(g.field(l, "f"), c.f[l], f"{what}: level {l}'s f")


@pytest.mark.parametrize("smoother", ["jacobi", "zline", "auto"])
@pytest.mark.parametrize("sname", list(STENCILS))
@pytest.mark.parametrize("dims", [(15, 15, 15), (16, 12, 20), (31, 31, 8)], ids=sid)
def test_cycles_against_the_model(dims, sname, smoother):
    """Every level's v and f word for word after one and after three V-cycles, the closing norms to 1e-12; the
    hierarchy, the level stencils and the per-level smoother as the model has them. (PERM with point Jacobi: one
    cycle. The reference's point Jacobi takes entry 0 of the stencil for the diagonal, which in the PERM order is an
    x weight, so that iteration diverges — 1e40 to 1e59 per cycle in the model — and overflows in the third cycle;
    the first cycle's fields are finite and are compared like the others'.)"""
    values, offsets = STENCILS[sname]
    f = Z.normal_rhs(dims, 3)
    c = S.Cycle(dims, values, offsets, smoother=smoother, f0=f)
    with make_grid(dims, sname, f=f) as g:
        assert g.coarsen == "xy" and g.numLevels() == len(c.ld)
        g.set_smoother(smoother)
        assert g.smoother == smoother
        for l, d in enumerate(c.ld):
            assert g.getLevel(l).levelDim == d
            assert g.level_stencil(l).values == list(c.values[l]) and g.level_stencil(l).offsets == [tuple(o) for o in offsets]
            assert g.level_smoother(l) == ("zline" if c.line[l] else "jacobi"), (l, c.pattern())
        for l in range(len(c.ld) - 1):
            assert g.level_aligned(l) == all(c.ld[l][a] == 2 * c.ld[l + 1][a] + 1 for a in (0, 1))
        for k in range(1 if (sname, smoother) == ("PERM", "jacobi") else 3):
            got, want = gsv.HipSolver.vcycle(g), c.vcycle()
            print(f"cycle {k}: device {got!r} model {want!r}")
            assert np.isfinite(want) and abs(got - want) <= 1e-12 * want
            if k in (0, 2):
                assert_levels(g, c, f"{sid(dims)} {sname} {smoother} after cycle {k + 1}")


def test_per_sweep_weights_and_solve_history():
    """solve() (speculative closing norms where level 0 is a point level) with per-sweep weights: the history to
    1e-12, every level word for word."""
    dims, pre, post = (16, 12, 20), (0.9, 0.7), (0.6, 1.0)
    f = Z.normal_rhs(dims, 4)
    for smoother in ("auto", "zline"):
        c = S.Cycle(dims, Z.WEAKZ, smoother=smoother, pre=pre, post=post, f0=f)
        want = c.solve(3)
        with make_grid(dims, f=f) as g:
            g.set_weights(pre, post)
            g.set_smoother(smoother)
            hist = gsv.HipSolver.solve(g)
            print(smoother, hist, want)
            assert len(hist) == len(want) and all(abs(a - b) <= 1e-12 * b for a, b in zip(hist, want))
            assert_levels(g, c, f"weighted solve, {smoother}")


@pytest.mark.parametrize("switch", ["GS_NO_FUSED_RR", "GS_NO_SPECULATION", "GS_NO_FUSED_SWEEPS", "GS_NO_ZERO_GUESS"])
def test_alternative_paths_give_the_same_bits(switch, monkeypatch):
    """The driver's alternative paths on an XY grid — the residual stored and restricted by gs_restrict_xy, the closing
    norm from a residual pass, single sweeps, the coarse zero stored — give the default XY path's bits."""
    dims = (31, 31, 8)
    f = Z.normal_rhs(dims, 6)

    def run():
        with make_grid(dims, f=f) as g:
            g.set_smoother("auto")
            return gsv.HipSolver.solve(g), [g.field(l, "v").copy() for l in range(g.numLevels())]

    want = run()
    monkeypatch.setenv(switch, "1")
    got = run()
    # (the norms: other kernels' partial sums, so to 1e-12; the fields word for word)
    assert len(got[0]) == len(want[0]) and all(abs(a - b) <= 1e-12 * b for a, b in zip(got[0], want[0]))
    for l, (a, b) in enumerate(zip(got[1], want[1])):
        same(a, b, f"{switch}: level {l}'s v")


def test_vcycle_level_jacobi_and_residual_norm():
    """gs_grid_vcycle_level rooted at level 1, stand-alone sweeps and the residual norm take the level's own stencil."""
    dims = (15, 15, 15)
    ld = S.level_dims(dims)
    whole = S.Cycle(dims, Z.WEAKZ, smoother="auto")
    f1, v1 = Z.normal_rhs(ld[1], 4), Z.normal_rhs(ld[1], 5) * 1e-3
    # level 1 of the 15^3 hierarchy as the root of a model of its own: its stencil list starts at level 1's
    c = S.Cycle(dims, Z.WEAKZ, smoother="auto")
    c.v[1], c.f[1] = v1.copy(), f1.copy()
    c.vcycle_from(1)
    with make_grid(dims) as g:
        g.set_smoother("auto")
        f0, v0 = g.field(0, "f").copy(), g.field(0, "v").copy()
        g.set_field(1, "f", f1)
        g.set_field(1, "v", v1)
        gsv.HipSolver.vcycle_from(g, 1)
        for l in range(1, len(ld)):
            same(g.field(l, "v"), c.v[l], f"level {l}'s v after a cycle rooted at level 1")
        same(g.field(0, "f"), f0, "level 0's f")
        same(g.field(0, "v"), v0, "level 0's v")
        r, want = gsv.HipSolver.compResidual(g, 1), c.residual(1)[1]
        assert abs(r - want) <= 1e-12 * want
        gsv.HipSolver.jacobi(g, 1, 3)
        v = c.v[1]
        for _ in range(3):
            v = O.jacobi(v, c.f[1], c.h[1], mode=O.LINEAR, omega=0.8, sweeps=1, stencil=whole.stencils[1])
        assert not whole.line[1]
        same(g.field(1, "v"), v, "level 1's v after three stand-alone sweeps")


@functools.lru_cache(maxsize=None)
def rhs63():
    f = Z.normal_rhs((63, 63, 63), 1)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def model63_cycles():
    return S.cycles_to(S.Cycle((63, 63, 63), Z.WEAKZ, smoother="auto", f0=rhs63()), 1e8)


def test_convergence_on_the_device():
    """63^3 WEAKZ: solve(tol 1e-8) with XY + auto stops within the model's cycle count + 1."""
    dims, n = (63, 63, 63), model63_cycles()
    with make_grid(dims, maxiter=n + 4, tol=1e-8, f=rhs63()) as g:
        g.set_smoother("auto")
        assert " ".join("Z" if g.level_smoother(l) == "zline" else "J" for l in range(g.numLevels())) == "J J J Z Z Z"
        hist = gsv.HipSolver.solve(g)
    print("model cycles", n, "device:", " ".join(f"{x:.3e}" for x in hist))
    assert len(hist) - 1 <= n + 1 and hist[-1] <= 1e-8 * hist[0]


class SemiPcg(P.Pcg):
    def M(self, r):
        c = S.Cycle(self.dims, Z.WEAKZ, smoother="auto", f0=r)
        c.vcycle_from(0)
        return c.v[0]


def test_pcg_on_an_xy_grid():
    """PCG preconditioned by the XY + auto cycle at 63^3: supported (an XY transition is by position), converges, and
    the CPU model fed the device's own alpha and beta gives the same iterate bit for bit."""
    dims = (63, 63, 63)
    with make_grid(dims, maxiter=6, tol=0.0, f=rhs63()) as g:
        g.set_smoother("auto")
        assert g.pcg_supported(), g.pcg_refusal
        hist = gsv.HipSolver.pcg(g)
        rec = g.pcg_record()
        x = g.field(0, "v")
        assert not g.pcg_breakdown and len(rec) == 6
        same(g.field(0, "f"), rhs63(), "f after PCG")
    m = SemiPcg(dims, rhs63(), stencil=O.Stencil.make(Z.WEAKZ))
    want, _ = m.replay([(r["alpha"], r["beta"]) for r in rec])
    print("device", hist, "replay", want)
    same(x, m.x, "x against the replayed model")
    assert all(abs(a - b) <= 1e-9 * b for a, b in zip(hist, want))
    # the stationary cycle gains at most 0.21 per cycle in the model (tests/test_semi_cpu.py): 0.21^6 < 1e-4; one
    # decade on top, as CG minimises the energy norm of the error and not the residual norm printed here
    assert hist[-1] <= 1e-3 * hist[0]


def launches(fn):
    """The kernel names one call enqueues in the two libraries the default path uses (each record's latest 16)."""
    k, t = gsv.kernels(), gsv.transfer()
    buf = C.create_string_buffer(1 << 16)
    k.gs_launch_record(buf, 1 << 16)
    t.gs_transfer_launch_record(buf, 1 << 16)
    fn()
    k.gs_launch_record(buf, 1 << 16)
    a = buf.value.decode()
    t.gs_transfer_launch_record(buf, 1 << 16)
    return a, buf.value.decode()


@pytest.mark.parametrize("mode", [gsv.GS_LINEAR, gsv.GS_NONLINEAR, gsv.GS_NEWTON])
def test_xyz_is_the_default_grid(mode):
    """gs_grid_create_coarsen(GS_COARSEN_XYZ), GS_COARSEN=xyz and a grid created after an XY grid was destroyed give a
    fresh default grid's bits (31^3, two cycles) and launch the same kernels in a V-cycle."""
    p = gsv.GridParams(maxiter=2, tol=0.0, gridDim=(31, 31, 31), mode=mode)
    name = "newtonV" if mode == gsv.GS_NEWTON else "v"

    def run(make):
        with make() as g:
            assert g.coarsen == "xyz" and g.level_stencil(2).values == [6.0, -1, -1, -1, -1, -1, -1]
            hist = gsv.HipSolver.solve(g)
            out = g.field(0, name).copy()
            rec = launches(lambda: gsv.HipSolver.vcycle(g)) if mode == gsv.GS_LINEAR else None
            return hist, out, rec

    want = run(lambda: gsv.HipGridData(p))
    with make_grid((16, 12, 20)) as g:
        gsv.HipSolver.vcycle(g)
    for what, make in (("coarsen=xyz", lambda: gsv.HipGridData(p, coarsen="xyz")), ("after an XY grid", lambda: gsv.HipGridData(p))):
        got = run(make)
        assert got[0] == want[0], what
        same(got[1], want[1], what)
        assert got[2] == want[2], what
    if mode == gsv.GS_LINEAR:
        assert "k_" in want[2][0]


def test_auto_on_an_xyz_grid_is_all_or_nothing():
    for sname, line in (("WEAKZ", False), ("ISO", False)):
        with make_grid((15, 15, 15), sname, coarsen="xyz") as g:
            g.set_smoother("auto")
            assert all(g.level_smoother(l) == ("zline" if line else "jacobi") for l in range(g.numLevels()))
    dims = (15, 15, 15)
    f = Z.normal_rhs(dims, 5)
    p = gsv.GridParams(maxiter=2, tol=0.0, gridDim=dims, stencil=gsv.Stencil(list(Z.STRONGZ)))
    with gsv.HipGridData(p) as g:
        g.set_field(0, "f", f)
        g.set_smoother("zline")
        want = gsv.HipSolver.solve(g), g.field(0, "v").copy()
    with gsv.HipGridData(p) as g:
        g.set_field(0, "f", f)
        g.set_smoother("auto")
        assert all(g.level_smoother(l) == "zline" for l in range(g.numLevels()))
        assert gsv.HipSolver.solve(g) == want[0]
        same(g.field(0, "v"), want[1], "AUTO on a strong-z XYZ grid is ZLINE")


def test_environment_switches(monkeypatch):
    p = gsv.GridParams(maxiter=2, tol=0.0, gridDim=(16, 12, 20), stencil=gsv.Stencil(list(Z.WEAKZ)))
    monkeypatch.setenv("GS_COARSEN", "xy")
    monkeypatch.setenv("GS_SMOOTHER", "auto")
    with gsv.HipGridData(p) as g:
        assert g.coarsen == "xy" and g.smoother == "auto" and g.numLevels() == 4
        got = gsv.HipSolver.solve(g), g.field(0, "v").copy()
    with gsv.HipGridData(p, coarsen="xyz") as g:   # the call does not read GS_COARSEN
        assert g.coarsen == "xyz"
    monkeypatch.delenv("GS_COARSEN")
    monkeypatch.delenv("GS_SMOOTHER")
    with gsv.HipGridData(p, coarsen="xy") as g:
        g.set_smoother("auto")
        assert gsv.HipSolver.solve(g) == got[0]
        same(g.field(0, "v"), got[1], "GS_COARSEN=xy GS_SMOOTHER=auto against the calls")
    monkeypatch.setenv("GS_COARSEN", "nonsense")
    with pytest.raises(gsv.GpuSolveError, match="GS_COARSEN=nonsense"):
        gsv.HipGridData(p)


def test_refusals(monkeypatch):
    for mode in (gsv.GS_NONLINEAR, gsv.GS_NEWTON):
        with pytest.raises(gsv.GpuSolveError, match="XY needs a LINEAR grid"):
            make_grid((15, 15, 15), "ISO", mode=mode)
    diag = list(O.CANONICAL)
    diag[1] = (1, 1, 0)
    p = gsv.GridParams(maxiter=1, tol=0.0, gridDim=(15, 15, 15), stencil=gsv.Stencil(list(Z.ISO), diag))
    with pytest.raises(gsv.GpuSolveError, match="XY needs a stencil of the seven axis offsets"):
        gsv.HipGridData(p, coarsen="xy")
    with pytest.raises(gsv.GpuSolveError, match="at least 2 points in x and in y"):
        make_grid((1, 15, 15))
    ap = gsv.GridParams(maxiter=1, tol=0.0, gridDim=(15, 15, 15)).to_abi()
    assert not gsv.driver().gs_grid_create_coarsen(C.byref(ap), 2) and b"coarsen" in gsv.driver().gs_last_error()
    # FMG on an XY grid: refused with its reason, nothing changed
    with make_grid((15, 15, 15)) as g:
        before = [g.field(l, "v").copy() for l in range(g.numLevels())]
        assert g.fmg_start_level() == 0
        with pytest.raises(gsv.GpuSolveError, match="FMG: not on an XY semi-coarsened grid"):
            gsv.HipSolver.fmg(g, 1)
        for l, b in enumerate(before):
            same(g.field(l, "v"), b, f"level {l}'s v after the refused FMG")
        # a smoother whose line levels have a stencil the line sweep refuses: nothing changed
        assert gsv.driver().gs_grid_set_smoother(g.handle, 7) == 1 and b"smoother" in gsv.driver().gs_last_error()
        assert g.smoother == "jacobi"
    weak = gsv.GridParams(maxiter=1, tol=0.0, gridDim=(15, 15, 15),
                          stencil=gsv.Stencil([1.9, -0.05, -0.05, -0.05, -0.05, -1.0, -1.0]))
    with gsv.HipGridData(weak) as g:
        with pytest.raises(gsv.GpuSolveError, match="AUTO needs a stencil"):
            g.set_smoother("auto")
        assert g.smoother == "jacobi" and g.level_smoother(0) == "jacobi"
    # a Z-slab grid (the loopback emulation: two ranks on one device): its creation under GS_COARSEN=xy fails with the
    # reason before any work, and the caller's buffers are untouched
    p = gsv.GridParams(maxiter=1, tol=0.0, gridDim=(70, 33, 41))
    nx, ny, nz = p.gridDim
    v = np.full((nz + 2, ny + 2, nx + 2), np.nan)
    cap = 16
    hist, cnt, ap = (C.c_double * cap)(*([-1.0] * cap)), C.c_int(-1), p.to_abi()
    monkeypatch.setenv("GS_COARSEN", "xy")
    rc = gsv.driver().gs_zslab_loopback_run(C.byref(ap), 2, 1000, 0, 1, hist, cap, C.byref(cnt), v.ctypes.data_as(A.dptr))
    assert rc == 1
    msg = gsv.driver().gs_last_error().decode()
    assert "XY needs a single-GPU grid" in msg and "Z-slab" in msg, msg
    assert np.isnan(v).all() and cnt.value == -1 and all(x == -1.0 for x in hist)
