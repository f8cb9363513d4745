"""The z-line smoother on the GPU (include/gpusolve_line.h): gs_zline_sweep through the C ABI against
tests/zline_ref.py in the layout harness of tests/layout_field.py, and ZLINE mode through the driver
(gs_grid_set_smoother, GS_SMOOTHER) against the V-cycle composed of zline_ref's sweep and the CPU oracle's transfers.

Tolerances. Everything is LINEAR arithmetic: the launcher's output and every level-0 field of the driver agree with the
model bit for bit (the numpy restatement rounds every product, sum and quotient as the kernels do); norms to 1e-12
(the device's fixed-order sum against the oracle's). Convergence at 63^3 to 1e-8: the model needs 8 cycles and 6 PCG
iterations; the device gets 10 and 8 — the spare ones cover a stop decision that falls on the
threshold.

Shapes of the launcher test: one point, one pair of planes, a 4093-plane column, odd sizes, several blocks of the
one-column kernel (33 x 5 x 9), and for the marching instance (canonical order, >= 32 * 32 columns): the smallest
shape that selects it (32 x 32 x 1), one below it (33 x 31: the one-column kernel), an x-tile plus one column with a
half-valid last lane pair and a last y-block of one row (129 x 129), a last y-block of three rows behind a full pair
in the second tile (130 x 127), two full x-tiles (256 x 65), and nz = ring depth - 1, the ring depth and + 1 (7, 8,
9)."""
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
import pcg_ref as P  # noqa: E402
import zline_ref as Z  # noqa: E402
from conftest import REPO  # noqa: E402
from fmg_ref import level_dims, prolong, start_level  # noqa: E402
from gpusolve import _abi as A  # noqa: E402
from layout_field import LAYOUT_IDS, POISON_OUT, LayoutField, layouts  # noqa: E402

EINVAL = A.GS_EINVAL
RING = 8  # ZL_R of csrc/gs_line_device.hpp
SHAPES = [(1, 1, 1), (1, 1, 2), (1, 1, 4093), (5, 1, 3), (2, 3, 1), (33, 5, 9),
          (32, 32, 1), (33, 31, 2), (129, 129, RING - 1), (130, 127, RING + 1), (256, 65, RING)]
STENCILS = {
    "strongz": (Z.STRONGZ, list(O.CANONICAL)),
    "iso": (Z.ISO, list(O.CANONICAL)),
    "uplo": (Z.UPLO, list(O.CANONICAL)),
    "permuted": Z.permuted(Z.UPLO),
}
LN = None


def ln():
    global LN
    if LN is None:
        assert torch.cuda.is_available(), "GPU tests need a GPU (no CPU fallback exists)"
        LN = gsv.line()
    return LN


def st():
    return torch.cuda.current_stream().cuda_stream


def sid(shape):
    return "x".join(str(n) for n in shape)


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def same(a, b, what):
    ne = bits(a) != bits(b)
    assert not ne.any(), f"{what}: {int(ne.sum())} words differ, first at {tuple(np.argwhere(ne)[0])}"


def abi(values, offsets):
    return gsv.Stencil(list(values), [tuple(o) for o in offsets]).to_abi()


class Tables:
    """A level's factors on the device (gs_zline_factors' own output), each between poisoned guards."""

    def __init__(self, S, nz):
        cp, den = np.zeros(nz + 2), np.zeros(nz + 2)
        assert ln().gs_zline_factors(C.byref(S), nz, cp.ctypes.data_as(A.dptr), den.ctypes.data_as(A.dptr)) == 0
        self.t = torch.zeros(2 * (nz + 2) + 24, dtype=torch.float64, device="cuda")
        self.t.view(torch.int64).fill_(POISON_OUT)
        self.t[8:8 + nz + 2] = torch.from_numpy(cp).cuda()
        self.t[16 + nz + 2:16 + 2 * (nz + 2)] = torch.from_numpy(den).cuda()
        base = self.t.data_ptr()
        self.abi = A.gs_zline_tables(base + 64, base + 8 * (16 + nz + 2), nz)


@functools.lru_cache(maxsize=None)
def host_inputs(shape):
    """(v, f) on the host, shared by every layout: v's ring zero, f's ring noise."""
    n = shape[0] * shape[1] * shape[2]
    rng = np.random.default_rng(17 + n)
    va, fa = O.zeros(*shape), rng.standard_normal(tuple(s + 2 for s in shape)) * 100.0  # (ring included: noise)
    P.inner(va)[...] = rng.standard_normal(shape)
    return va, fa


@functools.lru_cache(maxsize=None)
def wanted(shape, sname, omega, zero):
    """The model's sweep, computed once per case and left unchanged."""
    va, fa = host_inputs(shape)
    values, offsets = STENCILS[sname]
    out = Z.sweep(None if zero else va, fa, 1.0 / (shape[1] + 1), omega, values, offsets)
    out.setflags(write=False)
    return out


def inputs(shape, lay):
    """(v, f) in the layout, NaN outside both boxes."""
    va, fa = host_inputs(shape)
    v = LayoutField(*shape, lay.ldy, lay.ldz, lay.phase_in).from_xyz(va).poison_outside_box().snapshot()
    f = LayoutField(*shape, lay.ldy, lay.ldz, lay.phase_out).from_xyz(fa).poison_outside_box().snapshot()
    return va, fa, v, f


def expected_kernel(shape, sname, zero):
    march = STENCILS[sname][1] == list(O.CANONICAL) and shape[0] * shape[1] >= 32 * 32
    return f"k_zline_{'march' if march else 'col'}<{'true' if zero else 'false'}>"


@pytest.mark.parametrize("lid", LAYOUT_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_sweep_bit_for_bit(shape, lid):
    lay = layouts(*shape)[lid]
    h = 1.0 / (shape[1] + 1)
    va, fa, v, f = inputs(shape, lay)
    L = v.level(h)
    out = LayoutField(*shape, lay.ldy, lay.ldz, lay.phase_out)
    interior = out.interior_mask()
    for sname, (values, offsets) in STENCILS.items():
        S = abi(values, offsets)
        T = Tables(S, shape[2])
        for omega in (1.0, 0.8):
            for zero in (False, True):
                what = f"gs_zline_sweep {sid(shape)} {lid} {sname} omega={omega} zero={zero}"
                assert ln().gs_zline_kernel(C.byref(S), C.byref(L), int(zero)).decode() == \
                    expected_kernel(shape, sname, zero), what
                out.poison_all()
                rc = ln().gs_zline_sweep(C.byref(S), C.byref(L), omega, None if zero else v.ptr, out.ptr, f.ptr,
                                         C.byref(T.abi), st())
                assert rc == 0, what
                out.assert_written_exactly(interior, what + " v_out")
                v.assert_unchanged(what=what + " v_in")
                f.assert_unchanged(what=what + " f")
                same(P.inner(out.to_xyz()), P.inner(wanted(shape, sname, omega, zero)), what)


def test_zero_iterate_equals_a_zeroed_field():
    shape = (129, 129, 5)
    lay = layouts(*shape)["default"]
    _, _, _, f = inputs(shape, lay)
    zf = LayoutField(*shape, lay.ldy, lay.ldz, lay.phase_in)  # (zero-filled)
    L = zf.level(1.0 / 130)
    for sname in ("strongz", "permuted"):
        S = abi(*STENCILS[sname])
        T = Tables(S, shape[2])
        got = []
        for vin in (None, zf.ptr):
            out = LayoutField(*shape, lay.ldy, lay.ldz, lay.phase_out).poison_all()
            assert ln().gs_zline_sweep(C.byref(S), C.byref(L), 0.8, vin, out.ptr, f.ptr, C.byref(T.abi), st()) == 0
            got.append(P.inner(out.to_xyz()))
        assert np.array_equal(got[0], got[1]), sname  # (==: the sign of a zero may differ, gpusolve_line.h)


@pytest.mark.parametrize("shape", [(33, 5, 9), (129, 129, 5)], ids=sid)
def test_refused_calls_write_nothing(shape):
    lay = layouts(*shape)["default"]
    _, _, v, f = inputs(shape, lay)
    L = v.level(1.0 / (shape[1] + 1))
    S = abi(*STENCILS["strongz"])
    T, Tother = Tables(S, shape[2]), Tables(S, shape[2] + 1)
    out = LayoutField(*shape, lay.ldy, lay.ldz, lay.phase_out).poison_all()
    shifted = v.level(1.0 / (shape[1] + 1), z0=1)
    weak = abi((1.9, -0.05, -0.05, -0.05, -0.05, -1.0, -1.0), O.CANONICAL)
    diag = list(O.CANONICAL)
    diag[1] = (1, 1, 0)
    nulls = A.gs_zline_tables(None, T.abi.den, shape[2])
    call = lambda S_, L_, vin, vout, ff, T_: ln().gs_zline_sweep(C.byref(S_), C.byref(L_), 0.8, vin, vout, ff,
                                                                 C.byref(T_), st())
    cases = {"v_in == v_out": (S, L, v.ptr, v.ptr, f.ptr, T.abi), "f == v_out": (S, L, v.ptr, f.ptr, f.ptr, T.abi),
             "v_out inside v_in's box": (S, L, v.ptr, v.ptr + 8 * L.ldz, f.ptr, T.abi),
             "tables of another nz": (S, L, v.ptr, out.ptr, f.ptr, Tother.abi),
             "a null table": (S, L, v.ptr, out.ptr, f.ptr, nulls), "z0 != 0": (S, shifted, v.ptr, out.ptr, f.ptr, T.abi),
             "|s0| < |up| + |lo|": (weak, L, v.ptr, out.ptr, f.ptr, T.abi),
             "a diagonal offset": (abi(Z.STRONGZ, diag), L, v.ptr, out.ptr, f.ptr, T.abi),
             "v_out == NULL": (S, L, v.ptr, None, f.ptr, T.abi), "f == NULL": (S, L, v.ptr, out.ptr, None, T.abi)}
    for what, args in cases.items():
        assert call(*args) == EINVAL, what
    torch.cuda.synchronize()
    v.assert_unchanged(what="refused calls, v_in")
    f.assert_unchanged(what="refused calls, f")
    assert bool((out.i64 == POISON_OUT).all())
    assert ln().gs_zline_sweep(C.byref(S), C.byref(L), 0.8, v.ptr, out.ptr, f.ptr, None, st()) == EINVAL
    empty = LayoutField(0, 5, shape[2], 16, 16 * 7, 0)
    assert ln().gs_zline_sweep(C.byref(S), C.byref(empty.level(0.1)), 0.8, None, out.ptr, f.ptr, C.byref(T.abi), st()) == 0
    torch.cuda.synchronize()
    assert bool((out.i64 == POISON_OUT).all())


# ---- the driver ---------------------------------------------------------------------------------------------------
def make_grid(dims, values=Z.STRONGZ, pre=2, post=2, maxiter=3, tol=0.0, f=None, mode=gsv.GS_LINEAR, offsets=None):
    stc = gsv.Stencil(list(values)) if offsets is None else gsv.Stencil(list(values), [tuple(o) for o in offsets])
    g = gsv.HipGridData(gsv.GridParams(maxiter=maxiter, tol=tol, gridDim=dims, mode=mode, preSmoothing=pre,
                                       postSmoothing=post, stencil=stc))
    if f is not None:
        g.set_field(0, "f", f)
    return g


# id: (dims, pre weights, post weights, explicit weights?, transfer)
DRIVER_CASES = {
    "31-2+2": ((31, 31, 31), (0.8, 0.8), (0.8, 0.8), False, "reference"),
    "31-1+3": ((31, 31, 31), (0.8,), (0.8,) * 3, False, "reference"),
    "24x31x15-2+2": ((24, 31, 15), (0.8, 0.8), (0.8, 0.8), False, "reference"),
    "24x31x15-1+3": ((24, 31, 15), (0.8,), (0.8,) * 3, False, "reference"),
    "31-weights": ((31, 31, 31), (0.9, 0.7), (0.6, 1.0), True, "reference"),
    "24-position": ((24, 24, 24), (0.8, 0.8), (0.8, 0.8), False, "position"),
}


@pytest.mark.parametrize("cid", list(DRIVER_CASES))
def test_driver_cycles_against_the_model(cid):
    dims, pre, post, explicit, transfer = DRIVER_CASES[cid]
    f = Z.normal_rhs(dims, 3)
    cls = Z.ZCyclePa if transfer == "position" else Z.ZCycle
    c = cls(dims, Z.STRONGZ, pre=pre, post=post, f0=f)
    with make_grid(dims, pre=len(pre), post=len(post), f=f) as g:
        if transfer == "position":
            g.set_transfer("position")
        if explicit:
            g.set_weights(pre, post)
        g.set_smoother("zline")
        assert g.smoother == "zline"
        for k in range(2):
            got, want = gsv.HipSolver.vcycle(g), c.vcycle()
            print(f"{cid} cycle {k}: device {got!r} model {want!r} rel {abs(got - want) / want:.3e}")
            same(g.field(0, "v"), c.v[0], f"{cid}: level 0's v after cycle {k}")
            assert abs(got - want) <= 1e-12 * want
        same(g.field(0, "f"), f, f"{cid}: level 0's f")
        # stand-alone sweeps (gs_grid_jacobi) are line sweeps too, with the grid's omega
        gsv.HipSolver.jacobi(g, 0, 3)
        v = c.v[0]
        for _ in range(3):
            v = Z.sweep(v, f, c.h[0], 0.8, Z.STRONGZ)
        same(g.field(0, "v"), v, f"{cid}: v after three stand-alone sweeps")


def test_vcycle_level_from_level_one():
    dims = (31, 31, 31)
    ld = level_dims(dims)
    f1, v1 = Z.normal_rhs(ld[1], 4), Z.normal_rhs(ld[1], 5) * 1e-3
    c = Z.ZCycle(ld[1], Z.STRONGZ, f0=f1, v0=v1)
    c.vcycle_from(0)
    with make_grid(dims) as g:
        g.set_smoother("zline")
        f0, v0 = g.field(0, "f").copy(), g.field(0, "v").copy()
        g.set_field(1, "f", f1)
        g.set_field(1, "v", v1)
        gsv.HipSolver.vcycle_from(g, 1)
        same(g.field(1, "v"), c.v[0], "level 1's v after a cycle rooted there")
        same(g.field(0, "f"), f0, "level 0's f")
        same(g.field(0, "v"), v0, "level 0's v")


def test_fmg_follows_the_smoother():
    dims = (31, 31, 31)
    ld, s = level_dims(dims), start_level(dims)
    f = [Z.normal_rhs(dims, 6)]
    for l in range(s):
        f.append(O.restrict(f[l], ld[l + 1]))
    v = res = None
    for l in range(s, -1, -1):
        v0 = O.zeros(*ld[l])
        if v is not None:
            P.inner(v0)[...] = P.inner(prolong(v))
        c = Z.ZCycle(ld[l], Z.STRONGZ, f0=f[l], v0=v0)
        res = c.vcycle()
        v = c.v[0]
    with make_grid(dims, f=f[0]) as g:
        g.set_smoother("zline")
        got = gsv.HipSolver.fmg(g, 1)
        same(g.field(0, "v"), v, "v after FMG(1) with z-line cycles")
        assert abs(got - res) <= 1e-12 * res


@functools.lru_cache(maxsize=None)
def rhs63():
    return Z.normal_rhs((63, 63, 63), 1)


def test_convergence_on_the_device():
    """63^3 STRONGZ, f from the model's seed: solve(tol 1e-8, maxiter 12) stops within 10 cycles under ZLINE (model:
    8) and not at all under JACOBI; PCG on the z-line cycle stops within 8 iterations (model: 6)."""
    dims = (63, 63, 63)
    with make_grid(dims, maxiter=12, tol=1e-8, f=rhs63()) as g:
        jac = gsv.HipSolver.solve(g)
        g.set_field(0, "v", O.zeros(*dims))
        g.set_smoother("zline")
        zl = gsv.HipSolver.solve(g)
        g.set_field(0, "v", O.zeros(*dims))
        assert g.pcg_supported(), g.pcg_refusal
        pc = gsv.HipSolver.pcg(g)
    print("JACOBI:", " ".join(f"{x:.3e}" for x in jac))
    print("ZLINE: ", " ".join(f"{x:.3e}" for x in zl))
    print("ZLINE PCG:", " ".join(f"{x:.3e}" for x in pc))
    assert len(jac) == 13 and jac[-1] > 1e-8 * jac[0]
    assert len(zl) - 1 <= 10 and zl[-1] <= 1e-8 * zl[0]
    assert len(pc) - 1 <= 8 and pc[-1] <= 1e-8 * pc[0] and not g.pcg_breakdown
    assert abs(zl[0] - jac[0]) <= 1e-12 * jac[0]


def test_switching_back_restores_the_default_path():
    """ZLINE on, a cycle, and off again: a following default solve is a fresh grid's, bit for bit (63^3 with the unit
    stencil: tiled steps, the coarse-cycle launch, the speculative norm all run again)."""
    dims = (63, 63, 63)
    f = Z.normal_rhs(dims, 2)
    with make_grid(dims, values=Z.ISO, f=f) as g:
        want = gsv.HipSolver.solve(g)
        want_v = g.field(0, "v").copy()
    with make_grid(dims, values=Z.ISO, f=f) as g:
        g.set_smoother("zline")
        gsv.HipSolver.vcycle(g)
        g.set_smoother("zline")  # (again: nothing rebuilt, nothing changed)
        z2 = gsv.HipSolver.vcycle(g)
        g.set_smoother("jacobi")
        assert g.smoother == "jacobi"
        g.set_field(0, "v", O.zeros(*dims))
        assert gsv.HipSolver.solve(g) == want
        same(g.field(0, "v"), want_v, "v of the default solve after ZLINE was on and off")
    assert z2 != want[2]


CHILD = """
import sys
sys.path[:0] = {paths!r}
import numpy as np
import gpusolve as gsv
p = gsv.GridParams(maxiter=2, tol=0.0, gridDim=(15, 14, 9), stencil=gsv.Stencil({values!r}))
with gsv.HipGridData(p) as g:
    print(g.smoother, " ".join(x.hex() for x in gsv.HipSolver.solve(g)), g.field(0, "v").tobytes().hex()[-64:])
"""


def test_environment_switch(monkeypatch):
    p = gsv.GridParams(maxiter=2, tol=0.0, gridDim=(15, 14, 9), stencil=gsv.Stencil(list(Z.STRONGZ)))
    with gsv.HipGridData(p) as g:
        g.set_smoother("zline")
        hist, v = gsv.HipSolver.solve(g), g.field(0, "v").copy()
    with gsv.HipGridData(p) as g:
        plain = gsv.HipSolver.solve(g)
    assert plain != hist
    paths = [os.path.join(REPO, "gpu-solve_amd")]
    code = CHILD.format(paths=paths, values=list(Z.STRONGZ))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, GS_SMOOTHER="zline"))
    assert out.returncode == 0, out.stderr
    mode, *rest = out.stdout.split()
    assert mode == "zline"
    assert rest[:-1] == [x.hex() for x in hist] and rest[-1] == v.tobytes().hex()[-64:]
    monkeypatch.setenv("GS_SMOOTHER", "jacobi")
    with gsv.HipGridData(p) as g:
        assert g.smoother == "jacobi" and gsv.HipSolver.solve(g) == plain
    monkeypatch.setenv("GS_SMOOTHER", "nonsense")
    with pytest.raises(gsv.GpuSolveError, match="GS_SMOOTHER=nonsense"):
        gsv.HipGridData(p)
    monkeypatch.setenv("GS_SMOOTHER", "zline")
    with pytest.raises(gsv.GpuSolveError, match="ZLINE needs a LINEAR grid"):
        gsv.HipGridData(gsv.GridParams(maxiter=1, gridDim=(15, 15, 15), mode=gsv.GS_NONLINEAR))


def test_executable_follows_the_variable(tmp_path):
    """GpuSolve-hip under GS_SMOOTHER=zline prints the library's z-line history in the reference's line format; on a
    grid that cannot take the mode it prints the reason as its Exception line and no solve line."""
    import re
    iter_line = re.compile(r"iter: (\d+) residual: (\S+) Took (\d+)ms")  # (tools/run_experiments.py's ITER)
    params = gsv.GridParams(maxiter=4, tol=0.0, gridDim=(31, 31, 31), stencil=gsv.Stencil(list(Z.STRONGZ)))
    conf = tmp_path / "zline.conf"
    conf.write_text(params.config_text())
    with gsv.HipGridData(params) as g:
        g.set_smoother("zline")
        api = gsv.HipSolver.solve(g)
    exe = gsv._abi.EXECUTABLE
    out = subprocess.run([exe, str(conf)], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, GS_SMOOTHER="zline"))
    assert out.returncode == 0 and out.stderr == "", out.stderr
    lines = out.stdout.splitlines()
    assert lines[2] == f"Inital residual: {api[0]:.6g}"
    got = [iter_line.search(l) for l in lines[3:]]
    assert len(got) == 4 and all(got), out.stdout
    for m, want in zip(got, api[1:]):
        assert abs(float(m.group(2)) - want) <= 1e-5 * want, (m.group(0), want)
    plain = subprocess.run([exe, str(conf)], capture_output=True, text=True, timeout=120,
                           env=dict(os.environ, GS_SMOOTHER="jacobi"))
    assert plain.stdout.splitlines()[2] == lines[2] and plain.stdout.splitlines()[3] != lines[3]
    bad = tmp_path / "nonlinear.conf"
    bad.write_text(gsv.GridParams(maxiter=2, gridDim=(15, 15, 15), mode=gsv.GS_NONLINEAR).config_text())
    ref = subprocess.run([exe, str(bad)], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, GS_SMOOTHER="zline"))
    assert "Exception: smoother: ZLINE needs a LINEAR grid" in ref.stderr and not iter_line.search(ref.stdout)


def test_refusals(monkeypatch):
    def refused(g, reason):
        before = g.field(0, "v").copy()
        with pytest.raises(gsv.GpuSolveError, match=reason):
            g.set_smoother("zline")
        assert g.smoother == "jacobi"
        assert gsv.driver().gs_grid_set_smoother(g.handle, A.GS_SMOOTHER_ZLINE) == 1
        assert reason.encode() in gsv.driver().gs_last_error()
        assert gsv.driver().gs_grid_get_smoother(g.handle) == A.GS_SMOOTHER_JACOBI
        same(g.field(0, "v"), before, "v after a refused call")

    for mode in (gsv.GS_NONLINEAR, gsv.GS_NEWTON):
        with make_grid((15, 15, 15), values=Z.ISO, mode=mode) as g:
            refused(g, "ZLINE needs a LINEAR grid")
    with make_grid((15, 15, 15), values=(1.9, -0.05, -0.05, -0.05, -0.05, -1.0, -1.0)) as g:
        refused(g, "ZLINE needs a stencil")
    diag = list(O.CANONICAL)
    diag[1] = (1, 1, 0)
    with make_grid((15, 15, 15), offsets=diag) as g:
        refused(g, "ZLINE needs a stencil")
    with make_grid((15, 15, 15)) as g:
        with pytest.raises(ValueError):
            g.set_smoother("lines")
        assert gsv.driver().gs_grid_set_smoother(g.handle, 7) == 1 and b"smoother" in gsv.driver().gs_last_error()
        assert g.smoother == "jacobi"
    # a Z-slab grid (the loopback emulation: two ranks on one device): its creation under GS_SMOOTHER=zline fails
    # with the reason before any work, and the caller's buffers are untouched
    p = gsv.GridParams(maxiter=1, tol=0.0, gridDim=(70, 33, 41), stencil=gsv.Stencil(list(Z.STRONGZ)))
    nx, ny, nz = p.gridDim
    v = np.full((nz + 2, ny + 2, nx + 2), np.nan)
    cap = 16
    hist, cnt, ap = (C.c_double * cap)(*([-1.0] * cap)), C.c_int(-1), p.to_abi()
    monkeypatch.setenv("GS_SMOOTHER", "zline")
    rc = gsv.driver().gs_zslab_loopback_run(C.byref(ap), 2, 1000, 0, 1, hist, cap, C.byref(cnt), v.ctypes.data_as(A.dptr))
    assert rc == 1
    msg = gsv.driver().gs_last_error().decode()
    assert "ZLINE needs a single-GPU grid" in msg and "Z-slab" in msg, msg
    assert np.isnan(v).all() and cnt.value == -1 and all(x == -1.0 for x in hist)
    monkeypatch.delenv("GS_SMOOTHER")
    rc = gsv.driver().gs_zslab_loopback_run(C.byref(ap), 2, 1000, 0, 1, hist, cap, C.byref(cnt), v.ctypes.data_as(A.dptr))
    assert rc == 0 and cnt.value == 2
