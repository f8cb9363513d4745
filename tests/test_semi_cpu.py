"""XY semi-coarsening without a GPU (include/gpusolve_semi.h): the level-stencil rule against
tests/semi_ref.py word for word, the launchers' argument checks and kernel names in dry-run, the creation-time
refusals a schedule-trace grid can show, and the convergence the method is built for, on the model."""
import ctypes as C

import numpy as np
import pytest

import gpusolve as gsv
import oracle as O
import semi_ref as S
import zline_ref as Z

A = gsv._abi


def abi(values, offsets=O.CANONICAL):
    return gsv.Stencil(list(values), list(offsets)).to_abi()


def words(values):
    return np.asarray(values, dtype=np.float64).view(np.int64).tolist()


def level(nx, ny, nz):
    ldy, ldz, _, _ = gsv.field_layout(nx, ny, nz)
    return gsv.gs_level(nx, ny, nz, ldy, ldz, 0, 1.0 / (ny + 1))


STENCILS = {"WEAKZ": (Z.WEAKZ, O.CANONICAL), "ISO": (Z.ISO, O.CANONICAL), "UPLO": (Z.UPLO, O.CANONICAL),
            "STRONGZ": (Z.STRONGZ, O.CANONICAL), "PERM": Z.permuted(Z.UPLO),
            "odd": ((4.1 / 3, -1.0 / 3, -0.7, -1.0 / 7, -0.9, -0.05 / 3, -0.07), O.CANONICAL)}


@pytest.mark.parametrize("name", sorted(STENCILS))
def test_level_stencil_equals_the_model(name):
    """gs_semi_level_stencil is semi_ref.level_stencil word for word on every level of aligned and non-aligned
    hierarchies; level 0 is the input's bits; offsets and entry order are the input's."""
    values, offsets = STENCILS[name]
    lib = gsv.semi()
    src = abi(values, offsets)
    for dims in ((31, 31, 31), (16, 12, 20), (100, 37, 3), (511, 511, 2), (512, 512, 2)):
        hs = [1.0 / (d[1] + 1) for d in S.level_dims(dims)]
        for l, h in enumerate(hs):
            out = gsv.gs_stencil()
            assert lib.gs_semi_level_stencil(C.byref(src), hs[0], h, C.byref(out)) == 0
            assert words(list(out.s)) == words(S.level_stencil(values, hs[0], h, offsets)), (dims, l)
            assert [(out.ox[i], out.oy[i], out.oz[i]) for i in range(7)] == [tuple(o) for o in offsets]
            if l == 0:
                assert words(list(out.s)) == words(values)
    # in place
    assert lib.gs_semi_level_stencil(C.byref(src), 1.0 / 32, 1.0 / 8, C.byref(src)) == 0
    assert words(list(src.s)) == words(S.level_stencil(values, 1.0 / 32, 1.0 / 8, offsets))


def test_level_stencil_is_exact_on_aligned_sizes():
    """Sizes 2^k - 1 in y give r = 4^l exactly: the z weights are 4^l times the configuration's, the centre
    4^l s0 + (4^l - 1) (sum of the x / y weights), each rounded once."""
    hs = [1.0 / (d[1] + 1) for d in S.level_dims((63, 63, 5))]
    for l, h in enumerate(hs):
        got = S.level_stencil(Z.WEAKZ, hs[0], h)
        r = 4.0 ** l
        assert got[5] == r * Z.WEAKZ[5] and got[6] == r * Z.WEAKZ[6] and got[1:5] == Z.WEAKZ[1:5]
        assert got[0] == r * Z.WEAKZ[0] + (r - 1.0) * -4.0


def test_level_stencil_refusals():
    lib = gsv.semi()
    out = gsv.gs_stencil()
    out.s[:] = [7.0] * 7
    ok = abi(Z.WEAKZ)
    diag = list(O.CANONICAL)
    diag[1] = (1, 1, 0)
    twice = list(O.CANONICAL)
    twice[2] = (1, 0, 0)
    for bad in (abi(Z.WEAKZ, diag), abi(Z.WEAKZ, twice)):
        assert lib.gs_semi_level_stencil(C.byref(bad), 0.5, 0.5, C.byref(out)) == A.GS_EINVAL
    for h0, hl in ((0.0, 0.5), (0.5, -1.0), (float("nan"), 0.5), (0.5, float("inf"))):
        assert lib.gs_semi_level_stencil(C.byref(ok), h0, hl, C.byref(out)) == A.GS_EINVAL
    assert lib.gs_semi_level_stencil(None, 0.5, 0.5, C.byref(out)) == A.GS_EINVAL
    assert lib.gs_semi_level_stencil(C.byref(ok), 0.5, 0.5, None) == A.GS_EINVAL
    assert list(out.s) == [7.0] * 7
    # no dominance test: a stencil gs_zline_supported refuses is re-discretised all the same
    weak = abi((1.9, -0.05, -0.05, -0.05, -0.05, -1.0, -1.0))
    assert gsv.line().gs_zline_supported(C.byref(weak)) == 0
    assert lib.gs_semi_level_stencil(C.byref(weak), 0.5, 0.5, C.byref(out)) == 0


POISON = 0x7FF8_5E41_0000_0C33


class HostField:
    """A poisoned host buffer in a level's layout: a dry-run launcher must leave every word alone."""

    def __init__(self, L):
        self.a = np.full((L.nz + 2) * L.ldz + 64, POISON, dtype=np.int64)
        self.ptr = self.a.ctypes.data

    def untouched(self):
        return bool((self.a == POISON).all())


def host_tables(fl, cl, keep):
    """gs_transfer_tables over HOST arrays (never dereferenced in dry-run) for the XY transition fl -> cl."""
    T = gsv.gs_transfer_tables()
    for a, (nf, nc) in enumerate(((fl.nx, cl.nx), (fl.ny, cl.ny))):
        t = gsv.transfer_axis(nf)
        T.nf[a], T.nc[a] = nf, nc
        for key in ("pj", "pt", "rlo", "rcnt", "rw"):
            arr = np.ascontiguousarray(t[key])
            keep.append(arr)
            getattr(T, key)[a] = arr.ctypes.data
    T.nf[2] = T.nc[2] = fl.nz
    return T


def record(lib):
    buf = C.create_string_buffer(4096)
    n = lib.gs_semi_launch_record(buf, 4096)
    return n, buf.value.decode().split()


def test_launchers_in_dry_run():
    """Every launcher reports its kernel through the launch record (the names gs_semi_kernel gives) without touching
    its poisoned host buffers; every bad argument is GS_EINVAL with nothing recorded."""
    lib = gsv.semi()
    assert lib.gs_semi_launch_dry_run(1) == 0
    try:
        lib.gs_semi_launch_record(C.create_string_buffer(4096), 4096)
        sten = abi(Z.WEAKZ)
        for dims in ((2, 2, 1), (3, 2, 9), (7, 7, 5), (8, 6, 3), (129, 5, 3), (511, 511, 4), (512, 512, 4)):
            fl, cl = level(*dims), level(dims[0] // 2, dims[1] // 2, dims[2])
            keep = []
            T = host_tables(fl, cl, keep)
            v, f, cf, cv = HostField(fl), HostField(fl), HostField(cl), HostField(cl)
            name = lambda op: lib.gs_semi_kernel(op, C.byref(fl), C.byref(cl)).decode()
            assert lib.gs_residual_restrict_xy(C.byref(sten), C.byref(fl), v.ptr, f.ptr, cf.ptr, C.byref(cl), C.byref(T),
                                               None) == 0
            assert record(lib) == (1, ["k_resrestrict_xy"]) and name(A.GS_SEMI_RESIDUAL_RESTRICT) == "k_resrestrict_xy"
            assert lib.gs_restrict_xy(f.ptr, C.byref(fl), cf.ptr, C.byref(cl), C.byref(T), None) == 0
            assert record(lib) == (1, ["k_restrict_xy"]) and name(A.GS_SEMI_RESTRICT) == "k_restrict_xy"
            assert lib.gs_prolong_add_xy(cv.ptr, C.byref(cl), v.ptr, C.byref(fl), C.byref(T), None) == 0
            assert record(lib) == (1, ["k_prolong_add_xy"]) and name(A.GS_SEMI_PROLONG_ADD) == "k_prolong_add_xy"
            assert name(3) == ""

            def refused(fl2=fl, cl2=cl, T2=T, S2=sten, vp=v.ptr):
                sp = C.byref(S2) if S2 is not None else None
                assert lib.gs_residual_restrict_xy(sp, C.byref(fl2), vp, f.ptr, cf.ptr, C.byref(cl2), C.byref(T2),
                                                   None) == A.GS_EINVAL
                if S2 is sten:
                    assert lib.gs_restrict_xy(vp, C.byref(fl2), cf.ptr, C.byref(cl2), C.byref(T2), None) == A.GS_EINVAL
                    assert lib.gs_prolong_add_xy(cv.ptr, C.byref(cl2), vp, C.byref(fl2), C.byref(T2),
                                                 None) == A.GS_EINVAL
                assert record(lib) == (0, [])

            bad = level(*dims)
            bad.z0 = 1
            refused(fl2=bad)
            assert lib.gs_semi_kernel(0, C.byref(bad), C.byref(cl)) == b""
            refused(cl2=level(dims[0] // 2, dims[1] // 2, dims[2] + 1))   # the coarse level keeps nz
            refused(cl2=level(dims[0] // 2 + 1, dims[1] // 2, dims[2]))
            if dims[2] // 2 >= 1:  # a 3-D transition's coarse level
                refused(cl2=level(dims[0] // 2, dims[1] // 2, dims[2] // 2))
            T3 = host_tables(fl, cl, keep)
            T3.nf[2] = fl.nz + 1
            refused(T2=T3)
            T3 = host_tables(fl, cl, keep)
            T3.pj[2] = T3.pj[0]                                         # axis 2 carries no arrays
            refused(T2=T3)
            T3 = host_tables(fl, cl, keep)
            T3.rw[1] = None
            refused(T2=T3)
            T3 = host_tables(fl, cl, keep)
            T3.nf[0] += 1
            refused(T2=T3)
            refused(vp=None)
            refused(S2=None)
            assert all(x.untouched() for x in (v, f, cf, cv))
        # a level with an empty z axis: 0, nothing launched
        fl, cl = level(8, 8, 0), level(4, 4, 0)
        T = host_tables(fl, cl, keep)
        z = HostField(fl)
        assert lib.gs_restrict_xy(z.ptr, C.byref(fl), z.ptr, C.byref(cl), C.byref(T), None) == 0
        assert record(lib) == (0, []) and lib.gs_semi_kernel(1, C.byref(fl), C.byref(cl)) == b""
        # one point in x: no XY transition
        fl, cl = level(1, 8, 3), level(0, 4, 3)
        assert lib.gs_semi_kernel(0, C.byref(fl), C.byref(cl)) == b""
    finally:
        assert lib.gs_semi_launch_dry_run(0) == 1


def _schedule(params, nranks, rank=0):
    d = gsv.driver()
    p = params.to_abi()
    n = C.c_int64(-1)
    rc = d.gs_zslab_schedule(C.byref(p), nranks, rank, 0, None, 0, C.byref(n))
    return rc, n.value, d.gs_last_error().decode() if rc else ""


@pytest.mark.parametrize("nranks", [1, 2])
def test_trace_grid_is_refused(nranks, monkeypatch):
    """GS_COARSEN=xy on a schedule-trace grid (one rank, or a Z-slab of two) fails the creation with the reason;
    GS_COARSEN=xyz and no variable leave the schedule what it was; any other value fails too. GS_SMOOTHER=auto is
    refused there as zline is."""
    lin = gsv.GridParams(maxiter=2, tol=0.0, gridDim=(31, 31, 32), mode=gsv.GS_LINEAR)
    rc, n, _ = _schedule(lin, nranks)
    assert rc == 0 and n > 0
    monkeypatch.setenv("GS_COARSEN", "xyz")
    assert _schedule(lin, nranks) == (0, n, "")
    monkeypatch.setenv("GS_COARSEN", "xy")
    rc, got, err = _schedule(lin, nranks)
    assert rc == 1 and got == -1 and "XY needs a single-GPU grid" in err, err
    monkeypatch.setenv("GS_COARSEN", "nonsense")
    rc, got, err = _schedule(lin, nranks)
    assert rc == 1 and "GS_COARSEN=nonsense" in err, err
    monkeypatch.delenv("GS_COARSEN")
    monkeypatch.setenv("GS_SMOOTHER", "auto")
    rc, got, err = _schedule(lin, nranks)
    assert rc == 1 and got == -1 and "AUTO needs a single-GPU grid" in err, err
    # a mode XY cannot take is named before the grid kind
    monkeypatch.delenv("GS_SMOOTHER")
    monkeypatch.setenv("GS_COARSEN", "xy")
    rc, got, err = _schedule(gsv.GridParams(maxiter=2, tol=0.0, gridDim=(31, 31, 32), mode=gsv.GS_NEWTON), nranks)
    assert rc == 1 and "XY needs a LINEAR grid" in err, err


def test_header_exports_and_binding_agree():
    from conftest import REPO
    from test_abi import declared, exported
    import os

    names = set(declared(os.path.join(REPO, "include", "gpusolve_semi.h")))
    assert names == {"gs_semi_level_stencil", "gs_restrict_xy", "gs_prolong_add_xy", "gs_residual_restrict_xy",
                     "gs_residual_restrict_xy_chunk", "gs_semi_kernel", "gs_semi_launch_dry_run",
                     "gs_semi_launch_record"}
    assert {n for n in exported(A.SEMI_LIB) if n.startswith("gs_")} == names
    assert names == set(A.SEMI_API)


def test_python_names():
    assert (gsv.GS_COARSEN_XYZ, gsv.GS_COARSEN_XY, gsv.GS_SMOOTHER_AUTO) == (0, 1, 2)
    with pytest.raises(ValueError):
        gsv.HipGridData(gsv.GridParams(), coarsen="yz")


# ---- the model's convergence: what the method is for ------------------------------------------------------------
DIMS = (31, 31, 31)


@pytest.fixture(scope="module")
def rhs():
    return Z.normal_rhs(DIMS, seed=1)


def factors(c):
    return Z.factors_per_cycle(c, 8)[2:]  # cycles 3 .. 8


def test_model_convergence_weakz(rhs):
    """WEAKZ at 31^3: XY + z-line gains <= 0.25 per cycle and XY + auto <= 0.30 (levels J J J Z Z), where full
    coarsening stalls at >= 0.65 with either smoother."""
    zl = factors(S.Cycle(DIMS, Z.WEAKZ, smoother="zline", f0=rhs))
    auto_cycle = S.Cycle(DIMS, Z.WEAKZ, smoother="auto", f0=rhs)
    au = factors(auto_cycle)
    full = [factors(Z.cycle(DIMS, Z.WEAKZ, line, f0=rhs)) for line in (False, True)]
    print("XY zline", zl, "XY auto", au, "full point / z-line", full)
    assert auto_cycle.pattern() == "J J J Z Z"
    assert max(zl) <= 0.25 and max(au) <= 0.30
    assert min(full[0]) >= 0.65 and min(full[1]) >= 0.65


@pytest.mark.parametrize("name", ["ISO", "STRONGZ"])
def test_model_convergence_any_z_anisotropy(name, rhs):
    fac = factors(S.Cycle(DIMS, getattr(Z, name), smoother="zline", f0=rhs))
    print(name, "XY zline", fac)
    assert max(fac) <= 0.25


def test_auto_patterns():
    """AUTO's rule on the three stencils: strict inequality, per level stencil."""
    assert S.Cycle(DIMS, Z.ISO, smoother="auto").pattern() == "J Z Z Z Z"
    assert S.Cycle(DIMS, Z.STRONGZ, smoother="auto").pattern() == "Z Z Z Z Z"
    assert S.Cycle((63, 63, 63), Z.WEAKZ, smoother="auto").pattern() == "J J J Z Z Z"
