"""The z-line smoother without a GPU: gs_zline_factors and gs_zline_supported (pure host code of
libgpusolve_line.so) against the model of tests/zline_ref.py, the model's line solve against numpy.linalg.solve, the
convergence the feature is for — z-line V-cycles gain 0.11-0.15 per cycle on a stencil whose z weights dominate, where
point Jacobi V-cycles gain 0.67-0.78 — with the cases it does not help, the symmetry of the z-line cycle, and the new
library's boundary.

Set-up of the convergence figures: 2+2 sweeps at omega = 0.8, the oracle's transfers, a zero start,
f = default_rng(1).standard_normal on the interior."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import gpusolve as gsv
import oracle as O
import pcg_ref as P
import zline_ref as Z
from conftest import REPO

STENCILS = {
    "strongz": (Z.STRONGZ, list(O.CANONICAL)),
    "iso": (Z.ISO, list(O.CANONICAL)),
    "uplo": (Z.UPLO, list(O.CANONICAL)),
    "permuted": Z.permuted(Z.UPLO),
}


def abi(values, offsets):
    return gsv.Stencil(list(values), [tuple(o) for o in offsets]).to_abi()


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


@pytest.mark.parametrize("sname", list(STENCILS))
@pytest.mark.parametrize("nz", [1, 2, 3, 7, 300])
def test_factors_word_for_word(nz, sname):
    values, offsets = STENCILS[sname]
    S = abi(values, offsets)
    assert gsv.line().gs_zline_supported(C.byref(S)) == 1 and Z.supported(values, offsets)
    cp, den = np.full(nz + 4, np.nan), np.full(nz + 4, np.nan)  # two guard words behind each table
    assert gsv.line().gs_zline_factors(C.byref(S), nz, cp.ctypes.data_as(gsv._abi.dptr),
                                       den.ctypes.data_as(gsv._abi.dptr)) == 0
    wcp, wden = Z.factors(values, nz, offsets)
    assert (bits(cp[:nz + 2]) == bits(wcp)).all() and (bits(den[:nz + 2]) == bits(wden)).all()
    assert np.isnan(cp[nz + 2:]).all() and np.isnan(den[nz + 2:]).all()
    assert cp[0] == den[0] == cp[nz + 1] == den[nz + 1] == 0.0
    s0, up, lo, _ = Z.shape_of(values, offsets)
    assert den[1] == s0 and (np.abs(den[1:nz + 1]) >= abs(s0) - abs(lo)).all()  # the header's bound


def test_supported_refusals():
    ln = gsv.line()
    ok = lambda values, offsets=O.CANONICAL: ln.gs_zline_supported(C.byref(abi(values, offsets)))
    assert ok(Z.STRONGZ) == 1 and ok(Z.ISO) == 1 and ok(Z.WEAKZ) == 1
    rep = list(O.CANONICAL)
    rep[2] = (1, 0, 0)  # (+1, 0, 0) twice, (-1, 0, 0) missing
    diag = list(O.CANONICAL)
    diag[4] = (1, -1, 0)
    cases = {"a repeated offset": (Z.STRONGZ, rep), "a diagonal offset": (Z.STRONGZ, diag),
             "s0 = 0": ((0.0, -0.05, -0.05, -0.05, -0.05, 0.0, 0.0), O.CANONICAL),
             "|s0| < |up| + |lo|": ((1.9, -0.05, -0.05, -0.05, -0.05, -1.0, -1.0), O.CANONICAL),
             "a NaN weight": ((2.2, -0.05, -0.05, -0.05, -0.05, float("nan"), -1.0), O.CANONICAL)}
    for what, (values, offsets) in cases.items():
        assert ok(values, offsets) == 0, what
        assert not Z.supported(values, offsets), what
        cp, den = np.full(5, np.nan), np.full(5, np.nan)
        assert ln.gs_zline_factors(C.byref(abi(values, offsets)), 3, cp.ctypes.data_as(gsv._abi.dptr),
                                   den.ctypes.data_as(gsv._abi.dptr)) == gsv._abi.GS_EINVAL, what
        assert np.isnan(cp).all() and np.isnan(den).all(), what
    assert ok((2.0, -0.05, -0.05, -0.05, -0.05, -1.0, -1.0)) == 1  # equality is accepted
    assert ln.gs_zline_supported(None) == 0
    good = abi(Z.STRONGZ, O.CANONICAL)
    one = np.zeros(8)
    assert ln.gs_zline_factors(C.byref(good), -1, one.ctypes.data_as(gsv._abi.dptr),
                               one.ctypes.data_as(gsv._abi.dptr)) == gsv._abi.GS_EINVAL
    assert ln.gs_zline_factors(C.byref(good), 3, None, one.ctypes.data_as(gsv._abi.dptr)) == gsv._abi.GS_EINVAL


@pytest.mark.parametrize("sname", ["strongz", "iso"])
def test_line_solve_against_linalg(sname):
    """nz = 300: the two passes against numpy.linalg.solve on the column's matrix, to 1e-12 of the column's maximum
    (condition numbers <= 21 and <= 2; measured 3e-16)."""
    values, offsets = STENCILS[sname]
    nz = 300
    A = Z.column_matrix(values, nz, offsets)
    assert np.linalg.cond(A) <= (21 if sname == "strongz" else 2)
    b = np.random.default_rng(7).standard_normal((5, nz))
    u = Z.line_solve(b, values, offsets)
    ref = np.linalg.solve(A, b.T).T
    err = np.abs(u - ref).max(axis=1) / np.abs(ref).max(axis=1)
    print(f"{sname}: line solve against linalg.solve, max relative error {err.max():.3e}")
    assert (err <= 1e-12).all()


def test_sweep_is_the_exact_line_solve_at_omega_one():
    """omega = 1: A v_out = f along every column with the x / y neighbours of v_in (the oracle's residual of the
    mixed iterate is zero to rounding), and the zero iterate equals a zeroed field under ==."""
    dims = (5, 4, 9)
    rng = np.random.default_rng(3)
    v, f = O.zeros(*dims), O.zeros(*dims)
    P.inner(v)[...] = rng.standard_normal(dims)
    P.inner(f)[...] = rng.standard_normal(dims)
    h = 1.0 / (dims[1] + 1)
    out = Z.sweep(v, f, h, 1.0, Z.UPLO)
    s0, up, lo, xy = Z.shape_of(Z.UPLO)
    g = sum(w * v[1 + ox:6 + ox, 1 + oy:5 + oy, 1:-1] for w, (ox, oy) in xy)
    lhs = s0 * out[1:-1, 1:-1, 1:-1] + up * out[1:-1, 1:-1, 2:] + lo * out[1:-1, 1:-1, :-2] + g
    assert np.abs(lhs / (h * h) - P.inner(f)).max() <= 1e-12 * np.abs(P.inner(f)).max()
    assert np.array_equal(Z.sweep(None, f, h, 0.8, Z.UPLO), Z.sweep(O.zeros(*dims), f, h, 0.8, Z.UPLO))


@pytest.fixture(scope="module")
def strongz_factors():
    """Per-cycle factors of cycles 1-8 at 31^3 and 63^3, z-line and point: {(n, zline): [..]} — computed once."""
    out = {}
    for n in (31, 63):
        f = Z.normal_rhs((n, n, n))
        for zl in (True, False):
            out[n, zl] = Z.factors_per_cycle(Z.cycle((n, n, n), Z.STRONGZ, zl, f0=f))
            print(f"{n}^3 STRONGZ {'z-line' if zl else 'point '}: " + " ".join(f"{x:.3f}" for x in out[n, zl]))
    return out


@pytest.mark.parametrize("n,zmax,pmin", [(31, 0.130, 0.666), (63, 0.149, 0.670)])
def test_strongz_convergence(strongz_factors, n, zmax, pmin):
    zl, pt = strongz_factors[n, True][2:8], strongz_factors[n, False][2:8]
    assert max(zl) <= 0.2 and min(pt) >= 0.6
    # the figures DESIGN.md §4.11 states (measured max / min of cycles 3-8): within 0.02
    assert abs(max(zl) - zmax) <= 0.02 and abs(min(pt) - pmin) <= 0.02, (max(zl), min(pt))


@pytest.mark.parametrize("n,want", [(31, None), (63, (0.268, 0.271))])
def test_isotropic_stencil_gains_nothing(n, want):
    f = Z.normal_rhs((n, n, n))
    got = [max(Z.factors_per_cycle(Z.cycle((n, n, n), Z.ISO, zl, f0=f))[2:8]) for zl in (True, False)]
    print(f"{n}^3 isotropic: z-line {got[0]:.3f}, point {got[1]:.3f}")
    assert got[0] <= 0.3 and got[1] <= 0.3
    if want:
        assert abs(got[0] - want[0]) <= 0.02 and abs(got[1] - want[1]) <= 0.02, got


def test_weak_z_is_not_helped():
    """DESIGN.md §4.10's stencil (the weak axis is z): line relaxation along z changes nothing there."""
    n = 31
    f = Z.normal_rhs((n, n, n))
    got = [Z.factors_per_cycle(Z.cycle((n, n, n), Z.WEAKZ, zl, f0=f))[7] for zl in (True, False)]
    print(f"{n}^3 weak-z: cycle 8 factor z-line {got[0]:.3f}, point {got[1]:.3f}")
    assert abs(got[0] - got[1]) <= 0.02 and got[0] >= 0.6


def test_iterations_to_1e8_at_31():
    """89 / 22 / 8 / 6 at 31^3: point V-cycles, PCG on the point cycle, z-line V-cycles, PCG on the z-line cycle."""
    dims = (31, 31, 31)
    f = Z.normal_rhs(dims)
    counts = []
    for zl in (False, True):
        hist = Z.cycle(dims, Z.STRONGZ, zl, f0=f).solve(100 if not zl else 12)
        counts.append(next(i for i, r in enumerate(hist) if r <= 1e-8 * hist[0]))
        counts.append(Z.pcg_iterations(dims, Z.STRONGZ, f, zl)[0])
    print(f"31^3 STRONGZ to 1e-8: point V {counts[0]}, point PCG {counts[1]}, z-line V {counts[2]}, z-line PCG {counts[3]}")
    assert counts[2] <= 9 and counts[3] <= 7 and counts[0] >= 8 * counts[2] and counts[1] >= 3 * counts[3]


def test_zline_cycle_is_symmetric():
    """|<Ma, b> - <a, Mb>| / |<Ma, b>| at 15^3, 2+2, under tests/test_pcg_cpu.py's bound for its eligible grids."""
    dims = (15, 15, 15)
    a, b = P.random_rhs(dims, 5), P.random_rhs(dims, 6)

    def M(r):
        c = Z.ZCycle(dims, Z.STRONGZ, f0=r)
        c.vcycle_from(0)
        return c.v[0]

    mab, amb, maa = P.dot(M(a), b)[0], P.dot(a, M(b))[0], P.dot(M(a), a)[0]
    print(f"z-line cycle: defect {abs(mab - amb) / abs(mab):.3e}, <Ma, a> = {maa:.6e}")
    assert abs(mab - amb) <= 1e-12 * abs(mab)
    assert maa > 0.0


# ---- the library's boundary -------------------------------------------------------------------------------------
HEADER = os.path.join(REPO, "include", "gpusolve_line.h")
DECL = re.compile(r"^[A-Za-z_][\w \t\*]*?\b(gs_\w+)\s*\(", re.M)


def declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    return sorted(set(DECL.findall(text)))


def exported(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.strip()}


def test_line_library_exports_exactly_its_header():
    names = set(declared(HEADER))
    assert names == {"gs_zline_supported", "gs_zline_factors", "gs_zline_sweep", "gs_zline_kernel"}
    got = {n for n in exported(gsv._abi.LINE_LIB) if n.startswith("gs_")}
    assert got == names, got ^ names
    assert names == set(gsv._abi.LINE_API), names ^ set(gsv._abi.LINE_API)
    for other in ("gpusolve_hip.h", "gpusolve_transfer.h", "gpusolve_krylov.h", "gpusolve_driver.h", "gpusolve_diag.h"):
        assert not (names & set(declared(os.path.join(REPO, "include", other)))), other


def test_line_sources_read_no_environment():
    csrc = os.path.join(REPO, "gpu-solve_amd", "csrc")
    for name in ("gs_line.hip", "gs_line_device.hpp"):
        text = open(os.path.join(csrc, name)).read()
        assert "getenv" not in text, name
        assert not re.findall(r'"GS_[A-Z0-9_]+"', text), name


def test_driver_declares_and_binds_the_smoother():
    names = set(declared(os.path.join(REPO, "include", "gpusolve_driver.h")))
    want = {"gs_grid_set_smoother", "gs_grid_get_smoother"}
    assert want <= names and want <= set(gsv._abi.DRIVER_API) and want <= exported(gsv._abi.DRIVER_LIB)
    assert hasattr(gsv.HipGridData, "set_smoother") and hasattr(gsv.HipGridData, "smoother")
    assert (gsv.GS_SMOOTHER_JACOBI, gsv.GS_SMOOTHER_ZLINE) == (0, 1)


def test_instance_selection_needs_no_device():
    """gs_zline_kernel is the launcher's own predicate: the marching instance from 32 * 32 columns on, canonical
    order only; refused arguments and empty levels give the empty name."""
    ln = gsv.line()

    def level(nx, ny, nz):
        ldy, ldz, _, _ = gsv.field_layout(nx, ny, nz)
        return gsv.gs_level(nx, ny, nz, ldy, ldz, 0, 1.0 / (ny + 1))

    can, perm = abi(Z.STRONGZ, O.CANONICAL), abi(*Z.permuted(Z.STRONGZ))
    name = lambda S, L, zero: ln.gs_zline_kernel(C.byref(S), C.byref(L), zero).decode()
    assert name(can, level(32, 32, 1), 0) == "k_zline_march<false>"
    assert name(can, level(32, 32, 1), 1) == "k_zline_march<true>"
    assert name(can, level(33, 31, 5), 0) == "k_zline_col<false>"  # 1023 columns
    assert name(can, level(1, 1, 4093), 1) == "k_zline_col<true>"
    assert name(perm, level(128, 128, 3), 0) == "k_zline_col<false>"
    bad = level(33, 5, 9)
    bad.z0 = 1
    assert name(can, bad, 0) == "" and name(can, level(0, 5, 9), 0) == ""
    assert name(abi((1.9, -0.05, -0.05, -0.05, -0.05, -1.0, -1.0), O.CANONICAL), level(33, 5, 9), 0) == ""


def _schedule(params, nranks, rank=0):
    d = gsv.driver()
    p = params.to_abi()
    n = C.c_int64(-1)
    rc = d.gs_zslab_schedule(C.byref(p), nranks, rank, 0, None, 0, C.byref(n))
    return rc, n.value, d.gs_last_error().decode() if rc else ""


@pytest.mark.parametrize("nranks", [1, 2])
def test_trace_grid_is_refused(nranks, monkeypatch):
    """GS_SMOOTHER=zline on a schedule-trace grid (one rank, or a Z-slab of two) fails the creation with the reason;
    GS_SMOOTHER=jacobi and no variable leave the schedule what it was; any other value fails too."""
    lin = gsv.GridParams(maxiter=2, tol=0.0, gridDim=(31, 31, 32), mode=gsv.GS_LINEAR)
    rc, n, _ = _schedule(lin, nranks)
    assert rc == 0 and n > 0
    monkeypatch.setenv("GS_SMOOTHER", "jacobi")
    assert _schedule(lin, nranks) == (0, n, "")
    monkeypatch.setenv("GS_SMOOTHER", "zline")
    rc, got, err = _schedule(lin, nranks)
    assert rc == 1 and got == -1 and "ZLINE needs a single-GPU grid" in err, err
    monkeypatch.setenv("GS_SMOOTHER", "lines")
    rc, got, err = _schedule(lin, nranks)
    assert rc == 1 and "GS_SMOOTHER=lines" in err, err
