"""Preconditioned conjugate gradients without a GPU: the model (tests/pcg_ref.py) has the properties the driver's
refusals rest on — the cycle is a symmetric positive preconditioner exactly where gs_grid_pcg accepts a grid —, PCG
beats the stationary iteration, the replayed form reproduces the free-running one, and the new library's boundary is
the header's."""
import os
import re
import subprocess

import numpy as np
import pytest

import gpusolve as gsv
import oracle as O
import pcg_ref as P
from conftest import REPO

CHEB = (0.5695, 1.7319)
# (id, dims, transfer, pre, post, stencil values) — one configuration per kind of grid gs_grid_pcg accepts: aligned
# and even sizes, an anisotropic grid, an anisotropic stencil, explicit Chebyshev weights
ELIGIBLE = [
    ("31-reference", (31, 31, 31), "reference", (0.8, 0.8), (0.8, 0.8), None),
    ("32-position", (32, 32, 32), "position", (0.8, 0.8), (0.8, 0.8), None),
    ("17x33x20-position", (17, 33, 20), "position", (0.8, 0.8), (0.8, 0.8), None),
    ("31-anisotropic", (31, 31, 31), "reference", (0.8, 0.8), (0.8, 0.8), P.ANISO),
    ("31-chebyshev", (31, 31, 31), "reference", CHEB, CHEB, None),
]


def stencil(values):
    return None if values is None else O.Stencil.make(values)


def symmetry(dims, transfer, pre, post, values, seed=5):
    """(<Ma, b>, <a, Mb>, <Ma, a>) for two random vectors."""
    a, b = P.random_rhs(dims, seed), P.random_rhs(dims, seed + 1)
    s = P.Pcg(dims, a, pre=pre, post=post, transfer=transfer, stencil=stencil(values))
    Ma, Mb = s.M(a), s.M(b)
    return P.dot(Ma, b)[0], P.dot(a, Mb)[0], P.dot(Ma, a)[0]


@pytest.mark.parametrize("case", ELIGIBLE, ids=lambda c: c[0])
def test_cycle_is_a_symmetric_positive_preconditioner(case):
    _, dims, transfer, pre, post, values = case
    mab, amb, maa = symmetry(dims, transfer, pre, post, values)
    print(f"{case[0]}: defect {abs(mab - amb) / abs(mab):.3e}, <Ma, a> = {maa:.6e}")
    assert abs(mab - amb) <= 1e-12 * abs(mab)
    assert maa > 0.0


def test_unequal_smoothing_is_not_symmetric():
    """pre = 2, post = 1: why gs_grid_pcg refuses pre != post."""
    mab, amb, _ = symmetry((31, 31, 31), "reference", (0.8, 0.8), (0.8,), None)
    print(f"pre 2 / post 1: defect {abs(mab - amb) / abs(mab):.3e}")
    assert abs(mab - amb) > 1e-3 * abs(mab)


@pytest.fixture(scope="module")
def run32():
    dims = (32, 32, 32)
    f = P.random_rhs(dims, 11)
    s = P.Pcg(dims, f)
    hist, rec = s.run(8)
    return dims, f, hist, rec, s.x


def test_pcg_converges_faster_than_vcycles(run32):
    dims, f, hist, _, _ = run32
    vh, _ = P.vcycles(dims, f, 8)
    print(f"32^3 POSITION: 8 V-cycles {vh[0]:.3e} -> {vh[-1]:.3e}, 8 PCG iterations -> {hist[-1]:.3e}")
    assert len(hist) == 9 and abs(hist[0] - vh[0]) <= 1e-12 * vh[0]
    assert hist[-1] < 1e-2 * vh[-1]
    assert all(b < a for a, b in zip(hist, hist[1:]))


def test_replay_of_own_scalars_is_the_free_run(run32):
    dims, f, hist, rec, x = run32
    s = P.Pcg(dims, f)
    h2, r2 = s.replay([(r["alpha"], r["beta"]) for r in rec])
    assert h2 == hist
    assert np.array_equal(s.x.view(np.int64), x.view(np.int64))
    assert [r["rz"] for r in r2] == [r["rz"] for r in rec]
    for k, r in enumerate(rec):  # the scalars are the quotients of the sums
        assert r["alpha"] == r["rz"] / r["pq"]
        assert r["beta"] == (0.0 if k == 0 else r["rz"] / rec[k - 1]["rz"])


def test_stopping_rule_and_zero_rhs():
    dims = (15, 15, 15)
    f = P.random_rhs(dims, 3)
    full, _ = P.Pcg(dims, f).run(6)
    tol = full[3] / full[0] * 1.0000001  # stops at iteration 3 (the norms fall strictly)
    h, _ = P.Pcg(dims, f).run(6, tol)
    assert h == full[:4]
    h0, rec0 = P.Pcg(dims, O.zeros(*dims)).run(6)
    assert h0 == [0.0] and rec0 == []


def test_dot_bound_covers_a_float_sum():
    rng = np.random.default_rng(2)
    a, b = O.zeros(9, 8, 7), O.zeros(9, 8, 7)
    P.inner(a)[...] = rng.uniform(-1, 1, (9, 8, 7))
    P.inner(b)[...] = rng.uniform(-1, 1, (9, 8, 7))
    exact, sa = P.dot(a, b)
    assert sa > 10 * abs(exact)  # the mixed signs cancel: the bound is about the terms, not about the sum
    naive = 0.0
    for t in (P.inner(a) * P.inner(b)).ravel():
        naive += t
    assert abs(naive - exact) <= P.dot_bound(9 * 8 * 7, sa)


# ---- the library's boundary -------------------------------------------------------------------------------------
HEADER = os.path.join(REPO, "include", "gpusolve_krylov.h")
DECL = re.compile(r"^[A-Za-z_][\w \t\*]*?\b(gs_\w+)\s*\(", re.M)


def declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    return sorted(set(DECL.findall(text)))


def exported(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.strip()}


def test_krylov_library_exports_exactly_its_header():
    names = set(declared(HEADER))
    assert len(names) >= 8 and "gs_krylov_vec_chunk" in names
    got = {n for n in exported(gsv._abi.KRYLOV_LIB) if n.startswith("gs_")}
    assert got == names, got ^ names
    assert names == set(gsv._abi.KRYLOV_API), names ^ set(gsv._abi.KRYLOV_API)
    k = gsv._abi.krylov()
    assert all(hasattr(k, n) for n in names)
    for other in ("gpusolve_hip.h", "gpusolve_transfer.h", "gpusolve_driver.h", "gpusolve_diag.h"):
        assert not (names & set(declared(os.path.join(REPO, "include", other)))), other


def test_krylov_sources_read_no_environment():
    csrc = os.path.join(REPO, "gpu-solve_amd", "csrc")
    for name in ("gs_krylov.hip", "gs_krylov_device.hpp"):
        text = open(os.path.join(csrc, name)).read()
        assert "getenv" not in text, name
        assert not re.findall(r'"GS_[A-Z0-9_]+"', text), name


def test_driver_declares_and_binds_pcg():
    names = set(declared(os.path.join(REPO, "include", "gpusolve_driver.h")))
    want = {"gs_grid_pcg", "gs_grid_pcg_supported", "gs_grid_pcg_record"}
    assert want <= names and want <= set(gsv._abi.DRIVER_API) and want <= exported(gsv._abi.DRIVER_LIB)
    assert hasattr(gsv.HipSolver, "pcg") and hasattr(gsv.HipGridData, "pcg_supported")
    assert hasattr(gsv.HipGridData, "pcg_record")


def _schedule(params, nranks, rank=0):
    """(return code, schedule length, error text) of gs_zslab_schedule: the driver's solve on a trace grid, no device."""
    import ctypes as C
    d = gsv.driver()
    p = params.to_abi()
    n = C.c_int64(-1)
    rc = d.gs_zslab_schedule(C.byref(p), nranks, rank, 0, None, 0, C.byref(n))
    return rc, n.value, d.gs_last_error().decode() if rc else ""


@pytest.mark.parametrize("nranks", [1, 2])
def test_trace_grid_is_refused(nranks, monkeypatch):
    """gs_grid_pcg's "Z-slab / RCCL or trace grid" refusal, the trace half: under GS_SOLVER=pcg the solve of a LINEAR
    schedule-trace grid — one rank or a Z-slab of two — fails with the reason before one operation is recorded. The
    other modes keep their solver, and without the variable the schedule is what it was."""
    lin = gsv.GridParams(maxiter=2, tol=0.0, gridDim=(31, 31, 32), mode=gsv.GS_LINEAR)
    rc, n, _ = _schedule(lin, nranks)
    assert rc == 0 and n > 0
    monkeypatch.setenv("GS_SOLVER", "vcycle")
    assert _schedule(lin, nranks) == (0, n, "")
    monkeypatch.setenv("GS_SOLVER", "pcg")
    for rank in range(nranks):
        rc, got, err = _schedule(lin, nranks, rank)
        assert rc == 1 and got == -1, (rc, got)
        assert "PCG: single-GPU grids only (not a Z-slab / RCCL or schedule-trace grid)" in err, err
    nonlin = gsv.GridParams(maxiter=2, tol=0.0, gridDim=(31, 31, 32), mode=gsv.GS_NONLINEAR)
    rc, got, _ = _schedule(nonlin, nranks)
    assert rc == 0 and got > 0


def test_pcg_dir_instance_selection_needs_no_device():
    """gs_pcg_dir_kernel is the launcher's own predicate: the z-march from 1024 blocks of 4-plane chunks on, canonical
    stencil order only; refused arguments give the empty name and no partials."""
    k = gsv._abi.krylov()
    import ctypes as C

    def level(nx, ny, nz):
        ldy, ldz, _, _ = gsv.field_layout(nx, ny, nz)
        return gsv.gs_level(nx, ny, nz, ldy, ldz, 0, 1.0 / (ny + 1))

    unit, gen = gsv.Stencil().to_abi(), gsv.Stencil(list(P.ANISO)).to_abi()
    perm = gsv.Stencil([6, -1, -1, -1, -1, -1, -1], [gsv.CANONICAL_OFFSETS[i] for i in (0, 2, 1, 4, 3, 6, 5)]).to_abi()
    name = lambda S, L, first: k.gs_pcg_dir_kernel(C.byref(S), C.byref(L), first).decode()
    big, small = level(257, 17, 501), level(33, 17, 9)
    assert name(unit, big, 0) == "k_pcg_dir_rb<true, false>" and name(unit, big, 1) == "k_pcg_dir_rb<true, true>"
    assert name(gen, big, 0) == "k_pcg_dir_rb<false, false>" and name(gen, big, 1) == "k_pcg_dir_rb<false, true>"
    assert name(perm, big, 0) == "k_pcg_dir_gen<false>" and name(unit, small, 1) == "k_pcg_dir_gen<true>"
    assert k.gs_pcg_dir_num_partials(C.byref(unit), C.byref(big)) == 3 * 3 * 126
    assert k.gs_pcg_dir_num_partials(C.byref(unit), C.byref(small)) == 1 * 5 * 9
    bad = level(33, 17, 9)
    bad.z0 = 1
    assert name(unit, bad, 0) == "" and k.gs_pcg_dir_num_partials(C.byref(unit), C.byref(bad)) == 0
    assert k.gs_pcg_step_num_partials(C.byref(bad)) == 0 and k.gs_dot_num_partials(C.byref(bad)) == 0
