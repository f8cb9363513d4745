"""gs_grid_pcg on the device against tests/pcg_ref.py.

Replay: the model fed the device's own alpha_k and beta_k goes through the same roundings, so x must agree bit for bit;
each recorded sum must lie within the any-order bound (pcg_ref.dot_bound) of the exactly rounded sum over the replayed
fields, alpha and beta must be the IEEE quotients of the recorded sums and hist[k] the square root of the recorded
r . r. Free-running: every entry of the history agrees with the model's to 1e-9 relative (the project's LINEAR history
tolerance); the cases keep their last norm above 1e-8 r0. Then the state the call leaves behind, its stopping rule,
every refusal (the RCCL one on two rank processes; the schedule-trace one needs no device and is in
tests/test_pcg_cpu.py), the zero right-hand side, and GS_SOLVER through the executable."""
import functools
import importlib.util
import math
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import gpusolve as gsv  # noqa: E402
import oracle as O  # noqa: E402
import pcg_ref as P  # noqa: E402
import xfer_ref as X  # noqa: E402
from conftest import REPO  # noqa: E402

CHEB = (0.5695, 1.7319)
# id: (dims, transfer, pre weights, post weights, explicit weights?, stencil values, uploaded x0?)
CASES = {
    "31": ((31, 31, 31), "reference", (0.8, 0.8), (0.8, 0.8), False, None, False),
    "32-position": ((32, 32, 32), "position", (0.8, 0.8), (0.8, 0.8), False, None, False),
    "17x33x20-position-x0": ((17, 33, 20), "position", (0.8, 0.8), (0.8, 0.8), False, None, True),
    "15-anisotropic": ((15, 15, 15), "reference", (0.8, 0.8), (0.8, 0.8), False, P.ANISO, False),
    "31-chebyshev": ((31, 31, 31), "reference", CHEB, CHEB, True, None, False),
    "31-1+1": ((31, 31, 31), "reference", (0.8,), (0.8,), False, None, False),
    "31-3+3": ((31, 31, 31), "reference", (0.8,) * 3, (0.8,) * 3, False, None, False),
    "127x127x63": ((127, 127, 63), "reference", (0.8, 0.8), (0.8, 0.8), False, None, False),
}
ITERS = 6
by_case = pytest.mark.parametrize("cid", list(CASES))


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def same(a, b, what):
    ne = bits(a) != bits(b)
    assert not ne.any(), f"{what}: {int(ne.sum())} words differ, first at {tuple(np.argwhere(ne)[0])}"


def inputs(cid):
    dims = CASES[cid][0]
    f = P.random_rhs(dims, 100 + len(cid))
    x0 = P.random_rhs(dims, 200 + len(cid)) * 1e-3 if CASES[cid][6] else None
    return f, x0


def make_grid(cid, maxiter=ITERS, tol=0.0, f=None, x0=None):
    dims, transfer, pre, post, explicit, values, _ = CASES[cid]
    st = gsv.Stencil() if values is None else gsv.Stencil(list(values))
    g = gsv.HipGridData(gsv.GridParams(maxiter=maxiter, tol=tol, gridDim=dims, mode=gsv.GS_LINEAR, preSmoothing=len(pre),
                                       postSmoothing=len(post), stencil=st))
    if transfer == "position":
        g.set_transfer("position")
    if explicit:
        g.set_weights(pre, post)
    if f is not None:
        g.set_field(0, "f", f)
    if x0 is not None:
        g.set_field(0, "v", x0)
    return g


def model(cid, f, x0):
    dims, transfer, pre, post, _, values, _ = CASES[cid]
    return P.Pcg(dims, f, x0, pre, post, transfer, None if values is None else O.Stencil.make(values))


@functools.lru_cache(maxsize=None)
def device_run(cid):
    """One 6-iteration run with tol = 0: everything the tests below read, downloaded once."""
    f, x0 = inputs(cid)
    with make_grid(cid, f=f, x0=x0) as g:
        assert g.pcg_supported(), g.pcg_refusal
        hist = gsv.HipSolver.pcg(g)
        out = dict(hist=hist, breakdown=g.pcg_breakdown, rec=g.pcg_record(), x=g.field(0, "v").copy(),
                   f=g.field(0, "f").copy(), true_res=gsv.HipSolver.compResidual(g, 0),
                   fused=[bool(gsv.driver().gs_grid_level_fused(g.handle, l)) for l in range(g.numLevels())])
    return out


@functools.lru_cache(maxsize=None)
def replayed(cid):
    f, x0 = inputs(cid)
    d = device_run(cid)
    m = model(cid, f, x0)
    hist, rec = m.replay([(r["alpha"], r["beta"]) for r in d["rec"]])
    return hist, rec, m.x


@functools.lru_cache(maxsize=None)
def free_run(cid):
    f, x0 = inputs(cid)
    return model(cid, f, x0).run(ITERS)[0]


@by_case
def test_replay_gives_the_same_bits(cid):
    d = device_run(cid)
    assert not d["breakdown"] and len(d["hist"]) == ITERS + 1 and len(d["rec"]) == ITERS
    _, _, x = replayed(cid)
    same(d["x"], x, f"{cid}: x after {ITERS} iterations")
    if cid == "127x127x63":
        assert d["fused"][0] and d["fused"][1], d["fused"]  # fused pairs (and tiled legs below) took part


@by_case
def test_recorded_scalars(cid):
    d = device_run(cid)
    _, rec, _ = replayed(cid)
    dims = CASES[cid][0]
    n = dims[0] * dims[1] * dims[2]
    for k, (dv, rf) in enumerate(zip(d["rec"], rec)):
        for key in ("rz", "pq", "rr"):
            bound = P.dot_bound(n, rf[key + "_abs"])
            print(f"{cid} k={k} {key}: device {dv[key]!r} exact {rf[key]!r} bound {bound:.3e}")
            assert abs(dv[key] - rf[key]) <= bound, (cid, k, key)
        assert dv["flag"] == 0.0
        assert dv["alpha"] == dv["rz"] / dv["pq"], (cid, k)
        assert dv["beta"] == (0.0 if k == 0 else dv["rz"] / d["rec"][k - 1]["rz"]), (cid, k)
        assert d["hist"][k + 1] == math.sqrt(dv["rr"]), (cid, k)


@by_case
def test_free_running_history(cid):
    d, ref = device_run(cid), free_run(cid)
    assert len(ref) == ITERS + 1 and len(d["hist"]) == ITERS + 1
    # the cases are chosen so that ITERS iterations stay above 1e-8 r0 (the fastest, 3+3 sweeps and the Chebyshev
    # weights, end at 2.6e-8 and 2.9e-8 r0 in the model): every entry of the history is compared
    assert ref[-1] > 1e-8 * ref[0], (cid, ref)
    for k, (a, b) in enumerate(zip(d["hist"], ref)):
        print(f"{cid} hist[{k}]: device {a!r} model {b!r} rel {abs(a - b) / b:.3e}")
    for k, (a, b) in enumerate(zip(d["hist"], ref)):
        assert abs(a - b) <= 1e-9 * b, (cid, k)


@by_case
def test_true_residual_follows_the_recurrence(cid):
    d = device_run(cid)
    print(f"{cid}: true {d['true_res']!r} recurrence {d['hist'][-1]!r} r0 {d['hist'][0]!r}")
    assert abs(d["true_res"] - d["hist"][-1]) <= 1e-12 * d["hist"][0]


@by_case
def test_f_and_ring_after_the_call(cid):
    d = device_run(cid)
    f, _ = inputs(cid)
    same(d["f"], f, f"{cid}: level 0's f after the call")
    ring = d["x"].copy()
    P.inner(ring)[...] = 0.0
    assert not ring.any() and np.isfinite(d["x"]).all()


@pytest.mark.parametrize("nopipe", [False, True], ids=["pipelined", "GS_NO_PIPELINE"])
def test_stopping_rule(nopipe, monkeypatch):
    cid = "31"
    f, _ = inputs(cid)
    ref = free_run(cid)
    tol = math.sqrt(ref[3] * ref[2]) / ref[0]  # between the norms of iterations 2 and 3: stops at iteration 3
    if nopipe:
        monkeypatch.setenv("GS_NO_PIPELINE", "1")
    with make_grid(cid, maxiter=ITERS, tol=tol, f=f) as g:
        hist = gsv.HipSolver.pcg(g)
        x, rec = g.field(0, "v").copy(), g.pcg_record()
    assert len(hist) == 4 and len(rec) == 3
    m = model(cid, f, None)
    m.replay([(r["alpha"], r["beta"]) for r in rec])
    same(x, m.x, "x after a run that tol stopped at iteration 3")
    full = device_run(cid)
    assert hist == full["hist"][:4]  # the same bits with and without the overlap, and as the run that went on
    assert [r["alpha"] for r in rec] == [r["alpha"] for r in full["rec"][:3]]


def test_operations_after_the_call_continue_from_x():
    cid = "31"
    f, _ = inputs(cid)
    d = device_run(cid)
    dims, _, pre, post, _, _, _ = CASES[cid]
    with make_grid(cid, maxiter=3, f=f) as g:
        h1 = gsv.HipSolver.pcg(g)
        assert h1 == d["hist"][:4]
        x3 = g.field(0, "v").copy()
        # a second call continues from x
        h2 = gsv.HipSolver.pcg(g)
        m = P.Pcg(dims, f, x3, pre, post, "reference")
        m.replay([(r["alpha"], r["beta"]) for r in g.pcg_record()])
        same(g.field(0, "v"), m.x, "x after a second gs_grid_pcg")
        assert abs(h2[0] - h1[-1]) <= 1e-12 * h1[0]
        # a V-cycle and a solve continue from it too, bit for bit (LINEAR)
        c = X.Cycle(dims, O.LINEAR, pre, post, f0=f, v0=m.x, transfer="reference")
        res = gsv.HipSolver.vcycle(g)
        want = c.vcycle()
        same(g.field(0, "v"), c.v[0], "v after gs_grid_vcycle")
        assert abs(res - want) <= 1e-9 * want
        hs = gsv.HipSolver.solve(g)
        wants = c.solve(3)
        same(g.field(0, "v"), c.v[0], "v after gs_grid_solve")
        assert len(hs) == 4 and all(abs(a - b) <= 1e-9 * b for a, b in zip(hs, wants))
        same(g.field(0, "f"), f, "f after the session")


def refused(g, reason):
    before = [g.field(0, "v").copy(), g.field(0, "f").copy()]
    assert not g.pcg_supported()
    assert reason in g.pcg_refusal, g.pcg_refusal
    with pytest.raises(gsv.GpuSolveError, match=re.escape(reason)):
        gsv.HipSolver.pcg(g)
    n = gsv._abi.C.c_int(-5)
    assert gsv.driver().gs_grid_pcg(g.handle, 0, None, 0, gsv._abi.C.byref(n)) == 1 and n.value == -5
    same(g.field(0, "v"), before[0], "v after a refused call")
    same(g.field(0, "f"), before[1], "f after a refused call")


def grid(dims=(15, 15, 15), mode=gsv.GS_LINEAR, pre=2, post=2, stencil=None):
    return gsv.HipGridData(gsv.GridParams(maxiter=3, tol=0.0, gridDim=dims, mode=mode, preSmoothing=pre,
                                          postSmoothing=post, stencil=stencil or gsv.Stencil()))


def test_refusals():
    for mode in (gsv.GS_NONLINEAR, gsv.GS_NEWTON):
        with grid(mode=mode) as g:
            refused(g, "LINEAR grids only")
    for pre, post in ((2, 1), (1, 2), (0, 0)):
        with grid(pre=pre, post=post) as g:
            refused(g, "pre = post >= 1")
    with grid() as g:
        g.set_weights((0.8, 0.9), (0.8, 1.0))
        refused(g, "post-smoothing weights must be the pre-smoothing weights in some order")
        g.set_weights((0.8, 0.9), (0.9, 0.8))  # Jacobi factors commute: the order is free
        assert g.pcg_supported() and g.pcg_refusal is None
        g.clear_weights()
        assert g.pcg_supported()
    with grid(stencil=gsv.Stencil([6, -1, -1.5, -1, -1, -1, -1])) as g:
        refused(g, "stencil must be symmetric")
    off = list(gsv.CANONICAL_OFFSETS)
    off[2] = (1, 1, 0)  # (-1, 0, 0) is missing: (1, 0, 0) and (1, 1, 0) lack their pairs
    with grid(stencil=gsv.Stencil([6, -1, -1, -1, -1, -1, -1], off)) as g:
        refused(g, "stencil must be symmetric")
    with grid(dims=(16, 16, 16)) as g:
        refused(g, "do not align")
        g.set_transfer("position")
        assert g.pcg_supported()
    with grid() as g:
        with pytest.raises(gsv.GpuSolveError, match="no run to report"):
            g.pcg_record()


def test_rccl_grid_is_refused(tmp_path):
    """A Z-slab / RCCL grid: two rank processes on one GPU (the harness of tests/test_gpu_rccl_multirank.py) build
    their slabs under GS_SOLVER=pcg; each rank's solve is refused with the reason before any work or collective."""
    from test_gpu_rccl_multirank import start_ranks
    procs = start_ranks(tmp_path, 2, gsv.GS_LINEAR, (32, 32, 32), 3, {"GS_SOLVER": "pcg"})
    res = []
    for p, _ in procs:
        try:
            res.append(p.communicate(timeout=150))
        except subprocess.TimeoutExpired:
            for q, _ in procs:
                q.kill()
            raise
    for (p, out), (_, err) in zip(procs, res):
        assert p.returncode not in (0, None), err[-2000:]
        assert "PCG: single-GPU grids only" in err, err[-2000:]
        assert not os.path.exists(out)  # (the probe saves its slab after a solve: none ran)


def test_zero_right_hand_side():
    dims = (15, 15, 15)
    with grid(dims) as g:
        g.set_field(0, "f", O.zeros(*dims))
        hist = gsv.HipSolver.pcg(g)
        assert hist == [0.0] and g.pcg_breakdown
        x, rec = g.field(0, "v"), g.pcg_record()
        assert not x.any() and np.isfinite(x).all()
        assert len(rec) == 1 and rec[0]["flag"] != 0.0 and rec[0]["alpha"] == 0.0
        assert all(math.isfinite(v) for v in rec[0].values())
        n = gsv._abi.C.c_int(0)
        assert gsv.driver().gs_grid_pcg(g.handle, 0, None, 0, gsv._abi.C.byref(n)) == gsv.GS_PCG_BREAKDOWN
        assert n.value == 1


def _iter_regex():
    spec = importlib.util.spec_from_file_location("run_experiments", os.path.join(REPO, "tools", "run_experiments.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.ITER


def test_gs_solver_switch(tmp_path, monkeypatch):
    params = gsv.GridParams(maxiter=5, tol=0.0, gridDim=(31, 31, 31), mode=gsv.GS_LINEAR)
    conf = tmp_path / "pcg.conf"
    conf.write_text(params.config_text())
    exe = gsv._abi.EXECUTABLE
    with gsv.HipGridData(params) as g:
        api = gsv.HipSolver.pcg(g)
        plain = gsv.HipSolver.fmg(g, 1)  # (overwrites v: FMG's own residual, for the GS_FMG run below)
    out = subprocess.run([exe, str(conf)], capture_output=True, text=True, timeout=120, env=dict(os.environ, GS_SOLVER="pcg"))
    assert out.returncode == 0 and out.stderr == "", out.stderr
    lines = out.stdout.splitlines()
    assert lines[2] == f"Inital residual: {api[0]:.6g}"
    got = [_iter_regex().search(l) for l in lines[3:]]
    assert len(got) == 5 and all(got), out.stdout
    assert [int(m.group(1)) for m in got] == list(range(5))
    for m, want in zip(got, api[1:]):
        assert abs(float(m.group(2)) - want) <= 1e-5 * want, (m.group(0), want)
    # the V-cycle loop's norms are other numbers: the switch did something
    vc = subprocess.run([exe, str(conf)], capture_output=True, text=True, timeout=120, env=dict(os.environ, GS_SOLVER="vcycle"))
    assert vc.stdout.splitlines()[3] != lines[3] and vc.stdout.splitlines()[2] == lines[2]
    # after GS_FMG=1 PCG starts from FMG's iterate: its first norm is FMG's
    fm = subprocess.run([exe, str(conf)], capture_output=True, text=True, timeout=120,
                        env=dict(os.environ, GS_SOLVER="pcg", GS_FMG="1"))
    fl = fm.stdout.splitlines()
    m = re.match(r"fmg: cycles: 1 residual: (\S+) Took", fl[3])
    assert m and abs(float(m.group(1)) - plain) <= 1e-5 * plain, fm.stdout
    assert len([l for l in fl[4:] if _iter_regex().search(l)]) == 5
    # the library path: gs_grid_solve runs PCG, an ineligible grid fails before any work, a bad value fails the creation
    monkeypatch.setenv("GS_SOLVER", "pcg")
    with gsv.HipGridData(params) as g:
        assert gsv.HipSolver.solve(g) == api
    with gsv.HipGridData(gsv.GridParams(maxiter=2, gridDim=(15, 15, 15), preSmoothing=2, postSmoothing=1)) as g:
        before = g.field(0, "v").copy()
        with pytest.raises(gsv.GpuSolveError, match="pre = post"):
            gsv.HipSolver.solve(g)
        same(g.field(0, "v"), before, "v after a refused GS_SOLVER=pcg solve")
    with gsv.HipGridData(gsv.GridParams(maxiter=2, gridDim=(15, 15, 15), mode=gsv.GS_NONLINEAR)) as g:
        assert len(gsv.HipSolver.solve(g)) == 3  # other modes keep their solver
    monkeypatch.setenv("GS_SOLVER", "bogus")
    with pytest.raises(gsv.GpuSolveError, match="GS_SOLVER=bogus"):
        gsv.HipGridData(params)
    bad = subprocess.run([exe, str(conf)], capture_output=True, text=True, timeout=120, env=dict(os.environ, GS_SOLVER="bogus"))
    assert "GS_SOLVER=bogus" in bad.stderr and not _iter_regex().search(bad.stdout)
