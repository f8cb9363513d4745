"""Seeded sessions of mixed driver operations on ONE grid each, against tests/session_ref.py's CPU model (pinned to the
oracle by tests/test_session_ref_cpu.py): solve, vcycle, vcycle_level, jacobi, residual_norm, fmg, uploads, and weights
or the transfer mode changed in between, under drawn driver switches. What no single-operation test sees shows here: a
stale zero-iterate flag, a missing materialize, a speculative sweep adopted twice, a weight cursor off by one, a coarse
launch started on the wrong level.

After every operation the call's result (a norm or a history) and level 0's v (NEWTON: newtonV) are compared with the
model, and at the end v and f of every level the model marks specified (include/gpusolve_driver.h, gs_grid_solve).
LINEAR: fields word for word, norms within 1e-12, histories of equal length. NONLINEAR / NEWTON: fields within 1e-10 of
the field's maximum, norms within 1e-9 (tests/test_gpu_fuzz.py's bounds; the generator keeps such a session only where
its model is well conditioned and every stop decision has a margin of 1e-6, see session_ref.py).

GS_SESSIONS_N / GS_SESSIONS_SEED: a longer or different draw (the default run: session_ref.N sessions of session_ref.SEED).
The last test prints, per mode, the worst deviations seen and the slowest session."""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import gpusolve as gsv  # noqa: E402
import oracle as O  # noqa: E402
import session_ref as S  # noqa: E402
from conftest import rel  # noqa: E402

# every switch the driver reads per grid (the kernel library's own knobs are read once per process: left alone)
DRIVER_SWITCHES = S.SWITCHES + ("GS_TRANSFER", "GS_OMEGAS", "GS_FMG", "GS_NO_SWEEP3", "GS_METRICS", "GS_ZSLAB_MIN_POINTS",
                                "GS_NO_NEWTON_FUSED_UPDATE", "GS_NO_NEWTON_B", "GS_NEWTON_B_FUSED", "GS_NO_NEWTON_G",
                                "GS_NEWTON_PRO_POINTS", "GS_HALO_ORDER", "GS_SMOOTHER", "GS_COARSEN", "GS_SOLVER",
                                "GS_FMG_PROLONG")
MODES = {O.LINEAR: "LINEAR", O.NONLINEAR: "NONLINEAR", O.NEWTON: "NEWTON"}
WORST = {m: dict(field=0.0, norm=0.0, seconds=0.0, slowest="") for m in MODES}  # filled as the sessions run
SEEN = {}  # session index -> the regimes it reached


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for name in DRIVER_SWITCHES:
        monkeypatch.delenv(name, raising=False)
    assert torch.cuda.is_available(), "GPU tests need a GPU (no CPU fallback exists)"


def same(a, b, what):
    ne = np.ascontiguousarray(a).view(np.int64) != np.ascontiguousarray(b).view(np.int64)
    assert a.shape == b.shape and not ne.any(), f"{what}: {int(ne.sum())} words differ, first at {tuple(np.argwhere(ne)[0])}"


class GpuSession:
    """One HipGridData behind session_ref.Session's method names."""

    def __init__(self, case):
        p = gsv.GridParams(maxiter=case["maxiter"], tol=case["tol"], gridDim=case["dims"], mode=case["mode"],
                           preSmoothing=case["pre"], postSmoothing=case["post"], omega=case["omega"], gamma=case["gamma"],
                           stencil=gsv.Stencil(list(case["values"]), list(case["offsets"])))
        self.g = gsv.HipGridData(p, coarsen=case.get("coarsen"))  # (none: gs_grid_create, as every session here)
        self.cycle_triples = 0  # fused triples run inside solve / vcycle / vcycle_level / fmg

    def triples(self):
        return sum(gsv.driver().gs_grid_level_triples(self.g.handle, l) for l in range(self.g.numLevels()))

    def _cycling(self, f):
        before = self.triples()
        out = f()
        self.cycle_triples += self.triples() - before
        return out

    def solve(self, maxiter, tol):
        assert (maxiter, tol) == (self.g.params.maxiter, self.g.params.tol)
        solver = gsv.NewtonSolver if self.g.mode == gsv.GS_NEWTON else gsv.HipSolver
        return self._cycling(lambda: solver.solve(self.g))

    def vcycle(self):
        return self._cycling(lambda: gsv.HipSolver.vcycle(self.g))

    def vcycle_from(self, level):
        return self._cycling(lambda: gsv.HipSolver.vcycle_from(self.g, level))

    def fmg(self, k):
        return self._cycling(lambda: gsv.HipSolver.fmg(self.g, k))

    def jacobi(self, level, k):
        gsv.HipSolver.jacobi(self.g, level, k)

    def residual_norm(self, level):
        return gsv.HipSolver.compResidual(self.g, level)

    def set_weights(self, pre, post):
        self.g.set_weights(pre, post)

    def clear_weights(self):
        self.g.clear_weights()

    def set_transfer(self, mode):
        self.g.set_transfer(mode)

    def set_field(self, level, name, a):
        self.g.set_field(level, name, a)

    def field(self, level, name):
        return self.g.field(level, name)


class Compare:
    def __init__(self, case):
        self.case, self.linear = case, case["mode"] == O.LINEAR
        self.field_dev = self.norm_dev = 0.0

    def norms(self, got, want, what):
        got, want = np.atleast_1d(got), np.atleast_1d(want)
        assert len(got) == len(want), f"{what}: {list(got)} against {list(want)}"
        for a, b in zip(got, want):
            assert np.isfinite(a) and np.isfinite(b), f"{what}: {list(got)} against {list(want)}"
            self.norm_dev = max(self.norm_dev, rel(a, b))
            assert rel(a, b) < (1e-12 if self.linear else 1e-9), f"{what}: {list(got)} against {list(want)}"

    def fields(self, got, want, what):
        if self.linear:
            same(got, want, what)
            return
        assert np.isfinite(got).all(), f"{what}: non-finite values"
        scale = max(np.abs(want).max(), 1e-300)
        d = np.abs(got - want).max() / scale
        self.field_dev = max(self.field_dev, d)
        assert d <= 1e-10, f"{what}: {d} of the maximum {scale}"


def run_session(case, monkeypatch):
    """The session on a grid and on the model in lockstep, compared after every operation and at the end; returns the
    regimes it reached."""
    for name, value in case["env"].items():
        monkeypatch.setenv(name, value)
    t0 = time.perf_counter()
    model, cmp, name0 = S.new_session(case), Compare(case), S.final_name(case)
    gpu = GpuSession(case)
    with gpu.g as g:
        for k, op in enumerate(case["ops"]):
            what = f"operation {k} {op[:3]}"
            with np.errstate(all="ignore"):
                want = S.apply(model, case, op)
            got = S.apply(gpu, case, op)
            if want is not None:
                cmp.norms(got, want, what)
            cmp.fields(gpu.field(0, name0), model.field(0, name0), f"level 0's {name0} after {what}")
        for l in range(model.nl):
            for n in ("v", "f"):
                if model.specified(l, n):
                    cmp.fields(gpu.field(l, n), model.field(l, n), f"{n} of level {l} at the end")
        assert all(abs(r - 1.0) >= 1e-6 for r in model.ratios), "the generator keeps no session this close to a stop"
        nl = g.numLevels()
        assert nl == model.nl and g.fmg_start_level() == (S.start_level(case["dims"]) if case["mode"] != O.NEWTON else 0)
        reached = S.regimes(case, model.stops)
        nonaligned0 = nl > 1 and not g.level_aligned(0)
        assert nonaligned0 or not reached["position_pre3"]
        smoothed0 = any(op[0] in ("solve", "vcycle", "fmg") or (op[0] in ("vcycle_from", "jacobi") and op[1] == 0)
                        for op in case["ops"])
        reached["pairs_on_level0"] = bool(gsv.driver().gs_grid_level_fused(g.handle, 0)) and smoothed0
        reached["triple_in_a_cycle"] = gpu.cycle_triples > 0
    seconds = time.perf_counter() - t0
    w = WORST[case["mode"]]
    w["field"], w["norm"] = max(w["field"], cmp.field_dev), max(w["norm"], cmp.norm_dev)
    if seconds > w["seconds"]:
        w["seconds"], w["slowest"] = seconds, S.case_id(case)
    print(f"{S.case_id(case)}: env {case['env']} field deviation {cmp.field_dev:.3g} norm deviation {cmp.norm_dev:.3g} "
          f"{seconds:.2f} s, reached {sorted(k for k, v in reached.items() if v)}")
    SEEN[case["idx"]] = reached
    return reached


@pytest.mark.parametrize("case", S.cases(), ids=S.case_id)
def test_session(case, monkeypatch):
    run_session(case, monkeypatch)


def test_regimes_are_reached(monkeypatch):
    """Each regime the sessions exist for, judged on the grids themselves, by at least five sessions."""
    count = {}
    for case in S.cases():
        if case["idx"] not in SEEN:  # (this test selected on its own)
            with monkeypatch.context() as m:
                run_session(case, m)
        for k, v in SEEN[case["idx"]].items():
            count[k] = count.get(k, 0) + bool(v)
    print("sessions per regime:", count)
    for k in ("pairs_on_level0", "triple_in_a_cycle", "position_pre3", "weighted_early_stop", "fmg_weighted_coarse",
              "op_after_stop"):
        assert count[k] >= 5, count


# ---- hand-written sessions (the two reading findings, and every regression a drawn session has found) -----------------
def hand_case(dims, mode=O.LINEAR, pre=2, post=2, maxiter=8, tol=0.0, env=None, ops=()):
    return dict(idx=-1, attempt=0, dims=dims, mode=mode, pre=pre, post=post, omega=0.8, gamma=1.0,
                values=(6.0, -1, -1, -1, -1, -1, -1), offsets=tuple(S.CANON), env=env or {}, maxiter=maxiter, tol=tol,
                ops=tuple(ops))


def test_every_level_is_handed_back_materialised(monkeypatch):
    """gs_grid_download / gs_grid_upload copy v without looking at the level's zero-iterate flag: after a V-cycle run
    level by level (no coarse launch) every level's v must be the stored iterate, and an uploaded v must be what the
    next sweeps read."""
    case = hand_case((31, 31, 31), env={"GS_COARSE_POINTS": "0"})
    monkeypatch.setenv("GS_COARSE_POINTS", "0")
    model, gpu = S.new_session(case), GpuSession(case)
    with gpu.g:
        assert rel(gpu.vcycle(), model.vcycle()) < 1e-12
        for l in range(model.nl):
            same(gpu.field(l, "v"), model.field(l, "v"), f"v of level {l} after the V-cycle")
            same(gpu.field(l, "f"), model.field(l, "f"), f"f of level {l} after the V-cycle")
        a = S.noise(model.ld[1], 11, 1.0)
        for s in (model, gpu):
            s.set_field(1, "v", a)
            s.jacobi(1, 3)
        same(gpu.field(1, "v"), model.field(1, "v"), "level 1 after the upload and three sweeps")
        # ... and on a level whose iterate is the zero flag when the V-cycle reaches it
        for s in (model, gpu):
            s.set_field(2, "v", S.noise(model.ld[2], 12, 1.0))
            s.vcycle_from(1)
            s.jacobi(2, 1)
        for l in range(1, model.nl):
            same(gpu.field(l, "v"), model.field(l, "v"), f"v of level {l} after the V-cycle from level 1")


@pytest.mark.parametrize("transfer", ["reference", "position"])
def test_cycles_after_an_early_stop(transfer, monkeypatch):
    """46^3 smooths level 0 in pairs and the solve loop is pipelined: a solve stopped on tol after cycle 3 has the 4th
    cycle's down-leg on the levels below already and undoes the adoption of its speculative pair. Two more V-cycles
    must be the model's on every level."""
    dims = (46, 46, 46)
    probe = S.Session(dims)
    probe.set_transfer(transfer)
    h = probe.solve(8, 0.0)
    tol = (h[2] * h[3]) ** 0.5 / h[0]
    case = hand_case(dims, maxiter=8, tol=tol)
    model, gpu = S.new_session(case), GpuSession(case)
    cmp = Compare(case)
    with gpu.g as g:
        assert gsv.driver().gs_grid_level_fused(g.handle, 0) == 1
        for s in (model, gpu):
            s.set_transfer(transfer)
        want = model.solve(8, tol)
        assert len(want) == 4 and model.stops == [True] and all(abs(r - 1.0) >= 1e-6 for r in model.ratios)
        cmp.norms(gpu.solve(8, tol), want, "the stopped solve")
        same(gpu.field(0, "v"), model.field(0, "v"), "level 0 after the stopped solve")
        for k in range(2):
            cmp.norms(gpu.vcycle(), model.vcycle(), f"V-cycle {k} after the stop")
        for l in range(model.nl):
            same(gpu.field(l, "v"), model.field(l, "v"), f"v of level {l}")
            same(gpu.field(l, "f"), model.field(l, "f"), f"f of level {l}")


def test_deviation_table():
    """Not a check of its own: prints what the sessions of this run saw, per mode."""
    print("mode       worst field deviation   worst norm deviation   slowest session")
    for m, name in MODES.items():
        w = WORST[m]
        print(f"{name:<10} {w['field']:<23.3g} {w['norm']:<22.3g} {w['seconds']:.2f} s  {w['slowest']}")
