"""Seeded sessions of the driver operations added after tests/test_gpu_sessions.py's model was written — gs_grid_pcg,
gs_grid_set_smoother (ZLINE / AUTO), XY grids, gs_grid_set_fmg_prolong, gs_grid_import / gs_grid_export and refused
calls — mixed with the earlier ones on ONE grid each, against tests/session_ref.py's model (pinned to the single-feature
references by tests/test_feature_sessions_cpu.py). The adapter, the comparisons and the tolerances are
tests/test_gpu_sessions.py's: LINEAR fields word for word, norms within 1e-12; NONLINEAR / NEWTON fields within 1e-10
of the field's maximum, norms within 1e-9. After every operation the call's result and level 0's v (NEWTON: newtonV)
are compared, at the end v and f of every level the model marks specified.

pcg: the device runs first and the model replays its recorded alpha and beta, so x agrees word for word; the history
has the length of the model's free-running run (the generator's stop margin guarantees it), every recorded r.z, p.q and
r.r lies within pcg_ref.dot_bound of the replay's exactly rounded sums, hist[k + 1] is the square root of the recorded
r.r, hist[0] is held to the norm rule, and level 0's f is unchanged word for word.
load: the tensor is built from the model's noise in the drawn dtype, order and view; the side-stream half is produced
by a kernel on a second stream, loaded under it and overwritten with NaN on it straight after the call, unsynchronised.
store: into sentinel-filled storage; the image equals numpy's of the grid's own field word for word (LINEAR: and the
model's), and a strided view's words between the rows keep the sentinel.
refused: the call raises with a reason, the configuration getters read the same before and after, and the comparisons
that follow show that no field moved.

GS_FEATURE_SESSIONS_N / GS_FEATURE_SESSIONS_SEED: a longer or different draw. The last test prints the worst deviations
per mode, the slowest session and the sessions per regime."""
import copy
import math
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import gpusolve as gsv  # noqa: E402
import oracle as O  # noqa: E402
import pcg_ref as P  # noqa: E402
import session_ref as S  # noqa: E402
from test_gpu_io import expect_export, expect_import  # noqa: E402
from test_gpu_sessions import DRIVER_SWITCHES, MODES, Compare, GpuSession, same  # noqa: E402
from test_gpu_zline_lds import line_instances  # noqa: E402

WORST = {m: dict(field=0.0, norm=0.0, seconds=0.0, slowest="") for m in MODES}  # filled as the sessions run
SEEN = {}  # session index -> the regimes it reached
SENTINEL = 1.2345e30  # (exact in neither format's neighbourhood of the data: fields are far below it)
TT = {"float64": torch.float64, "float32": torch.float32}
REGIMES = ("line_then_jacobi", "jacobi_then_line", "pcg_after_stop", "cycle_after_pcg", "pcg_permuted", "xy_auto_pcg",
           "lds_instance", "non_lds_instance", "fmg_position_weighted", "load_then_rooted", "side_load", "fp32_store",
           "refused_mid")
SIDE = None


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for name in DRIVER_SWITCHES:
        monkeypatch.delenv(name, raising=False)
    assert {"GS_SMOOTHER", "GS_COARSEN", "GS_SOLVER", "GS_FMG_PROLONG"} <= set(DRIVER_SWITCHES)
    assert torch.cuda.is_available(), "GPU tests need a GPU (no CPU fallback exists)"


def side_stream():
    """The one extra stream of this file."""
    global SIDE
    if SIDE is None:
        SIDE = torch.cuda.Stream()
    return SIDE


def words64(a):
    """float32 values widened (exactly, one to one) so that test_gpu_sessions.same compares them word for word."""
    return np.ascontiguousarray(a, dtype=np.float64)


def test_the_models_io_arithmetic_is_test_gpu_ios():
    """session_ref restates expect_import / expect_export (it cannot import a GPU test module): the same words."""
    src = np.random.default_rng(5).uniform(-100.0, 100.0, (5, 4, 3))
    for dtype, npt in S.DTYPES.items():
        for scale in S.IO_SCALES:
            same(S.expect_import(src, dtype, scale), expect_import(src.astype(npt), scale), f"import {dtype} {scale}")
            same(words64(S.expect_export(src, dtype, scale)), words64(expect_export(src, scale, npt)),
                 f"export {dtype} {scale}")


class FeatureGpuSession(GpuSession):
    """GpuSession with the later operations, and the facts the regimes are judged by, read from the grid itself."""

    def __init__(self, case):
        super().__init__(case)
        self.case, self.keep, self.rec = case, [], None
        self.reached = dict.fromkeys(REGIMES, False)
        self.ran_line = self.ran_point = self.stopped = self.after_pcg = self.real_before = self.pending_refusal = False
        self.loaded = set()

    # ---- the grid's own account of its configuration
    def lines(self):
        return [self.g.level_smoother(l) == "zline" for l in range(self.g.numLevels())]

    def config(self):
        return (self.g.smoother, self.g.transfer, self.g.weights, self.g.fmg_start_level(), self.g.fmg_prolong,
                tuple(self.lines()))

    def nonaligned(self):
        return any(not self.g.level_aligned(l) for l in range(self.g.numLevels() - 1))

    # ---- regimes
    def note(self, op, result=None):
        """What operation `op`, just run, adds to the regimes (the order of tests/session_ref.py's feature_regimes)."""
        kind, r = op[0], self.reached
        if kind in ("vcycle_from", "jacobi", "residual_norm") and op[1] in self.loaded:
            r["load_then_rooted"] = True
        if kind == "load":
            if op[1] >= 1:
                self.loaded.add(op[1])
        elif kind != "set_field":
            self.loaded.clear()
        if kind in S.CYCLING:
            lines = self.lines()
            if any(lines):
                r["jacobi_then_line"] |= self.ran_point
                self.ran_line = True
                names = line_instances(self.g).values()
                r["lds_instance"] |= any("k_zline_lds" in n for n in names)
                r["non_lds_instance"] |= any("k_zline_lds" not in n for n in names)
            else:
                fused0 = gsv.driver().gs_grid_level_fused(self.g.handle, 0) == 1
                r["line_then_jacobi"] |= self.ran_line and fused0
                self.ran_point = True
            if kind != "pcg" and self.after_pcg:
                r["cycle_after_pcg"] = True
            if kind == "fmg" and self.g.fmg_prolong == "position" and self.g.weights is not None and self.nonaligned():
                r["fmg_position_weighted"] = True
            if kind == "pcg":
                w = self.g.weights
                r["pcg_after_stop"] |= self.stopped
                r["pcg_permuted"] |= w is not None and w[0] != w[1]
                r["xy_auto_pcg"] |= self.g.coarsen == "xy" and self.g.smoother == "auto" and not lines[0] and lines[-1]
                self.after_pcg = True
            if kind == "solve" and len(result) - 1 < self.case["maxiter"]:
                self.stopped = True
        if kind == "refused":
            self.pending_refusal = self.pending_refusal or self.real_before
        elif kind in S.CYCLING + ("jacobi", "residual_norm"):
            r["refused_mid"] |= self.pending_refusal
            self.real_before = True

    # ---- operations
    def pcg(self, maxiter, tol):
        assert (maxiter, tol) == (self.g.params.maxiter, self.g.params.tol)
        assert self.g.pcg_supported(), self.g.pcg_refusal
        hist = self._cycling(lambda: gsv.HipSolver.pcg(self.g))
        assert not self.g.pcg_breakdown, "the generator keeps no session whose PCG breaks down"
        self.rec = self.g.pcg_record()
        return hist

    def set_smoother(self, mode):
        self.g.set_smoother(mode)
        assert self.g.smoother == mode

    def set_fmg_prolong(self, mode):
        self.g.set_fmg_prolong(mode)
        assert self.g.fmg_prolong == mode

    def storage(self, shape, dtype, strided, fill):
        """(the tensor of `shape`, the storage it is a view of): contiguous, or rows of a larger one (pitch n + 3,
        starting at element 1)."""
        if not strided:
            t = torch.full(shape, fill, dtype=TT[dtype], device="cuda")
            return t, t
        big = torch.full(shape[:-1] + (shape[-1] + 3,), fill, dtype=TT[dtype], device="cuda")
        return big[..., 1:1 + shape[-1]], big

    def load(self, level, name, array, dtype="float64", scale=1.0, order="zyx", strided=False, side=False):
        host = np.asarray(array).astype(S.DTYPES[dtype])
        host = torch.from_numpy(np.ascontiguousarray(host.transpose(2, 1, 0) if order == "zyx" else host))
        stream = side_stream() if side else torch.cuda.current_stream()
        if side:
            stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            half = host.cuda() * 0.5
            t, big = self.storage(tuple(host.shape), dtype, strided, float("nan"))
            torch.add(half, half, out=t) if not strided else t.copy_(half + half)  # a kernel of this stream makes it
            self.g.load(name, t, level=level, scale=scale, order=order)
            big.fill_(float("nan"))  # "may be overwritten straight away": no synchronisation before the next operation
        self.reached["side_load"] |= bool(side)
        self.keep.append((big, half))

    def store(self, level, name, dtype="float64", scale=1.0, order="zyx", strided=False, side=False):
        geom = self.g.getLevel(level).geom
        n = {"x": geom.nx, "y": geom.ny, "z": geom.nz}
        shape = tuple(n[a] for a in order)
        stream = side_stream() if side else torch.cuda.current_stream()
        if side:
            stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            t, big = self.storage(shape, dtype, strided, SENTINEL)
            assert self.g.store(name, out=t, level=level, scale=scale, order=order) is t
            image = big.cpu().numpy()  # (waits for this stream only: the export is ordered before it)
        got = image[..., 1:1 + shape[-1]] if strided else image
        if strided:
            gap = np.concatenate([image[..., :1], image[..., 1 + shape[-1]:]], axis=-1)
            assert (gap == S.DTYPES[dtype](SENTINEL)).all(), "the words between the rows were written"
        got = np.ascontiguousarray(got.transpose(2, 1, 0) if order == "zyx" else got)
        # the export's own arithmetic, on the grid's own field: word for word in every mode
        own = S.expect_export(self.field(level, name)[1:-1, 1:-1, 1:-1], dtype, scale)
        same(words64(got), words64(own), f"store of level {level}'s {name} against numpy's image of the downloaded field")
        self.reached["fp32_store"] |= dtype == "float32"
        return got

    def refused(self, op):
        before = self.config()
        with pytest.raises(gsv.GpuSolveError) as e:
            if op[0] == "pcg":
                gsv.HipSolver.pcg(self.g)
            elif op[0] == "fmg":
                gsv.HipSolver.fmg(self.g, op[1])
            else:
                assert op[0] == "set_smoother"
                self.g.set_smoother(op[1])
        assert str(e.value).strip(), "a refusal carries its reason"
        assert self.config() == before, "a refused call changed the configuration"


def check_pcg(case, cmp, gpu, model, got, what):
    """The model's part of a pcg operation, after the device's: the replay of the recorded scalars."""
    free = copy.deepcopy(model)
    with np.errstate(all="ignore"):
        want_free = free.pcg(case["maxiter"], case["tol"])
        f0 = model.field(0, "f").copy()
        want = model.pcg(case["maxiter"], case["tol"], scalars=[(r["alpha"], r["beta"]) for r in gpu.rec])
    assert len(got) == len(want_free) == len(want) == len(gpu.rec) + 1, f"{what}: {got} against {want_free}"
    n = case["dims"][0] * case["dims"][1] * case["dims"][2]
    for k, (dv, rf) in enumerate(zip(gpu.rec, model.pcg_rec)):
        for key in ("rz", "pq", "rr"):
            bound = P.dot_bound(n, rf[key + "_abs"])
            assert abs(dv[key] - rf[key]) <= bound, f"{what}: iteration {k} {key}: {dv[key]!r} against {rf[key]!r}, bound {bound}"
        assert dv["flag"] == 0.0 and got[k + 1] == math.sqrt(dv["rr"]), (what, k)
    cmp.norms(got[:1], want[:1], what + " (the initial residual)")
    same(gpu.field(0, "f"), f0, f"level 0's f after {what}")
    same(model.field(0, "f"), f0, f"the model's f after {what}")


def run_session(case, monkeypatch):
    """The session on a grid and on the model in lockstep (pcg: the device first), compared after every operation and
    at the end; returns the regimes it reached."""
    for name, value in case["env"].items():
        monkeypatch.setenv(name, value)
    t0 = time.perf_counter()
    model, cmp, name0 = S.new_session(case), Compare(case), S.final_name(case)
    gpu = FeatureGpuSession(case)
    with gpu.g as g:
        assert g.coarsen == case["coarsen"] and g.numLevels() == model.nl
        for k, op in enumerate(case["ops"]):
            what = f"operation {k} {op[:3]}"
            if op[0] == "pcg":
                got = S.apply(gpu, case, op)
                check_pcg(case, cmp, gpu, model, got, what)
            else:
                with np.errstate(all="ignore"):
                    want = S.apply(model, case, op)
                got = S.apply(gpu, case, op)
                if op[0] == "store":
                    if cmp.linear:
                        same(words64(got), words64(want), what + " against the model")
                elif want is not None:
                    cmp.norms(got, want, what)
            gpu.note(op, got)
            cmp.fields(gpu.field(0, name0), model.field(0, name0), f"level 0's {name0} after {what}")
            assert g.fmg_start_level() == model.fmg_start_level(), what
        for l in range(model.nl):
            for n in ("v", "f"):
                if model.specified(l, n):
                    cmp.fields(gpu.field(l, n), model.field(l, n), f"{n} of level {l} at the end")
        assert all(abs(r - 1.0) >= 1e-6 for r in model.ratios), "the generator keeps no session this close to a stop"
        assert gpu.lines() == S.line_flags(model.smoother, model.level_values, model.offsets)
    seconds = time.perf_counter() - t0
    w = WORST[case["mode"]]
    w["field"], w["norm"] = max(w["field"], cmp.field_dev), max(w["norm"], cmp.norm_dev)
    if seconds > w["seconds"]:
        w["seconds"], w["slowest"] = seconds, S.feature_case_id(case)
    print(f"{S.feature_case_id(case)}: env {case['env']} field deviation {cmp.field_dev:.3g} norm deviation "
          f"{cmp.norm_dev:.3g} {seconds:.2f} s, reached {sorted(k for k, v in gpu.reached.items() if v)}")
    SEEN[case["idx"]] = gpu.reached
    return gpu.reached


@pytest.mark.parametrize("case", S.feature_cases(), ids=S.feature_case_id)
def test_feature_session(case, monkeypatch):
    run_session(case, monkeypatch)


def test_feature_regimes_are_reached(monkeypatch):
    """Each regime the feature sessions exist for, judged on the grids themselves, by at least five sessions."""
    count = dict.fromkeys(REGIMES, 0)
    for case in S.feature_cases():
        if case["idx"] not in SEEN:  # (this test selected on its own)
            with monkeypatch.context() as m:
                run_session(case, m)
        for k, v in SEEN[case["idx"]].items():
            count[k] += bool(v)
    print("sessions per regime:", count)
    for k in REGIMES:
        assert count[k] >= 5, count


def test_feature_deviation_table():
    """Not a check of its own: prints what the sessions of this run saw, per mode, and the sessions per regime."""
    print("mode       worst field deviation   worst norm deviation   slowest session")
    for m, name in MODES.items():
        w = WORST[m]
        print(f"{name:<10} {w['field']:<23.3g} {w['norm']:<22.3g} {w['seconds']:.2f} s  {w['slowest']}")
    print("regime                  sessions")
    for k in REGIMES:
        print(f"{k:<23} {sum(bool(r[k]) for r in SEEN.values())}")
