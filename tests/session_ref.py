"""A CPU model of one driver grid across a whole session of mixed operations, and the seeded generator of such sessions
— the reference of tests/test_session_ref_cpu.py and tests/test_gpu_sessions.py (TEST INFRASTRUCTURE ONLY; the product
never imports it).

Session holds every level's v and f (NEWTON: level 0's newtonV and the right-hand side F) and has one method per driver
operation, composed of tests/xfer_ref.py's Cycle (per-sweep weights, per-transition transfers, all three modes) and
tests/fmg_ref.py's prolongation. It also carries what the driver does NOT promise (include/gpusolve_driver.h,
gs_grid_solve), as a per-field "specified" mark:

  * after a solve that stopped on tol before its last cycle, v and f of the levels >= 1 are unspecified (the driver has
    the next cycle's down-leg on them already, or not, depending on its switches);
  * vcycle, fmg and a solve that ran all its cycles (or stopped on the last one) specify every level again;
  * vcycle_from(l) specifies the levels below l (it reads l's own v and f);
  * set_field specifies that one field;
  * NEWTON: only level 0's newtonV is specified after a solve (v and f are the inner solves' work fields).

Every stop decision the model takes (inner NEWTON solves included) that changes what is computed is recorded in
Session.ratios as norm / threshold: the generator keeps a session only if all of them are well away from 1.

cases(n, seed) draws the sessions. A draw is a pure function of (seed, index, attempt); a session is kept if its model
is finite, its stop ratios are at least 1e-6 away from 1 and (outside LINEAR mode) it is well conditioned: a second run
with level 0's f perturbed by 1e-14 relative ends within 1e-11 of the first. A rejected draw is drawn again with the
next attempt number. For the committed seed the attempt numbers are the table REDRAWS (checked against the model by
tests/test_session_ref_cpu.py), so that collecting the tests runs no model.

The later operations (tests/test_feature_sessions_cpu.py pins each to its single-feature reference; the earlier
methods behave as before for a session that uses none of them): a `coarsen` argument ("xy": semi_ref's hierarchy,
per-level stencils and transfers; set_transfer then changes nothing and fmg is refused), set_smoother (per-level line
flags by the header's rule; a line level's every smoothing step is zline_ref.sweep), set_fmg_prolong (fmg as
tests/fmg_pa_ref.py composes it), pcg (pcg_ref.Pcg with this session's own cycle as the preconditioner, free-running or
replaying a record; the levels >= 1 unspecified afterwards), load / store (gs_grid_import / gs_grid_export: interior
only) and refused (an operation refusal() says the driver refuses with nothing changed: the model does nothing).
draw_features / feature_cases are a second generator, with a seed and a redraw table of its own (FEATURE_REDRAWS), of
sessions that mix these with the earlier operations: the reference of tests/test_gpu_feature_sessions.py. draw() and
cases() are not touched by it (tests/test_feature_sessions_cpu.py holds repr(cases()) to a digest)."""
import functools
import os
import types

import numpy as np

import fmg_pa_ref
import oracle as O
import pcg_ref
import semi_ref
import weights_ref as W
import xfer_ref as X
import zline_ref
from fmg_ref import level_dims, prolong as fmg_prolong, start_level

CANON = [(0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
MAX_WEIGHTS = 8  # GS_MAX_WEIGHTS (tests/test_weights_cpu.py holds the library to >= 8)
SMOOTHERS = ("jacobi", "zline", "auto")
DTYPES = {"float64": np.float64, "float32": np.float32}


def threshold(initial, tol):
    """initial / (1 / tol) in IEEE arithmetic (tol = 0: 0), the reference's stop threshold."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.float64(initial) / (np.float64(1.0) / np.float64(tol)))


def noise(dims, seed, scale):
    """Seeded noise in [-scale, scale] on the interior of a padded array, zero ring."""
    a = np.zeros(tuple(n + 2 for n in dims))
    a[1:-1, 1:-1, 1:-1] = np.random.default_rng(seed).uniform(-scale, scale, dims)
    return a


def entries(stencil):
    """(values, offsets) of an oracle.Stencil (None: the default one)."""
    st = stencil or O.Stencil.make()
    return tuple(float(x) for x in st.s), [(int(st.ox[i]), int(st.oy[i]), int(st.oz[i])) for i in range(7)]


def hierarchy(dims, coarsen, values, offsets):
    """(level dims, one tuple of stencil values per level): fmg_ref's halving with the configuration's stencil on every
    level, or semi_ref's XY hierarchy with semi_ref.level_stencil's."""
    if coarsen == "xyz":
        ld = level_dims(dims)
        return ld, [tuple(values)] * len(ld)
    assert coarsen == "xy"
    ld = semi_ref.level_dims(dims)
    h = [1.0 / (d[1] + 1) for d in ld]
    return ld, [semi_ref.level_stencil(values, h[0], hl, offsets) for hl in h]


def line_flags(smoother, level_values, offsets):
    """include/gpusolve_driver.h's rule: JACOBI no level, ZLINE every level, AUTO per level by the level's own stencil."""
    assert smoother in SMOOTHERS
    if smoother == "auto":
        return [bool(z) for z in semi_ref.auto_flags(level_values, offsets)]
    return [smoother == "zline"] * len(level_values)


def refusal(cfg, kind, *args):
    """Why include/gpusolve_driver.h has the driver refuse operation `kind` "with nothing changed" on a grid configured
    as cfg (a Session, or the generator's plan: mode, coarsen, ld, npre, npost, weights, transfer, fmg_prolong, values,
    level_values, offsets), or None where it runs. The one statement of these rules: the model's operations assert
    None, Session.refused asserts a reason, and the generator draws by it."""
    xy = cfg.coarsen == "xy"
    nonaligned = [l for l in range(len(cfg.ld) - 1) if not X.aligned(cfg.ld[l], cfg.ld[l + 1])]
    if kind == "fmg":
        if cfg.mode == O.NEWTON:
            return "FMG: not in NEWTON mode"
        if xy:
            return "FMG: not on an XY grid"
        if args and args[0] < 1:
            return "FMG: cycles per level < 1"
        if cfg.fmg_prolong == "position":
            if cfg.transfer == "reference" and nonaligned:
                return "FMG by position over a non-aligned transition needs the POSITION transfers"
            return None if len(cfg.ld) > 1 else "FMG: one level"
        return "FMG: the coarse grids do not align" if nonaligned[:1] == [0] or len(cfg.ld) == 1 else None
    if kind == "pcg":
        if cfg.mode != O.LINEAR:
            return "PCG: LINEAR grids only"
        if cfg.npre != cfg.npost or cfg.npre == 0:
            return "PCG: pre = post >= 1"
        if cfg.weights and sorted(cfg.weights[0]) != sorted(cfg.weights[1]):
            return "PCG: the post weights must be a permutation of the pre weights"
        w = {}
        for v, o in zip(cfg.values, cfg.offsets):
            w[tuple(o)] = w.get(tuple(o), 0.0) + v
        if any(w.get(tuple(-a for a in o), 0.0) != v for o, v in w.items()):
            return "PCG: the stencil must be symmetric"
        if cfg.transfer == "reference" and not xy and nonaligned:
            return "PCG: a non-aligned transition needs the POSITION transfers"
        return None
    if kind == "set_smoother":
        if args[0] == "jacobi":
            return None
        if cfg.mode != O.LINEAR:
            return "smoother: line sweeps need a LINEAR grid"
        if args[0] == "zline" and not zline_ref.supported(cfg.values, cfg.offsets):
            return "smoother: ZLINE refuses the stencil"
        for lv, z in zip(cfg.level_values, line_flags(args[0], cfg.level_values, cfg.offsets)):
            if z and not zline_ref.supported(lv, cfg.offsets):
                return "smoother: a line level's stencil is refused"
        return None
    raise AssertionError(f"no refusal rule for {kind}")


def fmg_start(cfg):
    """gs_grid_fmg_start_level: 0 where FMG never applies, the coarsest level under POSITION, else fmg_ref's."""
    if cfg.mode == O.NEWTON or cfg.coarsen == "xy":
        return 0
    return len(cfg.ld) - 1 if cfg.fmg_prolong == "position" else start_level(cfg.dims)


def expect_import(src, dtype, scale):
    """tests/test_gpu_io.py's expect_import of the tensor dtype(src): one conversion, at most one multiply."""
    d = np.asarray(src).astype(DTYPES[dtype]).astype(np.float64)
    return d if scale == 1.0 else np.float64(scale) * d


def expect_export(f, dtype, scale):
    """tests/test_gpu_io.py's expect_export."""
    p = f if scale == 1.0 else np.float64(scale) * f
    return p.astype(DTYPES[dtype])


class SessionCycle(X.Cycle):
    """xfer_ref.Cycle with what a session may change: one stencil and one smoother flag per level (a line level runs
    zline_ref.sweep, the others the oracle's Jacobi) and, on an XY grid, semi_ref's hierarchy and transfers. On an XYZ
    grid with no line level it is xfer_ref.Cycle call for call."""

    def __init__(self, dims, mode, pre, post, gamma, transfer, stencil, coarsen="xyz", f0=None):
        super().__init__(dims, mode, pre, post, gamma, f0=f0, transfer=transfer, stencil=stencil)
        self.coarsen = coarsen
        values, self.offsets = entries(stencil)
        if coarsen == "xy":
            assert mode == O.LINEAR and zline_ref.shape_of(values, self.offsets) is not None and min(dims[:2]) >= 2
            self.ld, self.values = hierarchy(dims, "xy", values, self.offsets)
            self.h = [1.0 / (d[1] + 1) for d in self.ld]
            self.stencils = [O.Stencil.make(v, self.offsets) for v in self.values]
            self.f, self.v = self.f[:1], self.v[:1]
            for d in self.ld[1:]:
                self.f.append(O.zeros(*d))
                self.v.append(O.zeros(*d))
        else:
            self.values = [values] * len(self.ld)
            self.stencils = [stencil] * len(self.ld)
        self.line = [False] * len(self.ld)

    def R(self, l, a):
        return semi_ref.restrict_xy(a, self.ld[l]) if self.coarsen == "xy" else super().R(l, a)

    def P(self, l, c):
        return semi_ref.prolong_xy(c, self.ld[l]) if self.coarsen == "xy" else super().P(l, c)

    def _smooth(self, l, weights):
        for om in weights:
            if self.line[l]:
                self.v[l] = zline_ref.sweep(self.v[l], self.f[l], self.h[l], om, self.values[l], self.offsets)
            else:
                self.v[l] = O.jacobi(self.v[l], self.f[l], self.h[l], mode=self.mode, omega=float(om), gamma=self.gamma,
                                     sweeps=1, w=self._w(l), stencil=self.stencils[l])

    def residual(self, l=0):
        return O.residual(self.v[l], self.f[l], self.h[l], self.mode, self.gamma, w=self._w(l), stencil=self.stencils[l])


class Session:
    def __init__(self, dims, mode=O.LINEAR, pre=2, post=2, omega=0.8, gamma=1.0, stencil=None, coarsen="xyz"):
        self.dims, self.mode, self.npre, self.npost = tuple(int(d) for d in dims), mode, int(pre), int(post)
        self.omega, self.gamma, self.stencil = float(omega), float(gamma), stencil
        self.weights, self.transfer = None, "reference"
        self.coarsen, self.smoother, self.fmg_prolong = coarsen, "jacobi", "aligned"
        self.c = SessionCycle(self.dims, mode, [self.omega] * self.npre, [self.omega] * self.npost, self.gamma,
                              self.transfer, stencil, coarsen)
        self.ld = self.c.ld
        self.nl = len(self.ld)
        self.values, self.offsets, self.level_values = self.c.values[0], self.c.offsets, self.c.values
        self.spec = {(n, l): True for n in ("v", "f") for l in range(self.nl)}
        self.ratios = []
        self.stops = []  # one entry per solve and pcg (outer loops only): True if it stopped on tol before its last cycle
        self.breakdowns = 0  # free-running pcg runs that ended on a breakdown (the generator keeps no such session)
        if mode == O.NEWTON:
            self.newtonV = O.zeros(*self.ld[0])
            self.spec[("newtonV", 0)] = True

    # ---- configuration
    def set_weights(self, pre, post):
        assert len(pre) == self.npre and len(post) == self.npost and max(len(pre), len(post)) <= MAX_WEIGHTS
        self.weights = ([float(w) for w in pre], [float(w) for w in post])

    def clear_weights(self):
        self.weights = None

    def set_transfer(self, mode):
        """(On an XY grid the mode is kept and read back, and changes nothing: SessionCycle's transfers are semi_ref's.)"""
        assert mode in ("reference", "position")
        self.transfer = mode

    def set_smoother(self, mode):
        """Changes no field and no mark: the line flags every later smoothing step goes by."""
        assert refusal(self, "set_smoother", mode) is None
        self.smoother = mode

    def set_fmg_prolong(self, mode):
        assert mode in ("aligned", "position")
        self.fmg_prolong = mode

    def fmg_start_level(self):
        return fmg_start(self)

    def _sweeps(self):
        return self.weights if self.weights else ([self.omega] * self.npre, [self.omega] * self.npost)

    def _cfg(self):
        c = self.c
        c.pre, c.post = self._sweeps()
        c.transfer = self.transfer
        c.line = line_flags(self.smoother, self.level_values, self.offsets)
        return c

    def refused(self, op):
        """An operation the header has the driver refuse with nothing changed: the model does nothing."""
        kind, args = op[0], op[1:]
        assert refusal(self, kind, *args) is not None, f"{op} is not refused here"

    # ---- fields
    def set_field(self, level, name, a):
        a = np.ascontiguousarray(a, dtype=np.float64).copy()
        assert a.shape == tuple(n + 2 for n in self.ld[level])
        if name == "newtonV":
            assert self.mode == O.NEWTON and level == 0
            self.newtonV = a
        else:
            getattr(self.c, name)[level] = a
        self.spec[(name, level)] = True

    def load(self, level, name, array, dtype="float64", scale=1.0, **how):
        """gs_grid_import of the tensor dtype(array) (the level's interior, [x][y][z]): the interior becomes
        scale * float64(tensor), the ring keeps its values, the field is specified. `how` (the tensor's order, view and
        stream) changes nothing that is computed."""
        assert name != "newtonV" or (self.mode == O.NEWTON and level == 0)
        a = self.field(level, name).copy()
        assert np.shape(array) == tuple(self.ld[level])
        a[1:-1, 1:-1, 1:-1] = expect_import(array, dtype, scale)
        self.set_field(level, name, a)

    def store(self, level, name, dtype="float64", scale=1.0, **how):
        """gs_grid_export: dtype(scale * the interior), [x][y][z]."""
        assert self.specified(level, name)
        return expect_export(self.field(level, name)[1:-1, 1:-1, 1:-1], dtype, scale)

    def field(self, level, name):
        return self.newtonV if name == "newtonV" else getattr(self.c, name)[level]

    def specified(self, level, name):
        return self.spec.get((name, level), False)

    def _reads(self, level):
        assert self.spec[("v", level)] and self.spec[("f", level)], f"level {level} is unspecified here"

    def _mark(self, levels, value):
        for l in levels:
            self.spec[("v", l)] = self.spec[("f", l)] = value

    def _decide(self, norm, thr, matters):
        stop = norm <= thr
        if matters:
            self.ratios.append(norm / thr if thr > 0 else (1.0 if stop else np.inf))
        return stop

    # ---- operations
    def vcycle(self):
        assert self.mode != O.NEWTON
        self._reads(0)
        res = self._cfg().vcycle()
        self._mark(range(self.nl), True)
        return res

    def vcycle_from(self, level):
        assert self.mode != O.NEWTON
        self._reads(level)
        self._cfg().vcycle_from(level)
        self._mark(range(level + 1, self.nl), True)

    def jacobi(self, level, k):
        """k stand-alone sweeps with the grid's omega (never the weights)."""
        assert self.mode != O.NEWTON
        self._reads(level)
        c = self._cfg()
        if c.line[level]:
            c._smooth(level, [self.omega] * k)
            return
        c.v[level] = W.sweeps(c.v[level], c.f[level], c.h[level], self.mode, [self.omega] * k, self.gamma,
                              c.stencils[level])

    def residual_norm(self, level):
        assert self.mode != O.NEWTON
        self._reads(level)
        return self.c.residual(level)[1]

    def fmg(self, k):
        """ALIGNED: from fmg_ref's start level, every transition above it aligned. POSITION: from the coarsest level,
        as tests/fmg_pa_ref.py's fmg() composes it (a non-aligned transition takes its prolong, and Cycle.R's
        restriction by position)."""
        s = fmg_start(self)
        assert refusal(self, "fmg", k) is None and s > 0 and self.mode != O.NEWTON and k >= 1
        assert self.spec[("f", 0)]
        c = self._cfg()
        for l in range(s):
            c.f[l + 1] = c.R(l, c.f[l])
        for l in range(s, -1, -1):
            v0 = O.zeros(*self.ld[l])
            if l < s:
                fine = fmg_prolong(c.v[l + 1]) if X.aligned(self.ld[l], self.ld[l + 1]) else \
                    fmg_pa_ref.prolong(c.v[l + 1], self.ld[l])
                v0[1:-1, 1:-1, 1:-1] = fine[1:-1, 1:-1, 1:-1]
            c.v[l] = v0
            for _ in range(k):
                c.vcycle_from(l)
        self._mark(range(self.nl), True)
        return c.residual(0)[1]

    def solve(self, maxiter, tol):
        if self.mode == O.NEWTON:
            return self._newton(maxiter, tol)
        self._reads(0)
        c = self._cfg()
        hist = [c.residual(0)[1]]
        thr = threshold(hist[0], tol)
        early = False
        for i in range(maxiter):
            hist.append(c.vcycle())
            last = i + 1 == maxiter  # (the last norm decides nothing: the loop ends either way)
            if self._decide(hist[-1], thr, not last):
                early = not last
                break
        self.stops.append(early)
        if maxiter > 0:
            self._mark(range(self.nl), True)
        if early:
            self._mark(range(1, self.nl), False)
        return hist

    def pcg(self, maxiter, tol, scalars=None):
        """gs_grid_pcg: x0 = level 0's v as it stands, the preconditioner this session's own cycle (weights, transfers,
        smoother, coarsening) from a zero iterate. scalars None: free-running (pcg_ref.Pcg.run, its own alpha and
        beta). scalars = [(alpha_k, beta_k), ...]: the replay of a record (every field through the device's roundings);
        the record must be as long as the stop rule makes the replay's own norms. Returns the history; self.pcg_rec is
        pcg_ref's per-iteration record (exactly rounded sums). Level 0's v = x of the last complete iteration, its f
        untouched, v and f of the levels >= 1 unspecified."""
        assert refusal(self, "pcg") is None and maxiter >= 1
        self._reads(0)
        c = self._cfg()
        pre, post = self._sweeps()
        line = list(c.line)

        def cycle(r):
            k = SessionCycle(self.dims, O.LINEAR, pre, post, self.gamma, self.transfer, self.stencil, self.coarsen, f0=r)
            k.line = line
            return k

        p = pcg_ref.Pcg(self.dims, c.f[0], x0=c.v[0], stencil=self.stencil, cycle=cycle)
        if scalars is None:
            hist, rec = p.run(maxiter, tol)
        else:
            assert 1 <= len(scalars) <= maxiter
            hist, rec = p.replay(scalars)
        thr = threshold(hist[0], tol)
        early = False
        for k in range(len(hist) - 1):
            last = k + 1 == maxiter
            if self._decide(hist[k + 1], thr, not last):
                early = not last
                assert k + 2 == len(hist), "the record goes on past the iteration the stop rule ends on"
                break
        if not early and len(hist) - 1 < maxiter:
            assert scalars is None, "the record ends before the stop rule does"
            self.breakdowns += 1
        c.v[0] = p.x
        self.pcg_rec = rec
        self.stops.append(early)
        self._mark(range(1, self.nl), False)
        return hist

    def _newton(self, maxiter, tol):
        """NewtonSolver::solve, as xfer_ref.newton_solve: F is level 0's f as the grid was created with."""
        assert self.spec[("newtonV", 0)] and self.spec[("f", 0)] and not self.stops, "one NEWTON solve per session"
        h0 = 1.0 / (self.ld[0][1] + 1)
        F = self.c.f[0]
        pre, post = self.weights if self.weights else ([self.omega] * self.npre, [self.omega] * self.npost)
        w = [O.zeros(*d) for d in self.ld]
        w[0] = self.newtonV
        f0, r0 = O.newton_F(w[0], F, h0, self.gamma, self.stencil)
        hist = [r0]
        thr = threshold(r0, tol)
        early = False
        for i in range(maxiter):
            c = X.Cycle(self.dims, O.NEWTON, pre, post, self.gamma, f0=f0, transfer=self.transfer, w=w,
                        stencil=self.stencil)
            for l in range(1, self.nl - 1):  # the coarsest level keeps its newtonV
                w[l] = c.R(l - 1, w[l - 1])
            ithr = threshold(c.residual(0)[1], 0.1)
            for j in range(10):
                if self._decide(c.vcycle(), ithr, j < 9):
                    break
            w[0] = w[0] + c.v[0]
            f0, res = O.newton_F(w[0], F, h0, self.gamma, self.stencil)
            hist.append(res)
            last = i + 1 == maxiter
            if self._decide(res, thr, not last):
                early = not last
                break
        self.newtonV = w[0]
        self.stops.append(early)
        self._mark(range(self.nl), False)
        return hist


# ---- the generator ----------------------------------------------------------------------------------------------------
SEED = 20261022
N = 120
# (shape, weight of its draw): each schedule regime at its smallest size (tests/test_gpu_sessions.py asserts that they are
# reached); the shapes that reach the rarer regimes (FMG, triples, pairs over a non-aligned transition) are drawn more often
POOL = [((46, 46, 46), 0.12), ((48, 50, 46), 0.07), ((63, 63, 63), 0.15), ((64, 64, 64), 0.17), ((130, 20, 18), 0.06),
        ((31, 31, 31), 0.13), ((33, 31, 29), 0.05), ((40, 32, 24), 0.06), ((17, 9, 12), 0.05), ((12, 10, 8), 0.05),
        ((6, 5, 4), 0.05), ((3, 2, 9), 0.04)]
NEWTON_MAX_POINTS = 48 * 50 * 46  # a NEWTON session is up to 20 inner V-cycles: not on the two largest cubes
SWITCHES = ("GS_COARSE_POINTS", "GS_TILE_POINTS", "GS_SWEEP3_MIN_POINTS", "GS_NO_SPECULATION", "GS_NO_PIPELINE",
            "GS_NO_ZERO_GUESS", "GS_NO_FUSED_RR", "GS_NO_FUSED_PROLONG", "GS_NO_FUSED_SWEEPS")
# attempt numbers of the committed seed's redrawn sessions (index: attempt); every other session is attempt 0
REDRAWS = {}


def _weights(rng, n, mode):
    if n and mode == O.LINEAR and rng.uniform() < 0.3:  # the Chebyshev weights' closed form on [1/3, 2]
        return [float(1.0 / (7.0 / 6.0 + 5.0 / 6.0 * np.cos(np.pi * (2 * k - 1) / (2.0 * n)))) for k in range(1, n + 1)]
    hi = 1.3 if mode == O.LINEAR else 0.95
    return [float(np.round(rng.uniform(0.4 if mode == O.LINEAR else 0.5, hi), 3)) for _ in range(n)]


def draw(seed, idx, attempt=0):
    """One session's configuration and operations: a pure function of its arguments (no model is run)."""
    rng = np.random.default_rng([int(seed), int(idx), int(attempt)])
    u = rng.uniform()
    mode = O.LINEAR if u < 0.60 else (O.NONLINEAR if u < 0.85 else O.NEWTON)
    shapes, p = [s for s, _ in POOL], np.array([w for _, w in POOL])
    if mode == O.NEWTON:
        p = np.where([s[0] * s[1] * s[2] <= NEWTON_MAX_POINTS for s in shapes], p, 0.0)
    dims = shapes[int(rng.choice(len(shapes), p=p / p.sum()))]
    env = {}
    if rng.uniform() < 0.65:
        env["GS_COARSE_POINTS"] = str(int(rng.choice([0, 8, 4096])))
    for name, value, share in (("GS_TILE_POINTS", "0", 0.25), ("GS_SWEEP3_MIN_POINTS", "1", 0.5),
                               ("GS_NO_SPECULATION", "1", 0.2), ("GS_NO_PIPELINE", "1", 0.2),
                               ("GS_NO_ZERO_GUESS", "1", 0.2), ("GS_NO_FUSED_RR", "1", 0.2),
                               ("GS_NO_FUSED_PROLONG", "1", 0.2), ("GS_NO_FUSED_SWEEPS", "1", 0.15)):
        if rng.uniform() < share:
            env[name] = value
    # pre = 2 and 1 more often than the rest of 0..6: only there do the tiled down-leg step (pre = 2) and the pipelined
    # solve loop (every pre-smoothing sweep speculative: 2 on a level of pairs, else 1) run at all
    u = rng.uniform()
    pre, post = 2 if u < 0.25 else (1 if u < 0.35 else int(rng.integers(0, 7))), int(rng.integers(0, 7))
    if mode == O.LINEAR and "GS_SWEEP3_MIN_POINTS" in env and rng.uniform() < 0.7:
        # where triples are switched on, mostly the sweep counts that split into them (3: T, 5: T P, 6: T T), and
        # mostly those in which sweeps follow a triple (the weight cursor moves on past it)
        pre, post = (int(rng.choice([3, 5, 5, 6, 6])) for _ in range(2))
    if pre + post == 0:
        post = 1
    omega = float(np.round(rng.uniform(0.5, 0.95), 3))
    gamma = float(np.round(rng.uniform(0.0, 1.5), 3)) if mode else 1.0
    values, offsets = [6.0, -1, -1, -1, -1, -1, -1], list(CANON)
    u = rng.uniform()
    if u < 0.2:
        values = [float(np.round(6 + rng.uniform(0, 2), 2))] + [float(np.round(-rng.uniform(0.8, 1.2), 2)) for _ in range(6)]
    if u < 0.1:
        perm = [0] + [int(j) for j in 1 + rng.permutation(6)]
        values, offsets = [values[j] for j in perm], [offsets[j] for j in perm]
    ld = level_dims(dims)
    nl, fmg_ok = len(ld), mode != O.NEWTON and start_level(dims) > 0
    case = dict(idx=int(idx), attempt=int(attempt), dims=dims, mode=mode, pre=pre, post=post, omega=omega, gamma=gamma,
                values=tuple(values), offsets=tuple(offsets), env=env)
    ops = []
    fseed = [1000 * int(idx) + 17]

    def upload(level, name, scale):
        fseed[0] += 1
        ops.append(("set_field", int(level), name, fseed[0], scale))

    def feature():
        k = rng.uniform()
        if k < 0.45:
            ops.append(("set_weights", tuple(_weights(rng, pre, mode)), tuple(_weights(rng, post, mode))))
        elif k < 0.55:
            ops.append(("clear_weights",))
        else:
            ops.append(("set_transfer", "position" if rng.uniform() < 0.65 else "reference"))

    if mode == O.NEWTON:
        case["maxiter"], case["tol"] = int(rng.integers(1, 3)), 0.0
        if rng.uniform() < 0.5:
            ops.append(("set_weights", tuple(_weights(rng, pre, mode)), tuple(_weights(rng, post, mode))))
        if rng.uniform() < 0.5:
            ops.append(("set_transfer", "position"))
        if rng.uniform() < 0.5:
            upload(0, "newtonV", 0.1)
        ops.append(("solve",))
        case["ops"] = tuple(ops)
        return case
    linear = mode == O.LINEAR
    case["maxiter"] = int(rng.integers(2, 6)) if linear else int(rng.integers(1, 3))
    case["tol"] = 0.0 if rng.uniform() < 0.3 else float(np.round(10.0 ** -rng.uniform(0.2, 2.0), 6))
    budget = 10 ** 9 if linear else 4  # V-cycles a non-LINEAR session may still run (fmg(k): k + 1)
    # planned marks, on the safe side: any solve with a tol may leave the levels >= 1 unspecified
    spec = [True] * nl
    if rng.uniform() < 0.5:
        ops.append(("set_weights", tuple(_weights(rng, pre, mode)), tuple(_weights(rng, post, mode))))
    if rng.uniform() < 0.5:
        ops.append(("set_transfer", "position"))
    for _ in range(int(rng.integers(3, 7))):
        kinds = {"solve": 0.3, "vcycle": 0.2, "vcycle_from": 0.12, "fmg": 0.3 if fmg_ok else 0.0, "jacobi": 0.1,
                 "residual_norm": 0.06, "set_field": 0.06, "feature": 0.16}
        cost = {"solve": case["maxiter"], "vcycle": 1, "vcycle_from": 1, "fmg": 2}
        kinds = {k: w for k, w in kinds.items() if cost.get(k, 0) <= budget}
        names, pk = list(kinds), np.array(list(kinds.values()))
        kind = names[int(rng.choice(len(names), p=pk / pk.sum()))]
        budget -= cost.get(kind, 0)
        if kind == "feature":
            feature()
        elif kind == "set_field":
            upload(0, "v", 1.0)
        elif kind == "solve":
            ops.append(("solve",))
            spec = [True] * nl if case["tol"] == 0.0 else [True] + [False] * (nl - 1)
        elif kind == "vcycle":
            ops.append(("vcycle",))
            spec = [True] * nl
        elif kind == "fmg":
            if rng.uniform() < 0.3:
                upload(0, "f", 100.0)
            ops.append(("fmg", 1))
            spec = [True] * nl
        else:  # an operation rooted at a level of its own: its v and f uploaded first, always where unspecified
            level = int(rng.integers(0, nl))
            if not spec[level] or (level > 0 and rng.uniform() < 0.5):
                upload(level, "v", 1.0)
                upload(level, "f", 100.0)
                spec[level] = True
            if kind == "vcycle_from":
                ops.append(("vcycle_from", level))
                spec[level + 1:] = [True] * (nl - level - 1)
            elif kind == "jacobi":
                ops.append(("jacobi", level, int(rng.integers(1, 9))))
            else:
                ops.append(("residual_norm", level))
    if not any(op[0] in ("solve", "vcycle", "vcycle_from", "fmg", "jacobi", "residual_norm") for op in ops):
        ops.append(("vcycle",))  # (only switches and uploads were drawn)
    case["ops"] = tuple(ops)
    return case


def stencil_of(case):
    return O.Stencil.make(case["values"], case["offsets"])


def new_session(case):
    return Session(case["dims"], case["mode"], case["pre"], case["post"], case["omega"], case["gamma"], stencil_of(case),
                   case.get("coarsen", "xyz"))


def apply(target, case, op):
    """One operation of a case on `target` (a Session, or the GPU test's adapter with the same methods): its result."""
    kind = op[0]
    if kind == "solve":
        return target.solve(case["maxiter"], case["tol"])
    if kind == "pcg":
        return target.pcg(case["maxiter"], case["tol"])
    if kind == "load":
        _, level, name, seed, amp, dtype, scale, order, strided, side = op
        dims = hierarchy(case["dims"], case.get("coarsen", "xyz"), case["values"], case["offsets"])[0][level]
        return target.load(level, name, noise(dims, seed, amp)[1:-1, 1:-1, 1:-1], dtype, scale, order=order,
                           strided=strided, side=side)
    if kind == "store":
        _, level, name, dtype, scale, order, strided, side = op
        return target.store(level, name, dtype, scale, order=order, strided=strided, side=side)
    if kind == "refused":
        return target.refused(op[1])
    if kind == "set_field":
        _, level, name, seed, scale = op
        ld = semi_ref.level_dims(case["dims"]) if case.get("coarsen") == "xy" else level_dims(case["dims"])
        return target.set_field(level, name, noise(ld[level], seed, scale))
    if kind == "set_weights":
        return target.set_weights(list(op[1]), list(op[2]))
    return getattr(target, kind)(*op[1:])


def final_name(case):
    return "newtonV" if case["mode"] == O.NEWTON else "v"


def run_model(case, perturb=None):
    """The whole session on the model: (session, [result of every operation]). perturb: a seed; level 0's f is
    multiplied pointwise by 1 + 1e-14 u, u in [-1, 1], before the first operation (the conditioning check)."""
    s = new_session(case)
    if perturb is not None:
        u = np.random.default_rng(perturb).uniform(-1.0, 1.0, s.c.f[0].shape)
        s.c.f[0] = s.c.f[0] * (1.0 + 1e-14 * u)
    with np.errstate(all="ignore"):
        results = [apply(s, case, op) for op in case["ops"]]
    return s, results


def _finite(s, results):
    vals = [np.asarray(r, dtype=np.float64).ravel() for r in results if r is not None]
    fields = [s.field(0, "newtonV")] if s.mode == O.NEWTON else [a for n in ("v", "f") for a in getattr(s.c, n)]
    return all(np.isfinite(a).all() for a in vals + fields)


def accept(case):
    """(kept, reason, session, results) of one draw's model run."""
    s, results = run_model(case)
    if not _finite(s, results):
        return False, "non-finite", s, results
    if any(not np.isfinite(r) and r != np.inf or abs(r - 1.0) < 1e-6 for r in s.ratios):
        return False, "stop margin", s, results
    if s.breakdowns:
        return False, "pcg breakdown", s, results
    if case["mode"] != O.LINEAR:
        s2, _ = run_model(case, perturb=case["idx"] + 1)
        a, b = s.field(0, final_name(case)), s2.field(0, final_name(case))
        if not np.isfinite(b).all() or np.abs(a - b).max() > 1e-11 * max(np.abs(a).max(), 1e-300):
            return False, "conditioning", s, results
    return True, "", s, results


@functools.lru_cache(maxsize=None)
def resolve(seed, idx):
    """The first accepted attempt of session idx, by running the model: (case, rejected reasons, which of its solves
    stopped on tol before their last cycle)."""
    reasons = []
    for attempt in range(20):
        case = draw(seed, idx, attempt)
        ok, why, s, _ = accept(case)
        if ok:
            return case, tuple(reasons), tuple(s.stops)
        reasons.append(why)
    raise AssertionError(f"session {idx} of seed {seed}: 20 draws rejected {reasons}")


def cases(n=None, seed=None):
    """The sessions of a seed. GS_SESSIONS_N / GS_SESSIONS_SEED: a longer or different draw (any seed but the committed
    one runs the model to find the accepted attempts)."""
    n = int(os.environ.get("GS_SESSIONS_N", N)) if n is None else n
    seed = int(os.environ.get("GS_SESSIONS_SEED", SEED)) if seed is None else seed
    if seed == SEED and n <= N:
        return [draw(seed, i, REDRAWS.get(i, 0)) for i in range(n)]
    return [resolve(seed, i)[0] for i in range(n)]


def regimes(case, stops):
    """What a session reaches that the driver's switches cannot take away, from its draw and its solves' stops (one flag
    per solve, Session.stops): weights through an early-stopped solve; an operation (not a mere switch) after a
    tol-stopped solve; POSITION mode over a non-aligned level-0 transition with pre >= 3 in a cycle from level 0; fmg
    with weights under a moved GS_COARSE_POINTS."""
    ld = level_dims(case["dims"])
    nonaligned0 = len(ld) > 1 and not X.aligned(ld[0], ld[1])
    out = dict(weighted_early_stop=False, op_after_stop=False, position_pre3=False, fmg_weighted_coarse=False)
    weighted, transfer, stopped, k = False, "reference", False, 0
    for op in case["ops"]:
        kind = op[0]
        if stopped and kind not in ("set_weights", "clear_weights", "set_transfer"):
            out["op_after_stop"] = True
        if kind == "set_weights":
            weighted = True
        elif kind == "clear_weights":
            weighted = False
        elif kind == "set_transfer":
            transfer = op[1]
        elif kind == "solve":
            if stops[k]:
                stopped = True
                out["weighted_early_stop"] |= weighted
            k += 1
        if (kind in ("solve", "vcycle") or (kind == "vcycle_from" and op[1] == 0)) and transfer == "position" \
                and nonaligned0 and case["pre"] >= 3:
            out["position_pre3"] = True
        if kind == "fmg" and weighted and "GS_COARSE_POINTS" in case["env"]:
            out["fmg_weighted_coarse"] = True
    return out


def case_id(c):
    kinds = {"solve": "S", "vcycle": "V", "vcycle_from": "R", "fmg": "F", "jacobi": "J", "residual_norm": "N",
             "set_field": "u", "set_weights": "w", "clear_weights": "c", "set_transfer": "t"}
    return (f"s{c['idx']}-{'x'.join(map(str, c['dims']))}-m{c['mode']}-{c['pre']}+{c['post']}-"
            + "".join(kinds[op[0]] for op in c["ops"]))


# ---- the second generator: sessions of the operations added since (PCG, smoothers, XY grids, FMG by position, I/O) -------
FEATURE_SEED = 20261104
FEATURE_N = 96
UPLO_ORDER = (0, 5, 2, 6, 4, 1, 3)  # a permuted entry order with the centre first (the oracle's Jacobi divides by entry 0)
FAMILIES = {"ISO": (zline_ref.ISO, tuple(CANON)), "STRONGZ": (zline_ref.STRONGZ, tuple(CANON)),
            "UPLO": tuple(tuple(x) for x in zline_ref.permuted(zline_ref.UPLO, UPLO_ORDER)),
            "WEAKZ": (zline_ref.WEAKZ, tuple(CANON))}
FAMILY_SHARES = (0.22, 0.28, 0.12, 0.38)
# the smallest shapes that reach every line instance (marching, LDS, neither: nz < 64) and every schedule regime
XY_POOL = [((64, 64, 64), 0.22), ((33, 31, 70), 0.2), ((31, 31, 64), 0.2), ((16, 12, 70), 0.15), ((40, 32, 24), 0.13),
           ((6, 5, 4), 0.1)]
XYZ_POOL = [((46, 46, 130), 0.2), ((15, 15, 127), 0.12), ((63, 63, 63), 0.12), ((64, 64, 64), 0.16), ((46, 46, 46), 0.18),
            ((17, 9, 12), 0.14), ((3, 2, 9), 0.08)]
IO_SCALES = (1.0, -0.375, 0.5)
CYCLING = ("solve", "vcycle", "vcycle_from", "fmg", "pcg")
# attempt numbers of the committed feature seed's redrawn sessions (index: attempt); every other session is attempt 0
FEATURE_REDRAWS = {34: 1, 91: 1}


def draw_features(seed, idx, attempt=0):
    """One feature session's configuration and operations: a pure function of its arguments (no model is run). The
    eligibility of fmg, pcg and set_smoother at each point is refusal()'s on the planned configuration: an operation
    the driver refuses there is drawn as ("refused", operation)."""
    rng = np.random.default_rng([int(seed), int(idx), int(attempt)])
    u = rng.uniform()
    mode = O.LINEAR if u < 0.80 else (O.NONLINEAR if u < 0.91 else O.NEWTON)
    linear = mode == O.LINEAR
    family = list(FAMILIES)[int(rng.choice(len(FAMILIES), p=FAMILY_SHARES))]
    values, offsets = FAMILIES[family]
    coarsen = "xy" if linear and rng.uniform() < 0.5 else "xyz"
    pool = XY_POOL if coarsen == "xy" else XYZ_POOL
    shapes, p = [s for s, _ in pool], np.array([w for _, w in pool])
    if mode == O.NEWTON:
        p = np.where([s[0] * s[1] * s[2] <= NEWTON_MAX_POINTS for s in shapes], p, 0.0)
    dims = shapes[int(rng.choice(len(shapes), p=p / p.sum()))]
    env = {}
    if rng.uniform() < 0.65:
        env["GS_COARSE_POINTS"] = str(int(rng.choice([0, 8, 4096])))
    for name, value, share in (("GS_TILE_POINTS", "0", 0.25), ("GS_SWEEP3_MIN_POINTS", "1", 0.5),
                               ("GS_NO_SPECULATION", "1", 0.2), ("GS_NO_PIPELINE", "1", 0.2),
                               ("GS_NO_ZERO_GUESS", "1", 0.2), ("GS_NO_FUSED_RR", "1", 0.2),
                               ("GS_NO_FUSED_PROLONG", "1", 0.2), ("GS_NO_FUSED_SWEEPS", "1", 0.15)):
        if rng.uniform() < share:
            env[name] = value
    if not linear:
        pre, post = int(rng.integers(1, 4)), int(rng.integers(1, 4))
    elif rng.uniform() < 0.65:  # a symmetric cycle: PCG's condition
        pre = post = int(rng.choice([1, 2, 2, 3]))
    else:
        pre, post = int(rng.integers(0, 4)), int(rng.integers(0, 4))
        if pre == post:
            post = pre + 1
    omega = float(np.round(rng.uniform(0.5, 0.95), 3))
    gamma = float(np.round(rng.uniform(0.0, 1.5), 3)) if mode else 1.0
    ld, level_values = hierarchy(dims, coarsen, values, offsets)
    nl = len(ld)
    nonaligned = any(not X.aligned(ld[l], ld[l + 1]) for l in range(nl - 1))
    plan = types.SimpleNamespace(mode=mode, coarsen=coarsen, dims=dims, ld=ld, npre=pre, npost=post, weights=None,
                                 transfer="reference", fmg_prolong="aligned", smoother="jacobi", values=values,
                                 level_values=level_values, offsets=list(offsets))
    case = dict(idx=int(idx), attempt=int(attempt), dims=dims, mode=mode, pre=pre, post=post, omega=omega, gamma=gamma,
                values=tuple(values), offsets=tuple(offsets), env=env, coarsen=coarsen, family=family)
    ops, spec, count = [], [True] * nl, [0]
    fseed = [1000 * int(idx) + 517]

    def how():
        return ("float64" if rng.uniform() < 0.5 else "float32", IO_SCALES[int(rng.integers(0, 3))],
                "zyx" if rng.uniform() < 0.5 else "xyz", bool(rng.uniform() < 1.0 / 3.0), bool(rng.uniform() < 0.5))

    def upload(level, name, amp):
        fseed[0] += 1
        ops.append(("set_field", int(level), name, fseed[0], amp))

    def load(level, name, amp):
        fseed[0] += 1
        ops.append(("load", int(level), name, fseed[0], amp) + how())

    def provide(level, put=None):
        put = put or (load if rng.uniform() < 0.5 else upload)
        put(level, "v", 1.0)
        put(level, "f", 100.0)
        spec[level] = True

    def weights(permute=False):
        a, b = tuple(_weights(rng, pre, mode)), tuple(_weights(rng, post, mode))
        if permute and pre == post and pre >= 2:
            for shift in range(1, pre):  # the same weights in another order (a rotation that is not the identity)
                b = a[shift:] + a[:shift]
                if b != a:
                    break
        ops.append(("set_weights", a, b))
        plan.weights = (a, b)

    def emit(kind, arg=None):
        count[0] += 1
        op = {"fmg": ("fmg", 1), "pcg": ("pcg",), "set_smoother": ("set_smoother", arg)}.get(kind)
        if op is not None and refusal(plan, *op) is not None:
            ops.append(("refused", op))
        elif kind == "solve":
            ops.append(("solve",))
            spec[:] = [True] * nl if case["tol"] == 0.0 else [True] + [False] * (nl - 1)
        elif kind == "vcycle":
            ops.append(("vcycle",))
            spec[:] = [True] * nl
        elif kind == "fmg":
            if rng.uniform() < 0.3:
                upload(0, "f", 100.0)
            ops.append(op)
            spec[:] = [True] * nl
        elif kind == "pcg":
            ops.append(op)
            spec[:] = [True] + [False] * (nl - 1)
        elif kind == "set_smoother":
            ops.append(op)
            plan.smoother = arg
        elif kind == "set_fmg_prolong":
            ops.append((kind, arg))
            plan.fmg_prolong = arg
        elif kind == "set_transfer":
            ops.append((kind, arg))
            plan.transfer = arg
        elif kind == "set_weights":
            weights(bool(arg))
        elif kind == "clear_weights":
            ops.append((kind,))
            plan.weights = None
        elif kind == "set_field":
            upload(0, "v", 1.0)
        elif kind == "load":
            level = 0 if rng.uniform() < 0.6 else int(rng.choice([l for l in range(nl) if spec[l]]))
            name = "v" if rng.uniform() < 0.5 else "f"
            load(level, name, 1.0 if name == "v" else 100.0)
        elif kind == "store":
            level = 0 if rng.uniform() < 0.6 else int(rng.choice([l for l in range(nl) if spec[l]]))
            ops.append(("store", level, "v" if rng.uniform() < 0.7 else "f") + how())
        elif kind == "refused":
            cands = [c for c in (("fmg", 1), ("pcg",), ("set_smoother", "zline")) if refusal(plan, *c) is not None]
            if cands:
                ops.append(("refused", cands[int(rng.integers(0, len(cands)))]))
            elif coarsen == "xyz" and nonaligned:  # FMG by position without the POSITION transfers on an even size
                emit("set_fmg_prolong", "position")
                emit("set_transfer", "reference")
                ops.append(("refused", ("fmg", 1)))
            else:
                ops.append(("vcycle",))
                spec[:] = [True] * nl
        else:  # an operation rooted at a level of its own: its v and f provided first, always where unspecified
            level = int(rng.integers(0, nl)) if arg is None else int(arg)
            if not spec[level] or (level > 0 and rng.uniform() < 0.5):
                provide(level)
            if kind == "vcycle_from":
                ops.append(("vcycle_from", level))
                spec[level + 1:] = [True] * (nl - level - 1)
            elif kind == "jacobi":
                ops.append(("jacobi", level, int(rng.integers(1, 9))))
            else:
                assert kind == "residual_norm"
                ops.append(("residual_norm", level))

    def cycling():
        k = rng.uniform()
        emit("vcycle" if k < 0.45 else ("solve" if k < 0.8 else "vcycle_from"), 0 if k >= 0.8 else None)

    def line_mode():
        modes = ["zline"] + (["auto"] if any(line_flags("auto", level_values, offsets)) else [])
        return modes[int(rng.integers(0, len(modes)))]

    def io_ops():
        if rng.uniform() < 0.5:
            ops.append(("set_weights", tuple(_weights(rng, pre, mode)), tuple(_weights(rng, post, mode))))
        if rng.uniform() < 0.5:
            ops.append(("set_transfer", "position"))
        if rng.uniform() < 0.4:
            ops.append(("set_fmg_prolong", "position"))

    if mode == O.NEWTON:
        case["maxiter"], case["tol"] = int(rng.integers(1, 3)), 0.0
        io_ops()
        if rng.uniform() < 0.65:
            load(0, "newtonV", 0.1)
        ops.append(("solve",))
        ops.append(("store", 0, "newtonV") + how())
        case["ops"] = tuple(ops)
        return case
    case["maxiter"] = int(rng.integers(2, 6)) if linear else int(rng.integers(1, 3))
    case["tol"] = 0.0 if rng.uniform() < 0.3 else float(np.round(10.0 ** -rng.uniform(0.2, 2.0), 6))
    if rng.uniform() < 0.5:
        weights(permute=rng.uniform() < 0.6)
    if rng.uniform() < (0.75 if nonaligned and coarsen == "xyz" else 0.3):
        ops.append(("set_transfer", "position"))
        plan.transfer = "position"
    target = int(rng.integers(3, 8))
    if linear:
        def pcg_ready():
            if coarsen == "xyz" and nonaligned and plan.transfer == "reference":
                emit("set_transfer", "position")

        def line_then_jacobi():
            emit("set_smoother", line_mode())
            cycling()
            emit("set_smoother", "jacobi")
            cycling()

        def jacobi_then_line():
            if plan.smoother != "jacobi":
                emit("set_smoother", "jacobi")
            cycling()
            emit("set_smoother", line_mode())
            cycling()

        def pcg_after_stop():
            case["tol"] = float(np.round(10.0 ** -rng.uniform(0.1, 0.8), 6))  # (a tol the first cycles can reach)
            case["maxiter"] = max(case["maxiter"], 3)
            pcg_ready()
            emit("solve")
            emit("pcg")

        def cycle_after_pcg():
            pcg_ready()
            emit("pcg")
            cycling()

        def pcg_permuted():
            pcg_ready()
            emit("set_weights", True)
            emit("pcg")

        def xy_auto_pcg():
            emit("set_smoother", "auto")
            emit("pcg")

        def fmg_position():
            if plan.weights is None:
                emit("set_weights")
            if plan.transfer != "position":
                emit("set_transfer", "position")
            emit("set_fmg_prolong", "position")
            emit("fmg")

        def load_level():
            level = int(rng.integers(1, nl))
            provide(level, load)
            k = rng.uniform()
            emit("vcycle_from" if k < 0.4 else ("jacobi" if k < 0.7 else "residual_norm"), level)

        def refused_mid():
            cycling()
            emit("refused")
            cycling()

        # (theme, the most drawn operations it adds, whether this configuration can run it, its rank): up to two per
        # session, those that the fewest configurations can run first (rank 0, then 1, then 2)
        themes = [(line_then_jacobi, 4, True, 2), (jacobi_then_line, 4, True, 2),
                  (pcg_after_stop, 3, pre == post, 1), (cycle_after_pcg, 3, pre == post, 1),
                  (pcg_permuted, 3, pre == post and pre >= 2, 1),
                  (xy_auto_pcg, 2, coarsen == "xy" and family in ("ISO", "WEAKZ") and pre == post, 0),
                  (fmg_position, 4, coarsen == "xyz" and nonaligned, 1), (load_level, 1, nl > 1, 2),
                  (refused_mid, 5, True, 2)]
        themes = [t for t in themes if t[2]]
        order = [int(j) for j in rng.permutation(len(themes))]
        picked = 0
        for j in sorted(order, key=lambda j: themes[j][3]):
            if picked < 2 and count[0] + themes[j][1] <= 7:
                themes[j][0]()
                picked += 1
        kinds = {"solve": 0.1, "vcycle": 0.1, "vcycle_from": 0.08, "fmg": 0.06, "jacobi": 0.08, "residual_norm": 0.06,
                 "set_field": 0.03, "set_weights": 0.05, "clear_weights": 0.02, "set_transfer": 0.04, "pcg": 0.08,
                 "set_smoother": 0.08, "set_fmg_prolong": 0.04, "load": 0.07, "store": 0.16, "refused": 0.02}
    else:
        kinds = {"solve": 0.25, "vcycle": 0.15, "vcycle_from": 0.1, "fmg": 0.12, "jacobi": 0.07, "residual_norm": 0.05,
                 "set_field": 0.03, "set_weights": 0.05, "set_transfer": 0.04, "set_fmg_prolong": 0.08, "load": 0.1,
                 "store": 0.1, "refused": 0.06}
    budget = 10 ** 9 if linear else 4  # V-cycles a non-LINEAR session may still run (fmg(k): k + 1)
    cost = {"solve": case["maxiter"], "vcycle": 1, "vcycle_from": 1, "fmg": 2, "refused": 1}
    while count[0] < target:
        allowed = {k: w for k, w in kinds.items() if cost.get(k, 0) <= budget}
        names, pk = list(allowed), np.array(list(allowed.values()))
        kind = names[int(rng.choice(len(names), p=pk / pk.sum()))]
        budget -= cost.get(kind, 0)
        arg = None
        if kind == "set_smoother":
            arg = SMOOTHERS[int(rng.integers(0, 3))]
        elif kind == "set_transfer":
            arg = "position" if rng.uniform() < 0.65 else "reference"
        elif kind == "set_fmg_prolong":
            arg = "position" if rng.uniform() < 0.75 else "aligned"
        emit(kind, arg)
    if not any(op[0] in CYCLING + ("jacobi", "residual_norm") for op in ops):
        ops.append(("vcycle",))  # (only switches, transfers of fields and refusals were drawn)
    case["ops"] = tuple(ops)
    return case


@functools.lru_cache(maxsize=None)
def resolve_features(seed, idx):
    """resolve() for the feature family."""
    reasons = []
    for attempt in range(20):
        case = draw_features(seed, idx, attempt)
        ok, why, s, _ = accept(case)
        if ok:
            return case, tuple(reasons), tuple(s.stops)
        reasons.append(why)
    raise AssertionError(f"feature session {idx} of seed {seed}: 20 draws rejected {reasons}")


def feature_cases(n=None, seed=None):
    """The feature sessions of a seed. GS_FEATURE_SESSIONS_N / GS_FEATURE_SESSIONS_SEED: a longer or different draw."""
    n = int(os.environ.get("GS_FEATURE_SESSIONS_N", FEATURE_N)) if n is None else n
    seed = int(os.environ.get("GS_FEATURE_SESSIONS_SEED", FEATURE_SEED)) if seed is None else seed
    if seed == FEATURE_SEED and n <= FEATURE_N:
        return [draw_features(seed, i, FEATURE_REDRAWS.get(i, 0)) for i in range(n)]
    return [resolve_features(seed, i)[0] for i in range(n)]


def feature_regimes(case, stops):
    """What a feature session reaches by its draw and its stops (Session.stops: one flag per solve and pcg, in order).
    tests/test_gpu_feature_sessions.py judges the same regimes on the grid itself, and two more that only a grid can
    tell (which z-line instance a line level takes)."""
    ld, level_values = hierarchy(case["dims"], case["coarsen"], case["values"], case["offsets"])
    nonaligned = any(not X.aligned(ld[l], ld[l + 1]) for l in range(len(ld) - 1))
    out = dict(line_then_jacobi=False, jacobi_then_line=False, pcg_after_stop=False, cycle_after_pcg=False,
               pcg_permuted=False, xy_auto_pcg=False, fmg_position_weighted=False, load_then_rooted=False,
               side_load=False, fp32_store=False, refused_mid=False)
    smoother, weights, fmgp, k = "jacobi", None, "aligned", 0
    ran_line = ran_point = stopped = after_pcg = real_before = False
    loaded, pending_refusal = set(), False
    for op in case["ops"]:
        kind = op[0]
        flags = line_flags(smoother, level_values, case["offsets"])
        if kind == "set_smoother":
            smoother = op[1]
        elif kind == "set_weights":
            weights = (op[1], op[2])
        elif kind == "clear_weights":
            weights = None
        elif kind == "set_fmg_prolong":
            fmgp = op[1]
        elif kind == "load":
            out["side_load"] |= op[9]
            if op[1] >= 1:
                loaded.add(op[1])
        elif kind == "store":
            out["fp32_store"] |= op[3] == "float32"
        if kind in ("vcycle_from", "jacobi", "residual_norm") and op[1] in loaded:
            out["load_then_rooted"] = True
        if kind not in ("load", "set_field"):
            loaded.clear()
        if kind in CYCLING:
            if any(flags):
                out["jacobi_then_line"] |= ran_point
                ran_line = True
            else:
                out["line_then_jacobi"] |= ran_line
                ran_point = True
            if kind != "pcg" and after_pcg:
                out["cycle_after_pcg"] = True
            if kind == "fmg" and fmgp == "position" and weights is not None and nonaligned:
                out["fmg_position_weighted"] = True
        if kind == "pcg":
            out["pcg_after_stop"] |= stopped
            out["pcg_permuted"] |= weights is not None and tuple(weights[0]) != tuple(weights[1])
            out["xy_auto_pcg"] |= case["coarsen"] == "xy" and smoother == "auto" and not flags[0] and flags[-1]
            after_pcg = True
        if kind in ("solve", "pcg"):
            stopped = stopped or (kind == "solve" and stops[k])
            k += 1
        if kind == "refused":
            pending_refusal = pending_refusal or real_before
        elif kind in CYCLING + ("jacobi", "residual_norm"):
            out["refused_mid"] |= pending_refusal
            real_before = True
    return out


def feature_case_id(c):
    kinds = {"solve": "S", "vcycle": "V", "vcycle_from": "R", "fmg": "F", "jacobi": "J", "residual_norm": "N",
             "set_field": "u", "set_weights": "w", "clear_weights": "c", "set_transfer": "t", "pcg": "P",
             "set_smoother": "z", "set_fmg_prolong": "p", "load": "l", "store": "o", "refused": "x"}
    return (f"f{c['idx']}-{c['coarsen']}-{c['family']}-{'x'.join(map(str, c['dims']))}-m{c['mode']}-{c['pre']}+{c['post']}-"
            + "".join(kinds[op[0]] for op in c["ops"]))
