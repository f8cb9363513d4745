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
tests/test_session_ref_cpu.py), so that collecting the tests runs no model."""
import functools
import os

import numpy as np

import oracle as O
import weights_ref as W
import xfer_ref as X
from fmg_ref import level_dims, prolong as fmg_prolong, start_level

CANON = [(0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
MAX_WEIGHTS = 8  # GS_MAX_WEIGHTS (tests/test_weights_cpu.py holds the library to >= 8)


def threshold(initial, tol):
    """initial / (1 / tol) in IEEE arithmetic (tol = 0: 0), the reference's stop threshold."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.float64(initial) / (np.float64(1.0) / np.float64(tol)))


def noise(dims, seed, scale):
    """Seeded noise in [-scale, scale] on the interior of a padded array, zero ring."""
    a = np.zeros(tuple(n + 2 for n in dims))
    a[1:-1, 1:-1, 1:-1] = np.random.default_rng(seed).uniform(-scale, scale, dims)
    return a


class Session:
    def __init__(self, dims, mode=O.LINEAR, pre=2, post=2, omega=0.8, gamma=1.0, stencil=None):
        self.dims, self.mode, self.npre, self.npost = tuple(int(d) for d in dims), mode, int(pre), int(post)
        self.omega, self.gamma, self.stencil = float(omega), float(gamma), stencil
        self.weights, self.transfer = None, "reference"
        self.ld = level_dims(self.dims)
        self.nl = len(self.ld)
        self.c = X.Cycle(self.dims, mode, [self.omega] * self.npre, [self.omega] * self.npost, self.gamma,
                         transfer=self.transfer, stencil=stencil)
        self.spec = {(n, l): True for n in ("v", "f") for l in range(self.nl)}
        self.ratios = []
        self.stops = []  # one entry per solve (outer loops only): True if it stopped on tol before its last cycle
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
        assert mode in ("reference", "position")
        self.transfer = mode

    def _cfg(self):
        c = self.c
        c.pre, c.post = self.weights if self.weights else ([self.omega] * self.npre, [self.omega] * self.npost)
        c.transfer = self.transfer
        return c

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
        c = self.c
        c.v[level] = W.sweeps(c.v[level], c.f[level], c.h[level], self.mode, [self.omega] * k, self.gamma, self.stencil)

    def residual_norm(self, level):
        assert self.mode != O.NEWTON
        self._reads(level)
        return self.c.residual(level)[1]

    def fmg(self, k):
        s = start_level(self.dims)
        assert s > 0 and self.mode != O.NEWTON and k >= 1
        assert self.spec[("f", 0)]
        c = self._cfg()
        for l in range(s):
            c.f[l + 1] = c.R(l, c.f[l])
        for l in range(s, -1, -1):
            v0 = O.zeros(*self.ld[l])
            if l < s:
                v0[1:-1, 1:-1, 1:-1] = fmg_prolong(c.v[l + 1])[1:-1, 1:-1, 1:-1]
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
    return Session(case["dims"], case["mode"], case["pre"], case["post"], case["omega"], case["gamma"], stencil_of(case))


def apply(target, case, op):
    """One operation of a case on `target` (a Session, or the GPU test's adapter with the same methods): its result."""
    kind = op[0]
    if kind == "solve":
        return target.solve(case["maxiter"], case["tol"])
    if kind == "set_field":
        _, level, name, seed, scale = op
        return target.set_field(level, name, noise(level_dims(case["dims"])[level], seed, scale))
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
