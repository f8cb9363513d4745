"""tests/session_ref.py — the CPU model of a driver session and the generator of tests/test_gpu_sessions.py — pinned to
the CPU oracle and to the references it is composed of (no GPU). A session of solves only is oracle.Grid.solve() on every
level (fields bit for bit in LINEAR mode, within tests/test_weights_cpu.py's 1e-12 otherwise); repeated vcycle() is
solve(n, 0); fmg, vcycle_from and set_transfer are weights_ref.fmg, a stand-alone Cycle and a no-op on aligned sizes; and the committed
seed meets the generator's conditions: at most 5 % of the draws rejected, every mode within 5 points of its share, every
regime that depends on the draw alone reached by at least five sessions.

Norms. The oracle sums a norm's squares in an OpenMP reduction whose order is not fixed: the same call returns values one
or two ulps apart from run to run (oracle/gs_oracle.cpp's header: about 1e-14 relative). So norms and histories, unlike
fields, cannot be held to equality even in LINEAR mode, not even between two runs of the oracle: they are held to 1e-13,
ten times that figure and a tenth of the GPU tests' LINEAR bound."""
import collections
import functools

import numpy as np
import pytest

import oracle as O
import session_ref as S
import weights_ref as W
import xfer_ref as X
from fmg_ref import level_dims, start_level

SMALL = (12, 10, 8)  # four levels, no transition aligned: the oracle's transfers throughout
GENERAL = dict(values=(6.5, -1.25, -0.75, -1, -1.1, -0.9, -1), offsets=tuple(S.CANON))
PERMUTED = dict(values=(6.5, -1, -1.25, -0.9, -0.75, -1.1, -1),
                offsets=((0, 0, 0), (0, 0, -1), (1, 0, 0), (0, 0, 1), (-1, 0, 0), (0, -1, 0), (0, 1, 0)))


def same(a, b, what):
    ne = np.ascontiguousarray(a).view(np.int64) != np.ascontiguousarray(b).view(np.int64)
    assert a.shape == b.shape and not ne.any(), f"{what}: {int(ne.sum())} words differ, first at {tuple(np.argwhere(ne)[0])}"


def close(a, b, what, tol=1e-12):
    d = np.abs(np.asarray(a) - np.asarray(b)).max()
    assert d <= tol * np.abs(b).max(), f"{what}: {d} of {np.abs(b).max()}"


def norms_close(got, want, tol=1e-13):
    got, want = np.atleast_1d(got), np.atleast_1d(want)
    return len(got) == len(want) and all(abs(a - b) <= tol * abs(b) for a, b in zip(got, want))


def against_oracle(dims, mode, pre, post, maxiter, tol=0.0, omega=0.8, gamma=1.0, stencil=None):
    """One solve on a fresh Session and on oracle.Grid: histories, and v and f of every level the model specifies."""
    st = O.Stencil.make(**stencil) if stencil else None
    g = O.Grid(dims, mode=mode, maxiter=maxiter, tol=tol, omega=omega, gamma=gamma, pre=pre, post=post, stencil=st)
    want = g.solve()
    s = S.Session(dims, mode, pre, post, omega, gamma, st)
    got = s.solve(maxiter, tol)
    assert len(got) == len(want), (got, want)
    assert norms_close(got, want, 1e-13 if mode == O.LINEAR else 1e-12), (got, want)
    names = [("newtonV", 0)] if mode == O.NEWTON else [(n, l) for l in range(s.nl) for n in ("v", "f")]
    for n, l in names:
        if not s.specified(l, n):
            continue
        if mode == O.LINEAR:
            same(s.field(l, n), g.field(l, n), f"{n} of level {l}")
        elif mode == O.NONLINEAR and n == "v" and l > 0:
            # the driver keeps a coarse level's FAS iterate (gs_prolong_add subtracts restV on the fly); the reference
            # overwrites it with the correction v - restV (CpuSolver.cpp:121-124)
            close(s.field(l, n), g.field(l, "v") + g.field(l, "restV"), f"v of level {l}")
        else:
            close(s.field(l, n), g.field(l, n), f"{n} of level {l}")
    return s, got


@pytest.mark.parametrize("mode", [O.LINEAR, O.NONLINEAR, O.NEWTON])
@pytest.mark.parametrize("pre", range(9))
def test_plain_solve_is_the_oracle(pre, mode):
    for post in range(9):
        if pre + post:
            against_oracle(SMALL, mode, pre, post, 2, gamma=1.0 if mode == O.LINEAR else 0.7)


@pytest.mark.parametrize("mode", [O.LINEAR, O.NONLINEAR, O.NEWTON])
@pytest.mark.parametrize("stencil", [GENERAL, PERMUTED], ids=["general", "permuted"])
@pytest.mark.parametrize("dims", [SMALL, (15, 15, 15)], ids=str)
def test_plain_solve_with_a_stencil(dims, stencil, mode):
    against_oracle(dims, mode, 3, 2, 2, omega=0.7, stencil=stencil)


@pytest.mark.parametrize("mode,pre,dims", [(0, 2, (31, 31, 31)), (0, 1, (23, 19, 17)), (1, 2, (31, 31, 31)),
                                           (2, 2, (15, 15, 15))])
def test_early_stop(mode, pre, dims):
    """A tol between the 2nd and the 3rd cycle's ratios (tests/test_gpu_solver.py's test_early_stop_level0_exact): the
    solve stops after cycle 3 as the oracle's does, and the levels below 0 are unspecified from then on."""
    h = O.Grid(dims, mode=mode, maxiter=8, pre=pre, post=2).solve()
    tol = (h[2] * h[3]) ** 0.5 / h[0]
    s, got = against_oracle(dims, mode, pre, 2, 8, tol=tol)
    assert len(got) == 4 and s.stops == [True]
    assert all(abs(r - 1.0) > 1e-6 for r in s.ratios)
    if mode != O.NEWTON:
        assert len(s.ratios) == 3 and s.ratios[0] > 1 and s.ratios[1] > 1 and s.ratios[2] < 1
        assert s.specified(0, "v") and s.specified(0, "f")
        assert not any(s.specified(l, n) for l in range(1, s.nl) for n in ("v", "f"))
        with pytest.raises(AssertionError, match="unspecified"):
            s.jacobi(1, 1)
        s.set_field(1, "v", S.noise(s.ld[1], 1, 1.0))
        s.set_field(1, "f", S.noise(s.ld[1], 2, 1.0))
        s.vcycle_from(1)
        assert all(s.specified(l, n) for l in range(1, s.nl) for n in ("v", "f"))


def test_a_stop_on_the_last_cycle_specifies_every_level():
    h = O.Grid((15, 15, 15), maxiter=3).solve()
    s, got = against_oracle((15, 15, 15), O.LINEAR, 2, 2, 3, tol=(h[2] * h[3]) ** 0.5 / h[0])
    assert len(got) == 4 and s.stops == [False] and len(s.ratios) == 2
    assert all(s.specified(l, n) for l in range(s.nl) for n in ("v", "f"))


@pytest.mark.parametrize("mode", [O.LINEAR, O.NONLINEAR])
def test_repeated_vcycles_are_a_solve(mode):
    a, b = (S.Session((17, 9, 12), mode, 3, 1, 0.7, 0.5, O.Stencil.make(**GENERAL)) for _ in range(2))
    for s in (a, b):
        s.set_weights([0.6, 1.1, 0.9], [0.8])
        s.set_transfer("position")
    hist = a.solve(3, 0.0)
    assert norms_close([b.vcycle() for _ in range(3)], hist[1:])
    for l in range(a.nl):
        for n in ("v", "f"):
            same(a.field(l, n), b.field(l, n), f"{n} of level {l}")


@pytest.mark.parametrize("mode", [O.LINEAR, O.NONLINEAR])
@pytest.mark.parametrize("dims,k", [((15, 15, 15), 1), ((31, 15, 7), 2)], ids=str)
def test_fmg_is_weights_ref_fmg(dims, k, mode):
    pre, post = (0.6, 1.2, 0.9), (1.0, 0.7)
    f0 = S.noise(dims, 5, 100.0)
    want_v, want_res = W.fmg(dims, mode, k, pre, post, 0.8, f0=f0)
    s = S.Session(dims, mode, 3, 2, 0.8, 0.8)
    s.set_weights(pre, post)
    s.set_transfer("position")  # (aligned throughout: no difference)
    s.set_field(0, "f", f0)
    s.set_field(0, "v", S.noise(dims, 6, 1.0))  # overwritten
    assert norms_close(s.fmg(k), want_res)
    same(s.field(0, "v"), want_v, "level-0 v")
    # what it leaves on the levels is the last V-cycle's: one more from level 0 agrees with a stand-alone Cycle
    c = X.Cycle(dims, mode, pre, post, 0.8, f0=f0, v0=want_v)
    assert norms_close(s.vcycle(), c.vcycle())
    for l in range(s.nl):
        same(s.field(l, "v"), c.v[l], f"v of level {l}")
        same(s.field(l, "f"), c.f[l], f"f of level {l}")


@pytest.mark.parametrize("transfer", ["reference", "position"])
@pytest.mark.parametrize("mode", [O.LINEAR, O.NONLINEAR])
def test_vcycle_from_is_the_cycle_of_the_sub_hierarchy(mode, transfer):
    dims, st = (24, 20, 16), O.Stencil.make(**PERMUTED)
    s = S.Session(dims, mode, 2, 3, 0.75, 0.6, st)
    s.set_transfer(transfer)
    before = [s.field(0, n).copy() for n in ("v", "f")]
    v1, f1 = S.noise(s.ld[1], 7, 1.0), S.noise(s.ld[1], 8, 100.0)
    s.set_field(1, "v", v1)
    s.set_field(1, "f", f1)
    s.vcycle_from(1)
    assert level_dims(s.ld[1]) == s.ld[1:]
    c = X.Cycle(s.ld[1], mode, [0.75] * 2, [0.75] * 3, 0.6, f0=f1, v0=v1, transfer=transfer, stencil=st)
    c.vcycle_from(0)
    for l in range(1, s.nl):
        same(s.field(l, "v"), c.v[l - 1], f"v of level {l}")
        same(s.field(l, "f"), c.f[l - 1], f"f of level {l}")
    for a, n in zip(before, ("v", "f")):
        same(s.field(0, n), a, f"level 0's {n} (not touched)")
    # the whole hierarchy's own Cycle.vcycle_from agrees too
    w = X.Cycle(dims, mode, [0.75] * 2, [0.75] * 3, 0.6, transfer=transfer, stencil=st)
    w.v[1], w.f[1] = v1.copy(), f1.copy()
    w.vcycle_from(1)
    same(s.field(1, "v"), w.v[1], "Cycle.vcycle_from")


@pytest.mark.parametrize("mode", [O.LINEAR, O.NONLINEAR, O.NEWTON])
def test_set_transfer_changes_no_bit_on_aligned_sizes(mode):
    a, b = (S.Session((15, 7, 31), mode, 2, 1, 0.8, 0.9) for _ in range(2))
    b.set_transfer("position")
    assert norms_close(a.solve(2, 0.0), b.solve(2, 0.0))
    name = "newtonV" if mode == O.NEWTON else "v"
    same(a.field(0, name), b.field(0, name), name)
    # ... and does on others
    a, b = (S.Session((12, 10, 8), mode, 2, 1, 0.8, 0.9) for _ in range(2))
    b.set_transfer("position")
    assert not norms_close(a.solve(2, 0.0), b.solve(2, 0.0), 1e-6)


def test_jacobi_keeps_omega_and_newton_takes_an_initial_newtonv():
    s = S.Session((9, 8, 7), O.LINEAR, 2, 2, 0.65)
    s.set_weights([1.2, 0.5], [0.9, 0.4])
    s.jacobi(0, 3)
    same(s.field(0, "v"), O.jacobi(O.zeros(9, 8, 7), O.rhs(9, 8, 7, O.LINEAR), 1.0 / 9, omega=0.65, sweeps=3), "jacobi")
    w0 = S.noise((12, 10, 8), 3, 0.1)
    n = S.Session((12, 10, 8), O.NEWTON, 2, 2, 0.8, 1.0)
    n.set_field(0, "newtonV", w0)
    hist = n.solve(2, 0.0)
    want_h, want_w = X.newton_solve((12, 10, 8), 2, transfer="reference", w0=w0)
    assert norms_close(hist, want_h)
    same(n.field(0, "newtonV"), want_w, "newtonV")
    assert not norms_close(X.newton_solve((12, 10, 8), 2, transfer="reference")[0], want_h, 1e-6)


# ---- the generator ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def resolved():
    """The committed seed's sessions by running the model (what REDRAWS abbreviates)."""
    return [S.resolve(S.SEED, i) for i in range(S.N)]


def test_cases_are_a_pure_function_of_the_seed():
    assert S.cases() == S.cases() and len(S.cases()) == S.N
    assert S.draw(S.SEED, 7, 1) == S.draw(S.SEED, 7, 1) != S.draw(S.SEED, 7, 0)
    assert S.cases(5, S.SEED + 1) == S.cases(5, S.SEED + 1) != S.cases(5)
    assert len({S.case_id(c) for c in S.cases()}) == S.N  # the ids tell the sessions apart


def test_the_committed_table_of_redraws_is_the_models():
    got = [c for c, _, _ in resolved()]
    assert {c["idx"]: c["attempt"] for c in got if c["attempt"]} == S.REDRAWS
    assert got == S.cases()


def test_generator_conditions():
    rejected = collections.Counter(r for _, why, _ in resolved() for r in why)
    print("rejected draws:", dict(rejected))
    assert sum(rejected.values()) <= 0.05 * S.N
    modes = collections.Counter(c["mode"] for c in S.cases())
    print("modes:", dict(modes))
    for mode, share in ((O.LINEAR, 0.60), (O.NONLINEAR, 0.25), (O.NEWTON, 0.15)):
        assert modes[mode] >= (share - 0.05) * S.N, modes
    shapes = {s for s, _ in S.POOL}
    for c, _, stops in resolved():
        assert c["dims"] in shapes and max(c["dims"]) <= 130
        assert 0 <= c["pre"] <= 6 and 0 <= c["post"] <= 6 and c["pre"] + c["post"] > 0
        assert 0.5 <= c["omega"] <= 0.95 and 0.0 <= c["gamma"] <= 1.5
        assert set(c["env"]) <= set(S.SWITCHES)
        kinds = [op[0] for op in c["ops"]]
        cycling = sum(k in ("solve", "vcycle", "vcycle_from", "fmg", "jacobi", "residual_norm") for k in kinds)
        if c["mode"] == O.NEWTON:
            assert kinds[-1] == "solve" and kinds.count("solve") == 1 and c["maxiter"] <= 2
            assert set(kinds[:-1]) <= {"set_weights", "set_transfer", "set_field"}
        else:
            assert 1 <= cycling <= 6
            assert "fmg" not in kinds or start_level(c["dims"]) > 0
        if c["mode"] == O.NONLINEAR:  # at most four V-cycles (fmg: its level-0 cycle and the nested ones as one more)
            assert sum({"solve": c["maxiter"], "vcycle": 1, "vcycle_from": 1, "fmg": 2}.get(k, 0) for k in kinds) <= 4
        for op in c["ops"]:
            if op[0] == "set_weights":
                assert len(op[1]) == c["pre"] and len(op[2]) == c["post"] and max(c["pre"], c["post"]) <= S.MAX_WEIGHTS
        assert len(stops) == kinds.count("solve")


def test_a_session_too_close_to_a_stop_is_rejected():
    """The committed seed rejects nothing, so the filter is shown to work on a made-up session: a tol that puts the
    first cycle's norm within 1e-9 of its threshold is refused, the same session with a clear margin is kept."""
    case = dict(S.draw(S.SEED, 0), dims=(15, 15, 15), mode=O.LINEAR, pre=2, post=2, gamma=1.0, env={}, maxiter=3,
                tol=0.0, ops=(("solve",),))
    h = S.run_model(case)[1][0]
    ok, why, _, _ = S.accept(dict(case, tol=h[1] / h[0] * (1 + 1e-9)))
    assert not ok and why == "stop margin"
    ok, why, s, _ = S.accept(dict(case, tol=h[1] / h[0] * 1.5))
    assert ok and s.stops == [True]
    bad = dict(case, mode=O.NONLINEAR, gamma=1.5, ops=(("set_field", 0, "v", 1, 1e3), ("solve",)))  # exp overflows
    assert S.accept(bad)[:2] == (False, "non-finite")


def test_regimes_the_draw_decides_are_reached():
    count = collections.Counter()
    for c, _, stops in resolved():
        count.update(k for k, v in S.regimes(c, stops).items() if v)
        count["feature_between_cycles"] += feature_between_cycles(c)
    print("sessions per regime:", dict(count))
    for k in ("weighted_early_stop", "op_after_stop", "position_pre3", "fmg_weighted_coarse", "feature_between_cycles"):
        assert count[k] >= 5, count


def feature_between_cycles(c):
    """A weights or transfer change between two operations that cycle."""
    kinds = [op[0] for op in c["ops"]]
    cyc = [i for i, k in enumerate(kinds) if k in ("solve", "vcycle", "vcycle_from", "fmg")]
    return any(k in ("set_weights", "clear_weights", "set_transfer") and cyc and cyc[0] < i < cyc[-1]
               for i, k in enumerate(kinds))
