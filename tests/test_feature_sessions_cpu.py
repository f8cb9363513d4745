"""The pieces tests/session_ref.py's model gained for tests/test_gpu_feature_sessions.py — the smoother, XY grids, pcg,
FMG by position, load / store and the refusal rules — pinned to the single-feature references the project already
trusts (no GPU), and the feature generator held to its conditions. Fields are compared word for word (everything here
is LINEAR unless said), norms to 1e-13 (tests/test_session_ref_cpu.py has the reason: the oracle's norm is an OpenMP
reduction)."""
import collections
import functools
import hashlib

import numpy as np
import pytest

import fmg_pa_ref
import oracle as O
import pcg_ref as P
import semi_ref
import session_ref as S
import zline_ref as Z
from test_session_ref_cpu import norms_close, same

# sha256 of repr(session_ref.cases()) on the commit before the feature generator was added: the 120 sessions of
# tests/test_gpu_sessions.py may not move
CASES_DIGEST = "d4ad0bd15c69d3c008c377504b8b75a32358d0ad5c86f7dbbc99ef835aad6f91"
PRE, POST = (0.9, 0.6), (0.6, 0.9)


def stencil(values, offsets=O.CANONICAL):
    return O.Stencil.make(values, offsets)


def levels_same(s, c, what):
    assert s.nl == len(c.ld)
    for l in range(s.nl):
        same(s.field(l, "v"), c.v[l], f"{what}: v of level {l}")
        same(s.field(l, "f"), c.f[l], f"{what}: f of level {l}")


# ---- the smoother ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["STRONGZ", "UPLO"])
@pytest.mark.parametrize("dims,transfer", [((15, 15, 9), "reference"), ((12, 10, 8), "position")], ids=str)
def test_a_zline_session_is_zcycle(dims, transfer, family):
    values, offsets = S.FAMILIES[family]
    f = S.noise(dims, 3, 100.0)
    s = S.Session(dims, O.LINEAR, 2, 2, 0.8, 1.0, stencil(values, offsets))
    s.set_field(0, "f", f)
    s.set_weights(PRE, POST)
    s.set_transfer(transfer)
    s.set_smoother("zline")
    kw = dict(pre=PRE, post=POST, f0=f)
    c = Z.ZCycle(dims, values, list(offsets), **kw) if transfer == "reference" else Z.ZCyclePa(dims, values, list(offsets), **kw)
    assert norms_close([s.vcycle() for _ in range(2)], [c.vcycle() for _ in range(2)])
    levels_same(s, c, f"{family} {transfer}")
    # the stand-alone sweeps follow the smoother, with the grid's omega
    s.jacobi(1, 2)
    v = c.v[1]
    for _ in range(2):
        v = Z.sweep(v, c.f[1], c.h[1], 0.8, values, list(offsets))
    same(s.field(1, "v"), v, "two stand-alone line sweeps on level 1")
    # AUTO on an XYZ grid is all or nothing: lines for these two families
    assert S.line_flags("auto", s.level_values, s.offsets) == [True] * s.nl


@pytest.mark.parametrize("smoother", S.SMOOTHERS)
@pytest.mark.parametrize("family", ["WEAKZ", "UPLO"])
def test_an_xy_session_is_semi_refs_cycle(family, smoother):
    dims = (16, 12, 20)
    values, offsets = S.FAMILIES[family]
    f = S.noise(dims, 4, 100.0)
    s = S.Session(dims, O.LINEAR, 2, 2, 0.8, 1.0, stencil(values, offsets), coarsen="xy")
    s.set_field(0, "f", f)
    s.set_weights(PRE, POST)
    s.set_smoother(smoother)
    s.set_transfer("position")  # changes nothing on an XY grid
    c = semi_ref.Cycle(dims, values, list(offsets), smoother=smoother, pre=PRE, post=POST, f0=f)
    assert s.ld == c.ld and [tuple(v) for v in s.level_values] == [tuple(v) for v in c.values]
    assert S.line_flags(smoother, s.level_values, s.offsets) == c.line
    hist = s.solve(2, 0.0)
    assert norms_close(hist, c.solve(2))
    levels_same(s, c, f"{family} {smoother}")
    # a cycle rooted at level 1, and the residual norm there, take the level's own stencil
    v1, f1 = S.noise(s.ld[1], 5, 1.0), S.noise(s.ld[1], 6, 100.0)
    s.set_field(1, "v", v1)
    s.set_field(1, "f", f1)
    c.v[1], c.f[1] = v1.copy(), f1.copy()
    s.vcycle_from(1)
    c.vcycle_from(1)
    levels_same(s, c, "rooted at level 1")
    assert norms_close(s.residual_norm(1), c.residual(1)[1])
    assert S.refusal(s, "fmg", 1) and s.fmg_start_level() == 0


def test_back_to_jacobi_is_a_session_that_never_left():
    dims = (12, 10, 8)
    st = stencil(Z.STRONGZ)
    a = S.Session(dims, O.LINEAR, 2, 1, 0.7, 1.0, st)
    a.set_transfer("position")
    a.set_smoother("zline")
    a.vcycle()
    a.jacobi(0, 2)
    a.set_smoother("auto")
    a.solve(2, 0.0)
    before = [(a.field(l, "v").copy(), a.field(l, "f").copy(), a.specified(l, "v")) for l in range(a.nl)]
    a.set_smoother("jacobi")
    for l, (v, f, spec) in enumerate(before):  # the switch changes no field and no mark
        same(a.field(l, "v"), v, f"v of level {l} across the switch")
        same(a.field(l, "f"), f, f"f of level {l} across the switch")
        assert a.specified(l, "v") == spec
    b = S.Session(dims, O.LINEAR, 2, 1, 0.7, 1.0, st)
    b.set_transfer("position")
    for l, (v, f, _) in enumerate(before):
        b.set_field(l, "v", v)
        b.set_field(l, "f", f)
    assert norms_close(a.vcycle(), b.vcycle())
    a.jacobi(1, 3)
    b.jacobi(1, 3)
    for l in range(a.nl):
        same(a.field(l, "v"), b.field(l, "v"), f"v of level {l}")
        same(a.field(l, "f"), b.field(l, "f"), f"f of level {l}")


# ---- pcg ---------------------------------------------------------------------------------------------------------------
def test_free_running_pcg_is_pcg_ref():
    dims, st = (12, 10, 8), stencil(Z.WEAKZ)
    f, x0 = S.noise(dims, 7, 1.0), S.noise(dims, 8, 0.01)
    s = S.Session(dims, O.LINEAR, 2, 2, 0.8, 1.0, st)
    s.set_field(0, "f", f)
    s.set_field(0, "v", x0)
    assert S.refusal(s, "pcg")  # a non-aligned transition under the REFERENCE transfers
    s.set_transfer("position")
    s.set_weights(PRE, POST)
    hist = s.pcg(4, 0.0)
    ref = P.Pcg(dims, f, x0=x0, pre=PRE, post=POST, transfer="position", stencil=st)
    want, rec = ref.run(4)
    assert len(hist) == 5 and norms_close(hist, want)
    same(s.field(0, "v"), ref.x, "x")
    same(s.field(0, "f"), f, "f")
    assert s.stops == [False] and not any(s.specified(l, n) for l in range(1, s.nl) for n in ("v", "f"))
    with pytest.raises(AssertionError, match="unspecified"):
        s.vcycle_from(1)
    # the replay of the free run's own scalars is the free run, word for word
    t = S.Session(dims, O.LINEAR, 2, 2, 0.8, 1.0, st)
    t.set_field(0, "f", f)
    t.set_field(0, "v", x0)
    t.set_transfer("position")
    t.set_weights(PRE, POST)
    t.pcg(4, 0.0, scalars=[(r["alpha"], r["beta"]) for r in rec])
    same(t.field(0, "v"), ref.x, "replayed x")
    # a stop on tol: the history ends there, and a record that goes on is refused
    tol = (want[2] * want[3]) ** 0.5 / want[0]
    u = S.Session(dims, O.LINEAR, 2, 2, 0.8, 1.0, st)
    for name, a in (("f", f), ("v", x0)):
        u.set_field(0, name, a)
    u.set_transfer("position")
    u.set_weights(PRE, POST)
    assert len(u.pcg(4, tol)) == 4 and u.stops == [True] and all(abs(r - 1.0) > 1e-6 for r in u.ratios)
    w = S.Session(dims, O.LINEAR, 2, 2, 0.8, 1.0, st)
    for name, a in (("f", f), ("v", x0)):
        w.set_field(0, name, a)
    w.set_transfer("position")
    w.set_weights(PRE, POST)
    with pytest.raises(AssertionError, match="goes on past"):
        w.pcg(4, tol, scalars=[(r["alpha"], r["beta"]) for r in rec])


class SemiPcg(P.Pcg):
    """tests/test_gpu_semi.py's composition: pcg_ref with semi_ref's XY + AUTO cycle as the preconditioner."""

    def M(self, r):
        c = semi_ref.Cycle(self.dims, Z.WEAKZ, smoother="auto", f0=r)
        c.vcycle_from(0)
        return c.v[0]


def test_free_running_pcg_on_an_xy_grid_is_the_xy_composition():
    dims, st = (16, 12, 20), stencil(Z.WEAKZ)
    f = Z.normal_rhs(dims, 1)
    s = S.Session(dims, O.LINEAR, 2, 2, 0.8, 1.0, st, coarsen="xy")
    s.set_field(0, "f", f)
    s.set_smoother("auto")
    assert S.refusal(s, "pcg") is None  # (no POSITION transfers needed: an XY transition is by position)
    hist = s.pcg(3, 0.0)
    m = SemiPcg(dims, f, stencil=st)
    assert norms_close(hist, m.run(3)[0])
    same(s.field(0, "v"), m.x, "x")
    # a V-cycle after PCG specifies every level again
    s.vcycle()
    assert all(s.specified(l, n) for l in range(s.nl) for n in ("v", "f"))


# ---- FMG by position -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [O.LINEAR, O.NONLINEAR])
@pytest.mark.parametrize("dims", [(12, 10, 8), (17, 9, 12), (15, 15, 7)], ids=str)
def test_fmg_by_position_is_fmg_pa_ref(dims, mode):
    f = S.noise(dims, 9, 100.0)
    s = S.Session(dims, mode, 2, 2, 0.8, 0.7)
    s.set_field(0, "f", f)
    s.set_weights(PRE, POST)
    aligned = S.start_level(dims) == len(s.ld) - 1
    assert (S.refusal(s, "fmg", 1) is None) == aligned
    s.set_fmg_prolong("position")
    assert s.fmg_start_level() == s.nl - 1
    assert (S.refusal(s, "fmg", 1) is None) == aligned  # a non-aligned transition needs the POSITION transfers too
    s.set_transfer("position")
    res = s.fmg(1)
    want_v, want_res = fmg_pa_ref.fmg(dims, mode, 1, PRE, POST, 0.7, f0=f)
    assert norms_close(res, want_res, 1e-13 if mode == O.LINEAR else 1e-12)
    same(s.field(0, "v"), want_v, "level-0 v")


# ---- load / store, refusals ------------------------------------------------------------------------------------------------
def test_load_and_store():
    s = S.Session((6, 5, 4), O.LINEAR)
    ring = S.noise((6, 5, 4), 1, 1.0) + 3.0  # a field with a non-zero ring
    s.set_field(0, "f", ring)
    a = np.random.default_rng(2).uniform(-100.0, 100.0, (6, 5, 4))
    s.load(0, "f", a, "float32", -0.375, order="xyz", strided=True, side=True)
    got = s.field(0, "f")
    same(got[1:-1, 1:-1, 1:-1], np.float64(-0.375) * a.astype(np.float32).astype(np.float64), "the interior")
    keep = np.ones_like(ring, dtype=bool)
    keep[1:-1, 1:-1, 1:-1] = False
    assert (got[keep] == ring[keep]).all()  # the ring keeps its values
    out = s.store(0, "f", "float32", 0.5)
    assert out.dtype == np.float32 and (out == (np.float64(0.5) * got[1:-1, 1:-1, 1:-1]).astype(np.float32)).all()
    same(s.store(0, "f"), got[1:-1, 1:-1, 1:-1], "scale 1, float64: the words themselves")
    with pytest.raises(AssertionError):
        s.load(0, "newtonV", a)
    n = S.Session((6, 5, 4), O.NEWTON)
    n.load(0, "newtonV", 0.001 * a)
    same(n.field(0, "newtonV")[1:-1, 1:-1, 1:-1], 0.001 * a, "newtonV")
    # a load specifies its field
    t = S.Session((12, 10, 8), O.LINEAR)
    t.set_transfer("position")
    t.pcg(2, 0.0)
    for name in ("v", "f"):
        assert not t.specified(1, name)
        t.load(1, name, np.zeros(t.ld[1]))
        assert t.specified(1, name)


def test_refusals_are_the_headers():
    iso = S.Session((12, 10, 8), O.LINEAR, 2, 2)
    assert "align" in S.refusal(iso, "fmg", 1) and "POSITION" in S.refusal(iso, "pcg")
    iso.set_transfer("position")
    assert S.refusal(iso, "pcg") is None
    iso.set_weights((0.9, 0.6), (0.9, 0.7))
    assert "permutation" in S.refusal(iso, "pcg")
    iso.refused(("pcg",))
    with pytest.raises(AssertionError, match="not refused"):
        iso.refused(("set_smoother", "zline"))
    assert "pre = post" in S.refusal(S.Session((15, 15, 15), O.LINEAR, 2, 1), "pcg")
    assert "pre = post" in S.refusal(S.Session((15, 15, 15), O.LINEAR, 0, 0 + 1), "pcg")
    values, offsets = S.FAMILIES["UPLO"]
    uplo = S.Session((15, 15, 15), O.LINEAR, 2, 2, stencil=stencil(values, offsets))
    assert "symmetric" in S.refusal(uplo, "pcg") and S.refusal(uplo, "set_smoother", "zline") is None
    for mode in (O.NONLINEAR, O.NEWTON):
        n = S.Session((15, 15, 15), mode)
        assert "LINEAR" in S.refusal(n, "pcg") and "LINEAR" in S.refusal(n, "set_smoother", "zline")
        assert "LINEAR" in S.refusal(n, "set_smoother", "auto") and S.refusal(n, "set_smoother", "jacobi") is None
    assert "NEWTON" in S.refusal(S.Session((15, 15, 15), O.NEWTON), "fmg", 1)
    weak = S.Session((15, 15, 15), O.LINEAR, stencil=stencil((1.9, -0.05, -0.05, -0.05, -0.05, -1.0, -1.0)))
    assert S.refusal(weak, "set_smoother", "zline") and S.refusal(weak, "set_smoother", "auto")


# ---- the generator -----------------------------------------------------------------------------------------------------
def test_the_earlier_sessions_did_not_move():
    assert hashlib.sha256(repr(S.cases()).encode()).hexdigest() == CASES_DIGEST


@functools.lru_cache(maxsize=None)
def resolved():
    return [S.resolve_features(S.FEATURE_SEED, i) for i in range(S.FEATURE_N)]


def test_feature_cases_are_a_pure_function_of_the_seed():
    assert S.feature_cases() == S.feature_cases() and len(S.feature_cases()) == S.FEATURE_N == 96
    assert S.draw_features(S.FEATURE_SEED, 7, 1) == S.draw_features(S.FEATURE_SEED, 7, 1) != S.draw_features(S.FEATURE_SEED, 7, 0)
    assert S.feature_cases(3, S.FEATURE_SEED + 1) == S.feature_cases(3, S.FEATURE_SEED + 1) != S.feature_cases(3)
    assert len({S.feature_case_id(c) for c in S.feature_cases()}) == S.FEATURE_N
    assert S.FEATURE_SEED != S.SEED


def test_the_committed_table_of_feature_redraws_is_the_models():
    got = [c for c, _, _ in resolved()]
    assert {c["idx"]: c["attempt"] for c in got if c["attempt"]} == S.FEATURE_REDRAWS
    assert got == S.feature_cases()
    rejected = collections.Counter(r for _, why, _ in resolved() for r in why)
    print("rejected draws:", dict(rejected))
    assert 10 * len(S.FEATURE_REDRAWS) <= S.FEATURE_N  # at most one session in ten is a redraw


def test_feature_generator_conditions():
    modes = collections.Counter(c["mode"] for c in S.feature_cases())
    print("modes:", dict(modes))
    assert modes[O.LINEAR] >= 0.72 * S.FEATURE_N and modes[O.NONLINEAR] >= 5 and modes[O.NEWTON] >= 5
    shapes = {"xy": {s for s, _ in S.XY_POOL}, "xyz": {s for s, _ in S.XYZ_POOL}}
    new = {"pcg", "set_smoother", "set_fmg_prolong", "load", "store", "refused"}
    for c, _, stops in resolved():
        kinds = [op[0] for op in c["ops"]]
        assert c["dims"] in shapes[c["coarsen"]] and set(c["env"]) <= set(S.SWITCHES) and c["family"] in S.FAMILIES
        assert (c["values"], c["offsets"]) == tuple(tuple(x) for x in S.FAMILIES[c["family"]])
        assert c["maxiter"] <= 5 and len(stops) == kinds.count("solve") + kinds.count("pcg")
        drawn = [k for k in kinds if k not in ("set_field", "load")]
        if c["mode"] == O.NEWTON:
            assert kinds[-2:] == ["solve", "store"] and kinds.count("solve") == 1 and c["coarsen"] == "xyz"
            assert set(kinds[:-2]) <= {"set_weights", "set_transfer", "set_fmg_prolong", "load"}
            assert all(op[2] == "newtonV" for op in c["ops"] if op[0] in ("load", "store"))
            continue
        assert len(drawn) <= 12, kinds
        if c["mode"] == O.NONLINEAR:
            assert c["coarsen"] == "xyz" and not {"pcg", "set_smoother"} & set(kinds)
            assert sum({"solve": c["maxiter"], "vcycle": 1, "vcycle_from": 1, "fmg": 2}.get(k, 0) for k in kinds) <= 4
            assert all(op[1][0] in ("fmg", "pcg", "set_smoother") for op in c["ops"] if op[0] == "refused")
        for op in c["ops"]:
            if op[0] in ("load", "store"):
                how = op[5:] if op[0] == "load" else op[3:]
                assert how[0] in S.DTYPES and how[1] in S.IO_SCALES and how[2] in ("zyx", "xyz")
    assert any(new & {op[0] for op in c["ops"]} for c in S.feature_cases())
    loads = [op for c in S.feature_cases() for op in c["ops"] if op[0] == "load"]
    assert 0.2 <= np.mean([op[8] for op in loads]) <= 0.47 and 0.35 <= np.mean([op[9] for op in loads]) <= 0.65


def test_feature_regimes_the_draw_decides_are_reached():
    count = collections.Counter()
    for c, _, stops in resolved():
        count.update(k for k, v in S.feature_regimes(c, stops).items() if v)
    print("sessions per regime:", dict(count))
    for k in S.feature_regimes(S.feature_cases()[0], (False,) * 20):
        assert count[k] >= 5, count
