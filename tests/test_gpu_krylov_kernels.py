"""The launchers of include/gpusolve_krylov.h through the C ABI, in the layout harness of tests/layout_field.py: every
word outside an input's padded box a NaN, outputs NaN-poisoned whole; the written set is exactly the interior, inputs
come back word for word, and every value is bit-identical to the numpy expression the header states (the operator:
the CPU oracle's apply_op with gamma = 0). Dot products: within the standard any-order bound of the exactly rounded
sum (pcg_ref.dot_bound), and the same bits on a second run.

Shapes: the smallest at which each kernel can go wrong — one point, one pair, odd sizes, a wave plus a ragged pair
(129, 130), several x-blocks with a one-column last block (513, 2000) — and 257 x 17 x 501 for the four instances of
the z-march (three x-blocks with a one-column last one, three y-blocks with a one-row last one, 126 chunks of four
planes with a one-plane last one), selected through the launcher's own predicate; every shape in all five layouts, so
the z-march too runs with a plane pitch that is not ldy * (ny + 2) (`loose`) and with outputs whose phase differs from
the inputs' (`mixed`)."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import gpusolve as gsv  # noqa: E402
import oracle as O  # noqa: E402
import pcg_ref as P  # noqa: E402
from gpusolve import _abi as A  # noqa: E402
from layout_field import LAYOUT_IDS, POISON_OUT, LayoutField, layouts  # noqa: E402

EINVAL = A.GS_EINVAL
SMALL = [(1, 1, 1), (2, 1, 1), (7, 7, 7), (33, 17, 9), (129, 5, 3), (130, 5, 3), (513, 3, 4), (2000, 3, 5)]
BIG = (257, 17, 501)
PERM = [gsv.CANONICAL_OFFSETS[i] for i in (3, 0, 2, 6, 4, 1, 5)]
STENCILS = {
    "unit": ((6, -1, -1, -1, -1, -1, -1), list(gsv.CANONICAL_OFFSETS)),
    "general": (P.ANISO, list(gsv.CANONICAL_OFFSETS)),
    # a symmetric stencil in another order: weights follow their offsets
    "permuted": (tuple((4.1, -1.0, -1.0, -1.0, -1.0, -0.05, -0.05)[i] for i in (3, 0, 2, 6, 4, 1, 5)), PERM),
}
KR = None


def kr():
    global KR
    if KR is None:
        assert torch.cuda.is_available(), "GPU tests need a GPU (no CPU fallback exists)"
        KR = gsv.krylov()
    return KR


def st():
    return torch.cuda.current_stream().cuda_stream


def sid(shape):
    return "x".join(str(n) for n in shape)


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def same(a, b, what):
    ne = bits(a) != bits(b)
    assert not ne.any(), f"{what}: {int(ne.sum())} words differ, first at {tuple(np.argwhere(ne)[0])}"


def rand(shape, seed, scale=1.0):
    a = np.zeros(tuple(n + 2 for n in shape))
    P.inner(a)[...] = np.random.default_rng(seed).uniform(-scale, scale, shape)  # mixed signs: sum|ab| >> |sum ab|
    return a


def dev(values):
    return torch.tensor(list(values), dtype=torch.float64, device="cuda")


class Parts:
    """n partial sums between poisoned guards."""

    def __init__(self, n):
        self.n = n
        self.t = torch.zeros(n + 16, dtype=torch.float64, device="cuda")
        self.t.view(torch.int64).fill_(POISON_OUT)
        self.ptr = self.t.data_ptr() + 64

    def check(self, what):
        torch.cuda.synchronize()
        w = self.t.view(torch.int64).cpu().numpy()
        assert (w[:8] == POISON_OUT).all() and (w[8 + self.n:] == POISON_OUT).all(), f"{what}: a guard was written"
        assert (w[8:8 + self.n] != POISON_OUT).all(), f"{what}: a partial was not written"


def finish(parts, what=A.GS_PCG_RR):
    """The partials' sum as gs_pcg_scalars forms it (GS_PCG_RR stores the sum as it is when finite)."""
    rec = dev([1.0, 0, 0, 0, 0, 0, 0, 0])
    assert kr().gs_pcg_scalars(what, parts.ptr, parts.n, rec.data_ptr(), None, st()) == 0
    torch.cuda.synchronize()
    return rec.cpu().numpy()


def check_dot(got, a, b, n, what):
    exact, sabs = P.dot(a, b)
    print(f"{what}: device {got!r} exact {exact!r} bound {P.dot_bound(n, sabs):.3e} sum|ab| {sabs:.3e}")
    assert abs(got - exact) <= P.dot_bound(n, sabs), what


def field(shape, lay, arr, out):
    f = LayoutField(*shape, lay.ldy, lay.ldz, lay.phase_out if out else lay.phase_in)
    if out:
        return f.poison_all()
    return f.from_xyz(arr).poison_outside_box().snapshot()


def run_dir(shape, lid, sname, first, beta=-0.37):
    values, offsets = STENCILS[sname]
    S, So = gsv.Stencil(list(values), offsets).to_abi(), O.Stencil.make(values, offsets)
    lay = layouts(*shape)[lid]
    n = shape[0] * shape[1] * shape[2]
    h = 1.0 / (shape[1] + 1)
    za, pa = rand(shape, 1 + n), rand(shape, 2 + n, 3.0)
    z, p = field(shape, lay, za, False), field(shape, lay, pa, False)
    L = z.level(h)
    b = dev([beta])
    npart = kr().gs_pcg_dir_num_partials(C.byref(S), C.byref(L))
    want_p = za.copy() if first else za + beta * pa
    want_q = O.apply_op(np.ascontiguousarray(want_p), h, 0.0, So)
    got = []
    for rep in range(2):
        pout, q, parts = field(shape, lay, None, True), field(shape, lay, None, True), Parts(npart)
        rc = kr().gs_pcg_dir(C.byref(S), C.byref(L), z.ptr, None if first else p.ptr, pout.ptr, q.ptr,
                             None if first else b.data_ptr(), parts.ptr, st())
        what = f"gs_pcg_dir {sid(shape)} {lid} {sname} first={first}"
        assert rc == 0, what
        pout.assert_written_exactly(pout.interior_mask(), what + " p_out")
        q.assert_written_exactly(q.interior_mask(), what + " q")
        z.assert_unchanged(what=what + " z")
        p.assert_unchanged(what=what + " p_in")
        parts.check(what)
        gp, gq = pout.to_xyz(), q.to_xyz()
        same(P.inner(gp), P.inner(want_p), what + " p_out")
        same(P.inner(gq), P.inner(want_q), what + " q")
        got.append(finish(parts)[A.GS_PCG_RR_I])
    check_dot(got[0], want_p, want_q, n, what)
    assert bits(np.array(got[0])) == bits(np.array(got[1])), "the dot product is not the same on a second run"
    return S, L


@pytest.mark.parametrize("lid", LAYOUT_IDS)
@pytest.mark.parametrize("shape", SMALL, ids=sid)
def test_pcg_dir(shape, lid):
    for sname in STENCILS:
        for first in (False, True):
            S, L = run_dir(shape, lid, sname, first)
            assert kr().gs_pcg_dir_kernel(C.byref(S), C.byref(L), int(first)).decode() == \
                f"k_pcg_dir_gen<{'true' if first else 'false'}>"


@pytest.mark.parametrize("lid", LAYOUT_IDS)
@pytest.mark.parametrize("sname,first", [("unit", False), ("unit", True), ("general", False), ("general", True)])
def test_pcg_dir_zmarch(sname, first, lid):
    S, L = run_dir(BIG, lid, sname, first)
    un = "true" if sname == "unit" else "false"
    assert kr().gs_pcg_dir_kernel(C.byref(S), C.byref(L), int(first)).decode() == \
        f"k_pcg_dir_rb<{un}, {'true' if first else 'false'}>"


# the z-march's chunk is pass_plan's (nz * tiles / 2048 in 4..32): BIG runs its minimum only. Two thin levels of
# tests/test_gpu_rb_pass.py, shape: (chunk, blocks) — an odd chunk (the step whose results are discarded, in every
# chunk) and the 32-plane cap, both with a last chunk of one plane
THIN = {(3, 2, 14337): (7, 2049), (2, 3, 65537): (32, 2049)}


@pytest.mark.parametrize("lid", ["default", "tight_odd"])
@pytest.mark.parametrize("sname,first", [("unit", False), ("general", True)])
@pytest.mark.parametrize("shape", THIN, ids=sid)
def test_pcg_dir_zmarch_chunks(shape, sname, first, lid):
    zc, blocks = THIN[shape]
    values, offsets = STENCILS[sname]
    S = gsv.Stencil(list(values), offsets).to_abi()
    lay = layouts(*shape)[lid]
    L = gsv.gs_level(*shape, lay.ldy, lay.ldz, 0, 1.0 / (shape[1] + 1))
    # one x-y tile: the number of partials is the number of chunks, which only this chunk length gives
    assert blocks == -(-shape[2] // zc) and len({-(-shape[2] // c) for c in (zc - 1, zc, zc + 1)}) == 3
    assert kr().gs_pcg_dir_num_partials(C.byref(S), C.byref(L)) == blocks
    un = "true" if sname == "unit" else "false"
    assert kr().gs_pcg_dir_kernel(C.byref(S), C.byref(L), int(first)).decode() == \
        f"k_pcg_dir_rb<{un}, {'true' if first else 'false'}>"
    run_dir(shape, lid, sname, first)


def test_pcg_dir_first_is_beta_zero_and_aliasing_is_refused():
    shape = (33, 17, 9)
    values, offsets = STENCILS["unit"]
    S = gsv.Stencil(list(values), offsets).to_abi()
    lay = layouts(*shape)["default"]
    za, pa = rand(shape, 5), rand(shape, 6)
    z, p = field(shape, lay, za, False), field(shape, lay, pa, False)
    L = z.level(1.0 / 18)
    npart = kr().gs_pcg_dir_num_partials(C.byref(S), C.byref(L))
    b = dev([0.0])
    outs = []
    for pin in (None, p.ptr):
        pout, q, parts = field(shape, lay, None, True), field(shape, lay, None, True), Parts(npart)
        assert kr().gs_pcg_dir(C.byref(S), C.byref(L), z.ptr, pin, pout.ptr, q.ptr, b.data_ptr(), parts.ptr, st()) == 0
        outs.append((pout.to_xyz(), q.to_xyz(), finish(parts)[A.GS_PCG_RR_I]))
    same(P.inner(outs[0][0]), P.inner(outs[1][0]), "p_out, p_in = NULL against beta = 0")
    same(P.inner(outs[0][1]), P.inner(outs[1][1]), "q, p_in = NULL against beta = 0")
    assert outs[0][2] == outs[1][2]
    # aliasing: a block reads its neighbours' old values in its halo, so an in-place update races
    pout, q, parts = field(shape, lay, None, True), field(shape, lay, None, True), Parts(npart)
    args = lambda zz, pi, po, qq: kr().gs_pcg_dir(C.byref(S), C.byref(L), zz, pi, po, qq, b.data_ptr(), parts.ptr, st())
    for bad in ((z.ptr, p.ptr, p.ptr, q.ptr), (z.ptr, p.ptr, z.ptr, q.ptr), (z.ptr, p.ptr, pout.ptr, z.ptr),
                (z.ptr, p.ptr, pout.ptr, p.ptr), (z.ptr, p.ptr, pout.ptr, pout.ptr), (z.ptr, None, z.ptr, q.ptr)):
        assert args(*bad) == EINVAL
    torch.cuda.synchronize()
    z.assert_unchanged(what="refused call, z")
    p.assert_unchanged(what="refused call, p")
    assert bool((pout.i64 == POISON_OUT).all()) and bool((q.i64 == POISON_OUT).all())


@pytest.mark.parametrize("shape,lid", [(s, l) for s in SMALL + [BIG] for l in LAYOUT_IDS],
                         ids=lambda v: v if isinstance(v, str) else sid(v))
def test_pcg_step_and_dot(shape, lid):
    lay = layouts(*shape)[lid]
    n = shape[0] * shape[1] * shape[2]
    xa, ra, pa, qa = (rand(shape, s + n, sc) for s, sc in ((1, 1.0), (2, 100.0), (3, 2.0), (4, 50.0)))
    p, q = field(shape, lay, pa, False), field(shape, lay, qa, False)
    L = p.level(1.0 / (shape[1] + 1))
    npart = kr().gs_pcg_step_num_partials(C.byref(L))
    assert kr().gs_dot_num_partials(C.byref(L)) == npart
    for alpha in (0.61803, 0.0):
        got = []
        for rep in range(2):
            x, r = field(shape, lay, xa, False), field(shape, lay, ra, False)
            parts = Parts(npart)
            a = dev([alpha])
            what = f"gs_pcg_step {sid(shape)} {lid} alpha={alpha}"
            assert kr().gs_pcg_step(C.byref(L), x.ptr, r.ptr, p.ptr, q.ptr, a.data_ptr(), parts.ptr, st()) == 0, what
            p.assert_unchanged(what=what + " p")
            q.assert_unchanged(what=what + " q")
            parts.check(what)
            if alpha == 0.0:
                x.assert_unchanged(what=what + " x")
                r.assert_unchanged(what=what + " r")
                want_x, want_r = xa, ra
            else:
                x.assert_unchanged(~x.interior_mask(), what + " x outside the interior")
                r.assert_unchanged(~r.interior_mask(), what + " r outside the interior")
                want_x, want_r = xa + alpha * pa, ra - alpha * qa
            same(P.inner(x.to_xyz()), P.inner(want_x), what + " x")
            same(P.inner(r.to_xyz()), P.inner(want_r), what + " r")
            got.append(finish(parts)[A.GS_PCG_RR_I])
        check_dot(got[0], want_r, want_r, n, what + " r.r")
        assert bits(np.array(got[0])) == bits(np.array(got[1]))
    # gs_dot
    got = []
    for rep in range(2):
        parts = Parts(npart)
        assert kr().gs_dot(C.byref(L), p.ptr, q.ptr, parts.ptr, st()) == 0
        parts.check("gs_dot")
        got.append(finish(parts)[A.GS_PCG_RR_I])
    p.assert_unchanged(what="gs_dot a")
    q.assert_unchanged(what="gs_dot b")
    exact, sabs = P.dot(pa, qa)
    if n >= 1000:
        assert sabs > 10 * abs(exact)  # the mixed signs cancel: the bound is about the terms, not the sum
    check_dot(got[0], pa, qa, n, f"gs_dot {sid(shape)} {lid}")
    assert bits(np.array(got[0])) == bits(np.array(got[1]))
    # aliasing
    x, r = field(shape, lay, xa, False), field(shape, lay, ra, False)
    parts, a = Parts(npart), dev([0.5])
    for bad in ((x.ptr, x.ptr, p.ptr, q.ptr), (x.ptr, r.ptr, x.ptr, q.ptr), (x.ptr, r.ptr, p.ptr, r.ptr)):
        assert kr().gs_pcg_step(C.byref(L), *bad, a.data_ptr(), parts.ptr, st()) == EINVAL
    x.assert_unchanged(what="refused step, x")
    r.assert_unchanged(what="refused step, r")


def scalars(what, s, rec):
    """rec after gs_pcg_scalars(what) on one partial holding s, and the slot it wrote (GS_PCG_RR)."""
    part, d = dev([s]), dev(rec)
    slot = torch.full((8,), -7.0, dtype=torch.float64, device="cuda")
    assert kr().gs_pcg_scalars(what, part.data_ptr(), 1, d.data_ptr(), slot.data_ptr(), st()) == 0
    torch.cuda.synchronize()
    return d.cpu().numpy(), slot.cpu().numpy()


def test_pcg_scalars_quotients_and_breakdown():
    rz, pq = 0.7310585786300049, 3.3333333333333335
    rec, slot = scalars(A.GS_PCG_PQ, pq, [rz, 0, 0, 0.25, 0, 0, 0, 0])
    assert rec[A.GS_PCG_PQ_I] == pq and rec[A.GS_PCG_ALPHA_I] == rz / pq and rec[A.GS_PCG_FLAG_I] == 0.0
    assert (slot == -7.0).all()  # only GS_PCG_RR writes the slot
    new = 0.1234567890123
    rec, _ = scalars(A.GS_PCG_RZ, new, [rz, pq, rz / pq, 0, 0, 0, 0, 0])
    assert rec[A.GS_PCG_BETA_I] == new / rz and rec[A.GS_PCG_RZ_I] == new and rec[A.GS_PCG_FLAG_I] == 0.0
    rec, slot = scalars(A.GS_PCG_RR, 2.5, [rz, pq, 0.2, 0.3, 0, 0, 0, 0])
    assert rec[A.GS_PCG_RR_I] == 2.5 and list(slot[:6]) == [rz, pq, 0.2, 0.3, 2.5, 0.0]
    rec, _ = scalars(A.GS_PCG_RZ_FIRST, 4.0, [9, 9, 9, 9, 9, 3, 9, 9])
    assert list(rec) == [4.0, 0, 0, 0, 0, 0, 0, 0]
    # the fixed-order sum of many partials, against the exact one
    vals = np.random.default_rng(4).uniform(-1, 1, 5000)
    part, d = dev(vals), dev([1.0, 0, 0, 0, 0, 0, 0, 0])
    assert kr().gs_pcg_scalars(A.GS_PCG_RR, part.data_ptr(), 5000, d.data_ptr(), None, st()) == 0
    torch.cuda.synchronize()
    got = d.cpu().numpy()[A.GS_PCG_RR_I]
    assert abs(got - math.fsum(vals)) <= P.dot_bound(5000, math.fsum(np.abs(vals)))
    # breakdown: the quotient is 0, the flag is set, nothing non-finite is stored
    for s in (0.0, -1.0, math.nan, math.inf):
        rec, _ = scalars(A.GS_PCG_PQ, s, [rz, 0, 0.5, 0.25, 0, 0, 0, 0])
        assert np.isfinite(rec).all() and rec[A.GS_PCG_ALPHA_I] == 0.0, s
        assert int(rec[A.GS_PCG_FLAG_I]) & A.GS_PCG_BAD_PQ, s
    for s in (0.0, -1.0):
        rec, _ = scalars(A.GS_PCG_RZ, s, [rz, pq, 0.5, 0.25, 0, 0, 0, 0])
        assert np.isfinite(rec).all() and rec[A.GS_PCG_BETA_I] == 0.0 and int(rec[A.GS_PCG_FLAG_I]) & A.GS_PCG_BAD_RZ
        rec, _ = scalars(A.GS_PCG_RZ_FIRST, s, [rz, pq, 0.5, 0.25, 0, 0, 0, 0])
        assert np.isfinite(rec).all() and rec[A.GS_PCG_BETA_I] == 0.0 and int(rec[A.GS_PCG_FLAG_I]) == A.GS_PCG_BAD_RZ
    # r . r that is not finite: stored as 0 with its own flag bit, in the record and in the slot the host reads
    for s in (math.nan, math.inf, -math.inf):
        rec, slot = scalars(A.GS_PCG_RR, s, [rz, pq, 0.2, 0.3, 0, 0, 0, 0])
        assert np.isfinite(rec).all() and np.isfinite(slot).all(), s
        assert rec[A.GS_PCG_RR_I] == 0.0 and int(rec[A.GS_PCG_FLAG_I]) == A.GS_PCG_BAD_RR, s
        assert slot[A.GS_PCG_RR_I] == 0.0 and int(slot[A.GS_PCG_FLAG_I]) == A.GS_PCG_BAD_RR, s
    rec, slot = scalars(A.GS_PCG_RR, 0.0, [rz, pq, 0.2, 0.3, 0, 0, 0, 0])  # a residual that vanished is no breakdown
    assert rec[A.GS_PCG_RR_I] == 0.0 and rec[A.GS_PCG_FLAG_I] == 0.0 and slot[A.GS_PCG_FLAG_I] == 0.0
    # the flag is sticky: a good sum after a breakdown still gives 0
    rec, _ = scalars(A.GS_PCG_PQ, pq, [rz, 0, 0, 0, 0, float(A.GS_PCG_BAD_RZ), 0, 0])
    assert rec[A.GS_PCG_ALPHA_I] == 0.0 and int(rec[A.GS_PCG_FLAG_I]) == A.GS_PCG_BAD_RZ
    assert kr().gs_pcg_scalars(7, None, 0, dev([0] * 8).data_ptr(), None, st()) == EINVAL
