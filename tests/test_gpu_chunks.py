"""The launch shapes only large levels select: z-chunks above each rule's minimum, on thin levels.

The launchers of the transfer, semi and krylov libraries, the two FMG prolongations and gs_residual_restrict's LDS
kernel derive a z-chunk from the level's size, from the number of x-y tiles and not of points, and every other test
of theirs runs levels small enough for the rule's minimum. Here each runs at chunks above it: the loop over a chunk's
planes, a ragged last chunk of another length, the halo planes a chunk stages at its start, the per-block partial sum
over several planes. A level that is one or two tiles wide and thousands of rows long has the tiles of a 512^3 level
with few points.

Every case first asserts, through the launcher's chunk query (tests/test_chunks_cpu.py holds the queries to the
rules), the chunk it means to reach, the number of chunks and the length of the last one, and prints them. Then the
launcher runs in the layout harness of tests/layout_field.py exactly as in its own test file — inputs NaN-poisoned
outside their box, outputs NaN-poisoned whole, the written set exactly the documented one, inputs unchanged word for
word — in the layouts `default` and `tight_odd`, against the reference and with the tolerance its own file uses:
LINEAR bit for bit, modes 1-3 to 1e-12 of the field's magnitude, dot products per BLOCK within pcg_ref.dot_bound of
math.fsum over that block's points."""
import ctypes as C
import math
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import gpusolve as gsv  # noqa: E402
import oracle as O  # noqa: E402
import pcg_ref as P  # noqa: E402
import fmg_ref  # noqa: E402
import zline_ref as Z  # noqa: E402
import test_gpu_fmg_pa as FQ  # noqa: E402
import test_gpu_krylov_kernels as KK  # noqa: E402
import test_gpu_layouts as LY  # noqa: E402
import test_gpu_semi as XY  # noqa: E402
import test_gpu_transfer as PA  # noqa: E402
from gpusolve import _abi as A  # noqa: E402
from layout_field import layouts  # noqa: E402

LIDS = ("default", "tight_odd")
by_layout = pytest.mark.parametrize("lid", LIDS)


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for name in set(PA.SWITCHES) | set(XY.SWITCHES) | set(FQ.SWITCHES):
        monkeypatch.delenv(name, raising=False)
    assert torch.cuda.is_available(), "GPU tests need a GPU (no CPU fallback exists)"


@pytest.fixture(autouse=True)
def duration(request):
    t = time.perf_counter()
    yield
    print(f"[chunks] {request.node.name}: {time.perf_counter() - t:.2f} s")


def sid(shape):
    return "x".join(str(n) for n in shape)


def half(shape):
    return tuple(n // 2 for n in shape)


def level(nx, ny, nz):
    ldy, ldz, _, _ = gsv.field_layout(nx, ny, nz)
    return gsv.gs_level(nx, ny, nz, ldy, ldz, 0, 1.0 / (ny + 1))


def chunks_of(planes, chunk):
    """(number of chunks, length of the last one)"""
    n = (planes + chunk - 1) // chunk
    return n, planes - (n - 1) * chunk


def claim(what, chunk, planes, want_chunk, want_chunks):
    """The chunk the case means to reach, as the query reports it; want_chunks: every chunk's length."""
    n, last = chunks_of(planes, chunk)
    print(f"[chunks] {what}: chunk {chunk}, {n} chunks over {planes} planes, last {last}")
    assert chunk == want_chunk, (what, chunk)
    assert (n, last) == (len(want_chunks), want_chunks[-1]) and sum(want_chunks) == planes, (what, n, last)
    assert all(c == chunk for c in want_chunks[:-1]), what


# ---- gs_residual_restrict_pa --------------------------------------------------------------------------------------
# fine shape: (chunk in coarse planes, the chunks' lengths, modes). (2, 4096, 30): an odd chunk and a one-plane last
# one; (3, 8193, 91): the cap, y and z not aligned (8193 = 2 * 4096 + 1, 91 = 2 * 45 + 1); (130, 1024, 40): two x-tiles
PA_CASES = {(2, 4096, 30): (7, [7, 7, 1], (0, 1, 3)), (3, 8193, 91): (32, [32, 13], (0,)),
            (130, 1024, 40): (5, [5, 5, 5, 5], (0,))}


@by_layout
@pytest.mark.parametrize("shape", PA_CASES, ids=sid)
def test_residual_restrict_pa(shape, lid):
    chunk, lengths, modes = PA_CASES[shape]
    got = gsv.transfer().gs_residual_restrict_pa_chunk(C.byref(level(*shape)), C.byref(level(*half(shape))))
    claim(f"gs_residual_restrict_pa {sid(shape)}", got, shape[2] // 2, chunk, lengths)
    for mode in modes:
        out, want = PA.Run(shape, lid).fused(mode), PA.ref_fused(shape, mode)
        if mode == 0:
            PA.same(out, want, f"coarse f, {lid}")
        else:  # tests/test_gpu_transfer.py's bound for the modes with an exponential
            d = np.abs(out - want).max()
            print(f"mode {mode}: max difference {d} of {np.abs(want).max()}")
            assert d <= 1e-12 * np.abs(want).max(), (mode, lid)


# ---- gs_residual_restrict_xy --------------------------------------------------------------------------------------
# (2, 8192, 150): the cap; (2, 8192, 19): an odd chunk and a one-plane last one; (131, 1024, 75): two x-tiles
XY_CASES = {(2, 8192, 150): (64, [64, 64, 22]), (2, 8192, 19): (9, [9, 9, 1]),
            (131, 1024, 75): (9, [9] * 8 + [3])}


@by_layout
@pytest.mark.parametrize("shape", XY_CASES, ids=sid)
def test_residual_restrict_xy(shape, lid):
    chunk, lengths = XY_CASES[shape]
    coarse = (shape[0] // 2, shape[1] // 2, shape[2])
    got = gsv.semi().gs_residual_restrict_xy_chunk(C.byref(level(*shape)), C.byref(level(*coarse)))
    claim(f"gs_residual_restrict_xy {sid(shape)}", got, shape[2], chunk, lengths)
    XY.same(XY.Run(shape, lid).fused(), XY.ref_fused(shape), f"coarse f, WEAKZ, {lid}")
    if shape[0] == 2:  # one permuted stencil, on the two thin levels
        values, offsets = Z.permuted(Z.UPLO)
        S = gsv.Stencil(list(values), [tuple(o) for o in offsets]).to_abi()
        XY.same(XY.Run(shape, lid).fused(S), XY.ref_fused(shape, values, offsets), f"coarse f, permuted, {lid}")


# ---- gs_residual_restrict, the LDS kernel k_resrestrict ----------------------------------------------------------
RR_SHAPE = (3, 8193, 23)  # coarse (1, 4096, 11): 1024 tiles, chunk 11 * 1024 / 4096 = 2, six chunks, the last of one


@by_layout
def test_residual_restrict_generic(lid):
    shape, cd = RR_SHAPE, half(RR_SHAPE)
    values, offsets = LY.REORDERED
    S, So = LY.S_abi(values, offsets), O.Stencil.make(values, offsets)
    h = 1.0 / (shape[1] + 1)
    v0, f0, w0 = LY.fields(shape)[:3]
    k = gsv.kernels()
    for mode in (0, 1, 2, 3):
        got = k.gs_residual_restrict_chunk(C.byref(S), C.byref(level(*shape)), C.byref(level(*cd)), mode)
        claim(f"gs_residual_restrict {sid(shape)} m{mode}", got, cd[2], 2, [2, 2, 2, 2, 2, 1])
        wm = LY.w_of(shape, mode)

        def body(R):
            v, f = R.inp(v0, name="v"), R.inp(f0, "noise", "f", name="f")
            w = R.inp(wm, "noise", name="w") if wm is not None else None
            ca, cb = R.out(cd, "coarse_a"), R.out(cd, "coarse_b")
            LY.ok(k.gs_residual_restrict(C.byref(S), C.byref(v.level(h)), mode, LY.GAMMA, v.ptr, f.ptr,
                                         w.ptr if w else None, ca.ptr, cb.ptr, C.byref(ca.level(2 * h)), LY.st()))

        res = LY.both(lid, body, f"residual_restrict {shape} m{mode}")
        rr, _ = O.residual(v0, f0, h, min(mode, 2), LY.GAMMA, w=np.ascontiguousarray(w0), stencil=So)
        ref = LY.inner(O.restrict(rr, cd))
        for n in res:
            if mode == 0:
                LY.same(res[n], ref, f"{n} against the oracle")
            else:  # tests/test_gpu_kernels.py's assert_field
                d, scale = np.abs(res[n] - ref).max(), max(np.abs(ref).max(), 1e-300)
                print(f"mode {mode} {n}: max difference {d} of {scale}")
                assert d <= 1e-12 * scale, (mode, n)


# ---- the two FMG prolongations: the chunk is the device's choice --------------------------------------------------
# 2048 tiles of 128 x 8 fine points: at the minimum chunk more blocks than any capacity (256 units x at most 8 blocks)
FQ_SHAPES = [(2, 16384, 140), (2, 16384, 256)]


@by_layout
@pytest.mark.parametrize("shape", FQ_SHAPES, ids=sid)
def test_fmg_prolong_pa(shape, lid):
    chunk = gsv.transfer().gs_fmg_prolong_pa_chunk(C.byref(level(*shape)), C.byref(level(*half(shape))))
    n, last = chunks_of(shape[2], chunk)
    print(f"[chunks] gs_fmg_prolong_pa {sid(shape)}: the device chose chunk {chunk}, {n} chunks, last {last}")
    assert 16 < chunk <= 128 and chunk % 2 == 0 and n >= 2, chunk
    FQ.same(FQ.inner(FQ.Run(shape, lid).prolong()), FQ.inner(FQ.reference(shape)), f"fine interior, {lid}")


# coarse (1, 4095, nz): 1024 tiles of 64 x 4 cells; 64 and 41 z-cells
FP_SHAPES = [(1, 4095, 63), (1, 4095, 40)]


@by_layout
@pytest.mark.parametrize("cd", FP_SHAPES, ids=sid)
def test_fmg_prolong(cd, lid):
    shape = tuple(2 * n + 1 for n in cd)
    k = gsv.kernels()
    chunk = k.gs_fmg_prolong_chunk(C.byref(level(*cd)), C.byref(level(*shape)))
    n, last = chunks_of(cd[2] + 1, chunk)
    print(f"[chunks] gs_fmg_prolong {sid(cd)}: the device chose chunk {chunk}, {n} chunks of z-cells, last {last}")
    assert 8 < chunk <= 64 and n >= 2, chunk
    c0 = LY.noisy(LY.fields(cd, 5)[0])  # the coarse ring takes part as data

    def body(R):
        c = R.inp(c0, name="coarse")
        out = R.out(shape, "fine")
        LY.ok(k.gs_fmg_prolong(c.ptr, C.byref(c.level(0.2)), out.ptr, C.byref(out.level(0.1)), LY.st()))

    res = LY.both(lid, body, f"fmg_prolong {cd}")
    LY.same(res["fine"], LY.inner(fmg_ref.prolong(c0)), "fmg_prolong against the numpy restatement")


# ---- gs_dot / gs_pcg_step ------------------------------------------------------------------------------------------
# (3, 4096, 8): four exact chunks of two; (3, 4096, 29): an odd chunk, a one-plane last one; (3, 4096, 67): the cap;
# (130, 512, 67): two x-blocks, the second with one valid lane pair (columns 129, 130)
VEC_CASES = {(3, 4096, 8): (2, [2, 2, 2, 2]), (3, 4096, 29): (7, [7, 7, 7, 7, 1]), (3, 4096, 67): (16, [16] * 4 + [3]),
             (130, 512, 67): (4, [4] * 16 + [3])}


def block_sums(t, chunk):
    """Per block of 128 x 4 x chunk points of the products t[x][y][z] (interior): (exact sum, sum of magnitudes,
    points), in the partials' order — x-blocks fastest, then y, then z."""
    nx, ny, nz = t.shape
    out = []
    for z in range(0, nz, chunk):
        for y in range(0, ny, 4):
            for x in range(0, nx, 128):
                b = t[x:x + 128, y:y + 4, z:z + chunk].ravel()
                out.append((math.fsum(b), math.fsum(np.abs(b)), b.size))
    return out


def check_partials(parts, t, chunk, what):
    """Every block's partial against math.fsum over that block's points, to tests/test_gpu_krylov_kernels.py's bound."""
    parts.check(what)
    got = parts.t.cpu().numpy()[8:8 + parts.n]
    want = block_sums(t, chunk)
    assert len(want) == parts.n, (what, len(want), parts.n)
    worst = 0.0
    for i, (g, (exact, sabs, n)) in enumerate(zip(got, want)):
        bound = P.dot_bound(n, sabs)
        worst = max(worst, abs(g - exact) / bound if bound else 0.0)
        assert abs(g - exact) <= bound, f"{what}: partial {i} is {g!r}, exact {exact!r}, bound {bound:.3e}"
    print(f"{what}: {parts.n} partials, the worst at {worst:.3f} of its bound")


@by_layout
@pytest.mark.parametrize("shape", VEC_CASES, ids=sid)
def test_pcg_step_and_dot(shape, lid):
    chunk, lengths = VEC_CASES[shape]
    kr, st = KK.kr(), KK.st
    lay = layouts(*shape)[lid]
    n = shape[0] * shape[1] * shape[2]
    xa, ra, pa, qa = (KK.rand(shape, s + n, sc) for s, sc in ((1, 1.0), (2, 100.0), (3, 2.0), (4, 50.0)))
    p, q = KK.field(shape, lay, pa, False), KK.field(shape, lay, qa, False)
    L = p.level(1.0 / (shape[1] + 1))
    claim(f"gs_pcg_step / gs_dot {sid(shape)}", kr.gs_krylov_vec_chunk(C.byref(L)), shape[2], chunk, lengths)
    npart = kr.gs_pcg_step_num_partials(C.byref(L))
    assert npart == kr.gs_dot_num_partials(C.byref(L)) == -(-shape[0] // 128) * -(-shape[1] // 4) * len(lengths)
    for alpha in (0.61803, 0.0):
        x, r = KK.field(shape, lay, xa, False), KK.field(shape, lay, ra, False)
        parts, a = KK.Parts(npart), KK.dev([alpha])
        what = f"gs_pcg_step {sid(shape)} {lid} alpha={alpha}"
        assert kr.gs_pcg_step(C.byref(L), x.ptr, r.ptr, p.ptr, q.ptr, a.data_ptr(), parts.ptr, st()) == 0, what
        p.assert_unchanged(what=what + " p")
        q.assert_unchanged(what=what + " q")
        if alpha == 0.0:  # a breakdown: nothing is stored
            x.assert_unchanged(what=what + " x")
            r.assert_unchanged(what=what + " r")
            want_x, want_r = xa, ra
        else:
            x.assert_unchanged(~x.interior_mask(), what + " x outside the interior")
            r.assert_unchanged(~r.interior_mask(), what + " r outside the interior")
            want_x, want_r = xa + alpha * pa, ra - alpha * qa
        KK.same(P.inner(x.to_xyz()), P.inner(want_x), what + " x")
        KK.same(P.inner(r.to_xyz()), P.inner(want_r), what + " r")
        check_partials(parts, P.inner(want_r) * P.inner(want_r), chunk, what + " r.r")
        KK.check_dot(KK.finish(parts)[A.GS_PCG_RR_I], want_r, want_r, n, what + " r.r")
    parts = KK.Parts(npart)
    assert kr.gs_dot(C.byref(L), p.ptr, q.ptr, parts.ptr, st()) == 0
    p.assert_unchanged(what="gs_dot a")
    q.assert_unchanged(what="gs_dot b")
    check_partials(parts, P.inner(pa) * P.inner(qa), chunk, f"gs_dot {sid(shape)} {lid}")
    KK.check_dot(KK.finish(parts)[A.GS_PCG_RR_I], pa, qa, n, f"gs_dot {sid(shape)} {lid}")


# ---- the driver sizes and consumes the partials at a chunk above 1 ----------------------------------------------
PCG_DIMS, PCG_ITERS = (7, 511, 127), 3  # ((255, 255, 127) has the same chunk and chunks; its model takes 14 s)


def test_driver_pcg_at_chunk_three():
    """gs_grid_pcg on (7, 511, 127): level 0's element-wise passes take chunk 3 (128 tiles, 127 planes: 43 chunks, the
    last of one plane). Replayed with the device's alpha_k and beta_k the model goes through the same roundings:
    x agrees bit for bit, every recorded sum lies within the any-order bound of the exact one
    (tests/test_gpu_pcg.py)."""
    import test_gpu_pcg as G
    chunk = KK.kr().gs_krylov_vec_chunk(C.byref(level(*PCG_DIMS)))
    claim(f"gs_grid_pcg {sid(PCG_DIMS)}, level 0", chunk, PCG_DIMS[2], 3, [3] * 42 + [1])
    f = P.random_rhs(PCG_DIMS, 77)
    with gsv.HipGridData(gsv.GridParams(maxiter=PCG_ITERS, tol=0.0, gridDim=PCG_DIMS, mode=gsv.GS_LINEAR)) as g:
        g.set_field(0, "f", f)
        assert g.pcg_supported(), g.pcg_refusal
        hist = gsv.HipSolver.pcg(g)
        assert not g.pcg_breakdown
        rec, x = g.pcg_record(), g.field(0, "v").copy()
    assert len(hist) == PCG_ITERS + 1 and len(rec) == PCG_ITERS
    m = P.Pcg(PCG_DIMS, f, None, (0.8, 0.8), (0.8, 0.8), "reference", None)
    _, ref = m.replay([(r["alpha"], r["beta"]) for r in rec])
    G.same(x, m.x, f"x after {PCG_ITERS} iterations")
    n = PCG_DIMS[0] * PCG_DIMS[1] * PCG_DIMS[2]
    for k, (dv, rf) in enumerate(zip(rec, ref)):
        for key in ("rz", "pq", "rr"):
            bound = P.dot_bound(n, rf[key + "_abs"])
            print(f"k={k} {key}: device {dv[key]!r} exact {rf[key]!r} bound {bound:.3e}")
            assert abs(dv[key] - rf[key]) <= bound, (k, key)
        assert dv["flag"] == 0.0 and dv["alpha"] == dv["rz"] / dv["pq"]
        assert dv["beta"] == (0.0 if k == 0 else dv["rz"] / rec[k - 1]["rz"])
        assert hist[k + 1] == math.sqrt(dv["rr"])
