"""The register-blocked z-march (k_rb, gs_device.hpp) against the CPU oracle, field by field.

pass_plan gives a level to k_rb once it has at least 1024 blocks of 4-plane chunks; every other kernel-level oracle
comparison of the suite runs below that threshold and so checks k_generic. The shapes here are thin — few points,
many planes — and all take k_rb (test_plan asserts that through gs_newton_F_update_supported, which returns
pass_plan's choice, and through the partial count, which is k_rb's grid). Together they hit: one column and one row,
a ragged last lane pair, a last x-block of one column (the clamped right-edge column), rows past ny within a wave and
whole idle waves, odd chunk lengths (the step whose results are discarded), the RB_ZCMAX cap, last chunks of 1, 2, 3
and 5 planes, several x- and y-blocks, and the exact fit.

Tolerances (the suite's own, tests/test_gpu_kernels.py): LINEAR fields bit for bit; NONLINEAR / NEWTON fields to 1e-12
of the reference field's maximum (ocml's exp against glibc's); finished norms to 1e-12 relative, against
sqrt(fsum(r_ref^2)) over the oracle's residual field. A LINEAR block's partial sum against math.fsum of the oracle's
r^2 over that block's points: n_block 2^-53 relative, the worst case of any summation order of n_block non-negative
terms. GS_NEWTON_B against GS_NEWTON with the bounds of tests/test_gpu_newton_b.py (1e-13 sweep, 1e-12 residual).

Outputs are allocated full of NaN: whatever a call writes outside the interior (ring, pitch padding, second ghost
planes, the allocation's slack) shows as a word that is no longer NaN."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import gpusolve as gsv  # noqa: E402
from gpusolve.devfield import DevField  # noqa: E402
import oracle as O  # noqa: E402
from conftest import rel  # noqa: E402

# (nx, ny, nz): tiles, zc, blocks
SHAPES = {
    (1, 1, 4093): (1, 4, 1024),  # exactly at the threshold; one column, one row; last chunk 1 plane
    (3, 2, 14337): (1, 7, 2049),  # odd chunk length: a discarded step in every chunk; last chunk 1 plane
    (2, 3, 65537): (1, 32, 2049),  # the RB_ZCMAX cap; last chunk 1 plane
    (127, 9, 2047): (2, 4, 1024),  # half-valid last lane pair; second y-block of one live row; last chunk 3 planes
    (129, 7, 2050): (2, 4, 1026),  # second x-block of one column; a wave with one live row; last chunk 2 planes
    (128, 8, 4096): (1, 4, 1024),  # exact fit on every axis
    (129, 9, 3585): (4, 7, 2052),  # odd chunks with x- and y-block boundaries; last chunk 1 plane
    (257, 17, 1367): (9, 6, 2052),  # three x-blocks, three y-blocks; last chunk 5 planes
}
BELOW = (128, 8, 4092)  # 1023 blocks of 4-plane chunks: k_generic
GENERAL = ((4, -1, -1, -0.5, -0.5, -0.5, -0.5), 0.7, 0.5)  # values (canonical order), omega, gamma
GENERAL_SHAPES = [(127, 9, 2047), (129, 9, 3585)]
NEWTON_B_SHAPES = GENERAL_SHAPES
EXTREME_SHAPE = (127, 9, 2047)
SENTINEL = -12345.678


def sid(shape):
    return "x".join(str(n) for n in shape)


# Module scope: pytest runs the tests of one parameter position together, so a shape's fields and oracle results are
# computed once (the caches below are small). The two shapes of the shorter lists come first for that reason.
by_shape = pytest.mark.parametrize("shape", sorted(SHAPES, key=lambda s: s not in GENERAL_SHAPES), ids=sid,
                                   scope="module")

K = None


def k():
    global K
    if K is None:
        assert torch.cuda.is_available(), "GPU tests need a GPU (no CPU fallback exists)"
        K = gsv.kernels()
    return K


def stream():
    return torch.cuda.current_stream().cuda_stream


def ok(rc):
    assert rc == 0, k().gs_strerror(rc).decode()


def S_abi(values=(6, -1, -1, -1, -1, -1, -1)):
    return gsv.Stencil(list(values), list(gsv.CANONICAL_OFFSETS)).to_abi()


def cdiv(a, b):
    return -(-a // b)


def rb_plan(shape):
    """pass_plan's arithmetic, restated: (tiles, zc, (gx, gy, gz))."""
    nx, ny, nz = shape
    gx, gy = cdiv(nx, 128), cdiv(ny, 8)
    tiles = gx * gy
    zc = min(max(nz * tiles // 2048, 4), 32)
    return tiles, zc, (gx, gy, cdiv(nz, zc))


def dev(arr):
    nx, ny, nz = (s - 2 for s in arr.shape)
    return DevField(nx, ny, nz).from_xyz(arr)


def nan_field(shape):
    return DevField(*shape, fill=np.nan)


def inner(a):
    return a[1:-1, 1:-1, 1:-1]


def outside(fld):
    """Mask over the whole allocation: every word that is not an interior point of the level."""
    m = torch.ones_like(fld.buf, dtype=torch.bool)
    ext = m[fld.origin - fld.ldz: fld.origin + fld.span + fld.ldz].view(fld.nz + 4, fld.ny + 2, fld.ldy)
    ext[2:-2, 1:-1, 1:fld.nx + 1] = False
    return m


def assert_outside_nan(fld, what):
    torch.cuda.synchronize()
    m = outside(fld)
    assert bool(torch.isnan(fld.buf[m]).all()), f"{what}: a word outside the interior was written"
    assert not bool(torch.isnan(fld.buf[~m]).any()), f"{what}: an interior point was not written"


def assert_inner(got, ref, mode, what):
    """Interior of a NaN-ringed output against the reference (tests/test_gpu_kernels.assert_field's bounds)."""
    g, r = inner(got), inner(ref)
    if mode == gsv.GS_LINEAR:
        np.testing.assert_array_equal(g, r, err_msg=what)
    else:
        scale = max(np.abs(r).max(), 1e-300)
        err = np.abs(g - r).max()
        assert err <= 1e-12 * scale, (what, err, scale)


def close(got, ref, bound, what):
    """tests/test_gpu_newton_b.close on the interiors."""
    g, r = inner(got), inner(ref)
    assert np.all(np.isfinite(g)) and np.all(np.isfinite(r)), what
    d, scale = np.abs(g - r).max(), np.abs(r).max()
    assert d <= bound * scale, (what, d, scale)


class Guard:
    """Input fields must come back unchanged, word for word."""

    def __init__(self, *fields):
        self.fields = fields
        self.before = [f.buf.clone() for f in fields]

    def check(self, what):
        torch.cuda.synchronize()
        for i, (f, b) in enumerate(zip(self.fields, self.before)):
            assert f.buf.view(torch.int64).equal(b.view(torch.int64)), f"{what}: input {i} changed"


# ---- seeded fields and oracle results, per shape ----------------------------------------------------------------
# (the tests of one shape run together — the parametrisation's module scope — so these small caches hit)
def _rand(rng, shape, scale):
    a = np.zeros(tuple(n + 2 for n in shape))
    inner(a)[...] = rng.uniform(-scale, scale, shape)
    return a


@functools.lru_cache(maxsize=2)
def _fields(shape):
    """v, f, w: random interior, zero ring; f scaled by 100, w in the Newton modes' range (+-0.8)."""
    rng = np.random.default_rng(shape[0] + 1000 * shape[1] + 1000003 * shape[2])
    out = _rand(rng, shape, 1.0), _rand(rng, shape, 100.0), _rand(rng, shape, 0.8)
    for a in out:
        a.setflags(write=False)
    return out


def _h(shape):
    return 1.0 / (shape[1] + 1)


def _ro(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=8)
def _ref_jacobi(shape, mode, sweeps, zero=False, general=False):
    v0, f0, w0 = _fields(shape)
    if zero:
        v0 = np.zeros_like(v0)
    if general:
        vals, omega, gamma = GENERAL
        return _ro(O.jacobi(v0, f0, _h(shape), mode, omega, gamma, sweeps, stencil=O.Stencil.make(vals)))
    return _ro(O.jacobi(v0, f0, _h(shape), mode, 0.8, 1.0, sweeps, w=w0))


def fsum_norm(r):
    return math.sqrt(math.fsum((inner(r) * inner(r)).ravel().tolist()))


@functools.lru_cache(maxsize=6)
def _ref_residual(shape, mode, zero=False, general=False):
    """(r, sqrt(fsum(r^2))) of the oracle's residual field."""
    v0, f0, w0 = _fields(shape)
    if zero:
        v0 = np.zeros_like(v0)
    if general:
        vals, _, gamma = GENERAL
        r, _ = O.residual(v0, f0, _h(shape), mode, gamma, stencil=O.Stencil.make(vals))
    else:
        r, _ = O.residual(v0, f0, _h(shape), mode, 1.0, w=w0)
    return _ro(r, fsum_norm(r))


@functools.lru_cache(maxsize=2)
def _ref_block_sums(shape):
    """LINEAR: math.fsum of r_ref^2 over each block's points, and the point counts, in k_rb's partial order
    bx + gx (by + gy bz): x in 1 + 128 bx .., y in 1 + 8 by .., z in 1 + zc bz .., cut at the level."""
    r, _ = _ref_residual(shape, gsv.GS_LINEAR)
    sq = inner(r) * inner(r)
    _, zc, (gx, gy, gz) = rb_plan(shape)
    sums, counts = np.empty(gx * gy * gz), np.empty(gx * gy * gz)
    for bz in range(gz):
        for by in range(gy):
            for bx in range(gx):
                blk = sq[128 * bx: 128 * bx + 128, 8 * by: 8 * by + 8, zc * bz: zc * bz + zc]
                i = bx + gx * (by + gy * bz)
                sums[i], counts[i] = math.fsum(blk.ravel().tolist()), blk.size
    return _ro(sums, counts)


def nan_partials(n):
    return torch.full((n + 1,), float("nan"), dtype=torch.float64, device="cuda")


def finish(parts, n):
    out = torch.zeros(1, dtype=torch.float64, device="cuda")
    ok(k().gs_sumsq_finish(parts.data_ptr(), n, out.data_ptr(), 0, stream()))
    return out.item()


def check_partials(parts, shape, norm_ref, what, block_sums=False):
    """Every block's entry finite, the one past the end untouched, the finished norm; block_sums: each block's
    entry against _ref_block_sums (the LINEAR residual of the shape's fields)."""
    n = SHAPES[shape][2]
    norm = finish(parts, n)
    p = parts.cpu().numpy()
    assert np.all(np.isfinite(p[:n])), what
    assert np.isnan(p[n]), f"{what}: partials[{n}] (one past the end) was written"
    print(f"{what}: norm {norm!r}, reference {norm_ref!r}, rel {rel(norm, norm_ref):.3g}")
    assert rel(norm, norm_ref) < 1e-12, what
    if block_sums:
        sums, counts = _ref_block_sums(shape)
        err = np.abs(p[:n] - sums)
        bad = np.nonzero(err > counts * 2.0 ** -53 * sums)[0]
        assert bad.size == 0, (what, bad[:8], p[bad[:8]], sums[bad[:8]])
    return p[:n].copy(), norm


# ---- the plan ---------------------------------------------------------------------------------------------------
def test_plan():
    """Every shape of the table takes k_rb, with the table's tile count, chunk length and block count; the
    1023-block shape takes k_generic (one block per 64 x 4 points of a plane)."""
    S = S_abi()
    for shape, (tiles, zc, blocks) in SHAPES.items():
        L = gsv.gs_level(*shape, *gsv.field_layout(*shape)[:2], 0, _h(shape))
        t, c, (gx, gy, gz) = rb_plan(shape)
        assert (t, c, gx * gy * gz) == (tiles, zc, blocks), shape
        assert t * cdiv(shape[2], 4) >= 1024, shape
        assert k().gs_newton_F_update_supported(C.byref(S), C.byref(L)) == 1, shape
        assert k().gs_residual_num_partials(C.byref(S), C.byref(L)) == blocks, shape
    nx, ny, nz = BELOW
    assert cdiv(nx, 128) * cdiv(ny, 8) * cdiv(nz, 4) == 1023
    L = gsv.gs_level(*BELOW, *gsv.field_layout(*BELOW)[:2], 0, _h(BELOW))
    assert k().gs_newton_F_update_supported(C.byref(S), C.byref(L)) == 0
    assert k().gs_residual_num_partials(C.byref(S), C.byref(L)) == cdiv(nx, 64) * cdiv(ny, 4) * nz


# ---- 1. sweeps --------------------------------------------------------------------------------------------------
@by_shape
def test_sweep(shape):
    """gs_jacobi_sweep in modes 0, 1, 2: one sweep, then a second one on its output."""
    S, h = S_abi(), _h(shape)
    v0, f0, w0 = _fields(shape)
    v, f, w = dev(v0), dev(f0), dev(w0)
    L = v.level(h)
    guard = Guard(v, f, w)
    for mode in (0, 1, 2):
        out1, out2 = nan_field(shape), nan_field(shape)
        ok(k().gs_jacobi_sweep(C.byref(S), C.byref(L), mode, 0.8, 1.0, v.ptr, out1.ptr, f.ptr, w.ptr, stream()))
        assert_outside_nan(out1, f"sweep 1 {shape} m{mode}")
        assert_inner(out1.to_xyz(), _ref_jacobi(shape, mode, 1), mode, f"sweep 1 {shape} m{mode}")
        out1.buf[outside(out1)] = 0.0  # the iterate's ring is read by the next sweep
        ok(k().gs_jacobi_sweep(C.byref(S), C.byref(L), mode, 0.8, 1.0, out1.ptr, out2.ptr, f.ptr, w.ptr, stream()))
        assert_outside_nan(out2, f"sweep 2 {shape} m{mode}")
        assert_inner(out2.to_xyz(), _ref_jacobi(shape, mode, 2), mode, f"sweep 2 {shape} m{mode}")
    guard.check(f"sweep {shape}")


# ---- 2. residual, its partials and norm --------------------------------------------------------------------------
@by_shape
def test_residual(shape):
    """gs_residual in modes 0, 1, 2 with the field r and with r = NULL: the field, the per-block partials, the
    finished norm; twice the same call gives the same partials and norm bit for bit."""
    S, h = S_abi(), _h(shape)
    v0, f0, w0 = _fields(shape)
    v, f, w = dev(v0), dev(f0), dev(w0)
    L = v.level(h)
    n = SHAPES[shape][2]
    guard = Guard(v, f, w)
    for mode in (0, 1, 2):
        r_ref, norm_ref = _ref_residual(shape, mode)
        what = f"residual {shape} m{mode}"
        r = nan_field(shape)
        parts = nan_partials(n)
        ok(k().gs_residual(C.byref(S), C.byref(L), mode, 1.0, v.ptr, f.ptr, w.ptr, r.ptr, parts.data_ptr(), stream()))
        assert_outside_nan(r, what)
        assert_inner(r.to_xyz(), r_ref, mode, what)
        p1, n1 = check_partials(parts, shape, norm_ref, what, mode == 0)
        # r = NULL: the norm alone
        parts0 = nan_partials(n)
        ok(k().gs_residual(C.byref(S), C.byref(L), mode, 1.0, v.ptr, f.ptr, w.ptr, None, parts0.data_ptr(), stream()))
        p0, n0 = check_partials(parts0, shape, norm_ref, what + " r=NULL", mode == 0)
        assert p0.tobytes() == p1.tobytes() and n0 == n1, what + ": r = NULL changed the partials"
        # the same call again
        parts2 = nan_partials(n)
        ok(k().gs_residual(C.byref(S), C.byref(L), mode, 1.0, v.ptr, f.ptr, w.ptr, r.ptr, parts2.data_ptr(), stream()))
        p2, n2 = check_partials(parts2, shape, norm_ref, what + " again", mode == 0)
        assert p2.tobytes() == p1.tobytes() and n2 == n1, what + ": not reproducible"
    guard.check(f"residual {shape}")


@by_shape
def test_sweep_norm_partials(shape):
    """gs_jacobi_sweep_norm: the sweep's field, and partials that are the input iterate's residual."""
    S, h = S_abi(), _h(shape)
    v0, f0, w0 = _fields(shape)
    v, f, w = dev(v0), dev(f0), dev(w0)
    L = v.level(h)
    n = SHAPES[shape][2]
    guard = Guard(v, f, w)
    for mode in (0, 1, 2):
        what = f"sweep_norm {shape} m{mode}"
        got = []
        for _ in range(2):
            out, parts = nan_field(shape), nan_partials(n)
            ok(k().gs_jacobi_sweep_norm(C.byref(S), C.byref(L), mode, 0.8, 1.0, v.ptr, out.ptr, f.ptr, w.ptr,
                                        parts.data_ptr(), stream()))
            assert_outside_nan(out, what)
            assert_inner(out.to_xyz(), _ref_jacobi(shape, mode, 1), mode, what)
            got.append(check_partials(parts, shape, _ref_residual(shape, mode)[1], what, mode == 0))
        assert got[0][0].tobytes() == got[1][0].tobytes() and got[0][1] == got[1][1], what + ": not reproducible"
    guard.check(f"sweep_norm {shape}")


# ---- 3. / 4. the FAS operator and compF ---------------------------------------------------------------------------
@by_shape
def test_apply_op_and_newton_F(shape):
    """gs_apply_op, gs_apply_op_add (in place: fin = out) and gs_newton_F (compF: the NONLINEAR residual of newtonV
    against newtonF, with its norm)."""
    S, h = S_abi(), _h(shape)
    v0, f0, w0 = _fields(shape)
    v, w = dev(v0), dev(w0)
    L = v.level(h)
    a_ref = _ro(O.apply_op(v0, h, 1.0))
    guard = Guard(v, w)
    out = nan_field(shape)
    ok(k().gs_apply_op(C.byref(S), C.byref(L), 1.0, v.ptr, out.ptr, stream()))
    assert_outside_nan(out, f"apply_op {shape}")
    assert_inner(out.to_xyz(), a_ref, gsv.GS_NONLINEAR, f"apply_op {shape}")
    # in place, ring and padding of f a sentinel
    f = dev(f0)
    m = outside(f)
    f.buf[m] = SENTINEL
    ok(k().gs_apply_op_add(C.byref(S), C.byref(L), 1.0, v.ptr, f.ptr, stream()))
    torch.cuda.synchronize()
    assert bool((f.buf[m] == SENTINEL).all()), f"apply_op_add {shape}: a word outside the interior was written"
    assert_inner(f.to_xyz(), f0 + a_ref, gsv.GS_NONLINEAR, f"apply_op_add {shape}")
    # compF
    F = dev(f0)
    guard_F = Guard(F)
    n = SHAPES[shape][2]
    res, parts = nan_field(shape), nan_partials(n)
    ok(k().gs_newton_F(C.byref(S), C.byref(L), 1.0, w.ptr, F.ptr, res.ptr, parts.data_ptr(), stream()))
    assert_outside_nan(res, f"newton_F {shape}")
    f_ref, _ = O.newton_F(w0, f0, h, 1.0)
    assert_inner(res.to_xyz(), f_ref, gsv.GS_NEWTON, f"newton_F {shape}")
    check_partials(parts, shape, fsum_norm(f_ref), f"newton_F {shape}")
    guard.check(f"apply_op / newton_F {shape}")
    guard_F.check(f"newton_F {shape}")


# ---- 5. the zero iterate ------------------------------------------------------------------------------------------
@by_shape
def test_zero_iterate(shape):
    """gs_jacobi_sweep_norm with v_in = NULL (the ZV instances) in modes 0 and 2: the sweep of a zero array, and
    partials that are the zero array's residual."""
    S, h = S_abi(), _h(shape)
    _, f0, w0 = _fields(shape)
    f, w = dev(f0), dev(w0)
    L = f.level(h)
    n = SHAPES[shape][2]
    guard = Guard(f, w)
    for mode in (0, 2):
        what = f"zero iterate {shape} m{mode}"
        out, parts = nan_field(shape), nan_partials(n)
        ok(k().gs_jacobi_sweep_norm(C.byref(S), C.byref(L), mode, 0.8, 1.0, None, out.ptr, f.ptr, w.ptr,
                                    parts.data_ptr(), stream()))
        assert_outside_nan(out, what)
        assert_inner(out.to_xyz(), _ref_jacobi(shape, mode, 1, zero=True), mode, what)
        r_ref, norm_ref = _ref_residual(shape, mode, zero=True)
        check_partials(parts, shape, norm_ref, what)
        out2 = nan_field(shape)
        ok(k().gs_jacobi_sweep_norm(C.byref(S), C.byref(L), mode, 0.8, 1.0, None, out2.ptr, f.ptr, w.ptr, None,
                                    stream()))
        torch.cuda.synchronize()
        assert out2.buf.view(torch.int64).equal(out.buf.view(torch.int64)), what + ": partials = NULL changed the field"
    guard.check(f"zero iterate {shape}")


# ---- 6. a general stencil (the UN = false instances) --------------------------------------------------------------
@pytest.mark.parametrize("shape", GENERAL_SHAPES, ids=sid, scope="module")
def test_general_stencil(shape):
    vals, omega, gamma = GENERAL
    S, h = S_abi(vals), _h(shape)
    v0, f0, _ = _fields(shape)
    v, f = dev(v0), dev(f0)
    L = v.level(h)
    n = SHAPES[shape][2]
    assert k().gs_newton_F_update_supported(C.byref(S), C.byref(L)) == 1
    assert k().gs_residual_num_partials(C.byref(S), C.byref(L)) == n
    guard = Guard(v, f)
    for mode in (0, 1):
        what = f"general {shape} m{mode}"
        out = nan_field(shape)
        ok(k().gs_jacobi_sweep(C.byref(S), C.byref(L), mode, omega, gamma, v.ptr, out.ptr, f.ptr, None, stream()))
        assert_outside_nan(out, what + " sweep")
        assert_inner(out.to_xyz(), _ref_jacobi(shape, mode, 1, general=True), mode, what + " sweep")
        r, parts = nan_field(shape), nan_partials(n)
        ok(k().gs_residual(C.byref(S), C.byref(L), mode, gamma, v.ptr, f.ptr, None, r.ptr, parts.data_ptr(), stream()))
        assert_outside_nan(r, what + " residual")
        r_ref, norm_ref = _ref_residual(shape, mode, general=True)
        assert_inner(r.to_xyz(), r_ref, mode, what + " residual")
        check_partials(parts, shape, norm_ref, what + " residual")
    guard.check(f"general {shape}")


# ---- 7. GS_NEWTON_B -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", NEWTON_B_SHAPES, ids=sid, scope="module")
def test_newton_b_matches_newton(shape):
    """Mode 3 on B = gs_newton_bfac(w) against mode 2 on w (which test_sweep and test_residual pin to the oracle):
    1e-13 of the field's maximum for a sweep, 1e-12 for a residual (tests/test_gpu_newton_b.close)."""
    S, h = S_abi(), _h(shape)
    v0, f0, w0 = _fields(shape)
    v, f, w = dev(v0), dev(f0), dev(w0)
    L = v.level(h)
    b = nan_field(shape)
    ok(k().gs_newton_bfac(C.byref(L), 1.0, w.ptr, b.ptr, stream()))
    guard = Guard(v, f, w, b)
    out2, out3 = nan_field(shape), nan_field(shape)
    ok(k().gs_jacobi_sweep(C.byref(S), C.byref(L), gsv.GS_NEWTON, 0.8, 1.0, v.ptr, out2.ptr, f.ptr, w.ptr, stream()))
    ok(k().gs_jacobi_sweep(C.byref(S), C.byref(L), gsv.GS_NEWTON_B, 0.8, 1.0, v.ptr, out3.ptr, f.ptr, b.ptr,
                           stream()))
    assert_outside_nan(out3, f"mode 3 sweep {shape}")
    close(out3.to_xyz(), out2.to_xyz(), 1e-13, f"mode 3 sweep {shape}")
    # the zero iterate
    ok(k().gs_jacobi_sweep(C.byref(S), C.byref(L), gsv.GS_NEWTON, 0.8, 1.0, None, out2.ptr, f.ptr, w.ptr, stream()))
    ok(k().gs_jacobi_sweep(C.byref(S), C.byref(L), gsv.GS_NEWTON_B, 0.8, 1.0, None, out3.ptr, f.ptr, b.ptr,
                           stream()))
    assert_outside_nan(out3, f"mode 3 zero iterate {shape}")
    close(out3.to_xyz(), out2.to_xyz(), 1e-13, f"mode 3 zero iterate {shape}")
    n = SHAPES[shape][2]
    r2, r3, parts = nan_field(shape), nan_field(shape), nan_partials(n)
    ok(k().gs_residual(C.byref(S), C.byref(L), gsv.GS_NEWTON, 1.0, v.ptr, f.ptr, w.ptr, r2.ptr, None, stream()))
    ok(k().gs_residual(C.byref(S), C.byref(L), gsv.GS_NEWTON_B, 1.0, v.ptr, f.ptr, b.ptr, r3.ptr, parts.data_ptr(),
                       stream()))
    assert_outside_nan(r3, f"mode 3 residual {shape}")
    close(r3.to_xyz(), r2.to_xyz(), 1e-12, f"mode 3 residual {shape}")
    p = parts.cpu().numpy()
    assert np.all(np.isfinite(p[:n])) and np.isnan(p[n])
    guard.check(f"mode 3 {shape}")


# ---- 8. extreme magnitudes ----------------------------------------------------------------------------------------
def test_extreme_magnitudes_linear():
    """The magnitude table of tests/test_gpu_sweep2.test_sweep2_extreme_magnitudes (zeros, denormals, both ends of the
    fast h^2 division's range, 1e300) through one LINEAR sweep of k_rb: NaNs where the oracle has them, every other
    word bit-identical (results: zeros and denormals among them)."""
    shape = EXTREME_SHAPE
    rng = np.random.default_rng(shape[0])
    mags = np.array([0.0, 5e-324, 1e-310, 1e-280, 1e-272, 1.3e-271, 1e-270, 1e-200, 1.0, 1e100, 1e180, 4e180, 5e180,
                     1e200, 1e300])

    def field():
        a = _rand(rng, shape, 1.0)
        inner(a)[...] = np.sign(inner(a)) * rng.choice(mags, shape) * rng.uniform(0.5, 2.0, shape)
        return a

    h = _h(shape)
    v0, f0 = field(), field()
    ref = O.jacobi(v0, f0, h, 0, 0.8, 1.0, 1)
    v, f, out = dev(v0), dev(f0), nan_field(shape)
    S = S_abi()
    ok(k().gs_jacobi_sweep(C.byref(S), C.byref(v.level(h)), 0, 0.8, 1.0, v.ptr, out.ptr, f.ptr, None, stream()))
    got, want = inner(out.to_xyz()), inner(ref)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    m = ~np.isnan(want)
    assert np.array_equal(got[m].view(np.int64), want[m].view(np.int64))
