"""The per-sweep-weight launchers (`..._w`, include/gpusolve_hip.h) against the unfused sequences they replace, run
with one weight per single sweep: gs_jacobi_sweep2_w / _norm_w against two gs_jacobi_sweep calls, gs_jacobi_sweep3_w
against three, the prolongation pair and the tiled launchers against gs_prolong_add / gs_residual / gs_restrict around
weighted single sweeps, gs_coarse_cycle_w against tests/weights_ref.py. Every fused kernel evaluates the single
sweep's expression v + omega_k * (...) per point, so LINEAR results are compared bit for bit; NONLINEAR and NEWTON
pairs bit for bit too (tests/test_gpu_sweep2.py's bound for the equal-weight pair), GS_NEWTON_B to 1e-13 of the
field's maximum (tests/test_gpu_newton_b.py's bound for a sweep). With equal weights every `_w` launcher writes the
words of the launcher it extends.

Outputs are allocated full of NaN, so a word written outside the interior shows; inputs are compared afterwards."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import gpusolve as gsv  # noqa: E402
from gpusolve.devfield import DevField  # noqa: E402
import oracle as O  # noqa: E402
import weights_ref as W  # noqa: E402
from test_gpu_sweep3 import SHAPES as SWEEP3_SHAPES  # noqa: E402

LINEAR, NONLINEAR, NEWTON, NEWTON_B, NEWTON_G = (gsv.GS_LINEAR, gsv.GS_NONLINEAR, gsv.GS_NEWTON, gsv.GS_NEWTON_B,
                                                  gsv.GS_NEWTON_G)
W2 = (0.57, 1.73)
W3 = (0.53, 0.86, 2.25)
GAMMA = 1.0
UNIT = gsv.Stencil().to_abi()
GENERAL = gsv.Stencil([4, -1, -1, -0.5, -0.5, -0.5, -0.5], list(gsv.CANONICAL_OFFSETS)).to_abi()
EINVAL = gsv._abi.GS_EINVAL


def k():
    assert torch.cuda.is_available(), "GPU tests need a GPU (no CPU fallback exists)"
    return gsv.kernels()


def st():
    return torch.cuda.current_stream().cuda_stream


def ok(rc):
    assert rc == 0, k().gs_strerror(rc).decode()


def arr(*w):
    return (C.c_double * len(w))(*w)


def rand_full(rng, shape, scale=1.0):
    nx, ny, nz = shape
    a = np.zeros((nx + 2, ny + 2, nz + 2))
    a[1:nx + 1, 1:ny + 1, 1:nz + 1] = rng.uniform(-scale, scale, shape)
    return a


def dev(a):
    return DevField(*(s - 2 for s in a.shape)).from_xyz(a)


def nan_field(shape):
    return DevField(*shape, fill=np.nan)


def interior_only(out, shape):
    """The interior of a NaN-allocated output; nothing else of the allocation was written."""
    torch.cuda.synchronize()
    got = out.to_xyz()
    inner = got[1:-1, 1:-1, 1:-1]
    assert not np.isnan(inner).any()
    assert int((~torch.isnan(out.buf)).sum().item()) == shape[0] * shape[1] * shape[2]
    return inner


def fields(shape, mode, seed):
    """(v0, f0, w0) host arrays; w0 is the mode's w operand (newtonV, or the factor B for GS_NEWTON_B / _G)."""
    rng = np.random.default_rng(seed)
    v0, f0 = rand_full(rng, shape, 0.5), rand_full(rng, shape, 100.0 if mode == LINEAR else 2.0)
    w0 = rand_full(rng, shape, 0.8)
    if mode == NEWTON_B:
        w0 = GAMMA * (1 + w0) * np.exp(w0)  # the factor everywhere (ring and padding are never read as B's interior)
    if mode == NEWTON_G:
        w0 = np.full_like(w0, GAMMA)
    return v0, f0, w0


def single_sweeps(S, v0, f0, w0, mode, h, weights, zero=False):
    """One gs_jacobi_sweep per weight; zero: the first reads the zero iterate (v_in = NULL)."""
    shape = tuple(s - 2 for s in v0.shape)
    v, alt, f = dev(np.zeros_like(v0) if zero else v0), DevField(*shape), dev(f0)
    w = dev(w0) if mode >= NEWTON else None
    L = v.level(h)
    m = NEWTON_B if mode == NEWTON_G else mode  # (the single sweep reads the factor field: all gamma)
    for i, om in enumerate(weights):
        vin = None if zero and i == 0 else v.ptr
        ok(k().gs_jacobi_sweep(C.byref(S), C.byref(L), m, om, GAMMA, vin, alt.ptr, f.ptr, w.ptr if w else None, st()))
        v, alt = alt, v
    return v.to_xyz()


def compare(got, want, mode):
    if mode in (NEWTON_B, NEWTON_G):
        d = np.abs(got - want).max()
        print("max difference", d, "of", np.abs(want).max())
        assert d <= 1e-13 * np.abs(want).max()
    else:
        np.testing.assert_array_equal(got, want)


# 1x1x1, a tiny level, ragged rows, whole-wave rows (FX), column blocks (XH; 1030: a last block of six columns)
PAIR_SHAPES = [(1, 1, 1), (2, 5, 3), (100, 7, 9), (128, 8, 8), (256, 12, 9), (513, 5, 6), (1030, 6, 8)]
PAIR_CASES = [(m, z) for m in (LINEAR, NONLINEAR, NEWTON, NEWTON_B, NEWTON_G) for z in (False, True)
              if not (z and m == NONLINEAR)]


@pytest.mark.parametrize("mode,zero", PAIR_CASES)
@pytest.mark.parametrize("shape", PAIR_SHAPES)
def test_sweep2_w_equals_two_weighted_sweeps(shape, mode, zero):
    h = 1.0 / (shape[1] + 1)
    v0, f0, w0 = fields(shape, mode, sum(shape) * 31 + mode)
    want = single_sweeps(UNIT, v0, f0, w0, mode, h, W2, zero)[1:-1, 1:-1, 1:-1]
    v, f, w = dev(v0), dev(f0), dev(w0)
    L = v.level(h)
    wp = w.ptr if mode >= NEWTON else None
    vin = None if zero else v.ptr
    assert k().gs_jacobi_sweep2_supported_mode(C.byref(UNIT), C.byref(L), mode) >= 1
    out = nan_field(shape)
    ok(k().gs_jacobi_sweep2_w(C.byref(UNIT), C.byref(L), mode, arr(*W2), GAMMA, vin, out.ptr, f.ptr, wp, 0, 0, st()))
    compare(interior_only(out, shape), want, mode)
    # with the norm partials: the same field, and the partials of the uniform call (they are the input's norm)
    n = k().gs_jacobi_sweep2_num_partials(C.byref(UNIT), C.byref(L), mode)
    pw = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    pu = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    out_n, out_u = nan_field(shape), nan_field(shape)
    ok(k().gs_jacobi_sweep2_norm_w(C.byref(UNIT), C.byref(L), mode, arr(*W2), GAMMA, vin, out_n.ptr, f.ptr, wp, 0, 0,
                                   pw.data_ptr(), st()))
    ok(k().gs_jacobi_sweep2_norm(C.byref(UNIT), C.byref(L), mode, 0.8, GAMMA, vin, out_u.ptr, f.ptr, wp, 0, 0,
                                 pu.data_ptr(), st()))
    np.testing.assert_array_equal(interior_only(out_n, shape), interior_only(out, shape))
    assert not torch.isnan(pw).any() and torch.equal(pw, pu)
    # equal weights: the words of gs_jacobi_sweep2
    out_e = nan_field(shape)
    ok(k().gs_jacobi_sweep2_w(C.byref(UNIT), C.byref(L), mode, arr(0.8, 0.8), GAMMA, vin, out_e.ptr, f.ptr, wp, 0, 0,
                              st()))
    np.testing.assert_array_equal(interior_only(out_e, shape), interior_only(out_u, shape))
    for d, a in ((v, v0), (f, f0), (w, w0)):
        np.testing.assert_array_equal(d.to_xyz(), a)  # the inputs are left as they were


def test_sweep2_w_general_stencil_and_swapped_weights():
    """The general-stencil instances; and the weights are taken in order (swapped weights give another field)."""
    shape = (129, 13, 10)
    h = 1.0 / 14
    v0, f0, w0 = fields(shape, LINEAR, 5)
    v, f = dev(v0), dev(f0)
    L = v.level(h)
    for wts in (W2, W2[::-1]):
        want = single_sweeps(GENERAL, v0, f0, w0, LINEAR, h, wts)[1:-1, 1:-1, 1:-1]
        out = nan_field(shape)
        ok(k().gs_jacobi_sweep2_w(C.byref(GENERAL), C.byref(L), LINEAR, arr(*wts), 0.5, v.ptr, out.ptr, f.ptr, None,
                                  0, 0, st()))
        np.testing.assert_array_equal(interior_only(out, shape), want)
    a = single_sweeps(GENERAL, v0, f0, w0, LINEAR, h, W2)
    b = single_sweeps(GENERAL, v0, f0, w0, LINEAR, h, W2[::-1])
    assert np.any(a != b)


def test_w_launchers_reject_null_weights():
    shape = (16, 16, 16)
    v, f, out, c = DevField(*shape), DevField(*shape), DevField(*shape), DevField(8, 8, 8)
    L, Lc = v.level(1 / 17.0), c.level(1 / 9.0)
    S = C.byref(UNIT)
    assert k().gs_jacobi_sweep2_w(S, C.byref(L), 0, None, 1.0, v.ptr, out.ptr, f.ptr, None, 0, 0, st()) == EINVAL
    assert k().gs_jacobi_sweep2_norm_w(S, C.byref(L), 0, None, 1.0, v.ptr, out.ptr, f.ptr, None, 0, 0, None,
                                       st()) == EINVAL
    assert k().gs_jacobi_sweep3_w(S, C.byref(L), None, 1.0, v.ptr, out.ptr, f.ptr, st()) == EINVAL
    assert k().gs_jacobi_sweep2_prolong_w(S, C.byref(L), 0, None, 1.0, v.ptr, c.ptr, None, C.byref(Lc), out.ptr, f.ptr,
                                          None, 0, 0, st()) == EINVAL
    assert k().gs_smooth2_restrict_tiled_w(S, C.byref(L), 0, None, 1.0, v.ptr, out.ptr, f.ptr, None, c.ptr,
                                           C.byref(Lc), st()) == EINVAL
    assert k().gs_prolong_smooth2_tiled_w(S, C.byref(L), 0, None, 1.0, v.ptr, c.ptr, C.byref(Lc), out.ptr, f.ptr, None,
                                          st()) == EINVAL
    lv = (gsv._abi.gs_coarse_level * 2)()
    assert k().gs_coarse_cycle_w(S, lv, 1, 0, None, 1.0, 2, 2, None) == EINVAL
    mx = k().gs_max_weights()
    many = arr(*([0.8] * (2 * mx + 2)))
    assert k().gs_coarse_cycle_w(S, lv, 1, 0, many, 1.0, mx + 1, 1, None) == EINVAL  # more than the cap per leg
    assert k().gs_coarse_cycle_w(S, lv, 1, 0, many, 1.0, 1, mx + 1, None) == EINVAL
    assert k().gs_coarse_cycle_w(S, lv, 1, 0, many, 1.0, 0, 0, None) == EINVAL


# ---- the triple -------------------------------------------------------------------------------------------------

def triple_w(S, shape, v0, f0, h, weights, gamma):
    v, f, out = dev(v0), dev(f0), nan_field(shape)
    L = v.level(h)
    assert k().gs_jacobi_sweep3_supported(C.byref(S), C.byref(L)) >= 1
    ok(k().gs_jacobi_sweep3_w(C.byref(S), C.byref(L), arr(*weights), gamma, v.ptr, out.ptr, f.ptr, st()))
    got = interior_only(out, shape)
    np.testing.assert_array_equal(v.to_xyz(), v0)
    return got, (v, f, L)


@pytest.mark.parametrize("shape", SWEEP3_SHAPES)
def test_sweep3_w_equals_three_weighted_sweeps(shape):
    h = 1.0 / (shape[1] + 1)
    v0, f0, w0 = fields(shape, LINEAR, sum(s * 1000 ** i for i, s in enumerate(shape)) % 2**32)
    want = single_sweeps(UNIT, v0, f0, w0, LINEAR, h, W3)[1:-1, 1:-1, 1:-1]
    got, (v, f, L) = triple_w(UNIT, shape, v0, f0, h, W3, GAMMA)
    np.testing.assert_array_equal(got, want)
    # equal weights: the words of gs_jacobi_sweep3
    out_e, out_u = nan_field(shape), nan_field(shape)
    ok(k().gs_jacobi_sweep3_w(C.byref(UNIT), C.byref(L), arr(0.8, 0.8, 0.8), GAMMA, v.ptr, out_e.ptr, f.ptr, st()))
    ok(k().gs_jacobi_sweep3(C.byref(UNIT), C.byref(L), 0.8, GAMMA, v.ptr, out_u.ptr, f.ptr, st()))
    np.testing.assert_array_equal(interior_only(out_e, shape), interior_only(out_u, shape))


def test_sweep3_w_general_stencil():
    shape = (129, 13, 40)
    h = 1.0 / 14
    v0, f0, w0 = fields(shape, LINEAR, 77)
    want = single_sweeps(GENERAL, v0, f0, w0, LINEAR, h, W3)[1:-1, 1:-1, 1:-1]
    got, _ = triple_w(GENERAL, shape, v0, f0, h, W3, 0.5)
    np.testing.assert_array_equal(got, want)


# ---- the prolongation pair and the tiled launchers --------------------------------------------------------------

def corrected_then_swept(S, v0, f0, c0, w0, mode, h, weights):
    """gs_prolong_add (interpolate + v += e), then one weighted single sweep per weight."""
    shape = tuple(s - 2 for s in v0.shape)
    v, c = dev(v0), dev(c0)
    ok(k().gs_prolong_add(c.ptr, None, C.byref(c.level(2 * h)), v.ptr, C.byref(v.level(h)), st()))
    return single_sweeps(S, v.to_xyz(), f0, w0, mode, h, weights)[1:-1, 1:-1, 1:-1], shape


PRO_SHAPES = [(16, 16, 16), (13, 9, 11), (1030, 6, 8)]


@pytest.mark.parametrize("mode", [LINEAR, NEWTON, NEWTON_B])
@pytest.mark.parametrize("shape", PRO_SHAPES)
def test_prolong_pair_w(shape, mode):
    h = 1.0 / (shape[1] + 1)
    cd = tuple(s // 2 for s in shape)
    v0, f0, w0 = fields(shape, mode, sum(shape) * 13 + mode)
    c0 = rand_full(np.random.default_rng(sum(shape)), cd, 0.1)
    want, _ = corrected_then_swept(UNIT, v0, f0, c0, w0, mode, h, W2)
    v, f, w, c = dev(v0), dev(f0), dev(w0), dev(c0)
    L, Lc = v.level(h), c.level(2 * h)
    wp = w.ptr if mode >= NEWTON else None
    assert k().gs_jacobi_sweep2_prolong_supported(C.byref(UNIT), C.byref(L), mode) == 1
    n = k().gs_jacobi_sweep2_prolong_ws_elems(C.byref(UNIT), C.byref(L), mode)
    assert (n > 0) == (shape[0] > 512)
    ws = torch.empty(max(n, 1), dtype=torch.float64, device="cuda")
    out, out_e, out_u = nan_field(shape), nan_field(shape), nan_field(shape)
    ok(k().gs_jacobi_sweep2_prolong_ws_w(C.byref(UNIT), C.byref(L), mode, arr(*W2), GAMMA, v.ptr, c.ptr, None,
                                         C.byref(Lc), out.ptr, f.ptr, wp, 0, 0, ws.data_ptr(), n, st()))
    got = interior_only(out, shape)
    compare(got, want, mode)
    if n == 0:  # the call without a workspace is the same launch
        out2 = nan_field(shape)
        ok(k().gs_jacobi_sweep2_prolong_w(C.byref(UNIT), C.byref(L), mode, arr(*W2), GAMMA, v.ptr, c.ptr, None,
                                          C.byref(Lc), out2.ptr, f.ptr, wp, 0, 0, st()))
        np.testing.assert_array_equal(interior_only(out2, shape), got)
    else:
        assert k().gs_jacobi_sweep2_prolong_w(C.byref(UNIT), C.byref(L), mode, arr(*W2), GAMMA, v.ptr, c.ptr, None,
                                              C.byref(Lc), out_e.ptr, f.ptr, wp, 0, 0, st()) == EINVAL
    # equal weights: the words of gs_jacobi_sweep2_prolong_ws
    ok(k().gs_jacobi_sweep2_prolong_ws_w(C.byref(UNIT), C.byref(L), mode, arr(0.8, 0.8), GAMMA, v.ptr, c.ptr, None,
                                         C.byref(Lc), out_e.ptr, f.ptr, wp, 0, 0, ws.data_ptr(), n, st()))
    ok(k().gs_jacobi_sweep2_prolong_ws(C.byref(UNIT), C.byref(L), mode, 0.8, GAMMA, v.ptr, c.ptr, None, C.byref(Lc),
                                       out_u.ptr, f.ptr, wp, 0, 0, ws.data_ptr(), n, st()))
    np.testing.assert_array_equal(interior_only(out_e, shape), interior_only(out_u, shape))
    np.testing.assert_array_equal(v.to_xyz(), v0)


TILED_SHAPES = [(16, 16, 16), (13, 9, 11)]


@pytest.mark.parametrize("mode", [LINEAR, NEWTON, NEWTON_B])
@pytest.mark.parametrize("shape", TILED_SHAPES)
def test_prolong_smooth2_tiled_w(shape, mode):
    h = 1.0 / (shape[1] + 1)
    cd = tuple(s // 2 for s in shape)
    v0, f0, w0 = fields(shape, mode, sum(shape) * 17 + mode)
    c0 = rand_full(np.random.default_rng(sum(shape) + 1), cd, 0.1)
    want, _ = corrected_then_swept(UNIT, v0, f0, c0, w0, mode, h, W2)
    v, f, w, c = dev(v0), dev(f0), dev(w0), dev(c0)
    L, Lc = v.level(h), c.level(2 * h)
    wp = w.ptr if mode >= NEWTON else None
    assert k().gs_tiled_supported(C.byref(UNIT), C.byref(L), mode) == 1
    out, out_e, out_u = nan_field(shape), nan_field(shape), nan_field(shape)
    ok(k().gs_prolong_smooth2_tiled_w(C.byref(UNIT), C.byref(L), mode, arr(*W2), GAMMA, v.ptr, c.ptr, C.byref(Lc),
                                      out.ptr, f.ptr, wp, st()))
    compare(interior_only(out, shape), want, mode)
    ok(k().gs_prolong_smooth2_tiled_w(C.byref(UNIT), C.byref(L), mode, arr(0.8, 0.8), GAMMA, v.ptr, c.ptr, C.byref(Lc),
                                      out_e.ptr, f.ptr, wp, st()))
    ok(k().gs_prolong_smooth2_tiled(C.byref(UNIT), C.byref(L), mode, 0.8, GAMMA, v.ptr, c.ptr, C.byref(Lc), out_u.ptr,
                                    f.ptr, wp, st()))
    np.testing.assert_array_equal(interior_only(out_e, shape), interior_only(out_u, shape))
    np.testing.assert_array_equal(v.to_xyz(), v0)


@pytest.mark.parametrize("zero", [False, True])
@pytest.mark.parametrize("mode", [LINEAR, NEWTON, NEWTON_B])
@pytest.mark.parametrize("shape", TILED_SHAPES)
def test_smooth2_restrict_tiled_w(shape, mode, zero):
    """Against two weighted sweeps + gs_residual + gs_restrict."""
    h = 1.0 / (shape[1] + 1)
    cd = tuple(s // 2 for s in shape)
    ncoarse = cd[0] * cd[1] * cd[2]
    v0, f0, w0 = fields(shape, mode, sum(shape) * 19 + mode)
    swept = single_sweeps(UNIT, v0, f0, w0, mode, h, W2, zero)
    v, f, w, s2 = dev(v0), dev(f0), dev(w0), dev(swept)
    L = v.level(h)
    wp = w.ptr if mode >= NEWTON else None
    r, cref = DevField(*shape), DevField(*cd)
    Lc = cref.level(1.0 / (cd[1] + 1))
    ok(k().gs_residual(C.byref(UNIT), C.byref(L), mode, GAMMA, s2.ptr, f.ptr, wp, r.ptr, None, st()))
    ok(k().gs_restrict(r.ptr, C.byref(L), cref.ptr, C.byref(Lc), st()))
    want_c = cref.to_xyz()[1:-1, 1:-1, 1:-1]
    vin = None if zero else v.ptr

    def run(weights, uniform=False):
        out, cf = nan_field(shape), nan_field(cd)
        if uniform:
            ok(k().gs_smooth2_restrict_tiled(C.byref(UNIT), C.byref(L), mode, 0.8, GAMMA, vin, out.ptr, f.ptr, wp,
                                             cf.ptr, C.byref(Lc), st()))
        else:
            ok(k().gs_smooth2_restrict_tiled_w(C.byref(UNIT), C.byref(L), mode, arr(*weights), GAMMA, vin, out.ptr,
                                               f.ptr, wp, cf.ptr, C.byref(Lc), st()))
        torch.cuda.synchronize()
        assert int((~torch.isnan(cf.buf)).sum().item()) == ncoarse
        return interior_only(out, shape), cf.to_xyz()[1:-1, 1:-1, 1:-1]

    got_v, got_c = run(W2)
    compare(got_v, swept[1:-1, 1:-1, 1:-1], mode)
    if mode == LINEAR:
        np.testing.assert_array_equal(got_c, want_c)
    else:  # (the restricted residual of sweeps that agree to 1e-13: differences of O(1) terms, as test_gpu_newton_b)
        assert np.abs(got_c - want_c).max() <= 1e-12 * max(np.abs(want_c).max(), np.abs(f0).max())
    e_v, e_c = run((0.8, 0.8))
    u_v, u_c = run(None, uniform=True)
    np.testing.assert_array_equal(e_v, u_v)
    np.testing.assert_array_equal(e_c, u_c)
    np.testing.assert_array_equal(v.to_xyz(), v0)


# ---- the one-workgroup coarse cycle -----------------------------------------------------------------------------

def coarse_levels(dims, mode, v0, f0):
    ld = W.level_dims(dims)
    n = len(ld)
    lv = (gsv._abi.gs_coarse_level * n)()
    keep = []
    for l, d in enumerate(ld):
        v = dev(v0) if l == 0 else DevField(*d)
        f = dev(f0) if l == 0 else DevField(*d)
        va, r, rv = DevField(*d), DevField(*d), DevField(*d)
        keep.append((v, va, f, r, rv))
        lv[l].v, lv[l].v_alt, lv[l].f, lv[l].r = v.ptr, va.ptr, f.ptr, r.ptr
        lv[l].rest_v = rv.ptr if mode == NONLINEAR else None
        lv[l].newton_v = None
        lv[l].geom = v.level(1.0 / (d[1] + 1))
        lv[l].v_zero = 0 if (l == 0 or mode == NONLINEAR) else 1
    return lv, keep, ld


@pytest.mark.parametrize("pre,post", [(2, 2), (1, 2), (3, 3)])
@pytest.mark.parametrize("mode", [LINEAR, NONLINEAR])
@pytest.mark.parametrize("dims", [(7, 7, 7), (8, 5, 6)])
def test_coarse_cycle_w(dims, mode, pre, post):
    wts = {1: (1.2,), 2: W2, 3: W3}
    wpre, wpost = wts[pre], tuple(0.9 * x for x in wts[post])  # different weights on the two legs
    rng = np.random.default_rng(sum(dims) + 10 * pre + post + 100 * mode)
    v0, f0 = rand_full(rng, dims, 0.5), rand_full(rng, dims, 2.0)
    ref = W.Cycle(dims, mode, pre=wpre, post=wpost, gamma=GAMMA, f0=f0, v0=v0)
    ref.vcycle_from(0)
    lv, keep, ld = coarse_levels(dims, mode, v0, f0)
    assert len(ld) == 3
    ok(k().gs_coarse_cycle_w(C.byref(UNIT), lv, len(ld), mode, arr(*(wpre + wpost)), GAMMA, pre, post, st()))
    torch.cuda.synchronize()
    for l in range(len(ld)):
        got = keep[l][(pre + post) % 2].to_xyz()  # in v if pre + post is even, else in v_alt
        want = ref.v[l]
        if mode == LINEAR:
            np.testing.assert_array_equal(got[1:-1, 1:-1, 1:-1], want[1:-1, 1:-1, 1:-1], err_msg=f"level {l}")
        elif l == 0:
            assert np.abs(got - want)[1:-1, 1:-1, 1:-1].max() <= 1e-10 * np.abs(want).max()
    # equal weights: the words of gs_coarse_cycle
    lv_e, keep_e, _ = coarse_levels(dims, mode, v0, f0)
    lv_u, keep_u, _ = coarse_levels(dims, mode, v0, f0)
    ok(k().gs_coarse_cycle_w(C.byref(UNIT), lv_e, len(ld), mode, arr(*([0.8] * (pre + post))), GAMMA, pre, post, st()))
    ok(k().gs_coarse_cycle(C.byref(UNIT), lv_u, len(ld), mode, 0.8, GAMMA, pre, post, st()))
    for l in range(len(ld)):
        np.testing.assert_array_equal(keep_e[l][(pre + post) % 2].to_xyz(), keep_u[l][(pre + post) % 2].to_xyz())
