"""Full multigrid on the GPU — the tricubic prolongation kernel (gs_fmg_prolong), the V-cycle rooted below level 0
(gs_grid_vcycle_level), the FMG driver (gs_grid_fmg, GS_FMG) — against the numpy + CPU-oracle restatement of
tests/fmg_ref.py.

Tolerances: the kernel and every LINEAR field bit for bit (the library is built with -ffp-contract=off and the
restatement keeps the kernel's evaluation order); LINEAR norms to 1e-9 relative (only the summation order
differs); NONLINEAR fields to 1e-10 of the field's maximum, the bound tests/test_gpu_solver.py applies to that mode
(ocml's exp against glibc's)."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import gpusolve as gsv  # noqa: E402
from gpusolve.devfield import DevField  # noqa: E402
import oracle as O  # noqa: E402
import fmg_ref as R  # noqa: E402
from conftest import REPO, rel  # noqa: E402

PROBE = os.path.join(REPO, "tests", "fmg_probe.py")


def K():
    assert torch.cuda.is_available(), "GPU tests need a GPU (no CPU fallback exists)"
    return gsv.kernels()


def stream():
    return torch.cuda.current_stream().cuda_stream


def padded(dims, rng):
    """Random interior, zero ring."""
    a = np.zeros(tuple(n + 2 for n in dims))
    a[1:-1, 1:-1, 1:-1] = rng.standard_normal(dims)
    return a


def assert_field(got, ref, mode, what=""):
    if mode == gsv.GS_LINEAR:
        np.testing.assert_array_equal(got, ref, err_msg=what)
    else:
        assert np.abs(got - ref).max() <= 1e-10 * np.abs(ref).max(), (what, np.abs(got - ref).max())


@functools.lru_cache(maxsize=None)
def _ref_fmg(dims, mode, k, pre, post):
    _, v, res = R.fmg(dims, mode=mode, cycles_per_level=k, pre=pre, post=post)
    v.setflags(write=False)
    return v, res


# ---- the kernel -------------------------------------------------------------------------------------------------
# one coarse point (the three-value axis), two (first and last odd point share every value), three (one interior odd
# point), several x-y tiles and z-chunks, unequal axes, and rows that cross the 64-, 128- and 512-point tile edges
SHAPES = [(1, 1, 1), (2, 2, 2), (3, 3, 3), (15, 15, 15), (7, 3, 15), (130, 3, 2), (300, 2, 2)]


@pytest.mark.parametrize("cd", SHAPES)
def test_prolong_bitwise(cd):
    fd = tuple(2 * n + 1 for n in cd)
    c = padded(cd, np.random.default_rng(1000 + sum(cd)))
    fine0 = np.zeros(tuple(n + 2 for n in fd))
    fine0[1:-1, 1:-1, 1:-1] = np.nan
    cf, ff = DevField(*cd).from_xyz(c), DevField(*fd).from_xyz(fine0)
    cl, fl = cf.level(1.0 / (cd[1] + 1)), ff.level(1.0 / (fd[1] + 1))
    assert K().gs_fmg_prolong_supported(C.byref(cl), C.byref(fl)) == 1
    rc = K().gs_fmg_prolong(cf.ptr, C.byref(cl), ff.ptr, C.byref(fl), stream())
    assert rc == 0, K().gs_strerror(rc).decode()
    got = ff.to_xyz()
    ref = R.prolong(c)
    np.testing.assert_array_equal(got[1:-1, 1:-1, 1:-1], ref[1:-1, 1:-1, 1:-1])
    # the ring stays zero, and so does everything else of the allocation (pitch padding, second ghost planes)
    ring = got.copy()
    ring[1:-1, 1:-1, 1:-1] = 0.0
    assert not ring.any()
    whole = ff.zyx_ext.clone()
    whole[2:-2, 1:-1, 1:fd[0] + 1] = 0.0
    assert not bool(whole.any()) and not bool(torch.isnan(whole).any())
    np.testing.assert_array_equal(cf.to_xyz(), c)


def test_prolong_rejects():
    c, f8, f9 = DevField(4, 4, 4), DevField(8, 8, 8), DevField(9, 9, 9)
    cl, l8, l9 = c.level(0.2), f8.level(1 / 9), f9.level(0.1)
    assert K().gs_fmg_prolong_supported(C.byref(cl), C.byref(l8)) == 0
    assert K().gs_fmg_prolong_supported(C.byref(cl), C.byref(l9)) == 1
    assert K().gs_fmg_prolong(c.ptr, C.byref(cl), f8.ptr, C.byref(l8), stream()) == gsv._abi.GS_EINVAL
    assert K().gs_fmg_prolong(None, C.byref(cl), f9.ptr, C.byref(l9), stream()) == gsv._abi.GS_EINVAL
    assert K().gs_fmg_prolong(c.ptr, C.byref(cl), None, C.byref(l9), stream()) == gsv._abi.GS_EINVAL
    assert K().gs_fmg_prolong(c.ptr, None, f9.ptr, C.byref(l9), stream()) == gsv._abi.GS_EINVAL
    assert K().gs_fmg_prolong(c.ptr, C.byref(cl), f9.ptr, None, stream()) == gsv._abi.GS_EINVAL
    torch.cuda.synchronize()
    assert not bool(f8.buf.any()) and not bool(f9.buf.any())


# ---- the V-cycle rooted below level 0 ---------------------------------------------------------------------------
def _coarse_from(dims):
    """The first level of the one-launch coarse end at the default GS_COARSE_POINTS (512 points)."""
    return next(l for l, d in enumerate(R.level_dims(dims)) if l >= 1 and d[0] * d[1] * d[2] <= 512)


@pytest.mark.parametrize("mode", [gsv.GS_LINEAR, gsv.GS_NONLINEAR])
@pytest.mark.parametrize("dims,root", [((31, 31, 31), 1), ((31, 31, 31), 2), ((31, 31, 31), "coarse"),
                                       ((31, 31, 31), "below"), ((31, 15, 63), 1)])
def test_vcycle_level(dims, root, mode):
    cf = _coarse_from(dims)
    assert cf == 2 or dims != (31, 31, 31)
    level = {"coarse": cf, "below": cf + 1}.get(root, root)
    ld = R.level_dims(dims)[level]
    rng = np.random.default_rng(7 * level + mode)
    f, v = padded(ld, rng), padded(ld, rng)
    p = gsv.GridParams(maxiter=1, tol=0.0, gridDim=dims, mode=mode)
    with gsv.HipGridData(p) as g:
        g.set_field(0, "v", padded(dims, rng))
        v0, f0 = g.field(0, "v"), g.field(0, "f")
        g.set_field(level, "f", f)
        g.set_field(level, "v", v)
        gsv.HipSolver.vcycle_from(g, level)
        got = g.field(level, "v")
        np.testing.assert_array_equal(g.field(0, "v"), v0)
        np.testing.assert_array_equal(g.field(0, "f"), f0)
        np.testing.assert_array_equal(g.field(level, "f"), f)
    og = O.Grid(ld, mode=mode, maxiter=1)
    og.field(0, "f")[...] = f
    og.field(0, "v")[...] = v
    og.vcycle()
    assert_field(got, og.field(0, "v"), mode, f"{dims} rooted at {level}")


# ---- the FMG driver ---------------------------------------------------------------------------------------------
def _gpu_fmg(dims, mode, k, pre=2, post=2, f0=None):
    p = gsv.GridParams(maxiter=1, tol=0.0, gridDim=dims, mode=mode, preSmoothing=pre, postSmoothing=post)
    with gsv.HipGridData(p) as g:
        if f0 is not None:
            g.set_field(0, "f", f0)
        res = gsv.HipSolver.fmg(g, k)
        return g.field(0, "v"), res, g.fmg_start_level()


@pytest.mark.parametrize("dims,k,pre,post", [((31, 31, 31), 1, 2, 2), ((31, 31, 31), 2, 2, 2), ((63, 63, 63), 1, 2, 2),
                                             ((63, 63, 63), 2, 2, 2), ((63, 31, 127), 1, 2, 2),
                                             ((31, 31, 31), 1, 1, 1), ((31, 31, 31), 1, 2, 1), ((31, 31, 31), 1, 3, 3)])
def test_fmg_linear_bit_identical(dims, k, pre, post):
    v, res, s = _gpu_fmg(dims, gsv.GS_LINEAR, k, pre, post)
    ref_v, ref_res = _ref_fmg(dims, O.LINEAR, k, pre, post)
    assert s == R.start_level(dims)
    np.testing.assert_array_equal(v, ref_v)
    print(f"{dims} k={k} {pre}+{post}: residual {res!r}, restatement {ref_res!r}")
    assert rel(res, ref_res) < 1e-9


def test_fmg_nonlinear():
    dims = (31, 31, 31)
    v, res, _ = _gpu_fmg(dims, gsv.GS_NONLINEAR, 1)
    ref_v, ref_res = _ref_fmg(dims, O.NONLINEAR, 1, 2, 2)
    assert_field(v, ref_v, gsv.GS_NONLINEAR)
    assert rel(res, ref_res) < 1e-6  # BASELINE's contract for residual norms in the non-linear modes


def test_fmg_honours_uploaded_f():
    dims = (31, 31, 31)
    f0 = padded(dims, np.random.default_rng(31))
    v, res, _ = _gpu_fmg(dims, gsv.GS_LINEAR, 1, f0=f0)
    _, ref_v, ref_res = R.fmg(dims, f0=f0)
    np.testing.assert_array_equal(v, ref_v)
    assert rel(res, ref_res) < 1e-9


def test_fmg_beats_three_cycles_on_gpu():
    dims = (63, 63, 63)
    with gsv.HipGridData(gsv.GridParams(maxiter=3, tol=0.0, gridDim=dims, mode=gsv.GS_LINEAR)) as g:
        plain = gsv.HipSolver.solve(g)
    _, res, _ = _gpu_fmg(dims, gsv.GS_LINEAR, 1)
    print("FMG(1)", res, "plain history", plain)
    assert res < plain[3]


# ---- start level and errors -------------------------------------------------------------------------------------
def test_fmg_95_starts_at_size_two():
    dims = (95, 95, 95)
    v, res, s = _gpu_fmg(dims, gsv.GS_LINEAR, 1)
    assert s == 5 and R.level_dims(dims)[s] == (2, 2, 2)
    ref_v, ref_res = _ref_fmg(dims, O.LINEAR, 1, 2, 2)
    np.testing.assert_array_equal(v, ref_v)
    assert rel(res, ref_res) < 1e-9


@pytest.mark.parametrize("dims,mode,k,msg", [((64, 64, 64), gsv.GS_LINEAR, 1, "2^k - 1"),
                                             ((31, 31, 31), gsv.GS_NEWTON, 1, "NEWTON"),
                                             ((31, 31, 31), gsv.GS_LINEAR, 0, "at least 1")])
def test_fmg_errors_leave_v(dims, mode, k, msg):
    v0 = padded(dims, np.random.default_rng(5))
    with gsv.HipGridData(gsv.GridParams(maxiter=1, tol=0.0, gridDim=dims, mode=mode)) as g:
        g.set_field(0, "v", v0)
        f0 = g.field(0, "f")
        f1 = g.field(1, "f")
        assert g.fmg_start_level() == (4 if (mode, k) == (gsv.GS_LINEAR, 0) else 0)
        with pytest.raises(gsv.GpuSolveError, match=re.escape(msg)) as e:
            gsv.HipSolver.fmg(g, k)
        assert dims != (64, 64, 64) or "do not align" in str(e.value)
        np.testing.assert_array_equal(g.field(0, "v"), v0)
        np.testing.assert_array_equal(g.field(0, "f"), f0)
        np.testing.assert_array_equal(g.field(1, "f"), f1)


# ---- alternative paths and the executable -----------------------------------------------------------------------
_OURS = ("GS_COARSE_POINTS", "GS_TILE_POINTS", "GS_NO_FUSED_SWEEPS", "GS_FMG", "GS_FMG_NT")
_probe_default = {}


def _probe(tmp, what, n, cycles, env_extra):
    out = str(tmp / "probe.npz")
    env = {k: v for k, v in os.environ.items() if k not in _OURS}
    env.update(env_extra)
    r = subprocess.run([sys.executable, PROBE, out, what, str(n), str(cycles)], env=env, capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    d = np.load(out)
    return d["v"], list(d["hist"])


@pytest.mark.parametrize("env", [{"GS_COARSE_POINTS": "0"}, {"GS_TILE_POINTS": "0"}, {"GS_NO_FUSED_SWEEPS": "1"},
                                 {"GS_FMG_NT": "1"}],  # (63^3 stores through the caches by default)
                         ids=lambda e: "_".join(e))
def test_fmg_alternative_paths_bit_identical(tmp_path_factory, env):
    if not _probe_default:
        _probe_default["r"] = _probe(tmp_path_factory.mktemp("d"), "fmg", 63, 1, {})
        np.testing.assert_array_equal(_probe_default["r"][0], _ref_fmg((63, 63, 63), O.LINEAR, 1, 2, 2)[0])
    v0, h0 = _probe_default["r"]
    v, h = _probe(tmp_path_factory.mktemp("s"), "fmg", 63, 1, env)
    assert v.tobytes() == v0.tobytes(), f"{env}: level-0 field differs"
    assert rel(h[0], h0[0]) < 1e-12


def test_executable_fmg_line(tmp_path):
    """GS_FMG=1 GpuSolve-hip, 63^3 LINEAR, tol 0, maxiter 3: the fmg: line, then three iter: lines, their residuals
    the restatement's (FMG(1), then three V-cycles on its level-0 grid) — as printed (six digits), and to 1e-9 in
    the history the same solve returns through the C ABI."""
    dims = (63, 63, 63)
    g, _, res = R.fmg(dims)
    ref = [res] + [g.vcycle() for _ in range(3)]
    p = gsv.GridParams(maxiter=3, tol=0.0, gridDim=dims, mode=gsv.GS_LINEAR)
    conf = tmp_path / "fmg.conf"
    conf.write_text(p.config_text())
    env = {k: v for k, v in os.environ.items() if k not in _OURS}
    env["GS_FMG"] = "1"
    out = subprocess.run([gsv._abi.EXECUTABLE, str(conf)], capture_output=True, text=True, timeout=240, env=env)
    assert out.returncode == 0 and out.stderr == "", out.stderr
    lines = out.stdout.splitlines()
    assert lines[1] == "Solving linear problem" and lines[2].startswith("Inital residual: ")
    m = re.fullmatch(r"fmg: cycles: 1 residual: (\S+) Took \d+ms", lines[3])
    assert m, lines[3]
    its = [re.fullmatch(r"iter: (\d+) residual: (\S+) Took \d+ms", l) for l in lines[4:]]
    assert len(its) == 3 and all(its), lines[4:]
    assert [int(i.group(1)) for i in its] == [0, 1, 2]
    assert [m.group(1)] + [i.group(2) for i in its] == ["%g" % r for r in ref]
    # the reference harness's regex (runExperiments.py:46) does not take the fmg: line for a V-cycle
    assert len(re.findall(r"iter: (\d+) residual: ([\d\.e-]+) Took (\d+)ms", out.stdout)) == 3
    _, hist = _probe(tmp_path, "solve", 63, 3, {"GS_FMG": "1"})
    assert len(hist) == 5
    for a, b in zip(hist[1:], ref):
        assert rel(a, b) < 1e-9, (hist, ref)
    # NEWTON and unaligned grids throw under GS_FMG
    p64 = gsv.GridParams(maxiter=1, tol=0.0, gridDim=(64, 64, 64), mode=gsv.GS_LINEAR)
    conf.write_text(p64.config_text())
    out = subprocess.run([gsv._abi.EXECUTABLE, str(conf)], capture_output=True, text=True, timeout=240, env=env)
    assert "Exception: FMG" in out.stderr and "2^k - 1" in out.stderr and "iter:" not in out.stdout
