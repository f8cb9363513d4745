"""Every kernel instance of the product, launched once against the CPU oracle (tests/instance_table.py: one row per
instance of libgpusolve_hip.so and per launchable instance of libgpusolve_transfer.so, at the smallest shape that
selects it).

Per row: LayoutField operands in the default layout, inputs NaN-poisoned outside their padded box, outputs poisoned
whole (tests/test_gpu_layouts.py's Side). The library's launch record names the row's kernel; the return code is 0;
inputs come back unchanged word for word; exactly the documented set is written; the values are the oracle's for the
call: LINEAR bit for bit, modes 1 and 2 within 1e-12 of the reference field's largest magnitude (the suite's bound,
test_gpu_kernels.assert_field), mode 3 within test_gpu_newton_b.close's bounds of the same call in mode 2 on the GPU
(1e-13 for swept fields, 1e-12 for residuals, restricted residuals and norms; B = gamma (1 + w) e^w), that mode-2 run
being held to the oracle. Norm partials sum to the oracle's norm of the input iterate's residual within 1e-12.
The one-workgroup coarse cycle's references are test_gpu_layouts.test_coarse_cycle's: the weighted oracle V-cycle in
LINEAR mode, the per-operator launch sequence bit for bit in modes 1 and 2; its mode-3 run is held to its mode-2 run
at 1e-12, the bound of the residuals it contains."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import gpusolve as gsv  # noqa: E402
import oracle as O  # noqa: E402
import fmg_ref  # noqa: E402
import fmg_pa_ref as PA  # noqa: E402
import instance_table as IT  # noqa: E402
import test_gpu_layouts as LY  # noqa: E402
import weights_ref as W  # noqa: E402
import xfer_ref as X  # noqa: E402
from instance_table import GAMMA, OMEGA, W2, W3, fields, half, inner, w_of  # noqa: E402


class Vec:
    """A small device array (a one-dimensional input or a table)."""

    def __init__(self, data):
        self.t = torch.from_numpy(np.ascontiguousarray(data)).cuda()
        self.ptr = self.t.data_ptr()
        self.snap = self.t.clone()


class GSide(LY.Side):
    """Side plus the one-dimensional operands of the element-wise launchers and the transfer tables."""

    def vec(self, data, name, out=False):
        v = Vec(data)
        self.held.append(v)
        if out:
            self.results[name] = lambda: v.t.cpu().numpy()
        else:
            def check():
                assert torch.equal(v.t.view(torch.uint8), v.snap.view(torch.uint8)), f"input {name} changed"
            self.checks.append(check)
        return v


def st():
    return torch.cuda.current_stream().cuda_stream


def So(row):
    return O.Stencil.make(*IT.STENCILS[row.stencil])


def sweeps(v, f, h, m, weights, s, w):
    for om in weights:
        v = O.jacobi(np.ascontiguousarray(v), f, h, m, float(om), GAMMA, 1, w=w, stencil=s)
    return v


def residual(v, f, h, m, s, w):
    return O.residual(np.ascontiguousarray(v), f, h, m, GAMMA, w=w, stencil=s)[0]


def norm_of(r):
    return math.sqrt(math.fsum((inner(r) * inner(r)).ravel().tolist()))


def operands(row, m, zero=False):
    """v (zeros for a zero iterate), f, the oracle's w (newtonV in mode 2, else none), h."""
    v0, f0, w0 = fields(row.shape)[:3]
    if zero:
        v0 = np.zeros_like(v0)
    return v0, f0, (np.ascontiguousarray(w0) if m == 2 else None), 1.0 / (row.shape[1] + 1)


# ---- the oracle, composed per call: name of a result -> (reference, kind) -------------------------------------------------
# kinds: "exact" (bit for bit in every mode), "sweep" / "residual" (bit for bit in LINEAR mode, else the mode's bound),
# "norm" (the partials' sum against a norm), "tol:<rel>" (a relative bound of the existing test of that launcher)
def ref_pair(row, m):
    v, f, w, h = operands(row, m, row.opts.get("zero", False))
    return {"out": (inner(sweeps(v, f, h, m, W2, So(row), w)), "sweep"),
            "partials": (norm_of(residual(v, f, h, m, So(row), w)), "norm")}


def corrected(row):
    return fields(row.shape)[0] + O.interpolate(np.ascontiguousarray(IT.coarse_of(row.shape)), row.shape)


def ref_prolong(row, m):
    _, f, w, h = operands(row, m)
    return {"out": (inner(sweeps(corrected(row), f, h, m, W2, So(row), w)), "sweep")}


def ref_triple(row, m):
    v, f, _, h = operands(row, 0)
    return {"out": (inner(sweeps(v, f, h, 0, W3, So(row), None)), "sweep")}


def ref_sweep(row, m):
    v, f, w, h = operands(row, m, row.opts.get("zero", False))
    return {"out": (inner(sweeps(v, f, h, m, (OMEGA,), So(row), w)), "sweep"),
            "partials": (norm_of(residual(v, f, h, m, So(row), w)), "norm")}


def ref_residual(row, m):
    v, f, w, h = operands(row, m)
    r = residual(v, f, h, m, So(row), w)
    return {"out": (inner(r), "residual"), "partials": (norm_of(r), "norm")}


def ref_apply_op(row, m):
    u, f, _, h = operands(row, 1)
    a = O.apply_op(np.ascontiguousarray(u), h, GAMMA, So(row))
    return {"out": (inner(f + a if row.opts["add"] else a), "residual")}


def ref_resrestrict(row, m):
    v, f, w, h = operands(row, m)
    c = inner(O.restrict(residual(v, f, h, m, So(row), w), half(row.shape)))
    return {"coarse_a": (c, "residual"), "coarse_b": (c, "residual")}


def ref_tile_pre(row, m):
    v, f, w, h = operands(row, m, row.opts.get("zero", False))
    s = sweeps(v, f, h, m, W2, So(row), w)
    return {"out": (inner(s), "sweep"),
            "coarse_f": (inner(O.restrict(residual(s, f, h, m, So(row), w), half(row.shape))), "residual")}


def ref_tile_pro(row, m):
    return ref_prolong(row, m)


def ref_newton_upd(row, m):
    v0, F0, w0 = fields(row.shape)[:3]
    h, wsum = 1.0 / (row.shape[1] + 1), w0 + 0.25 * v0
    f, _ = O.newton_F(np.ascontiguousarray(wsum), F0, h, GAMMA, So(row))
    ref = {"w_out": (inner(wsum), "exact"), "f": (inner(f), "residual"), "partials": (norm_of(f), "norm")}
    if row.opts["rs"]:
        ref["coarse_w"] = (inner(O.restrict(wsum, half(row.shape))), "exact")
    if row.opts["bf"]:
        ref["b_out"] = (inner(GAMMA * (1.0 + wsum) * np.exp(wsum)), "tol:1e-12")
    return ref


def ref_coarse_cycle(row, m):
    ld = IT.cc_levels(row.shape)
    v0, f0 = fields(ld[0], 3)[0] * 0.5, fields(ld[0], 3)[1] * 0.02
    wpre, wpost = IT.CC_WEIGHTS[:IT.CC_PRE], IT.CC_WEIGHTS[IT.CC_PRE:]
    it = "v_alt" if (IT.CC_PRE + IT.CC_POST) % 2 else "v"
    if m == 0:
        c = W.Cycle(ld[0], 0, pre=wpre, post=wpost, gamma=GAMMA, f0=f0, v0=v0)
        c.vcycle_from(0)
        return {it + str(l): (inner(c.v[l]), "exact") for l in range(len(ld))}
    want = LY.per_operator_cycle("default", ld, m, v0, f0, wpre, wpost)
    return {it + str(l): (x, "exact") for l, x in enumerate(want)}


def ref_prolong_add(row, m):
    c, sub = fields(half(row.shape), 5)[:2]
    d = np.ascontiguousarray(c - sub if row.opts["sub"] else c)
    return {"out": (inner(fields(row.shape)[1] + O.interpolate(d, row.shape)), "exact")}


def ref_fmg_prolong(row, m):
    return {"out": (inner(fmg_ref.prolong(IT.fmg_coarse(row.shape))), "exact")}


def ref_rhs(row, m):
    nx, ny, nz = row.shape
    return {"out": (inner(O.rhs(nx, ny, nz, 0, GAMMA, 1.0 / (ny + 1))), "exact")}


def ref_restrict(row, m):
    return {"out": (inner(O.restrict(fields(row.shape)[0], half(row.shape))), "exact")}


def ref_interpolate(row, m):
    return {"out": (O.interpolate(np.ascontiguousarray(fields(half(row.shape), 5)[0]), row.shape), "exact")}


def ref_bfac(row, m):
    box, lo, hi = IT.bfac_planes(row.shape)
    w = np.concatenate([lo[:, :, None], box, hi[:, :, None]], axis=2)
    return {"out": (GAMMA * (1.0 + w) * np.exp(w), "tol:1e-14")}  # (test_newton_bfac_heads' bound)


def ref_copy(row, m):
    return {"out": (IT.vec_data(row.shape[0]), "exact")}


def ref_fill(row, m):
    return {"out": (np.full(row.shape[0], 2.5), "exact")}


def ref_axpy(row, m):
    n = row.shape[0]
    return {"out": (IT.vec_data(n, 1) + 0.5 * IT.vec_data(n), "exact")}


def ref_sumsq(row, m):
    n = row.shape[0]
    x = IT.vec_data(n) ** 2  # (test_copy_fill_axpy_sumsq's bound: n roundings of the sum)
    return {"out": (np.array([math.sqrt(float(np.sum(x)))]), f"tol:{n * 2.0 ** -52}")}


def ref_resrestrict_pa(row, m):
    v, f, w, h = operands(row, m)
    return {"out": (inner(X.restrict(residual(v, f, h, m, So(row), w), row.shape)), "residual")}


def ref_prolong_add_pa(row, m):
    c, sub = fields(half(row.shape), 5)[:2]
    return {"out": (inner(fields(row.shape)[0] + X.prolong(c - sub if row.opts["sub"] else c, row.shape)), "exact")}


def ref_fmg_prolong_pa(row, m):
    return {"out": (inner(PA.prolong(fields(half(row.shape), 5)[0], row.shape)), "exact")}


def ref_restrict_pa(row, m):
    c = inner(X.restrict(fields(row.shape)[0], row.shape))
    return {"out": (c, "exact"), "out_b": (c, "exact")}


REFS = {n[4:]: f for n, f in list(globals().items()) if n.startswith("ref_")}
assert set(REFS) == set(IT.CALLS)
# results a call also produces that no reference names: the coarse cycle's working fields
UNCOMPARED = {"coarse_cycle"}


def compare(got, ref, kind, linear, what, mode3=False):
    """mode3: `ref` is the same call's mode-2 result on the GPU (test_gpu_newton_b.close's bounds)."""
    if kind == "norm":
        g = math.sqrt(math.fsum(np.asarray(got).ravel().tolist())) if not mode3 else got
        print(f"{what}: norm {g!r}, reference {ref!r}")
        assert abs(g - ref) <= 1e-12 * abs(ref), (what, g, ref)
        return
    assert np.all(np.isfinite(got)), what
    if kind == "exact" or (linear and not mode3 and not kind.startswith("tol:")):
        LY.same(got, ref, what)
        return
    if mode3:
        bound = 1e-13 if kind == "sweep" else 1e-12
    else:
        bound = float(kind[4:]) if kind.startswith("tol:") else 1e-12
    d, scale = np.abs(got - ref).max(), np.abs(ref).max()
    print(f"{what}: max difference {d:.3g} of {scale:.3g}, bound {bound:g} relative")
    assert d <= bound * scale, (what, d, scale)


def run(row, mode):
    R = GSide("default")
    rc, names = IT.launch(row, R, st(), mode)
    if rc not in (0, gsv._abi.GS_EINVAL):  # a HIP error: nothing more may run on this device in this session
        pytest.exit(f"{row}: HIP error {rc} ({gsv.kernels().gs_strerror(rc).decode()})", returncode=3)
    assert rc == 0, (row, rc)
    try:
        res = R.finish()  # (synchronises; the inputs, the written sets)
    except RuntimeError as e:  # the device's report of a fault, at the synchronisation
        pytest.exit(f"{row}: {e}", returncode=3)
    return names, res


def check_row(row):
    names, res = run(row, row.mode)
    assert names == row.launches, (row, names)
    m = row.mode
    ref = REFS[row.call](row, min(m, 2))
    assert set(ref) <= set(res) and (row.call in UNCOMPARED or set(ref) == set(res)), (sorted(ref), sorted(res))
    if m == 3:  # against the same call in mode 2 on the GPU, which is then held to the oracle
        names2, res2 = run(row, 2)
        assert len(names2) == len(names) and names2 != names, (names2, names)
        for n, (_, kind) in ref.items():
            a, bq = res[n], res2[n]
            if kind == "norm":
                a, bq = (math.sqrt(math.fsum(x.ravel().tolist())) for x in (a, bq))
            elif row.call == "coarse_cycle":
                kind = "residual"
            compare(a, bq, kind, False, f"{row.name} {n}: mode 3 against mode 2", mode3=True)
        res, m = res2, 2
    for n, (want, kind) in ref.items():
        compare(res[n], want, kind, m == 0, f"{row.name} {n} against the oracle")


@pytest.mark.parametrize("row", [r for r in IT.rows() if not r.env], ids=lambda r: r.id)
def test_instance(row):
    check_row(row)


def test_instances_under_switches():
    """The six instances that only A/B switches select below 2^25 points: the same checks in one child process."""
    rows = [r for r in IT.rows() if r.env]
    probe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "instance_probe.py")
    r = subprocess.run([sys.executable, probe, "gpu"], env=dict(os.environ, **IT.KNOBS), capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert [l for l in r.stdout.splitlines() if l.startswith("ok ")] == ["ok " + x.name for x in rows]
