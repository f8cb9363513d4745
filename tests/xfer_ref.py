"""numpy restatement of the position-aware grid transfers (include/gpusolve_transfer.h) and the V-cycle / Newton
iteration composed of them and the CPU oracle's jacobi, residual and apply_op — the reference of
tests/test_transfer_cpu.py and tests/test_gpu_transfer.py (TEST INFRASTRUCTURE ONLY; the product never imports it).

Tables and operators are the header's definitions in the header's evaluation order; numpy rounds every product and
sum once, as the kernels do under -ffp-contract=off, so the two agree bit for bit. Arrays are padded and indexed
[x][y][z] (the oracle's layout).

The composition is tests/weights_ref.py's Cycle (pinned to oracle.Grid.vcycle()) with the transfers chosen per
transition, as the driver chooses them in POSITION mode: an aligned transition (fine n = 2 coarse n + 1 on all three
axes) keeps the oracle's restrict / interpolate, every other one takes the operators below. transfer="reference"
keeps the oracle's everywhere."""
import numpy as np

import oracle as O
import weights_ref
from fmg_ref import level_dims


def axis_tables(n):
    """The closed form of gs_transfer_axis for fine n -> coarse m = n // 2: dict of pj, pt (n + 2 entries), rlo, rcnt
    (m + 2) and rw ((m + 2, 4))."""
    n = int(n)
    m, D = n // 2, n + 1
    i = np.arange(n + 2, dtype=np.int64)
    q = i * (m + 1)
    pj, rem = q // D, q % D
    pt = rem.astype(np.float64) / np.float64(D)
    pj[[0, n + 1]] = 0
    pt[[0, n + 1]] = 0.0
    rem[[0, n + 1]] = 0
    pa = 1.0 - pt
    s = np.float64(m + 1) / np.float64(D)
    rlo, rcnt, rw = np.zeros(m + 2, np.int32), np.zeros(m + 2, np.int32), np.zeros((m + 2, 4))
    # coarse J gathers the fine k with pj[k] == J (weight s * pa[k]) or pj[k] == J - 1 and rem[k] > 0 (s * pt[k]):
    # all (J, k, weight) pairs at once, ascending in k within every J (a long axis has too many for a loop per J)
    k = np.arange(1, n + 1, dtype=np.int64)
    up = k[rem[1:n + 1] > 0]
    J = np.concatenate([pj[k], pj[up] + 1])
    fi = np.concatenate([k, up])
    w = np.concatenate([s * pa[k], s * pt[up]])
    keep = (J >= 1) & (J <= m)  # the coarse ring gathers nothing
    J, fi, w = J[keep], fi[keep], w[keep]
    order = np.lexsort((fi, J))
    J, fi, w = J[order], fi[order], w[order]
    first = np.searchsorted(J, np.arange(1, m + 1))
    count = np.searchsorted(J, np.arange(1, m + 1), side="right") - first
    assert ((count >= 1) & (count <= 4)).all(), n
    slot = np.arange(J.size) - first[J - 1]
    assert (fi == fi[first][J - 1] + slot).all(), n  # consecutive fine points
    rlo[1:m + 1], rcnt[1:m + 1] = fi[first], count
    rw[J, slot] = w
    return {"pj": pj.astype(np.int32), "pt": pt, "rlo": rlo, "rcnt": rcnt, "rw": rw}


_cache = {}


def tables(n):
    if n not in _cache:
        _cache[n] = axis_tables(n)
    return _cache[n]


def aligned(fine, coarse):
    return all(f == 2 * c + 1 for f, c in zip(fine, coarse))


def _prolong_axis(d, axis, n):
    """(m + 2) padded values along `axis` -> (n + 2): pa[i] * d[pj[i]] + pt[i] * d[pj[i] + 1] at i = 1..n, ring 0."""
    T = tables(n)
    d = np.moveaxis(d, axis, 0)
    out = np.zeros((n + 2,) + d.shape[1:])
    sh = (n,) + (1,) * (d.ndim - 1)
    j = T["pj"][1:n + 1].astype(np.int64)
    pt = T["pt"][1:n + 1].reshape(sh)
    pa = 1.0 - pt
    out[1:n + 1] = pa * d[j] + pt * d[j + 1]
    return np.moveaxis(out, 0, axis)


def prolong(d, fine_dims):
    """P d of a padded coarse array: X, then Y, then Z pass; the fine ring is 0 (the kernel leaves it alone)."""
    a = np.asarray(d, dtype=np.float64)
    for axis in range(3):
        a = _prolong_axis(a, axis, fine_dims[axis])
    return np.ascontiguousarray(a)


def _restrict_axis(r, axis, n):
    T = tables(n)
    m = n // 2
    r = np.moveaxis(r, axis, 0)
    out = np.zeros((m + 2,) + r.shape[1:])
    sh = (m,) + (1,) * (r.ndim - 1)
    lo, cnt = T["rlo"][1:m + 1].astype(np.int64), T["rcnt"][1:m + 1]
    acc = None
    for k in range(4):
        term = T["rw"][1:m + 1, k].reshape(sh) * r[np.minimum(lo + k, n)]
        acc = term if k == 0 else np.where((cnt > k).reshape(sh), acc + term, acc)
    out[1:m + 1] = acc
    return np.moveaxis(out, 0, axis)


def restrict(r, fine_dims):
    """R r of a padded fine array: X, then Y, then Z pass, each the truncated left-to-right sum; coarse ring 0."""
    a = np.asarray(r, dtype=np.float64)
    for axis in range(3):
        a = _restrict_axis(a, axis, fine_dims[axis])
    return np.ascontiguousarray(a)


class Cycle(weights_ref.Cycle):
    """weights_ref.Cycle with the transfers chosen per transition, and NEWTON's inner V-cycle (w: every level's
    linearisation point newtonV)."""

    def __init__(self, dims, mode=O.LINEAR, pre=(0.8, 0.8), post=(0.8, 0.8), gamma=1.0, f0=None, v0=None,
                 transfer="position", w=None, stencil=None):
        inner = O.LINEAR if mode == O.NEWTON else mode
        super().__init__(dims, inner, pre, post, gamma, f0=f0, v0=v0, stencil=stencil)
        self.mode, self.transfer, self.w = mode, transfer, w
        if f0 is None and mode == O.NEWTON:
            self.f[0] = O.rhs(*self.ld[0], mode, gamma)

    def pa(self, l):
        """Whether the transition l -> l + 1 takes the position-aware operators."""
        return self.transfer == "position" and not aligned(self.ld[l], self.ld[l + 1])

    def R(self, l, a):
        return restrict(a, self.ld[l]) if self.pa(l) else O.restrict(np.ascontiguousarray(a), self.ld[l + 1])

    def P(self, l, c):
        """fine-level correction from level l + 1's padded array c."""
        return prolong(c, self.ld[l]) if self.pa(l) else O.interpolate(np.ascontiguousarray(c), self.ld[l])

    def _w(self, l):
        return self.w[l] if self.mode == O.NEWTON else None

    def _smooth(self, l, weights):
        for om in weights:
            self.v[l] = O.jacobi(self.v[l], self.f[l], self.h[l], mode=self.mode, omega=float(om), gamma=self.gamma,
                                 sweeps=1, w=self._w(l), stencil=self.stencil)

    def residual(self, l=0):
        return O.residual(self.v[l], self.f[l], self.h[l], self.mode, self.gamma, w=self._w(l), stencil=self.stencil)

    def vcycle_from(self, root=0):
        nl = len(self.ld)
        rest = [None] * nl
        for l in range(root, nl - 1):
            self._smooth(l, self.pre)
            r, _ = self.residual(l)
            self.f[l + 1] = self.R(l, r)
            if self.mode != O.NONLINEAR:
                self.v[l + 1] = O.zeros(*self.ld[l + 1])
            else:
                rest[l + 1] = self.R(l, self.v[l])
                self.v[l + 1] = rest[l + 1].copy()
                self.f[l + 1] = self.f[l + 1] + O.apply_op(rest[l + 1], self.h[l + 1], self.gamma, self.stencil)
        self._smooth(nl - 1, self.pre + self.post)
        for l in range(nl - 1, root, -1):
            c = self.v[l] - rest[l] if self.mode == O.NONLINEAR else self.v[l]
            self.v[l - 1] = self.v[l - 1] + self.P(l - 1, c)
            self._smooth(l - 1, self.post)


def newton_solve(dims, iters, transfer="position", pre=(0.8, 0.8), post=(0.8, 0.8), gamma=1.0, stencil=None, w0=None):
    """NewtonSolver::solve as oracle/gs_oracle.cpp restates it (inner solve: at most 10 V-cycles, tol 0.1), with the
    transfers chosen per transition: (history, level-0 newtonV). w0: level 0's initial newtonV (default zero)."""
    ld = level_dims(dims)
    h0 = 1.0 / (ld[0][1] + 1)
    F = O.rhs(*ld[0], O.NEWTON, gamma)
    w = [O.zeros(*d) for d in ld]
    if w0 is not None:
        w[0] = np.ascontiguousarray(w0, dtype=np.float64).copy()
    f0, r0 = O.newton_F(w[0], F, h0, gamma, stencil)
    hist = [r0]
    for _ in range(iters):
        c = Cycle(dims, O.NEWTON, pre, post, gamma, f0=f0, transfer=transfer, w=w, stencil=stencil)
        for l in range(1, len(ld) - 1):  # the coarsest level keeps its newtonV
            w[l] = c.R(l - 1, w[l - 1])
        start = c.residual(0)[1]
        for _ in range(10):
            if c.vcycle() <= start / (1.0 / 0.1):
                break
        w[0] = w[0] + c.v[0]
        f0, res = O.newton_F(w[0], F, h0, gamma, stencil)
        hist.append(res)
    return hist, w[0]
