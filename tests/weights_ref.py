"""The V-cycle with one relaxation weight per sweep, composed of the CPU oracle's operators — the reference of
tests/test_weights_cpu.py and the tests/test_gpu_weights*.py files (TEST INFRASTRUCTURE ONLY; the product never
imports it).

It is the recursion of CpuSolver::vcycle (src/cpu/CpuSolver.cpp:85-139) as oracle/gs_oracle.cpp restates it, with
every jacobi(k sweeps, omega) replaced by k calls of oracle.jacobi, one sweep and one weight each: on every level the
k-th pre-smoothing sweep takes pre[k], the k-th post-smoothing sweep post[k], and the coarsest level's pre + post
sweeps (CpuSolver.cpp:117) take the pre weights and then the post weights. LINEAR: the coarse iterate starts at zero.
NONLINEAR (FAS): restV = v_c = R v, f_c = R r + A(restV), correction v_c - restV. h_l = 1 / (ny_l + 1). With equal
weights it is oracle.Grid.vcycle() (tests/test_weights_cpu.py holds it to that, bitwise in LINEAR mode)."""
import numpy as np

import oracle as O
from fmg_ref import level_dims, prolong, start_level


def sweeps(v, f, h, mode, weights, gamma=1.0, stencil=None):
    """One oracle Jacobi sweep per weight, in order."""
    for w in weights:
        v = O.jacobi(v, f, h, mode=mode, omega=float(w), gamma=gamma, sweeps=1, stencil=stencil)
    return v


class Cycle:
    """A level hierarchy for `dims` whose level-0 v and f are the caller's (default: v = 0, the analytic f)."""

    def __init__(self, dims, mode=O.LINEAR, pre=(0.8, 0.8), post=(0.8, 0.8), gamma=1.0, f0=None, v0=None, stencil=None):
        assert mode in (O.LINEAR, O.NONLINEAR)
        self.ld = level_dims(dims)
        self.h = [1.0 / (d[1] + 1) for d in self.ld]
        self.mode, self.gamma, self.stencil = mode, gamma, stencil
        self.pre, self.post = [float(w) for w in pre], [float(w) for w in post]
        self.f = [np.ascontiguousarray(f0, dtype=np.float64).copy() if f0 is not None else O.rhs(*self.ld[0], mode, gamma)]
        self.v = [np.ascontiguousarray(v0, dtype=np.float64).copy() if v0 is not None else O.zeros(*self.ld[0])]
        for d in self.ld[1:]:
            self.f.append(O.zeros(*d))
            self.v.append(O.zeros(*d))

    def _smooth(self, l, weights):
        self.v[l] = sweeps(self.v[l], self.f[l], self.h[l], self.mode, weights, self.gamma, self.stencil)

    def residual(self, l=0):
        return O.residual(self.v[l], self.f[l], self.h[l], self.mode, self.gamma, stencil=self.stencil)

    def vcycle_from(self, root=0):
        """The V-cycle rooted at level `root` (its v and f as they stand), without the closing norm."""
        nl = len(self.ld)
        rest = [None] * nl
        for l in range(root, nl - 1):
            self._smooth(l, self.pre)
            r, _ = self.residual(l)
            self.f[l + 1] = O.restrict(r, self.ld[l + 1])
            if self.mode != O.NONLINEAR:
                self.v[l + 1] = O.zeros(*self.ld[l + 1])
            else:
                rest[l + 1] = O.restrict(self.v[l], self.ld[l + 1])
                self.v[l + 1] = rest[l + 1].copy()
                self.f[l + 1] = self.f[l + 1] + O.apply_op(rest[l + 1], self.h[l + 1], self.gamma, self.stencil)
        self._smooth(nl - 1, self.pre + self.post)
        for l in range(nl - 1, root, -1):
            c = self.v[l] - rest[l] if self.mode == O.NONLINEAR else self.v[l]
            self.v[l - 1] = self.v[l - 1] + O.interpolate(np.ascontiguousarray(c), self.ld[l - 1])
            self._smooth(l - 1, self.post)

    def vcycle(self):
        """One V-cycle from level 0; returns the level-0 residual norm, as oracle.Grid.vcycle()."""
        self.vcycle_from(0)
        return self.residual(0)[1]

    def solve(self, cycles):
        """[initial norm, the norm after each cycle], as oracle.Grid.solve() with tol = 0."""
        hist = [self.residual(0)[1]]
        for _ in range(cycles):
            hist.append(self.vcycle())
        return hist


def fmg(dims, mode=O.LINEAR, cycles_per_level=1, pre=(0.8, 0.8), post=(0.8, 0.8), gamma=1.0, f0=None):
    """tests/fmg_ref.py's fmg() with weighted V-cycles: (level-0 v, the level-0 residual norm)."""
    ld, s = level_dims(dims), start_level(dims)
    assert s > 0, "FMG needs aligned coarse grids (sizes 2^k - 1)"
    f = [np.ascontiguousarray(f0) if f0 is not None else O.rhs(*ld[0], mode, gamma)]
    for l in range(s):
        f.append(O.restrict(f[l], ld[l + 1]))
    v, res = None, None
    for l in range(s, -1, -1):
        v0 = O.zeros(*ld[l])
        if v is not None:
            v0[1:-1, 1:-1, 1:-1] = prolong(v)[1:-1, 1:-1, 1:-1]
        c = Cycle(ld[l], mode, pre, post, gamma, f0=f[l], v0=v0)
        for _ in range(cycles_per_level):
            res = c.vcycle()
        v = c.v[0]
    return v, res
