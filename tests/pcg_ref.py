"""Conjugate gradients preconditioned by the model V-cycle, on the CPU — the reference of tests/test_pcg_cpu.py and
tests/test_gpu_pcg.py (TEST INFRASTRUCTURE ONLY; the product never imports it).

It is composed of what the driver composes on the device: M^-1 r is tests/xfer_ref.py's Cycle from a
zero iterate with r as right-hand side (vcycle_from(0)), A u is the oracle's LINEAR residual of a zero right-hand side,
negated (apply_op with gamma = 0, bit for bit), the initial residual the oracle's residual, and the updates are numpy expressions that round every product and sum once, as the
kernels do under -ffp-contract=off: p = z + beta * p, x = x + alpha * p, r = r - alpha * q. The dot products are
math.fsum over the interior, i.e. exactly rounded: the device's fixed-order sums differ from them within the standard
bound dot_bound().

Two forms. run() is free-running: alpha and beta are the quotients of its own sums. replay() takes alpha_k and beta_k
from a record (the device's, or run()'s own): every field then goes through the same roundings as on the device, so x
agrees bit for bit, and the sums it reports are the exact ones of those fields. Arrays are padded, [x][y][z]."""
import math

import numpy as np

import oracle as O
import xfer_ref as X

ANISO = (4.1, -1.0, -1.0, -1.0, -1.0, -0.05, -0.05)  # a symmetric stencil on which plain V-cycles stall


def inner(a):
    return a[1:-1, 1:-1, 1:-1]


def dot(a, b):
    """(the exactly rounded a . b over the interior, sum |a_i b_i|)"""
    t = (inner(a) * inner(b)).ravel()  # each product rounded once, as on the device
    return math.fsum(t), math.fsum(np.abs(t))


def dot_bound(n, sum_abs):
    """|any-order floating-point sum of n products - exact sum| <= gamma_n * sum |a_i b_i| with u = 2^-53 (Higham,
    Accuracy and Stability of Numerical Algorithms, §4.2: every summation order)."""
    nu = n * 2.0 ** -53
    return nu / (1.0 - nu) * sum_abs


class Pcg:
    def __init__(self, dims, f, x0=None, pre=(0.8, 0.8), post=(0.8, 0.8), transfer="position", stencil=None, cycle=None):
        """cycle: a factory r -> a Cycle on right-hand side r with a zero iterate (its vcycle_from(0) and v[0] are
        used); None: xfer_ref.Cycle with this object's pre, post, transfer and stencil."""
        self.dims, self.cycle = tuple(dims), cycle
        self.pre, self.post, self.transfer, self.stencil = tuple(pre), tuple(post), transfer, stencil
        self.h = 1.0 / (self.dims[1] + 1)
        self.f = np.ascontiguousarray(f, dtype=np.float64)
        self.x = O.zeros(*self.dims) if x0 is None else np.ascontiguousarray(x0, dtype=np.float64).copy()
        self.n = self.dims[0] * self.dims[1] * self.dims[2]

    def M(self, r):
        """One model V-cycle from the zero iterate on right-hand side r: the preconditioner."""
        if self.cycle is not None:
            c = self.cycle(r)
        else:
            c = X.Cycle(self.dims, O.LINEAR, self.pre, self.post, f0=r, transfer=self.transfer, stencil=self.stencil)
        c.vcycle_from(0)
        return c.v[0]

    def A(self, u):
        """A u as 0 - (0 - A u) of the oracle's LINEAR residual: the same stencil sum and division as apply_op with
        gamma = 0, bit for bit, without its 0 * u * exp(u), which is NaN where |u| is large enough for exp to overflow
        (a preconditioned residual of an unscaled right-hand side is)."""
        u = np.ascontiguousarray(u)
        r, _ = O.residual(u, np.zeros_like(u), self.h, O.LINEAR, stencil=self.stencil)
        return 0.0 - r

    def _start(self):
        self.r, _ = O.residual(self.x, self.f, self.h, O.LINEAR, stencil=self.stencil)
        self.p = None
        return math.sqrt(dot(self.r, self.r)[0])

    def _iterate(self, iters, tol, scalars):
        hist = [self._start()]
        rec = []
        rz_old = None
        for k in range(iters):
            z = self.M(self.r)
            rz, rz_abs = dot(self.r, z)
            if scalars is None:
                if not (0.0 < rz < math.inf):
                    break
                beta = 0.0 if k == 0 else rz / rz_old
            else:
                beta = scalars[k][1]
            self.p = z.copy() if k == 0 else z + beta * self.p
            q = self.A(self.p)
            pq, pq_abs = dot(self.p, q)
            if scalars is None:
                if not (0.0 < pq < math.inf):
                    break
                alpha = rz / pq
            else:
                alpha = scalars[k][0]
            self.x = self.x + alpha * self.p
            self.r = self.r - alpha * q
            rr, rr_abs = dot(self.r, self.r)
            rec.append(dict(rz=rz, pq=pq, alpha=alpha, beta=beta, rr=rr, rz_abs=rz_abs, pq_abs=pq_abs, rr_abs=rr_abs))
            rz_old = rz
            hist.append(math.sqrt(rr))
            if hist[-1] <= hist[0] / (1.0 / tol if tol != 0.0 else math.inf):
                break
        return hist, rec

    def run(self, iters, tol=0.0):
        """Free-running: (history, per-iteration record); the driver's stopping rule res <= r0 / (1 / tol)."""
        return self._iterate(iters, tol, None)

    def replay(self, scalars):
        """Replayed with scalars = [(alpha_k, beta_k), ...] (beta_0 is not used: the first direction is z)."""
        return self._iterate(len(scalars), 0.0, list(scalars))


def vcycles(dims, f, cycles, pre=(0.8, 0.8), post=(0.8, 0.8), transfer="position", stencil=None, x0=None):
    """The stationary iteration PCG is compared with: [initial norm, the norm after each model V-cycle], and x."""
    c = X.Cycle(dims, O.LINEAR, pre, post, f0=f, v0=x0, transfer=transfer, stencil=stencil)
    return c.solve(cycles), c.v[0]


def random_rhs(dims, seed):
    """A right-hand side with mixed signs: interior uniform in (-1, 1), ring zero."""
    f = O.zeros(*dims)
    inner(f)[...] = np.random.default_rng(seed).uniform(-1.0, 1.0, size=tuple(dims))
    return f
