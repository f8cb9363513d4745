"""numpy restatement of the z-line Jacobi smoother (include/gpusolve_line.h) and the V-cycle composed of it and the
CPU oracle's residual / restrict / interpolate — the reference of tests/test_zline_cpu.py and tests/test_gpu_zline.py
(TEST INFRASTRUCTURE ONLY; the product never imports it).

factors() and sweep() are the header's definitions in the header's expression order; numpy rounds every product, sum
and quotient once, as the kernels do under -ffp-contract=off, so the two agree bit for bit. sweep() is vectorised over
the columns and sequential in k. Arrays are padded and indexed [x][y][z] (the oracle's layout).

ZlineMixin overrides the smoothing step of tests/weights_ref.py's and tests/xfer_ref.py's Cycle, so that both run
z-line sweeps between the oracle's (or xfer_ref's position-aware) transfers: ZCycle and ZCyclePa."""
import numpy as np

import oracle as O
import weights_ref
import xfer_ref

STRONGZ = (2.2, -0.05, -0.05, -0.05, -0.05, -1.0, -1.0)   # thin cells in z: the case line relaxation is for
ISO = (6.0, -1.0, -1.0, -1.0, -1.0, -1.0, -1.0)
UPLO = (2.2, -0.05, -0.07, -0.05, -0.03, -1.0, -0.9)      # up != lo, and four different x / y weights
WEAKZ = (4.1, -1.0, -1.0, -1.0, -1.0, -0.05, -0.05)       # DESIGN.md §4.10's stencil: the weak axis is z
PERM = (3, 0, 5, 2, 6, 4, 1)                              # a non-canonical order of the entries


def permuted(values, perm=PERM, offsets=O.CANONICAL):
    """(values, offsets) with the entries in the order perm: weights follow their offsets."""
    return tuple(values[i] for i in perm), [offsets[i] for i in perm]


def shape_of(values, offsets=O.CANONICAL):
    """(s0, up, lo, [(weight, (ox, oy)) of the four x / y entries in config order]); None unless the offsets are the
    seven axis offsets once each."""
    if sorted(tuple(o) for o in offsets) != sorted(O.CANONICAL):
        return None
    s0 = up = lo = None
    xy = []
    for w, (ox, oy, oz) in zip(values, offsets):
        if (ox, oy, oz) == (0, 0, 0):
            s0 = float(w)
        elif oz == 1:
            up = float(w)
        elif oz == -1:
            lo = float(w)
        else:
            xy.append((float(w), (ox, oy)))
    return s0, up, lo, xy


def supported(values, offsets=O.CANONICAL):
    sh = shape_of(values, offsets)
    if sh is None:
        return False
    s0, up, lo, _ = sh
    return bool(s0 != 0.0 and abs(s0) >= abs(up) + abs(lo))


def factors(values, nz, offsets=O.CANONICAL):
    """(cp, den), nz + 2 entries each: den[1] = s0, cp[k] = up / den[k], den[k+1] = s0 - lo * cp[k]; 0 at both ends."""
    s0, up, lo, _ = shape_of(values, offsets)
    s0, up, lo = np.float64(s0), np.float64(up), np.float64(lo)
    cp, den = np.zeros(nz + 2), np.zeros(nz + 2)
    dk = s0
    for k in range(1, nz + 1):
        den[k] = dk
        cp[k] = up / dk
        t = lo * cp[k]
        dk = s0 - t
    return cp, den


def line_solve(b, values, offsets=O.CANONICAL):
    """u of the header's two passes for right-hand sides b shaped (..., nz): d_1 = b_1 / den[1],
    d_k = (b_k - lo * d_{k-1}) / den[k]; u_nz = d_nz, u_k = d_k - cp[k] * u_{k+1}."""
    nz = b.shape[-1]
    _, _, lo, _ = shape_of(values, offsets)
    lo = np.float64(lo)
    cp, den = factors(values, nz, offsets)
    d = np.empty_like(b)
    d[..., 0] = b[..., 0] / den[1]
    for k in range(2, nz + 1):
        t = lo * d[..., k - 2]
        d[..., k - 1] = (b[..., k - 1] - t) / den[k]
    u = np.empty_like(b)
    u[..., nz - 1] = d[..., nz - 1]
    for k in range(nz - 1, 0, -1):
        t = cp[k] * u[..., k]
        u[..., k - 1] = d[..., k - 1] - t
    return u


def sweep(v, f, h, omega, values, offsets=O.CANONICAL):
    """One sweep: the padded v_out (ring zero). v is None: the zero iterate (b = (h*h) * f, v_out = omega * u)."""
    nx, ny, nz = (n - 2 for n in f.shape)
    _, _, _, xy = shape_of(values, offsets)
    hh = np.float64(h) * np.float64(h)
    omega = np.float64(omega)
    b = hh * f[1:-1, 1:-1, 1:-1]
    if v is not None:
        g = None
        for w, (ox, oy) in xy:
            term = np.float64(w) * v[1 + ox:nx + 1 + ox, 1 + oy:ny + 1 + oy, 1:-1]
            g = term if g is None else g + term
        b = b - g
    u = line_solve(b, values, offsets)
    out = np.zeros_like(f)
    if v is None:
        out[1:-1, 1:-1, 1:-1] = omega * u
    else:
        vi = v[1:-1, 1:-1, 1:-1]
        w = u - vi
        t = omega * w
        out[1:-1, 1:-1, 1:-1] = vi + t
    return out


def column_matrix(values, nz, offsets=O.CANONICAL):
    """The tridiagonal matrix a line solve inverts: s0 on the diagonal, up above it, lo below it."""
    s0, up, lo, _ = shape_of(values, offsets)
    return s0 * np.eye(nz) + up * np.eye(nz, k=1) + lo * np.eye(nz, k=-1)


class ZlineMixin:
    """_smooth of a Cycle as z-line sweeps, one per weight (LINEAR only). The stencil is given as values / offsets
    (zvalues, zoffsets); the Cycle's own `stencil` (an oracle.Stencil of the same entries) serves the residual."""

    def _smooth(self, l, weights):
        assert self.mode == O.LINEAR
        for om in weights:
            self.v[l] = sweep(self.v[l], self.f[l], self.h[l], om, self.zvalues, self.zoffsets)


class ZCycle(ZlineMixin, weights_ref.Cycle):
    def __init__(self, dims, values, offsets=O.CANONICAL, pre=(0.8, 0.8), post=(0.8, 0.8), f0=None, v0=None):
        super().__init__(dims, O.LINEAR, pre, post, f0=f0, v0=v0, stencil=O.Stencil.make(values, offsets))
        self.zvalues, self.zoffsets = tuple(values), list(offsets)


class ZCyclePa(ZlineMixin, xfer_ref.Cycle):
    def __init__(self, dims, values, offsets=O.CANONICAL, pre=(0.8, 0.8), post=(0.8, 0.8), f0=None, v0=None,
                 transfer="position"):
        super().__init__(dims, O.LINEAR, pre, post, f0=f0, v0=v0, transfer=transfer,
                         stencil=O.Stencil.make(values, offsets))
        self.zvalues, self.zoffsets = tuple(values), list(offsets)


def cycle(dims, values, zline, **kw):
    """A model cycle on `values` with z-line (zline) or the oracle's point Jacobi sweeps."""
    if zline:
        return ZCycle(dims, values, **kw)
    return weights_ref.Cycle(dims, O.LINEAR, kw.pop("pre", (0.8, 0.8)), kw.pop("post", (0.8, 0.8)),
                             stencil=O.Stencil.make(values), **kw)


def normal_rhs(dims, seed=1):
    """The right-hand side of DESIGN.md §4.11's figures: default_rng(seed).standard_normal on the interior, ring 0."""
    f = O.zeros(*dims)
    f[1:-1, 1:-1, 1:-1] = np.random.default_rng(seed).standard_normal(tuple(dims))
    return f


def factors_per_cycle(c, cycles=8):
    """The residual-reduction factor of each of `cycles` cycles: [r1 / r0, r2 / r1, ...]."""
    hist = c.solve(cycles)
    return [b / a for a, b in zip(hist, hist[1:])]


def pcg_iterations(dims, values, f, zline, tol=1e-8, maxiter=60):
    """Iterations conjugate gradients preconditioned by one model cycle (from zero) need for ||r|| <= tol ||r0||:
    tests/pcg_ref.py's run() with the preconditioner swapped."""
    import pcg_ref as P

    class Z(P.Pcg):
        def M(self, r):
            c = cycle(self.dims, values, zline, f0=r)
            c.vcycle_from(0)
            return c.v[0]

    hist, _ = Z(dims, f, stencil=O.Stencil.make(values)).run(maxiter, tol)
    return len(hist) - 1, hist
