"""numpy restatement of XY semi-coarsening (include/gpusolve_semi.h) and the V-cycle composed of it, the CPU oracle's
jacobi / residual and zline_ref's sweep — the reference of tests/test_semi_cpu.py and tests/test_gpu_semi.py (TEST
INFRASTRUCTURE ONLY; the product never imports it).

level_stencil() is the header's rule in the header's evaluation order; restrict_xy / prolong_xy are xfer_ref's per-axis
passes on axes 0 and 1 only. numpy rounds every product and sum once, as the library does under -ffp-contract=off, so
the two agree bit for bit. Arrays are padded and indexed [x][y][z] (the oracle's layout).

Cycle is xfer_ref.Cycle (so weights_ref.Cycle's recursion) with an XY level list, one stencil and one smoother flag per
level: a level whose flag is set runs zline_ref.sweep with its own stencil, the others the oracle's point Jacobi."""
import math

import numpy as np

import oracle as O
import xfer_ref
import zline_ref as Z


def level_dims(dims):
    """Interior extents of every level of an XY hierarchy: floor(log2(min(nx, ny))) + 1 levels, x and y halved."""
    nx, ny, nz = (int(d) for d in dims)
    nlev = int(math.floor(math.log(min(nx, ny)) / math.log(2.0))) + 1
    out = [(nx, ny, nz)]
    for _ in range(nlev - 1):
        out.append((out[-1][0] // 2, out[-1][1] // 2, nz))
    return out


def level_stencil(values, h0, hl, offsets=O.CANONICAL):
    """The seven weights of a level of mesh width hl under a level 0 of mesh width h0, in the entries' own order;
    None unless the offsets are the seven axis offsets once each."""
    sh = Z.shape_of(values, offsets)
    if sh is None:
        return None
    q = np.float64(hl) / np.float64(h0)
    r = q * q
    xy = [np.float64(w) for w, (ox, oy, oz) in zip(values, offsets) if (ox, oy) != (0, 0)]
    s = ((xy[0] + xy[1]) + xy[2]) + xy[3]
    out = []
    for w, (ox, oy, oz) in zip(values, offsets):
        w = np.float64(w)
        if (ox, oy, oz) == (0, 0, 0):
            a = r * w
            b = (r - np.float64(1.0)) * s
            out.append(float(a + b))
        elif oz != 0:
            out.append(float(r * w))
        else:
            out.append(float(w))
    return tuple(out)


def restrict_xy(r, fine_dims):
    """R_xy r of a padded fine array: X, then Y pass of xfer_ref's restriction; coarse ring 0, z untouched (the ring
    planes z = 0 and nz + 1 come out 0)."""
    a = np.asarray(r, dtype=np.float64)
    for axis in range(2):
        a = xfer_ref._restrict_axis(a, axis, fine_dims[axis])
    a = np.ascontiguousarray(a)
    a[:, :, 0] = 0.0
    a[:, :, -1] = 0.0
    return a


def prolong_xy(d, fine_dims):
    """P_xy d of a padded coarse array (its ring included, as data): X, then Y pass of xfer_ref's prolongation; only
    the fine interior is meaningful (the kernel writes nothing else), the ring is set to 0."""
    a = np.asarray(d, dtype=np.float64)
    for axis in range(2):
        a = xfer_ref._prolong_axis(a, axis, fine_dims[axis])
    a = np.ascontiguousarray(a)
    a[:, :, 0] = 0.0
    a[:, :, -1] = 0.0
    return a


def auto_flags(stencils, offsets=O.CANONICAL):
    """The AUTO rule per level: lines where the largest |z weight| is strictly greater than the largest |x / y
    weight|."""
    out = []
    for values in stencils:
        mz = max(abs(w) for w, (ox, oy, oz) in zip(values, offsets) if oz != 0)
        mxy = max(abs(w) for w, (ox, oy, oz) in zip(values, offsets) if (ox, oy) != (0, 0))
        out.append(mz > mxy)
    return out


class Cycle(xfer_ref.Cycle):
    """The LINEAR V-cycle of an XY hierarchy. smoother: "jacobi", "zline", "auto", or a list of per-level flags
    (True: z-line sweeps)."""

    def __init__(self, dims, values, offsets=O.CANONICAL, smoother="jacobi", pre=(0.8, 0.8), post=(0.8, 0.8), f0=None,
                 v0=None):
        super().__init__(dims, O.LINEAR, pre, post, f0=f0, v0=v0, stencil=O.Stencil.make(values, offsets))
        self.ld = level_dims(dims)
        self.h = [1.0 / (d[1] + 1) for d in self.ld]
        self.offsets = list(offsets)
        self.values = [level_stencil(values, self.h[0], h, offsets) for h in self.h]
        self.stencils = [O.Stencil.make(v, offsets) for v in self.values]
        self.f, self.v = self.f[:1], self.v[:1]
        for d in self.ld[1:]:
            self.f.append(O.zeros(*d))
            self.v.append(O.zeros(*d))
        if smoother == "auto":
            self.line = auto_flags(self.values, offsets)
        elif smoother in ("jacobi", "zline"):
            self.line = [smoother == "zline"] * len(self.ld)
        else:
            self.line = [bool(x) for x in smoother]
            assert len(self.line) == len(self.ld)

    def pattern(self):
        return " ".join("Z" if z else "J" for z in self.line)

    def R(self, l, a):
        return restrict_xy(a, self.ld[l])

    def P(self, l, c):
        return prolong_xy(c, self.ld[l])

    def _smooth(self, l, weights):
        for om in weights:
            if self.line[l]:
                self.v[l] = Z.sweep(self.v[l], self.f[l], self.h[l], om, self.values[l], self.offsets)
            else:
                self.v[l] = O.jacobi(self.v[l], self.f[l], self.h[l], mode=O.LINEAR, omega=float(om), sweeps=1,
                                     stencil=self.stencils[l])

    def residual(self, l=0):
        return O.residual(self.v[l], self.f[l], self.h[l], O.LINEAR, stencil=self.stencils[l])


def cycles_to(c, reduction=1e8, maxcycles=60):
    """How many cycles the model needs for ||r|| <= ||r0|| / reduction (maxcycles + 1 if it does not get there)."""
    r0 = c.residual(0)[1]
    for k in range(1, maxcycles + 1):
        if c.vcycle() <= r0 / reduction:
            return k
    return maxcycles + 1
