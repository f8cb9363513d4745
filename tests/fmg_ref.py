"""numpy + CPU-oracle restatement of the full-multigrid (FMG) start — the reference of tests/test_fmg_cpu.py and
tests/test_gpu_fmg.py (TEST INFRASTRUCTURE ONLY; the product never imports it).

prolong(c): the tricubic prolongation of include/gpusolve_hip.h's gs_fmg_prolong, per axis x, then y, then z, every
expression in the header's evaluation order — numpy rounds each product and sum once, as the kernel does under
-ffp-contract=off, so the two agree bit for bit. Arrays are padded, indexed [x][y][z] (the oracle's layout); the
output keeps the ring (injected / interpolated from the coarse ring), of which the kernel writes the interior only.

fmg(dims, ...): nested iteration composed of the oracle's operators, one oracle.Grid(dims_l) per level: with
h_l = 1/(ny_l + 1), a stand-alone grid of level l's size is level l of the big one."""
import math

import numpy as np

import oracle as O


def cubic_axis(c, axis):
    """(n + 2) padded values along `axis` -> (2n + 3): padded fine index 2i takes coarse index i."""
    c = np.moveaxis(np.asarray(c, dtype=np.float64), axis, 0)
    P = c.shape[0]
    n = P - 2
    assert n >= 1
    out = np.empty((2 * n + 3,) + c.shape[1:])
    out[0::2] = c
    if n == 1:
        out[1] = ((3 * c[0] + 6 * c[1]) - c[2]) / 8
        out[3] = ((3 * c[2] + 6 * c[1]) - c[0]) / 8
    else:
        out[1] = (((5 * c[0] + 15 * c[1]) - 5 * c[2]) + c[3]) / 16
        out[2 * n + 1] = (((5 * c[P - 1] + 15 * c[P - 2]) - 5 * c[P - 3]) + c[P - 4]) / 16
        # odd index 2i+1, i = 1 .. n-1
        out[3:2 * n:2] = (((-c[0:n - 1] + 9 * c[1:n]) + 9 * c[2:n + 1]) - c[3:n + 2]) / 16
    return np.moveaxis(out, 0, axis)


def prolong(c):
    """Tricubic prolongation of a padded coarse array (nx+2, ny+2, nz+2) -> (2nx+3, 2ny+3, 2nz+3)."""
    return np.ascontiguousarray(cubic_axis(cubic_axis(cubic_axis(c, 0), 1), 2))


def level_dims(dims):
    """Interior extents of every level (src/cpu/CpuGridData.cpp:19-41: floor(log2(min)) + 1 levels, halved)."""
    nlev = int(math.floor(math.log(min(dims)) / math.log(2.0))) + 1
    out = [tuple(int(d) for d in dims)]
    for _ in range(nlev - 1):
        out.append(tuple(d // 2 for d in out[-1]))
    return out


def start_level(dims):
    """The deepest level with every transition above it aligned (fine n = 2 coarse n + 1 per axis); 0: none."""
    ld = level_dims(dims)
    s = 0
    while s + 1 < len(ld) and all(f == 2 * c + 1 for f, c in zip(ld[s], ld[s + 1])):
        s += 1
    return s


def fmg(dims, mode=O.LINEAR, cycles_per_level=1, pre=2, post=2, omega=0.8, gamma=1.0, f0=None, prolongation=prolong):
    """FMG(cycles_per_level): (level-0 oracle grid, its v, the level-0 residual norm).

    Coarse right-hand sides are the full-weighting restrictions of level 0's f (f0, default the analytic one); the
    start level is iterated from zero, every finer level from `prolongation` of the level below."""
    ld = level_dims(dims)
    s = start_level(dims)
    assert s > 0, "FMG needs aligned coarse grids (sizes 2^k - 1)"
    f = [np.ascontiguousarray(f0) if f0 is not None else O.rhs(*ld[0], mode, gamma)]
    for l in range(s):
        f.append(O.restrict(f[l], ld[l + 1]))
    v, g, res = None, None, None
    for l in range(s, -1, -1):
        g = O.Grid(ld[l], mode=mode, maxiter=1, omega=omega, gamma=gamma, pre=pre, post=post)
        g.field(0, "f")[...] = f[l]
        gv = g.field(0, "v")
        gv[...] = 0.0
        if v is not None:
            gv[1:-1, 1:-1, 1:-1] = prolongation(v)[1:-1, 1:-1, 1:-1]
        for _ in range(cycles_per_level):
            res = g.vcycle()
        v = gv.copy()
    return g, v, res


def trilinear(c):
    """The reference's interpolate (a correction's prolongation) in prolong()'s place, for comparison."""
    return O.interpolate(np.ascontiguousarray(c), tuple(2 * (n - 2) + 1 for n in c.shape))
