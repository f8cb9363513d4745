"""numpy restatement of full multigrid's prolongation by position (gs_fmg_prolong_pa, include/gpusolve_transfer.h) and
of the FMG start composed of it — the reference of tests/test_fmg_pa_cpu.py and tests/test_gpu_fmg_pa.py (TEST
INFRASTRUCTURE ONLY; the product never imports it).

Tables and operator are the header's definitions in the header's evaluation order; numpy rounds every product and sum
once, as the kernel does under -ffp-contract=off, so the two agree bit for bit. Arrays are padded and indexed
[x][y][z] (the oracle's layout).

fmg() is the driver's FMG with the POSITION prolongation: tests/xfer_ref.py's Cycle (POSITION transfers) carries the
hierarchy, f is restricted through Cycle.R, the coarsest level is iterated from zero, and every finer level's v
interior comes from tests/fmg_ref.py's prolong on an aligned transition and from prolong() below on every other one."""
import numpy as np

import fmg_ref
import oracle as O
import xfer_ref as X


def axis_tables(n):
    """The closed form of gs_fmg_axis for fine n -> coarse m = n // 2: dict of cj (int32, n + 2 entries) and cw
    ((n + 2, 4)); entries 0 and n + 1 are zero. K = 4 nodes per point, K = 3 (cw[:, 3] = 0) where m = 1."""
    n = int(n)
    m, D = n // 2, n + 1
    P = m + 2
    i = np.arange(n + 2, dtype=np.int64)
    q = i * (m + 1)
    pj, rem = q // D, q % D
    cj = np.clip(pj - 1, 0, P - 4) if P >= 4 else np.zeros_like(pj)
    t = (pj - cj).astype(np.float64) + rem.astype(np.float64) / np.float64(D)
    if P >= 4:
        w = [-(((t - 1) * (t - 2)) * (t - 3)) / 6, ((t * (t - 2)) * (t - 3)) / 2, -((t * (t - 1)) * (t - 3)) / 2,
             ((t * (t - 1)) * (t - 2)) / 6]
    else:
        w = [((t - 1) * (t - 2)) / 2, -(t * (t - 2)), (t * (t - 1)) / 2, np.zeros_like(t)]
    cw = np.stack(w, axis=1)
    cj[[0, n + 1]] = 0
    cw[[0, n + 1]] = 0.0
    return {"cj": cj.astype(np.int32), "cw": np.ascontiguousarray(cw)}


_cache = {}


def tables(n):
    if n not in _cache:
        _cache[n] = axis_tables(n)
    return _cache[n]


def prolong_axis(c, axis, n):
    """(m + 2) padded values along `axis` -> (n + 2): ((w0 c[cj] + w1 c[cj+1]) + w2 c[cj+2]) + w3 c[cj+3], truncated
    to K terms, at i = 1..n; ring 0."""
    T = tables(n)
    c = np.moveaxis(np.asarray(c, dtype=np.float64), axis, 0)
    assert c.shape[0] == n // 2 + 2, (c.shape, n)
    K = 4 if c.shape[0] >= 4 else 3
    out = np.zeros((n + 2,) + c.shape[1:])
    sh = (n,) + (1,) * (c.ndim - 1)
    j = T["cj"][1:n + 1].astype(np.int64)
    w = [T["cw"][1:n + 1, k].reshape(sh) for k in range(4)]
    s = (w[0] * c[j] + w[1] * c[j + 1]) + w[2] * c[j + 2]
    if K == 4:
        s = s + w[3] * c[j + 3]
    out[1:n + 1] = s
    return np.moveaxis(out, 0, axis)


def prolong(c, fine_dims):
    """P c of a padded coarse array: X, then Y, then Z pass; the fine ring is 0 (the kernel leaves it alone)."""
    a = np.asarray(c, dtype=np.float64)
    for axis in range(3):
        a = prolong_axis(a, axis, fine_dims[axis])
    return np.ascontiguousarray(a)


def fmg(dims, mode=O.LINEAR, cycles_per_level=1, pre=(0.8, 0.8), post=(0.8, 0.8), gamma=1.0, f0=None, stencil=None,
        cubic=True):
    """FMG(cycles_per_level) from the coarsest level with POSITION transfers: (level-0 v, the level-0 residual norm).
    cubic=False puts the V-cycle's own (trilinear) prolongation of a correction in the cubic's place, for comparison."""
    c = X.Cycle(dims, mode, pre, post, gamma, f0=f0, transfer="position", stencil=stencil)
    nl = len(c.ld)
    for l in range(nl - 1):
        c.f[l + 1] = c.R(l, c.f[l])
    for l in range(nl - 1, -1, -1):
        v = O.zeros(*c.ld[l])
        if l < nl - 1:
            src = c.v[l + 1]
            if not cubic:
                fine = c.P(l, src)
            elif X.aligned(c.ld[l], c.ld[l + 1]):
                fine = fmg_ref.prolong(src)
            else:
                fine = prolong(src, c.ld[l])
            v[1:-1, 1:-1, 1:-1] = fine[1:-1, 1:-1, 1:-1]
        c.v[l] = v
        for _ in range(cycles_per_level):
            c.vcycle_from(l)
    return c.v[0], c.residual(0)[1]
