"""The kernel ABI's layout contract (include/gpusolve_hip.h, "Layout contract"): every launcher, at the smallest shapes
that select each kernel family, in every named layout of tests/layout_field.py — gs_field_layout's own, tight even
pitches, loose pitches with a gap between planes, odd pitches (every 16-byte pair access at an address that is 8 mod
16) and operands of one call at different 16-byte phases.

Inputs: seeded random interiors; the ring of v / e / restV exactly 0 (the header requires it); the rings of f, w, F and
of the GS_NEWTON_B factor finite non-zero noise (no reference path reads them); EVERY word outside the padded box a NaN
(pitch padding, plane gaps, the second ghost planes unless zlo / zhi names them as read, guard margins). Outputs are
NaN-poisoned whole. Per call: the return code is 0; the written set is exactly the documented one; every input is
unchanged word for word, its poison included; LINEAR values are bit-identical to the CPU oracle's operators; every
mode's values, and the norm partials, are bit-identical to the same call on ordinary DevFields with zero rings and
zero padding (which the rest of the suite pins to the oracle at each mode's tolerance): layout cannot change a
per-point expression, so equality is the bound and needs no tolerance."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import gpusolve as gsv  # noqa: E402
from gpusolve.devfield import DevField  # noqa: E402
import oracle as O  # noqa: E402
import fmg_ref  # noqa: E402
import weights_ref as W  # noqa: E402
from layout_field import LAYOUT_IDS, POISON_IN, POISON_OUT, LayoutField, layouts  # noqa: E402

EINVAL = gsv._abi.GS_EINVAL
OMEGA, GAMMA = 0.8, 1.0
W2, W3 = (0.9, 1.3), (0.7, 1.1, 1.4)
RB_LAYOUTS = ("default", "tight_even", "tight_odd", "mixed")  # the large cases
REORDERED = ((-1, -1, 6, -1, -1, -1, -1), [(0, 0, 1), (-1, 0, 0), (0, 0, 0), (0, 0, -1), (1, 0, 0), (0, 1, 0), (0, -1, 0)])
GENERAL = ((4, -1, -1, -0.5, -0.5, -0.5, -0.5), list(gsv.CANONICAL_OFFSETS))

by_layout = pytest.mark.parametrize("lid", LAYOUT_IDS)
K = None


def k():
    global K
    if K is None:
        assert torch.cuda.is_available(), "GPU tests need a GPU (no CPU fallback exists)"
        K = gsv.kernels()
    return K


def st():
    return torch.cuda.current_stream().cuda_stream


def ok(rc):
    assert rc == 0, k().gs_strerror(rc).decode()


def S_abi(values=(6, -1, -1, -1, -1, -1, -1), offsets=gsv.CANONICAL_OFFSETS):
    return gsv.Stencil(list(values), list(offsets)).to_abi()


UNIT = S_abi()


def arr(*w):
    return (C.c_double * len(w))(*w)


def sid(shape):
    return "x".join(str(n) for n in shape)


def half(shape):
    return tuple(n // 2 for n in shape)


def inner(a):
    return a[1:-1, 1:-1, 1:-1]


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def same(a, b, what):
    assert a.shape == b.shape, what
    ne = bits(a) != bits(b)
    assert not ne.any(), f"{what}: {int(ne.sum())} words differ, first at {tuple(np.argwhere(ne)[0])}"


def rand_full(rng, dims, scale=1.0):
    """Random interior, zero ring."""
    a = np.zeros(tuple(n + 2 for n in dims))
    inner(a)[...] = rng.uniform(-scale, scale, dims)
    return a


def noisy(a, zdata=(False, False)):
    """`a` with its ring replaced by finite non-zero noise; zdata: that z-face (plane 0 / nz+1) holds data, kept."""
    rng = np.random.default_rng(a.size)
    n = np.where(rng.random(a.shape) < 0.5, -1.0, 1.0) * rng.uniform(0.5, 50.0, a.shape)
    out = n.copy()
    z0, z1 = (0 if zdata[0] else 1), a.shape[2] - (0 if zdata[1] else 1)
    out[1:-1, 1:-1, z0:z1] = a[1:-1, 1:-1, z0:z1]
    return out


def level_of(fld, h, nz=None, z0=0):
    return gsv.gs_level(fld.nx, fld.ny, fld.nz if nz is None else nz, fld.ldy, fld.ldz, z0, h)


@functools.lru_cache(maxsize=8)
def fields(shape, seed=0):
    """v (+-1), f (+-100), w (+-0.8, the Newton modes' range) with zero rings; B = gamma (1 + w) e^w; gamma."""
    rng = np.random.default_rng(shape[0] + 1000 * shape[1] + 1000003 * shape[2] + seed)
    v, f, w = rand_full(rng, shape), rand_full(rng, shape, 100.0), rand_full(rng, shape, 0.8)
    b = GAMMA * (1.0 + w) * np.exp(w)
    g = np.full_like(w, GAMMA)
    for a in (v, f, w, b, g):
        a.setflags(write=False)
    return v, f, w, b, g


def w_of(shape, mode, seed=0):
    """The `w` operand of a mode: None, newtonV, the factor B, or the field of gamma."""
    _, _, w, b, g = fields(shape, seed)
    return {0: None, 1: None, 2: w, 3: b, 4: g}[mode]


# ---- one side of a comparison -----------------------------------------------------------------------------------
class Parts:
    """Norm partials (or any small device array) of n entries with poisoned guards on both sides."""

    def __init__(self, n, odd):
        self.n = n
        self.t = torch.zeros(n + 20, dtype=torch.float64, device="cuda")
        self.t.view(torch.int64).fill_(POISON_OUT)
        self.o = 8 + ((self.t.data_ptr() // 8 + (1 if odd else 0)) % 2)  # 16-byte aligned, or 8 mod 16
        self.ptr = self.t.data_ptr() + 8 * self.o
        assert self.ptr % 16 == (8 if odd else 0)

    def guards(self, what):
        torch.cuda.synchronize()
        w = self.t.view(torch.int64).cpu().numpy()
        assert (w[:self.o] == POISON_OUT).all() and (w[self.o + self.n:] == POISON_OUT).all(), \
            f"{what}: an entry outside its {self.n} was written (the one past the end included)"
        return w

    def result(self, what):
        w = self.guards(what)
        assert (w[self.o:self.o + self.n] != POISON_OUT).all(), f"{what}: a partial was not written"
        return self.t.cpu().numpy()[self.o:self.o + self.n].copy()


class Side:
    """The fields of one run: in the named layout (poisoned LayoutFields, every contract check made in finish()), or
    — lid None — the comparison run on DevFields with zero rings and zero padding."""

    def __init__(self, lid):
        self.lid = lid
        self.checks, self.results, self.held = [], {}, []

    def _new(self, dims, role):
        if self.lid is None:
            fld = DevField(*dims)
        else:
            lay = layouts(*dims)[self.lid]
            fld = LayoutField(*dims, lay.ldy, lay.ldz, lay.phase_in if role == "in" else lay.phase_out)
        self.held.append(fld)
        return fld

    @property
    def odd(self):
        return self.lid in ("tight_odd", "mixed")

    def _fill(self, fld, box, ring, zdata, below, above):
        data = np.asarray(box)
        if self.lid is None:
            if ring == "noise":  # no reference path reads these rings: zero here, noise in the layout run
                z = np.zeros_like(data)
                z0, z1 = (0 if zdata[0] else 1), data.shape[2] - (0 if zdata[1] else 1)
                z[1:-1, 1:-1, z0:z1] = data[1:-1, 1:-1, z0:z1]
                data = z
            ext = np.zeros(data.shape[:2] + (data.shape[2] + 2,))
            ext[:, :, 1:-1] = data
            if below is not None:
                ext[:, :, 0] = below
            if above is not None:
                ext[:, :, -1] = above
            fld.zero().from_xyz_ext(ext)
            return
        if ring == "noise":
            data = noisy(data, zdata)
        fld.poison_all(POISON_IN).from_xyz(data)
        e = fld._ext(fld.buf)
        if below is not None:
            e[0] = torch.from_numpy(np.ascontiguousarray(np.asarray(below).T)).to(fld.buf.device)
        if above is not None:
            e[-1] = torch.from_numpy(np.ascontiguousarray(np.asarray(above).T)).to(fld.buf.device)

    def inp(self, box, ring="zero", role="in", zdata=(False, False), below=None, above=None, name=None):
        """An input: `box` in the padded box, ghost planes -1 / nz+2 from `below` / `above` where the call reads them,
        poison everywhere else. Must come back unchanged, word for word."""
        fld = self._new(tuple(n - 2 for n in np.asarray(box).shape), role)
        self._fill(fld, box, ring, zdata, below, above)
        if self.lid is not None:
            fld.snapshot()
            self.checks.append(lambda: fld.assert_unchanged(what=f"input {name or len(self.checks)}"))
        return fld

    def out(self, dims, name, written="interior", zero_ring=False):
        """An output, poisoned whole (zero_ring: the box's ring then set to 0, as gs_newton_F_update's w_out needs).
        written: 'interior', 'box', 'planes' (-1 .. nz+2 at full pitch) or ('z', z1, z2): the interior's planes z1..z2."""
        fld = self._new(dims, "out")
        if self.lid is None:
            self.results[name] = lambda: self._region(fld, written)
            return fld
        fld.poison_all()
        if zero_ring:
            ring = fld.box_mask() & ~fld.interior_mask()
            fld.buf[ring] = 0.0
        fld.snapshot()
        mask = self._mask(fld, written)

        def check():
            fld.assert_unchanged(~mask, what=f"output {name}")
            assert bool((fld.i64[mask] != POISON_OUT).all()), f"output {name}: a word of the documented set was not written"
            if not zero_ring:
                fld.assert_written_exactly(mask, what=f"output {name}")
        self.checks.append(check)
        self.results[name] = lambda: self._region(fld, written)
        return fld

    def inout(self, box, name, ring="zero", role="out", written="interior"):
        """A field updated in place: everything outside the written set must come back unchanged."""
        fld = self._new(tuple(n - 2 for n in np.asarray(box).shape), role)
        self._fill(fld, box, ring, (False, False), None, None)
        if self.lid is not None:
            fld.snapshot()
            mask = self._mask(fld, written)
            self.checks.append(lambda: fld.assert_unchanged(~mask, what=f"in-place field {name}"))
        self.results[name] = lambda: self._region(fld, written)
        return fld

    def parts(self, n, name):
        p = Parts(n, self.odd)
        self.results[name] = lambda: p.result(name)
        return p

    def ws(self, n):
        """A poisoned workspace of n elements; only its guards are checked (what it holds is the launcher's own)."""
        p = Parts(n, self.odd)
        self.held.append(p)
        self.checks.append(lambda: p.guards("workspace"))
        return p

    @staticmethod
    def _mask(fld, written):
        if written == "interior":
            return fld.interior_mask()
        if written == "box":
            return fld.box_mask()
        if written == "planes":
            return fld.planes_mask()
        _, z1, z2 = written
        m = fld._mask()
        fld._box(m)[z1:z2 + 1, 1:-1, 1:-1] = True
        return m

    @staticmethod
    def _region(fld, written):
        """The words of the written set that both sides have in common, as an array."""
        if written == "planes":  # (the pitch padding differs between the layouts: the box-shaped part)
            if isinstance(fld, LayoutField):
                return fld.to_xyz_ext()
            torch.cuda.synchronize()
            return np.ascontiguousarray(fld.zyx_ext[:, :, :fld.nx + 2].cpu().numpy().transpose(2, 1, 0))
        a = fld.to_xyz()
        if written == "box":
            return a
        if written == "interior":
            return inner(a).copy()
        _, z1, z2 = written
        return a[1:-1, 1:-1, z1:z2 + 1].copy()

    def finish(self):
        torch.cuda.synchronize()
        for c in self.checks:
            c()
        return {n: get() for n, get in self.results.items()}


def both(lid, body, what):
    """Runs `body` on the layout side and on the DevField side; every result of the two must agree bit for bit.
    Returns the layout side's results."""
    a = Side(lid)
    body(a)
    ra = a.finish()
    b = Side(None)
    body(b)
    rb = b.finish()
    assert ra.keys() == rb.keys()
    for n in ra:
        same(ra[n], rb[n], f"{what} [{lid}] {n} against the DevField run")
    return ra


# ---- k_generic ---------------------------------------------------------------------------------------------------
GENERIC_SHAPES = [(37, 11, 9), (130, 7, 5)]


def is_generic(S, shape):
    L = gsv.gs_level(*shape, *gsv.field_layout(*shape)[:2], 0, 1.0 / (shape[1] + 1))
    return k().gs_newton_F_update_supported(C.byref(S), C.byref(L)) == 0


def pass_launchers(R, S, shape, mode, stencil_w=True):
    """gs_jacobi_sweep, _norm (real and zero iterate) and gs_residual on one set of inputs."""
    h = 1.0 / (shape[1] + 1)
    v0, f0 = fields(shape)[:2]
    w0 = w_of(shape, mode) if stencil_w else None
    v, f = R.inp(v0, name="v"), R.inp(f0, "noise", "f", name="f")
    w = R.inp(w0, "noise", name="w") if w0 is not None else None
    wp = w.ptr if w else None
    L = v.level(h)
    n = k().gs_residual_num_partials(C.byref(S), C.byref(L))
    out = R.out(shape, "sweep")
    ok(k().gs_jacobi_sweep(C.byref(S), C.byref(L), mode, OMEGA, GAMMA, v.ptr, out.ptr, f.ptr, wp, st()))
    out, p = R.out(shape, "sweep_norm"), R.parts(n, "sweep_norm partials")
    ok(k().gs_jacobi_sweep_norm(C.byref(S), C.byref(L), mode, OMEGA, GAMMA, v.ptr, out.ptr, f.ptr, wp, p.ptr, st()))
    r, p = R.out(shape, "residual"), R.parts(n, "residual partials")
    ok(k().gs_residual(C.byref(S), C.byref(L), mode, GAMMA, v.ptr, f.ptr, wp, r.ptr, p.ptr, st()))
    if mode != 1:  # the zero iterate (not in FAS mode)
        out, p = R.out(shape, "sweep zero"), R.parts(n, "sweep zero partials")
        ok(k().gs_jacobi_sweep_norm(C.byref(S), C.byref(L), mode, OMEGA, GAMMA, None, out.ptr, f.ptr, wp, p.ptr, st()))


def check_pass_linear(res, shape, stencil=None):
    h = 1.0 / (shape[1] + 1)
    v0, f0 = fields(shape)[:2]
    ref = inner(O.jacobi(v0, f0, h, 0, OMEGA, GAMMA, 1, stencil=stencil))
    same(res["sweep"], ref, "sweep against the oracle")
    same(res["sweep_norm"], ref, "sweep_norm against the oracle")
    same(res["residual"], inner(O.residual(v0, f0, h, 0, GAMMA, stencil=stencil)[0]), "residual against the oracle")
    same(res["sweep zero"], inner(O.jacobi(np.zeros_like(v0), f0, h, 0, OMEGA, GAMMA, 1, stencil=stencil)),
         "zero-iterate sweep against the oracle")


@by_layout
@pytest.mark.parametrize("shape", GENERIC_SHAPES, ids=sid)
def test_generic_pass(shape, lid):
    """k_generic: gs_jacobi_sweep, gs_jacobi_sweep_norm, gs_residual in modes 0-3, real and zero iterates."""
    assert is_generic(UNIT, shape)
    for mode in (0, 1, 2, 3):
        res = both(lid, lambda R: pass_launchers(R, UNIT, shape, mode), f"generic {shape} m{mode}")
        if mode == 0:
            check_pass_linear(res, shape)


@by_layout
@pytest.mark.parametrize("stencil", [REORDERED, GENERAL], ids=["reordered", "general"])
def test_generic_pass_stencils(stencil, lid):
    shape = GENERIC_SHAPES[0]
    S, So = S_abi(*stencil), O.Stencil.make(*stencil)
    assert is_generic(S, shape)
    for mode in (0, 1):
        res = both(lid, lambda R: pass_launchers(R, S, shape, mode, False), f"generic stencil {shape} m{mode}")
        if mode == 0:
            check_pass_linear(res, shape, So)


def operator_launchers(R, S, shape):
    """gs_apply_op, gs_apply_op_add (in place) and gs_newton_F."""
    h = 1.0 / (shape[1] + 1)
    v0, f0, w0 = fields(shape)[:3]
    u, w, F = R.inp(v0, name="u"), R.inp(w0, name="w"), R.inp(f0, "noise", "f", name="F")
    L = u.level(h)
    out = R.out(shape, "apply_op")
    ok(k().gs_apply_op(C.byref(S), C.byref(L), GAMMA, u.ptr, out.ptr, st()))
    f = R.inout(f0, "apply_op_add", "noise")
    ok(k().gs_apply_op_add(C.byref(S), C.byref(L), GAMMA, u.ptr, f.ptr, st()))
    n = k().gs_residual_num_partials(C.byref(S), C.byref(L))
    res, p = R.out(shape, "newton_F"), R.parts(n, "newton_F partials")
    ok(k().gs_newton_F(C.byref(S), C.byref(L), GAMMA, w.ptr, F.ptr, res.ptr, p.ptr, st()))


@by_layout
@pytest.mark.parametrize("shape", GENERIC_SHAPES, ids=sid)
def test_generic_operators(shape, lid):
    assert is_generic(UNIT, shape)
    both(lid, lambda R: operator_launchers(R, UNIT, shape), f"generic operators {shape}")


# ---- k_rb and k_newton_upd ----------------------------------------------------------------------------------------
RB_SHAPES = [(127, 9, 2047), (129, 7, 2050)]
by_rb_layout = pytest.mark.parametrize("lid", RB_LAYOUTS)
by_rb_shape = pytest.mark.parametrize("shape", RB_SHAPES, ids=sid)


def is_rb(S, shape):
    L = gsv.gs_level(*shape, *gsv.field_layout(*shape)[:2], 0, 1.0 / (shape[1] + 1))
    return k().gs_newton_F_update_supported(C.byref(S), C.byref(L)) == 1


@by_rb_layout
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@by_rb_shape
def test_rb_sweep(shape, mode, lid):
    """gs_jacobi_sweep through k_rb. [127x9x2047-0-tight_odd] is the narrowest call of the misaligned class: every
    pair load and store of the register-blocked march at an address that is 8 mod 16."""
    assert is_rb(UNIT, shape)
    h = 1.0 / (shape[1] + 1)
    v0, f0 = fields(shape)[:2]
    w0 = w_of(shape, mode)

    def body(R):
        v, f = R.inp(v0, name="v"), R.inp(f0, "noise", "f", name="f")
        w = R.inp(w0, "noise", name="w") if w0 is not None else None
        out = R.out(shape, "sweep")
        ok(k().gs_jacobi_sweep(C.byref(UNIT), C.byref(v.level(h)), mode, OMEGA, GAMMA, v.ptr, out.ptr, f.ptr,
                               w.ptr if w else None, st()))

    res = both(lid, body, f"k_rb sweep {shape} m{mode}")
    if mode == 0:
        same(res["sweep"], inner(O.jacobi(v0, f0, h, 0, OMEGA, GAMMA, 1)), "k_rb sweep against the oracle")


@by_rb_layout
@by_rb_shape
def test_rb_pass(shape, lid):
    """The other launchers of launch_pass through k_rb: LINEAR and GS_NEWTON_B norms, residuals and zero iterates, a
    general stencil (the UN = false instances), the FAS operator and compF."""
    assert is_rb(UNIT, shape) and is_rb(S_abi(*GENERAL), shape)
    for mode in (0, 3):
        res = both(lid, lambda R: pass_launchers(R, UNIT, shape, mode), f"k_rb {shape} m{mode}")
        if mode == 0:
            check_pass_linear(res, shape)
    res = both(lid, lambda R: pass_launchers(R, S_abi(*GENERAL), shape, 0, False), f"k_rb general {shape}")
    check_pass_linear(res, shape, O.Stencil.make(*GENERAL))
    both(lid, lambda R: operator_launchers(R, UNIT, shape), f"k_rb operators {shape}")


@by_rb_layout
@by_rb_shape
def test_newton_update(shape, lid):
    """k_newton_upd: gs_newton_F_update, _restrict and _restrict_bfac (w_out's ring holds the zeros the header asks
    for and must keep them; everything else of every output starts as poison)."""
    cd = half(shape)
    h = 1.0 / (shape[1] + 1)
    v0, f0, w0 = fields(shape)[:3]
    e0 = 0.25 * v0
    assert is_rb(UNIT, shape)

    def body(R):
        w, e, F = R.inp(w0, name="w"), R.inp(e0, name="e"), R.inp(f0, "noise", "f", name="F")
        L = w.level(h)
        n = k().gs_residual_num_partials(C.byref(UNIT), C.byref(L))
        wo, f, p = R.out(shape, "w_out", zero_ring=True), R.out(shape, "f"), R.parts(n, "partials")
        ok(k().gs_newton_F_update(C.byref(UNIT), C.byref(L), GAMMA, w.ptr, e.ptr, F.ptr, wo.ptr, f.ptr, p.ptr, st()))
        wo, f, p = R.out(shape, "w_out r", zero_ring=True), R.out(shape, "f r"), R.parts(n, "partials r")
        cw = R.out(cd, "coarse_w r")
        Lc = cw.level(2 * h)
        assert k().gs_newton_F_update_restrict_supported(C.byref(UNIT), C.byref(L), C.byref(Lc)) == 1
        ok(k().gs_newton_F_update_restrict(C.byref(UNIT), C.byref(L), GAMMA, w.ptr, e.ptr, F.ptr, wo.ptr, f.ptr, p.ptr,
                                           cw.ptr, C.byref(Lc), st()))
        wo, f, p = R.out(shape, "w_out b", zero_ring=True), R.out(shape, "f b"), R.parts(n, "partials b")
        cw, b = R.out(cd, "coarse_w b"), R.out(shape, "b_out")
        ok(k().gs_newton_F_update_restrict_bfac(C.byref(UNIT), C.byref(L), GAMMA, w.ptr, e.ptr, F.ptr, wo.ptr, f.ptr,
                                                p.ptr, cw.ptr, C.byref(Lc), b.ptr, st()))

    res = both(lid, body, f"newton update {shape}")
    # w_out = w + e is exact arithmetic of the oracle's fields; coarse_w = R(w_out) the oracle's restriction
    wsum = w0 + e0
    for tag in ("", " r", " b"):
        same(res["w_out" + tag], inner(wsum), "w_out against w + e")
    for tag in (" r", " b"):
        same(res["coarse_w" + tag], inner(O.restrict(wsum, cd)), "coarse_w against the oracle's restriction")


# ---- the fused pairs (k_tb2y whole rows, FX, column blocks) -------------------------------------------------------
# shape -> (what gs_jacobi_sweep2_kernel must name, FX, modes)
PAIR_CASES = {
    (130, 7, 9): ("k_tb2y:", False, (0, 1, 2, 3, 4)),
    (257, 9, 6): ("k_tb2y:", False, (0, 1, 2, 3, 4)),
    (128, 8, 8): ("k_tb2y:", True, (0, 1, 2, 3, 4)),
    (256, 8, 10): ("k_tb2y:", True, (0, 1, 2, 3, 4)),
    (700, 6, 5): ("XH", False, (0, 1, 3)),
    (1024, 4, 3): ("XH", True, (0, 1, 3)),
}


def slab_of(a, lo, nz, zlo, zhi):
    """Local planes 0 .. nz+1 of a global field as a box, and its ghost planes -1 / nz+2 where that side is internal."""
    box = a[:, :, lo - 1: lo + nz + 1]
    return box, (a[:, :, lo - 2] if zlo else None), (a[:, :, lo + nz + 1] if zhi else None)


def pair_launch(R, S, shape, mode, weights, zlo, zhi, zero, norm, seed=0):
    """One fused pair on the slab (local planes 1..nz) of a global level that has two more planes on each internal
    side. weights None: gs_jacobi_sweep2(_norm) with OMEGA; else gs_jacobi_sweep2(_norm)_w."""
    nx, ny, nz = shape
    glob = (nx, ny, nz + 2 * zlo + 2 * zhi)
    lo = 1 + 2 * zlo
    h = 1.0 / (ny + 1)
    v0, f0 = fields(glob, seed)[:2]
    w0 = w_of(glob, mode, seed)
    zd = (bool(zlo), bool(zhi))
    vb, vl, vh = slab_of(v0, lo, nz, zlo, zhi)
    v = None if zero else R.inp(vb, below=vl, above=vh, name="v")
    f = R.inp(slab_of(f0, lo, nz, 0, 0)[0], "noise", "f", zdata=zd, name="f")
    w = R.inp(slab_of(w0, lo, nz, 0, 0)[0], "noise", zdata=zd, name="w") if w0 is not None else None
    out = R.out(shape, "pair")
    L = level_of(out, h, z0=lo - 1)
    assert k().gs_jacobi_sweep2_supported_mode(C.byref(S), C.byref(L), mode) >= 1
    vp, wp = (v.ptr if v else None), (w.ptr if w else None)
    if norm:
        p = R.parts(k().gs_jacobi_sweep2_num_partials(C.byref(S), C.byref(L), mode), "pair partials")
        if weights is None:
            ok(k().gs_jacobi_sweep2_norm(C.byref(S), C.byref(L), mode, OMEGA, GAMMA, vp, out.ptr, f.ptr, wp, zlo, zhi,
                                         p.ptr, st()))
        else:
            ok(k().gs_jacobi_sweep2_norm_w(C.byref(S), C.byref(L), mode, arr(*weights), GAMMA, vp, out.ptr, f.ptr, wp,
                                           zlo, zhi, p.ptr, st()))
    elif weights is None:
        ok(k().gs_jacobi_sweep2(C.byref(S), C.byref(L), mode, OMEGA, GAMMA, vp, out.ptr, f.ptr, wp, zlo, zhi, st()))
    else:
        ok(k().gs_jacobi_sweep2_w(C.byref(S), C.byref(L), mode, arr(*weights), GAMMA, vp, out.ptr, f.ptr, wp, zlo, zhi,
                                  st()))


def pair_oracle(shape, weights, zlo, zhi, zero, stencil=None, seed=0):
    nx, ny, nz = shape
    glob = (nx, ny, nz + 2 * zlo + 2 * zhi)
    lo = 1 + 2 * zlo
    v0, f0 = fields(glob, seed)[:2]
    if zero:
        v0 = np.zeros_like(v0)
    ref = W.sweeps(v0, f0, 1.0 / (ny + 1), 0, weights or (OMEGA, OMEGA), GAMMA, stencil)
    return ref[1:-1, 1:-1, lo: lo + nz]


@by_layout
@pytest.mark.parametrize("shape", PAIR_CASES, ids=sid)
def test_pairs(shape, lid):
    """gs_jacobi_sweep2, _norm, _w, _norm_w: every mode of the family, the zero iterate, zlo / zhi each alone and
    both (their ghost planes real data, the other side's poison)."""
    name, fx, modes = PAIR_CASES[shape]
    L = gsv.gs_level(*shape, *gsv.field_layout(*shape)[:2], 0, 1.0 / (shape[1] + 1))
    for mode in modes:
        assert name in k().gs_jacobi_sweep2_kernel(C.byref(UNIT), C.byref(L), mode).decode(), (shape, mode)
    assert fx == (shape[0] % (512 if name == "XH" else 128) == 0)
    for mode in modes:
        runs = [(None, 0, 0, False, True), (W2, 0, 0, False, False), (None, 1, 0, False, False),
                (W2, 0, 1, False, True), (None, 1, 1, False, False)]
        if mode != 1:
            runs += [(None, 0, 0, True, False), (W2, 0, 0, True, True)]
        for weights, zlo, zhi, zero, norm in runs:
            what = f"pair {shape} m{mode} w={weights} zlo={zlo} zhi={zhi} zero={zero} norm={norm}"
            res = both(lid, lambda R: pair_launch(R, UNIT, shape, mode, weights, zlo, zhi, zero, norm), what)
            if mode == 0:
                same(res["pair"], pair_oracle(shape, weights, zlo, zhi, zero), what + " against the oracle")


@by_layout
def test_pairs_general_stencil(lid):
    shape, S, So = (130, 7, 9), S_abi(*GENERAL), O.Stencil.make(*GENERAL)
    for zlo, zhi in ((0, 0), (1, 1)):
        res = both(lid, lambda R: pair_launch(R, S, shape, 0, W2, zlo, zhi, False, True), f"general pair {zlo}{zhi}")
        same(res["pair"], pair_oracle(shape, W2, zlo, zhi, False, So), "general pair against the oracle")


# ---- the fused triple (k_tb3y) ------------------------------------------------------------------------------------
@by_layout
@pytest.mark.parametrize("shape,stencil", [((130, 7, 9), None), ((256, 8, 8), None), ((130, 7, 9), GENERAL)],
                         ids=["130x7x9", "256x8x8-scalar-bases", "130x7x9-general"])
def test_triples(shape, stencil, lid):
    """gs_jacobi_sweep3 and gs_jacobi_sweep3_w (three distinct weights): the general instance, the whole-wave rows
    instance that addresses through scalar row bases, and the general-stencil instance."""
    S = S_abi(*stencil) if stencil else UNIT
    So = O.Stencil.make(*stencil) if stencil else None
    h = 1.0 / (shape[1] + 1)
    v0, f0 = fields(shape)[:2]
    L = gsv.gs_level(*shape, *gsv.field_layout(*shape)[:2], 0, h)
    assert k().gs_jacobi_sweep3_supported(C.byref(S), C.byref(L)) >= 1

    def body(R):
        v, f = R.inp(v0, name="v"), R.inp(f0, "noise", "f", name="f")
        out = R.out(shape, "triple")
        ok(k().gs_jacobi_sweep3(C.byref(S), C.byref(v.level(h)), OMEGA, GAMMA, v.ptr, out.ptr, f.ptr, st()))
        out = R.out(shape, "triple_w")
        ok(k().gs_jacobi_sweep3_w(C.byref(S), C.byref(v.level(h)), arr(*W3), GAMMA, v.ptr, out.ptr, f.ptr, st()))

    res = both(lid, body, f"triple {shape}")
    same(res["triple"], inner(O.jacobi(v0, f0, h, 0, OMEGA, GAMMA, 3, stencil=So)), "triple against the oracle")
    same(res["triple_w"], inner(W.sweeps(v0, f0, h, 0, W3, GAMMA, So)), "weighted triple against the oracle")


# ---- the prolongation pairs ---------------------------------------------------------------------------------------
# shape -> modes (255: the NEWTON two-x-wave instance; 384: FX; 700: column blocks with a workspace)
PRO_CASES = {(130, 9, 10): (0, 2, 3), (255, 7, 8): (0, 2, 3), (384, 6, 6): (0, 3), (700, 6, 6): (0, 2)}


def prolong_launch(R, shape, mode, weights, rng_planes):
    """gs_jacobi_sweep2_prolong(_ws)(_w) on the whole level, or — rng_planes = (z1, z2), z1 odd — on that plane range
    of it (z0 = z1 - 1 even, both sides internal), the coarse level passed whole."""
    nx, ny, nz = shape
    cd = half(shape)
    h = 1.0 / (ny + 1)
    v0, f0 = fields(shape)[:2]
    w0 = w_of(shape, mode)
    c0 = fields(cd, 5)[0] * 0.1
    v, f, c = R.inp(v0, name="v"), R.inp(f0, "noise", "f", name="f"), R.inp(c0, name="coarse_v")
    w = R.inp(w0, "noise", name="w") if w0 is not None else None
    z1, z2 = rng_planes or (1, nz)
    out = R.out(shape, "pair", written=("z", z1, z2))
    L = level_of(v, h, nz=z2 - z1 + 1, z0=z1 - 1)
    Lc = c.level(2 * h)
    zlo, zhi = int(z1 > 1), int(z2 < nz)
    off = 8 * (z1 - 1) * L.ldz
    assert k().gs_jacobi_sweep2_prolong_supported(C.byref(UNIT), C.byref(L), mode) == 1
    n = k().gs_jacobi_sweep2_prolong_ws_elems(C.byref(UNIT), C.byref(L), mode)
    assert (n > 0) == (nx > 512)
    ws = R.ws(n) if n else None
    args = (v.ptr + off, c.ptr, None, C.byref(Lc), out.ptr + off, f.ptr + off, w.ptr + off if w else None, zlo, zhi)
    if ws is None and weights is None:
        ok(k().gs_jacobi_sweep2_prolong(C.byref(UNIT), C.byref(L), mode, OMEGA, GAMMA, *args, st()))
    elif ws is None:
        ok(k().gs_jacobi_sweep2_prolong_w(C.byref(UNIT), C.byref(L), mode, arr(*weights), GAMMA, *args, st()))
    elif weights is None:
        ok(k().gs_jacobi_sweep2_prolong_ws(C.byref(UNIT), C.byref(L), mode, OMEGA, GAMMA, *args, ws.ptr, n, st()))
    else:
        ok(k().gs_jacobi_sweep2_prolong_ws_w(C.byref(UNIT), C.byref(L), mode, arr(*weights), GAMMA, *args, ws.ptr, n,
                                             st()))


@by_layout
@pytest.mark.parametrize("shape", PRO_CASES, ids=sid)
def test_prolong_pairs(shape, lid):
    nz = shape[2]
    cd = half(shape)
    h = 1.0 / (shape[1] + 1)
    v0, f0 = fields(shape)[:2]
    c0 = fields(cd, 5)[0] * 0.1
    corrected = v0 + O.interpolate(np.ascontiguousarray(c0), shape)
    for mode in PRO_CASES[shape]:
        for weights, planes in ((None, None), (W2, None), (W2, (3, nz - 2)), (None, (3, nz - 2))):
            what = f"prolongation pair {shape} m{mode} w={weights} planes={planes}"
            res = both(lid, lambda R: prolong_launch(R, shape, mode, weights, planes), what)
            if mode == 0:
                ref = W.sweeps(corrected, f0, h, 0, weights or (OMEGA, OMEGA), GAMMA)
                z1, z2 = planes or (1, nz)
                same(res["pair"], ref[1:-1, 1:-1, z1:z2 + 1], what + " against the oracle")


# ---- the tiled small levels ---------------------------------------------------------------------------------------
@by_layout
@pytest.mark.parametrize("shape", [(9, 9, 9), (17, 9, 12)], ids=sid)
def test_tiled(shape, lid):
    """gs_smooth2_restrict_tiled(_w) (real and zero iterate) and gs_prolong_smooth2_tiled(_w), modes 0 and 2."""
    cd = half(shape)
    h = 1.0 / (shape[1] + 1)
    v0, f0 = fields(shape)[:2]
    c0 = fields(cd, 5)[0] * 0.1
    for mode in (0, 2):
        w0 = w_of(shape, mode)

        def body(R):
            v, f, c = R.inp(v0, name="v"), R.inp(f0, "noise", "f", name="f"), R.inp(c0, name="coarse_v")
            w = R.inp(w0, "noise", name="w") if w0 is not None else None
            wp = w.ptr if w else None
            L, Lc = v.level(h), c.level(1.0 / (cd[1] + 1))
            assert k().gs_tiled_supported(C.byref(UNIT), C.byref(L), mode) == 1
            for tag, vin in (("", v.ptr), (" zero", None)):
                out, cf = R.out(shape, "pre" + tag), R.out(cd, "coarse_f" + tag)
                ok(k().gs_smooth2_restrict_tiled(C.byref(UNIT), C.byref(L), mode, OMEGA, GAMMA, vin, out.ptr, f.ptr, wp,
                                                 cf.ptr, C.byref(Lc), st()))
                out, cf = R.out(shape, "pre_w" + tag), R.out(cd, "coarse_f_w" + tag)
                ok(k().gs_smooth2_restrict_tiled_w(C.byref(UNIT), C.byref(L), mode, arr(*W2), GAMMA, vin, out.ptr,
                                                   f.ptr, wp, cf.ptr, C.byref(Lc), st()))
            out = R.out(shape, "post")
            ok(k().gs_prolong_smooth2_tiled(C.byref(UNIT), C.byref(L), mode, OMEGA, GAMMA, v.ptr, c.ptr, C.byref(Lc),
                                            out.ptr, f.ptr, wp, st()))
            out = R.out(shape, "post_w")
            ok(k().gs_prolong_smooth2_tiled_w(C.byref(UNIT), C.byref(L), mode, arr(*W2), GAMMA, v.ptr, c.ptr,
                                              C.byref(Lc), out.ptr, f.ptr, wp, st()))

        res = both(lid, body, f"tiled {shape} m{mode}")
        if mode == 0:
            for tag, vv in (("", v0), (" zero", np.zeros_like(v0))):
                for wt, weights in (("", (OMEGA, OMEGA)), ("_w", W2)):
                    s = W.sweeps(vv, f0, h, 0, weights, GAMMA)
                    same(res["pre" + wt + tag], inner(s), f"tiled pre{wt}{tag} against the oracle")
                    same(res["coarse_f" + wt + tag], inner(O.restrict(O.residual(s, f0, h, 0, GAMMA)[0], cd)),
                         f"tiled coarse_f{wt}{tag} against the oracle")
            corrected = v0 + O.interpolate(np.ascontiguousarray(c0), shape)
            same(res["post"], inner(W.sweeps(corrected, f0, h, 0, (OMEGA, OMEGA), GAMMA)), "tiled post")
            same(res["post_w"], inner(W.sweeps(corrected, f0, h, 0, W2, GAMMA)), "tiled post_w")


# ---- residual + restriction ---------------------------------------------------------------------------------------
@by_layout
@pytest.mark.parametrize("shape,stencil", [((129, 33, 20), None), ((255, 10, 33), None), ((1100, 3, 4), None),
                                           ((129, 33, 20), REORDERED)],
                         ids=["129x33x20", "255x10x33", "1100x3x4-lds", "129x33x20-reordered-lds"])
def test_residual_restrict(shape, stencil, lid):
    """gs_residual_restrict in modes 0-4: k_rr2 (the register kernel) and k_resrestrict (rows too long for it, or a
    stencil out of canonical order); one output and two."""
    S = S_abi(*stencil) if stencil else UNIT
    cd = half(shape)
    h = 1.0 / (shape[1] + 1)
    v0, f0 = fields(shape)[:2]
    L = gsv.gs_level(*shape, *gsv.field_layout(*shape)[:2], 0, h)
    rr2 = k().gs_residual_restrict_slab_supported(C.byref(S), C.byref(L)) == 1
    assert rr2 == (stencil is None and shape[0] <= 1024 and shape != (1100, 3, 4))
    for mode in ((0, 1, 2, 3, 4) if stencil is None else (0, 1)):
        w0 = w_of(shape, mode)

        def body(R):
            v, f = R.inp(v0, name="v"), R.inp(f0, "noise", "f", name="f")
            w = R.inp(w0, "noise", name="w") if w0 is not None else None
            wp = w.ptr if w else None
            ca = R.out(cd, "coarse_a alone")
            Lf, Lc = v.level(h), ca.level(2 * h)
            ok(k().gs_residual_restrict(C.byref(S), C.byref(Lf), mode, GAMMA, v.ptr, f.ptr, wp, ca.ptr, None,
                                        C.byref(Lc), st()))
            ca, cb = R.out(cd, "coarse_a"), R.out(cd, "coarse_b")
            ok(k().gs_residual_restrict(C.byref(S), C.byref(Lf), mode, GAMMA, v.ptr, f.ptr, wp, ca.ptr, cb.ptr,
                                        C.byref(Lc), st()))

        res = both(lid, body, f"residual_restrict {shape} m{mode}")
        if mode == 0:
            So = O.Stencil.make(*stencil) if stencil else None
            ref = inner(O.restrict(O.residual(v0, f0, h, 0, GAMMA, stencil=So)[0], cd))
            for n in res:
                same(res[n], ref, f"residual_restrict {n} against the oracle")


@by_layout
def test_residual_restrict_slab(lid):
    """gs_residual_restrict_slab, zhi = 1, on the lower m = 14 planes of (129, 17, 30): the planes above the slab are
    the level's own, so coarse planes 1..7 are the whole level's; the coarse planes above them are not written."""
    shape, m = (129, 17, 30), 14
    cd = half(shape)
    h = 1.0 / (shape[1] + 1)
    v0, f0 = fields(shape)[:2]
    for mode in (0, 1, 2, 3, 4):
        w0 = w_of(shape, mode)

        def body(R):
            v, f = R.inp(v0, name="v"), R.inp(f0, "noise", "f", name="f")
            w = R.inp(w0, "noise", name="w") if w0 is not None else None
            ca = R.out(cd, "coarse_a", written=("z", 1, m // 2))
            Ls, Lcs = level_of(v, h, nz=m), level_of(ca, 2 * h, nz=m // 2)
            assert k().gs_residual_restrict_slab_supported(C.byref(UNIT), C.byref(Ls)) == 1
            ok(k().gs_residual_restrict_slab(C.byref(UNIT), C.byref(Ls), mode, GAMMA, v.ptr, f.ptr,
                                             w.ptr if w else None, ca.ptr, None, C.byref(Lcs), 1, st()))

        res = both(lid, body, f"residual_restrict_slab m{mode}")
        if mode == 0:
            ref = O.restrict(O.residual(v0, f0, h, 0, GAMMA)[0], cd)
            same(res["coarse_a"], ref[1:-1, 1:-1, 1:m // 2 + 1], "residual_restrict_slab against the oracle")


# ---- transfer operators -------------------------------------------------------------------------------------------
@by_layout
@pytest.mark.parametrize("shape", [(3, 5, 7), (129, 33, 20)], ids=sid)
def test_transfer(shape, lid):
    """gs_restrict, gs_restrict2, gs_interpolate (the whole padded fine box is written), gs_prolong_add with and
    without coarse_sub."""
    cd = half(shape)
    fine0, base0 = fields(shape)[:2]
    c0, sub0 = fields(cd, 5)[:2]

    def body(R):
        fine, c, sub = R.inp(fine0, name="fine"), R.inp(c0, name="coarse"), R.inp(sub0, name="coarse_sub")
        Lf, Lc = fine.level(0.1), c.level(0.2)
        out = R.out(cd, "restrict")
        ok(k().gs_restrict(fine.ptr, C.byref(Lf), out.ptr, C.byref(Lc), st()))
        a, b = R.out(cd, "restrict2 a"), R.out(cd, "restrict2 b")
        ok(k().gs_restrict2(fine.ptr, C.byref(Lf), a.ptr, b.ptr, C.byref(Lc), st()))
        e = R.out(shape, "interpolate", written="box")
        ok(k().gs_interpolate(c.ptr, C.byref(Lc), e.ptr, C.byref(Lf), st()))
        v = R.inout(base0, "prolong_add")
        ok(k().gs_prolong_add(c.ptr, None, C.byref(Lc), v.ptr, C.byref(Lf), st()))
        v = R.inout(base0, "prolong_add sub")
        ok(k().gs_prolong_add(c.ptr, sub.ptr, C.byref(Lc), v.ptr, C.byref(Lf), st()))

    res = both(lid, body, f"transfer {shape}")
    r = inner(O.restrict(fine0, cd))
    for n in ("restrict", "restrict2 a", "restrict2 b"):
        same(res[n], r, n + " against the oracle")
    same(res["interpolate"], O.interpolate(c0, shape), "interpolate against the oracle")
    same(res["prolong_add"], inner(base0 + O.interpolate(c0, shape)), "prolong_add against the oracle")
    same(res["prolong_add sub"], inner(base0 + O.interpolate(c0 - sub0, shape)), "prolong_add (sub) against the oracle")


@by_layout
@pytest.mark.parametrize("cd", [(1, 1, 1), (3, 2, 5), (17, 9, 12)], ids=sid)
def test_fmg_prolong(cd, lid):
    """gs_fmg_prolong against tests/fmg_ref.prolong. The launcher stores fine pairs with one 16-byte store when
    al = (fine + 1 is 16-byte aligned and both fine pitches are even); the misaligned layouts are al == 0."""
    shape = tuple(2 * n + 1 for n in cd)
    c0 = noisy(fields(cd, 5)[0])  # the coarse ring takes part as data: any values, the same on both sides
    claimed = {}

    def body(R):
        c = R.inp(c0, name="coarse")
        out = R.out(shape, "fine")
        Lc, Lf = c.level(0.2), out.level(0.1)
        assert k().gs_fmg_prolong_supported(C.byref(Lc), C.byref(Lf)) == 1
        if R.lid is not None:  # the launcher's predicate, restated
            claimed["al"] = ((out.ptr + 8) & 15) == 0 and Lf.ldy % 2 == 0 and Lf.ldz % 2 == 0
        ok(k().gs_fmg_prolong(c.ptr, C.byref(Lc), out.ptr, C.byref(Lf), st()))

    res = both(lid, body, f"fmg_prolong {cd}")
    assert claimed["al"] == (lid in ("default", "tight_even", "loose"))
    same(res["fine"], inner(fmg_ref.prolong(c0)), "fmg_prolong against the numpy restatement")


# ---- the one-workgroup coarse cycle -------------------------------------------------------------------------------
def per_operator_cycle(lid, ld, mode, v0, f0, wpre, wpost):
    """The launch sequence gs_coarse_cycle replaces (CpuSolver::vcycle below ld[0]), one launcher per operator, on
    fields in the same-named layouts; returns every level's final iterate (interior)."""
    R, S, n = Side(lid), C.byref(UNIT), len(ld)
    lev = []
    for l, d in enumerate(ld):
        zero = np.zeros(tuple(x + 2 for x in d))
        q = dict(cur=R.inout(v0 if l == 0 else zero, f"v{l}"), alt=R.inout(zero, f"v_alt{l}"),
                 f=R.inp(f0, "noise", "f", name="f0") if l == 0 else R.inout(zero, f"f{l}", role="f"),
                 r=R.inout(zero, f"r{l}"), rv=R.inout(zero, f"rest_v{l}"),
                 w=R.inp(fields(d, 7)[2], "noise", name=f"newtonV{l}") if mode == 2 else None,
                 zero=l > 0 and mode != 1)
        q["L"], q["wp"] = q["cur"].level(1.0 / (d[1] + 1)), (q["w"].ptr if q["w"] else None)
        lev.append(q)

    def smooth(q, weights):
        for om in weights:
            ok(k().gs_jacobi_sweep(S, C.byref(q["L"]), mode, om, GAMMA, None if q["zero"] else q["cur"].ptr,
                                   q["alt"].ptr, q["f"].ptr, q["wp"], st()))
            q["cur"], q["alt"], q["zero"] = q["alt"], q["cur"], False

    for q, c in zip(lev, lev[1:]):
        smooth(q, wpre)
        ok(k().gs_residual(S, C.byref(q["L"]), mode, GAMMA, q["cur"].ptr, q["f"].ptr, q["wp"], q["r"].ptr, None, st()))
        ok(k().gs_restrict(q["r"].ptr, C.byref(q["L"]), c["f"].ptr, C.byref(c["L"]), st()))
        if mode == 1:  # FAS: restV = v_c = R v, f_c += A(restV)
            ok(k().gs_restrict2(q["cur"].ptr, C.byref(q["L"]), c["rv"].ptr, c["cur"].ptr, C.byref(c["L"]), st()))
            ok(k().gs_apply_op_add(S, C.byref(c["L"]), GAMMA, c["rv"].ptr, c["f"].ptr, st()))
    smooth(lev[-1], tuple(wpre) + tuple(wpost))
    for q, c in reversed(list(zip(lev, lev[1:]))):
        ok(k().gs_prolong_add(c["cur"].ptr, c["rv"].ptr if mode == 1 else None, C.byref(c["L"]), q["cur"].ptr,
                              C.byref(q["L"]), st()))
        smooth(q, wpost)
    R.finish()
    return [inner(q["cur"].to_xyz()) for q in lev]


@by_layout
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("dims", [(17, 9, 12), (33, 31, 29)], ids=sid)
def test_coarse_cycle(dims, mode, lid):
    """gs_coarse_cycle and gs_coarse_cycle_w from the hierarchy's second level down, each level in the same-named
    layout of its own extents: only interiors are written, the top level's f and every newtonV are unchanged, every
    level's iterate is the DevField run's and that of the per-operator launch sequence in the same layouts, and in
    LINEAR mode the weighted oracle V-cycle's (tests/weights_ref.py)."""
    ld = W.level_dims(dims)[1:]
    n = len(ld)
    assert 2 <= n <= k().gs_coarse_cycle_max_levels()
    pre, post = 2, 1
    f0 = fields(ld[0], 3)[1] * 0.02
    v0 = fields(ld[0], 3)[0] * 0.5

    def body(R, weighted):
        lv = (gsv._abi.gs_coarse_level * n)()
        for l, d in enumerate(ld):
            zero = np.zeros(tuple(x + 2 for x in d))
            v = R.inout(v0 if l == 0 else zero, f"v{l}")
            va = R.inout(zero, f"v_alt{l}")
            f = R.inp(f0, "noise", "f", name="f0") if l == 0 else R.inout(zero, f"f{l}", role="f")
            r = R.inout(zero, f"r{l}")
            rv = R.inout(zero, f"rest_v{l}") if mode == 1 else None
            w = R.inp(fields(d, 7)[2], "noise", name=f"newtonV{l}") if mode == 2 else None
            lv[l].v, lv[l].v_alt, lv[l].f, lv[l].r = v.ptr, va.ptr, f.ptr, r.ptr
            lv[l].rest_v = rv.ptr if rv else None
            lv[l].newton_v = w.ptr if w else None
            lv[l].geom = v.level(1.0 / (d[1] + 1))
            lv[l].v_zero = 0 if (l == 0 or mode == 1) else 1
            R.keep = getattr(R, "keep", []) + [(v, va, f, r, rv, w)]
        if weighted:
            ok(k().gs_coarse_cycle_w(C.byref(UNIT), lv, n, mode, arr(*(W2 + (1.1,))), GAMMA, pre, post, st()))
        else:
            ok(k().gs_coarse_cycle(C.byref(UNIT), lv, n, mode, OMEGA, GAMMA, pre, post, st()))

    for weighted in (False, True):
        res = both(lid, lambda R: body(R, weighted), f"coarse cycle {dims} m{mode} weighted={weighted}")
        wpre, wpost = (W2, (1.1,)) if weighted else ((OMEGA,) * pre, (OMEGA,) * post)
        it = "v_alt" if (pre + post) % 2 else "v"
        for l, want in enumerate(per_operator_cycle(lid, ld, mode, v0, f0, wpre, wpost)):
            same(res[it + str(l)], want, f"coarse cycle level {l} against the per-operator sequence")
        if mode == 0:
            ref = W.Cycle(ld[0], 0, pre=wpre, post=wpost, gamma=GAMMA, f0=f0, v0=v0)
            ref.vcycle_from(0)
            for l in range(n):
                same(res[it + str(l)], inner(ref.v[l]),
                     f"coarse cycle level {l} against the oracle")


# ---- elementwise ----------------------------------------------------------------------------------------------------
@by_layout
@pytest.mark.parametrize("z0", [0, 6])
@pytest.mark.parametrize("mode", [0, 1])
def test_rhs_init(mode, z0, lid):
    """gs_rhs_init: LINEAR writes the interior, NONLINEAR the whole padded box; a whole level and a slab (z0 = 6) of
    a taller one, against the oracle's right-hand side (bit for bit in LINEAR mode)."""
    nx, ny, NZ, nz = 37, 11, 15, 7
    h0 = 1.0 / (ny + 1)
    shape = (nx, ny, NZ if z0 == 0 else nz)

    def body(R):
        f = R.out(shape, "f", written="interior" if mode == 0 else "box")
        ok(k().gs_rhs_init(C.byref(f.level(h0, z0)), f.ptr, mode, h0, GAMMA, st()))

    res = both(lid, body, f"rhs_init m{mode} z0={z0}")
    ref = O.rhs(nx, ny, NZ, mode, GAMMA, h0)[:, :, z0: z0 + shape[2] + 2]
    if mode == 0:
        same(res["f"], inner(ref), "rhs_init against the oracle")
    else:
        assert np.abs(res["f"] - ref).max() <= 1e-12 * np.abs(ref).max()


@pytest.mark.parametrize("want", [-1, 0, 1])
def test_newton_bfac_heads(want):
    """gs_newton_bfac's three alignment paths: head = -1 (w and b at different 16-byte phases: the element-wise
    kernel), 0 and 1 (a common phase: dwordx4 bodies after 0 or 1 leading elements). The predicate is restated from
    the launcher. b = gamma (1 + w) e^w at every element of planes -1 .. nz+2 at full pitch, and nothing else."""
    shape = (37, 11, 9)
    lay = layouts(*shape)["default"]
    pw, pb = {-1: (0, 8), 0: (8, 8), 1: (0, 0)}[want]
    w = LayoutField(*shape, lay.ldy, lay.ldz, pw)
    b = LayoutField(*shape, lay.ldy, lay.ldz, pb)
    a, c = b.ptr - 8 * b.ldz, w.ptr - 8 * w.ldz
    head = -1 if ((a ^ c) & 15) else (a & 15) // 8
    assert head == want
    rng = np.random.default_rng(want + 5)
    w.poison_all(POISON_IN)
    w.buf[w.planes_mask()] = torch.from_numpy(rng.uniform(-0.8, 0.8, w.planes)).cuda()
    w.snapshot()
    b.poison_all()
    L = w.level(1.0 / 12)
    ok(k().gs_newton_bfac(C.byref(L), GAMMA, w.ptr, b.ptr, st()))
    b.assert_written_exactly(b.planes_mask(), f"bfac head {want}")
    w.assert_unchanged(what="bfac w")
    # against the element-wise path on an ordinary pair of DevFields with the same words (the rest of the suite pins
    # its values to gamma (1 + w) e^w at the Newton modes' tolerance)
    got = b.buf[b.planes_mask()].cpu().numpy()
    win = w.buf[w.planes_mask()].cpu().numpy()
    ref = GAMMA * (1.0 + win) * np.exp(win)
    assert np.abs(got - ref).max() <= 1e-14 * np.abs(ref).max()
    dw, db = DevField(*shape), DevField(*shape)
    dw.zyx_ext[:, :, : shape[0] + 2] = w._ext(w.buf)
    ok(k().gs_newton_bfac(C.byref(dw.level(1.0 / 12)), GAMMA, dw.ptr, db.ptr, st()))
    torch.cuda.synchronize()
    assert torch.equal(db.zyx_ext[:, :, : shape[0] + 2].contiguous().view(torch.int64),
                       b._ext(b.buf).contiguous().view(torch.int64))
    # overlapping fields are refused
    assert k().gs_newton_bfac(C.byref(L), GAMMA, w.ptr, w.ptr + 8 * w.ldz, st()) == EINVAL
    w.assert_unchanged(what="bfac refused")


@pytest.mark.parametrize("n", [1, 2, 255, 256, 1001, 70001, 600002])
@pytest.mark.parametrize("pd,ps", [(0, 0), (8, 8), (0, 8), (8, 0)])
def test_copy_fill_axpy_sumsq(pd, ps, n):
    """gs_copy (head 0, head 1 and — no common 16-byte phase — the hipMemcpyAsync fallback, each by the launcher's
    restated predicate), gs_fill, gs_axpy and gs_sumsq_finish at both phases, odd and even n, guards on both sides."""
    rng = np.random.default_rng(n + pd + 3 * ps)
    dst, src = Parts(n, pd == 8), Parts(n, ps == 8)
    x = rng.uniform(-1, 1, n)
    src.t[src.o:src.o + n] = torch.from_numpy(x).cuda()
    snap = src.t.clone()
    path = "memcpy" if ((dst.ptr ^ src.ptr) & 15) else ("head1" if dst.ptr & 15 else "head0")
    assert path == {(0, 0): "head0", (8, 8): "head1", (0, 8): "memcpy", (8, 0): "memcpy"}[(pd, ps)]
    ok(k().gs_copy(dst.ptr, src.ptr, n, st()))
    same(dst.result("copy"), x, f"copy {path}")
    ok(k().gs_axpy(dst.ptr, src.ptr, -1.0, n, st()))
    same(dst.result("axpy"), x - x, "axpy")
    ok(k().gs_fill(dst.ptr, 2.5, n, st()))
    same(dst.result("fill"), np.full(n, 2.5), "fill")
    ok(k().gs_axpy(dst.ptr, src.ptr, 0.5, n, st()))
    same(dst.result("axpy"), 2.5 + 0.5 * x, "axpy")
    torch.cuda.synchronize()
    assert torch.equal(src.t.view(torch.int64), snap.view(torch.int64)), "the source changed"
    # gs_sumsq_finish: partials (the non-negative squares) at this phase, the result next to a guard
    sq = Parts(n, ps == 8)
    sq.t[sq.o:sq.o + n] = torch.from_numpy(x * x).cuda()
    for acc in (0, 1):
        out = Parts(1, pd == 8)
        ok(k().gs_sumsq_finish(sq.ptr, n, out.ptr, acc, st()))
        got, want = out.result("sumsq")[0], float(np.sum(x * x))
        assert abs(got - (want if acc else np.sqrt(want))) <= n * 2.0 ** -52 * want + 1e-300


# ---- rejections, and the list of launchers -------------------------------------------------------------------------
def launcher_table():
    """name -> call(L, Lc) with otherwise valid arguments, for every launcher that takes a level (fine L = 15^3, coarse
    Lc = 7^3, which is both its half and the level it is 2 n + 1 of; the buffers are poisoned LayoutFields in the default layout, shared by all calls)."""
    shape, cd = (15, 15, 15), (7, 7, 7)
    lay, clay = layouts(*shape)["default"], layouts(*cd)["default"]
    F = [LayoutField(*shape, lay.ldy, lay.ldz, 0).poison_all() for _ in range(6)]
    Cc = [LayoutField(*cd, clay.ldy, clay.ldz, 0).poison_all() for _ in range(3)]
    p = Parts(70000, False)
    a, b, c, d, e, g = (x.ptr for x in F)
    ca, cb, cc = (x.ptr for x in Cc)
    S, s, B = C.byref(UNIT), st(), C.byref
    kk = k()
    w2, w3 = arr(*W2), arr(*W3)

    def coarse(fn, L, Lc, *mid):
        lv = (gsv._abi.gs_coarse_level * 2)()
        for i, (lev, q) in enumerate(((L, (a, b, c, d)), (Lc, (ca, cb, cc, None)))):
            lv[i].v, lv[i].v_alt, lv[i].f, lv[i].r = q
            lv[i].geom, lv[i].v_zero = lev, i
        return fn(S, lv, 2, 0, *mid, GAMMA, 1, 1, s)

    T = {
        "gs_rhs_init": lambda L, Lc: kk.gs_rhs_init(B(L), a, 0, 0.1, GAMMA, s),
        "gs_jacobi_sweep": lambda L, Lc: kk.gs_jacobi_sweep(S, B(L), 0, OMEGA, GAMMA, a, b, c, None, s),
        "gs_jacobi_sweep_norm": lambda L, Lc: kk.gs_jacobi_sweep_norm(S, B(L), 0, OMEGA, GAMMA, a, b, c, None, p.ptr, s),
        "gs_jacobi_sweep2": lambda L, Lc: kk.gs_jacobi_sweep2(S, B(L), 0, OMEGA, GAMMA, a, b, c, None, 0, 0, s),
        "gs_jacobi_sweep2_w": lambda L, Lc: kk.gs_jacobi_sweep2_w(S, B(L), 0, w2, GAMMA, a, b, c, None, 0, 0, s),
        "gs_jacobi_sweep2_norm": lambda L, Lc: kk.gs_jacobi_sweep2_norm(S, B(L), 0, OMEGA, GAMMA, a, b, c, None, 0, 0,
                                                                        p.ptr, s),
        "gs_jacobi_sweep2_norm_w": lambda L, Lc: kk.gs_jacobi_sweep2_norm_w(S, B(L), 0, w2, GAMMA, a, b, c, None, 0, 0,
                                                                            p.ptr, s),
        "gs_jacobi_sweep3": lambda L, Lc: kk.gs_jacobi_sweep3(S, B(L), OMEGA, GAMMA, a, b, c, s),
        "gs_jacobi_sweep3_w": lambda L, Lc: kk.gs_jacobi_sweep3_w(S, B(L), w3, GAMMA, a, b, c, s),
        "gs_jacobi_sweep2_prolong": lambda L, Lc: kk.gs_jacobi_sweep2_prolong(S, B(L), 0, OMEGA, GAMMA, a, ca, None, B(Lc),
                                                                              b, c, None, 0, 0, s),
        "gs_jacobi_sweep2_prolong_w": lambda L, Lc: kk.gs_jacobi_sweep2_prolong_w(S, B(L), 0, w2, GAMMA, a, ca, None,
                                                                                  B(Lc), b, c, None, 0, 0, s),
        "gs_jacobi_sweep2_prolong_ws": lambda L, Lc: kk.gs_jacobi_sweep2_prolong_ws(S, B(L), 0, OMEGA, GAMMA, a, ca, None,
                                                                                    B(Lc), b, c, None, 0, 0, p.ptr,
                                                                                    70000, s),
        "gs_jacobi_sweep2_prolong_ws_w": lambda L, Lc: kk.gs_jacobi_sweep2_prolong_ws_w(S, B(L), 0, w2, GAMMA, a, ca,
                                                                                        None, B(Lc), b, c, None, 0, 0,
                                                                                        p.ptr, 70000, s),
        "gs_smooth2_restrict_tiled": lambda L, Lc: kk.gs_smooth2_restrict_tiled(S, B(L), 0, OMEGA, GAMMA, a, b, c, None,
                                                                                ca, B(Lc), s),
        "gs_smooth2_restrict_tiled_w": lambda L, Lc: kk.gs_smooth2_restrict_tiled_w(S, B(L), 0, w2, GAMMA, a, b, c, None,
                                                                                    ca, B(Lc), s),
        "gs_prolong_smooth2_tiled": lambda L, Lc: kk.gs_prolong_smooth2_tiled(S, B(L), 0, OMEGA, GAMMA, a, ca, B(Lc), b,
                                                                              c, None, s),
        "gs_prolong_smooth2_tiled_w": lambda L, Lc: kk.gs_prolong_smooth2_tiled_w(S, B(L), 0, w2, GAMMA, a, ca, B(Lc), b,
                                                                                  c, None, s),
        "gs_residual": lambda L, Lc: kk.gs_residual(S, B(L), 0, GAMMA, a, c, None, b, p.ptr, s),
        "gs_residual_restrict": lambda L, Lc: kk.gs_residual_restrict(S, B(L), 0, GAMMA, a, c, None, ca, cb, B(Lc), s),
        "gs_residual_restrict_slab": lambda L, Lc: kk.gs_residual_restrict_slab(S, B(L), 0, GAMMA, a, c, None, ca, cb,
                                                                                B(Lc), 0, s),
        "gs_restrict": lambda L, Lc: kk.gs_restrict(a, B(L), ca, B(Lc), s),
        "gs_restrict2": lambda L, Lc: kk.gs_restrict2(a, B(L), ca, cb, B(Lc), s),
        "gs_interpolate": lambda L, Lc: kk.gs_interpolate(ca, B(Lc), a, B(L), s),
        "gs_prolong_add": lambda L, Lc: kk.gs_prolong_add(ca, None, B(Lc), a, B(L), s),
        "gs_apply_op": lambda L, Lc: kk.gs_apply_op(S, B(L), GAMMA, a, b, s),
        "gs_apply_op_add": lambda L, Lc: kk.gs_apply_op_add(S, B(L), GAMMA, a, b, s),
        "gs_newton_F": lambda L, Lc: kk.gs_newton_F(S, B(L), GAMMA, a, c, b, p.ptr, s),
        "gs_newton_F_update": lambda L, Lc: kk.gs_newton_F_update(S, B(L), GAMMA, a, b, c, d, e, p.ptr, s),
        "gs_newton_F_update_restrict": lambda L, Lc: kk.gs_newton_F_update_restrict(S, B(L), GAMMA, a, b, c, d, e, p.ptr,
                                                                                    ca, B(Lc), s),
        "gs_newton_F_update_restrict_bfac": lambda L, Lc: kk.gs_newton_F_update_restrict_bfac(S, B(L), GAMMA, a, b, c, d,
                                                                                              e, p.ptr, ca, B(Lc), g, s),
        "gs_newton_bfac": lambda L, Lc: kk.gs_newton_bfac(B(L), GAMMA, a, b, s),
        "gs_coarse_cycle": lambda L, Lc: coarse(kk.gs_coarse_cycle, L, Lc, OMEGA),
        "gs_coarse_cycle_w": lambda L, Lc: coarse(kk.gs_coarse_cycle_w, L, Lc, w2),
    }
    T["gs_fmg_prolong"] = lambda L, Lc: kk.gs_fmg_prolong(ca, B(Lc), a, B(L), s)
    return T, F + Cc, p, lay, clay, shape, cd


TWO_LEVEL = {"gs_jacobi_sweep2_prolong", "gs_jacobi_sweep2_prolong_w", "gs_jacobi_sweep2_prolong_ws",
             "gs_jacobi_sweep2_prolong_ws_w", "gs_smooth2_restrict_tiled", "gs_smooth2_restrict_tiled_w",
             "gs_prolong_smooth2_tiled", "gs_prolong_smooth2_tiled_w", "gs_residual_restrict", "gs_residual_restrict_slab",
             "gs_restrict", "gs_restrict2", "gs_interpolate", "gs_prolong_add", "gs_newton_F_update_restrict",
             "gs_newton_F_update_restrict_bfac", "gs_coarse_cycle", "gs_coarse_cycle_w", "gs_fmg_prolong"}
NO_LEVEL = {"gs_sumsq_finish", "gs_fill", "gs_copy", "gs_axpy"}


def test_bad_pitches_are_refused():
    """ldy = nx + 1 and ldz = ldy (ny + 2) - 1 — on the fine level and, where there is one, on the coarse level — are
    GS_EINVAL from every launcher that takes a level, and nothing is written."""
    T, flds, p, lay, clay, shape, cd = launcher_table()
    good = gsv.gs_level(*shape, lay.ldy, lay.ldz, 0, 1.0 / 16)
    cgood = gsv.gs_level(*cd, clay.ldy, clay.ldz, 0, 1.0 / 8)
    bad = [gsv.gs_level(*shape, shape[0] + 1, lay.ldz, 0, 1.0 / 16),
           gsv.gs_level(*shape, lay.ldy, lay.ldy * (shape[1] + 2) - 1, 0, 1.0 / 16)]
    cbad = [gsv.gs_level(*cd, cd[0] + 1, clay.ldz, 0, 1.0 / 8),
            gsv.gs_level(*cd, clay.ldy, clay.ldy * (cd[1] + 2) - 1, 0, 1.0 / 8)]
    for name, call in T.items():
        for L in bad:
            assert call(L, cgood) == EINVAL, (name, "fine", L.ldy, L.ldz)
        if name in TWO_LEVEL:
            for Lc in cbad:
                assert call(good, Lc) == EINVAL, (name, "coarse", Lc.ldy, Lc.ldz)
    torch.cuda.synchronize()
    for f in flds:
        assert bool((f.i64 == POISON_OUT).all()), "a refused call wrote a field"
    assert bool((p.t.view(torch.int64) == POISON_OUT).all()), "a refused call wrote partials"


# launcher -> the test of this file that runs it in every layout
MATRIX = {
    "gs_rhs_init": "test_rhs_init",
    "gs_jacobi_sweep": "test_generic_pass", "gs_jacobi_sweep_norm": "test_generic_pass",
    "gs_residual": "test_generic_pass",
    "gs_apply_op": "test_generic_operators", "gs_apply_op_add": "test_generic_operators",
    "gs_newton_F": "test_generic_operators",
    "gs_newton_F_update": "test_newton_update", "gs_newton_F_update_restrict": "test_newton_update",
    "gs_newton_F_update_restrict_bfac": "test_newton_update",
    "gs_jacobi_sweep2": "test_pairs", "gs_jacobi_sweep2_norm": "test_pairs", "gs_jacobi_sweep2_w": "test_pairs",
    "gs_jacobi_sweep2_norm_w": "test_pairs",
    "gs_jacobi_sweep3": "test_triples", "gs_jacobi_sweep3_w": "test_triples",
    "gs_jacobi_sweep2_prolong": "test_prolong_pairs", "gs_jacobi_sweep2_prolong_w": "test_prolong_pairs",
    "gs_jacobi_sweep2_prolong_ws": "test_prolong_pairs", "gs_jacobi_sweep2_prolong_ws_w": "test_prolong_pairs",
    "gs_smooth2_restrict_tiled": "test_tiled", "gs_smooth2_restrict_tiled_w": "test_tiled",
    "gs_prolong_smooth2_tiled": "test_tiled", "gs_prolong_smooth2_tiled_w": "test_tiled",
    "gs_residual_restrict": "test_residual_restrict", "gs_residual_restrict_slab": "test_residual_restrict_slab",
    "gs_restrict": "test_transfer", "gs_restrict2": "test_transfer", "gs_interpolate": "test_transfer",
    "gs_prolong_add": "test_transfer", "gs_fmg_prolong": "test_fmg_prolong",
    "gs_coarse_cycle": "test_coarse_cycle", "gs_coarse_cycle_w": "test_coarse_cycle",
    "gs_newton_bfac": "test_newton_bfac_heads",
    "gs_sumsq_finish": "test_copy_fill_axpy_sumsq", "gs_fill": "test_copy_fill_axpy_sumsq",
    "gs_copy": "test_copy_fill_axpy_sumsq", "gs_axpy": "test_copy_fill_axpy_sumsq",
}


def header_launchers():
    """Every function of include/gpusolve_hip.h that takes a stream: the launchers."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gpusolve_hip.h")
    with open(path) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return {m.group(1) for m in re.finditer(r"\bint\s+(gs_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S)
            if "hipStream_t" in m.group(2)}


def test_every_launcher_is_in_the_matrix():
    """The header's launchers, the matrix above, the rejection table and the source of the tests named agree."""
    launchers = header_launchers()
    assert len(launchers) >= 38 and "gs_jacobi_sweep3_w" in launchers and "gs_field_layout" not in launchers
    assert launchers == set(MATRIX), (sorted(launchers - set(MATRIX)), sorted(set(MATRIX) - launchers))
    T = launcher_table()[0]
    assert set(T) == launchers - NO_LEVEL
    import inspect
    here = globals()
    helpers = inspect.getsource(pass_launchers) + inspect.getsource(operator_launchers) + \
        inspect.getsource(pair_launch) + inspect.getsource(prolong_launch)
    for name, test in MATRIX.items():
        assert test in here and callable(here[test]), (name, test)
        src = inspect.getsource(here[test]) + helpers
        assert re.search(r"\b" + name + r"\(", src), f"{test} does not call {name}"
