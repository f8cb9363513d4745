"""k_zline_lds on the GPU (csrc/gs_line_device.hpp): the z-line sweep of levels with few, long columns
— fewer than 32 * 32 columns, ZF_MIN_NZ to ZF_MAX_NZ planes, any order of the stencil's entries — whose recurrence
runs out of LDS. tests/test_gpu_zline.py's harness at the shapes that select it, and the driver on grids whose line
levels select it.

Tolerances. None: the instance keeps include/gpusolve_line.h's evaluation order, so every word of a sweep's output and
of every level's v and f equals tests/zline_ref.py's (through semi_ref.Cycle and zline_ref.ZCycle for the driver).
Norms to 1e-12 (the device's fixed-order sum of squares against the oracle's).

Shapes of the launcher test (a block owns ZF_CB = 8 consecutive columns of the flattened index x - 1 + nx * (y - 1);
phase A and C cover 32 planes per pass; the forward ring holds 4 planes, the backward ring 8):
  (1, 1, MIN)       one chain lane, the smallest plane count
  (8, 1, MIN)       one full tile
  (7, 1, MIN + 1)   a ragged tile; an odd plane count: both rings end inside a group
  (9, 2, MIN + 3)   18 columns: two full tiles, the second across the row end, and a tile of two columns
  (3, 3, 257)       more planes than one pass of phases A and C covers, by one; a second block of one column
  (33, 31, MIN)     the largest column count (1023: 128 blocks, the last with seven columns)
  (1, 1, MAX)       the whole LDS array"""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import gpusolve as gsv  # noqa: E402
import oracle as O  # noqa: E402
import pcg_ref as P  # noqa: E402
import semi_ref as S  # noqa: E402
import zline_ref as Z  # noqa: E402
from gpusolve import _abi as A  # noqa: E402
from layout_field import LAYOUT_IDS, POISON_OUT, LayoutField, layouts  # noqa: E402

ZF_CB, ZF_MIN_NZ, ZF_MAX_NZ = 8, 64, 1536  # csrc/gs_line_device.hpp
MARCH_COLUMNS = 32 * 32                    # ZL_MARCH_COLUMNS of csrc/gs_line.hip
SHAPES = [(1, 1, ZF_MIN_NZ), (ZF_CB, 1, ZF_MIN_NZ), (ZF_CB - 1, 1, ZF_MIN_NZ + 1), (ZF_CB + 1, 2, ZF_MIN_NZ + 3),
          (3, 3, 257), (33, 31, ZF_MIN_NZ), (1, 1, ZF_MAX_NZ)]
STENCILS = {
    "strongz": (Z.STRONGZ, list(O.CANONICAL)),
    "iso": (Z.ISO, list(O.CANONICAL)),
    "uplo": (Z.UPLO, list(O.CANONICAL)),
    "permuted": Z.permuted(Z.UPLO),
}
LN = None


def ln():
    global LN
    if LN is None:
        assert torch.cuda.is_available(), "GPU tests need a GPU (no CPU fallback exists)"
        LN = gsv.line()
    return LN


def st():
    return torch.cuda.current_stream().cuda_stream


def sid(shape):
    return "x".join(str(n) for n in shape)


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def same(a, b, what):
    ne = bits(a) != bits(b)
    assert a.shape == b.shape and not ne.any(), \
        f"{what}: {int(ne.sum())} words differ, first at {tuple(np.argwhere(ne)[0])}"


def abi(values, offsets):
    return gsv.Stencil(list(values), [tuple(o) for o in offsets]).to_abi()


def lds(zero):
    return f"k_zline_lds<{'true' if zero else 'false'}>"


class Tables:
    """A level's factors on the device (gs_zline_factors' own output), each between poisoned guards."""

    def __init__(self, stencil, nz):
        cp, den = np.zeros(nz + 2), np.zeros(nz + 2)
        assert ln().gs_zline_factors(C.byref(stencil), nz, cp.ctypes.data_as(A.dptr), den.ctypes.data_as(A.dptr)) == 0
        self.t = torch.zeros(2 * (nz + 2) + 24, dtype=torch.float64, device="cuda")
        self.t.view(torch.int64).fill_(POISON_OUT)
        self.t[8:8 + nz + 2] = torch.from_numpy(cp).cuda()
        self.t[16 + nz + 2:16 + 2 * (nz + 2)] = torch.from_numpy(den).cuda()
        base = self.t.data_ptr()
        self.abi = A.gs_zline_tables(base + 64, base + 8 * (16 + nz + 2), nz)


@functools.lru_cache(maxsize=None)
def host_inputs(shape):
    """(v, f) on the host, shared by every layout: v's ring zero, f's ring noise."""
    rng = np.random.default_rng(23 + shape[0] * shape[1] * shape[2])
    va, fa = O.zeros(*shape), rng.standard_normal(tuple(s + 2 for s in shape)) * 100.0  # (ring included: noise)
    P.inner(va)[...] = rng.standard_normal(shape)
    return va, fa


@functools.lru_cache(maxsize=None)
def wanted(shape, sname, omega, zero):
    """The model's sweep, computed once per case and left unchanged."""
    va, fa = host_inputs(shape)
    values, offsets = STENCILS[sname]
    out = Z.sweep(None if zero else va, fa, 1.0 / (shape[1] + 1), omega, values, offsets)
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("lid", LAYOUT_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_sweep_bit_for_bit(shape, lid):
    """NaN outside every input's box, noise in f's ring, a NaN-filled output: exactly the interior is written, the
    inputs keep every word, and the result is the model's bit for bit — by the LDS instance in every case."""
    lay = layouts(*shape)[lid]
    h = 1.0 / (shape[1] + 1)
    va, fa = host_inputs(shape)
    v = LayoutField(*shape, lay.ldy, lay.ldz, lay.phase_in).from_xyz(va).poison_outside_box().snapshot()
    f = LayoutField(*shape, lay.ldy, lay.ldz, lay.phase_out).from_xyz(fa).poison_outside_box().snapshot()
    L = v.level(h)
    out = LayoutField(*shape, lay.ldy, lay.ldz, lay.phase_out)
    interior = out.interior_mask()
    for sname, (values, offsets) in STENCILS.items():
        stencil = abi(values, offsets)
        T = Tables(stencil, shape[2])
        for omega in (1.0, 0.8):
            for zero in (False, True):
                what = f"gs_zline_sweep {sid(shape)} {lid} {sname} omega={omega} zero={zero}"
                assert ln().gs_zline_kernel(C.byref(stencil), C.byref(L), int(zero)).decode() == lds(zero), what
                out.poison_all()
                rc = ln().gs_zline_sweep(C.byref(stencil), C.byref(L), omega, None if zero else v.ptr, out.ptr, f.ptr,
                                         C.byref(T.abi), st())
                assert rc == 0, what
                out.assert_written_exactly(interior, what + " v_out")
                v.assert_unchanged(what=what + " v_in")
                f.assert_unchanged(what=what + " f")
                same(P.inner(out.to_xyz()), P.inner(wanted(shape, sname, omega, zero)), what)


# ---- the driver ---------------------------------------------------------------------------------------------------
XY_STENCILS = {"WEAKZ": (Z.WEAKZ, list(O.CANONICAL)), "PERM": Z.permuted(Z.UPLO)}


def line_instances(g):
    """Level -> the instance gs_zline_sweep takes on it (non-zero iterate), for the levels that run line sweeps."""
    out = {}
    for l in range(g.numLevels()):
        if g.level_smoother(l) != "zline":
            continue
        nx, ny, nz = g.getLevel(l).levelDim
        ldy, ldz, _, _ = gsv.field_layout(nx, ny, nz)
        L = gsv.gs_level(nx, ny, nz, ldy, ldz, 0, g.getLevel(l).h)
        stencil = g.level_stencil(l).to_abi()
        out[l] = ln().gs_zline_kernel(C.byref(stencil), C.byref(L), 0).decode()
    return out


@pytest.mark.parametrize("sname,smoother", [("WEAKZ", "zline"), ("WEAKZ", "auto"), ("PERM", "zline")])
@pytest.mark.parametrize("dims", [(31, 31, ZF_MIN_NZ), (16, 12, ZF_MIN_NZ + 6)], ids=sid)
def test_xy_cycles_against_the_model(dims, sname, smoother):
    """XY hierarchies whose line levels all have fewer than 32 * 32 columns: every level's v and f word for word after
    one and after three V-cycles, the closing norms to 1e-12."""
    values, offsets = XY_STENCILS[sname]
    f = Z.normal_rhs(dims, 3)
    c = S.Cycle(dims, values, offsets, smoother=smoother, f0=f)
    p = gsv.GridParams(maxiter=3, tol=0.0, gridDim=dims, mode=gsv.GS_LINEAR, preSmoothing=2, postSmoothing=2,
                       stencil=gsv.Stencil(list(values), [tuple(o) for o in offsets]))
    with gsv.HipGridData(p, coarsen="xy") as g:
        g.set_field(0, "f", f)
        g.set_smoother(smoother)
        assert g.numLevels() == len(c.ld)
        inst = line_instances(g)
        assert sorted(inst) == [l for l, z in enumerate(c.line) if z] != [], c.pattern()
        for l, name in inst.items():
            nx, ny, nz = c.ld[l]
            assert nx * ny < MARCH_COLUMNS and ZF_MIN_NZ <= nz <= ZF_MAX_NZ and name == lds(False), (l, c.ld[l], name)
        for k in range(3):
            got, want = gsv.HipSolver.vcycle(g), c.vcycle()
            print(f"{sid(dims)} {sname} {smoother} cycle {k}: device {got!r} model {want!r}")
            assert np.isfinite(want) and abs(got - want) <= 1e-12 * want
            if k in (0, 2):
                for l in range(len(c.ld)):
                    same(g.field(l, "v"), c.v[l], f"level {l}'s v after cycle {k + 1}")
                    same(g.field(l, "f"), c.f[l], f"level {l}'s f after cycle {k + 1}")


def test_full_coarsening_cycles_mix_the_instances():
    """(15, 15, 2 MIN - 1) under ZLINE with full coarsening: level 0 runs the LDS instance, level 1 (MIN - 1 planes)
    and the levels below it k_zline_col; level 0 word for word after each of two cycles."""
    dims = (15, 15, 2 * ZF_MIN_NZ - 1)
    f = Z.normal_rhs(dims, 5)
    c = Z.ZCycle(dims, Z.STRONGZ, f0=f)
    p = gsv.GridParams(maxiter=2, tol=0.0, gridDim=dims, mode=gsv.GS_LINEAR, preSmoothing=2, postSmoothing=2,
                       stencil=gsv.Stencil(list(Z.STRONGZ)))
    with gsv.HipGridData(p) as g:
        g.set_field(0, "f", f)
        g.set_smoother("zline")
        inst = line_instances(g)
        assert g.getLevel(1).levelDim[2] == ZF_MIN_NZ - 1
        assert inst[0] == lds(False) and all(inst[l] == "k_zline_col<false>" for l in range(1, g.numLevels())), inst
        for k in range(2):
            got, want = gsv.HipSolver.vcycle(g), c.vcycle()
            print(f"cycle {k}: device {got!r} model {want!r}")
            same(g.field(0, "v"), c.v[0], f"level 0's v after cycle {k + 1}")
            assert abs(got - want) <= 1e-12 * want
        same(g.field(0, "f"), f, "level 0's f")
