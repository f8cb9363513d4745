"""tests/layout_field.py on host memory: the layouts it names are layouts the ABI accepts, its masks partition the
buffer, its copies round-trip, and its checks have teeth — a torch-written fake "kernel" with one planted fault is
caught every time, a correct one passes. No GPU."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
import gpusolve as gsv  # noqa: E402
from layout_field import (ALIGNED_IDS, LAYOUT_IDS, POISON_IN, POISON_OUT, LayoutField, default_pitches,  # noqa: E402
                          layouts)

# nx odd, nx even, nx + 2 already a multiple of 16 (and of 128), a single point
EXTENTS = [(5, 3, 4), (8, 2, 3), (14, 3, 2), (126, 2, 1), (1, 1, 1)]
cases = pytest.mark.parametrize("lid", LAYOUT_IDS)
extents = pytest.mark.parametrize("dims", EXTENTS, ids=lambda d: "x".join(map(str, d)))


def make(dims, lid, out=False):
    lay = layouts(*dims)[lid]
    return LayoutField(*dims, lay.ldy, lay.ldz, lay.phase_out if out else lay.phase_in, device="cpu")


def rand_box(dims, seed=0, ext=0):
    return np.random.default_rng(seed).uniform(1.0, 2.0, (dims[0] + 2, dims[1] + 2, dims[2] + 2 + ext))


@extents
def test_default_pitches_are_the_librarys(dims):
    assert default_pitches(*dims) == gsv.field_layout(*dims)[:2]


@extents
@cases
def test_pitches_and_phase(dims, lid):
    nx, ny, nz = dims
    lay = layouts(*dims)[lid]
    assert lay.ldy >= nx + 2 and lay.ldz >= lay.ldy * (ny + 2)  # bad_level's inequalities
    D, Dz = default_pitches(*dims)
    want = {"default": (D, Dz, 0, 0), "loose": (D + 6, (D + 6) * (ny + 2) + 10, 64, 64), "mixed": (D, Dz, 0, 8)}
    if lid in want:
        assert (lay.ldy, lay.ldz, lay.phase_in, lay.phase_out) == want[lid]
    if lid == "tight_even":
        assert lay.ldy % 2 == 0 and lay.ldy - (nx + 2) in (0, 1) and lay.ldz == lay.ldy * (ny + 2)
        assert (lay.phase_in, lay.phase_out) == (16, 16)
    if lid == "tight_odd":
        assert lay.ldy % 2 == 1 and lay.ldy - (nx + 2) in (0, 1)
        assert lay.ldz % 2 == 1 and lay.ldz - lay.ldy * (ny + 2) in (0, 1)
        assert (lay.phase_in, lay.phase_out) == (8, 8)
    assert lay.aligned == (lid in ALIGNED_IDS)
    for out in (False, True):
        f = make(dims, lid, out)
        phase = lay.phase_out if out else lay.phase_in
        assert (f.ptr + 8) % 128 == phase and f.ptr == f.buf.data_ptr() + 8 * f.origin
        # the aligned class: every pair (x odd, x+1) of every row and plane starts 16-byte aligned; the others not
        pair_aligned = all((f.ptr + 8 * (1 + y * f.ldy + z * f.ldz)) % 16 == 0 for y in range(ny + 2)
                           for z in range(nz + 2))
        if lay.aligned:
            assert pair_aligned
        elif lid == "tight_odd":
            assert not pair_aligned
        else:
            assert pair_aligned != out  # mixed: inputs aligned, outputs and f not
        # the margins: at least 2 ldz + 64 elements before plane -1 and after plane nz+2
        assert f.origin - f.ldz >= 2 * f.ldz + 64
        assert f.buf.numel() - (f.origin + (nz + 3) * f.ldz) >= 2 * f.ldz + 64
        L = f.level(0.25, 3)
        assert (L.nx, L.ny, L.nz, L.ldy, L.ldz, L.z0, L.h) == (nx, ny, nz, f.ldy, f.ldz, 3, 0.25)


@extents
@cases
def test_masks_partition_the_buffer(dims, lid):
    nx, ny, nz = dims
    f = make(dims, lid)
    box, inner, ext, planes = f.box_mask(), f.interior_mask(), f.ext_box_mask(), f.planes_mask()
    assert int(box.sum()) == (nx + 2) * (ny + 2) * (nz + 2)
    assert int(inner.sum()) == nx * ny * nz
    assert int(ext.sum()) == (nx + 2) * (ny + 2) * (nz + 4)
    assert int(planes.sum()) == f.ldz * (nz + 4)
    for small, big in ((inner, box), (box, ext), (ext, planes)):
        assert not bool((small & ~big).any())
    # interior | ring | outside the box: disjoint, and together the whole buffer
    ring, outside = box & ~inner, ~box
    assert int(inner.sum()) + int(ring.sum()) + int(outside.sum()) == f.buf.numel()
    # the box is where element (x, y, z) lives by the header's formula
    idx = torch.nonzero(box).ravel().numpy() - f.origin
    want = sorted(x + y * f.ldy + z * f.ldz for z in range(nz + 2) for y in range(ny + 2) for x in range(nx + 2))
    assert idx.tolist() == want


@extents
@cases
def test_round_trip(dims, lid):
    f = make(dims, lid)
    a = rand_box(dims, 1)
    f.poison_all().from_xyz(a)
    assert np.array_equal(f.to_xyz(), a)
    assert bool((f.i64[~f.box_mask()] == POISON_OUT).all())  # from_xyz writes the box alone
    e = rand_box(dims, 2, ext=2)
    f.from_xyz_ext(e)
    assert np.array_equal(f.to_xyz_ext(), e) and np.array_equal(f.to_xyz(), e[:, :, 1:-1])
    assert bool((f.i64[~f.ext_box_mask()] == POISON_OUT).all())
    f.from_xyz(a).poison_outside_box()
    assert np.array_equal(f.to_xyz(), a)
    assert bool((f.i64[~f.box_mask()] == POISON_IN).all())
    assert bool(torch.isnan(f.buf[~f.box_mask()]).all())


# ---- the harness has teeth --------------------------------------------------------------------------------------
def fake_kernel(src, dst, fault=None):
    """dst(interior) = 2 * src(interior), as a launcher that writes the interior would; `fault` plants one bug."""
    s, d = src._box(src.buf), dst._box(dst.buf)
    d[1:-1, 1:-1, 1:-1] = 2.0 * s[1:-1, 1:-1, 1:-1]
    nx = src.nx
    if fault == "pad" and dst.ldy > nx + 2:
        dst.buf[dst.origin + dst.ldz + dst.ldy + nx + 2] = 1.0  # pitch padding of row 1, plane 1
    elif fault == "pad":
        dst.buf[dst.origin - 1] = 1.0  # no pitch padding in this layout: the word before the box
    elif fault == "ring":
        d[1, 1, 0] = 0.0  # x = 0
    elif fault == "skip":
        dst.i64[dst.origin + dst.nz * dst.ldz + dst.ny * dst.ldy + nx] = POISON_OUT  # the last interior point
    elif fault == "leak":
        # the clamped lane's load: the word after the last interior point's row pair, outside the box or in the ring
        d[-2, -2, -2] = 2.0 * src.buf[src.origin - 1]
    elif fault == "input":
        src.i64[src.origin + src.ldz * (src.nz + 2)] ^= 1  # ghost plane nz+2: one bit of its poison


def run_fake(dims, lid, fault):
    src, dst = make(dims, lid), make(dims, lid, out=True)
    a = rand_box(dims, 3)
    src.from_xyz(a).poison_outside_box().snapshot()
    dst.poison_all()
    fake_kernel(src, dst, fault)
    dst.assert_written_exactly(dst.interior_mask(), "fake")
    src.assert_unchanged(what="fake input")
    assert np.array_equal(dst.to_xyz()[1:-1, 1:-1, 1:-1], 2.0 * a[1:-1, 1:-1, 1:-1]), "values differ"


@extents
@cases
def test_correct_fake_passes(dims, lid):
    run_fake(dims, lid, None)


@extents
@cases
@pytest.mark.parametrize("fault,caught_by", [("pad", "outside the documented set was written"),
                                             ("ring", "outside the documented set was written"),
                                             ("skip", "of the documented set was not written"),
                                             ("leak", "values differ"), ("input", "fake input: word .* changed")])
def test_planted_fault_is_caught(dims, lid, fault, caught_by):
    with pytest.raises(AssertionError, match=caught_by):
        run_fake(dims, lid, fault)


def test_describe_names_the_region():
    f = make((5, 3, 4), "loose")
    assert "box" in f.describe(f.origin)
    assert "pitch padding" in f.describe(f.origin + 7)
    assert "plane gap" in f.describe(f.origin + f.ldy * 5)
    assert "ghost plane" in f.describe(f.origin - f.ldz)
    assert "guard margin" in f.describe(0)
