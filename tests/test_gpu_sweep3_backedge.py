"""The fused triple's staggered instance (k_tb3y<true, true, true, true>: rows of whole waves, scalar row bases) after its
load slots were given registers of their own across the z loop's back-edge (the plane state is moved out of a slot
before the slot is refilled) and f's two parity slots moved from LDS into registers: gs_jacobi_sweep3 against three
gs_jacobi_sweep calls, word for word, on the instance the launch record names. The z loop runs two plane steps per
iteration and a chunk of c planes takes c + 5 steps, so with the 4-plane chunks of small levels nz = 4..7, 9, 13 give
chunks of 4, 1, 2 and 3 planes: an odd and an even number of iterations, a last step that is the first and the second
of its iteration, and one to four chunks with their seams. ny = 3, 4, 9: one tile with a clipped mirrored wave, one
whole tile, three tiles with the last one clipped. nx = 128, 256: one and two x-waves of whole rows."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import gpusolve as gsv  # noqa: E402
from gpusolve.devfield import DevField  # noqa: E402
from layout_field import POISON_IN, POISON_OUT, LayoutField, layouts  # noqa: E402

UNIT = gsv.Stencil().to_abi()
STAGGERED = "k_tb3y<true, true, true, true>"
W1 = (0.8, 0.8, 0.8)
W3 = (0.5695, 1.0, 1.7319)


def k():
    assert torch.cuda.is_available()
    return gsv.kernels()


def st():
    return torch.cuda.current_stream().cuda_stream


def ok(rc):
    assert rc == 0, k().gs_strerror(rc).decode()


def record():
    """The launch record of this thread, cleared: the kernel names enqueued since the last call."""
    buf = C.create_string_buffer(1 << 12)
    n = k().gs_launch_record(buf, len(buf))
    names = buf.value.decode().splitlines()
    assert n == len(names), (n, names)
    return names


def random_fields(shape, seed):
    rng = np.random.default_rng(seed)
    nx, ny, nz = shape
    v, f = np.zeros((nx + 2, ny + 2, nz + 2)), np.zeros((nx + 2, ny + 2, nz + 2))
    v[1:-1, 1:-1, 1:-1] = rng.uniform(-1.0, 1.0, shape)
    f[1:-1, 1:-1, 1:-1] = rng.uniform(-100.0, 100.0, shape)
    return v, f


def three_sweeps(shape, weights, v0, f0):
    """Three gs_jacobi_sweep calls on fields of the default layout: the words the triple has to give."""
    v, f, a, b = (DevField(*shape) for _ in range(4))
    v.from_xyz(v0), f.from_xyz(f0)
    L = v.level(1.0 / (shape[1] + 1))
    src = v
    for w, dst in zip(weights, (a, b, a)):
        ok(k().gs_jacobi_sweep(C.byref(UNIT), C.byref(L), 0, w, 1.0, src.ptr, dst.ptr, f.ptr, None, st()))
        src = dst
    return src.to_xyz()


def triple(shape, weights, v0, f0):
    """One gs_jacobi_sweep3_w call on fields of the default layout; the staggered instance ran it."""
    v, f, out = (DevField(*shape) for _ in range(3))
    v.from_xyz(v0), f.from_xyz(f0)
    L = v.level(1.0 / (shape[1] + 1))
    assert k().gs_jacobi_sweep3_supported(C.byref(UNIT), C.byref(L)) >= 1
    record()
    ok(k().gs_jacobi_sweep3_w(C.byref(UNIT), C.byref(L), (C.c_double * 3)(*weights), 1.0, v.ptr, out.ptr, f.ptr, st()))
    assert record() == [STAGGERED]
    got = out.to_xyz()
    np.testing.assert_array_equal(v.to_xyz(), v0)
    return got


@pytest.mark.parametrize("nz", [4, 5, 6, 7, 9, 13])
@pytest.mark.parametrize("ny", [3, 4, 9])
@pytest.mark.parametrize("nx", [128, 256])
def test_shapes(nx, ny, nz):
    shape = (nx, ny, nz)
    v0, f0 = random_fields(shape, 1000 * nx + 20 * ny + nz)
    want = three_sweeps(shape, W1, v0, f0)
    assert np.any(want[1:-1, 1:-1, 1:-1] != v0[1:-1, 1:-1, 1:-1])
    np.testing.assert_array_equal(triple(shape, W1, v0, f0), want)


def test_chunks_of_the_shapes():
    """The plan behind the shapes above: 4-plane chunks, so nz = 4, 5, 9, 13 are 1, 2, 3 and 4 chunks."""
    for nz, n in ((4, 1), (5, 2), (7, 2), (9, 3), (13, 4)):
        L = DevField(128, 9, nz).level(0.1)
        blocks = gsv.diag().gs_debug_pair_blocks(C.byref(UNIT), C.byref(L), 0)
        assert blocks == 3 * n, (nz, blocks)


def test_three_different_weights():
    shape = (256, 9, 13)
    v0, f0 = random_fields(shape, 77)
    want = three_sweeps(shape, W3, v0, f0)
    np.testing.assert_array_equal(triple(shape, W3, v0, f0), want)
    back = three_sweeps(shape, W3[::-1], v0, f0)
    np.testing.assert_array_equal(triple(shape, W3[::-1], v0, f0), back)
    assert np.any(back != want)  # the order of the weights matters at all


def test_padded_pitch_poisoned_padding():
    """Rows six words longer than the default pitch and a gap between the planes, x = 1 at byte 64 of a 128-byte line,
    every word outside the inputs' boxes a NaN: the result is the default layout's, and only the interior is written."""
    shape = (256, 9, 13)
    lay = layouts(*shape)["loose"]
    v0, f0 = random_fields(shape, 78)
    want = three_sweeps(shape, W3, v0, f0)
    v, f, out = (LayoutField(*shape, lay.ldy, lay.ldz, ph) for ph in (lay.phase_in, lay.phase_out, lay.phase_out))
    for fld, a in ((v, v0), (f, f0)):
        fld.poison_all(POISON_IN).from_xyz(a)
        fld.snapshot()
    out.poison_all(POISON_OUT)
    L = v.level(1.0 / (shape[1] + 1))
    record()
    ok(k().gs_jacobi_sweep3_w(C.byref(UNIT), C.byref(L), (C.c_double * 3)(*W3), 1.0, v.ptr, out.ptr, f.ptr, st()))
    assert record() == [STAGGERED]
    out.assert_written_exactly(out.interior_mask(), "the triple's output")
    v.assert_unchanged(what="v"), f.assert_unchanged(what="f")
    np.testing.assert_array_equal(out.to_xyz()[1:-1, 1:-1, 1:-1], want[1:-1, 1:-1, 1:-1])


def test_division_range_in_some_lanes_only():
    """The stencil sums are divided by h^2 in batches behind ONE range test per batch (exponent field 124..1623: the
    three-operation quotient; else the IEEE division for the whole batch). A few points whose sums are exactly zero,
    far below and far above that range, in a few lanes of a few rows and planes: the lanes of one wave take different
    paths, and both are the one-sweep kernels' words."""
    shape = (256, 9, 13)
    v0, f0 = random_fields(shape, 79)
    v0[40:43, 2:5, 3:6] = 0.0           # the centre's sum is 0 in sweep 1 (exponent field 0)
    v0[130:133, 6:9, 8:11] *= 1e-290    # sums below 2^-899
    v0[200, 5, 6] = 1e200               # sums above 2^601 at the point and its six neighbours, two more rings later
    v0[129, 4, 12] = -3e190             # the same across an x-wave boundary and into the last plane
    want = three_sweeps(shape, W3, v0, f0)
    assert np.all(np.isfinite(want))
    np.testing.assert_array_equal(triple(shape, W3, v0, f0), want)
