"""The fused triple's staggered step (k_tb3y on rows of whole waves: the mirrored y-waves, waves 4-7 of the 8-wave block,
run half a step behind the others; sweep 1 first, one plane later, then their loads, then sweeps 2 and 3) against three
gs_jacobi_sweep calls, bit for bit, where two halves out of phase can break: every y-situation of the two halves at every
depth around the pipeline's, the seams between z-chunks, a field that names its plane and row (a v row exchanged from the
wrong plane or the wrong half changes words), three different weights, repeated calls (the reordered LDS traffic must not
depend on timing), the general stencil. nx = 512 is the 8-wave block of the staggered instance, nx = 500 the same block of
the general-rows instance."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import gpusolve as gsv  # noqa: E402
from gpusolve.devfield import DevField  # noqa: E402

UNIT = gsv.Stencil().to_abi()
GENERAL = gsv.Stencil([4, -1, -1, -0.5, -0.5, -0.5, -0.5], list(gsv.CANONICAL_OFFSETS)).to_abi()
W1 = (0.8, 0.8, 0.8)
W3 = (0.5695, 1.0, 1.7319)


def k():
    assert torch.cuda.is_available()
    return gsv.kernels()


def st():
    return torch.cuda.current_stream().cuda_stream


def ok(rc):
    assert rc == 0, k().gs_strerror(rc).decode()


def random_fields(shape, seed):
    rng = np.random.default_rng(seed)
    nx, ny, nz = shape
    v, f = np.zeros((nx + 2, ny + 2, nz + 2)), np.zeros((nx + 2, ny + 2, nz + 2))
    v[1:-1, 1:-1, 1:-1] = rng.uniform(-1.0, 1.0, shape)
    f[1:-1, 1:-1, 1:-1] = rng.uniform(-100.0, 100.0, shape)
    return v, f


def named_fields(shape):
    """v = 1000 z + y + x / 1024 on the interior (every row of every plane its own words), f = 0."""
    nx, ny, nz = shape
    x, y, z = np.meshgrid(np.arange(nx + 2.0), np.arange(ny + 2.0), np.arange(nz + 2.0), indexing="ij")
    v = np.zeros((nx + 2, ny + 2, nz + 2))
    v[1:-1, 1:-1, 1:-1] = (1000.0 * z + y + x / 1024.0)[1:-1, 1:-1, 1:-1]
    return v, np.zeros_like(v)


class Case:
    """The fields of one shape on the GPU and the reference of three gs_jacobi_sweep calls, computed once."""

    def __init__(self, S, shape, weights, gamma, v0, f0):
        self.S, self.shape, self.weights, self.gamma, self.v0 = S, shape, weights, gamma, v0
        self.v, self.f, a, b = (DevField(*shape) for _ in range(4))
        self.v.from_xyz(v0), self.f.from_xyz(f0)
        self.L = self.v.level(1.0 / (shape[1] + 1))
        assert k().gs_jacobi_sweep3_supported(C.byref(S), C.byref(self.L)) >= 1
        src = self.v
        for w, dst in zip(weights, (a, b, a)):
            ok(k().gs_jacobi_sweep(C.byref(S), C.byref(self.L), 0, w, gamma, src.ptr, dst.ptr, self.f.ptr, None, st()))
            src = dst
        self.want = src.to_xyz()

    def triple(self):
        """One gs_jacobi_sweep3_w call into a fresh output field."""
        out = DevField(*self.shape)
        ok(k().gs_jacobi_sweep3_w(C.byref(self.S), C.byref(self.L), (C.c_double * 3)(*self.weights), self.gamma,
                                  self.v.ptr, out.ptr, self.f.ptr, st()))
        got = out.to_xyz()
        np.testing.assert_array_equal(self.v.to_xyz(), self.v0)
        return got


def case(S, shape, weights=W1, gamma=1.0, seed=None):
    v0, f0 = random_fields(shape, sum(shape) if seed is None else seed)
    return Case(S, shape, weights, gamma, v0, f0)


def chunks(S, shape):
    """z-chunks of the plan the triple launches with (the pair's: blocks = y-tiles of 4 rows x z-chunks)."""
    L = DevField(*shape).level(1.0 / (shape[1] + 1))
    blocks = gsv.diag().gs_debug_pair_blocks(C.byref(S), C.byref(L), 0)
    tiles = (shape[1] + 3) // 4
    assert blocks > 0 and blocks % tiles == 0
    return blocks // tiles


# ny = 1..8 puts the mirrored (lagging) wave of the last tile wholly outside the grid (ny = 1, 2, 5, 6), half outside
# (3, 7) and wholly inside (4, 8), with one tile and with two; nz = 1..3 is shorter than the pipeline, 4 its length,
# 7 longer. nx = 512: four whole x-waves, the staggered instance; nx = 500: the same block, the general-rows instance
@pytest.mark.parametrize("nz", [1, 2, 3, 4, 7])
@pytest.mark.parametrize("ny", range(1, 9))
@pytest.mark.parametrize("nx", [512, 500])
def test_eight_wave_block(nx, ny, nz):
    c = case(UNIT, (nx, ny, nz), seed=1000 * nx + 10 * ny + nz)
    assert np.any(c.want[1:-1, 1:-1, 1:-1] != 0.0)
    np.testing.assert_array_equal(c.triple(), c.want)


@pytest.mark.parametrize("shape", [(512, 8, 11), (512, 5, 14)])
def test_chunk_seams(shape):
    assert chunks(UNIT, shape) >= 3
    c = case(UNIT, shape)
    np.testing.assert_array_equal(c.triple(), c.want)


@pytest.mark.parametrize("named", [True, False])
def test_field_names_its_plane_and_row(named):
    shape = (512, 8, 9)
    v0, f0 = named_fields(shape) if named else random_fields(shape, 529)
    c = Case(UNIT, shape, W3, 1.0, v0, f0)
    np.testing.assert_array_equal(c.triple(), c.want)


@pytest.mark.parametrize("shape", [(512, 4, 5), (512, 7, 13)])
def test_three_different_weights(shape):
    c = case(UNIT, shape, W3)
    np.testing.assert_array_equal(c.triple(), c.want)
    r = case(UNIT, shape, W3[::-1])
    np.testing.assert_array_equal(r.triple(), r.want)
    # the weights matter at all: the reversed order gives other words
    assert np.any(r.want != c.want)


@pytest.mark.parametrize("shape", [(512, 7, 13), (512, 8, 5)])
def test_repeatable(shape):
    c = case(UNIT, shape, W3)
    first = c.triple()
    np.testing.assert_array_equal(first, c.want)
    for _ in range(19):
        np.testing.assert_array_equal(c.triple(), first)


@pytest.mark.parametrize("weights", [(0.7, 0.7, 0.7), W3])
def test_general_stencil(weights):
    c = case(GENERAL, (129, 13, 9), weights, 0.5, seed=11)
    np.testing.assert_array_equal(c.triple(), c.want)
