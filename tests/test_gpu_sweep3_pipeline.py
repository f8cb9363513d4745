"""The fused triple's software pipeline (k_tb3y: sweep 1 runs one plane ahead of sweeps 2 and 3, four prologue steps
per z-chunk, one more sweep-1 plane carried across the step) against three gs_jacobi_sweep calls, bit for bit, where a
reordered pipeline can break: every depth from one plane to more than the pipeline holds, the seams between z-chunks,
three different weights in one call (a swapped stage weight shows in nothing else), the general stencil."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import gpusolve as gsv  # noqa: E402
from gpusolve.devfield import DevField  # noqa: E402

UNIT = gsv.Stencil().to_abi()
GENERAL = gsv.Stencil([4, -1, -1, -0.5, -0.5, -0.5, -0.5], list(gsv.CANONICAL_OFFSETS)).to_abi()
W3 = (0.5695, 1.0, 1.7319)


def k():
    assert torch.cuda.is_available()
    return gsv.kernels()


def st():
    return torch.cuda.current_stream().cuda_stream


def ok(rc):
    assert rc == 0, k().gs_strerror(rc).decode()


def fields(shape, seed):
    rng = np.random.default_rng(seed)
    nx, ny, nz = shape
    v, f = np.zeros((nx + 2, ny + 2, nz + 2)), np.zeros((nx + 2, ny + 2, nz + 2))
    v[1:-1, 1:-1, 1:-1] = rng.uniform(-1.0, 1.0, shape)
    f[1:-1, 1:-1, 1:-1] = rng.uniform(-100.0, 100.0, shape)
    return v, f


def both(S, shape, weights, gamma, seed):
    """(three gs_jacobi_sweep calls, one gs_jacobi_sweep3 / _w call) on the same random fields."""
    v0, f0 = fields(shape, seed)
    h = 1.0 / (shape[1] + 1)
    v, f, alt, out = (DevField(*shape) for _ in range(4))
    v.from_xyz(v0), f.from_xyz(f0)
    L = v.level(h)
    assert k().gs_jacobi_sweep3_supported(C.byref(S), C.byref(L)) >= 1
    if len(set(weights)) == 1:
        ok(k().gs_jacobi_sweep3(C.byref(S), C.byref(L), weights[0], gamma, v.ptr, out.ptr, f.ptr, st()))
    else:
        ok(k().gs_jacobi_sweep3_w(C.byref(S), C.byref(L), (C.c_double * 3)(*weights), gamma, v.ptr, out.ptr, f.ptr,
                                  st()))
    got = out.to_xyz()
    np.testing.assert_array_equal(v.to_xyz(), v0)
    for w in weights:
        ok(k().gs_jacobi_sweep(C.byref(S), C.byref(L), 0, w, gamma, v.ptr, alt.ptr, f.ptr, None, st()))
        v, alt = alt, v
    return v.to_xyz(), got


def chunks(S, shape):
    """z-chunks of the plan the triple launches with (the pair's: blocks = y-tiles of 4 rows x z-chunks)."""
    L = DevField(*shape).level(1.0 / (shape[1] + 1))
    blocks = gsv.diag().gs_debug_pair_blocks(C.byref(S), C.byref(L), 0)
    tiles = (shape[1] + 3) // 4
    assert blocks > 0 and blocks % tiles == 0
    return blocks // tiles


# (4, 5, nz): two y-tiles, the second ragged; (130, 3, nz): ragged rows in the third x-wave, the general-rows instance;
# (128, 4, nz): rows of whole waves, the instance without per-lane range selects
@pytest.mark.parametrize("nz", range(1, 10))
@pytest.mark.parametrize("nxy", [(4, 5), (130, 3), (128, 4)])
def test_every_pipeline_depth(nxy, nz):
    shape = nxy + (nz,)
    want, got = both(UNIT, shape, (0.8, 0.8, 0.8), 1.0, 100 * nxy[0] + nz)
    assert np.any(want[1:-1, 1:-1, 1:-1] != 0.0)
    np.testing.assert_array_equal(got, want)


# last chunks of 1, 2 and 3 planes; several y-tiles beside the seams in the last two
@pytest.mark.parametrize("shape", [(5, 4, 33), (130, 9, 14), (128, 8, 11)])
def test_chunk_seams(shape):
    assert chunks(UNIT, shape) >= 3
    want, got = both(UNIT, shape, (0.8, 0.8, 0.8), 1.0, sum(shape))
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("shape", [(130, 9, 14), (128, 4, 5), (4, 5, 2)])
def test_three_different_weights(shape):
    want, got = both(UNIT, shape, W3, 1.0, 7 + sum(shape))
    np.testing.assert_array_equal(got, want)
    # the weights matter at all: another order gives other words
    other, _ = both(UNIT, shape, W3[::-1], 1.0, 7 + sum(shape))
    assert np.any(other != want)


@pytest.mark.parametrize("weights", [(0.7, 0.7, 0.7), W3])
def test_general_stencil(weights):
    want, got = both(GENERAL, (129, 13, 9), weights, 0.5, 11)
    np.testing.assert_array_equal(got, want)
