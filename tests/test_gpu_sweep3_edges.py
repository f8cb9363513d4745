"""What the fused triple's (k_tb3y) instruction cut touches: the x-edge values that cross an x-wave boundary through LDS
straight into the DPP shift.

Edge transport: gs_jacobi_sweep3 against three gs_jacobi_sweep calls, bit for bit on the uint64 view (NaNs by their
bits), with special values planted in the columns on both sides of every x-wave boundary (128|129, 256|257, 384|385)
and in columns 1 and nx, in every row and every plane, so all three stages carry them across the boundary."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import gpusolve as gsv  # noqa: E402
from gpusolve.devfield import DevField  # noqa: E402

UNIT = gsv.Stencil().to_abi()
GENERAL = gsv.Stencil([4, -1, -1, -0.5, -0.5, -0.5, -0.5], list(gsv.CANONICAL_OFFSETS)).to_abi()  # UN = false


def st():
    return torch.cuda.current_stream().cuda_stream


def ok(rc):
    assert rc == 0, gsv.kernels().gs_strerror(rc).decode()


def from_bits(sign, expo, mant):
    """doubles from sign (0 / 1), biased exponent 0..2047 and 52-bit mantissa arrays"""
    b = (np.asarray(sign, np.uint64) << np.uint64(63)) | (np.asarray(expo, np.uint64) << np.uint64(52)) | \
        np.asarray(mant, np.uint64)
    return b.view(np.float64)


def planted_values():
    """-0.0, a denormal, +-inf, a NaN with a payload of its own, and the powers of two around both ends of the fast
    division's operand range (biased exponents 120..128 and 1619..1627; the range is 124..1623)"""
    special = np.array([0x8000000000000000, 0x0000000000012345, 0x7FF0000000000000, 0xFFF0000000000000,
                        0x7FF8000000ABCDEF], dtype=np.uint64).view(np.float64)
    expo = np.concatenate([np.arange(120, 129), np.arange(1619, 1628)])
    return np.concatenate([special, from_bits(np.zeros_like(expo), expo, np.zeros_like(expo))])


def planted_field(rng, nx, ny, nz):
    a = np.zeros((nx + 2, ny + 2, nz + 2))
    a[1:nx + 1, 1:ny + 1, 1:nz + 1] = rng.uniform(-1.0, 1.0, (nx, ny, nz))
    vals = planted_values()
    cols = sorted({1, nx} | {c for b in (128, 256, 384) for c in (b, b + 1) if c <= nx})
    # every value in turn over the boundary columns of every row and plane
    n = 0
    for z in range(1, nz + 1):
        for y in range(1, ny + 1):
            for c in cols:
                a[c, y, z] = vals[n % vals.size]
                n += 1
    assert n >= vals.size and nz >= 3
    return a


def three_sweeps(S, v0, f0, h, omega, gamma):
    nx, ny, nz = (s - 2 for s in v0.shape)
    v, f, alt = DevField(nx, ny, nz).from_xyz(v0), DevField(nx, ny, nz).from_xyz(f0), DevField(nx, ny, nz)
    L = v.level(h)
    for _ in range(3):
        ok(gsv.kernels().gs_jacobi_sweep(C.byref(S), C.byref(L), 0, omega, gamma, v.ptr, alt.ptr, f.ptr, None, st()))
        v, alt = alt, v
    return v.to_xyz()


def triple(S, v0, f0, h, omega, gamma):
    nx, ny, nz = (s - 2 for s in v0.shape)
    v, f, out = DevField(nx, ny, nz).from_xyz(v0), DevField(nx, ny, nz).from_xyz(f0), DevField(nx, ny, nz)
    L = v.level(h)
    assert gsv.kernels().gs_jacobi_sweep3_supported(C.byref(S), C.byref(L)) >= 1
    ok(gsv.kernels().gs_jacobi_sweep3(C.byref(S), C.byref(L), omega, gamma, v.ptr, out.ptr, f.ptr, st()))
    return out.to_xyz()


# (129, 3, 5): two x-waves, the second with one column; (256, 6, 7): two whole-wave x-waves (FX), a ragged mirrored
# y-tile; (385, 5, 6): four x-waves, the last with one column; (512, 5, 6): four whole-wave x-waves (FX)
CASES = [((129, 3, 5), "unit"), ((256, 6, 7), "unit"), ((385, 5, 6), "unit"), ((512, 5, 6), "unit"),
         ((385, 5, 6), "general")]


IDS = [f"{s[0]}x{s[1]}x{s[2]}-{n}" for s, n in CASES]


@pytest.mark.parametrize("shape,stencil", CASES, ids=IDS)
def test_edge_transport_bitwise(shape, stencil):
    """gs_jacobi_sweep3 against three gs_jacobi_sweep calls, the whole arrays word for word on the uint64 view: signed
    zeros, denormals, infinities, both ends of the division's range, and the NaNs by their sign and payload."""
    assert torch.cuda.is_available()
    rng = np.random.default_rng(shape[0] * 31 + shape[1])
    S, omega, gamma = (UNIT, 0.8, 1.0) if stencil == "unit" else (GENERAL, 0.7, 0.5)
    h = 1.0 / (shape[1] + 1)
    v0 = planted_field(rng, *shape)
    f0 = np.zeros_like(v0)
    f0[1:-1, 1:-1, 1:-1] = rng.uniform(-100.0, 100.0, shape)
    want = three_sweeps(S, v0, f0, h, omega, gamma).view(np.uint64)
    got = triple(S, v0, f0, h, omega, gamma).view(np.uint64)
    wf = want.view(np.float64)
    assert np.isnan(wf).any() and np.isinf(wf).any() and np.isfinite(wf[1:-1, 1:-1, 1:-1]).any()  # the values spread
    bad = np.argwhere(got != want)
    assert bad.shape[0] == 0, [(tuple(i), hex(got[tuple(i)]), hex(want[tuple(i)])) for i in bad[:6]]


# ---- NaN bits of the one-sweep kernels ---------------------------------------------------------------------------
# The comparison above takes the one-sweep kernel as its reference, and gs_jacobi_sweep runs two of them: the
# one-point kernel (k_generic) on small levels, the register-blocked march (k_rb) on large ones. With a unit stencil
# both form the sum as s - x (as the pairs and triples do), which negates a NaN neighbour's sign once, and the
# residual f - A(v) negates it back: after one sweep the six neighbours of a planted NaN hold the planted word itself,
# and so does the point. (Before, k_generic summed s + (-1) * x, which keeps the sign: its neighbours came out with
# the sign flipped, and small levels disagreed with large levels, pairs and triples on those bits alone.)

NAN_WORDS = [0x7FF8000000ABCDEF, 0xFFF8000000012345]
# (40, 9, 7): k_generic; (256, 64, 256): 16 tiles x 64 four-plane chunks, the smallest that takes k_rb
NAN_SHAPES = [(40, 9, 7), (256, 64, 256)]


@pytest.mark.parametrize("shape", NAN_SHAPES, ids=["one-point", "march"])
@pytest.mark.parametrize("word", NAN_WORDS, ids=["+nan", "-nan"])
def test_unit_stencil_nan_bits_are_the_same_in_every_sweep_kernel(shape, word):
    assert torch.cuda.is_available()
    nx, ny, nz = shape
    rng = np.random.default_rng(nx)
    v0 = np.zeros((nx + 2, ny + 2, nz + 2))
    v0[1:-1, 1:-1, 1:-1] = rng.uniform(-1.0, 1.0, shape)
    f0 = np.zeros_like(v0)
    f0[1:-1, 1:-1, 1:-1] = rng.uniform(-100.0, 100.0, shape)
    x, y, z = nx // 2, ny // 2, nz // 2
    v0[x, y, z] = np.array([word], dtype=np.uint64).view(np.float64)[0]
    v, f, one, two = (DevField(*shape) for _ in range(4))
    v.from_xyz(v0)
    f.from_xyz(f0)
    L = v.level(1.0 / (ny + 1))
    ok(gsv.kernels().gs_jacobi_sweep(C.byref(UNIT), C.byref(L), 0, 0.8, 1.0, v.ptr, one.ptr, f.ptr, None, st()))
    ok(gsv.kernels().gs_jacobi_sweep(C.byref(UNIT), C.byref(L), 0, 0.8, 1.0, one.ptr, two.ptr, f.ptr, None, st()))
    r1, r2 = one.to_xyz().view(np.uint64), two.to_xyz().view(np.uint64)
    star = [(x, y, z), (x + 1, y, z), (x - 1, y, z), (x, y + 1, z), (x, y - 1, z), (x, y, z + 1), (x, y, z - 1)]
    assert int(np.isnan(r1.view(np.float64)).sum()) == 7
    assert [hex(r1[p]) for p in star] == [hex(word)] * 7
    nan2 = np.isnan(r2.view(np.float64))
    assert int(nan2.sum()) == 25 and np.all(r2[nan2] == np.uint64(word))
    # the fused pair, where the level takes one, leaves the same words as the two sweeps
    if gsv.kernels().gs_jacobi_sweep2_supported(C.byref(UNIT), C.byref(L)) >= 1:
        pair = DevField(*shape)
        ok(gsv.kernels().gs_jacobi_sweep2(C.byref(UNIT), C.byref(L), 0, 0.8, 1.0, v.ptr, pair.ptr, f.ptr, None, 0, 0,
                                          st()))
        assert np.array_equal(pair.to_xyz().view(np.uint64), r2)
