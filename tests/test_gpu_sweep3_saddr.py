"""The fused triple's addressing (k_tb3y: wave-uniform row bases on the scalar unit plus one 32-bit lane offset; with
GS_T3_SADDR=0 per-lane 64-bit addresses) against three gs_jacobi_sweep calls, bit for bit, where an address can go
wrong: the three instances at the smallest shapes with every address form (clamped lanes, clamped rows, predicated
stores, a chunk shorter than the prologue), the seams between z-chunks, both store forms in one row, no word written
outside the owned points, the same words from call to call, and both address paths (a child process each)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import gpusolve as gsv  # noqa: E402
from gpusolve.devfield import DevField  # noqa: E402
from sweep3_saddr_probe import CASES, SEAMS, STENCILS, Problem, case_id  # noqa: E402

PROBE = os.path.join(REPO, "tests", "sweep3_saddr_probe.py")
_ref = {}


def reference(case):
    """The three-sweep result of a case, computed once and shared (read-only)."""
    if case not in _ref:
        assert torch.cuda.is_available()
        _ref[case] = Problem(case).reference()
        _ref[case].setflags(write=False)
    return _ref[case]


def chunks(S, shape):
    """z-chunks of the plan the triple launches with (the pair's: blocks = y-tiles of 4 rows x z-chunks)."""
    L = DevField(*shape).level(1.0 / (shape[1] + 1))
    blocks = gsv.diag().gs_debug_pair_blocks(C.byref(S), C.byref(L), 0)
    tiles = (shape[1] + 3) // 4
    assert blocks > 0 and blocks % tiles == 0
    return blocks // tiles


def check(case, got):
    """Owned points: the reference's words, all finite. Everything else of the output field: the NaN it started as."""
    want = reference(case)
    inner = (slice(1, -1),) * 3
    assert np.any(want[inner] != 0.0)
    np.testing.assert_array_equal(got[inner], want[inner])
    assert np.all(np.isfinite(got[inner]))
    ghost = np.ones(got.shape, dtype=bool)
    ghost[inner] = False
    assert np.all(np.isnan(got[ghost]))


# (128, 4, 5): rows of whole waves, one y-tile; (130, 9, 14): general rows, clamped lanes in the third x-wave, a ragged
# last y-tile (clamped rows, predicated stores); (4, 5, 2): one lane pair, a chunk shorter than the prologue;
# (129, 13, 9): the general stencil, equal and different weights; (5, 4, 33), (128, 8, 11): chunk seams;
# (129, 5, 6), (127, 5, 6): the last lane's one-point store and the two-point store in one row
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_triple_equals_three_sweeps(case):
    p = Problem(case)
    got = p.triple()
    check(case, got)
    nx, ny, nz = case[1]
    assert p.written == nx * ny * nz  # no stray word anywhere in the allocation, pitch padding included


@pytest.mark.parametrize("shape", SEAMS)
def test_chunk_seams_repeat_word_for_word(shape):
    case = ("unit", shape, (0.8, 0.8, 0.8), 1.0)
    assert case in CASES and chunks(STENCILS["unit"], shape) >= 3
    p = Problem(case)
    first = p.triple()
    check(case, first)
    inner = (slice(1, -1),) * 3
    words = np.ascontiguousarray(first[inner]).view(np.uint64)
    for i in range(1, 20):
        again = np.ascontiguousarray(p.triple()[inner]).view(np.uint64)
        np.testing.assert_array_equal(again, words, err_msg="call %d" % i)


@pytest.mark.parametrize("saddr", ["0", "1"])
def test_both_address_paths(tmp_path, saddr):
    out = str(tmp_path / ("saddr%s.npz" % saddr))
    env = dict(os.environ, GS_T3_SADDR=saddr)
    r = subprocess.run([sys.executable, PROBE, out], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    with np.load(out) as d:
        for i, case in enumerate(CASES):
            check(case, d["got%d" % i])
            # the one-sweep kernels do not read the switch: the child's reference is this process's
            np.testing.assert_array_equal(d["want%d" % i], reference(case))
