"""The full-multigrid restatement (tests/fmg_ref.py: numpy's tricubic prolongation + the CPU oracle's operators),
which tests/test_gpu_fmg.py holds the GPU path against. No GPU needed.

- FMG(1) with the tricubic prolongation lands below three plain V-cycles from zero at 63^3, in LINEAR and
  NONLINEAR mode (DESIGN.md's FMG table: 2.76 < 8.87 and 0.234 < 2.64).
- The per-axis cubic is exact for cubics: every monomial x^a y^b z^c, a, b, c <= 3, sampled on a 7 -> 15 grid
  including its (non-zero) boundary values comes back to 1e-13."""
import itertools

import numpy as np
import pytest

import oracle as O
import fmg_ref as R

# the table of DESIGN.md's FMG section at 63^3 (CPU oracle, 2+2 smoothing, omega 0.8, gamma 1): FMG(1), 3 V-cycles
TABLE = {O.LINEAR: (2.76, 8.87), O.NONLINEAR: (0.234, 2.64)}


@pytest.mark.parametrize("mode", [O.LINEAR, O.NONLINEAR])
def test_fmg1_beats_three_cycles(mode):
    dims = (63, 63, 63)
    assert R.start_level(dims) == 5
    _, _, res = R.fmg(dims, mode=mode, cycles_per_level=1)
    plain = O.Grid(dims, mode=mode, maxiter=3).solve()
    print(f"mode {mode}: FMG(1) {res:.6g}, plain history {[float('%.6g' % h) for h in plain]}")
    assert res < plain[3]
    fmg_doc, plain_doc = TABLE[mode]
    assert abs(res - fmg_doc) <= 0.005 * fmg_doc  # the documented figures, to the three digits they are quoted to
    assert abs(plain[3] - plain_doc) <= 0.005 * plain_doc


def test_cubic_reproduces_cubics():
    nc = 7
    tc = np.arange(nc + 2) / (nc + 1.0)            # padded coarse points 0 .. 1
    tf = np.arange(2 * nc + 3) / (2.0 * (nc + 1))  # padded fine points: index 2i is coarse index i
    worst = 0.0
    for a, b, c in itertools.product(range(4), repeat=3):
        coarse = (1.0 + tc[:, None, None]) ** a * (0.5 - tc[None, :, None]) ** b * (2.0 * tc[None, None, :] - 0.3) ** c
        fine = (1.0 + tf[:, None, None]) ** a * (0.5 - tf[None, :, None]) ** b * (2.0 * tf[None, None, :] - 0.3) ** c
        assert np.abs(coarse[0]).max() > 0  # non-zero boundary values take part
        got = R.prolong(coarse)
        assert got.shape == fine.shape == (15 + 2,) * 3
        worst = max(worst, np.abs(got - fine).max() / max(1.0, np.abs(fine).max()))
    print("worst deviation over 64 monomials:", worst)
    assert worst <= 1e-13


def test_three_point_axis_and_start_levels():
    # an axis with one coarse interior point: the quadratic through its three padded values
    c = np.array([0.3, -1.2, 0.7]).reshape(3, 1, 1) * np.ones((1, 3, 3))
    got = R.cubic_axis(c, 0)[:, 0, 0]
    q = np.polyfit([0.0, 1.0, 2.0], [0.3, -1.2, 0.7], 2)
    np.testing.assert_allclose(got, np.polyval(q, np.arange(5) / 2.0), atol=1e-14)
    assert R.start_level((31, 31, 31)) == 4 and R.start_level((95, 95, 95)) == 5
    assert R.start_level((64, 64, 64)) == 0 and R.start_level((63, 31, 127)) == 4
