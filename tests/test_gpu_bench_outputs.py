"""bench.py --dump-outputs and the plain / --full split. The dump is what the timed sweeps computed from the
grid's initial iterate (v = 0), whatever ran before them: reset_iterate after earlier sweeps must leave exactly
the state of a fresh grid, dump_outputs must write the owned points (or its documented seeded sample), and a
plain run of the benchmark itself must time `--steps` sweeps, report ms_per_step, leave every other leg null
and write the same array as `steps` sweeps of a fresh grid."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import gpusolve as gsv  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def params(dims):
    return gsv.GridParams(maxiter=1, tol=0.0, gridDim=dims, mode=gsv.GS_LINEAR, preSmoothing=2, postSmoothing=2)


def fresh_sweeps(dims, k):
    """Level 0's padded iterate [x][y][z] after k sweeps of a fresh grid."""
    with gsv.HipGridData(params(dims)) as g:
        gsv.HipSolver.jacobi(g, 0, k)
        g.sync()
        return g.field(0, "v")


# 64^3: the fused pair's level; 33x31x29: odd sizes, rows shorter than their pitch
@pytest.mark.parametrize("dims", [(64, 64, 64), (33, 31, 29)])
@pytest.mark.parametrize("before", [0, 5, 8])  # odd and even: the iterate in either of the level's two buffers
def test_reset_iterate_restores_the_initial_state(dims, before):
    import bench
    want = fresh_sweeps(dims, 3)
    with gsv.HipGridData(params(dims)) as g:
        if before:
            gsv.HipSolver.jacobi(g, 0, before)
            g.sync()
            assert np.any(g.field(0, "v") != 0.0)
        bench.reset_iterate(g)
        torch.cuda.synchronize()
        assert not np.any(g.field(0, "v"))
        gsv.HipSolver.jacobi(g, 0, 3)
        g.sync()
        np.testing.assert_array_equal(g.field(0, "v"), want)


def test_dump_outputs_whole_block_and_seeded_sample(tmp_path, monkeypatch):
    import bench
    dims = (33, 31, 29)
    with gsv.HipGridData(params(dims)) as g:
        gsv.HipSolver.jacobi(g, 0, 3)
        g.sync()
        own = g.field(0, "v")[1:-1, 1:-1, 1:-1]  # [x][y][z]
        info = bench.dump_outputs(g, str(tmp_path / "whole"), 0, 1)
        got = np.load(tmp_path / "whole" / "v.npy")
        assert got.dtype == np.float64 and got.shape == (29, 31, 33) and info["sample"] is None
        np.testing.assert_array_equal(got, own.transpose(2, 1, 0))
        monkeypatch.setattr(bench, "DUMP_MAX_POINTS", 1000)
        bench.dump_outputs(g, str(tmp_path / "sample"), 0, 1)
        got = np.load(tmp_path / "sample" / "v.npy")
        idx = np.random.default_rng(bench.DUMP_SEED).integers(0, own.size, size=1000)
        assert got.dtype == np.float64 and got.shape == (1000,)
        np.testing.assert_array_equal(got, own.transpose(2, 1, 0).reshape(-1)[idx])
        assert np.count_nonzero(got) > 0


def test_plain_run_times_the_steps_and_dumps_them(tmp_path):
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "4",
                        "--ramp-ms", "20", "--size", "64", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["full"] is False
    assert line["ms_per_step"] > 0 and line["value"] > 0
    assert line["value"] == pytest.approx(64 ** 3 / line["ms_per_step"] / 1e3, rel=2e-2)  # (both figures are rounded)
    for leg in ("single_sweep_kernel", "measured_ceilings", "vcycle", "newton", "config2", "config5_single_gpu",
                "cpu_baseline"):
        assert line[leg] is None, leg
    assert line["warmup_sweeps_total"] > 4  # the ramp ran: the dump must not depend on its length
    got = np.load(out / "v.npy")
    assert sorted(os.listdir(out)) == ["v.npy"] and got.dtype == np.float64
    np.testing.assert_array_equal(got, fresh_sweeps((64, 64, 64), 3)[1:-1, 1:-1, 1:-1].transpose(2, 1, 0))
