"""Child process of tests/test_gpu_fmg.py: full multigrid under the environment it was started with (the library
reads its switches once per process).   python tests/fmg_probe.py <out.npz> fmg|solve <n> <cycles>
fmg: HipSolver.fmg(grid, cycles) on an n^3 LINEAR grid -> level 0's v and the returned norm.
solve: HipSolver.solve with maxiter = cycles (GS_FMG in the environment decides the start) -> v and the history."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gpu-solve_amd"))
import gpusolve as gsv  # noqa: E402

out, what, n, cycles = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4])
p = gsv.GridParams(maxiter=cycles, tol=0.0, gridDim=(n, n, n), mode=gsv.GS_LINEAR)
with gsv.HipGridData(p) as g:
    hist = [gsv.HipSolver.fmg(g, cycles)] if what == "fmg" else gsv.HipSolver.solve(g)
    v = g.field(0, "v")
np.savez(out, v=v, hist=np.array(hist))
