"""Minimal launcher for profiling the fused triple: level-0 LINEAR sweeps of bench.py's grid through gs_grid_jacobi
(at 512^3: k_tb3y triples, then the pairs that finish the count), nothing else on the GPU.

    rocprofv3 --kernel-trace --stats -d <dir> -o run --output-format csv -- python tools/prof_triples.py
    tools/pmc_run.sh <tag> tools/prof_triples.py --sweeps 12          (counters: a run of their own)
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gpu-solve_amd"))
import gpusolve as gsv  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--sweeps", type=int, default=99, help="sweeps per gs_grid_jacobi call (99: 33 triples)")
    ap.add_argument("--calls", type=int, default=1)
    a = ap.parse_args()
    n = a.size
    p = gsv.GridParams(maxiter=1, tol=0.0, gridDim=(n, n, n), mode=gsv.GS_LINEAR, preSmoothing=2, postSmoothing=2)
    with gsv.HipGridData(p) as g:
        for _ in range(a.calls):
            gsv.HipSolver.jacobi(g, 0, a.sweeps)
        g.sync()
        print("triples launched on level 0:", gsv.driver().gs_grid_level_triples(g.handle, 0), gsv.build_info()[:20])


if __name__ == "__main__":
    main()
