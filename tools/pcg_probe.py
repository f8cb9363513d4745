"""A few launches of gs_pcg_dir, gs_pcg_step and gs_dot beside the k_rb Jacobi sweep on seeded noise, for a counter
pass (tools/pmc_run.sh pcg tools/pcg_probe.py [n] [launches]): nothing is timed or checked here.

    python tools/pcg_probe.py [n=512] [launches=3]"""
import ctypes as C
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "gpu-solve_amd"))
sys.path.insert(0, HERE)

import torch  # noqa: E402

import gpusolve as gsv  # noqa: E402
from gpusolve.devfield import DevField  # noqa: E402
from pcg_timing import noise  # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    launches = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    kr, k = gsv.krylov(), gsv.kernels()
    z, p_in, x, r, f = (noise(DevField(n, n, n), s) for s in range(5))
    p_out, q = DevField(n, n, n), DevField(n, n, n)
    L, S = z.level(1.0 / (n + 1)), gsv.Stencil().to_abi()
    nparts = max(kr.gs_pcg_dir_num_partials(C.byref(S), C.byref(L)), kr.gs_pcg_step_num_partials(C.byref(L)), 1)
    parts = torch.zeros(nparts, dtype=torch.float64, device="cuda")
    scal = torch.tensor([1e-3, -0.25], dtype=torch.float64, device="cuda")  # alpha, beta
    s = torch.cuda.current_stream().cuda_stream
    for _ in range(launches):
        rcs = (kr.gs_pcg_dir(C.byref(S), C.byref(L), z.ptr, p_in.ptr, p_out.ptr, q.ptr, scal.data_ptr() + 8,
                             parts.data_ptr(), s),
               kr.gs_pcg_step(C.byref(L), x.ptr, r.ptr, p_out.ptr, q.ptr, scal.data_ptr(), parts.data_ptr(), s),
               kr.gs_dot(C.byref(L), r.ptr, z.ptr, parts.data_ptr(), s),
               k.gs_jacobi_sweep(C.byref(S), C.byref(L), 0, 0.8, 1.0, z.ptr, p_out.ptr, f.ptr, None, s))
        assert rcs == (0, 0, 0, 0), rcs
        torch.cuda.synchronize()
    print("ok", n, launches)


if __name__ == "__main__":
    main()
