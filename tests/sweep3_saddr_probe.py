"""Helpers of tests/test_gpu_sweep3_saddr.py, and its child process: every case of CASES under the environment the
process was started with (the library reads GS_T3_SADDR once, when it is loaded), the three-sweep reference and the
triple's output of each case saved to an .npz.   python tests/sweep3_saddr_probe.py <out.npz>"""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gpu-solve_amd"))
import gpusolve as gsv  # noqa: E402
from gpusolve.devfield import DevField  # noqa: E402

STENCILS = {
    "unit": gsv.Stencil().to_abi(),
    "general": gsv.Stencil([4, -1, -1, -0.5, -0.5, -0.5, -0.5], list(gsv.CANONICAL_OFFSETS)).to_abi(),
}
W3 = (0.5695, 1.0, 1.7319)
SEAMS = [(5, 4, 33), (130, 9, 14), (128, 8, 11)]
# (stencil, shape, weights, gamma): the three instances at the smallest shapes with every address form, the chunk
# seams, and both store forms (one point / two points) in one row
CASES = ([("unit", s, (0.8, 0.8, 0.8), 1.0) for s in [(128, 4, 5), (130, 9, 14), (4, 5, 2)]] +
         [("general", (129, 13, 9), w, 0.5) for w in [(0.7, 0.7, 0.7), W3]] +
         [("unit", s, (0.8, 0.8, 0.8), 1.0) for s in SEAMS if s != (130, 9, 14)] +
         [("unit", (nx, 5, 6), W3, 1.0) for nx in (129, 127)])


def case_id(case):
    name, shape, weights, _ = case
    return "%s-%dx%dx%d-%s" % (name, *shape, "w3" if len(set(weights)) > 1 else "w1")


def seed_of(case):
    return 1000 * len(case[0]) + sum(case[1]) + (7 if len(set(case[2])) > 1 else 0)


def st():
    import torch

    return torch.cuda.current_stream().cuda_stream


def ok(rc):
    assert rc == 0, gsv.kernels().gs_strerror(rc).decode()


def fields(shape, seed):
    rng = np.random.default_rng(seed)
    nx, ny, nz = shape
    v, f = np.zeros((nx + 2, ny + 2, nz + 2)), np.zeros((nx + 2, ny + 2, nz + 2))
    v[1:-1, 1:-1, 1:-1] = rng.uniform(-1.0, 1.0, shape)
    f[1:-1, 1:-1, 1:-1] = rng.uniform(-100.0, 100.0, shape)
    return v, f


class Problem:
    """Random fields of one case on the device; the output field starts as NaN everywhere, ghost layer included."""

    def __init__(self, case):
        name, self.shape, self.weights, self.gamma = case
        self.S = STENCILS[name]
        self.v0, f0 = fields(self.shape, seed_of(case))
        self.v, self.f = DevField(*self.shape).from_xyz(self.v0), DevField(*self.shape).from_xyz(f0)
        self.L = self.v.level(1.0 / (self.shape[1] + 1))
        assert gsv.kernels().gs_jacobi_sweep3_supported(C.byref(self.S), C.byref(self.L)) >= 1

    def triple(self):
        """One gs_jacobi_sweep3 / _w call into a NaN field; the whole field, ghost layer included."""
        k, w = gsv.kernels(), self.weights
        out = DevField(*self.shape, fill=float("nan"))
        if len(set(w)) == 1:
            ok(k.gs_jacobi_sweep3(C.byref(self.S), C.byref(self.L), w[0], self.gamma, self.v.ptr, out.ptr, self.f.ptr,
                                  st()))
        else:
            ok(k.gs_jacobi_sweep3_w(C.byref(self.S), C.byref(self.L), (C.c_double * 3)(*w), self.gamma, self.v.ptr,
                                    out.ptr, self.f.ptr, st()))
        got = out.to_xyz()
        np.testing.assert_array_equal(self.v.to_xyz(), self.v0)
        # words of the whole allocation (pitch padding and second ghost planes too) that are no longer NaN
        self.written = int((~out.buf.isnan()).sum())
        return got

    def reference(self):
        """Three gs_jacobi_sweep calls (the input iterate is left as it was)."""
        k = gsv.kernels()
        a, b = DevField(*self.shape).from_xyz(self.v0), DevField(*self.shape)
        for w in self.weights:
            ok(k.gs_jacobi_sweep(C.byref(self.S), C.byref(self.L), 0, w, self.gamma, a.ptr, b.ptr, self.f.ptr, None,
                                 st()))
            a, b = b, a
        return a.to_xyz()


def main():
    res = {}
    for i, case in enumerate(CASES):
        p = Problem(case)
        res["want%d" % i], res["got%d" % i] = p.reference(), p.triple()
    np.savez(sys.argv[1], **res)


if __name__ == "__main__":
    main()
