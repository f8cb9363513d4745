#!/usr/bin/env python3
"""The launchers' plan queries over a fixed list of levels (CPU only: the queries launch nothing and need no
device). Two trees whose outputs are equal choose the same shapes, chunks, grids and workspaces.

  python3 tools/plan_queries.py [--lib path/to/libgpusolve_hip.so] [--fold] > plans.txt

One line per (stencil, nx, ny, nz, z0). First the queries that take no mode: gs_jacobi_sweep3_supported,
gs_residual_num_partials, gs_residual_restrict_slab_supported, gs_newton_F_update_supported and
gs_newton_F_update_restrict_supported (against the hierarchy's coarse level, n / 2 per axis). Then, per group of
modes that answer alike (m0 LINEAR .. m4 NEWTON_G): gs_jacobi_sweep2_supported_mode, the shape gs_jacobi_sweep2_kernel
names (- none, Y whole rows, X column blocks), gs_jacobi_sweep2_num_partials, gs_jacobi_sweep2_prolong_supported,
gs_jacobi_sweep2_prolong_ws_elems and gs_tiled_supported.
--fold: one line per (stencil, nx) instead, the SHA-1 of its 75 lines (a record short enough to keep; where two
records differ, the unfolded outputs show which levels).
"""
import argparse
import ctypes as C
import hashlib
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpu-solve_amd"))
import gpusolve as gsv  # noqa: E402

NX = (1, 63, 64, 127, 128, 130, 256, 257, 511, 512, 513, 700, 1024, 1025, 2000, 2**20, 2**20 + 1)
NYZ = (1, 6, 64, 255, 512)
Z0 = (0, 1, 2)
STENCILS = {"unit": [6.0] + [-1.0] * 6, "general": [6.5, -1.0, -1.25, -1.0, -0.75, -1.0, -1.0]}


def level(k, nx, ny, nz, z0=0):
    ldy, ldz, alloc, origin = (C.c_int64() for _ in range(4))
    assert k.gs_field_layout(nx, ny, nz, C.byref(ldy), C.byref(ldz), C.byref(alloc), C.byref(origin)) == 0
    return gsv._abi.gs_level(nx, ny, nz, ldy.value, ldz.value, z0, 1.0 / (ny + 1))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    # (only the library asked for is loaded: its entry points call each other by name)
    ap.add_argument("--lib", help="another build's libgpusolve_hip.so (default: this tree's)")
    ap.add_argument("--fold", action="store_true", help="one line per (stencil, nx): the SHA-1 of its lines")
    a = ap.parse_args()
    k = gsv._abi._load(os.path.abspath(a.lib), gsv._abi.KERNEL_API) if a.lib else gsv.kernels()
    for sname, values in STENCILS.items():
        S = gsv._abi.gs_stencil()
        S.s[:] = values
        S.ox[:], S.oy[:], S.oz[:] = zip(*gsv.CANONICAL_OFFSETS)
        s = C.byref(S)
        for nx in NX:
            lines = []
            for ny in NYZ:
                for nz in NYZ:
                    cl = level(k, nx // 2, ny // 2, nz // 2)
                    for z0 in Z0:
                        L = level(k, nx, ny, nz, z0)
                        p = C.byref(L)
                        out = [f"{sname} {nx} {ny} {nz} z0={z0}", "t3=%d rp=%d slab=%d nu=%d nur=%d" % (
                            k.gs_jacobi_sweep3_supported(s, p), k.gs_residual_num_partials(s, p),
                            k.gs_residual_restrict_slab_supported(s, p), k.gs_newton_F_update_supported(s, p),
                            k.gs_newton_F_update_restrict_supported(s, p, C.byref(cl)))]
                        groups = {}
                        for mode in range(5):
                            name = k.gs_jacobi_sweep2_kernel(s, p, mode).decode()
                            shape = "-" if not name else ("Y" if name.startswith("k_tb2y:") else "X")
                            ans = "%d%s p=%d pro=%d ws=%d tiled=%d" % (
                                k.gs_jacobi_sweep2_supported_mode(s, p, mode), shape,
                                k.gs_jacobi_sweep2_num_partials(s, p, mode),
                                k.gs_jacobi_sweep2_prolong_supported(s, p, mode),
                                k.gs_jacobi_sweep2_prolong_ws_elems(s, p, mode), k.gs_tiled_supported(s, p, mode))
                            groups.setdefault(ans, []).append(str(mode))
                        out += ["m" + "".join(ms) + ":" + ans for ans, ms in groups.items()]
                        lines.append(" | ".join(out))
            if a.fold:
                print(f"{sname} {nx}: {len(lines)} levels sha1={hashlib.sha1(chr(10).join(lines).encode()).hexdigest()}")
            else:
                print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
