"""The z-line smoother against point Jacobi on one GPU (DESIGN.md §4.11 quotes the result).

    python tools/zline_timing.py [--rounds 3] [--out profiles/zline] [--small] [--sweeps-only]

One process, alternated rounds (no side gets the colder or the warmer half of the job):
  (a) time to reduce the residual by 10^8 — tol = 1e-8, from a zero iterate, host wall time around gs_grid_solve /
      gs_grid_pcg with the stream idle before and after — for the point V-cycle (cap 150 cycles), PCG on the point
      cycle, the z-line V-cycle and PCG on the z-line cycle, LINEAR 2+2 at omega = 0.8, on the strong-z stencil
      (2.2, -0.05, -0.05, -0.05, -0.05, -1, -1) at 255^3 and 511^3 and on the isotropic stencil at 511^3 (where the
      z-line cycle is expected to lose). f: seeded standard normal on the interior. Each case: one grid, one untimed
      run of each of the four first, then `rounds` alternations. A side that does not reach the tolerance in its cap
      is reported with the reduction it did reach.
  (b) per-launch time of gs_zline_sweep (48 B per point; the zero-iterate form: 32 B) at 511^3 and 255^3 on seeded
      noise, events around single launches, alternated launch by launch with one k_rb Jacobi sweep (gs_jacobi_sweep,
      24 B per point): bytes per second of each and the line sweep's rate over k_rb's.
--small: 63^3 / 127^3 instead (a functional check of the tool, not a measurement).
Writes <out>/zline_timing.json and prints it."""
import argparse
import ctypes as C
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "gpu-solve_amd"))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import gpusolve as gsv  # noqa: E402
from gpusolve.devfield import DevField  # noqa: E402
from fmg_timing import median  # noqa: E402
from pcg_timing import timed  # noqa: E402

STRONGZ = [2.2, -0.05, -0.05, -0.05, -0.05, -1.0, -1.0]
ISO = [6.0, -1.0, -1.0, -1.0, -1.0, -1.0, -1.0]
F_FIELD = 3  # gpusolve.FIELDS["f"]


def normal(field, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    field.zyx[1:-1, 1:-1, 1:field.nx + 1] = torch.randn((field.nz, field.ny, field.nx), generator=g, device="cuda",
                                                        dtype=torch.float64)
    return field


def solve_case(name, n, stencil, rounds, rhs):
    p = gsv.GridParams(maxiter=150, tol=1e-8, gridDim=(n, n, n), mode=gsv.GS_LINEAR, preSmoothing=2, postSmoothing=2,
                       stencil=gsv.Stencil(stencil))
    sides = [("point_vcycle", "jacobi", gsv.HipSolver.solve), ("point_pcg", "jacobi", gsv.HipSolver.pcg),
             ("zline_vcycle", "zline", gsv.HipSolver.solve), ("zline_pcg", "zline", gsv.HipSolver.pcg)]
    out = {"case": name, "n": n, "stencil": stencil, "tol": 1e-8, "iteration_cap": 150}
    with gsv.HipGridData(p) as g:
        geom = g.getLevel(0).geom
        assert (geom.ldy, geom.ldz) == (rhs.ldy, rhs.ldz)
        rc = gsv.kernels().gs_copy(gsv.driver().gs_grid_field(g.handle, 0, F_FIELD), rhs.ptr, rhs.span, g.stream())
        assert rc == 0, rc
        g.sync()
        assert g.pcg_supported(), g.pcg_refusal
        ms = {k: [] for k, _, _ in sides}
        hist = {}
        for r in range(rounds + 1):  # round 0 is untimed: first launches, PCG's allocation, the factors' upload
            for key, smoother, fn in sides:
                g.set_smoother(smoother)
                t, hist[key] = timed(g, fn)
                if r > 0:
                    ms[key].append(t)
        g.set_smoother("jacobi")
    for key, _, _ in sides:
        h = hist[key]
        it = len(h) - 1
        out[key] = {"ms_rounds": ms[key], "ms": median(ms[key]), "iterations": it, "reached": h[-1] <= h[0] * 1e-8,
                    "reduction": h[-1] / h[0], "ms_per_iteration": median(ms[key]) / max(it, 1),
                    "mean_factor": (h[-1] / h[0]) ** (1.0 / max(it, 1)), "history": h}
    out["point_pcg_over_zline_vcycle_time"] = out["point_pcg"]["ms"] / out["zline_vcycle"]["ms"]
    out["zline_cycle_over_point_cycle_time"] = out["zline_vcycle"]["ms_per_iteration"] / out["point_vcycle"]["ms_per_iteration"]
    return out


def sweeps(n, launches):
    ln, k = gsv.line(), gsv.kernels()
    v, f = normal(DevField(n, n, n), 2), normal(DevField(n, n, n), 3)
    out = DevField(n, n, n)
    L = v.level(1.0 / (n + 1))
    S = gsv.Stencil(STRONGZ).to_abi()
    cp, den = np.zeros(n + 2), np.zeros(n + 2)
    assert ln.gs_zline_factors(C.byref(S), n, cp.ctypes.data_as(gsv._abi.dptr), den.ctypes.data_as(gsv._abi.dptr)) == 0
    tab = torch.from_numpy(np.concatenate([cp, den])).cuda()
    T = gsv.gs_zline_tables(tab.data_ptr(), tab.data_ptr() + 8 * (n + 2), n)
    st = torch.cuda.current_stream()
    s = st.cuda_stream
    pts = float(n) ** 3
    runs = {
        "gs_zline_sweep": (48, lambda: ln.gs_zline_sweep(C.byref(S), C.byref(L), 0.8, v.ptr, out.ptr, f.ptr, C.byref(T), s)),
        "gs_zline_sweep_zero": (32, lambda: ln.gs_zline_sweep(C.byref(S), C.byref(L), 0.8, None, out.ptr, f.ptr, C.byref(T), s)),
        "k_rb_sweep": (24, lambda: k.gs_jacobi_sweep(C.byref(S), C.byref(L), 0, 0.8, 1.0, v.ptr, out.ptr, f.ptr, None, s)),
    }
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = {name: [] for name in runs}
    torch.cuda.synchronize()
    for i in range(launches + 2):  # the first two rounds are warm-up
        for name, (_, fn) in runs.items():
            e0.record(st)
            rc = fn()
            e1.record(st)
            assert rc == 0, (name, rc)
            e1.synchronize()
            if i >= 2:
                ms[name].append(e0.elapsed_time(e1))
    res = {"n": n, "launches": launches, "instance": ln.gs_zline_kernel(C.byref(S), C.byref(L), 0).decode()}
    for name, (bpp, _) in runs.items():
        m = median(ms[name])
        res[name] = {"ms": m, "ms_launches": ms[name], "bytes_per_point": bpp, "gbps": bpp * pts / m / 1e6}
    for name in ("gs_zline_sweep", "gs_zline_sweep_zero"):
        res[name]["over_k_rb"] = res[name]["gbps"] / res["k_rb_sweep"]["gbps"]
        res[name]["ms_over_k_rb_ms"] = res[name]["ms"] / res["k_rb_sweep"]["ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--sweeps-only", action="store_true", help="part (b) alone")
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "zline"))
    a = ap.parse_args()
    assert a.rounds >= 1 and torch.cuda.is_available()
    mid, big = (63, 127) if a.small else (255, 511)
    res = {"device": torch.cuda.get_device_name(0), "build": gsv.build_info().split(":")[0], "smoothing": "2+2",
           "omega": 0.8, "mode": "LINEAR", "rounds": a.rounds, "solves": []}
    if not a.sweeps_only:
        for n, stencil, name in ((mid, STRONGZ, f"{mid}^3 strong-z"), (big, STRONGZ, f"{big}^3 strong-z"),
                                 (big, ISO, f"{big}^3 isotropic")):
            res["solves"].append(solve_case(name, n, stencil, a.rounds, normal(DevField(n, n, n), 1)))
    res["sweeps"] = [sweeps(big, 7), sweeps(mid, 7)]
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "zline_timing.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
