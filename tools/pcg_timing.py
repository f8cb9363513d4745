"""Preconditioned conjugate gradients against plain V-cycles on one GPU (DESIGN.md §4.10 quotes the result).

    python tools/pcg_timing.py [--rounds 5] [--out profiles/pcg] [--small] [--passes-only]

One process, alternated rounds (neither side gets the colder or the warmer half of the job):
  (a) time to reduce the residual by 10^8 — tol = 1e-8, from a zero iterate, host wall time around gs_grid_pcg and
      gs_grid_solve with the stream idle before and after — in four LINEAR 2+2 cases: 511^3, 512^3 with the POSITION
      transfers, 511^3 with Chebyshev weights on both legs, 255^3 with the anisotropic stencil
      (4.1, -1, -1, -1, -1, -0.05, -0.05). Each case: one grid, one untimed run of each solver first (first launches,
      PCG's allocation), then `rounds` alternations. A side that does not reach the tolerance in its iteration cap is
      reported with the reduction it did reach.
  (b) per-launch times of gs_pcg_dir, gs_pcg_step and gs_dot at 512^3 on seeded noise (events around single launches),
      alternated launch by launch with one k_rb Jacobi sweep (gs_jacobi_sweep, 24 B per point), the flat triad
      (gs_debug_stream_triad, 24 B per point) and the best copy (gs_debug_bw kind 2, 16 B per point): bytes per second
      of each, and the passes' rates over k_rb's and over the ceilings'.
--small: 127^3 / 128^3 / 63^3 instead (a functional check of the tool, not a measurement).
Writes <out>/pcg_timing.json and prints it."""
import argparse
import ctypes as C
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "gpu-solve_amd"))
sys.path.insert(0, HERE)

import torch  # noqa: E402

import gpusolve as gsv  # noqa: E402
from gpusolve.devfield import DevField  # noqa: E402
from fmg_timing import median  # noqa: E402

ANISO = [4.1, -1.0, -1.0, -1.0, -1.0, -0.05, -0.05]


def zero_iterate(g):
    geom = g.getLevel(0).geom
    ptr = gsv.driver().gs_grid_field(g.handle, 0, 0)
    rc = gsv.kernels().gs_fill(ptr, 0.0, geom.ldz * (geom.nz + 2), g.stream())
    assert rc == 0, rc
    g.sync()


def timed(g, fn):
    zero_iterate(g)
    t0 = time.perf_counter()
    hist = fn(g)
    g.sync()
    return (time.perf_counter() - t0) * 1e3, hist


def solve_case(name, dims, rounds, cap, transfer=None, cheb=False, stencil=None):
    p = gsv.GridParams(maxiter=cap, tol=1e-8, gridDim=dims, mode=gsv.GS_LINEAR, preSmoothing=2, postSmoothing=2,
                       stencil=gsv.Stencil(stencil) if stencil else gsv.Stencil())
    out = {"case": name, "dims": list(dims), "tol": 1e-8, "iteration_cap": cap}
    with gsv.HipGridData(p) as g:
        if transfer:
            g.set_transfer(transfer)
        if cheb:
            w = gsv.chebyshev_weights(2)
            g.set_weights(w, w)
            out["weights"] = list(w)
        assert g.pcg_supported(), g.pcg_refusal
        timed(g, gsv.HipSolver.pcg)
        timed(g, gsv.HipSolver.solve)
        pcg_ms, vc_ms, ph, vh = [], [], None, None
        for _ in range(rounds):
            ms, ph = timed(g, gsv.HipSolver.pcg)
            pcg_ms.append(ms)
            ms, vh = timed(g, gsv.HipSolver.solve)
            vc_ms.append(ms)
    for key, ms, h in (("pcg", pcg_ms, ph), ("vcycle", vc_ms, vh)):
        it = len(h) - 1
        out[key] = {"ms_rounds": ms, "ms": median(ms), "iterations": it, "reached": h[-1] <= h[0] * 1e-8,
                    "reduction": h[-1] / h[0], "ms_per_iteration": median(ms) / max(it, 1),
                    "mean_factor": (h[-1] / h[0]) ** (1.0 / max(it, 1)), "history": h}
    out["vcycle_over_pcg_time"] = out["vcycle"]["ms"] / out["pcg"]["ms"]
    return out


def noise(field, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    field.zyx[1:-1, 1:-1, 1:field.nx + 1] = torch.rand((field.nz, field.ny, field.nx), generator=g, device="cuda",
                                                       dtype=torch.float64) - 0.5
    return field


def passes(n, launches):
    kr, k, kd = gsv.krylov(), gsv.kernels(), gsv.diag()
    z, p_in, x, r, f = (noise(DevField(n, n, n), s) for s in range(5))
    p_out, q = DevField(n, n, n), DevField(n, n, n)
    L = z.level(1.0 / (n + 1))
    S = gsv.Stencil().to_abi()
    nparts = max(kr.gs_pcg_dir_num_partials(C.byref(S), C.byref(L)), kr.gs_pcg_step_num_partials(C.byref(L)), 1)
    parts = torch.zeros(nparts, dtype=torch.float64, device="cuda")
    scal = torch.tensor([1e-3, -0.25], dtype=torch.float64, device="cuda")  # alpha, beta
    a_ptr, b_ptr = scal.data_ptr(), scal.data_ptr() + 8
    pts = float(n) ** 3
    flat = 2 * (z.span // 2)
    sink = torch.zeros(1, dtype=torch.float64, device="cuda")
    st = torch.cuda.current_stream()
    s = st.cuda_stream
    copies = [(0, 4, 1), (0, 2, 1), (2048, 4, 1), (0, 4, 0)]
    runs = {
        "gs_pcg_dir": (32, lambda: kr.gs_pcg_dir(C.byref(S), C.byref(L), z.ptr, p_in.ptr, p_out.ptr, q.ptr, b_ptr,
                                                  parts.data_ptr(), s)),
        "gs_pcg_dir_first": (24, lambda: kr.gs_pcg_dir(C.byref(S), C.byref(L), z.ptr, None, p_out.ptr, q.ptr, None,
                                                        parts.data_ptr(), s)),
        "gs_pcg_step": (48, lambda: kr.gs_pcg_step(C.byref(L), x.ptr, r.ptr, p_out.ptr, q.ptr, a_ptr, parts.data_ptr(), s)),
        "gs_dot": (16, lambda: kr.gs_dot(C.byref(L), r.ptr, z.ptr, parts.data_ptr(), s)),
        "k_rb_sweep": (24, lambda: k.gs_jacobi_sweep(C.byref(S), C.byref(L), 0, 0.8, 1.0, z.ptr, p_out.ptr, f.ptr, None, s)),
        "triad": (24 * flat / pts, lambda: kd.gs_debug_stream_triad(p_out.ptr, z.ptr, p_in.ptr, flat, s)),
    }
    for blocks, unroll, nt in copies:
        runs[f"copy blocks={blocks or 'flat'} unroll={unroll} nt={nt}"] = (
            16 * flat / pts, lambda b=blocks, u=unroll, t=nt: kd.gs_debug_bw(2, u, t, b, p_out.ptr, z.ptr, z.ptr, flat,
                                                                              sink.data_ptr(), s))
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
    res = {"n": n, "launches": launches, "instance": kr.gs_pcg_dir_kernel(C.byref(S), C.byref(L), 0).decode()}
    for name, (bpp, _) in runs.items():
        m = median(ms[name])
        res[name] = {"ms": m, "ms_launches": ms[name], "bytes_per_point": bpp, "gbps": bpp * pts / m / 1e6}
    best_copy = max((v for kname, v in res.items() if kname.startswith("copy ")), key=lambda v: v["gbps"])
    res["copy_best_gbps"] = best_copy["gbps"]
    for name in ("gs_pcg_dir", "gs_pcg_dir_first", "gs_pcg_step", "gs_dot"):
        res[name]["over_k_rb"] = res[name]["gbps"] / res["k_rb_sweep"]["gbps"]
        res[name]["over_triad"] = res[name]["gbps"] / res["triad"]["gbps"]
        res[name]["over_copy"] = res[name]["gbps"] / best_copy["gbps"]
    res["three_passes_ms"] = res["gs_pcg_dir"]["ms"] + res["gs_pcg_step"]["ms"] + res["gs_dot"]["ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--passes-only", action="store_true", help="part (b) alone")
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "pcg"))
    a = ap.parse_args()
    assert a.rounds >= 1 and torch.cuda.is_available()
    odd, even, an = (127, 128, 63) if a.small else (511, 512, 255)
    res = {"device": torch.cuda.get_device_name(0), "build": gsv.build_info().split(":")[0], "smoothing": "2+2",
           "mode": "LINEAR", "rounds": a.rounds, "solves": []}
    if not a.passes_only:
        res["solves"].append(solve_case(f"{odd}^3", (odd,) * 3, a.rounds, 40))
        res["solves"].append(solve_case(f"{even}^3 POSITION", (even,) * 3, a.rounds, 40, transfer="position"))
        res["solves"].append(solve_case(f"{odd}^3 chebyshev", (odd,) * 3, a.rounds, 40, cheb=True))
        res["solves"].append(solve_case(f"{an}^3 anisotropic", (an,) * 3, a.rounds, 150, stencil=ANISO))
    res["passes"] = passes(even, 7)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "pcg_timing.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
