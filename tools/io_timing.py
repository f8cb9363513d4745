#!/usr/bin/env python3
"""Device time of the field import / export instances against gs_copy, and the end-to-end cost of feeding a grid
(profiles/io/).

    python tools/io_timing.py kernels --n 512 [--rounds 7] [--out profiles/io/kernels_512.json]
        level 0 of an n^3 grid. Per round, one launch each, in this order, HIP events around every single launch:
        gs_copy (padded -> padded, 16 B per point), rows fp64 import, rows fp64 export, gs_copy again, rows fp32
        import / export (12 B per point), tile fp64 import / export (order "xyz"), tile fp32 import / export.
        The first round warms up and is dropped. GB/s counts interior points x (8 + external element size) for the
        io instances and the copied span x 16 for gs_copy.
    python tools/io_timing.py e2e --n 511 [--reps 5] [--out profiles/io/e2e_511.json]
        host wall time, median: load("f") + store("v") (device tensors, with a final stream synchronise) against
        set_field + field (host arrays).

Run one sub-command per process, each under its own time limit."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "gpu-solve_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import gpusolve as gsv  # noqa: E402
from gpusolve import _abi as A  # noqa: E402
from gpusolve.devfield import DevField  # noqa: E402


def timed(fn, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    rc = fn()
    b.record(stream)
    assert rc == 0, rc
    b.synchronize()
    return a.elapsed_time(b)


def kernels(n, rounds):
    io, k = gsv.io(), gsv.kernels()
    stream = torch.cuda.current_stream()
    st = stream.cuda_stream
    fa, fb = DevField(n, n, n, fill=1.0), DevField(n, n, n)
    L = fa.level(1.0 / (n + 1))
    pts = n ** 3
    ext = {A.GS_IO_F64: torch.rand(pts, dtype=torch.float64, device="cuda"),
           A.GS_IO_F32: torch.rand(pts, dtype=torch.float32, device="cuda")}
    rows, xyz = (A.i64 * 3)(1, n, n * n), (A.i64 * 3)(n * n, n, 1)
    span = fa.span

    def copy():
        return k.gs_copy(fb.ptr, fa.ptr, span, st)

    def imp(dt, s):
        return lambda: io.gs_io_import(fb.ptr, C.byref(L), ext[dt].data_ptr(), dt, s, 1.0, st)

    def exp(dt, s):
        return lambda: io.gs_io_export(fa.ptr, C.byref(L), ext[dt].data_ptr(), dt, s, 1.0, st)

    steps = [("gs_copy", copy, 16 * span), ("rows_f64_import", imp(0, rows), 16 * pts),
             ("rows_f64_export", exp(0, rows), 16 * pts), ("gs_copy_2", copy, 16 * span),
             ("rows_f32_import", imp(1, rows), 12 * pts), ("rows_f32_export", exp(1, rows), 12 * pts),
             ("tile_f64_import", imp(0, xyz), 16 * pts), ("tile_f64_export", exp(0, xyz), 16 * pts),
             ("tile_f32_import", imp(1, xyz), 12 * pts), ("tile_f32_export", exp(1, xyz), 12 * pts)]
    ms = {name: [] for name, _, _ in steps}
    for r in range(rounds + 1):
        for name, fn, _ in steps:
            t = timed(fn, stream)
            if r:
                ms[name].append(t)
    out = {"n": n, "rounds": rounds, "points": pts, "span": span, "device": torch.cuda.get_device_name(0),
           "instances": {"rows_f64": io.gs_io_kernel(0, 0, C.byref(L), rows).decode(),
                         "rows_f32": io.gs_io_kernel(0, 1, C.byref(L), rows).decode(),
                         "tile_f64": io.gs_io_kernel(0, 0, C.byref(L), xyz).decode()}, "steps": {}}
    for name, _, nbytes in steps:
        v = ms[name]
        med = statistics.median(v)
        out["steps"][name] = {"ms": v, "median_ms": med, "min_ms": min(v), "max_ms": max(v), "bytes": nbytes,
                              "gbps_median": nbytes / med / 1e6, "gbps_min": nbytes / max(v) / 1e6,
                              "gbps_max": nbytes / min(v) / 1e6}
    return out


def e2e(n, reps):
    p = gsv.GridParams(maxiter=1, tol=0.0, gridDim=(n, n, n), mode=gsv.GS_LINEAR)
    dev, host = [], []
    with gsv.HipGridData(p) as g:
        f_dev = torch.rand(n, n, n, dtype=torch.float64, device="cuda")
        out = torch.empty_like(f_dev)
        f_host = np.zeros((n + 2, n + 2, n + 2))
        f_host[1:-1, 1:-1, 1:-1] = f_dev.cpu().numpy().transpose(2, 1, 0)
        torch.cuda.synchronize()
        for r in range(reps + 1):
            t0 = time.perf_counter()
            g.load("f", f_dev)
            g.store("v", out=out)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            g.set_field(0, "f", f_host)
            v = g.field(0, "v")
            t2 = time.perf_counter()
            if r:
                dev.append(1e3 * (t1 - t0))
                host.append(1e3 * (t2 - t1))
            del v
    return {"n": n, "reps": reps, "device_path_ms": dev, "host_path_ms": host,
            "device_path_median_ms": statistics.median(dev), "host_path_median_ms": statistics.median(host)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=["kernels", "e2e"])
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    ap.add_argument("--io-lib", help="kernels: another build of libgpusolve_io.so to time (an A/B of a source change)")
    a = ap.parse_args()
    if a.io_lib:
        A.IO_LIB = os.path.abspath(a.io_lib)
    res = kernels(a.n, a.rounds) if a.what == "kernels" else e2e(a.n, a.reps)
    res["io_lib"] = a.io_lib
    text = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    brief = ({k: round(v["median_ms"], 4) for k, v in res["steps"].items()} if a.what == "kernels" else
             {k: res[k] for k in ("device_path_median_ms", "host_path_median_ms")})
    print(json.dumps({"what": a.what, "n": a.n, **brief}))


if __name__ == "__main__":
    main()
