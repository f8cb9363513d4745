"""Full multigrid against the plain V-cycle on one GPU (DESIGN.md's FMG section quotes the result).

    python tools/fmg_timing.py [--n 511] [--rounds 4] [--cycles 10] [--out profiles/fmg]

One process, one n^3 LINEAR 2+2 grid:
  - a plain solve from zero (12 V-cycles): the residual history FMG(1)'s residual is placed in -> m, the number of
    plain V-cycles that get under it;
  - `rounds` alternations of FMG(1) (events on the grid's stream around gs_grid_fmg, closing norm included; host wall
    time beside it) and gs_grid_time_vcycles (the solve loop's V-cycle, `cycles` of them per round);
  - gs_fmg_prolong alone at level 0 (level 1's v -> level 0's v) against the store-only stream ceiling over an
    array of the same size (gs_debug_bw kind 1, the shapes of bench.py's ceilings), taken in the same process.
Writes <out>/fmg_timing.json and prints it."""
import argparse
import ctypes as C
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "gpu-solve_amd"))

import torch  # noqa: E402

import gpusolve as gsv  # noqa: E402


def median(xs):
    s = sorted(xs)
    return s[len(s) // 2] if len(s) % 2 else 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2])


def store_ceiling(n):
    """Best store-only stream over n doubles: (ms, description)."""
    kd = gsv.diag()
    n -= n & 1  # (the probe stores 16 bytes per lane)
    O = torch.empty(n, dtype=torch.float64, device="cuda")
    A = torch.zeros(16, dtype=torch.float64, device="cuda")
    sink = torch.zeros(1, dtype=torch.float64, device="cuda")
    st = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = None
    for blocks, unroll in [(2048, 4), (4096, 4), (0, 1), (0, 2), (0, 4)]:
        for nt in (1, 0):
            def run():
                rc = kd.gs_debug_bw(1, unroll, nt, blocks, O.data_ptr(), A.data_ptr(), A.data_ptr(), n,
                                    sink.data_ptr(), st.cuda_stream)
                assert rc == 0, rc
            run()
            e0.record(st)
            for _ in range(5):
                run()
            e1.record(st)
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / 5
            if best is None or ms < best[0]:
                best = (ms, f"blocks={blocks or 'flat'} unroll={unroll} nt={nt}")
    del O
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=511)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--cycles", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "fmg"))
    a = ap.parse_args()
    assert a.rounds >= 1 and torch.cuda.is_available()
    n = a.n
    d = gsv.driver()
    p = gsv.GridParams(maxiter=12, tol=0.0, gridDim=(n, n, n), mode=gsv.GS_LINEAR, preSmoothing=2, postSmoothing=2)
    res = {"n": n, "mode": "LINEAR", "smoothing": "2+2", "device": torch.cuda.get_device_name(0),
           "build": gsv.build_info().split(":")[0]}
    with gsv.HipGridData(p) as g:
        plain = gsv.HipSolver.solve(g)
        res["plain_history"] = plain
        res["fmg_start_level"] = g.fmg_start_level()
        ext = torch.cuda.ExternalStream(g.stream())
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fmg_ms, fmg_wall_ms, vc_ms, fmg_res = [], [], [], None
        gsv.HipSolver.fmg(g, 1)  # untimed: first launches of every kernel
        for _ in range(a.rounds):
            g.sync()
            t0 = time.perf_counter()
            e0.record(ext)
            fmg_res = gsv.HipSolver.fmg(g, 1)
            e1.record(ext)
            e1.synchronize()
            fmg_wall_ms.append((time.perf_counter() - t0) * 1e3)
            fmg_ms.append(e0.elapsed_time(e1))
            ms, last = C.c_double(), C.c_double()
            rc = d.gs_grid_time_vcycles(g.handle, a.cycles, C.byref(ms), C.byref(last))
            assert rc == 0, d.gs_last_error().decode()
            vc_ms.append(ms.value / a.cycles)
        res["fmg1_residual"] = fmg_res
        res["fmg1_ms"] = {"rounds": fmg_ms, "median": median(fmg_ms), "host_wall_median": median(fmg_wall_ms)}
        res["vcycle_ms"] = {"rounds": vc_ms, "median": median(vc_ms), "cycles_per_round": a.cycles}
        res["fmg1_over_vcycle"] = median(fmg_ms) / median(vc_ms)
        # m: plain V-cycles from zero to get under FMG(1)'s residual (plain[0] is the initial residual)
        m = next((i for i, r in enumerate(plain) if i >= 1 and r < fmg_res), None)
        res["m_plain_cycles_under_fmg1"] = m
        # the prolongation kernel alone at level 0
        kl = gsv.kernels()
        c, f = g.getLevel(1).geom, g.getLevel(0).geom
        cv, fv = d.gs_grid_field(g.handle, 1, 0), d.gs_grid_field(g.handle, 0, 0)
        st = torch.cuda.current_stream()
        g.sync()
        torch.cuda.synchronize()
        times = []
        for i in range(7):
            e0.record(st)
            rc = kl.gs_fmg_prolong(cv, C.byref(c), fv, C.byref(f), st.cuda_stream)
            e1.record(st)
            assert rc == 0, rc
            e1.synchronize()
            if i >= 2:
                times.append(e0.elapsed_time(e1))
        torch.cuda.synchronize()
    pts = float(n) ** 3
    pro_ms = median(times)
    ceil_ms, ceil_shape = store_ceiling(n ** 3)
    res["prolong_level0"] = {"ms": pro_ms, "launches": times, "store_bytes": 8 * pts, "store_gbps": 8 * pts / pro_ms / 1e6,
                             "read_bytes": 8 * float(n // 2 + 2) ** 3}
    res["store_only_ceiling"] = {"ms": ceil_ms, "gbps": 8 * pts / ceil_ms / 1e6, "shape": ceil_shape}
    res["prolong_fraction_of_store_ceiling"] = ceil_ms / pro_ms
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "fmg_timing.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
