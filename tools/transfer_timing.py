"""Position-aware grid transfers against the default ones on one GPU (DESIGN.md §4.9 quotes the result).

    python tools/transfer_timing.py [--n 512] [--aligned 511] [--rounds 4] [--cycles 10] [--out profiles/transfer]
                                    [--no-trace]

One process, LINEAR 2+2, first an n^3 grid (512: every transition non-aligned), then an aligned one (511^3), on which
both modes must give the same bits and the same times:
  - the residual history of ten cycles from zero in each mode, and with the Chebyshev pair (GS_OMEGAS=cheb's weights)
    in POSITION mode;
  - ms per V-cycle (gs_grid_time_vcycles: the solve loop's V-cycle, norm readback included) in POSITION mode against
    the default mode on the same grid, alternated `rounds` times, v zeroed before every batch; the same with the
    Chebyshev pair;
  - the time to the residual the sixth POSITION cycle reaches: cycles needed x ms per cycle, per variant (null where
    ten cycles do not get there);
  - gs_residual_restrict_pa at level 0 alternated against the two-pass composition it replaces (gs_residual with a
    stored r, then gs_restrict_pa), and its algorithmic bytes per second (16 B read per fine point + 8 B written per
    coarse point) as a fraction of the read-only stream ceiling taken in the same process (gs_debug_bw kind 0 over
    bench.py's shapes);
  - unless --no-trace: a kernel trace in a run of its own (a child process under rocprofv3 --kernel-trace --stats
    running three POSITION V-cycles and three stand-alone gs_restrict_pa launches per level), reduced to the
    per-launch times of the three new kernels at levels 0 and 1.
Writes <out>/transfer_timing.json (+ <out>/kernel_trace.csv, kernel_stats.csv) and prints the JSON."""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "gpu-solve_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import gpusolve as gsv  # noqa: E402

NEW_KERNELS = ("k_resrestrict_pa", "k_prolong_add_pa", "k_restrict_pa")


def median(xs):
    s = sorted(xs)
    return s[len(s) // 2] if len(s) % 2 else 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2])


def spread(xs):
    return max(xs) - min(xs)


class Tables:
    """Device copies of one transition's tables (gpusolve.transfer_axis) and their gs_transfer_tables."""

    def __init__(self, fine):
        self.keep, self.abi = [], gsv.gs_transfer_tables()
        for a in range(3):
            T = gsv.transfer_axis(fine[a])
            self.abi.nf[a], self.abi.nc[a] = fine[a], fine[a] // 2
            for key in ("pj", "pt", "rlo", "rcnt", "rw"):
                t = torch.from_numpy(np.ascontiguousarray(T[key]).reshape(-1)).cuda()
                self.keep.append(t)
                getattr(self.abi, key)[a] = t.data_ptr()


def zero_v(g):
    """Level 0's iterate back to zero (the whole padded field), on the grid's stream."""
    L = g.getLevel(0).geom
    rc = gsv.kernels().gs_fill(gsv.driver().gs_grid_field(g.handle, 0, 0), 0.0, L.ldz * (L.nz + 2), g.stream())
    assert rc == 0, rc
    g.sync()


def history(g):
    zero_v(g)
    return gsv.HipSolver.solve(g)


def time_cycles(g, cycles):
    zero_v(g)
    ms, last = C.c_double(), C.c_double()
    rc = gsv.driver().gs_grid_time_vcycles(g.handle, cycles, C.byref(ms), C.byref(last))
    assert rc == 0, gsv.driver().gs_last_error().decode()
    return ms.value / cycles


def read_ceiling(n):
    """Best read-only stream over n doubles: (GB/s, description)."""
    kd = gsv.diag()
    n -= n & 1
    A = torch.zeros(n, dtype=torch.float64, device="cuda")
    O = torch.zeros(16, dtype=torch.float64, device="cuda")
    sink = torch.zeros(1, dtype=torch.float64, device="cuda")
    st = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = None
    for blocks, unroll in [(b, u) for b in (1024, 2048, 4096) for u in (1, 4)] + [(0, u) for u in (1, 2, 4)]:
        for nt in (1, 0):
            def run():
                rc = kd.gs_debug_bw(0, unroll, nt, blocks, O.data_ptr(), A.data_ptr(), A.data_ptr(), n, sink.data_ptr(),
                                    st.cuda_stream)
                assert rc == 0, rc
            run()
            e0.record(st)
            for _ in range(5):
                run()
            e1.record(st)
            torch.cuda.synchronize()
            gbps = 8.0 * n / (e0.elapsed_time(e1) / 5) / 1e6
            if best is None or gbps > best[0]:
                best = (gbps, f"blocks={blocks or 'flat'} unroll={unroll} nt={nt}")
    return best


def fused_against_two_pass(g, rounds, reps=5):
    """gs_residual_restrict_pa at level 0 against gs_residual (r stored) + gs_restrict_pa, alternated."""
    d, t, k = gsv.driver(), gsv.transfer(), gsv.kernels()
    F, Cl = g.getLevel(0).geom, g.getLevel(1).geom
    T = Tables((F.nx, F.ny, F.nz))
    S = gsv.Stencil().to_abi()
    v, f, r = (d.gs_grid_field(g.handle, 0, i) for i in (0, 3, 4))
    cf = d.gs_grid_field(g.handle, 1, 3)
    st = torch.cuda.current_stream()
    g.sync()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def fused():
        assert t.gs_residual_restrict_pa(C.byref(S), C.byref(F), 0, 1.0, v, f, None, cf, C.byref(Cl), C.byref(T.abi),
                                         st.cuda_stream) == 0

    def two_pass():
        assert k.gs_residual(C.byref(S), C.byref(F), 0, 1.0, v, f, None, r, None, st.cuda_stream) == 0
        assert t.gs_restrict_pa(r, C.byref(F), cf, None, C.byref(Cl), C.byref(T.abi), st.cuda_stream) == 0

    def timed(fn):
        fn()
        e0.record(st)
        for _ in range(reps):
            fn()
        e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    a, b = [], []
    for _ in range(rounds):
        a.append(timed(fused))
        b.append(timed(two_pass))
    torch.cuda.synchronize()
    pts, cpts = float(F.nx) * F.ny * F.nz, float(Cl.nx) * Cl.ny * Cl.nz
    return {"fused_ms": {"rounds": a, "median": median(a)}, "two_pass_ms": {"rounds": b, "median": median(b), "spread": spread(b)},
            "fused_faster_by_ms": median(b) - median(a), "fused_wins": median(b) - median(a) > 2 * spread(b),
            "algorithmic_bytes": 16 * pts + 8 * cpts, "fused_gbps": (16 * pts + 8 * cpts) / median(a) / 1e6}


def measure(n, rounds, cycles, kernels):
    p = gsv.GridParams(maxiter=10, tol=0.0, gridDim=(n, n, n), mode=gsv.GS_LINEAR, preSmoothing=2, postSmoothing=2)
    cheb = gsv.chebyshev_weights(2)
    res = {"n": n}
    with gsv.HipGridData(p) as g:
        res["levels"] = g.numLevels()
        res["aligned_transitions"] = [g.level_aligned(l) for l in range(g.numLevels() - 1)]
        same_bits = all(res["aligned_transitions"])  # then both modes must give the same bits: compared below
        res["history_default"] = history(g)
        v_def = g.field(0, "v") if same_bits else None
        g.set_transfer("position")
        res["history_position"] = history(g)
        if same_bits:
            res["identical_fields"] = bool(np.array_equal(v_def, g.field(0, "v")))
        del v_def
        g.set_weights(cheb, cheb)
        res["history_position_cheb"] = history(g)
        g.clear_weights()
        res["identical_histories"] = res["history_default"] == res["history_position"]
        ms = {"default": [], "position": [], "position_cheb": []}
        for _ in range(rounds):
            g.set_transfer("reference")
            ms["default"].append(time_cycles(g, cycles))
            g.set_transfer("position")
            ms["position"].append(time_cycles(g, cycles))
            g.set_weights(cheb, cheb)
            ms["position_cheb"].append(time_cycles(g, cycles))
            g.clear_weights()
        res["vcycle_ms"] = {k: {"rounds": v, "median": median(v), "spread": spread(v)} for k, v in ms.items()}
        res["position_over_default"] = median(ms["position"]) / median(ms["default"])
        target = res["history_position"][6]
        res["target_residual"] = target
        reach = {}
        for name, key in (("default", "history_default"), ("position", "history_position"),
                          ("position_cheb", "history_position_cheb")):
            m = next((i for i, r in enumerate(res[key]) if i >= 1 and r <= target), None)
            reach[name] = {"cycles": m, "ms": None if m is None else m * median(ms[name])}
        res["time_to_target"] = reach
        if kernels and not all(res["aligned_transitions"]):
            res["residual_restrict_level0"] = fused_against_two_pass(g, rounds)
    if "residual_restrict_level0" in res:
        gbps, shape = read_ceiling(n ** 3)
        res["read_only_ceiling"] = {"gbps": gbps, "shape": shape}
        res["residual_restrict_level0"]["fraction_of_read_ceiling"] = res["residual_restrict_level0"]["fused_gbps"] / gbps
    return res


def trace_child(n):
    """The traced run: three POSITION V-cycles, then three stand-alone gs_restrict_pa launches per level 0 and 1."""
    p = gsv.GridParams(maxiter=3, tol=0.0, gridDim=(n, n, n), mode=gsv.GS_LINEAR, preSmoothing=2, postSmoothing=2)
    d, t = gsv.driver(), gsv.transfer()
    with gsv.HipGridData(p) as g:
        g.set_transfer("position")
        gsv.HipSolver.solve(g)
        for l in (0, 1):
            F, Cl = g.getLevel(l).geom, g.getLevel(l + 1).geom
            T = Tables((F.nx, F.ny, F.nz))
            for _ in range(3):
                rc = t.gs_restrict_pa(d.gs_grid_field(g.handle, l, 0), C.byref(F), d.gs_grid_field(g.handle, l + 1, 4),
                                      None, C.byref(Cl), C.byref(T.abi), g.stream())
                assert rc == 0, rc
            g.sync()


def kernel_trace(n, out):
    """Runs trace_child under rocprofv3 and reduces its kernel trace: {kernel: {"level0": [...us], "level1": [...]}}."""
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    tmp = tempfile.mkdtemp(prefix="transfer_trace_")
    cmd = [exe, "--kernel-trace", "--stats", "-d", tmp, "-o", "run", "--output-format", "csv", "--", sys.executable,
           os.path.abspath(__file__), "--trace-child", "--n", str(n)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        return {"error": (r.stderr or r.stdout)[-400:]}
    trace = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
    stats = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
    if not trace:
        return {"error": "no kernel trace written"}
    per = {}
    rows = []
    for row in csv.DictReader(open(trace[0])):
        name = row["Kernel_Name"].replace("(anonymous namespace)::", "").split("(")[0]
        rows.append(row)
        for kname in NEW_KERNELS:
            if name.split("<")[0].strip().split(" ")[-1] == kname:
                blocks = int(row["Grid_Size_X"]) * int(row["Grid_Size_Y"]) * int(row["Grid_Size_Z"])
                per.setdefault(kname, {}).setdefault(blocks, []).append(
                    (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    # the trace itself, new kernels only (the whole one is tens of thousands of lines), and the stats table
    with open(os.path.join(out, "kernel_trace.csv"), "w", newline="") as fh:
        w = csv.DictWriter(fh, fieldnames=list(rows[0].keys()))
        w.writeheader()
        for row in rows:
            if any(kname in row["Kernel_Name"] for kname in NEW_KERNELS):
                w.writerow(row)
    if stats:
        shutil.copy(stats[0], os.path.join(out, "kernel_stats.csv"))
    shutil.rmtree(tmp, ignore_errors=True)
    res = {}
    for kname, by_grid in per.items():
        sizes = sorted(by_grid, reverse=True)  # the largest grid is level 0's
        res[kname] = {f"level{i}": {"grid_threads": s, "us": by_grid[s], "median_us": median(by_grid[s])}
                      for i, s in enumerate(sizes[:2])}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--aligned", type=int, default=511)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--cycles", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "transfer"))
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    assert torch.cuda.is_available()
    if a.trace_child:
        trace_child(a.n)
        return
    assert a.rounds >= 4
    os.makedirs(a.out, exist_ok=True)
    res = {"mode": "LINEAR", "smoothing": "2+2", "device": torch.cuda.get_device_name(0),
           "build": gsv.build_info().split(":")[0], "cycles_per_round": a.cycles}
    res["even"] = measure(a.n, a.rounds, a.cycles, kernels=True)
    res["aligned"] = measure(a.aligned, a.rounds, a.cycles, kernels=False)
    if not a.no_trace:
        res["kernel_trace"] = kernel_trace(a.n, a.out)
    with open(os.path.join(a.out, "transfer_timing.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
