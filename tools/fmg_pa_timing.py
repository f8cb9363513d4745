"""Full multigrid with the POSITION prolongation against the POSITION V-cycle on one GPU, on an even size (DESIGN.md
§4.7 "FMG on every size" quotes the result).

    python tools/fmg_pa_timing.py [--n 512] [--rounds 5] [--cycles 10] [--out profiles/fmg_pa]

One process, one n^3 LINEAR 2+2 grid with the POSITION transfers and the POSITION prolongation:
  - a plain solve from zero (12 V-cycles): the residual history FMG(1)'s residual is placed in -> m, the number of
    plain V-cycles that get under it;
  - `rounds` alternations of FMG(1) (events on the grid's stream around gs_grid_fmg, closing norm included; host wall
    time beside it) and gs_grid_time_vcycles (the solve loop's V-cycle, `cycles` of them per round); per round, whether
    FMG(1) took less time than m V-cycles;
  - gs_fmg_prolong_pa alone, n/2 -> n, alternated launch by launch with gs_fmg_prolong, n/2 - 1 -> n - 1 (the aligned
    kernel on the neighbouring odd size: the same bytes within 0.6 %), both on seeded noise in fields of their own;
  - the store-only stream ceiling over an array of n^3 doubles (gs_debug_bw kind 1, the shapes of bench.py's
    ceilings), taken in the same process.
Writes <out>/fmg_pa_timing.json and prints it."""
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
from fmg_timing import median, store_ceiling  # noqa: E402


def fmg_tables(nf):
    """Device copies of the tables of the cube transition nf -> nf // 2: (gs_fmg_tables, the tensors behind it)."""
    T, keep = gsv.gs_fmg_tables(), []
    host = gsv.fmg_axis(nf)
    for a in range(3):
        T.nf[a], T.nc[a] = nf, nf // 2
        for key in ("cj", "cw"):
            t = torch.from_numpy(host[key].reshape(-1).copy()).cuda()
            keep.append(t)
            getattr(T, key)[a] = t.data_ptr()
    return T, keep


def noise(field):
    g = torch.Generator(device="cuda")
    g.manual_seed(field.nx)
    field.zyx[1:-1, 1:-1, 1:field.nx + 1] = torch.rand((field.nz, field.ny, field.nx), generator=g, device="cuda",
                                                       dtype=torch.float64)
    return field


def kernels_alone(n, launches=7):
    """gs_fmg_prolong_pa n/2 -> n beside gs_fmg_prolong n/2 - 1 -> n - 1, alternated; the first two pairs are warm-up."""
    na = n - 1
    cp, fp = noise(DevField(n // 2, n // 2, n // 2)), DevField(n, n, n)
    ca, fa = noise(DevField(na // 2, na // 2, na // 2)), DevField(na, na, na)
    T, keep = fmg_tables(n)
    lv = [x.level(1.0 / (x.ny + 1)) for x in (cp, fp, ca, fa)]
    st = torch.cuda.current_stream()
    e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    pa, al = [], []
    torch.cuda.synchronize()
    for i in range(launches):
        e0.record(st)
        rc0 = gsv.transfer().gs_fmg_prolong_pa(cp.ptr, C.byref(lv[0]), fp.ptr, C.byref(lv[1]), C.byref(T), st.cuda_stream)
        e1.record(st)
        rc1 = gsv.kernels().gs_fmg_prolong(ca.ptr, C.byref(lv[2]), fa.ptr, C.byref(lv[3]), st.cuda_stream)
        e2.record(st)
        assert rc0 == 0 and rc1 == 0, (rc0, rc1)
        e2.synchronize()
        if i >= 2:
            pa.append(e0.elapsed_time(e1))
            al.append(e1.elapsed_time(e2))
    del keep
    return pa, al


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cycles", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "fmg_pa"))
    a = ap.parse_args()
    assert a.rounds >= 1 and a.n % 2 == 0 and torch.cuda.is_available()
    n = a.n
    d = gsv.driver()
    p = gsv.GridParams(maxiter=12, tol=0.0, gridDim=(n, n, n), mode=gsv.GS_LINEAR, preSmoothing=2, postSmoothing=2)
    res = {"n": n, "mode": "LINEAR", "smoothing": "2+2", "transfer": "position", "fmg_prolong": "position",
           "device": torch.cuda.get_device_name(0), "build": gsv.build_info().split(":")[0]}
    with gsv.HipGridData(p) as g:
        g.set_transfer("position")
        g.set_fmg_prolong("position")
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
    res["fmg1_faster_than_m_vcycles"] = None if m is None else [f < m * v for f, v in zip(fmg_ms, vc_ms)]
    pa, al = kernels_alone(n)
    pts = float(n) ** 3
    res["prolong_pa"] = {"transition": [n // 2, n], "ms": median(pa), "launches": pa, "store_bytes": 8 * pts,
                         "store_gbps": 8 * pts / median(pa) / 1e6, "read_bytes": 8 * float(n // 2 + 2) ** 3}
    pts_a = float(n - 1) ** 3
    res["prolong_aligned"] = {"transition": [(n - 1) // 2, n - 1], "ms": median(al), "launches": al,
                              "store_bytes": 8 * pts_a, "store_gbps": 8 * pts_a / median(al) / 1e6}
    res["prolong_pa_over_aligned"] = median(pa) / median(al)
    ceil_ms, ceil_shape = store_ceiling(n ** 3)
    res["store_only_ceiling"] = {"ms": ceil_ms, "gbps": 8 * pts / ceil_ms / 1e6, "shape": ceil_shape}
    res["prolong_pa_fraction_of_store_ceiling"] = ceil_ms / median(pa)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "fmg_pa_timing.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
