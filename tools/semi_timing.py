"""XY semi-coarsening against the existing options on one GPU (DESIGN.md §4.12 quotes the result).

    python tools/semi_timing.py [--rounds 3] [--out profiles/semi] [--small] [--kernels-only]

One process, alternated rounds (no side gets the colder or the warmer half of the job):
  (a) time to reduce the residual by 10^8 — tol = 1e-8, from a zero iterate, host wall time around gs_grid_solve /
      gs_grid_pcg with the stream idle before and after, LINEAR 2+2 at omega = 0.8 — at 255^3 and 511^3 on the
      weak-z stencil (4.1, -1, -1, -1, -1, -0.05, -0.05), the isotropic one and the strong-z one
      (2.2, -0.05, -0.05, -0.05, -0.05, -1, -1), for six sides: point V-cycles, PCG on the point cycle, z-line
      V-cycles (all three on the full-coarsening grid), and on the XY grid z-line V-cycles, AUTO V-cycles and PCG on
      the AUTO cycle. Iteration cap 150. f: seeded standard normal on the interior. Each case: the two grids, one
      untimed run of every side first, then `rounds` alternations; median of the rounds. A side that does not reach
      the tolerance in its cap is reported with the reduction it did reach. Then, on a third grid created under
      GS_METRICS=1, the device time per level and cycle of XY + AUTO (which level dominates).
  (b) per-launch times of the three XY kernels at 511 x 511 x 511 and 512 x 512 x 512 on seeded noise (the unit
      stencil, so that gs_residual_restrict runs k_rr2), events around
      single launches, alternated launch by launch with gs_residual_restrict (k_rr2; aligned sizes only),
      gs_residual_restrict_pa, gs_prolong_add (aligned only) and gs_prolong_add_pa: TB/s of each launcher's
      algorithmic bytes per fine point and the fused XY kernel's rate over gs_residual_restrict_pa's and k_rr2's.
--small: 63^3 / 127^3 and 127 / 128 instead (a functional check of the tool, not a measurement).
Writes <out>/semi_timing.json and <out>/summary.md and prints the JSON."""
import argparse
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "gpu-solve_amd"))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import gpusolve as gsv  # noqa: E402
from gpusolve.devfield import DevField  # noqa: E402
from fmg_timing import median  # noqa: E402
from pcg_timing import timed  # noqa: E402
from zline_timing import ISO, STRONGZ, normal  # noqa: E402

WEAKZ = [4.1, -1.0, -1.0, -1.0, -1.0, -0.05, -0.05]
F_FIELD = 3  # gpusolve.FIELDS["f"]
CAP = 150
# (key, grid, smoother, solver)
SIDES = [("point_vcycle", "xyz", "jacobi", gsv.HipSolver.solve), ("point_pcg", "xyz", "jacobi", gsv.HipSolver.pcg),
         ("full_zline", "xyz", "zline", gsv.HipSolver.solve), ("xy_zline", "xy", "zline", gsv.HipSolver.solve),
         ("xy_auto", "xy", "auto", gsv.HipSolver.solve), ("xy_auto_pcg", "xy", "auto", gsv.HipSolver.pcg)]
EXISTING = ("point_vcycle", "point_pcg", "full_zline")


def params(n, stencil):
    return gsv.GridParams(maxiter=CAP, tol=1e-8, gridDim=(n, n, n), mode=gsv.GS_LINEAR, preSmoothing=2, postSmoothing=2,
                          stencil=gsv.Stencil(stencil))


def set_rhs(g, rhs):
    geom = g.getLevel(0).geom
    assert (geom.ldy, geom.ldz) == (rhs.ldy, rhs.ldz)
    rc = gsv.kernels().gs_copy(gsv.driver().gs_grid_field(g.handle, 0, F_FIELD), rhs.ptr, rhs.span, g.stream())
    assert rc == 0, rc
    g.sync()


def level_times(n, stencil, rhs):
    """Device ms per level and cycle of XY + AUTO (the per-level clock: an unpipelined solve on a grid of its own)."""
    old = os.environ.get("GS_METRICS")
    os.environ["GS_METRICS"] = "1"
    try:
        with gsv.HipGridData(params(n, stencil), coarsen="xy") as g:
            set_rhs(g, rhs)
            g.set_smoother("auto")
            gsv.HipSolver.solve(g)
            nl = g.numLevels()
            lv = (C.c_double * nl)()
            line = C.create_string_buffer(4096)
            if gsv.driver().gs_grid_metrics(g.handle, line, 4096, lv, nl):
                raise gsv.GpuSolveError(gsv.driver().gs_last_error().decode())
            return {"levels": [list(g.getLevel(l).levelDim) for l in range(nl)],
                    "smoother": [g.level_smoother(l) for l in range(nl)], "ms_per_cycle": [float(x) for x in lv]}
    finally:
        if old is None:
            os.environ.pop("GS_METRICS", None)
        else:
            os.environ["GS_METRICS"] = old


def solve_case(name, n, stencil, rounds, rhs):
    out = {"case": name, "n": n, "stencil": stencil, "tol": 1e-8, "iteration_cap": CAP}
    p = params(n, stencil)
    with gsv.HipGridData(p, coarsen="xyz") as gz, gsv.HipGridData(p, coarsen="xy") as gy:
        grids = {"xyz": gz, "xy": gy}
        for g in grids.values():
            set_rhs(g, rhs)
        ms = {k: [] for k, _, _, _ in SIDES}
        hist, refused = {}, {}
        for r in range(rounds + 1):  # round 0 is untimed: first launches, PCG's allocation, the factors' upload
            for key, which, smoother, fn in SIDES:
                if key in refused:
                    continue
                g = grids[which]
                try:
                    g.set_smoother(smoother)
                except gsv.GpuSolveError as e:  # (z-line sweeps on a stencil the line solve refuses)
                    refused[key] = str(e)
                    continue
                t, hist[key] = timed(g, fn)
                if r > 0:
                    ms[key].append(t)
        out["xy_auto_levels"] = " ".join("Z" if gy.level_smoother(l) == "zline" else "J" for l in range(gy.numLevels()))
    for key, _, _, _ in SIDES:
        if key in refused:
            out[key] = {"refused": refused[key]}
            continue
        h = hist[key]
        it = len(h) - 1
        out[key] = {"ms_rounds": ms[key], "ms": median(ms[key]), "iterations": it, "reached": h[-1] <= h[0] * 1e-8,
                    "reduction": h[-1] / h[0], "ms_per_iteration": median(ms[key]) / max(it, 1),
                    "mean_factor": (h[-1] / h[0]) ** (1.0 / max(it, 1)), "history": h}
    done = [k for k in EXISTING if "ms" in out[k] and out[k]["reached"]]
    best = min(done, key=lambda k: out[k]["ms"]) if done else None
    out["best_existing"] = best
    if best and out["xy_auto"]["reached"]:
        out["best_existing_over_xy_auto_time"] = out[best]["ms"] / out["xy_auto"]["ms"]
    out["xy_auto_level_ms"] = level_times(n, stencil, rhs)
    return out


class Tables:
    """Device copies of one transition's tables (gpusolve.transfer_axis): axes = 3 for the _pa launchers, 2 for _xy."""

    def __init__(self, fine, axes):
        self.keep, self.abi = [], gsv.gs_transfer_tables()
        for a in range(axes):
            T = gsv.transfer_axis(fine[a])
            self.abi.nf[a], self.abi.nc[a] = fine[a], fine[a] // 2
            for key in ("pj", "pt", "rlo", "rcnt", "rw"):
                t = torch.from_numpy(np.ascontiguousarray(T[key]).reshape(-1)).cuda()
                self.keep.append(t)
                getattr(self.abi, key)[a] = t.data_ptr()
        if axes == 2:
            self.abi.nf[2] = self.abi.nc[2] = fine[2]


def kernels(n, launches):
    k, t, sm = gsv.kernels(), gsv.transfer(), gsv.semi()
    m = n // 2
    aligned = n == 2 * m + 1
    v, f = normal(DevField(n, n, n), 2), normal(DevField(n, n, n), 3)
    c3, cxy = normal(DevField(m, m, m), 4), normal(DevField(m, m, n), 5)
    o3, oxy = DevField(m, m, m), DevField(m, m, n)
    L, L3, Lxy = v.level(1.0 / (n + 1)), c3.level(1.0 / (m + 1)), cxy.level(1.0 / (m + 1))
    S = gsv.Stencil(ISO).to_abi()  # (the unit stencil: gs_residual_restrict then runs k_rr2, the yardstick)
    T3, T2 = Tables((n, n, n), 3), Tables((n, n, n), 2)
    st = torch.cuda.current_stream()
    s = st.cuda_stream
    B = C.byref
    # name: (algorithmic bytes per fine point, call)
    runs = {
        "gs_residual_restrict_xy": (18.0, lambda: sm.gs_residual_restrict_xy(B(S), B(L), v.ptr, f.ptr, oxy.ptr, B(Lxy), B(T2.abi), s)),
        "gs_restrict_xy": (10.0, lambda: sm.gs_restrict_xy(f.ptr, B(L), oxy.ptr, B(Lxy), B(T2.abi), s)),
        "gs_prolong_add_xy": (18.0, lambda: sm.gs_prolong_add_xy(cxy.ptr, B(Lxy), v.ptr, B(L), B(T2.abi), s)),
        "gs_residual_restrict_pa": (17.0, lambda: t.gs_residual_restrict_pa(B(S), B(L), 0, 1.0, v.ptr, f.ptr, None, o3.ptr, B(L3), B(T3.abi), s)),
        "gs_prolong_add_pa": (17.0, lambda: t.gs_prolong_add_pa(c3.ptr, None, B(L3), v.ptr, B(L), B(T3.abi), s)),
    }
    if aligned:
        runs["gs_residual_restrict"] = (17.0, lambda: k.gs_residual_restrict(B(S), B(L), 0, 1.0, v.ptr, f.ptr, None, o3.ptr, None, B(L3), s))
        runs["gs_prolong_add"] = (17.0, lambda: k.gs_prolong_add(c3.ptr, None, B(L3), v.ptr, B(L), s))
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
    pts = float(n) ** 3
    res = {"n": n, "launches": launches, "stencil": ISO}
    for name, (bpp, _) in runs.items():
        md = median(ms[name])
        res[name] = {"ms": md, "ms_launches": ms[name], "bytes_per_fine_point": bpp, "tbps": bpp * pts / md / 1e9}
    fx = res["gs_residual_restrict_xy"]["tbps"]
    res["fused_xy_rate_over_rr_pa"] = fx / res["gs_residual_restrict_pa"]["tbps"]
    if aligned:
        res["fused_xy_rate_over_k_rr2"] = fx / res["gs_residual_restrict"]["tbps"]
    res["prolong_add_xy_rate_over_pa"] = res["gs_prolong_add_xy"]["tbps"] / res["gs_prolong_add_pa"]["tbps"]
    return res


def summary(res):
    lines = ["# XY semi-coarsening: timings (tools/semi_timing.py)", "",
             f"Device: {res['device']}; LINEAR, 2+2 sweeps, omega 0.8, tol 1e-8 from a zero iterate, cap {CAP} iterations; "
             f"median of {res['rounds']} alternated rounds, host wall ms.", "",
             "| case | " + " | ".join(k for k, _, _, _ in SIDES) + " | XY auto levels | best existing / XY auto |",
             "|---|" + "---|" * (len(SIDES) + 2)]
    for c in res["solves"]:
        cells = []
        for k, _, _, _ in SIDES:
            e = c[k]
            if "refused" in e:
                cells.append("refused")
            elif e["reached"]:
                cells.append(f"{e['ms']:.1f} ms ({e['iterations']})")
            else:
                cells.append(f"not reached: {e['reduction']:.1e} in {e['iterations']} ({e['ms']:.1f} ms)")
        ratio = c.get("best_existing_over_xy_auto_time")
        lines.append(f"| {c['case']} | " + " | ".join(cells) + f" | {c['xy_auto_levels']} | " +
                     (f"{c['best_existing']}: {ratio:.2f}x" if ratio else "-") + " |")
    lines += ["", "XY + AUTO, device ms per level and cycle (GS_METRICS grid, unpipelined):", ""]
    for c in res["solves"]:
        lv = c["xy_auto_level_ms"]
        lines.append(f"- {c['case']}: " + ", ".join(f"L{l} {s[0].upper()} {x:.3f}" for l, (s, x) in
                                                    enumerate(zip(lv["smoother"], lv["ms_per_cycle"]))))
    lines += ["", "Per-launch times (events around single launches, alternated; TB/s of algorithmic bytes):", "",
              "| n | launcher | ms | B / fine point | TB/s |", "|---|---|---|---|---|"]
    for kr in res["kernels"]:
        for name, e in kr.items():
            if isinstance(e, dict):
                lines.append(f"| {kr['n']} | {name} | {e['ms']:.4f} | {e['bytes_per_fine_point']:.0f} | {e['tbps']:.3f} |")
        extra = f"; over k_rr2's {kr['fused_xy_rate_over_k_rr2']:.3f}" if "fused_xy_rate_over_k_rr2" in kr else ""
        lines.append(f"| {kr['n']} | fused XY rate over gs_residual_restrict_pa's | {kr['fused_xy_rate_over_rr_pa']:.3f}{extra} | | |")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--kernels-only", action="store_true", help="part (b) alone")
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "semi"))
    a = ap.parse_args()
    assert a.rounds >= 1 and torch.cuda.is_available()
    sizes = (63, 127) if a.small else (255, 511)
    res = {"device": torch.cuda.get_device_name(0), "build": gsv.build_info().split(":")[0], "smoothing": "2+2",
           "omega": 0.8, "mode": "LINEAR", "rounds": a.rounds, "solves": []}
    if not a.kernels_only:
        for n in sizes:
            rhs = normal(DevField(n, n, n), 1)
            for stencil, sname in ((WEAKZ, "WEAKZ"), (ISO, "ISO"), (STRONGZ, "STRONGZ")):
                res["solves"].append(solve_case(f"{sname} {n}^3", n, stencil, a.rounds, rhs))
    res["kernels"] = [kernels(n, 7) for n in ((127, 128) if a.small else (511, 512))]
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "semi_timing.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    with open(os.path.join(a.out, "summary.md"), "w") as fh:
        fh.write(summary(res))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
