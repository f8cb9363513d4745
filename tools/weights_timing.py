"""Per-sweep relaxation weights against the uniform omega on one GPU (DESIGN.md §4.8 quotes the result).

    python tools/weights_timing.py [--n 511] [--nonlinear-n 255] [--rounds 4] [--cycles 10] [--out profiles/weights]

One process. n^3 LINEAR 2+2, weights = gpusolve.chebyshev_weights(2) on both legs:
  - the residual history of `cycles` V-cycles from zero, uniform and weighted, and m: the number of uniform cycles
    that get under the weighted run's residual after 6 cycles;
  - the same two histories behind a full-multigrid start (HipSolver.fmg(grid, 1) with and without the weights);
  - `rounds` alternations of gs_grid_time_vcycles (the solve loop's V-cycle, `cycles` per round) with the weights
    cleared and set, on one grid: ms per V-cycle each way (the launches and the bytes are the same).
Then one NONLINEAR (FAS) grid of --nonlinear-n points per axis: both histories and ms per V-cycle, and from them the
time each way to the weighted run's 6-cycle residual. Writes <out>/weights_timing.json and prints it."""
import argparse
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "gpu-solve_amd"))

import torch  # noqa: E402

import gpusolve as gsv  # noqa: E402


def median(xs):
    s = sorted(xs)
    return s[len(s) // 2] if len(s) % 2 else 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2])


def history(p, w, fmg=False):
    """[initial, one norm per V-cycle]; fmg: [initial, FMG(1)'s residual, one norm per V-cycle after it]."""
    with gsv.HipGridData(p) as g:
        if w:
            g.set_weights(w, w)
        if not fmg:
            return gsv.HipSolver.solve(g)
        first = gsv.HipSolver.compResidual(g, 0)
        out = [first, gsv.HipSolver.fmg(g, 1)]
        for _ in range(int(p.maxiter)):
            out.append(gsv.HipSolver.vcycle(g))
        return out


def cycles_under(hist, target, first=1):
    """The first index >= first of hist whose residual is below target (None: never)."""
    return next((i for i, r in enumerate(hist) if i >= first and r < target), None)


def vcycle_ms(p, w, rounds, cycles):
    d = gsv.driver()
    out = {"uniform": [], "weighted": []}
    with gsv.HipGridData(p) as g:
        ms, last = C.c_double(), C.c_double()
        for kind in ("uniform", "weighted"):  # untimed: first launches of every kernel
            g.set_weights(w, w) if kind == "weighted" else g.clear_weights()
            assert d.gs_grid_time_vcycles(g.handle, 2, C.byref(ms), C.byref(last)) == 0, d.gs_last_error().decode()
        for _ in range(rounds):
            for kind in ("uniform", "weighted"):
                g.set_weights(w, w) if kind == "weighted" else g.clear_weights()
                rc = d.gs_grid_time_vcycles(g.handle, cycles, C.byref(ms), C.byref(last))
                assert rc == 0, d.gs_last_error().decode()
                out[kind].append(ms.value / cycles)
    return {k: {"rounds": v, "median": median(v), "spread": (max(v) - min(v)) / median(v)} for k, v in out.items()}


def case(n, mode, w, rounds, cycles, with_fmg):
    p = gsv.GridParams(maxiter=cycles, tol=0.0, gridDim=(n, n, n), mode=mode, preSmoothing=2, postSmoothing=2)
    res = {"n": n, "mode": {gsv.GS_LINEAR: "LINEAR", gsv.GS_NONLINEAR: "NONLINEAR"}[mode], "smoothing": "2+2",
           "weights": list(w)}
    res["uniform_history"] = history(p, None)
    res["weighted_history"] = history(p, w)
    target = res["weighted_history"][6]
    res["uniform_cycles_under_weighted_6"] = cycles_under(res["uniform_history"], target)
    if with_fmg:
        res["fmg_uniform_history"] = history(p, None, True)
        res["fmg_weighted_history"] = history(p, w, True)
        t = res["fmg_weighted_history"][1 + 6]  # FMG(1) and six V-cycles
        m = cycles_under(res["fmg_uniform_history"], t, 2)
        res["fmg_uniform_cycles_under_fmg_weighted_6"] = None if m is None else m - 1
    res["vcycle_ms"] = vcycle_ms(p, w, rounds, cycles)
    u, wt = res["vcycle_ms"]["uniform"]["median"], res["vcycle_ms"]["weighted"]["median"]
    m = res["uniform_cycles_under_weighted_6"]
    res["ms_to_weighted_6_residual"] = {"residual": target, "weighted": 6 * wt, "uniform": None if m is None else m * u}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=511)
    ap.add_argument("--nonlinear-n", type=int, default=255)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--cycles", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "weights"))
    a = ap.parse_args()
    assert a.rounds >= 1 and a.cycles >= 6 and torch.cuda.is_available()
    w = gsv.chebyshev_weights(2)
    res = {"device": torch.cuda.get_device_name(0), "build": gsv.build_info().split(":")[0],
           "linear": case(a.n, gsv.GS_LINEAR, w, a.rounds, a.cycles, True),
           "nonlinear": case(a.nonlinear_n, gsv.GS_NONLINEAR, w, a.rounds, a.cycles, False)}
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "weights_timing.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
