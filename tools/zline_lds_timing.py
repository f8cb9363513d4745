"""The LDS instance of the z-line sweep (k_zline_lds) against other builds of libgpusolve_line.so on
one GPU (profiles/zline_lds/summary.md quotes the results).

    python tools/zline_lds_timing.py --sweeps [--lib NAME=PATH ...] [--shapes 31x31x511,...] [--launches 9]
    python tools/zline_lds_timing.py --solves [--pkg DIR] [--rounds 3] [--small]
    ... [--out profiles/zline_lds] [--tag NAME]

--sweeps: per-launch times of gs_zline_sweep and of its zero-iterate form, events around single launches, alternated
  launch by launch between this tree's library ("this") and every --lib (another build of libgpusolve_line.so: the
  parent commit's, or a scratch build with another selection), all loaded into one process. Seeded noise, the
  strong-z stencil, omega 0.8. Default shapes: the five deepest line levels of a 511^3 XY hierarchy (31^2, 15^2, 7^2,
  3^2, 1^2 columns of 511 planes) and 31^2 x 255. Per shape and form: each build's instance name, its median and
  every launch's ms, and whether "this" was the fastest in every alternated round. The first two rounds are warm-up.
--solves: tools/semi_timing.py's weak-z rows (time to reduce the residual by 10^8 at 255^3 and 511^3: point V-cycles,
  PCG on the point cycle, XY + z-line, XY + AUTO, PCG on the XY + AUTO cycle; alternated rounds in one process) and
  the per-level clock of XY + AUTO. --pkg names the directory that holds the `gpusolve` package to measure (its lib/
  beside it), so that a job can alternate processes of two builds.
Writes <out>/sweeps[_TAG].json or <out>/solves[_TAG].json and prints it."""
import argparse
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def early_pkg():
    """--pkg has to take effect before gpusolve is first imported (the other tools insert this tree's path)."""
    for i, a in enumerate(sys.argv):
        if a == "--pkg" and i + 1 < len(sys.argv):
            return os.path.abspath(sys.argv[i + 1])
        if a.startswith("--pkg="):
            return os.path.abspath(a[6:])
    return os.path.join(HERE, "..", "gpu-solve_amd")


sys.path.insert(0, early_pkg())
sys.path.insert(1, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import gpusolve as gsv  # noqa: E402
from gpusolve.devfield import DevField  # noqa: E402
import semi_timing  # noqa: E402
from fmg_timing import median  # noqa: E402
from zline_timing import STRONGZ, normal  # noqa: E402

SHAPES = [(31, 31, 511), (15, 15, 511), (7, 7, 511), (3, 3, 511), (1, 1, 511), (31, 31, 255)]


def sweep_shape(libs, shape, launches):
    nx, ny, nz = shape
    v, f = normal(DevField(nx, ny, nz), 2), normal(DevField(nx, ny, nz), 3)
    out = DevField(nx, ny, nz)
    L = v.level(1.0 / (ny + 1))
    S = gsv.Stencil(STRONGZ).to_abi()
    cp, den = np.zeros(nz + 2), np.zeros(nz + 2)
    assert libs["this"].gs_zline_factors(C.byref(S), nz, cp.ctypes.data_as(gsv._abi.dptr),
                                         den.ctypes.data_as(gsv._abi.dptr)) == 0
    tab = torch.from_numpy(np.concatenate([cp, den])).cuda()
    T = gsv.gs_zline_tables(tab.data_ptr(), tab.data_ptr() + 8 * (nz + 2), nz)
    st = torch.cuda.current_stream()
    s = st.cuda_stream
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    res = {"shape": list(shape), "launches": launches}
    for form, vin in (("gs_zline_sweep", v.ptr), ("gs_zline_sweep_zero", None)):
        ms = {name: [] for name in libs}
        ref = None
        torch.cuda.synchronize()
        for i in range(launches + 2):  # the first two rounds are warm-up
            for name, ln in libs.items():
                e0.record(st)
                rc = ln.gs_zline_sweep(C.byref(S), C.byref(L), 0.8, vin, out.ptr, f.ptr, C.byref(T), s)
                e1.record(st)
                assert rc == 0, (name, rc)
                e1.synchronize()
                if i >= 2:
                    ms[name].append(e0.elapsed_time(e1))
                if i == 0:  # every build computes the same words
                    got = out.zyx[1:-1, 1:-1, 1:nx + 1].clone()
                    if ref is None:
                        ref = got
                    assert torch.equal(got.view(torch.int64), ref.view(torch.int64)), (shape, form, name)
        entry = {name: {"instance": ln.gs_zline_kernel(C.byref(S), C.byref(L), int(vin is None)).decode(),
                        "ms": median(ms[name]), "ms_launches": ms[name]} for name, ln in libs.items()}
        others = [n for n in libs if n != "this"]
        entry["this_fastest_in_every_round"] = all(ms["this"][i] < ms[n][i] for n in others for i in range(launches))
        for n in others:
            entry[n]["ms_over_this_ms"] = entry[n]["ms"] / entry["this"]["ms"]
        res[form] = entry
    return res


def solves(rounds, small):
    semi_timing.SIDES = [s for s in semi_timing.SIDES if s[0] != "full_zline"]
    semi_timing.EXISTING = ("point_vcycle", "point_pcg")
    out = []
    for n in ((63, 127) if small else (255, 511)):
        rhs = normal(DevField(n, n, n), 1)
        out.append(semi_timing.solve_case(f"WEAKZ {n}^3", n, semi_timing.WEAKZ, rounds, rhs))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweeps", action="store_true")
    ap.add_argument("--solves", action="store_true")
    ap.add_argument("--lib", action="append", default=[], metavar="NAME=PATH")
    ap.add_argument("--pkg", default=None)
    ap.add_argument("--shapes", default=None, help="comma-separated NXxNYxNZ")
    ap.add_argument("--launches", type=int, default=9)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "zline_lds"))
    a = ap.parse_args()
    assert a.sweeps != a.solves and torch.cuda.is_available()
    res = {"device": torch.cuda.get_device_name(0), "build": gsv.build_info().split(":")[0],
           "libraries": os.path.relpath(os.path.dirname(gsv._abi.LINE_LIB), os.path.join(HERE, ".."))}
    if a.sweeps:
        libs = {"this": gsv.line()}
        for spec in a.lib:
            name, path = spec.split("=", 1)
            libs[name] = gsv._abi._load(os.path.abspath(path), gsv._abi.LINE_API)
        shapes = SHAPES if not a.shapes else [tuple(int(x) for x in s.split("x")) for s in a.shapes.split(",")]
        res["stencil"], res["omega"] = STRONGZ, 0.8
        res["sweeps"] = [sweep_shape(libs, shape, a.launches) for shape in shapes]
    else:
        res["rounds"] = a.rounds
        res["solves"] = solves(a.rounds, a.small)
    os.makedirs(a.out, exist_ok=True)
    name = ("sweeps" if a.sweeps else "solves") + (f"_{a.tag}" if a.tag else "") + ".json"
    with open(os.path.join(a.out, name), "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
