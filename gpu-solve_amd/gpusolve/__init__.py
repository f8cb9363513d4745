"""gpusolve — Python mirror of the GpuSolve-hip backend interface (MI355X, HIP, fp64).

Same names, argument meaning and error behaviour as the reference's C++ backend contract
(Bricktricker/gpu-solve):

    GridParams / Stencil          src/gridParams.h:7-47
    read_config                   src/main.cpp:32-85 (14-line config file)
    HipGridData(params)           CpuGridData(const GridParams&)      src/cpu/CpuGridData.cpp:15-79
    HipSolver.solve(grid)         CpuSolver::solve                    src/cpu/CpuSolver.cpp:12-43
    HipSolver.vcycle / jacobi / compResidual                          src/cpu/CpuSolver.cpp:45-180
    NewtonSolver.solve(grid)      NewtonSolver::solve                 src/cpu/NewtonSolver.cpp:10-44

Everything runs through libgpusolve_driver.so -> libgpusolve_hip.so (hand-written gfx950 kernels).
There is no CPU fallback: without the built libraries or a GPU the calls raise.
"""
import ctypes as C
from dataclasses import dataclass, field
from typing import List, Tuple

import numpy as np

from . import _abi
from ._abi import GS_LINEAR, GS_MAX_WEIGHTS, GS_NEWTON, GS_NEWTON_B, GS_NEWTON_G, GS_NONLINEAR, gs_level, gs_params, gs_stencil, kernels, driver, diag  # noqa: F401
from ._abi import GS_TRANSFER_POSITION, GS_TRANSFER_REFERENCE, gs_transfer_tables, transfer  # noqa: F401
from ._abi import GS_FMG_PROLONG_ALIGNED, GS_FMG_PROLONG_POSITION, gs_fmg_tables  # noqa: F401
from ._abi import GS_PCG_BREAKDOWN, krylov  # noqa: F401
from ._abi import GS_SMOOTHER_JACOBI, GS_SMOOTHER_ZLINE, gs_zline_tables, line  # noqa: F401
from ._abi import GS_COARSEN_XY, GS_COARSEN_XYZ, GS_SMOOTHER_AUTO, semi  # noqa: F401
from ._abi import GS_IO_EXPORT, GS_IO_F32, GS_IO_F64, GS_IO_IMPORT, io  # noqa: F401

CANONICAL_OFFSETS = [(0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]


class GpuSolveError(RuntimeError):
    """A backend failure; str() is what GpuSolve-hip prints after "Exception: "."""


@dataclass
class Stencil:
    values: List[float] = field(default_factory=lambda: [6.0, -1, -1, -1, -1, -1, -1])
    offsets: List[Tuple[int, int, int]] = field(default_factory=lambda: list(CANONICAL_OFFSETS))

    def to_abi(self) -> gs_stencil:
        s = gs_stencil()
        for i in range(7):
            s.s[i] = float(self.values[i])
            s.ox[i], s.oy[i], s.oz[i] = (int(o) for o in self.offsets[i])
        return s


@dataclass
class GridParams:
    LINEAR = GS_LINEAR
    NONLINEAR = GS_NONLINEAR
    NEWTON = GS_NEWTON

    maxiter: int = 10
    tol: float = 0.0
    gridDim: Tuple[int, int, int] = (31, 31, 31)
    mode: int = GS_LINEAR
    preSmoothing: int = 2
    postSmoothing: int = 2
    omega: float = 0.8
    gamma: float = 1.0
    stencil: Stencil = field(default_factory=Stencil)
    printProgress: bool = True

    @property
    def h(self) -> float:  # src/main.cpp:84
        return 1.0 / (self.gridDim[1] + 1)

    def to_abi(self) -> gs_params:
        p = gs_params()
        p.maxiter, p.tol = int(self.maxiter), float(self.tol)
        for i in range(3):
            p.dims[i] = int(self.gridDim[i])
        p.mode, p.pre, p.post = int(self.mode), int(self.preSmoothing), int(self.postSmoothing)
        p.omega, p.gamma = float(self.omega), float(self.gamma)
        p.stencil = self.stencil.to_abi()
        return p

    def config_text(self) -> str:
        st = self.stencil
        return "\n".join([str(self.maxiter), repr(float(self.tol)), *(str(d) for d in self.gridDim), str(self.mode),
                          str(self.preSmoothing), str(self.postSmoothing), repr(float(self.omega)),
                          repr(float(self.gamma)), " ".join(repr(float(v)) for v in st.values),
                          *(" ".join(str(o[a]) for o in st.offsets) for a in range(3))]) + "\n"


def parse_config(text: str) -> GridParams:
    """Parses the reference's 14-line config text (README.md:17-33) with the library's parser."""
    p = gs_params()
    rc = driver().gs_parse_config(text.encode(), C.byref(p))
    if rc == 1:
        raise ValueError("Invalid mode")
    if rc == 2:
        raise ValueError("Invalid stencil offset (must be -1, 0 or 1)")
    st = Stencil([p.stencil.s[i] for i in range(7)],
                 [(p.stencil.ox[i], p.stencil.oy[i], p.stencil.oz[i]) for i in range(7)])
    return GridParams(maxiter=p.maxiter, tol=p.tol, gridDim=tuple(p.dims), mode=p.mode, preSmoothing=p.pre,
                      postSmoothing=p.post, omega=p.omega, gamma=p.gamma, stencil=st)


def read_config(path: str) -> GridParams:
    with open(path) as f:
        return parse_config(f.read())


def _check(rc: int):
    if rc != 0:
        raise GpuSolveError(driver().gs_last_error().decode())


_TRANSFERS = {"reference": GS_TRANSFER_REFERENCE, "position": GS_TRANSFER_POSITION}
_FMG_PROLONGS = {"aligned": GS_FMG_PROLONG_ALIGNED, "position": GS_FMG_PROLONG_POSITION}
_SMOOTHERS = {"jacobi": GS_SMOOTHER_JACOBI, "zline": GS_SMOOTHER_ZLINE, "auto": GS_SMOOTHER_AUTO}
_COARSENINGS = {"xyz": GS_COARSEN_XYZ, "xy": GS_COARSEN_XY}
FIELDS = {"v": 0, "restV": 1, "newtonV": 2, "f": 3, "r": 4, "newtonF": 5}


@dataclass
class LevelInfo:
    levelDim: Tuple[int, int, int]
    h: float
    geom: gs_level


class HipGridData:
    """Device-resident level hierarchy (fields in HBM for the object's lifetime)."""

    def __init__(self, params: GridParams, coarsen: str = None):
        """coarsen: None (gs_grid_create: GS_COARSEN decides, xyz without it), "xyz", or "xy" — semi-coarsening for a
        weak z coupling: x and y halve per level, nz stays, every level has its own stencil (level_stencil) and the
        transfers do not touch z (include/gpusolve_semi.h). LINEAR single-GPU grids; GpuSolveError with the reason
        otherwise."""
        self.params = params
        self._abi_params = params.to_abi()
        if coarsen is None:
            self.handle = driver().gs_grid_create(C.byref(self._abi_params))
        else:
            if coarsen not in _COARSENINGS:
                raise ValueError(f"coarsen must be one of {sorted(_COARSENINGS)}")
            self.handle = driver().gs_grid_create_coarsen(C.byref(self._abi_params), _COARSENINGS[coarsen])
        if not self.handle:
            raise GpuSolveError(driver().gs_last_error().decode())
        # the device the grid lives on (the current one at creation): load / store hold their tensors to it. The
        # HIP runtime is among the driver library's dependencies, so its symbols resolve through the handle.
        dev = C.c_int(-1)
        driver().hipGetDevice(C.byref(dev))
        self.device_index = dev.value

    def close(self):
        if getattr(self, "handle", None):
            driver().gs_grid_destroy(self.handle)
            self.handle = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def mode(self):
        return self.params.mode

    def numLevels(self) -> int:
        return driver().gs_grid_num_levels(self.handle)

    def getLevel(self, l: int) -> LevelInfo:
        g = gs_level()
        if driver().gs_grid_level(self.handle, l, C.byref(g)) != 0:
            raise IndexError(l)
        return LevelInfo((g.nx, g.ny, g.nz), g.h, g)

    def stream(self) -> int:
        return driver().gs_grid_stream(self.handle)

    def fmg_start_level(self) -> int:
        """The level HipSolver.fmg starts on; 0 when full multigrid is not applicable to this grid."""
        return driver().gs_grid_fmg_start_level(self.handle)

    def set_weights(self, pre, post):
        """Per-sweep relaxation weights: on every level the k-th pre-smoothing sweep of each V-cycle takes pre[k] and
        the k-th post-smoothing sweep post[k] instead of omega (the coarsest level: pre, then post). len(pre) /
        len(post) must equal the grid's preSmoothing / postSmoothing (each at most GS_MAX_WEIGHTS) and every weight
        be finite, else GpuSolveError and the grid is unchanged. Equal weights give the unweighted solve bit for bit.
        HipSolver.jacobi (stand-alone sweeps) keeps omega."""
        pre, post = [float(w) for w in pre], [float(w) for w in post]
        a, b = (C.c_double * max(1, len(pre)))(*pre), (C.c_double * max(1, len(post)))(*post)
        _check(driver().gs_grid_set_weights(self.handle, a, len(pre), b, len(post)))

    def clear_weights(self):
        """Back to the grid's omega for every sweep."""
        _check(driver().gs_grid_set_weights(self.handle, None, 0, None, 0))

    @property
    def weights(self):
        """(pre, post) tuples of the per-sweep weights in force (set_weights or GS_OMEGAS), or None."""
        npre, npost = int(self.params.preSmoothing), int(self.params.postSmoothing)
        a, b = (C.c_double * max(1, npre))(), (C.c_double * max(1, npost))()
        if not driver().gs_grid_get_weights(self.handle, a, b):
            return None
        return tuple(a[:npre]), tuple(b[:npost])

    def set_transfer(self, mode: str):
        """The grid transfers of the V-cycle: "reference" (the default: the reference's index-aligned restrict /
        interpolate on every transition) or "position" (the position-aware operators of include/gpusolve_transfer.h
        on every transition that is not aligned, so that even sizes such as 512^3 converge; aligned transitions, and
        so grids of sizes 2^k - 1, are unchanged bit for bit). GpuSolveError, with nothing changed, on a Z-slab grid."""
        if mode not in _TRANSFERS:
            raise ValueError(f"transfer must be one of {sorted(_TRANSFERS)}")
        _check(driver().gs_grid_set_transfer(self.handle, _TRANSFERS[mode]))

    @property
    def transfer(self) -> str:
        """The transfer mode in force (set_transfer or GS_TRANSFER): "reference" or "position"."""
        m = driver().gs_grid_get_transfer(self.handle)
        return next(k for k, v in _TRANSFERS.items() if v == m)

    def set_smoother(self, mode: str):
        """The smoother of every sweep: "jacobi" (the default: damped point Jacobi) or "zline" (each sweep solves every
        z-column's tridiagonal system exactly and stays Jacobi across columns: include/gpusolve_line.h) — for stencils
        whose z weights dominate, where point Jacobi V-cycles stall; no gain on an isotropic stencil or a weak z axis.
        solve, vcycle, vcycle_from, jacobi, fmg and pcg follow it. GpuSolveError, with nothing changed, on a grid that
        is not LINEAR, on a Z-slab grid, and for a stencil gs_zline_supported refuses. "auto" chooses per level: z-line
        sweeps where the level stencil's largest |z weight| exceeds its largest |x / y weight|, the point path
        otherwise (level_smoother) — all or nothing on an "xyz" grid, the point kernels on the fine levels and lines
        below on an "xy" grid."""
        if mode not in _SMOOTHERS:
            raise ValueError(f"smoother must be one of {sorted(_SMOOTHERS)}")
        _check(driver().gs_grid_set_smoother(self.handle, _SMOOTHERS[mode]))

    @property
    def smoother(self) -> str:
        """The smoother in force (set_smoother or GS_SMOOTHER): "jacobi", "zline" or "auto"."""
        m = driver().gs_grid_get_smoother(self.handle)
        return next(k for k, v in _SMOOTHERS.items() if v == m)

    @property
    def coarsen(self) -> str:
        """The coarsening the grid was created with: "xyz" or "xy"."""
        m = driver().gs_grid_get_coarsen(self.handle)
        return next(k for k, v in _COARSENINGS.items() if v == m)

    def level_stencil(self, level: int) -> Stencil:
        """The stencil level `level` runs with: the configuration's on an "xyz" grid, the re-discretised one
        (gs_semi_level_stencil) on an "xy" grid."""
        s = gs_stencil()
        if driver().gs_grid_level_stencil(self.handle, level, C.byref(s)) != 0:
            raise IndexError(level)
        return Stencil([float(x) for x in s.s], [(s.ox[i], s.oy[i], s.oz[i]) for i in range(7)])

    def level_smoother(self, level: int) -> str:
        """"zline" where level `level` runs z-line sweeps, "jacobi" where it runs the point path."""
        r = driver().gs_grid_level_smoother(self.handle, level)
        if r < 0:
            raise IndexError(level)
        return "zline" if r else "jacobi"

    def set_fmg_prolong(self, mode: str):
        """Full multigrid's prolongation: "aligned" (the default: HipSolver.fmg needs sizes 2^k - 1) or "position"
        (FMG starts at the coarsest level of every LINEAR / NONLINEAR single-GPU grid; transitions that are not
        aligned take the tricubic prolongation by position, gs_fmg_prolong_pa, and need set_transfer("position");
        aligned transitions, and so grids of sizes 2^k - 1, are unchanged bit for bit)."""
        if mode not in _FMG_PROLONGS:
            raise ValueError(f"fmg_prolong must be one of {sorted(_FMG_PROLONGS)}")
        _check(driver().gs_grid_set_fmg_prolong(self.handle, _FMG_PROLONGS[mode]))

    @property
    def fmg_prolong(self) -> str:
        """The FMG prolongation in force (set_fmg_prolong or GS_FMG_PROLONG): "aligned" or "position"."""
        m = driver().gs_grid_get_fmg_prolong(self.handle)
        return next(k for k, v in _FMG_PROLONGS.items() if v == m)

    def level_aligned(self, level: int) -> bool:
        """Whether the transition from `level` to `level + 1` is aligned (fine n = 2 coarse n + 1 on all three axes:
        the reference's transfers are exact there and POSITION mode changes nothing)."""
        r = driver().gs_grid_level_aligned(self.handle, level)
        if r < 0:
            raise IndexError(level)
        return bool(r)

    def pcg_supported(self) -> bool:
        """Whether HipSolver.pcg can run on this grid as it is configured now (LINEAR, one GPU, a symmetric stencil
        and a symmetric cycle: pre = post >= 1, post weights a permutation of the pre weights, POSITION transfers
        where a transition is not aligned). False leaves the reason in pcg_refusal."""
        ok = driver().gs_grid_pcg_supported(self.handle) == 1
        self.pcg_refusal = None if ok else driver().gs_last_error().decode()
        return ok

    def pcg_record(self):
        """The last HipSolver.pcg run's scalars, one dict per iteration it started (a run that broke down includes the
        iteration that did): rz = r.z and beta as that iteration's direction used them, pq = p.q, alpha = rz / pq,
        rr = the new r.r, flag (0, or GS_PCG_BAD_PQ | GS_PCG_BAD_RZ | GS_PCG_BAD_RR)."""
        n = driver().gs_grid_pcg_record(self.handle, None, 0)
        if n < 0:
            raise GpuSolveError(driver().gs_last_error().decode())
        buf = (C.c_double * max(1, 6 * n))()
        driver().gs_grid_pcg_record(self.handle, buf, n)
        keys = ("rz", "pq", "alpha", "beta", "rr", "flag")
        return [dict(zip(keys, buf[6 * k:6 * k + 6])) for k in range(n)]

    def field(self, level: int, name: str) -> np.ndarray:
        """Copy of a padded field as a dense array indexed [x][y][z] (the reference's axis order)."""
        g = self.getLevel(level).geom
        host = np.empty((g.nz + 2, g.ny + 2, g.nx + 2), dtype=np.float64)
        _check(driver().gs_grid_download(self.handle, level, FIELDS[name], host.ctypes.data_as(_abi.dptr)))
        return host.transpose(2, 1, 0)

    def set_field(self, level: int, name: str, arr_xyz: np.ndarray):
        g = self.getLevel(level).geom
        host = np.ascontiguousarray(np.asarray(arr_xyz, dtype=np.float64).transpose(2, 1, 0))
        assert host.shape == (g.nz + 2, g.ny + 2, g.nx + 2)
        _check(driver().gs_grid_upload(self.handle, level, FIELDS[name], host.ctypes.data_as(_abi.dptr)))

    def _io_call(self, name, t, level, scale, order):
        """Checks a tensor against a field of `level` (ValueError before any driver call) and returns gs_grid_import's
        / gs_grid_export's arguments after the grid handle: the tensor's own strides, by grid axis, through `order`."""
        import torch

        if name not in FIELDS:
            raise ValueError(f"field must be one of {sorted(FIELDS)}")
        if not isinstance(order, str) or sorted(order) != ["x", "y", "z"]:
            raise ValueError('order must be a permutation of "xyz" naming the tensor\'s index order')
        if not 0 <= level < self.numLevels():
            raise ValueError(f"no level {level}")
        if not isinstance(t, torch.Tensor):
            raise ValueError("a torch tensor is needed")
        g = self.getLevel(level).geom
        n = {"x": g.nx, "y": g.ny, "z": g.nz}
        want = tuple(n[a] for a in order)
        if tuple(t.shape) != want:
            raise ValueError(f"shape {tuple(t.shape)}: level {level}'s interior in order {order!r} is {want}")
        if t.dtype not in (torch.float32, torch.float64):
            raise ValueError(f"dtype {t.dtype}: float32 or float64 is needed")
        if not t.is_cuda or t.device.index != self.device_index:
            raise ValueError(f"device {t.device}: the grid lives on cuda:{self.device_index}")
        stride = (_abi.i64 * 3)(*(t.stride(order.index(a)) for a in "xyz"))
        dtype = GS_IO_F32 if t.dtype == torch.float32 else GS_IO_F64
        user = torch.cuda.current_stream(t.device).cuda_stream
        return level, FIELDS[name], C.c_void_p(t.data_ptr()), dtype, stride, float(scale), C.c_void_p(user)

    def load(self, name: str, tensor, level: int = 0, scale: float = 1.0, order: str = "zyx"):
        """Field `name`'s interior on `level` = scale * tensor, on the device: no host copy, no synchronisation
        (gs_grid_import of include/gpusolve_driver.h). `order` is a permutation of "xyz" naming the tensor's index
        order — "zyx" is torch-natural ([z][y][x], x fastest), "xyz" is what field() returns — and the tensor's own
        strides go through it: views, slices, permuted and expanded (stride 0) tensors need no .contiguous(). float32
        or float64 on the grid's device, shaped as the level's interior in that order; ValueError otherwise, before any
        call. Ordered after the work on torch.cuda.current_stream(); the tensor may be reused there straight away."""
        _check(driver().gs_grid_import(self.handle, *self._io_call(name, tensor, level, scale, order)))

    def store(self, name: str, out=None, level: int = 0, scale: float = 1.0, order: str = "zyx", dtype=None):
        """out = scale * field `name`'s interior on `level`, on the device (gs_grid_export); returns `out`. Without
        `out` a contiguous tensor in `order` of `dtype` (float64 without one) is made on the grid's device; with it,
        its own strides are used (they must not make two points share an element) and `dtype`, if given, must be
        its. Work enqueued on torch.cuda.current_stream() after the call sees the result; nothing is synchronised."""
        import torch

        if not isinstance(order, str) or sorted(order) != ["x", "y", "z"]:
            raise ValueError('order must be a permutation of "xyz" naming the tensor\'s index order')
        if not 0 <= level < self.numLevels():
            raise ValueError(f"no level {level}")
        if out is None:
            g = self.getLevel(level).geom
            n = {"x": g.nx, "y": g.ny, "z": g.nz}
            dtype = torch.float64 if dtype is None else dtype
            if dtype not in (torch.float32, torch.float64):
                raise ValueError(f"dtype {dtype}: float32 or float64 is needed")
            out = torch.empty(tuple(n[a] for a in order), dtype=dtype, device=f"cuda:{self.device_index}")
        elif dtype is not None and isinstance(out, torch.Tensor) and out.dtype != dtype:
            raise ValueError(f"dtype {dtype} asked for, but out is {out.dtype}")
        _check(driver().gs_grid_export(self.handle, *self._io_call(name, out, level, scale, order)))
        return out

    def sync(self):
        _check(driver().gs_grid_sync(self.handle))

    def dump(self, path: str, level: int = 0, name: str = "v"):
        """Vector3::dump (src/cpu/Vector3.cpp:56-78) of a field: the plotter.py input format."""
        _check(driver().gs_grid_dump(self.handle, level, FIELDS[name], path.encode()))


def dump_write(arr_xyz: np.ndarray, path: str):
    """Vector3::dump text of a padded host array indexed [x][y][z] (the driver's writer)."""
    a = np.ascontiguousarray(np.asarray(arr_xyz, dtype=np.float64).transpose(2, 1, 0))
    px, py, pz = arr_xyz.shape
    _check(driver().gs_dump_write(a.ctypes.data_as(_abi.dptr), px, py, pz, path.encode()))


def read_dump(path: str) -> np.ndarray:
    """plotter.py's readFile (reference plotter.py:10-26): a dump back into an [x][y][z] array."""
    with open(path) as f:
        px, py, pz = (int(t) for t in f.readline().split())
        data = np.loadtxt(f, ndmin=2)
    out = np.zeros((px, py, pz))
    out[data[:, 0].astype(int), data[:, 1].astype(int), data[:, 2].astype(int)] = data[:, 3]
    return out


def analytic_error(mesh: np.ndarray) -> float:
    """Max |computed - u| over the mesh, u = (x-x^2)(y-y^2)(z-z^2) on linspace(0, 1, n) per axis
    (reference plotter.py:7-8, 28-31: the exact solution of the NONLINEAR / NEWTON problems)."""
    g = [np.linspace(0.0, 1.0, n) for n in mesh.shape]
    X, Y, Z = np.meshgrid(*g, indexing="ij")
    return float(np.abs(mesh - (X - X * X) * (Y - Y * Y) * (Z - Z * Z)).max())


class HipSolver:
    @staticmethod
    def solve(grid: HipGridData, print_progress: bool = False) -> List[float]:
        """Runs the solve for grid's mode (main.cpp:88-94 dispatch); returns the residual history."""
        cap = 4 * (int(grid.params.maxiter) + 2)
        hist = (C.c_double * cap)()
        n = C.c_int(0)
        _check(driver().gs_grid_solve(grid.handle, 1 if print_progress else 0, hist, cap, C.byref(n)))
        return list(hist[: min(n.value, cap)])

    @staticmethod
    def vcycle(grid: HipGridData) -> float:
        r = C.c_double()
        _check(driver().gs_grid_vcycle(grid.handle, C.byref(r)))
        return r.value

    @staticmethod
    def vcycle_from(grid: HipGridData, level: int):
        """One V-cycle rooted at `level` (its f and v as they stand); the levels above it are not touched."""
        _check(driver().gs_grid_vcycle_level(grid.handle, level))

    @staticmethod
    def fmg(grid: HipGridData, cycles_per_level: int = 1) -> float:
        """Full multigrid start: coarse right-hand sides restricted from level 0's f, the start level iterated from
        zero, every finer level from the tricubic prolongation of the level below, `cycles_per_level` V-cycles
        each. Overwrites v on every level; returns the level-0 residual norm. Raises GpuSolveError where FMG is
        not applicable (sizes other than 2^k - 1 unless grid.set_fmg_prolong("position"), NEWTON mode, Z-slab
        grids, cycles_per_level < 1)."""
        r = C.c_double()
        _check(driver().gs_grid_fmg(grid.handle, cycles_per_level, C.byref(r)))
        return r.value

    @staticmethod
    def pcg(grid: HipGridData, print_progress: bool = False) -> List[float]:
        """Conjugate gradients preconditioned by one V-cycle, from level 0's iterate as it stands (an upload or a
        preceding fmg is honoured), with the grid's maxiter and tol and solve's stopping rule; returns the residual
        history [||f - A x0||, then one norm per iteration]. LINEAR single-GPU grids whose cycle is symmetric
        (grid.pcg_supported()); GpuSolveError with nothing touched otherwise. A breakdown (p.q or r.z not a positive
        finite number: a zero right-hand side, or convergence to the last bit) ends the run cleanly with the last
        complete iteration's x; grid.pcg_breakdown says whether that happened."""
        cap = int(grid.params.maxiter) + 2
        hist = (C.c_double * cap)()
        n = C.c_int(0)
        rc = driver().gs_grid_pcg(grid.handle, 1 if print_progress else 0, hist, cap, C.byref(n))
        if rc not in (0, GS_PCG_BREAKDOWN):
            _check(rc)
        grid.pcg_breakdown = rc == GS_PCG_BREAKDOWN
        return list(hist[: min(n.value, cap)])

    @staticmethod
    def jacobi(grid: HipGridData, level: int, sweeps: int):
        _check(driver().gs_grid_jacobi(grid.handle, level, sweeps))

    @staticmethod
    def compResidual(grid: HipGridData, level: int) -> float:
        r = C.c_double()
        _check(driver().gs_grid_residual_norm(grid.handle, level, C.byref(r)))
        return r.value


class NewtonSolver:
    @staticmethod
    def solve(grid: HipGridData, print_progress: bool = False) -> List[float]:
        if grid.mode != GS_NEWTON:
            raise ValueError("NewtonSolver needs mode NEWTON")
        return HipSolver.solve(grid, print_progress)


def chebyshev_weights(nu: int, lo: float = 1.0 / 3.0, hi: float = 2.0) -> Tuple[float, ...]:
    """The nu Chebyshev relaxation weights on [lo, hi], w_k = 1 / ((hi+lo)/2 + (hi-lo)/2 cos(pi (2k-1) / (2 nu))):
    prod (1 - w_k x) is the polynomial of least maximum on [lo, hi] among those that are 1 at 0. The default
    interval is the high-frequency band of D^-1 A for the 7-point operator. Pure host code (no device needed)."""
    nu = int(nu)
    out = (C.c_double * max(1, nu))()
    _check(driver().gs_chebyshev_weights(nu, float(lo), float(hi), out))
    return tuple(out[:nu])


def parse_omegas(text: str, pre: int, post: int) -> Tuple[Tuple[float, ...], Tuple[float, ...]]:
    """GS_OMEGAS's value ("w1,w2/w3,w4" or "cheb") for a grid of pre / post smoothing sweeps, as (pre, post)
    weights, with the library's parser; GpuSolveError on a malformed value or a count mismatch. No device needed."""
    out = (C.c_double * max(1, pre + post))()
    _check(driver().gs_parse_omegas(text.encode(), int(pre), int(post), out))
    return tuple(out[:pre]), tuple(out[pre:pre + post])


def transfer_axis(nf: int):
    """The position-aware transfer tables of one axis for fine nf -> coarse nf // 2 (gs_transfer_axis; pure host
    code, no device needed): dict of pj (int32, nf + 2), pt (nf + 2), rlo, rcnt (int32, nf // 2 + 2) and rw
    ((nf // 2 + 2, 4)). ValueError for nf < 2."""
    nf = int(nf)
    nc = nf // 2
    pj, pt = np.zeros(max(nf, 0) + 2, np.int32), np.zeros(max(nf, 0) + 2)
    rlo, rcnt, rw = np.zeros(nc + 2, np.int32), np.zeros(nc + 2, np.int32), np.zeros((nc + 2, 4))
    i32 = C.POINTER(C.c_int32)
    rc = transfer().gs_transfer_axis(nf, nc, pj.ctypes.data_as(i32), pt.ctypes.data_as(_abi.dptr),
                                     rlo.ctypes.data_as(i32), rcnt.ctypes.data_as(i32), rw.ctypes.data_as(_abi.dptr))
    if rc:
        raise ValueError(kernels().gs_strerror(rc).decode())
    return {"pj": pj, "pt": pt, "rlo": rlo, "rcnt": rcnt, "rw": rw}


def fmg_axis(nf: int):
    """The tables of full multigrid's prolongation by position for one axis, fine nf -> coarse nf // 2 (gs_fmg_axis;
    pure host code, no device needed): dict of cj (int32, nf + 2: the first of the K = 4 coarse nodes, K = 3 where
    nf // 2 == 1) and cw ((nf + 2, 4): their Lagrange weights). ValueError for nf < 2."""
    nf = int(nf)
    cj, cw = np.zeros(max(nf, 0) + 2, np.int32), np.zeros((max(nf, 0) + 2, 4))
    rc = transfer().gs_fmg_axis(nf, nf // 2, cj.ctypes.data_as(C.POINTER(C.c_int32)), cw.ctypes.data_as(_abi.dptr))
    if rc:
        raise ValueError(kernels().gs_strerror(rc).decode())
    return {"cj": cj, "cw": cw}


def field_layout(nx: int, ny: int, nz: int):
    """(ldy, ldz, alloc_elems, origin_offset) of include/gpusolve_hip.h's pitched layout."""
    a, b, c, d = (C.c_int64() for _ in range(4))
    rc = kernels().gs_field_layout(nx, ny, nz, C.byref(a), C.byref(b), C.byref(c), C.byref(d))
    if rc:
        raise ValueError(kernels().gs_strerror(rc).decode())
    return a.value, b.value, c.value, d.value


def build_info() -> str:
    return kernels().gs_build_info().decode()
