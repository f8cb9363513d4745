"""Device-side field import / export on the GPU (include/gpusolve_io.h): gs_io_import / gs_io_export
under the kernel ABI's layout contract for the field side and sentinel-filled torch storage for the external side,
and HipGridData.load / store through the driver against the upload / download path.

Tolerances: none. The header's arithmetic is one conversion and at most one multiply per point, which numpy restates
exactly; every word is compared as an integer. Driver histories and fields are compared bit for bit with the runs fed
through set_field / field: both feed the same kernels the same words."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import gpusolve as gsv  # noqa: E402
from gpusolve import _abi as A  # noqa: E402
from layout_field import LAYOUT_IDS, LayoutField, layouts  # noqa: E402

# degenerate, all-ragged; a row ending inside a 16-byte pair, one whole 128-point wave segment, the segment crossed by
# one; tile: one whole tile, ragged in both tile axes, ragged with a short x
SHAPES = [(1, 1, 1), (2, 3, 5), (127, 5, 3), (128, 4, 2), (129, 3, 2), (64, 2, 64), (65, 3, 66), (3, 66, 65)]
SENTINEL = {np.float64: 0x7FF8_0E57_0000_0D44, np.float32: 0x7FC0_5E47}
NAN64, NAN32 = 0x7FF8_0246_8000_0000, 0x7FC1_2345  # payloads whose leading bits survive either conversion
TIE_SCALE = 0.5
TIES = (2.0 + 2.0 ** -23, 2.0 + 3 * 2.0 ** -23)  # 0.5 x: 1 + 2^-24, 1 + 3 2^-24 — halfway between two floats
SCALES = (1.0, -0.375, TIE_SCALE)
NPT = {A.GS_IO_F64: np.float64, A.GS_IO_F32: np.float32}
TT = {A.GS_IO_F64: torch.float64, A.GS_IO_F32: torch.float32}
IW = {np.float64: np.int64, np.float32: np.int32}


@pytest.fixture(autouse=True)
def needs_gpu():
    assert torch.cuda.is_available(), "GPU tests need a GPU (no CPU fallback exists)"


def st():
    return torch.cuda.current_stream().cuda_stream


def sid(shape):
    return "x".join(str(n) for n in shape)


def words(a):
    a = np.ascontiguousarray(a)
    return a.view(IW[a.dtype.type])


def same(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    ne = words(a) != words(b)
    assert not ne.any(), f"{what}: {int(ne.sum())} words differ, first at {tuple(np.argwhere(ne)[0])}"


def stride_classes(nx, ny, nz):
    """name -> (element strides by grid axis, instance family, import only)."""
    return {
        "zyx": ((1, nx, nx * ny), "rows", False),
        "row pitch nx+3": ((1, nx + 3, (nx + 3) * ny), "rows", False),
        "xyz": ((ny * nz, nz, 1), "tile", False),
        "sy = 1": ((ny * nz, 1, ny), "tile", False),
        "sx = 2": ((2, 2 * nx + 2, (2 * nx + 2) * ny + 4), "gen", False),
        "sz = 0": ((1, nx, 0), "rows", True),
    }


def index(shape, s):
    """Element offsets of the interior points, indexed [x][y][z]."""
    x, y, z = np.meshgrid(*(np.arange(n, dtype=np.int64) for n in shape), indexing="ij")
    return x * s[0] + y * s[1] + z * s[2]


@functools.lru_cache(maxsize=None)
def field_values(shape):
    """The export source: a padded [x][y][z] array, ring and interior non-zero noise; read-only."""
    rng = np.random.default_rng(7 + shape[0] + 1000 * shape[1] + 1000003 * shape[2])
    a = rng.uniform(0.5, 3.0, tuple(n + 2 for n in shape)) * np.where(rng.random(tuple(n + 2 for n in shape)) < 0.5, -1, 1)
    a.setflags(write=False)
    return a


def salted(vals, scale, nan_word):
    """`vals` (flat, writable) with the case's special words: a NaN payload at scale 1.0, the ties at TIE_SCALE."""
    if scale == 1.0:
        vals.view(IW[vals.dtype.type])[vals.size // 2] = nan_word
    elif scale == TIE_SCALE and vals.dtype == np.float64:
        vals[0], vals[-1] = TIES[0], TIES[1]
    return vals


def expect_import(src, scale):
    d = src.astype(np.float64)
    return d if scale == 1.0 else np.float64(scale) * d


def expect_export(f, scale, npt):
    p = f if scale == 1.0 else np.float64(scale) * f
    return p.astype(npt)


def test_tie_values_are_ties():
    """The chosen scale and field values do land halfway between two floats, and round to even."""
    ulp = 2.0 ** -23
    for v, lo, want in zip(TIES, (1.0, 1.0 + ulp), (1.0, 1.0 + 2 * ulp)):
        p = TIE_SCALE * v
        assert float(np.float32(lo)) == lo and p - lo == (lo + ulp) - p == ulp / 2
        assert float(np.float64(p).astype(np.float32)) == want


@pytest.mark.parametrize("layout", LAYOUT_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_kernels_word_for_word(shape, layout):
    """Every stride class, dtype, direction, scale and base alignment: the written words equal numpy's, exactly the
    documented set is written, and the source is untouched."""
    lib = gsv.io()
    lay = layouts(*shape)[layout]
    dst = LayoutField(*shape, lay.ldy, lay.ldz, lay.phase_out)
    src = LayoutField(*shape, lay.ldy, lay.ldz, lay.phase_in)
    L = dst.level(1.0 / (shape[1] + 1))
    interior = dst.interior_mask()
    rng = np.random.default_rng(11)
    for cls, (s, family, import_only) in stride_classes(*shape).items():
        idx = index(shape, s)
        sabi = (A.i64 * 3)(*s)
        for dtype in (A.GS_IO_F64, A.GS_IO_F32):
            npt = NPT[dtype]
            name = lib.gs_io_kernel(A.GS_IO_IMPORT, dtype, C.byref(L), sabi).decode()
            assert name.startswith(f"k_io_{family}<") or shape == (1, 1, 1), (cls, name)
            for off in (0, 1):
                n = off + int(idx.max()) + 1 + 8
                for scale in SCALES:
                    what = f"{cls} dtype {dtype} base +{off} scale {scale}"
                    # ---- import: the whole storage is data (a broadcast reads some of it many times) -------------
                    host = salted(rng.uniform(-2.0, 2.0, n).astype(npt), scale, NAN64 if dtype == 0 else NAN32)
                    ext = torch.from_numpy(host).cuda()
                    dst.poison_all()
                    rc = lib.gs_io_import(dst.ptr, C.byref(L), ext.data_ptr() + off * host.itemsize, dtype, sabi,
                                          scale, st())
                    assert rc == 0, what
                    dst.assert_written_exactly(interior, "import " + what)
                    same(dst.to_xyz()[1:-1, 1:-1, 1:-1], expect_import(host[off + idx], scale), "import " + what)
                    same(ext.cpu().numpy(), host, "import source " + what)
                    if import_only:
                        continue
                    # ---- export: sentinel storage, a poisoned field around the box ---------------------------------
                    fv = field_values(shape).copy()
                    flat = fv[1:-1, 1:-1, 1:-1].reshape(-1).copy()
                    fv[1:-1, 1:-1, 1:-1] = salted(flat, scale, NAN64).reshape(shape)
                    src.from_xyz(fv).poison_outside_box().snapshot()
                    sent = np.full(n, SENTINEL[npt], dtype=IW[npt]).view(npt)
                    ext = torch.from_numpy(sent.copy()).cuda()
                    rc = lib.gs_io_export(src.ptr, C.byref(L), ext.data_ptr() + off * sent.itemsize, dtype, sabi,
                                          scale, st())
                    assert rc == 0, what
                    want = sent.copy()
                    want[off + idx] = expect_export(fv[1:-1, 1:-1, 1:-1], scale, npt)
                    same(ext.cpu().numpy(), want, "export " + what)
                    src.assert_unchanged(what="export source " + what)


# ---- the rows' non-temporal instance --------------------------------------------------------------------------------
# The smallest level that selects k_io_rows<d, t, 1, 1> without a switch: exactly 2^25 points, unit-stride x and pitches
# that allow 16-byte accesses; beside it the cached instance just below the threshold, whose rows of 4095 points in the
# same pitch of 4096 end in one ragged 16-byte group. The external side is a contiguous [z][y][4096] tensor.
NT_PITCH = 4096
NT_SHAPES = {(4096, 64, 128): 1, (4095, 64, 128): 0}


@pytest.mark.parametrize("dtype", [A.GS_IO_F64, A.GS_IO_F32], ids=["f64", "f32"])
@pytest.mark.parametrize("shape", NT_SHAPES, ids=sid)
def test_rows_at_the_nt_threshold(shape, dtype):
    """Both directions at scale -0.375 in the default layout: import into a NaN-poisoned field (exactly the interior is
    written), export of that field into sentinel storage; words equal to numpy's, the source unchanged."""
    lib, nt, scale = gsv.io(), NT_SHAPES[shape], -0.375
    nx, ny, nz = shape
    assert (nx * ny * nz >= 1 << 25) == bool(nt) and (NT_PITCH - 1) * ny * nz < 1 << 25
    npt = NPT[dtype]
    s = (1, NT_PITCH, NT_PITCH * ny)
    sabi = (A.i64 * 3)(*s)
    lay = layouts(*shape)["default"]
    fld = LayoutField(*shape, lay.ldy, lay.ldz, lay.phase_out)
    L = fld.level(1.0 / (ny + 1))
    for d in (A.GS_IO_IMPORT, A.GS_IO_EXPORT):
        assert lib.gs_io_kernel(d, dtype, C.byref(L), sabi).decode() == f"k_io_rows<{d}, {dtype}, 1, {nt}>"
    host = np.random.default_rng(5).uniform(-2.0, 2.0, (nz, ny, NT_PITCH)).astype(npt)  # [z][y][x]: all of it data
    ext = torch.from_numpy(host).cuda()
    fld.poison_all()
    assert lib.gs_io_import(fld.ptr, C.byref(L), ext.data_ptr(), dtype, sabi, scale, st()) == 0
    fld.assert_written_exactly(fld.interior_mask(), "import")
    got = fld._box(fld.buf)[1:-1, 1:-1, 1:-1].cpu().numpy()
    want = np.float64(scale) * host[:, :, :nx].astype(np.float64)
    same(got, want, "import")
    same(ext.cpu().numpy(), host, "import source")
    del ext
    # export what the import left: a field whose every word outside the interior is a NaN
    fld.snapshot()
    sent = np.full((nz, ny, NT_PITCH), SENTINEL[npt], dtype=IW[npt]).view(npt)
    out = torch.from_numpy(sent).cuda()
    assert lib.gs_io_export(fld.ptr, C.byref(L), out.data_ptr(), dtype, sabi, scale, st()) == 0
    torch.cuda.synchronize()
    sent[:, :, :nx] = (np.float64(scale) * want).astype(npt)
    same(out.cpu().numpy(), sent, "export")
    fld.assert_unchanged(what="export source")


# ---- the driver ---------------------------------------------------------------------------------------------------
def make_grid(kind, maxiter=3):
    if kind == "xy":
        return gsv.HipGridData(gsv.GridParams(maxiter=maxiter, tol=0.0, gridDim=(15, 15, 8), mode=gsv.GS_LINEAR),
                               coarsen="xy")
    mode = gsv.GS_NEWTON if kind == "newton" else gsv.GS_LINEAR
    return gsv.HipGridData(gsv.GridParams(maxiter=maxiter, tol=0.0, gridDim=(15, 15, 15), mode=mode))


def interior_values(g, level=0, seed=3, scale=50.0):
    geom = g.getLevel(level).geom
    return np.random.default_rng(seed).uniform(-scale, scale, (geom.nx, geom.ny, geom.nz))


def upload(g, name, vals, level=0):
    """The host path: the field as it stands with its interior replaced."""
    a = np.array(g.field(level, name))
    a[1:-1, 1:-1, 1:-1] = vals
    g.set_field(level, name, a)


def zyx(vals, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(vals.transpose(2, 1, 0))).cuda().to(dtype)


def cycles(g, n=3):
    return [gsv.HipSolver.vcycle(g) for _ in range(n)], np.array(g.field(0, "v"))


@pytest.mark.parametrize("kind", ["linear", "xy"])
def test_load_f_equals_set_field(kind):
    with make_grid(kind) as a, make_grid(kind) as b:
        f = interior_values(a)
        upload(a, "f", f)
        b.load("f", zyx(f))
        ha, va = cycles(a)
        hb, vb = cycles(b)
        same(np.array(ha), np.array(hb), "histories")
        same(va, vb, "level-0 v")
    # the reference's axis order, fp32 and a scale: the same words as the upload of the scaled, widened values
    with make_grid(kind) as a, make_grid(kind) as b:
        f32 = interior_values(a).astype(np.float32)
        upload(a, "f", np.float64(-0.375) * f32.astype(np.float64))
        b.load("f", torch.from_numpy(f32).cuda(), scale=-0.375, order="xyz")
        same(np.array(a.field(0, "f")), np.array(b.field(0, "f")), "f")
        ha, va = cycles(a)
        hb, vb = cycles(b)
        same(np.array(ha), np.array(hb), "histories")
        same(va, vb, "level-0 v")


@pytest.mark.parametrize("kind", ["linear", "xy"])
def test_load_v_warm_start(kind):
    with make_grid(kind) as a, make_grid(kind) as b:
        v = interior_values(a, seed=5, scale=1.0)
        upload(a, "v", v)
        b.load("v", zyx(v))
        ha, va = cycles(a, 1)
        hb, vb = cycles(b, 1)
        same(np.array(ha), np.array(hb), "residual")
        same(va, vb, "level-0 v")
        assert not np.array(b.field(0, "v"))[0].any() and not np.array(b.field(0, "v"))[:, :, -1].any()  # the ring


def test_load_newton_v():
    with make_grid("newton", 1) as a, make_grid("newton", 1) as b:
        v = interior_values(a, seed=9, scale=0.1)
        upload(a, "newtonV", v)
        b.load("newtonV", zyx(v))
        ha, hb = gsv.NewtonSolver.solve(a), gsv.NewtonSolver.solve(b)
        same(np.array(ha), np.array(hb), "Newton history")
        same(np.array(a.field(0, "newtonV")), np.array(b.field(0, "newtonV")), "newtonV")


@pytest.mark.parametrize("kind", ["linear", "xy"])
def test_store_equals_field(kind):
    with make_grid(kind) as g:
        g.load("f", zyx(interior_values(g)))
        gsv.HipSolver.solve(g)
        for level in (0, 1):
            want = np.array(g.field(level, "v"))[1:-1, 1:-1, 1:-1]
            assert np.abs(want).max() > 0.0
            got = g.store("v", level=level)
            assert got.dtype == torch.float64 and got.is_contiguous()
            same(got.cpu().numpy().transpose(2, 1, 0), want, f"store v level {level}")
            same(g.store("v", level=level, order="xyz").cpu().numpy(), want, f"store v xyz level {level}")
            # a permuted fp32 out: torch-natural indices over storage in the reference's order
            base = torch.full(want.shape, 7.0, dtype=torch.float32, device="cuda")
            out = base.permute(2, 1, 0)
            assert g.store("v", out=out, level=level, scale=2.0) is out
            same(base.cpu().numpy(), (np.float64(2.0) * want).astype(np.float32), f"store v fp32 level {level}")


def test_ordering_without_synchronisation():
    """f made by a chain of dependent torch ops on a side stream, then load, solve, store and a torch consumer with no
    synchronise call in between: the same words as the run that synchronises after every step."""
    # the chain runs on 2^22 elements so that the device is still at it when the host reaches load()
    base = torch.from_numpy(np.random.default_rng(13).uniform(-1.0, 1.0, 1 << 22)).cuda()

    def run(sync):
        wait = torch.cuda.synchronize if sync else (lambda: None)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with make_grid("linear") as g, torch.cuda.stream(side):
            big = base.clone()
            for _ in range(60):
                big = torch.cos(big * 3.0) + 0.5
            f = big[5:5 + 15 ** 3].view(15, 15, 15)  # a view at an odd offset: no .contiguous()
            wait()
            g.load("f", f, scale=40.0)
            del f, big
            junk = torch.full_like(base, 1e30)  # may take the chain's block: the stream order protects the copy
            wait()
            hist = gsv.HipSolver.solve(g)
            out = g.store("v", dtype=torch.float32)
            wait()
            res = out.double() * 3.0 + 1.0
            wait()
            res = res.cpu().numpy()  # (the one readback, at the end)
            del junk
        torch.cuda.current_stream().wait_stream(side)
        return hist, res

    h0, r0 = run(True)
    h1, r1 = run(False)
    same(np.array(h0), np.array(h1), "histories")
    same(r0, r1, "consumer's result")
    assert np.isfinite(r0).all() and np.abs(r0 - 1.0).max() > 0.0


def test_bad_tensors_raise_before_any_call():
    with make_grid("linear") as g:
        g.load("f", zyx(interior_values(g)))
        before = {n: np.array(g.field(0, n)) for n in ("f", "v")}
        good = torch.zeros(15, 15, 15, dtype=torch.float64, device="cuda")
        for bad in (torch.zeros(15, 15, 14, dtype=torch.float64, device="cuda"),
                    torch.zeros(15, 15, dtype=torch.float64, device="cuda"),
                    torch.zeros(15, 15, 15, dtype=torch.float16, device="cuda"),
                    torch.zeros(15, 15, 15, dtype=torch.int64, device="cuda"),
                    torch.zeros(15, 15, 15, dtype=torch.float64), np.zeros((15, 15, 15))):
            with pytest.raises(ValueError):
                g.load("f", bad)
            with pytest.raises(ValueError):
                g.store("v", out=bad)
        for kw in ({"order": "xyy"}, {"order": "xy"}, {"level": 9}, {"level": -1}):
            with pytest.raises(ValueError):
                g.load("f", good, **kw)
            with pytest.raises(ValueError):
                g.store("f", **kw)
        with pytest.raises(ValueError):
            g.load("nope", good)
        with pytest.raises(ValueError):
            g.store("v", out=good, dtype=torch.float32)
        with pytest.raises(ValueError):
            g.store("v", dtype=torch.float16)
        # what the driver refuses: nothing touched either
        with pytest.raises(gsv.GpuSolveError, match="no such field"):
            g.load("newtonV", good)
        with pytest.raises(gsv.GpuSolveError, match="alias"):
            g.store("v", out=torch.zeros(15, 15, 1, dtype=torch.float64, device="cuda").expand(15, 15, 15))
        with pytest.raises(gsv.GpuSolveError, match="finite"):
            g.load("f", good, scale=float("inf"))
        for n, a in before.items():
            same(np.array(g.field(0, n)), a, n)
