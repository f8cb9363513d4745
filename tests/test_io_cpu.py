"""Device-side field import / export without a GPU (include/gpusolve_io.h): the library's export list
against its header and the ctypes table, the instance a call launches (gs_io_kernel) against the launch record in
dry-run for every stride class, dtype and direction, and every refusal recording nothing."""
import ctypes as C
import os

import numpy as np
import pytest

import gpusolve as gsv
from conftest import REPO
from test_abi import declared, exported

A = gsv._abi
POISON = 0x7FF8_5E41_0000_0C33
SHAPES = [(1, 1, 1), (2, 3, 5), (127, 5, 3), (128, 4, 2), (129, 3, 2), (64, 2, 64), (65, 3, 66), (3, 66, 65),
          (511, 511, 511), (512, 512, 512)]


def level(nx, ny, nz):
    ldy, ldz, _, _ = gsv.field_layout(nx, ny, nz)
    return gsv.gs_level(nx, ny, nz, ldy, ldz, 0, 1.0 / (ny + 1))


def strides(*s):
    return (A.i64 * 3)(*s)


class HostBuf:
    """A poisoned, 16-byte-aligned host buffer: a dry-run launcher must leave every word alone."""

    def __init__(self, words=4096):
        self.a = np.full(words + 2, POISON, dtype=np.int64)
        self.ptr = self.a.ctypes.data + (-self.a.ctypes.data) % 16

    def untouched(self):
        return bool((self.a == POISON).all())


def record(lib):
    buf = C.create_string_buffer(4096)
    n = lib.gs_io_launch_record(buf, 4096)
    return n, buf.value.decode().split("\n")[:-1]


def stride_classes(nx, ny, nz):
    """name -> (strides, the instance family); every class of tests/test_gpu_io.py, plus the 16-byte row pitch."""
    return {
        "zyx": ((1, nx, nx * ny), "rows"),
        "zyx pitch nx+3": ((1, nx + 3, (nx + 3) * ny), "rows"),
        "zyx pitch 16 B": ((1, (nx + 3) // 4 * 4 + 4, ((nx + 3) // 4 * 4 + 4) * ny), "rows"),
        "xyz": ((ny * nz, nz, 1), "tile"),
        "sy = 1": ((ny * nz, 1, ny), "tile"),
        "sx = 2": ((2, 2 * nx + 2, (2 * nx + 2) * ny), "gen"),
    }


def test_header_exports_and_binding_agree():
    names = set(declared(os.path.join(REPO, "include", "gpusolve_io.h")))
    assert names == {"gs_io_import", "gs_io_export", "gs_io_kernel", "gs_io_launch_dry_run", "gs_io_launch_record"}
    assert {n for n in exported(A.IO_LIB) if n.startswith("gs_")} == names
    assert set(A.IO_API) == names
    assert {"gs_grid_import", "gs_grid_export"} <= set(A.DRIVER_API)
    assert {"gs_grid_import", "gs_grid_export"} <= exported(A.DRIVER_LIB)
    assert (gsv.GS_IO_F64, gsv.GS_IO_F32, gsv.GS_IO_IMPORT, gsv.GS_IO_EXPORT) == (0, 1, 0, 1)


def test_import_gpusolve_does_not_import_torch():
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r); import gpusolve; gpusolve.io(); "
            "assert 'torch' not in sys.modules, 'torch imported'" % os.path.join(REPO, "gpu-solve_amd"))
    subprocess.run([sys.executable, "-c", code], check=True)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_name_is_the_launch_record(shape):
    lib = gsv.io()
    L = level(*shape)
    fld, ext = HostBuf(), HostBuf()
    assert lib.gs_io_launch_dry_run(1) == 0
    try:
        record(lib)
        for cls, (s, family) in stride_classes(*shape).items():
            # the header's rule; on one point the dense orders all have stride[0] == 1
            rule = "rows" if s[0] == 1 else "tile" if 1 in s[1:] else "gen"
            assert rule == family or shape == (1, 1, 1)
            family = rule
            for dtype in (A.GS_IO_F64, A.GS_IO_F32):
                for d, call in ((A.GS_IO_IMPORT, lib.gs_io_import), (A.GS_IO_EXPORT, lib.gs_io_export)):
                    name = lib.gs_io_kernel(d, dtype, C.byref(L), strides(*s)).decode()
                    # field + 1 is 16-byte aligned, as gs_field_layout's origin is
                    assert call(fld.ptr + 8, C.byref(L), ext.ptr, dtype, strides(*s), -0.375, None) == 0
                    assert record(lib) == (1, [name]), (cls, dtype, d)
                    if family == "rows":
                        mod = 4 if dtype == A.GS_IO_F32 else 2
                        wide = int(s[1] % mod == 0 and s[2] % mod == 0)
                        nt = int(wide and shape[0] * shape[1] * shape[2] >= 2 ** 25)
                        assert name == f"k_io_rows<{d}, {dtype}, {wide}, {nt}>", (cls, name)
                        # a pointer off the 16-byte grid on either side: the 8-byte instance
                        for fp, ep in ((fld.ptr, ext.ptr), (fld.ptr + 8, ext.ptr + (4 if dtype else 8))):
                            assert call(fp, C.byref(L), ep, dtype, strides(*s), 1.0, None) == 0
                            assert record(lib) == (1, [f"k_io_rows<{d}, {dtype}, 0, 0>"])
                    else:
                        assert name == f"k_io_{family}<{d}, {dtype}>", (cls, name)
        # import only: stride 0 broadcasts one plane into every z (rows) or one row into every x (tile)
        nx, ny, nz = shape
        nt = int(nx * ny * nz >= 2 ** 25)
        for s, want in (((1, nx + (nx & 1), 0), f"k_io_rows<0, 0, 1, {nt}>"), ((0, 1, ny), "k_io_tile<0, 0>"),
                        ((0, 0, 0), "k_io_gen<0, 0>")):
            assert lib.gs_io_kernel(0, 0, C.byref(L), strides(*s)).decode() == want
            assert lib.gs_io_import(fld.ptr + 8, C.byref(L), ext.ptr, 0, strides(*s), 1.0, None) == 0
            assert record(lib) == (1, [want])
        assert fld.untouched() and ext.untouched()
    finally:
        assert lib.gs_io_launch_dry_run(0) == 1


def test_refusals_record_nothing():
    lib = gsv.io()
    L = level(4, 2, 2)
    ok = strides(1, 4, 8)
    fld, ext = HostBuf(), HostBuf()
    assert lib.gs_io_launch_dry_run(1) == 0
    try:
        record(lib)

        def refused(call, d, f=fld.ptr + 8, Lp=L, e=ext.ptr, dtype=0, s=ok, scale=1.0):
            assert call(f, C.byref(Lp) if Lp is not None else None, e, dtype, s, scale, None) == A.GS_EINVAL
            assert record(lib) == (0, [])
            if f and e and np.isfinite(scale):
                assert lib.gs_io_kernel(d, dtype, C.byref(Lp) if Lp is not None else None, s) == b""

        bad_pitch, bad_z0 = level(4, 2, 2), level(4, 2, 2)
        bad_pitch.ldy = 5
        bad_z0.z0 = 1
        for d, call in ((A.GS_IO_IMPORT, lib.gs_io_import), (A.GS_IO_EXPORT, lib.gs_io_export)):
            assert call(fld.ptr + 8, C.byref(L), ext.ptr, 0, ok, 1.0, None) == 0
            assert record(lib)[0] == 1
            refused(call, d, f=None)
            refused(call, d, e=None)
            refused(call, d, s=None)
            refused(call, d, Lp=None)
            refused(call, d, Lp=bad_pitch)
            refused(call, d, Lp=bad_z0)
            refused(call, d, dtype=2)
            refused(call, d, dtype=-1)
            for scale in (float("inf"), float("-inf"), float("nan")):
                refused(call, d, scale=scale)
            refused(call, d, s=strides(1, -4, 8))
            refused(call, d, s=strides(-1, 4, 8))
        assert lib.gs_io_kernel(2, 0, C.byref(L), ok) == b""
        # export: a zero stride, aliasing strides
        for s in ((1, 4, 0), (0, 1, 2), (1, 4, 4), (1, 3, 8), (2, 1, 2), (1, 4, 7), (2, 2, 8)):
            refused(lib.gs_io_export, A.GS_IO_EXPORT, s=strides(*s))
        # ... which an import takes
        for s in ((1, 4, 0), (1, 4, 4), (0, 0, 0)):
            assert lib.gs_io_import(fld.ptr + 8, C.byref(L), ext.ptr, 0, strides(*s), 1.0, None) == 0
            assert record(lib)[0] == 1
        # not aliasing: any order of the axes, gaps, an axis of one point whatever its stride
        for s in ((4, 2, 1), (2, 1, 8), (1, 4, 9), (3, 12, 24)):
            assert lib.gs_io_export(fld.ptr + 8, C.byref(L), ext.ptr, 0, strides(*s), 1.0, None) == 0
            assert record(lib)[0] == 1
        # rows are the launch grid's y and z: 65535 at the most; the same level goes through the other instances
        tall = level(4, 65536, 1)
        refused(lib.gs_io_import, A.GS_IO_IMPORT, Lp=tall, s=strides(1, 4, 4 * 65536))
        assert lib.gs_io_import(fld.ptr + 8, C.byref(tall), ext.ptr, 0, strides(65536, 1, 4 * 65536), 1.0, None) == 0
        assert record(lib) == (1, ["k_io_tile<0, 0>"])
        one = level(4, 1, 2)
        assert lib.gs_io_export(fld.ptr + 8, C.byref(one), ext.ptr, 0, strides(1, 2, 4), 1.0, None) == 0
        assert record(lib)[0] == 1
        assert fld.untouched() and ext.untouched()
    finally:
        assert lib.gs_io_launch_dry_run(0) == 1


@pytest.mark.parametrize("dims", [(0, 3, 3), (3, 0, 3), (3, 3, 0)])
def test_empty_axis_launches_nothing(dims):
    lib = gsv.io()
    L = level(*dims)
    fld, ext = HostBuf(), HostBuf()
    assert lib.gs_io_launch_dry_run(1) == 0
    try:
        record(lib)
        for d, call in ((0, lib.gs_io_import), (1, lib.gs_io_export)):
            for dtype in (0, 1):
                assert call(fld.ptr + 8, C.byref(L), ext.ptr, dtype, strides(1, 3, 9), 2.0, None) == 0
                assert record(lib) == (0, [])
                assert lib.gs_io_kernel(d, dtype, C.byref(L), strides(1, 3, 9)) == b""
        # a bad argument is still one
        assert lib.gs_io_import(fld.ptr + 8, C.byref(L), ext.ptr, 3, strides(1, 3, 9), 2.0, None) == A.GS_EINVAL
    finally:
        assert lib.gs_io_launch_dry_run(0) == 1
    # outside dry-run too: nothing is launched, so no device is needed
    assert lib.gs_io_import(fld.ptr + 8, C.byref(L), ext.ptr, 0, strides(1, 3, 9), 1.0, None) == 0
    assert fld.untouched() and ext.untouched()
