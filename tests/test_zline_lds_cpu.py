"""Which z-line instance a level gets, without a GPU: gs_zline_kernel is the launcher's own predicate (zl_plan of
csrc/gs_line.hip). k_zline_lds takes the levels of few, long columns — fewer than 32 * 32 columns, ZF_MIN_NZ to
ZF_MAX_NZ planes, in any order of the stencil's entries; every other level keeps the instance it had
(tests/test_zline_cpu.py pins those below ZF_MIN_NZ planes and at nz = 4093)."""
import ctypes as C

import pytest

import gpusolve as gsv
import oracle as O
import zline_ref as Z

ZF_MIN_NZ, ZF_MAX_NZ = 64, 1536  # csrc/gs_line_device.hpp
ORDERS = {"canonical": (Z.STRONGZ, list(O.CANONICAL)), "permuted": Z.permuted(Z.STRONGZ)}


def abi(values, offsets):
    return gsv.Stencil(list(values), [tuple(o) for o in offsets]).to_abi()


def level(nx, ny, nz):
    ldy, ldz, _, _ = gsv.field_layout(nx, ny, nz)
    return gsv.gs_level(nx, ny, nz, ldy, ldz, 0, 1.0 / (ny + 1))


def name(S, L, zero):
    return gsv.line().gs_zline_kernel(C.byref(S), C.byref(L), zero).decode()


def inst(kernel, zero):
    return f"{kernel}<{'true' if zero else 'false'}>"


def test_the_constants_leave_the_pinned_levels_alone():
    # tests/test_zline_cpu.py and tests/test_gpu_zline.py pin k_zline_col at nz <= 9 and at nz = 4093
    assert 10 <= ZF_MIN_NZ <= ZF_MAX_NZ and 1024 <= ZF_MAX_NZ <= 4092


@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("zero", [0, 1])
def test_few_long_columns_take_the_lds_instance(order, zero):
    S = abi(*ORDERS[order])
    for dims in ((31, 31, ZF_MIN_NZ), (33, 31, ZF_MIN_NZ), (1, 1, ZF_MAX_NZ), (1, 1, ZF_MIN_NZ), (3, 3, 511)):
        assert name(S, level(*dims), zero) == inst("k_zline_lds", zero), dims


@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("zero", [0, 1])
def test_every_other_level_keeps_its_instance(order, zero):
    S = abi(*ORDERS[order])
    for dims in ((1, 1, ZF_MAX_NZ + 1), (31, 31, ZF_MIN_NZ - 1), (33, 31, ZF_MAX_NZ + 1), (33, 31, 9), (1, 1, 4093)):
        assert name(S, level(*dims), zero) == inst("k_zline_col", zero), dims
    # from 32 * 32 columns on nothing changed: the marching instance in canonical order, one column per thread else
    want = "k_zline_march" if order == "canonical" else "k_zline_col"
    for dims in ((32, 32, ZF_MIN_NZ), (32, 32, ZF_MAX_NZ), (64, 16, 511), (32, 32, 1)):
        assert name(S, level(*dims), zero) == inst(want, zero), dims


def test_refused_arguments_give_the_empty_name():
    can = abi(*ORDERS["canonical"])
    weak = abi((1.9, -0.05, -0.05, -0.05, -0.05, -1.0, -1.0), O.CANONICAL)
    diag = list(O.CANONICAL)
    diag[1] = (1, 1, 0)
    shifted = level(31, 31, ZF_MIN_NZ)
    shifted.z0 = 1
    for zero in (0, 1):
        assert name(weak, level(31, 31, ZF_MIN_NZ), zero) == ""
        assert name(abi(Z.STRONGZ, diag), level(31, 31, ZF_MIN_NZ), zero) == ""
        assert name(can, shifted, zero) == ""
        for dims in ((0, 31, ZF_MIN_NZ), (31, 0, ZF_MIN_NZ), (31, 31, 0)):
            assert name(can, level(*dims), zero) == "", dims
