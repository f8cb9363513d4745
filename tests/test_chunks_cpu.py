"""The launch shapes only large levels select, without a GPU: the chunk queries of the six launchers whose z-chunk
has no A/B switch (gs_krylov_vec_chunk, gs_residual_restrict_pa_chunk, gs_residual_restrict_xy_chunk,
gs_residual_restrict_chunk, gs_fmg_prolong_pa_chunk, gs_fmg_prolong_chunk). Each query shares its plan function with
its launcher, so what it reports is what a launch takes; tests/test_gpu_chunks.py states the chunk it means to reach
through them.

Clamp rules: the query against the rule restated here, at each rule's first level above its minimum, at its cap, on
the thin levels tests/test_gpu_chunks.py runs and at 511^3 / 512^3 / 1024^3. fit_chunk rules (the two FMG
prolongations): without a device the capacity is 256 blocks; the result is in range, even where the rule says so, and
the minimum for every shape tests/test_gpu_fmg.py and tests/test_gpu_fmg_pa.py run — which is what those files
cover."""
import ctypes as C

import gpusolve as gsv

UNIT = gsv.Stencil().to_abi()
# the centre third: out of canonical order, so gs_residual_restrict takes k_resrestrict
REORDERED = gsv.Stencil([-1, -1, 6, -1, -1, -1, -1],
                        [(0, 0, 1), (-1, 0, 0), (0, 0, 0), (0, 0, -1), (1, 0, 0), (0, 1, 0), (0, -1, 0)]).to_abi()


def level(nx, ny, nz):
    ldy, ldz, _, _ = gsv.field_layout(nx, ny, nz)
    return gsv.gs_level(nx, ny, nz, ldy, ldz, 0, 1.0 / (ny + 1))


def half(shape):
    return tuple(n // 2 for n in shape)


def cdiv(a, b):
    return (a + b - 1) // b


def clamp(x, lo, hi):
    return max(lo, min(hi, x))


# ---- the clamp rules, restated -------------------------------------------------------------------
def vec_rule(nx, ny, nz):
    """gs_pcg_step / gs_dot: 128 x 4 points per block and plane, ~4096 blocks, 1..16 planes."""
    return clamp(nz * cdiv(nx, 128) * cdiv(ny, 4) // 4096, 1, 16)


def pa_rule(fine):
    """gs_residual_restrict_pa: 64 x 4 coarse points per block and plane, ~1024 blocks, 4..32 coarse planes."""
    cx, cy, cz = half(fine)
    return clamp(cz * cdiv(cx, 64) * cdiv(cy, 4) // 1024, 4, 32)


def xy_rule(fine):
    """gs_residual_restrict_xy: 64 x 4 coarse points per block and plane, ~2048 blocks, 8..64 planes."""
    return clamp(fine[2] * cdiv(fine[0] // 2, 64) * cdiv(fine[1] // 2, 4) // 2048, 8, 64)


def rr_rule(fine):
    """gs_residual_restrict's k_resrestrict: 64 x 4 coarse points per block and plane, ~4096 blocks, 1..16."""
    cx, cy, cz = half(fine)
    return clamp(cz * cdiv(cx, 64) * cdiv(cy, 4) // 4096, 1, 16)


def q_vec(shape):
    return gsv.krylov().gs_krylov_vec_chunk(C.byref(level(*shape)))


def q_pa(fine, coarse=None):
    return gsv.transfer().gs_residual_restrict_pa_chunk(C.byref(level(*fine)), C.byref(level(*(coarse or half(fine)))))


def q_xy(fine, coarse=None):
    coarse = coarse or (fine[0] // 2, fine[1] // 2, fine[2])
    return gsv.semi().gs_residual_restrict_xy_chunk(C.byref(level(*fine)), C.byref(level(*coarse)))


def q_rr(S, fine, mode=0, coarse=None):
    return gsv.kernels().gs_residual_restrict_chunk(C.byref(S), C.byref(level(*fine)),
                                                    C.byref(level(*(coarse or half(fine)))), mode)


CUBES = [(511, 511, 511), (512, 512, 512), (1024, 1024, 1024)]
SMALL = [(2, 2, 2), (7, 7, 7), (33, 17, 9), (130, 6, 4), (257, 17, 501), (127, 127, 63), (64, 64, 64)]


def test_krylov_rule():
    # (3, 4096, 8): the first level above the minimum; (3, 4096, 64) the first at the cap; the thin GPU cases
    cases = {(3, 4096, 7): 1, (3, 4096, 8): 2, (3, 4096, 29): 7, (3, 4096, 63): 15, (3, 4096, 64): 16,
             (3, 4096, 67): 16, (130, 512, 67): 4, (255, 255, 127): 3}
    for shape, want in cases.items():
        assert q_vec(shape) == vec_rule(*shape) == want, shape
    for shape in SMALL + [(1, 1, 1)]:
        assert q_vec(shape) == vec_rule(*shape) == 1, shape
    for shape in CUBES:
        assert q_vec(shape) == vec_rule(*shape), shape
    assert q_vec((512, 512, 512)) == 16
    # the chunk and the partial count are one plan's
    k = gsv.krylov()
    for shape in list(cases) + CUBES:
        L = level(*shape)
        n = cdiv(shape[0], 128) * cdiv(shape[1], 4) * cdiv(shape[2], q_vec(shape))
        assert k.gs_pcg_step_num_partials(C.byref(L)) == k.gs_dot_num_partials(C.byref(L)) == n, shape


def test_pa_rule():
    cases = {(130, 1024, 38): 4, (130, 1024, 40): 5, (2, 4096, 30): 7, (3, 8193, 63): 31, (3, 8193, 64): 32,
             (3, 8193, 91): 32}
    for shape, want in cases.items():
        assert q_pa(shape) == pa_rule(shape) == want, shape
    for shape in SMALL:
        assert q_pa(shape) == pa_rule(shape) == 4, shape
    for shape in CUBES:
        assert q_pa(shape) == pa_rule(shape), shape
    assert q_pa((512, 512, 512)) == 32


def test_xy_rule():
    cases = {(2, 8192, 17): 8, (2, 8192, 18): 9, (2, 8192, 19): 9, (131, 1024, 40): 8, (131, 1024, 75): 9,
             (2, 8192, 127): 63, (2, 8192, 128): 64, (2, 8192, 150): 64}
    for shape, want in cases.items():
        assert q_xy(shape) == xy_rule(shape) == want, shape
    for shape in SMALL + [(131, 10, 17), (31, 31, 8)]:
        assert q_xy(shape) == xy_rule(shape) == 8, shape
    for shape in CUBES:
        assert q_xy(shape) == xy_rule(shape), shape
    assert q_xy((512, 512, 512)) == 64


def test_generic_residual_restrict_rule():
    """k_resrestrict's chunk where the call takes it (a stencil out of canonical order; rows of more than 1024
    points), 0 where k_rr2 does (its chunks have the switches GS_RR_ZC / GS_RR_ZC_BIG)."""
    cases = {(3, 8193, 15): 1, (3, 8193, 16): 2, (3, 8193, 23): 2, (3, 8193, 129): 16, (3, 8193, 140): 16}
    for shape, want in cases.items():
        for mode in (0, 1, 2, 3, 4):
            assert q_rr(REORDERED, shape, mode) == rr_rule(shape) == want, (shape, mode)
        assert q_rr(UNIT, shape) == 0, shape
    for shape in SMALL:
        assert q_rr(REORDERED, shape) == rr_rule(shape) == 1 and q_rr(UNIT, shape) == 0, shape
    for shape in CUBES:
        assert q_rr(REORDERED, shape) == rr_rule(shape) >= 15 and q_rr(UNIT, shape) == 0, shape
    assert q_rr(REORDERED, (512, 512, 512)) == 16
    # rows of more than 1024 points: more x-waves than k_rr2 has
    assert q_rr(UNIT, (1100, 3, 4)) == 1 and q_rr(UNIT, (1024, 4, 3)) == 0
    assert q_rr(UNIT, (2050, 1024, 70)) == rr_rule((2050, 1024, 70)) == 16
    # test_gpu_kernels.py's (511, 515, 256) takes k_rr2: the one tuple of the suite whose rule would give 8
    assert rr_rule((511, 515, 256)) == 8 and q_rr(gsv.Stencil([6, -1, -1.5, -1, -0.5, -1, -1]).to_abi(),
                                                   (511, 515, 256)) == 0


def test_bad_levels_give_zero():
    fine = (130, 1024, 40)
    assert q_pa(fine) > 0 and q_xy(fine) > 0 and q_rr(REORDERED, fine) > 0 and q_vec(fine) > 0
    # a coarse level that is not fine / 2 (XY: with the fine level's nz)
    assert q_pa(fine, (66, 512, 20)) == 0 and q_xy(fine, (65, 512, 20)) == 0 and q_xy(fine, (66, 512, 40)) == 0
    assert q_rr(REORDERED, fine, 0, (66, 512, 20)) == 0          # coarse columns without their fine columns
    assert q_rr(REORDERED, fine, 5) == 0 and q_rr(REORDERED, fine, -1) == 0
    assert q_rr(REORDERED, fine, 0, (0, 512, 20)) == 0           # an empty coarse level: nothing is launched
    k, t, s, kr = gsv.kernels(), gsv.transfer(), gsv.semi(), gsv.krylov()
    good, cg = level(*fine), level(*half(fine))
    for field, value in (("z0", 1), ("ldy", fine[0] + 1), ("ldz", 1), ("nz", -1)):
        bad = level(*fine)
        setattr(bad, field, value)
        assert kr.gs_krylov_vec_chunk(C.byref(bad)) == 0, field
        assert t.gs_residual_restrict_pa_chunk(C.byref(bad), C.byref(cg)) == 0, field
        assert t.gs_fmg_prolong_pa_chunk(C.byref(bad), C.byref(cg)) == 0, field
        assert s.gs_residual_restrict_xy_chunk(C.byref(bad), C.byref(level(65, 512, 40))) == 0, field
        if field != "z0":  # (gs_residual_restrict takes slabs: z0 is a plane condition there)
            assert k.gs_residual_restrict_chunk(C.byref(REORDERED), C.byref(bad), C.byref(cg), 0) == 0, field
    assert kr.gs_krylov_vec_chunk(None) == 0 and kr.gs_krylov_vec_chunk(C.byref(level(0, 4, 4))) == 0
    assert t.gs_residual_restrict_pa_chunk(None, C.byref(cg)) == 0
    assert t.gs_residual_restrict_pa_chunk(C.byref(good), None) == 0
    assert t.gs_fmg_prolong_pa_chunk(C.byref(good), None) == 0 and s.gs_residual_restrict_xy_chunk(None, None) == 0
    assert k.gs_residual_restrict_chunk(None, C.byref(good), C.byref(cg), 0) == 0
    assert k.gs_residual_restrict_chunk(C.byref(REORDERED), None, C.byref(cg), 0) == 0
    assert k.gs_fmg_prolong_chunk(None, C.byref(good)) == 0
    # the grid limits the launchers have: one block per plane / per four fine rows in the grid's z / y extent
    assert q_pa((2, 2, 65536)) == 0 and q_xy((2, 2, 65536)) == 0 and q_pa((2, 2, 65534)) == pa_rule((2, 2, 65534)) == 31
    assert q_xy((1, 8, 3), (0, 4, 3)) == 0 and q_xy((8, 8, 0), (4, 4, 0)) == 0   # no XY transition; nz = 0
    # the aligned prolongation: fine = 2 coarse + 1 only
    assert k.gs_fmg_prolong_chunk(C.byref(level(3, 3, 3)), C.byref(level(7, 7, 7))) == 8
    assert k.gs_fmg_prolong_chunk(C.byref(level(3, 3, 3)), C.byref(level(6, 6, 6))) == 0
    assert k.gs_fmg_prolong_chunk(C.byref(level(7, 7, 7)), C.byref(level(3, 3, 3))) == 0
    assert t.gs_fmg_prolong_pa_chunk(C.byref(level(6, 6, 6)), C.byref(level(3, 3, 3))) == 16
    assert t.gs_fmg_prolong_pa_chunk(C.byref(level(6, 6, 6)), C.byref(level(2, 3, 3))) == 0
    assert t.gs_fmg_prolong_pa_chunk(C.byref(level(1, 6, 6)), C.byref(level(0, 3, 3))) == 0


def test_queries_launch_nothing():
    """A query enqueues no kernel: the launch records of the three libraries that keep one stay empty."""
    k, t, s = gsv.kernels(), gsv.transfer(), gsv.semi()
    buf = C.create_string_buffer(4096)
    for lib, rec in ((k, k.gs_launch_record), (t, t.gs_transfer_launch_record), (s, s.gs_semi_launch_record)):
        rec(buf, 4096)
    q_pa((130, 1024, 40)), q_xy((131, 1024, 40)), q_rr(REORDERED, (3, 8193, 23))
    fmg_pa_chunk((2, 32768, 140)), fmg_chunk((1, 4095, 63))
    for rec in (k.gs_launch_record, t.gs_transfer_launch_record, s.gs_semi_launch_record):
        assert rec(buf, 4096) == 0 and buf.value == b""


# ---- the two fit_chunk rules ------------------------------------------------------------------------------------
def fmg_pa_chunk(fine):
    return gsv.transfer().gs_fmg_prolong_pa_chunk(C.byref(level(*fine)), C.byref(level(*half(fine))))


def fmg_chunk(cd):
    fd = tuple(2 * n + 1 for n in cd)
    return gsv.kernels().gs_fmg_prolong_chunk(C.byref(level(*cd)), C.byref(level(*fd)))


def fit_chunk(tiles, planes, cap, lo, hi, even, halo):
    """gs_device.hpp's fit_chunk, restated: the chunk in [lo, hi] with the best (fill of whole rounds) x c / (c + halo)
    among those that leave no resident block idle; the shortest chunk stands where none does."""
    best, bc = -1.0, 0
    for c in range(lo, hi + 1):
        if even and c % 2:
            continue
        blocks = tiles * cdiv(planes, c)
        if blocks < cap and bc:
            continue
        score = blocks / (cdiv(blocks, cap) * cap) * c / (c + halo)
        if score > best:
            best, bc = score, c
    return bc


NO_DEVICE_CAPACITY = 256  # resident_blocks without a device: 256 compute units x one block


def have_device():
    import torch
    return torch.cuda.is_available()


def test_fit_chunk_queries():
    pa_shapes = [(2, 32768, 140), (2, 32768, 150), (2, 8192, 140), (512, 512, 512), (511, 511, 511), (64, 64, 64),
                 (130, 6, 4), (4, 4, 70)]
    for fine in pa_shapes:
        c = fmg_pa_chunk(fine)
        assert 16 <= c <= 128 and c % 2 == 0, (fine, c)
        if not have_device():
            tiles = cdiv(fine[0], 128) * cdiv(fine[1], 8)
            assert c == fit_chunk(tiles, fine[2], NO_DEVICE_CAPACITY, 16, 128, True, 6.0), (fine, c)
    al_shapes = [(1, 4095, 63), (1, 4095, 31), (255, 255, 255), (31, 31, 31), (1, 1, 1), (300, 2, 2)]
    for cd in al_shapes:
        c = fmg_chunk(cd)
        assert 8 <= c <= 64, (cd, c)
        if not have_device():
            tiles = (cd[0] + 64) // 64 * ((cd[1] + 4) // 4)
            assert c == fit_chunk(tiles, cd[2] + 1, NO_DEVICE_CAPACITY, 8, 64, False, 3.0), (cd, c)
    # a level whose blocks at the minimum chunk do not fill even the smallest capacity keeps the minimum on any
    # device; the thin levels of tests/test_gpu_chunks.py have more tiles than any capacity, and leave it
    assert fmg_pa_chunk((130, 6, 4)) == 16 and fmg_chunk((31, 31, 31)) == 8
    if not have_device():
        assert fmg_pa_chunk((2, 32768, 140)) > 16 and fmg_chunk((1, 4095, 63)) > 8


def test_existing_fmg_shapes_take_the_minimum():
    """What tests/test_gpu_fmg.py, tests/test_gpu_fmg_pa.py and the FMG case of tests/test_gpu_layouts.py cover: every
    kernel-level shape of theirs, and every level of the grids their driver cases build, launches at the minimum
    chunk (at most ~256 blocks, against a capacity in the thousands)."""
    aligned = [(1, 1, 1), (2, 2, 2), (3, 3, 3), (15, 15, 15), (7, 3, 15), (130, 3, 2), (300, 2, 2),  # test_gpu_fmg.py
               (3, 2, 5), (17, 9, 12)]  # test_gpu_layouts.py
    for dims in ((31, 31, 31), (63, 63, 63), (95, 95, 95), (127, 127, 127)):  # its FMG grids
        d = dims
        while min(d) >= 3 and all(n % 2 for n in d):
            d = half(d)
            aligned.append(d)
    for cd in aligned:
        assert fmg_chunk(cd) == 8, cd
    pa = [(2, 2, 2), (3, 3, 3), (4, 4, 4), (5, 4, 6), (7, 6, 2), (130, 6, 4), (258, 3, 2), (6, 18, 4), (4, 4, 19),
          (63, 64, 6), (4, 4, 70), (6, 20, 4), (6, 5, 4)]  # test_gpu_fmg_pa.py
    for dims in ((32, 32, 32), (40, 32, 24), (46, 46, 46), (64, 64, 64), (31, 31, 31)):  # its FMG grids
        d = dims
        while min(d) >= 2:
            pa.append(d)
            d = half(d)
    for fine in pa:
        if min(half(fine)) >= 1:
            assert fmg_pa_chunk(fine) == 16, fine
