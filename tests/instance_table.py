"""The index of the product's kernel instances — TEST INFRASTRUCTURE ONLY.

One Row per kernel instance of libgpusolve_hip.so (147) and per launchable instance of libgpusolve_transfer.so (9):
its normalised name (demangled, without `(anonymous namespace)::`, the return type and the argument list, as
gs_launch_record reports it), the launcher call that selects it (`call`, one of CALLS below, with its mode, stencil
and options), the smallest shape that selects it and still has every edge, and the A/B switches it needs, if any.

Which combinations of template arguments exist is stated HERE, family by family, never asked of the library:
tests/test_instance_table_cpu.py holds rows + EXCLUDED to the kernels of the built libraries and every row's dry-run
launch record to the row's name; tests/test_gpu_instances.py launches every row against the CPU oracle.

A call body takes R, an operand factory with the interface of tests/test_gpu_layouts.py's Side (inp / out / inout /
parts / ws, plus vec for small one-dimensional inputs): poisoned LayoutFields on the GPU, poisoned host buffers
(HostSide below) for the dry runs, which dereference no pointer."""
import ctypes as C
import functools

import numpy as np

import gpusolve as gsv

OMEGA, GAMMA = 0.8, 1.0
W2 = (0.9, 1.3)  # two different weights: a swapped stage shows
W3 = (0.7, 1.1, 1.4)
POISON_IN = 0x7FF8_C0DE_0000_0A11   # tests/layout_field.py's
POISON_OUT = 0x7FF8_DEAD_0000_0B22
STENCILS = {
    "unit": ((6, -1, -1, -1, -1, -1, -1), list(gsv.CANONICAL_OFFSETS)),
    "general": ((4, -1, -1, -0.5, -0.5, -0.5, -0.5), list(gsv.CANONICAL_OFFSETS)),
    "reordered": ((-1, -1, 6, -1, -1, -1, -1),
                  [(0, 0, 1), (-1, 0, 0), (0, 0, 0), (0, 0, -1), (1, 0, 0), (0, 1, 0), (0, -1, 0)]),
}
# the switches (read when the library is loaded) under which the six instances run that no shape below 2^25 points
# selects; their rows run together in one child process
KNOBS = {"GS_RR_NR": "2", "GS_T3_SADDR": "0", "GS_FMG_NT": "1"}
HIP, TRANSFER = "libgpusolve_hip.so", "libgpusolve_transfer.so"

# kernels libgpusolve_transfer.so compiles from the shared header and has no launcher for
EXCLUDED = {
    HIP: {},
    TRANSFER: {
        "k_rhs": "gs_device.hpp's right-hand side; only gs_rhs_init of libgpusolve_hip.so launches it",
        "k_bfac": "gs_device.hpp's Newton factor; only gs_newton_bfac of libgpusolve_hip.so launches it",
        "k_copy": "gs_device.hpp's copy; only gs_copy of libgpusolve_hip.so launches it",
        "k_fill": "gs_device.hpp's fill; only gs_fill of libgpusolve_hip.so launches it",
        "k_axpy": "gs_device.hpp's axpy; only gs_axpy of libgpusolve_hip.so launches it",
        "k_interpolate": "the reference prolongation; only gs_interpolate of libgpusolve_hip.so launches it",
        "k_restrict": "the reference restriction; only gs_restrict(2) of libgpusolve_hip.so launches it",
        "k_sumsq_finish": "the norm's last step; only gs_sumsq_finish of libgpusolve_hip.so launches it",
    },
}


class Row:
    def __init__(self, family, name, call, shape, mode=0, stencil="unit", lib=HIP, env=None, launches=None, **opts):
        self.family, self.name, self.call, self.shape, self.mode, self.stencil = family, name, call, shape, mode, stencil
        self.lib, self.env, self.opts = lib, dict(env or {}), opts
        self.launches = launches or [name]  # what the call's launch record holds, in order

    @property
    def id(self):
        return self.name.replace(" ", "")

    def __repr__(self):
        return f"Row({self.name!r}, {self.call}, mode {self.mode}, {self.stencil}, {self.shape}, {self.opts}, {self.env})"


def b(x):
    return "true" if x else "false"


def half(shape):
    return tuple(n // 2 for n in shape)


# ---- the fused pair k_tb2y: 51 ----------------------------------------------------------------------------------
def tb2y_name(m, zv, xh, un, fx, pro, wx2):
    """k_tb2y<M, RY, WXMAX, NT, NTF, ZV, SPEC, PRO, PFD, XH, UN, TS, WPE, FX>: two rows per wave in every mode, four
    x-waves (two: WX2), non-temporal stores, cached f loads, per-wave-row code, no timestamps, default registers; the
    prefetch distance is 2 for LINEAR plain pairs outside the zero-iterate column blocks, else 1."""
    pfd = 1 if (pro or (xh and zv) or m != 0) else 2
    return (f"k_tb2y<{m}, 2, {2 if wx2 else 4}, true, false, {b(zv)}, true, {1 if pro else 0}, {pfd}, {b(xh)}, {b(un)}, "
            f"false, 0, {b(fx)}>")


def pair_shape(xh, fx, pro=False, wide=False):
    """ny = 7: two y-tiles, the second ragged; nz = 10: three 4-plane chunks, the last ragged. Whole rows: 130 points
    (two x-waves, the second nearly empty; a NEWTON prolongation pair takes its two-x-wave instance there, and the
    four-x-wave one from 300), FX 128 (the prolongation pairs' FX needs four whole x-waves: 512); column blocks: 513
    (the last block one column; one workspace boundary), FX 1024."""
    if xh:
        nx = 1024 if fx else 513
    elif fx:
        nx = 512 if pro else 128
    else:
        nx = 300 if wide else 130
    return (nx, 7, 10)


def tb2y_rows():
    rows = []
    for un in (True, False):
        st = "unit" if un else "general"
        for xh in (False, True):
            for m in (0, 1, 2, 3):
                for zv in (False, True):  # plain pairs: every mode in both shapes, a zero iterate outside NONLINEAR
                    if zv and m == 1:
                        continue
                    rows.append(Row("k_tb2y", tb2y_name(m, zv, xh, un, False, False, False), "pair",
                                    pair_shape(xh, False), m, st, zero=zv))
            for m in (0, 2, 3):  # prolongation pairs: LINEAR and the NEWTON modes, four x-waves
                rows.append(Row("k_tb2y", tb2y_name(m, False, xh, un, False, True, False), "prolong",
                                pair_shape(xh, False, True, wide=m != 0), m, st))
            if not xh:  # NEWTON's whole rows of two x-waves
                for m in (2, 3):
                    rows.append(Row("k_tb2y", tb2y_name(m, False, False, un, False, True, True), "prolong",
                                    pair_shape(False, False, True), m, st))
    # FX (rows of whole waves), unit stencil only: LINEAR plain pairs in both shapes and NEWTON_B's whole rows;
    # LINEAR and NEWTON_B prolongation pairs in both shapes
    for m, xh in ((0, False), (0, True), (3, False)):
        rows.append(Row("k_tb2y", tb2y_name(m, False, xh, True, True, False, False), "pair", pair_shape(xh, True), m))
    for m in (0, 3):
        for xh in (False, True):
            rows.append(Row("k_tb2y", tb2y_name(m, False, xh, True, True, True, False), "prolong",
                            pair_shape(xh, True, True), m))
    for r in rows:  # column-block prolongation pairs: the edge-column strips first
        if r.call == "prolong" and r.shape[0] > 512:
            r.launches = ["k_pro_strip<false>", r.name]
    return rows


# ---- the one-point passes k_rb (26) and k_generic (10) --------------------------------------------------------------
RB_SHAPE = (130, 9, 1021)  # 2 x 2 tiles of 256 x 8 points, 256 four-plane chunks: 1024 blocks (pass_plan), every edge ragged
GENERIC_SHAPE = (37, 11, 9)


def pass_rows():
    rows = []
    for un in (True, False):
        st = "unit" if un else "general"
        for m in (0, 1, 2, 3):
            for z in (False, True):  # sweeps; the zero iterate outside NONLINEAR
                if z and m == 1:
                    continue
                rows.append(Row("k_rb", f"k_rb<{m}, 0, false, 2, 4, true, true, false, false, {b(z)}, {b(un)}>",
                                "sweep", RB_SHAPE, m, st, zero=z))
            rows.append(Row("k_rb", f"k_rb<{m}, 1, false, 2, 4, true, true, false, false, false, {b(un)}>",
                            "residual", RB_SHAPE, m, st))
        for add in (False, True):  # the FAS operator: NONLINEAR only
            rows.append(Row("k_rb", f"k_rb<1, 2, {b(add)}, 2, 4, true, true, false, false, false, {b(un)}>",
                            "apply_op", RB_SHAPE, 1, st, add=add))
    # k_generic: any stencil order (and the levels too small for k_rb); the zero iterate is a run-time branch
    for m in (0, 1, 2, 3):
        rows.append(Row("k_generic", f"k_generic<{m}, 0, false>", "sweep", GENERIC_SHAPE, m, "reordered", zero=False))
        rows.append(Row("k_generic", f"k_generic<{m}, 1, false>", "residual", GENERIC_SHAPE, m, "reordered"))
    for add in (False, True):
        rows.append(Row("k_generic", f"k_generic<1, 2, {b(add)}>", "apply_op", GENERIC_SHAPE, 1, "reordered", add=add))
    return rows


# ---- residual + restriction: k_rr2 (10), k_resrestrict (4) ----------------------------------------------------------
RR_SHAPE = (130, 7, 10)


def rr_rows():
    rows = []
    for un in (True, False):
        st = "unit" if un else "general"
        for m in (0, 1, 2, 3):
            rows.append(Row("k_rr2", f"k_rr2<{m}, 1, {b(un)}>", "resrestrict", RR_SHAPE, m, st))
        # two coarse rows per block: LINEAR levels of >= 2^26 points, or GS_RR_NR=2
        rows.append(Row("k_rr2", f"k_rr2<0, 2, {b(un)}>", "resrestrict", RR_SHAPE, 0, st, env=KNOBS))
    for m in (0, 1, 2, 3):
        rows.append(Row("k_resrestrict", f"k_resrestrict<{m}>", "resrestrict", RR_SHAPE, m, "reordered"))
    return rows


# ---- the rest of libgpusolve_hip.so ------------------------------------------------------------------------------------
TILE_SHAPE = (17, 9, 12)
CC_DIMS = (17, 9, 12)  # the coarse cycle runs its hierarchy from the second level down
FMG_COARSE = (17, 9, 12)


def other_rows():
    rows = []
    for m in (0, 2, 3):  # the tiled small levels: LINEAR and the NEWTON modes
        for un in (True, False):
            st = "unit" if un else "general"
            for z in (False, True):
                rows.append(Row("k_tile_pre_rr", f"k_tile_pre_rr<{m}, {b(z)}, {b(un)}>", "tile_pre", TILE_SHAPE, m, st,
                                zero=z))
            rows.append(Row("k_tile_pro2", f"k_tile_pro2<{m}, {b(un)}>", "tile_pro", TILE_SHAPE, m, st))
    for un in (True, False):  # the NEWTON update: alone, + level-1 restriction, + the next factor B
        st = "unit" if un else "general"
        for rs, bf in ((False, False), (True, False), (True, True)):
            rows.append(Row("k_newton_upd", f"k_newton_upd<2, 4, {b(un)}, {b(rs)}, {b(bf)}>", "newton_upd", RB_SHAPE, 2,
                            st, rs=rs, bf=bf))
    for m in (0, 1, 2, 3):
        rows.append(Row("k_coarse_cycle", f"k_coarse_cycle<{m}>", "coarse_cycle", CC_DIMS, m))
    # the fused triple k_tb3y<UN, FX, UN, SADDR>: the unit stencil with scalar row bases (GS_T3_SADDR=0: without),
    # rows of whole waves or not; the general stencil's one instance
    for fx in (True, False):
        shape = pair_shape(False, fx)
        rows.append(Row("k_tb3y", f"k_tb3y<true, {b(fx)}, true, true>", "triple", shape))
        rows.append(Row("k_tb3y", f"k_tb3y<true, {b(fx)}, true, false>", "triple", shape, env=KNOBS))
    rows.append(Row("k_tb3y", "k_tb3y<false, false, false, false>", "triple", pair_shape(False, False), 0, "general"))
    for sub in (True, False):
        rows.append(Row("k_prolong_add", f"k_prolong_add<{b(sub)}>", "prolong_add", RR_SHAPE, sub=sub))
    # non-temporal fine stores: from 2^25 fine points, or GS_FMG_NT=1
    rows.append(Row("k_fmg_prolong", "k_fmg_prolong<false>", "fmg_prolong", FMG_COARSE))
    rows.append(Row("k_fmg_prolong", "k_fmg_prolong<true>", "fmg_prolong", FMG_COARSE, env=KNOBS))
    # two workspace boundaries; the pair behind it is the LINEAR column-block prolongation pair
    rows.append(Row("k_pro_strip", "k_pro_strip<false>", "prolong", (1025, 7, 10),
                    launches=["k_pro_strip<false>", tb2y_name(0, False, True, True, False, True, False)]))
    rows += [Row("one-off", "k_rhs", "rhs", GENERIC_SHAPE), Row("one-off", "k_restrict", "restrict", RR_SHAPE),
             Row("one-off", "k_interpolate", "interpolate", RR_SHAPE), Row("one-off", "k_bfac", "bfac", GENERIC_SHAPE),
             Row("one-off", "k_copy", "copy", (70001,)), Row("one-off", "k_fill", "fill", (70001,)),
             Row("one-off", "k_axpy", "axpy", (70001,)), Row("one-off", "k_sumsq_finish", "sumsq", (70001,))]
    return rows


# ---- libgpusolve_transfer.so: 9 launchable ----------------------------------------------------------------------------
PA_SHAPE = (130, 6, 4)  # (tests/test_gpu_transfer.py: even axes, rows of more than one wave)


def transfer_rows():
    rows = [Row("k_resrestrict_pa", f"k_resrestrict_pa<{m}>", "resrestrict_pa", PA_SHAPE, m, lib=TRANSFER)
            for m in (0, 1, 2, 3)]
    rows += [Row("k_prolong_add_pa", f"k_prolong_add_pa<{b(sub)}>", "prolong_add_pa", PA_SHAPE, lib=TRANSFER, sub=sub)
             for sub in (True, False)]
    rows.append(Row("k_fmg_prolong_pa", "k_fmg_prolong_pa<false>", "fmg_prolong_pa", PA_SHAPE, lib=TRANSFER))
    rows.append(Row("k_fmg_prolong_pa", "k_fmg_prolong_pa<true>", "fmg_prolong_pa", PA_SHAPE, lib=TRANSFER, env=KNOBS))
    rows.append(Row("k_restrict_pa", "k_restrict_pa", "restrict_pa", PA_SHAPE, lib=TRANSFER))
    return rows


@functools.lru_cache(maxsize=None)
def rows():
    """Every row; the families the rest of the suite already exercises come first (unit-stencil whole-row pairs, the
    one-point passes, ...), the general-stencil column blocks and multi-wave NEWTON pairs that no other test runs last
    within the pair family."""
    pairs = tb2y_rows()
    known = [r for r in pairs if r.stencil == "unit"]
    new = [r for r in pairs if r.stencil != "unit"]
    new.sort(key=lambda r: (r.shape[0] > 512, r.mode != 0))
    return tuple(other_rows() + pass_rows() + rr_rows() + transfer_rows() + known + new)


FAMILY_COUNTS = {"k_tb2y": 51, "k_rb": 26, "k_generic": 10, "k_rr2": 10, "k_resrestrict": 4, "k_tile_pre_rr": 12,
                 "k_tile_pro2": 6, "k_newton_upd": 6, "k_coarse_cycle": 4, "k_tb3y": 5, "k_prolong_add": 2,
                 "k_fmg_prolong": 2, "k_pro_strip": 1, "one-off": 8,
                 "k_resrestrict_pa": 4, "k_prolong_add_pa": 2, "k_fmg_prolong_pa": 2, "k_restrict_pa": 1}


# ---- inputs ----------------------------------------------------------------------------------------------------------
def inner(a):
    return a[1:-1, 1:-1, 1:-1]


def rand_full(rng, dims, scale=1.0):
    a = np.zeros(tuple(n + 2 for n in dims))
    inner(a)[...] = rng.uniform(-scale, scale, dims)
    return a


@functools.lru_cache(maxsize=6)
def fields(shape, seed=0):
    """v (+-1), f (+-100), w (+-0.8, the Newton modes' range) with zero rings, and B = gamma (1 + w) e^w; read-only."""
    rng = np.random.default_rng(shape[0] + 1000 * shape[1] + 1000003 * shape[2] + seed)
    v, f, w = rand_full(rng, shape), rand_full(rng, shape, 100.0), rand_full(rng, shape, 0.8)
    bf = GAMMA * (1.0 + w) * np.exp(w)
    for a in (v, f, w, bf):
        a.setflags(write=False)
    return v, f, w, bf


def w_of(shape, mode, seed=0):
    """The `w` operand of a mode: none, newtonV, or the factor B."""
    return {0: None, 1: None, 2: fields(shape, seed)[2], 3: fields(shape, seed)[3]}[mode]


def coarse_of(shape):
    """A coarse iterate (+-0.1, zero ring) for the prolongation of `shape`'s level."""
    return fields(half(shape), 5)[0] * 0.1


@functools.lru_cache(maxsize=None)
def stencil_abi(name):
    return gsv.Stencil(list(STENCILS[name][0]), list(STENCILS[name][1])).to_abi()


def arr(*w):
    return (C.c_double * len(w))(*w)


def vec_data(n, seed=0):
    return np.random.default_rng(n + seed).uniform(-1.0, 1.0, n)


# ---- the calls ---------------------------------------------------------------------------------------------------------
# body(R, K, row, st, mode) -> return code. K: the row's library (gsv.kernels() / gsv.transfer()); st: the stream;
# mode: the row's, or 2 for the GS_NEWTON comparison run of a GS_NEWTON_B row (same operands but `w`).
def _svfw(R, row, mode, zero=False):
    shape = row.shape
    v0, f0 = fields(shape)[:2]
    w0 = w_of(shape, mode)
    v = None if zero else R.inp(v0, name="v")
    f = R.inp(f0, "noise", "f", name="f")
    w = R.inp(w0, "noise", name="w") if w0 is not None else None
    return C.byref(stencil_abi(row.stencil)), v, f, w, 1.0 / (shape[1] + 1)


def ptr(x):
    return x.ptr if x is not None else None


def call_pair(R, K, row, st, mode):
    S, v, f, w, h = _svfw(R, row, mode, row.opts.get("zero", False))
    out = R.out(row.shape, "out")
    L = C.byref(out.level(h))
    p = R.parts(K.gs_jacobi_sweep2_num_partials(S, L, mode), "partials")
    return K.gs_jacobi_sweep2_norm_w(S, L, mode, arr(*W2), GAMMA, ptr(v), out.ptr, f.ptr, ptr(w), 0, 0, p.ptr, st)


def call_prolong(R, K, row, st, mode):
    S, v, f, w, h = _svfw(R, row, mode)
    c = R.inp(coarse_of(row.shape), name="coarse_v")
    out = R.out(row.shape, "out")
    L, Lc = C.byref(out.level(h)), C.byref(c.level(2 * h))
    n = K.gs_jacobi_sweep2_prolong_ws_elems(S, L, mode)
    assert (n > 0) == (row.shape[0] > 512)
    ws = R.ws(n) if n else None
    return K.gs_jacobi_sweep2_prolong_ws_w(S, L, mode, arr(*W2), GAMMA, v.ptr, c.ptr, None, Lc, out.ptr, f.ptr, ptr(w),
                                           0, 0, ptr(ws), n, st)


def call_triple(R, K, row, st, mode):
    S, v, f, _, h = _svfw(R, row, 0)
    out = R.out(row.shape, "out")
    return K.gs_jacobi_sweep3_w(S, C.byref(out.level(h)), arr(*W3), GAMMA, v.ptr, out.ptr, f.ptr, st)


def call_sweep(R, K, row, st, mode):
    S, v, f, w, h = _svfw(R, row, mode, row.opts.get("zero", False))
    out = R.out(row.shape, "out")
    L = C.byref(out.level(h))
    p = R.parts(K.gs_residual_num_partials(S, L), "partials")
    return K.gs_jacobi_sweep_norm(S, L, mode, OMEGA, GAMMA, ptr(v), out.ptr, f.ptr, ptr(w), p.ptr, st)


def call_residual(R, K, row, st, mode):
    S, v, f, w, h = _svfw(R, row, mode)
    out = R.out(row.shape, "out")
    L = C.byref(out.level(h))
    p = R.parts(K.gs_residual_num_partials(S, L), "partials")
    return K.gs_residual(S, L, mode, GAMMA, v.ptr, f.ptr, ptr(w), out.ptr, p.ptr, st)


def call_apply_op(R, K, row, st, mode):
    shape = row.shape
    u0, f0 = fields(shape)[:2]
    S, h = C.byref(stencil_abi(row.stencil)), 1.0 / (shape[1] + 1)
    u = R.inp(u0, name="u")
    if row.opts["add"]:
        f = R.inout(f0, "out", "noise")
        return K.gs_apply_op_add(S, C.byref(u.level(h)), GAMMA, u.ptr, f.ptr, st)
    out = R.out(shape, "out")
    return K.gs_apply_op(S, C.byref(u.level(h)), GAMMA, u.ptr, out.ptr, st)


def call_resrestrict(R, K, row, st, mode):
    S, v, f, w, h = _svfw(R, row, mode)
    ca, cb = R.out(half(row.shape), "coarse_a"), R.out(half(row.shape), "coarse_b")
    return K.gs_residual_restrict(S, C.byref(v.level(h)), mode, GAMMA, v.ptr, f.ptr, ptr(w), ca.ptr, cb.ptr,
                                  C.byref(ca.level(2 * h)), st)


def call_tile_pre(R, K, row, st, mode):
    S, v, f, w, h = _svfw(R, row, mode, row.opts.get("zero", False))
    cd = half(row.shape)
    out, cf = R.out(row.shape, "out"), R.out(cd, "coarse_f")
    return K.gs_smooth2_restrict_tiled_w(S, C.byref(out.level(h)), mode, arr(*W2), GAMMA, ptr(v), out.ptr, f.ptr, ptr(w),
                                         cf.ptr, C.byref(cf.level(1.0 / (cd[1] + 1))), st)


def call_tile_pro(R, K, row, st, mode):
    S, v, f, w, h = _svfw(R, row, mode)
    cd = half(row.shape)
    c = R.inp(coarse_of(row.shape), name="coarse_v")
    out = R.out(row.shape, "out")
    return K.gs_prolong_smooth2_tiled_w(S, C.byref(out.level(h)), mode, arr(*W2), GAMMA, v.ptr, c.ptr,
                                        C.byref(c.level(1.0 / (cd[1] + 1))), out.ptr, f.ptr, ptr(w), st)


def call_newton_upd(R, K, row, st, mode):
    shape, cd = row.shape, half(row.shape)
    v0, f0, w0 = fields(shape)[:3]
    S, h = C.byref(stencil_abi(row.stencil)), 1.0 / (shape[1] + 1)
    w, e, F = R.inp(w0, name="w"), R.inp(0.25 * v0, name="e"), R.inp(f0, "noise", "f", name="F")
    L = C.byref(w.level(h))
    wo, f = R.out(shape, "w_out", zero_ring=True), R.out(shape, "f")
    p = R.parts(K.gs_residual_num_partials(S, L), "partials")
    if not row.opts["rs"]:
        return K.gs_newton_F_update(S, L, GAMMA, w.ptr, e.ptr, F.ptr, wo.ptr, f.ptr, p.ptr, st)
    cw = R.out(cd, "coarse_w")
    bo = R.out(shape, "b_out") if row.opts["bf"] else None
    return K.gs_newton_F_update_restrict_bfac(S, L, GAMMA, w.ptr, e.ptr, F.ptr, wo.ptr, f.ptr, p.ptr, cw.ptr,
                                              C.byref(cw.level(2 * h)), ptr(bo), st)


def cc_levels(dims):
    import fmg_ref
    return fmg_ref.level_dims(dims)[1:]


CC_PRE, CC_POST, CC_WEIGHTS = 2, 1, W2 + (1.1,)


def call_coarse_cycle(R, K, row, st, mode):
    ld = cc_levels(row.shape)
    n = len(ld)
    assert 2 <= n <= K.gs_coarse_cycle_max_levels()
    v0, f0 = fields(ld[0], 3)[0] * 0.5, fields(ld[0], 3)[1] * 0.02
    lv = (gsv._abi.gs_coarse_level * n)()
    for l, d in enumerate(ld):
        zero = np.zeros(tuple(x + 2 for x in d))
        v, va = R.inout(v0 if l == 0 else zero, f"v{l}"), R.inout(zero, f"v_alt{l}")
        f = R.inp(f0, "noise", "f", name="f0") if l == 0 else R.inout(zero, f"f{l}", role="f")
        r = R.inout(zero, f"r{l}")
        rv = R.inout(zero, f"rest_v{l}") if mode == 1 else None
        w = R.inp(w_of(d, mode, 7), "noise", name=f"newtonV{l}") if mode >= 2 else None
        lv[l].v, lv[l].v_alt, lv[l].f, lv[l].r = v.ptr, va.ptr, f.ptr, r.ptr
        lv[l].rest_v, lv[l].newton_v = ptr(rv), ptr(w)
        lv[l].geom = v.level(1.0 / (d[1] + 1))
        lv[l].v_zero = 0 if (l == 0 or mode == 1) else 1
    return K.gs_coarse_cycle_w(C.byref(stencil_abi(row.stencil)), lv, n, mode, arr(*CC_WEIGHTS), GAMMA, CC_PRE, CC_POST,
                               st)


def call_prolong_add(R, K, row, st, mode):
    shape, cd = row.shape, half(row.shape)
    c, sub = R.inp(fields(cd, 5)[0], name="coarse"), R.inp(fields(cd, 5)[1], name="coarse_sub")
    v = R.inout(fields(shape)[1], "out")
    return K.gs_prolong_add(c.ptr, sub.ptr if row.opts["sub"] else None, C.byref(c.level(0.2)), v.ptr,
                            C.byref(v.level(0.1)), st)


def fmg_coarse(cd):
    """The coarse field of the tricubic prolongation: its ring takes part as data."""
    rng = np.random.default_rng(sum(cd))
    return rng.uniform(-1.0, 1.0, tuple(n + 2 for n in cd))


def call_fmg_prolong(R, K, row, st, mode):
    cd = row.shape
    c = R.inp(fmg_coarse(cd), name="coarse")
    out = R.out(tuple(2 * n + 1 for n in cd), "out")
    return K.gs_fmg_prolong(c.ptr, C.byref(c.level(0.2)), out.ptr, C.byref(out.level(0.1)), st)


def call_rhs(R, K, row, st, mode):
    nx, ny, nz = row.shape
    f = R.out(row.shape, "out")
    h0 = 1.0 / (ny + 1)
    return K.gs_rhs_init(C.byref(f.level(h0)), f.ptr, 0, h0, GAMMA, st)


def call_restrict(R, K, row, st, mode):
    fine = R.inp(fields(row.shape)[0], name="fine")
    out = R.out(half(row.shape), "out")
    return K.gs_restrict(fine.ptr, C.byref(fine.level(0.1)), out.ptr, C.byref(out.level(0.2)), st)


def call_interpolate(R, K, row, st, mode):
    c = R.inp(fields(half(row.shape), 5)[0], name="coarse")
    e = R.out(row.shape, "out", written="box")
    return K.gs_interpolate(c.ptr, C.byref(c.level(0.2)), e.ptr, C.byref(e.level(0.1)), st)


def bfac_planes(shape):
    """newtonV on the padded box, and its two second ghost planes."""
    rng = np.random.default_rng(sum(shape))
    box = rng.uniform(-0.8, 0.8, tuple(n + 2 for n in shape))
    return box, rng.uniform(-0.8, 0.8, box.shape[:2]), rng.uniform(-0.8, 0.8, box.shape[:2])


def call_bfac(R, K, row, st, mode):
    box, lo, hi = bfac_planes(row.shape)
    w = R.inp(box, "keep", below=lo, above=hi, name="w")
    bo = R.out(row.shape, "out", written="planes")
    return K.gs_newton_bfac(C.byref(w.level(0.1)), GAMMA, w.ptr, bo.ptr, st)


def call_copy(R, K, row, st, mode):
    n = row.shape[0]
    x, y = R.vec(vec_data(n), "x"), R.parts(n, "out")
    return K.gs_copy(y.ptr, x.ptr, n, st)


def call_fill(R, K, row, st, mode):
    n = row.shape[0]
    return K.gs_fill(R.parts(n, "out").ptr, 2.5, n, st)


def call_axpy(R, K, row, st, mode):
    n = row.shape[0]
    x, y = R.vec(vec_data(n), "x"), R.vec(vec_data(n, 1), "out", out=True)
    return K.gs_axpy(y.ptr, x.ptr, 0.5, n, st)


def call_sumsq(R, K, row, st, mode):
    n = row.shape[0]
    x, y = R.vec(vec_data(n) ** 2, "x"), R.parts(1, "out")
    return K.gs_sumsq_finish(x.ptr, n, y.ptr, 0, st)


# the position-aware transfers: the tables are small host arrays, placed by R.vec
def _tables(R, fine, fmg=False):
    abi = gsv.gs_fmg_tables() if fmg else gsv.gs_transfer_tables()
    for a in range(3):
        T = gsv.fmg_axis(fine[a]) if fmg else gsv.transfer_axis(fine[a])
        abi.nf[a], abi.nc[a] = fine[a], fine[a] // 2
        for key in (("cj", "cw") if fmg else ("pj", "pt", "rlo", "rcnt", "rw")):
            getattr(abi, key)[a] = R.vec(np.ascontiguousarray(T[key]).reshape(-1), f"{key}{a}").ptr
    return abi


def call_resrestrict_pa(R, K, row, st, mode):
    S, v, f, w, h = _svfw(R, row, mode)
    T = _tables(R, row.shape)
    cd = half(row.shape)
    out = R.out(cd, "out")
    return K.gs_residual_restrict_pa(S, C.byref(v.level(h)), mode, GAMMA, v.ptr, f.ptr, ptr(w), out.ptr,
                                     C.byref(out.level(1.0 / (cd[1] + 1))), C.byref(T), st)


def call_prolong_add_pa(R, K, row, st, mode):
    shape, cd = row.shape, half(row.shape)
    T = _tables(R, shape)
    c, sub = R.inp(fields(cd, 5)[0], name="coarse"), R.inp(fields(cd, 5)[1], name="coarse_sub")
    v = R.inout(fields(shape)[0], "out")
    return K.gs_prolong_add_pa(c.ptr, sub.ptr if row.opts["sub"] else None, C.byref(c.level(1.0 / (cd[1] + 1))), v.ptr,
                               C.byref(v.level(1.0 / (shape[1] + 1))), C.byref(T), st)


def call_fmg_prolong_pa(R, K, row, st, mode):
    shape, cd = row.shape, half(row.shape)
    T = _tables(R, shape, fmg=True)
    c = R.inp(fields(cd, 5)[0], name="coarse")
    out = R.out(shape, "out")
    return K.gs_fmg_prolong_pa(c.ptr, C.byref(c.level(1.0 / (cd[1] + 1))), out.ptr,
                               C.byref(out.level(1.0 / (shape[1] + 1))), C.byref(T), st)


def call_restrict_pa(R, K, row, st, mode):
    shape, cd = row.shape, half(row.shape)
    T = _tables(R, shape)
    fine = R.inp(fields(shape)[0], name="fine")
    a, bb = R.out(cd, "out"), R.out(cd, "out_b")
    return K.gs_restrict_pa(fine.ptr, C.byref(fine.level(1.0 / (shape[1] + 1))), a.ptr, bb.ptr,
                            C.byref(a.level(1.0 / (cd[1] + 1))), C.byref(T), st)


CALLS = {n[5:]: f for n, f in list(globals().items()) if n.startswith("call_")}


def library(row):
    return gsv.kernels() if row.lib == HIP else gsv.transfer()


def take_record(row):
    """The row's library's launch record, cleared: a list of names."""
    K = library(row)
    take = K.gs_launch_record if row.lib == HIP else K.gs_transfer_launch_record
    buf = C.create_string_buffer(1 << 14)
    n = take(buf, len(buf))
    names = buf.value.decode().splitlines()
    assert n == len(names), (n, names)
    return names


def launch(row, R, st=None, mode=None):
    """Runs the row's call on R's operands; returns (return code, the launch record of the call)."""
    take_record(row)
    rc = CALLS[row.call](R, library(row), row, st, row.mode if mode is None else mode)
    return rc, take_record(row)


def dry_run(row, on):
    K = library(row)
    return (K.gs_launch_dry_run if row.lib == HIP else K.gs_transfer_launch_dry_run)(1 if on else 0)


# ---- host operands for the dry runs ------------------------------------------------------------------------------------
class HostBuf:
    """A host buffer filled with a poison word; `ptr` points `origin` elements in."""

    def __init__(self, n, origin, word):
        self.a = np.full(n, word, dtype=np.uint64)
        self.word, self.ptr = word, self.a.ctypes.data + 8 * origin

    def untouched(self):
        return bool((self.a == self.word).all())


class HostField(HostBuf):
    def __init__(self, dims, word):
        self.nx, self.ny, self.nz = dims
        self.ldy, self.ldz, alloc, origin = gsv.field_layout(*dims)
        super().__init__(alloc, origin, word)

    def level(self, h, z0=0):
        return gsv.gs_level(self.nx, self.ny, self.nz, self.ldy, self.ldz, z0, h)


class HostSide:
    """Side's interface over poisoned host memory: every operand a buffer of one word repeated, inputs included (a dry
    run reads none of them); untouched() after the call says that none was read into or written."""

    def __init__(self):
        self.bufs = []

    def _field(self, dims, word):
        self.bufs.append(HostField(tuple(dims), word))
        return self.bufs[-1]

    def inp(self, box, ring="zero", role="in", zdata=(False, False), below=None, above=None, name=None):
        return self._field([n - 2 for n in np.asarray(box).shape], POISON_IN)

    def out(self, dims, name, written="interior", zero_ring=False):
        return self._field(dims, POISON_OUT)

    def inout(self, box, name, ring="zero", role="out", written="interior"):
        return self._field([n - 2 for n in np.asarray(box).shape], POISON_OUT)

    def parts(self, n, name):
        self.bufs.append(HostBuf(n + 16, 8, POISON_OUT))
        return self.bufs[-1]

    def ws(self, n):
        return self.parts(n, "workspace")

    def vec(self, data, name, out=False):
        return self.parts(np.asarray(data).size, name)

    def untouched(self):
        return all(x.untouched() for x in self.bufs)
