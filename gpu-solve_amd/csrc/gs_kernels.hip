// gs_kernels.hip — the product library libgpusolve_hip.so: the extern "C" launchers declared in
// include/gpusolve_hip.h over the gfx950 kernels of gs_device.hpp. Diagnostics (tuning variants,
// bandwidth probes, the rejected k_prr) live in gs_diag.hip -> libgpusolve_diag.so.
#include "gs_device.hpp"

namespace {

// The product's instance of the fused pair k_tb2y for what a launch knows: the base mode, a zero iterate (zv), column
// blocks (colb, else whole rows), the unit stencil, FX (rows of whole waves: no per-lane range selects), a prolongation
// pair (pro, else a plain pair) and, of the NEWTON prolongation pairs, the instance sized for two x-waves (wx2). The
// only place that spells the kernel's template arguments: `plain` and `prolong` list the 51 instances that exist
// (DESIGN.md §9), any other combination has none (nullptr).
PairKernel tb2y_kernel(int mode, bool zv, bool colb, bool unit, bool fx, bool pro, bool wx2)
{
    return with_mode([](auto M, auto ZV, auto XH, auto UN, auto FX, auto PRO, auto WX2) -> PairKernel {
        // the product's fixed choices (libgpusolve_diag.so varies them): non-temporal output stores, cached f loads,
        // per-wave-row code, no timestamps, the default register allocation (one wave per SIMD allowed)
        constexpr bool NT = true, NTF = false, SPEC = true, TS = false;
        constexpr int WPE = 0;
        constexpr int RY = newtonish(M) ? TBY_RY_NEWTON : TBY_RY, WXMAX = WX2 ? 2 : TBY_WX;
        // tby_pfd's prefetch distance; one step for the prolongation pairs and the zero-iterate column blocks
        constexpr int PFD = (PRO || (XH && ZV)) ? 1 : tby_pfd(M);
        // plain pairs: every mode in both shapes, a zero iterate outside NONLINEAR; FX for the unit stencil's LINEAR
        // pairs and NEWTON_B's whole-row pair
        constexpr bool plain = !PRO && !WX2 && !(ZV && M == GS_NONLINEAR) &&
                               (!FX || (UN && !ZV && (M == GS_LINEAR || (M == GS_NEWTON_B && !XH))));
        // prolongation pairs: LINEAR and NEWTON in both shapes, NEWTON's whole rows for two x-waves too; FX for the
        // unit stencil's LINEAR / NEWTON_B pairs of four x-waves
        constexpr bool prolong = PRO && !ZV && (M == GS_LINEAR || newtonish(M)) &&
                                 (!WX2 || (newtonish(M) && !XH && !FX)) &&
                                 (!FX || (UN && (M == GS_LINEAR || M == GS_NEWTON_B)));
        if constexpr (plain || prolong)
            return k_tb2y<M, RY, WXMAX, NT, NTF, ZV, SPEC, PRO ? 1 : 0, PFD, XH, UN, TS, WPE, FX>;
        else
            return nullptr;
    }, mode, zv, colb, unit, fx, pro, wx2);
}

// The prolongation pair's plan (fills = 0: unsupported): LINEAR and NEWTON (NONLINEAR carries restV too). Rows of more
// than 512 points (column blocks, XH, NEWTON too since r04) with the workspace of prolong_ws_elems (the corrected edge
// columns). The fine planes' parities must be the global ones (even z0): they select each plane's combination
PairPlan prolong_plan(const gs_stencil* S, const gs_level* L, int mode)
{
    if (bad_level(L) || !valid_stencil(S) || !(mode == GS_LINEAR || newtonish(mode)) || L->z0 % 2 != 0) return PairPlan{};
    return tb2_plan(S, L, mode);
}

int64_t prolong_ws_elems(const gs_level* L, const PairPlan& plan)
{
    if (!plan.fills || !plan.colb) return 0;
    const int64_t bw = 2 * WAVE * TBY_WX, nb = (L->nx + bw - 1) / bw - 1; // interior block boundaries
    return nb * (L->nz + 4) * 4 * (L->ny + 2);
}

// The NEWTON update + compF pass k_newton_upd per (unit stencil, + the level-1 restriction to coarse_w on `cl`, + the
// next factor B to b_out) over pass_plan's grid: the grid and partial layout of gs_newton_F (k_rb KIND 1)
int launch_newton_upd(const gs_stencil* S, const gs_level* L, double gamma, const double* w, const double* e,
                      const double* F, double* w_out, double* f, double* partials, double* coarse_w, const gs_level* cl,
                      double* b_out, hipStream_t st)
{
    const Coef k = make_coef(S, L, 0.0, gamma);
    const PassPlan plan = pass_plan(S, L);
    const gs_level c = cl ? *cl : gs_level{};
    with_bools([&](auto U, auto RS, auto BF) {
        if constexpr (RS || !BF)
            launch((k_newton_upd<RB_RY, RB_W, U, RS, BF>), plan.grid, dim3(WAVE, RB_W), st, k, w, e, F,
                               w_out, f, partials, (int)L->nx, (int)L->ny, (int)L->nz, L->ldy, L->ldz, plan.zc, coarse_w,
                               (int)c.nx, (int)c.ny, (int)c.nz, c.ldy, c.ldz, b_out);
    }, k.unit, cl != nullptr, b_out != nullptr);
    return launch_status();
}

// gs_residual_restrict's LDS kernel k_resrestrict (the levels k_rr2 does not take): >= 4096 blocks where the level
// has them, 1..16 coarse planes each
struct RrPlan {
    int zc;
    dim3 grid;
};
RrPlan rr_lds_plan(const gs_level* cl)
{
    const int64_t tiles = ((cl->nx + RR_TXC - 1) / RR_TXC) * ((cl->ny + RR_TYC - 1) / RR_TYC);
    int64_t zc = tiles * cl->nz / 4096;
    zc = zc < 1 ? 1 : (zc > 16 ? 16 : zc);
    return RrPlan{(int)zc, dim3((unsigned)((cl->nx + RR_TXC - 1) / RR_TXC), (unsigned)((cl->ny + RR_TYC - 1) / RR_TYC),
                                (unsigned)((cl->nz + zc - 1) / zc))};
}

// gs_residual_restrict's checks of what is not a pointer (mode: a base mode)
bool bad_rr_levels(const gs_stencil* S, const gs_level* fl, const gs_level* cl, int mode)
{
    return !S || !valid_stencil(S) || mode < GS_LINEAR || mode > GS_NEWTON_B || bad_level(fl) || bad_level(cl);
}
// the residual is evaluated on fine local planes 2z+zoff-1 .. 2z+zoff+1 of the interior only
// (planes 0 and nz+1 hold r = 0): they must exist, as must the coarse points' fine columns
bool bad_rr_planes(const gs_level* fl, const gs_level* cl)
{
    const int64_t zoff = 2 * cl->z0 - fl->z0; // fine local centre plane = 2 z + zoff
    return 2 * cl->nx + 1 > fl->nx + 1 || 2 * cl->ny + 1 > fl->ny + 1 || 2 + zoff - 1 < 0 ||
           2 * cl->nz + zoff + 1 > fl->nz + 1;
}

// k_rr2 takes this residual + restriction (else k_resrestrict): no GS_RR_LDS, canonical stencil order, coarse plane z
// over fine plane 2 z, rows of at most RR2_WXMAX x-waves
bool rr2_takes(const gs_stencil* S, const gs_level* fl, const gs_level* cl)
{
    const int64_t zoff = 2 * cl->z0 - fl->z0;
    const int64_t wxs = ((fl->nx + 1) / 2 + WAVE - 1) / WAVE; // x-waves covering coarse columns 1..(fnx+1)/2
    return !kKnobs.rrLds && canonical_order(S) && zoff == 0 && wxs <= RR2_WXMAX;
}

// gs_fmg_prolong's launch shape. Non-temporal fine stores for a stream larger than the Infinity Cache (GS_FMG_NT
// forces either, A/B). z-cells per block: 8 on levels that do not fill the chip, else the chunk of 8..64 that makes
// the grid whole rounds of resident blocks (fit_chunk; each chunk stages three planes more than it has cells)
struct FpPlan {
    bool nt;
    int zc;
    dim3 grid;
};
FpPlan fp_plan(const gs_level* cl, const gs_level* fl)
{
    const bool nt = kKnobs.fmgNt < 0 ? fl->nx * fl->ny * fl->nz >= ((int64_t)1 << 25) : kKnobs.fmgNt != 0;
    const int64_t cells = cl->nz + 1;
    const int64_t tiles = ((cl->nx + FP_TX) / FP_TX) * ((cl->ny + FP_TY) / FP_TY);
    const auto fn = nt ? k_fmg_prolong<true> : k_fmg_prolong<false>;
    int zc = fit_chunk(tiles, cells, resident_blocks((const void*)fn, FP_TX * FP_TY), 8, 64, false, 3.0);
    if (zc < 8) zc = tiles >= 256 && cells >= 128 ? 32 : 8; // (GS_FIT_ROUNDS=0)
    return FpPlan{nt, zc,
                  dim3((unsigned)((cl->nx + FP_TX) / FP_TX), (unsigned)((cl->ny + FP_TY) / FP_TY),
                       (unsigned)((cells + zc - 1) / zc))};
}

} // namespace

// =============================================================================================
extern "C" {

int gs_field_layout(int64_t nx, int64_t ny, int64_t nz, int64_t* ldy, int64_t* ldz, int64_t* alloc_elems,
                    int64_t* origin_offset)
{
    if (nx < 0 || ny < 0 || nz < 0 || !ldy || !ldz || !alloc_elems || !origin_offset) return GS_EINVAL;
    // x=1 of every row 128-B aligned: pitch a multiple of 16 doubles, origin at 15 (mod 16).
    const int64_t py = ((nx + 2 + 15) / 16) * 16;
    *ldy = py;
    *ldz = py * (ny + 2);
    // one extra plane below plane 0 and above plane nz+1 (Z-slab ghost depth 2 for the fused
    // two-sweep kernel), plus slack for the clamped pair loads at the last row
    *origin_offset = 15 + *ldz;
    *alloc_elems = *ldz * (nz + 4) + 32;
    return 0;
}

int gs_rhs_init(const gs_level* L, double* f, int mode, double h0, double gamma, hipStream_t st)
{
    if (bad_level(L) || !f) return GS_EINVAL;
    const dim3 g((unsigned)((L->nx + 2 + 63) / 64), (unsigned)((L->ny + 2 + 3) / 4), (unsigned)(L->nz + 2)), b(64, 4);
    launch(k_rhs, g, b, st, f, mode, h0, gamma, (int)L->nx, (int)L->ny, (int)L->nz, L->z0, L->ldy,
                       L->ldz);
    return launch_status();
}

int gs_jacobi_sweep(const gs_stencil* S, const gs_level* L, int mode, double omega, double gamma,
                    const double* v_in, double* v_out, const double* f, const double* w, hipStream_t st)
{
    return gs_jacobi_sweep_norm(S, L, mode, omega, gamma, v_in, v_out, f, w, nullptr, st);
}

int gs_jacobi_sweep_norm(const gs_stencil* S, const gs_level* L, int mode, double omega, double gamma,
                         const double* v_in, double* v_out, const double* f, const double* w, double* partials,
                         hipStream_t st)
{
    mode = base_mode(mode);
    if (!v_out || !f || v_in == v_out || (newtonish(mode) && !w)) return GS_EINVAL;
    if (partials && L && (L->nx == 0 || L->ny == 0 || L->nz == 0))
        return launch_dry() ? 0 : (int)hipMemsetAsync(partials, 0, sizeof(double), st);
    return launch_pass<0, false>(S, L, mode, omega, gamma, v_in, f, w, v_out, partials, st);
}

int gs_jacobi_sweep2_supported_mode(const gs_stencil* S, const gs_level* L, int mode)
{
    mode = base_mode(mode);
    if (mode < GS_LINEAR || mode > GS_NEWTON_B) return 0;
    return (!bad_level(L) && valid_stencil(S)) ? tb2_plan(S, L, mode).fills : 0;
}

int gs_jacobi_sweep2_supported(const gs_stencil* S, const gs_level* L)
{
    int r = 2;
    for (int m = GS_LINEAR; m <= GS_NEWTON; m++) {
        const int q = gs_jacobi_sweep2_supported_mode(S, L, m);
        r = q < r ? q : r;
    }
    return r;
}

int gs_jacobi_sweep2(const gs_stencil* S, const gs_level* L, int mode, double omega, double gamma,
                     const double* v_in, double* v_out, const double* f, const double* w, int zlo, int zhi,
                     hipStream_t st)
{
    return gs_jacobi_sweep2_norm(S, L, mode, omega, gamma, v_in, v_out, f, w, zlo, zhi, nullptr, st);
}

int gs_jacobi_sweep2_w(const gs_stencil* S, const gs_level* L, int mode, const double* omegas, double gamma,
                       const double* v_in, double* v_out, const double* f, const double* w, int zlo, int zhi,
                       hipStream_t st)
{
    return gs_jacobi_sweep2_norm_w(S, L, mode, omegas, gamma, v_in, v_out, f, w, zlo, zhi, nullptr, st);
}

const char* gs_jacobi_sweep2_kernel(const gs_stencil* S, const gs_level* L, int mode)
{
    mode = base_mode(mode);
    if (bad_level(L) || !valid_stencil(S)) return "";
    const PairPlan plan = tb2_plan(S, L, mode);
    if (!plan.fills) return "";
    if (!plan.colb) return "k_tb2y: 4x2 waves, 2 rows per wave, LDS halo-row exchange, per-wave-row code";
    return "k_tb2y XH: 512-point column blocks of 4x2 waves, edge columns computed lane-parallel";
}

int64_t gs_jacobi_sweep2_num_partials(const gs_stencil* S, const gs_level* L, int mode)
{
    mode = base_mode(mode);
    if (bad_level(L) || !valid_stencil(S)) return 0;
    const PairPlan plan = tb2_plan(S, L, mode);
    return plan.fills ? (int64_t)plan.grid.x * plan.grid.y : 0;
}

int gs_jacobi_sweep2_norm(const gs_stencil* S, const gs_level* L, int mode, double omega, double gamma,
                          const double* v_in, double* v_out, const double* f, const double* w, int zlo, int zhi,
                          double* partials, hipStream_t st)
{
    const double omegas[2] = {omega, omega};
    return gs_jacobi_sweep2_norm_w(S, L, mode, omegas, gamma, v_in, v_out, f, w, zlo, zhi, partials, st);
}

int gs_jacobi_sweep2_norm_w(const gs_stencil* S, const gs_level* L, int mode, const double* omegas, double gamma,
                            const double* v_in, double* v_out, const double* f, const double* w, int zlo, int zhi,
                            double* partials, hipStream_t st)
{
    // GS_NEWTON_G: the GS_NEWTON_B kernels take gamma for the factor instead of loading it (Coef::bconst)
    const int bconst = mode == GS_NEWTON_G;
    mode = base_mode(mode);
    if (!S || !omegas || bad_level(L) || !valid_stencil(S) || !v_out || !f || v_in == v_out ||
        (!v_in && mode == GS_NONLINEAR) ||
        (newtonish(mode) && !w) || mode < GS_LINEAR || mode > GS_NEWTON_B)
        return GS_EINVAL;
    PairPlan plan = tb2_plan(S, L, mode);
    if (!plan.fills) return GS_EINVAL;
    const Coef k = make_coef_w(S, L, omegas, 2, gamma, bconst);
    const int nx = (int)L->nx;
    const bool zv = !v_in, xh = plan.colb, y2 = !plan.colb;
    // FX (r06): LINEAR plain pairs over rows of whole 128-point waves (512-point column blocks) take the instance
    // without per-lane range selects (k_tb2y FX; GS_PAIR_FX=0: the general instance, A/B); so does GS_NEWTON_B's
    // whole-row pair
    const bool fx = (mode == GS_LINEAR && !zv && k.unit && kKnobs.pairFx &&
                     ((xh && nx % (2 * WAVE * TBY_WX) == 0) || (y2 && nx % (2 * WAVE) == 0))) ||
                    (mode == GS_NEWTON_B && !zv && y2 && k.unit && kKnobs.pairFx && nx % (2 * WAVE) == 0);
    const PairKernel fn = tb2y_kernel(mode, zv, xh, k.unit, fx, false, false);
    // LINEAR zero-iterate pairs (the first sweep of a coarse level, v = 0: the lightest variant, three
    // blocks per CU) below 2^26 points: chunks fitted to whole rounds of resident blocks (256^3: 61 vs
    // 71 us; the same rule measured no better for the other pairs, worse for k_rr2 and for NEWTON's
    // zero-iterate pair at two blocks per CU: 133 vs 120 us, r02 tools/fit_session.sh)
    const bool refit = !v_in && !partials && (int64_t)L->nx * L->ny * L->nz < ((int64_t)1 << 26);
    if (refit && mode == GS_LINEAR && y2)
        refit_chunks(fn, (int)(plan.block.x * plan.block.y * plan.block.z), L->nz, 4, 64, true, 2.0, &plan.zc,
                     &plan.grid);
    return launch_tb2y(fn, plan, k, L, v_in, f, w, v_out, partials, zlo, zhi, st);
}

// The fused triple (k_tb3y): LINEAR, whole rows of <= 512 points, whole levels (z0 = 0), the pair's plan
int gs_jacobi_sweep3_supported(const gs_stencil* S, const gs_level* L)
{
    if (!S || bad_level(L) || !valid_stencil(S) || L->z0 != 0) return 0;
    const PairPlan plan = tb2_plan(S, L, GS_LINEAR);
    return plan.colb ? 0 : plan.fills;
}

int gs_jacobi_sweep3(const gs_stencil* S, const gs_level* L, double omega, double gamma, const double* v_in,
                     double* v_out, const double* f, hipStream_t st)
{
    const double omegas[3] = {omega, omega, omega};
    return gs_jacobi_sweep3_w(S, L, omegas, gamma, v_in, v_out, f, st);
}

int gs_jacobi_sweep3_w(const gs_stencil* S, const gs_level* L, const double* omegas, double gamma, const double* v_in,
                       double* v_out, const double* f, hipStream_t st)
{
    if (!S || !omegas || bad_level(L) || !valid_stencil(S) || L->z0 != 0 || !v_in || !v_out || !f || v_in == v_out)
        return GS_EINVAL;
    const PairPlan plan = tb2_plan(S, L, GS_LINEAR);
    if (!plan.fills || plan.colb) return GS_EINVAL;
    const Coef k = make_coef_w(S, L, omegas, 3, gamma);
    const int nx = (int)L->nx, ny = (int)L->ny, nz = (int)L->nz;
    // FX: rows of whole 128-point waves, as the pair's (GS_PAIR_FX=0: the general instance). The unit-stencil instances
    // address through scalar row bases (GS_T3_SADDR=0: per-lane 64-bit addresses, A/B); the general-stencil instance
    // keeps the per-lane addresses, with scalar bases it spills 13 SGPRs to VGPR lanes
    with_bools([&](auto U, auto X, auto A) {
        if constexpr (U || (!X && !A))
            launch((k_tb3y<U, X, U, A>), plan.grid, plan.block, st, k, v_in, f, v_out, nx, ny, nz, L->ldy,
                               L->ldz, plan.zc);
    }, k.unit, k.unit && kKnobs.pairFx && nx % (2 * WAVE) == 0, k.unit && kKnobs.t3Saddr);
    return launch_status();
}

int gs_jacobi_sweep2_prolong_supported(const gs_stencil* S, const gs_level* L, int mode)
{
    return prolong_plan(S, L, base_mode(mode)).fills != 0;
}

int64_t gs_jacobi_sweep2_prolong_ws_elems(const gs_stencil* S, const gs_level* L, int mode)
{
    return prolong_ws_elems(L, prolong_plan(S, L, base_mode(mode)));
}

int gs_jacobi_sweep2_prolong(const gs_stencil* S, const gs_level* L, int mode, double omega, double gamma,
                             const double* v_in, const double* coarse_v, const double* coarse_sub, const gs_level* cl,
                             double* v_out, const double* f, const double* w, int zlo, int zhi, hipStream_t st)
{
    return gs_jacobi_sweep2_prolong_ws(S, L, mode, omega, gamma, v_in, coarse_v, coarse_sub, cl, v_out, f, w, zlo, zhi,
                                       nullptr, 0, st);
}

int gs_jacobi_sweep2_prolong_w(const gs_stencil* S, const gs_level* L, int mode, const double* omegas, double gamma,
                               const double* v_in, const double* coarse_v, const double* coarse_sub,
                               const gs_level* cl, double* v_out, const double* f, const double* w, int zlo, int zhi,
                               hipStream_t st)
{
    return gs_jacobi_sweep2_prolong_ws_w(S, L, mode, omegas, gamma, v_in, coarse_v, coarse_sub, cl, v_out, f, w, zlo,
                                         zhi, nullptr, 0, st);
}

int gs_jacobi_sweep2_prolong_ws(const gs_stencil* S, const gs_level* L, int mode, double omega, double gamma,
                                const double* v_in, const double* coarse_v, const double* coarse_sub,
                                const gs_level* cl, double* v_out, const double* f, const double* w, int zlo, int zhi,
                                double* ws, int64_t ws_elems, hipStream_t st)
{
    const double omegas[2] = {omega, omega};
    return gs_jacobi_sweep2_prolong_ws_w(S, L, mode, omegas, gamma, v_in, coarse_v, coarse_sub, cl, v_out, f, w, zlo,
                                         zhi, ws, ws_elems, st);
}

int gs_jacobi_sweep2_prolong_ws_w(const gs_stencil* S, const gs_level* L, int mode, const double* omegas, double gamma,
                                  const double* v_in, const double* coarse_v, const double* coarse_sub,
                                  const gs_level* cl, double* v_out, const double* f, const double* w, int zlo, int zhi,
                                  double* ws, int64_t ws_elems, hipStream_t st)
{
    const int bconst = mode == GS_NEWTON_G; // (Coef::bconst, as gs_jacobi_sweep2_norm)
    mode = base_mode(mode);
    const PairPlan plan = prolong_plan(S, L, mode);
    // coarse plane of fine local plane z: (z >> 1) + czoff, z0 even (a slab, or a plane range of one)
    const int64_t czoff = cl && plan.fills ? L->z0 / 2 - cl->z0 : 0;
    if (!omegas || !plan.fills || bad_level(cl) || czoff < 0 || !v_in ||
        !coarse_v || !v_out || !f || v_in == v_out || (mode == GS_NONLINEAR) != (coarse_sub != nullptr) || (newtonish(mode) && !w) ||
        (L->nx + 1) / 2 > cl->nx + 1 || (L->ny + 1) / 2 > cl->ny + 1 || (L->nz + 1) / 2 + czoff > cl->nz + 1)
        return GS_EINVAL;
    const int64_t need = prolong_ws_elems(L, plan);
    if (need > 0 && (!ws || ws_elems < need)) return GS_EINVAL;
    // the kernel indexes the coarse field from the plane under fine local plane 0
    coarse_v += czoff * cl->ldz;
    if (coarse_sub) coarse_sub += czoff * cl->ldz;
    const Coef k = make_coef_w(S, L, omegas, 2, gamma, bconst);
    const bool xh = plan.colb;
    if (xh && need > 0) {
        const int bw = 2 * WAVE * TBY_WX, nb = (int)((L->nx + bw - 1) / bw - 1);
        launch(k_pro_strip<false>, dim3((unsigned)((L->ny + 2 + 63) / 64), (unsigned)(L->nz + 4), (unsigned)nb),
                           dim3(256), st, v_in, coarse_v, nullptr, ws, (int)L->nx, (int)L->ny, (int)L->nz, L->ldy,
                           L->ldz, cl->ldy, cl->ldz, bw, zlo ? 1 : 0, zhi ? 1 : 0);
    }
    const dim3 b = plan.block;
    // NEWTON's variant keeps ~37 KB of state per x-wave in LDS (its RECOMP rows): rows of <= 256 points
    // (two x-waves) take the instance sized for two, so that two blocks share a CU (8 waves, the VGPR
    // limit) instead of one block of 4 waves holding the whole LDS of a four-x-wave instance
    // (NEWTON column blocks: the RECOMP LDS state and the edge columns together, 144 B per lane spilled)
    const bool wx2 = newtonish(mode) && !xh && b.y <= 2;
    // FX (r06, as the plain pairs): unit-stencil LINEAR / GS_NEWTON_B prolongation pairs of four x-waves over rows of
    // whole 128-point waves (512-point column blocks) take the instance without per-lane range selects
    const bool fx = k.unit && kKnobs.pairFx && b.y == TBY_WX && (xh ? L->nx % (2 * WAVE * TBY_WX) == 0 : L->nx % (2 * WAVE) == 0);
    const PairKernel fn = tb2y_kernel(mode, false, xh, k.unit, fx && !wx2 && (mode == GS_LINEAR || mode == GS_NEWTON_B), true, wx2);
    return launch_tb2y(fn, plan, k, L, v_in, f, w, v_out, nullptr, zlo, zhi, st,
                       PairOperands{coarse_v, coarse_sub, (int)cl->nx, (int)cl->ny, (int)(cl->nz - czoff), cl->ldy,
                                    cl->ldz, ws});
}

// the small-level tiled kernels (gs_device.hpp k_tile_*): LINEAR / NEWTON, canonical stencil order, whole levels
int gs_tiled_supported(const gs_stencil* S, const gs_level* L, int mode)
{
    mode = base_mode(mode);
    return S && valid_stencil(S) && canonical_order(S) && (mode == GS_LINEAR || newtonish(mode)) && !bad_level(L) &&
           L->z0 == 0 && L->nx >= 1 && L->ny >= 1 && L->nz >= 1;
}

int gs_smooth2_restrict_tiled(const gs_stencil* S, const gs_level* fl, int mode, double omega, double gamma,
                              const double* v_in, double* v_out, const double* f, const double* w, double* coarse_f,
                              const gs_level* cl, hipStream_t st)
{
    const double omegas[2] = {omega, omega};
    return gs_smooth2_restrict_tiled_w(S, fl, mode, omegas, gamma, v_in, v_out, f, w, coarse_f, cl, st);
}

int gs_smooth2_restrict_tiled_w(const gs_stencil* S, const gs_level* fl, int mode, const double* omegas, double gamma,
                                const double* v_in, double* v_out, const double* f, const double* w, double* coarse_f,
                                const gs_level* cl, hipStream_t st)
{
    mode = base_mode(mode); // (the tiled kernels read the factor field, which holds gamma under GS_NEWTON_G)
    if (!omegas || !gs_tiled_supported(S, fl, mode) || bad_level(cl) || cl->z0 != 0 || !v_out || !f || !coarse_f ||
        v_in == v_out || (newtonish(mode) && !w) || cl->nx != fl->nx / 2 || cl->ny != fl->ny / 2 ||
        cl->nz != fl->nz / 2)
        return GS_EINVAL;
    const Coef k = make_coef_w(S, fl, omegas, 2, gamma);
    const dim3 g((unsigned)((fl->nx + TS - 1) / TS), (unsigned)((fl->ny + TS - 1) / TS), (unsigned)((fl->nz + TS - 1) / TS));
    with_mode([&](auto M, auto Z, auto U) {
        if constexpr (M != GS_NONLINEAR)
            launch((k_tile_pre_rr<M, Z, U>), g, dim3(TS_T), st, k, v_in, f, w, v_out, coarse_f, (int)fl->nx,
                               (int)fl->ny, (int)fl->nz, fl->ldy, fl->ldz, (int)cl->nx, (int)cl->ny, (int)cl->nz, cl->ldy,
                               cl->ldz);
    }, mode, !v_in, k.unit);
    return launch_status();
}

int gs_prolong_smooth2_tiled(const gs_stencil* S, const gs_level* fl, int mode, double omega, double gamma,
                             const double* v_in, const double* coarse_v, const gs_level* cl, double* v_out,
                             const double* f, const double* w, hipStream_t st)
{
    const double omegas[2] = {omega, omega};
    return gs_prolong_smooth2_tiled_w(S, fl, mode, omegas, gamma, v_in, coarse_v, cl, v_out, f, w, st);
}

int gs_prolong_smooth2_tiled_w(const gs_stencil* S, const gs_level* fl, int mode, const double* omegas, double gamma,
                               const double* v_in, const double* coarse_v, const gs_level* cl, double* v_out,
                               const double* f, const double* w, hipStream_t st)
{
    mode = base_mode(mode);
    if (!omegas || !gs_tiled_supported(S, fl, mode) || bad_level(cl) || cl->z0 != 0 || !v_in || !coarse_v || !v_out ||
        !f ||
        v_in == v_out || (newtonish(mode) && !w) || (fl->nx + 1) / 2 > cl->nx + 1 || (fl->ny + 1) / 2 > cl->ny + 1 ||
        (fl->nz + 1) / 2 > cl->nz + 1)
        return GS_EINVAL;
    const Coef k = make_coef_w(S, fl, omegas, 2, gamma);
    const dim3 g((unsigned)((fl->nx + TS - 1) / TS), (unsigned)((fl->ny + TS - 1) / TS), (unsigned)((fl->nz + TS - 1) / TS));
    with_mode([&](auto M, auto U) {
        if constexpr (M != GS_NONLINEAR)
            launch((k_tile_pro2<M, U>), g, dim3(TS_T), st, k, v_in, coarse_v, f, w, v_out, (int)fl->nx,
                               (int)fl->ny, (int)fl->nz, fl->ldy, fl->ldz, cl->ldy, cl->ldz);
    }, mode, k.unit);
    return launch_status();
}

int64_t gs_residual_num_partials(const gs_stencil* S, const gs_level* L)
{
    if (!S || !L) return 0;
    if (L->nx == 0 || L->ny == 0 || L->nz == 0) return 1;
    const dim3 g = pass_plan(S, L).grid;
    return (int64_t)g.x * g.y * g.z;
}

int gs_residual(const gs_stencil* S, const gs_level* L, int mode, double gamma, const double* v, const double* f,
                const double* w, double* r, double* partials, hipStream_t st)
{
    mode = base_mode(mode);
    if (!f || (newtonish(mode) && !w)) return GS_EINVAL;
    if (partials && (L && (L->nx == 0 || L->ny == 0 || L->nz == 0)))
        return launch_dry() ? 0 : (int)hipMemsetAsync(partials, 0, sizeof(double), st);
    return launch_pass<1, false>(S, L, mode, 0.0, gamma, v, f, w, r, partials, st);
}

int gs_sumsq_finish(const double* partials, int64_t n, double* out, int accumulate, hipStream_t st)
{
    if (!partials || !out || n < 0) return GS_EINVAL;
    launch(k_sumsq_finish, dim3(1), dim3(FIN_T), st, partials, n, out, accumulate);
    return launch_status();
}

int gs_restrict2(const double* fine, const gs_level* fl, double* ca, double* cb, const gs_level* cl, hipStream_t st)
{
    if (!fine || !ca || bad_level(fl) || bad_level(cl)) return GS_EINVAL;
    if (cl->nx == 0 || cl->ny == 0 || cl->nz == 0) return 0;
    const int64_t zoff = 2 * cl->z0 - fl->z0; // fine local centre plane = 2 z + zoff
    if (2 * cl->nx + 1 > fl->nx + 1 || 2 * cl->ny + 1 > fl->ny + 1 || 2 + zoff - 1 < 0 ||
        2 * cl->nz + zoff + 1 > fl->nz + 1)
        return GS_EINVAL;
    const dim3 g((unsigned)((cl->nx + 63) / 64), (unsigned)((cl->ny + 3) / 4), (unsigned)cl->nz), b(64, 4);
    launch(k_restrict, g, b, st, fine, ca, cb, (int)cl->nx, (int)cl->ny, (int)cl->nz, fl->ldy, fl->ldz,
                       cl->ldy, cl->ldz, (int)zoff);
    return launch_status();
}

int gs_residual_restrict(const gs_stencil* S, const gs_level* fl, int mode, double gamma, const double* v,
                         const double* f, const double* w, double* ca, double* cb, const gs_level* cl, hipStream_t st)
{
    return gs_residual_restrict_slab(S, fl, mode, gamma, v, f, w, ca, cb, cl, 0, st);
}

int gs_residual_restrict_chunk(const gs_stencil* S, const gs_level* fl, const gs_level* cl, int mode)
{
    if (bad_rr_levels(S, fl, cl, base_mode(mode))) return 0;
    if (cl->nx == 0 || cl->ny == 0 || cl->nz == 0 || bad_rr_planes(fl, cl)) return 0;
    return rr2_takes(S, fl, cl) ? 0 : rr_lds_plan(cl).zc;
}

int gs_residual_restrict_slab_supported(const gs_stencil* S, const gs_level* fl)
{
    const bool ldsOnly = kKnobs.rrLds;
    return S && fl && !bad_level(fl) && valid_stencil(S) && canonical_order(S) && !ldsOnly &&
           ((fl->nx + 1) / 2 + WAVE - 1) / WAVE <= RR2_WXMAX;
}

int gs_residual_restrict_slab(const gs_stencil* S, const gs_level* fl, int mode, double gamma, const double* v,
                              const double* f, const double* w, double* ca, double* cb, const gs_level* cl, int zhi,
                              hipStream_t st)
{
    const int bconst = mode == GS_NEWTON_G; // (Coef::bconst: k_rr2 takes gamma for the factor)
    mode = base_mode(mode);
    if (!v || !f || !ca || (newtonish(mode) && !w) || bad_rr_levels(S, fl, cl, mode)) return GS_EINVAL;
    if (cl->nx == 0 || cl->ny == 0 || cl->nz == 0) return 0;
    if (bad_rr_planes(fl, cl)) return GS_EINVAL;
    const int64_t zoff = 2 * cl->z0 - fl->z0; // fine local centre plane = 2 z + zoff
    const Coef k = make_coef(S, fl, 0.0, gamma, bconst);
    const int64_t wxs = ((fl->nx + 1) / 2 + WAVE - 1) / WAVE; // x-waves covering coarse columns 1..(fnx+1)/2
    const bool rr2 = rr2_takes(S, fl, cl); // (GS_RR_LDS: A/B switch for tools/ measurements)
    if (zhi && !rr2) return GS_EINVAL; // the slab form exists for the register kernel only
    if (rr2) {
        // >= 2048 blocks of one coarse row where the level has them (chunks of <= 32 coarse planes)
        // LINEAR levels of >= 2^26 points: two coarse rows per block (231 VGPRs, 2 waves per SIMD): 0.507 vs
        // 0.529 ms at 512^3, but 0.072 vs 0.068 ms at 256^3 (gpurun_out/rrnr2, tools/rr_ab.py);
        // NONLINEAR / NEWTON: one row (VGPR budget). GS_RR_NR=1|2 forces the choice (A/B, tests).
        const int nr_env = kKnobs.rrNr;
        const bool big = fl->nx * fl->ny * fl->nz >= ((int64_t)1 << RR2_NR2_LOG2_POINTS);
        // (NEWTON with two rows spills 19 VGPRs: 40.5 vs 38.9 ms per 512^3 Newton iteration, gpurun_out/rrn)
        const int nr = mode == GS_LINEAR && (nr_env == 2 || (nr_env == 0 && big)) ? 2 : 1;
        const int64_t rows = (cl->ny + nr - 1) / nr; // blocks along y
        const int64_t chunks = (2048 + rows - 1) / rows;
        int64_t zc = (cl->nz + chunks - 1) / chunks;
        zc = zc < 1 ? 1 : (zc > 32 ? 32 : zc);
        // levels of >= 2^26 points: 64-coarse-plane chunks (512^3: 512 blocks, one round at two per CU): k_rr2
        // 0.454-0.462 vs 0.496-0.500 ms, V-cycle 2.111-2.118 vs 2.145-2.148 ms; 1024^3: 4.06 vs 4.12 ms,
        // V-cycle 16.71 vs 16.83-16.86 ms (16 / 32 / 128 planes all slower; profiles/r04/r04w_rr2_zc_big_ab.txt)
        if (big) zc = cl->nz < 64 ? (cl->nz < 1 ? 1 : cl->nz) : 64;
        if (kKnobs.rrZc > 0 && !big) zc = kKnobs.rrZc;       // (A/B: fine levels of < 2^26 points)
        if (kKnobs.rrZcBig > 0 && big) zc = kKnobs.rrZcBig; // (A/B: fine levels of >= 2^26 points)
        const dim3 g((unsigned)rows, (unsigned)((cl->nz + zc - 1) / zc)), b(WAVE, (unsigned)wxs);
        // (the kernel's one operand slot and its non-temporal loads of the rows no neighbouring block reads: the
        // measured choices)
        with_mode([&](auto M, auto N2, auto U) {
            if constexpr (!N2 || M == GS_LINEAR)
                launch((k_rr2<M, N2 ? 2 : 1, U>), g, b, st, k, v, f, w, ca, cb, (int)fl->nx, (int)fl->ny,
                                   (int)fl->nz, fl->ldy, fl->ldz, (int)cl->nx, (int)cl->ny, (int)cl->nz, cl->ldy, cl->ldz,
                                   (int)zc, zhi ? 1 : 0, kKnobs.rrReverse);
        }, mode, nr == 2, k.unit);
        return launch_status();
    }
    StencilOffsets so;
    for (int t = 0; t < 7; t++) {
        so.lds[t] = S->ox[t] + S->oy[t] * RR_VX;
        so.oz[t] = S->oz[t];
    }
    const RrPlan plan = rr_lds_plan(cl);
    const int zc = plan.zc;
    const dim3 g = plan.grid;
    with_mode([&](auto M) {
        launch(k_resrestrict<M>, g, dim3(RR_T), st, k, so, v, f, w, ca, cb, (int)fl->nx, (int)fl->ny,
                           (int)fl->nz, fl->ldy, fl->ldz, (int)cl->nx, (int)cl->ny, (int)cl->nz, cl->ldy, cl->ldz,
                           (int)zoff, (int)zc);
    }, mode);
    return launch_status();
}

int gs_restrict(const double* fine, const gs_level* fl, double* coarse, const gs_level* cl, hipStream_t st)
{
    return gs_restrict2(fine, fl, coarse, nullptr, cl, st);
}

int gs_interpolate(const double* coarse, const gs_level* cl, double* e, const gs_level* fl, hipStream_t st)
{
    if (!coarse || !e || bad_level(fl) || bad_level(cl) || fl->z0 != 0 || cl->z0 != 0) return GS_EINVAL;
    if ((fl->nx + 1) / 2 > cl->nx + 1 || (fl->ny + 1) / 2 > cl->ny + 1 || (fl->nz + 1) / 2 > cl->nz + 1) return GS_EINVAL;
    const dim3 g((unsigned)((fl->nx + 2 + 63) / 64), (unsigned)((fl->ny + 2 + 3) / 4), (unsigned)(fl->nz + 2)), b(64, 4);
    launch(k_interpolate, g, b, st, coarse, e, (int)fl->nx + 2, (int)fl->ny + 2, (int)fl->nz + 2,
                       fl->ldy, fl->ldz, cl->ldy, cl->ldz);
    return launch_status();
}

int gs_prolong_add(const double* coarse_v, const double* coarse_sub, const gs_level* cl, double* fine_v,
                   const gs_level* fl, hipStream_t st)
{
    if (!coarse_v || !fine_v || bad_level(fl) || bad_level(cl)) return GS_EINVAL;
    if (fl->nx == 0 || fl->ny == 0 || fl->nz == 0) return 0;
    // coarse planes read: global floor(gz/2) and +1 for fine global gz in [fz0+1, fz0+fnz]
    const int64_t clo = (fl->z0 + 1) / 2 - cl->z0, chi = (fl->z0 + fl->nz) / 2 + 1 - cl->z0;
    if ((fl->nx + 1) / 2 > cl->nx + 1 || (fl->ny + 1) / 2 > cl->ny + 1 || clo < 0 || chi > cl->nz + 1)
        return GS_EINVAL;
    const dim3 g((unsigned)((fl->nx + 127) / 128), (unsigned)((fl->ny + 3) / 4), (unsigned)fl->nz), b(64, 4);
    with_bools([&](auto SUB) {
        launch(k_prolong_add<SUB>, g, b, st, coarse_v, coarse_sub, fine_v, (int)fl->nx, (int)fl->ny,
                           (int)fl->nz, fl->ldy, fl->ldz, cl->ldy, cl->ldz, (int)fl->z0, (int)cl->z0);
    }, coarse_sub != nullptr);
    return launch_status();
}

int gs_fmg_prolong_supported(const gs_level* cl, const gs_level* fl)
{
    return (!bad_level(cl) && !bad_level(fl) && cl->z0 == 0 && fl->z0 == 0 && cl->nx >= 1 && cl->ny >= 1 &&
            cl->nz >= 1 && fl->nx == 2 * cl->nx + 1 && fl->ny == 2 * cl->ny + 1 && fl->nz == 2 * cl->nz + 1)
               ? 1
               : 0;
}

int gs_fmg_prolong_chunk(const gs_level* cl, const gs_level* fl)
{
    if (!gs_fmg_prolong_supported(cl, fl)) return 0;
    const FpPlan plan = fp_plan(cl, fl);
    return plan.grid.y > 65535u || plan.grid.z > 65535u ? 0 : plan.zc;
}

int gs_fmg_prolong(const double* coarse, const gs_level* cl, double* fine, const gs_level* fl, hipStream_t st)
{
    if (!coarse || !fine || !gs_fmg_prolong_supported(cl, fl)) return GS_EINVAL;
    const FpPlan plan = fp_plan(cl, fl);
    const auto fn = plan.nt ? k_fmg_prolong<true> : k_fmg_prolong<false>;
    const int zc = plan.zc;
    const dim3 g = plan.grid, b(FP_TX, FP_TY);
    if (g.y > 65535u || g.z > 65535u) return GS_EINVAL;
    // the fine pair (2i+1, 2i+2) as one 16-byte store where the layout aligns it (gs_field_layout does)
    const int al = ((reinterpret_cast<uintptr_t>(fine + 1) & 15) == 0 && fl->ldy % 2 == 0 && fl->ldz % 2 == 0) ? 1 : 0;
    launch(fn, g, b, st, coarse, fine, (int)cl->nx, (int)cl->ny, (int)cl->nz, cl->ldy, cl->ldz, fl->ldy,
                       fl->ldz, zc, al);
    return launch_status();
}

int gs_apply_op(const gs_stencil* S, const gs_level* L, double gamma, const double* u, double* out, hipStream_t st)
{
    if (!out) return GS_EINVAL;
    return launch_pass<2, false>(S, L, GS_NONLINEAR, 0.0, gamma, u, nullptr, nullptr, out, nullptr, st);
}

int gs_apply_op_add(const gs_stencil* S, const gs_level* L, double gamma, const double* u, double* f, hipStream_t st)
{
    if (!f) return GS_EINVAL;
    return launch_pass<2, true>(S, L, GS_NONLINEAR, 0.0, gamma, u, nullptr, nullptr, f, nullptr, st);
}

int gs_newton_F(const gs_stencil* S, const gs_level* L, double gamma, const double* w, const double* F, double* f,
                double* partials, hipStream_t st)
{
    if (!f || !F) return GS_EINVAL;
    // compF (NewtonSolver.cpp:48-81) is the NONLINEAR residual of newtonV against newtonF
    return gs_residual(S, L, GS_NONLINEAR, gamma, w, F, nullptr, f, partials, st);
}

int gs_newton_F_update_supported(const gs_stencil* S, const gs_level* L)
{
    return (S && !bad_level(L) && valid_stencil(S) && L->nx > 0 && L->ny > 0 && L->nz > 0 && pass_plan(S, L).rb) ? 1
                                                                                                               : 0;
}

int gs_newton_F_update(const gs_stencil* S, const gs_level* L, double gamma, const double* w, const double* e,
                       const double* F, double* w_out, double* f, double* partials, hipStream_t st)
{
    if (!w || !e || !F || !w_out || !f || w_out == w || w_out == e || !gs_newton_F_update_supported(S, L))
        return GS_EINVAL;
    return launch_newton_upd(S, L, gamma, w, e, F, w_out, f, partials, nullptr, nullptr, nullptr, st);
}

int gs_newton_F_update_restrict_supported(const gs_stencil* S, const gs_level* L, const gs_level* cl)
{
    // a whole level (z0 = 0) and its coarse level (n/2 per axis, the hierarchy's), RB_RY = 2 rows per wave
    return (gs_newton_F_update_supported(S, L) && cl && !bad_level(cl) && L->z0 == 0 && cl->z0 == 0 &&
            cl->nx == L->nx / 2 && cl->ny == L->ny / 2 && cl->nz == L->nz / 2 && cl->nx > 0 && cl->ny > 0 && cl->nz > 0)
               ? 1
               : 0;
}

int gs_newton_F_update_restrict(const gs_stencil* S, const gs_level* L, double gamma, const double* w, const double* e,
                                const double* F, double* w_out, double* f, double* partials, double* coarse_w,
                                const gs_level* cl, hipStream_t st)
{
    return gs_newton_F_update_restrict_bfac(S, L, gamma, w, e, F, w_out, f, partials, coarse_w, cl, nullptr, st);
}

int gs_newton_F_update_restrict_bfac(const gs_stencil* S, const gs_level* L, double gamma, const double* w,
                                     const double* e, const double* F, double* w_out, double* f, double* partials,
                                     double* coarse_w, const gs_level* cl, double* b_out, hipStream_t st)
{
    if (!w || !e || !F || !w_out || !f || !coarse_w || w_out == w || w_out == e ||
        (b_out && (b_out == w_out || b_out == w || b_out == e || b_out == f)) ||
        !gs_newton_F_update_restrict_supported(S, L, cl))
        return GS_EINVAL;
    static_assert(RB_RY == 2, "the fused restriction takes two fine rows per wave");
    return launch_newton_upd(S, L, gamma, w, e, F, w_out, f, partials, coarse_w, cl, b_out, st);
}

int gs_newton_bfac(const gs_level* L, double gamma, const double* w, double* b, hipStream_t st)
{
    if (bad_level(L) || !w || !b) return GS_EINVAL;
    const int64_t n = L->ldz * (L->nz + 4); // planes -1 .. nz+2
    const double *ws = w - L->ldz;
    double* bs = b - L->ldz;
    if (ws < bs + n && bs < ws + n) return GS_EINVAL;
    const uintptr_t a = reinterpret_cast<uintptr_t>(bs), c = reinterpret_cast<uintptr_t>(ws);
    if ((a & 7) || (c & 7)) return GS_EINVAL;
    const int head = ((a ^ c) & 15) ? -1 : (int)((a & 15) / 8); // -1: no common dwordx4 alignment
    launch(k_bfac, dim3(1024), dim3(256), st, bs, ws, n, gamma, head);
    return launch_status();
}

int gs_fill(double* dst, double value, int64_t n, hipStream_t st)
{
    if (!dst || n < 0) return GS_EINVAL;
    if (n == 0) return 0;
    int64_t blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    launch(k_fill, dim3((unsigned)blocks), dim3(256), st, dst, value, n);
    return launch_status();
}

int gs_copy(double* dst, const double* src, int64_t n, hipStream_t st)
{
    if (!dst || !src || n < 0) return GS_EINVAL;
    if (n == 0 || dst == src) return 0;
    const uintptr_t a = reinterpret_cast<uintptr_t>(dst), b = reinterpret_cast<uintptr_t>(src);
    if (((a ^ b) & 15) || (a & 7)) // no common dwordx4 alignment
        return launch_dry() ? 0 : (int)hipMemcpyAsync(dst, src, sizeof(double) * n, hipMemcpyDeviceToDevice, st);
    launch(k_copy, dim3(1024), dim3(256), st, dst, src, n, (a & 15) ? 1 : 0);
    return launch_status();
}

int gs_axpy(double* y, const double* x, double a, int64_t n, hipStream_t st)
{
    if (!y || !x || n < 0) return GS_EINVAL;
    if (n == 0) return 0;
    int64_t blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    launch(k_axpy, dim3((unsigned)blocks), dim3(256), st, y, x, a, n);
    return launch_status();
}

int gs_coarse_cycle_max_levels(void) { return CC_MAXLEV; }

int gs_max_weights(void) { return GS_MAX_WEIGHTS; }

} // extern "C"

// the one-workgroup coarse cycle with one omega, or (omegas != NULL) pre weights followed by post weights
static int coarse_cycle(const gs_stencil* S, const gs_coarse_level* lv, int n, int mode, double omega,
                        const double* omegas, double gamma, int pre, int post, hipStream_t st)
{
    mode = base_mode(mode); // (the coarse levels read their factor fields, which hold gamma under GS_NEWTON_G)
    if (!S || !valid_stencil(S) || !lv || n < 1 || n > CC_MAXLEV || mode < GS_LINEAR || mode > GS_NEWTON_B ||
        pre < 0 || post < 0)
        return GS_EINVAL;
    CcPlan P{};
    P.n = n;
    P.pre = pre;
    P.post = post;
    P.weighted = omegas != nullptr;
    for (int i = 0; omegas && i < pre; i++) P.wpre[i] = omegas[i];
    for (int i = 0; omegas && i < post; i++) P.wpost[i] = omegas[pre + i];
    for (int l = 0; l < n; l++) {
        const gs_coarse_level& a = lv[l];
        const gs_level* g = &a.geom;
        if (bad_level(g) || g->z0 != 0 || g->nx < 1 || g->ny < 1 || g->nz < 1 ||
            g->nx * g->ny * g->nz > (int64_t)INT32_MAX || !a.v || !a.v_alt || a.v == a.v_alt || !a.f ||
            (l + 1 < n && !a.r) || (newtonish(mode) && !a.newton_v) ||
            (mode == GS_NONLINEAR && ((l > 0 && !a.rest_v) || a.v_zero)))
            return GS_EINVAL;
        if (l > 0) { // consecutive levels of one hierarchy (the restriction / prolongation bounds)
            const gs_level* fg = &lv[l - 1].geom;
            if (g->nx != fg->nx / 2 || g->ny != fg->ny / 2 || g->nz != fg->nz / 2) return GS_EINVAL;
        }
        CcLevel& L = P.L[l];
        L.v = a.v;
        L.va = a.v_alt;
        L.f = a.f;
        L.r = a.r;
        L.rv = a.rest_v;
        L.w = a.newton_v;
        L.ldy = g->ldy;
        L.ldz = g->ldz;
        L.nx = (int)g->nx;
        L.ny = (int)g->ny;
        L.nz = (int)g->nz;
        L.vz = a.v_zero != 0;
        L.k = make_coef(S, g, omega, gamma);
    }
    with_mode([&](auto M) { launch(k_coarse_cycle<M>, dim3(1), dim3(CC_T), st, P); }, mode);
    return launch_status();
}

extern "C" {

int gs_coarse_cycle(const gs_stencil* S, const gs_coarse_level* lv, int n, int mode, double omega, double gamma,
                    int pre, int post, hipStream_t st)
{
    return coarse_cycle(S, lv, n, mode, omega, nullptr, gamma, pre, post, st);
}

int gs_coarse_cycle_w(const gs_stencil* S, const gs_coarse_level* lv, int n, int mode, const double* omegas,
                      double gamma, int pre, int post, hipStream_t st)
{
    if (!omegas || pre < 0 || post < 0 || pre > GS_MAX_WEIGHTS || post > GS_MAX_WEIGHTS || pre + post < 1)
        return GS_EINVAL;
    return coarse_cycle(S, lv, n, mode, omegas[0], omegas, gamma, pre, post, st);
}

const char* gs_strerror(int code)
{
    if (code == 0) return "success";
    if (code == GS_EINVAL) return "gpusolve: invalid argument";
    return hipGetErrorString((hipError_t)code);
}

const char* gs_build_info(void)
{
    return "gpusolve_hip v19: LINEAR triples k_tb3y(the pair's whole-row tile, three sweeps per pass, sweep 1 one plane "
           "ahead and last in the step, whole-wave rows: the mirrored y-waves half a step behind (sweep 1 first, own z "
           "loop, s_setprio 1), two load slots that keep their registers across the back-edge, scalar row bases + 32-bit "
           "lane offsets, previous-plane rows in registers, per-lane f in LDS (whole-wave rows: in registers), x-edge "
           "values read row by row from LDS into the DPP shift), "
           "pairs k_tb2y(4x2 waves, 2 rows/wave, one round of z-chunks on large levels, LINEAR 2-step prefetch; +prolong; "
           "512-point column blocks for longer rows in every mode; from 64^3 levels; zero-iterate chunks fitted to "
           "resident rounds; zero iterates q = +0; whole-wave rows without range selects (FX); LINEAR loads grouped by "
           "field; x-edge values in VGPRs for LINEAR and the NEWTON_B whole-row plain pair), sweeps k_rb(ry2 w4 zc<=32 "
           "dpp nt), fused residual+restriction (2 coarse rows per block from 2^26 points, descending z-chunks, halo rows "
           "loaded first, non-temporal unshared rows), NEWTON update + "
           "compF (+ level-1 restriction, + the next factor B), NEWTON inner solves on B (GS_NEWTON_B: reciprocal "
           "quotient, shared per pair; GS_NEWTON_G: B = gamma unread), unit-neighbour stencil sums, tiled small levels, "
           "one-workgroup coarse cycle; full-multigrid start (GS_FMG=k, gs_grid_fmg): tricubic gs_fmg_prolong "
           "(k_fmg_prolong: z-march, coarse planes staged in LDS, 16-byte fine stores); fp-contract=off";
}

int gs_launch_dry_run(int on) { return launch_dry_run(on); }

int64_t gs_launch_record(char* buf, int64_t cap) { return launch_record_take(buf, cap); }

} // extern "C"

#ifdef GS_EXP_EFIELD
// timing-only build (gs_device.hpp): the E field's element distance from newtonV
extern "C" void gs_exp_set_efoff(int64_t n) { gs_exp_efoff = n; }
#endif
