// gs_semi.hip — libgpusolve_semi.so: the XY semi-coarsening rule and transfers of include/gpusolve_semi.h
// (definitions and evaluation order there). Its own library and header: the other libraries' export lists and kernels
// stay what they are. gs_device.hpp gives Coef, the residual's point expressions and the launch helpers; as in the
// transfer and line libraries its non-template kernels come along as code objects nothing here launches, and its
// Knobs are read from the environment once, when the library is loaded. No launcher reads the environment.
#include "gs_device.hpp"
#include "gs_semi_device.hpp"

#include "gpusolve_semi.h"

namespace {

// the seven axis offsets once each: index of the centre, of (0,0,+1), of (0,0,-1), and the four x / y entries in
// config order; false for any other set (gs_zline_supported's shape test)
struct SemiShape {
    int c, up, lo, xy[4];
};
bool semi_shape(const gs_stencil* S, SemiShape* out)
{
    SemiShape z{-1, -1, -1, {-1, -1, -1, -1}};
    int nxy = 0;
    bool seen[7] = {};
    for (int i = 0; i < 7; i++) {
        const int ox = S->ox[i], oy = S->oy[i], oz = S->oz[i];
        if (ox < -1 || ox > 1 || oy < -1 || oy > 1 || oz < -1 || oz > 1) return false;
        if ((ox != 0) + (oy != 0) + (oz != 0) > 1) return false; // a diagonal offset
        const int id = ox ? (ox > 0 ? 1 : 2) : oy ? (oy > 0 ? 3 : 4) : oz ? (oz > 0 ? 5 : 6) : 0;
        if (seen[id]) return false; // a repeated offset
        seen[id] = true;
        if (id == 0) z.c = i;
        else if (id == 5) z.up = i;
        else if (id == 6) z.lo = i;
        else z.xy[nxy++] = i;
    }
    *out = z;
    return true;
}

// whole levels, fine (nx, ny, nz) -> coarse (nx / 2, ny / 2, nz), tables for exactly that; one block per plane in
// the grid's z extent (the two stored-field kernels) and per XY_TYC / 4 rows in its y extent
bool bad_xy_pair(const gs_level* fl, const gs_level* cl)
{
    if (bad_level(fl) || bad_level(cl) || fl->z0 != 0 || cl->z0 != 0) return true;
    if (fl->nx < 2 || fl->ny < 2 || cl->nx != fl->nx / 2 || cl->ny != fl->ny / 2 || cl->nz != fl->nz) return true;
    return fl->nz > 65535 || (fl->ny + 3) / 4 > 65535;
}

bool bad_xy(const gs_level* fl, const gs_level* cl, const gs_transfer_tables* T)
{
    if (bad_xy_pair(fl, cl) || !T) return true;
    const int64_t nf[2] = {fl->nx, fl->ny}, nc[2] = {cl->nx, cl->ny};
    for (int a = 0; a < 2; a++) {
        if (T->nf[a] != nf[a] || T->nc[a] != nc[a]) return true;
        if (!T->pj[a] || !T->pt[a] || !T->rlo[a] || !T->rcnt[a] || !T->rw[a]) return true;
    }
    if (T->nf[2] != fl->nz || T->nc[2] != fl->nz) return true;
    if (T->pj[2] || T->pt[2] || T->rlo[2] || T->rcnt[2] || T->rw[2]) return true;
    return false;
}

// gs_residual_restrict_xy's launch shape: z-chunks of 8..64 planes (a chunk re-reads two v planes), for ~2048 blocks
// where the level has them
struct XyPlan {
    int zc;
    dim3 grid;
};
XyPlan xy_plan(const gs_level* fl, const gs_level* cl)
{
    const int64_t tiles = ((cl->nx + XY_TXC - 1) / XY_TXC) * ((cl->ny + XY_TYC - 1) / XY_TYC);
    int64_t zc = fl->nz * tiles / 2048;
    zc = zc < 8 ? 8 : (zc > 64 ? 64 : zc);
    return XyPlan{(int)zc, dim3((unsigned)((cl->nx + XY_TXC - 1) / XY_TXC), (unsigned)((cl->ny + XY_TYC - 1) / XY_TYC),
                                (unsigned)((fl->nz + zc - 1) / zc))};
}

XyTables device_tables(const gs_transfer_tables* T)
{
    XyTables d;
    for (int a = 0; a < 2; a++) {
        d.pj[a] = T->pj[a];
        d.pt[a] = T->pt[a];
        d.rlo[a] = T->rlo[a];
        d.rcnt[a] = T->rcnt[a];
        d.rw[a] = T->rw[a];
    }
    return d;
}

} // namespace

extern "C" {

int gs_semi_level_stencil(const gs_stencil* S, double h0, double hl, gs_stencil* out)
{
    SemiShape z;
    if (!S || !out || !(h0 > 0.0) || !(hl > 0.0) || !std::isfinite(h0) || !std::isfinite(hl) || !semi_shape(S, &z))
        return GS_EINVAL;
    const double q = hl / h0;
    const double r = q * q;
    const double sum = ((S->s[z.xy[0]] + S->s[z.xy[1]]) + S->s[z.xy[2]]) + S->s[z.xy[3]];
    const double a = r * S->s[z.c];
    const double b = (r - 1.0) * sum;
    gs_stencil t = *S;
    t.s[z.c] = a + b;
    t.s[z.up] = r * S->s[z.up];
    t.s[z.lo] = r * S->s[z.lo];
    *out = t;
    return 0;
}

int gs_restrict_xy(const double* fine, const gs_level* fl, double* coarse, const gs_level* cl,
                   const gs_transfer_tables* T, hipStream_t st)
{
    if (!fine || !coarse || bad_xy(fl, cl, T)) return GS_EINVAL;
    if (fl->nz == 0) return 0;
    const dim3 g((unsigned)((cl->nx + 63) / 64), (unsigned)((cl->ny + 3) / 4), (unsigned)cl->nz), b(64, 4);
    launch(k_restrict_xy, g, b, st, device_tables(T), fine, coarse, (int)cl->nx, (int)cl->ny, (int)fl->nx, (int)fl->ny,
           fl->ldy, fl->ldz, cl->ldy, cl->ldz);
    return launch_status();
}

int gs_prolong_add_xy(const double* coarse_v, const gs_level* cl, double* fine_v, const gs_level* fl,
                      const gs_transfer_tables* T, hipStream_t st)
{
    if (!coarse_v || !fine_v || bad_xy(fl, cl, T)) return GS_EINVAL;
    if (fl->nz == 0) return 0;
    const dim3 g((unsigned)((fl->nx + 127) / 128), (unsigned)((fl->ny + 3) / 4), (unsigned)fl->nz), b(64, 4);
    // the fine pair (x odd, x + 1) as one 16-byte access where the layout aligns it (gs_field_layout does)
    const int al = ((reinterpret_cast<uintptr_t>(fine_v + 1) & 15) == 0 && fl->ldy % 2 == 0 && fl->ldz % 2 == 0) ? 1 : 0;
    launch(k_prolong_add_xy, g, b, st, device_tables(T), coarse_v, fine_v, (int)fl->nx, (int)fl->ny, (int)cl->nx,
           (int)cl->ny, fl->ldy, fl->ldz, cl->ldy, cl->ldz, al);
    return launch_status();
}

int gs_residual_restrict_xy(const gs_stencil* S, const gs_level* fl, const double* v, const double* f, double* coarse_f,
                            const gs_level* cl, const gs_transfer_tables* T, hipStream_t st)
{
    if (!S || !valid_stencil(S) || !v || !f || !coarse_f || bad_xy(fl, cl, T)) return GS_EINVAL;
    if (fl->nz == 0) return 0;
    const Coef k = make_coef(S, fl, 0.0, 0.0);
    XyStencil so;
    for (int t = 0; t < 7; t++) {
        so.lds[t] = S->ox[t] + S->oy[t] * XY_VX;
        so.oz[t] = S->oz[t];
    }
    const XyPlan plan = xy_plan(fl, cl);
    const int zc = plan.zc;
    const dim3 g = plan.grid, b(XY_T);
    launch(k_resrestrict_xy, g, b, st, k, so, device_tables(T), v, f, coarse_f, (int)fl->nx, (int)fl->ny, (int)fl->nz,
           fl->ldy, fl->ldz, (int)cl->nx, (int)cl->ny, cl->ldy, cl->ldz, (int)zc);
    return launch_status();
}

int gs_residual_restrict_xy_chunk(const gs_level* fl, const gs_level* cl)
{
    if (bad_xy_pair(fl, cl) || fl->nz == 0) return 0;
    return xy_plan(fl, cl).zc;
}

const char* gs_semi_kernel(int op, const gs_level* fl, const gs_level* cl)
{
    if (bad_level(fl) || bad_level(cl) || fl->z0 != 0 || cl->z0 != 0 || fl->nx < 2 || fl->ny < 2 ||
        cl->nx != fl->nx / 2 || cl->ny != fl->ny / 2 || cl->nz != fl->nz || fl->nz == 0 || fl->nz > 65535 ||
        (fl->ny + 3) / 4 > 65535)
        return "";
    switch (op) {
    case GS_SEMI_RESIDUAL_RESTRICT: return "k_resrestrict_xy";
    case GS_SEMI_RESTRICT: return "k_restrict_xy";
    case GS_SEMI_PROLONG_ADD: return "k_prolong_add_xy";
    default: return "";
    }
}

int gs_semi_launch_dry_run(int on) { return launch_dry_run(on); }

int64_t gs_semi_launch_record(char* buf, int64_t cap) { return launch_record_take(buf, cap); }

} // extern "C"
