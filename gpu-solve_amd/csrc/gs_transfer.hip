// gs_transfer.hip — libgpusolve_transfer.so: the position-aware grid transfers of include/gpusolve_transfer.h
// (definitions and evaluation order there). Its own library and header: libgpusolve_hip.so's export list and its
// kernels stay what they are. gs_device.hpp gives Coef, the residual's point expressions and the launch helpers.
#include "gs_device.hpp"
#include "gs_transfer_device.hpp"

#include "gpusolve_transfer.h"

namespace {

// whole levels, coarse = fine / 2 per axis
bool bad_pair(const gs_level* fl, const gs_level* cl)
{
    if (bad_level(fl) || bad_level(cl) || fl->z0 != 0 || cl->z0 != 0) return true;
    const int64_t nf[3] = {fl->nx, fl->ny, fl->nz}, nc[3] = {cl->nx, cl->ny, cl->nz};
    for (int a = 0; a < 3; a++)
        if (nf[a] < 2 || nc[a] != nf[a] / 2) return true;
    return false;
}

// one block per plane (transfers) / per PA_TYC coarse rows: the grid's y and z extents
bool bad_pa_grid(const gs_level* fl) { return fl->nz > 65535 || (fl->ny + 3) / 4 > 65535; }

bool bad_transfer(const gs_level* fl, const gs_level* cl, const gs_transfer_tables* T)
{
    if (bad_pair(fl, cl) || !T) return true;
    const int64_t nf[3] = {fl->nx, fl->ny, fl->nz}, nc[3] = {cl->nx, cl->ny, cl->nz};
    for (int a = 0; a < 3; a++) {
        if (T->nf[a] != nf[a] || T->nc[a] != nc[a]) return true;
        if (!T->pj[a] || !T->pt[a] || !T->rlo[a] || !T->rcnt[a] || !T->rw[a]) return true;
    }
    return bad_pa_grid(fl);
}

PaTables device_tables(const gs_transfer_tables* T)
{
    PaTables d;
    for (int a = 0; a < 3; a++) {
        d.pj[a] = T->pj[a];
        d.pt[a] = T->pt[a];
        d.rlo[a] = T->rlo[a];
        d.rcnt[a] = T->rcnt[a];
        d.rw[a] = T->rw[a];
    }
    return d;
}

// (the kernel's 32-bit offsets inside a staged tile)
bool bad_fmg_pair(const gs_level* fl, const gs_level* cl) { return bad_pair(fl, cl) || cl->ldy > INT32_MAX / 16; }

bool bad_fmg_transfer(const gs_level* fl, const gs_level* cl, const gs_fmg_tables* T)
{
    if (bad_fmg_pair(fl, cl) || !T) return true;
    const int64_t nf[3] = {fl->nx, fl->ny, fl->nz}, nc[3] = {cl->nx, cl->ny, cl->nz};
    for (int a = 0; a < 3; a++) {
        if (T->nf[a] != nf[a] || T->nc[a] != nc[a]) return true;
        if (!T->cj[a] || !T->cw[a]) return true;
    }
    return false;
}

// gs_fmg_prolong_pa's launch shape. Non-temporal fine stores for a stream larger than the Infinity Cache, as
// gs_fmg_prolong (GS_FMG_NT: A/B). Fine planes per block: 16 on levels that do not fill the chip, else the even chunk
// of 16..128 that makes the grid whole rounds of resident blocks (fit_chunk; a chunk stages about three coarse
// planes, six fine ones, more than it covers)
struct FqPlan {
    bool nt;
    int zc;
    dim3 grid;
};
FqPlan fq_plan(const gs_level* fl)
{
    const bool nt = kKnobs.fmgNt < 0 ? fl->nx * fl->ny * fl->nz >= ((int64_t)1 << 25) : kKnobs.fmgNt != 0;
    const int64_t tiles = ((fl->nx + 2 * FQ_TX - 1) / (2 * FQ_TX)) * ((fl->ny + 2 * FQ_TY - 1) / (2 * FQ_TY));
    const auto fn = nt ? k_fmg_prolong_pa<true> : k_fmg_prolong_pa<false>;
    int zc = fit_chunk(tiles, fl->nz, resident_blocks((const void*)fn, FQ_T), 16, 128, true, 6.0);
    if (zc < 16) zc = tiles >= 256 && fl->nz >= 256 ? 64 : 16; // (GS_FIT_ROUNDS=0)
    return FqPlan{nt, zc,
                  dim3((unsigned)((fl->nx + 2 * FQ_TX - 1) / (2 * FQ_TX)),
                       (unsigned)((fl->ny + 2 * FQ_TY - 1) / (2 * FQ_TY)), (unsigned)((fl->nz + zc - 1) / zc))};
}

// gs_residual_restrict_pa's: z-chunks of 4..32 coarse planes, for ~1024 blocks where the level has them
struct PaPlan {
    int zc;
    dim3 grid;
};
PaPlan pa_plan(const gs_level* cl)
{
    const int64_t tiles = ((cl->nx + PA_TXC - 1) / PA_TXC) * ((cl->ny + PA_TYC - 1) / PA_TYC);
    int64_t zc = cl->nz * tiles / 1024;
    zc = zc < 4 ? 4 : (zc > 32 ? 32 : zc);
    return PaPlan{(int)zc, dim3((unsigned)((cl->nx + PA_TXC - 1) / PA_TXC), (unsigned)((cl->ny + PA_TYC - 1) / PA_TYC),
                                (unsigned)((cl->nz + zc - 1) / zc))};
}

} // namespace

extern "C" {

int gs_transfer_axis(int64_t nf, int64_t nc, int32_t* pj, double* pt, int32_t* rlo, int32_t* rcnt, double* rw)
{
    if (nf < 2 || nf > INT32_MAX / 2 || nc != nf / 2 || !pj || !pt || !rlo || !rcnt || !rw) return GS_EINVAL;
    const int64_t D = nf + 1;
    const double s = (double)(nc + 1) / (double)D;
    for (int64_t J = 0; J <= nc + 1; J++) {
        rlo[J] = 0;
        rcnt[J] = 0;
        for (int k = 0; k < 4; k++) rw[4 * J + k] = 0.0;
    }
    pj[0] = pj[nf + 1] = 0;
    pt[0] = pt[nf + 1] = 0.0;
    // fine point i feeds coarse pj[i] + 1 (weight s * pt[i], if rem > 0) and coarse pj[i] (weight s * pa[i]): taken in
    // ascending i, every coarse point's list comes out ascending, its pj = J - 1 points before its pj = J points
    auto feed = [&](int64_t J, int64_t i, double w) {
        if (J < 1 || J > nc) return true; // the coarse ring gathers nothing
        if (rcnt[J] == 0) rlo[J] = (int32_t)i;
        if (rcnt[J] >= 4 || rlo[J] + rcnt[J] != i) return false;
        rw[4 * J + rcnt[J]++] = w;
        return true;
    };
    for (int64_t i = 1; i <= nf; i++) {
        const int64_t q = i * (nc + 1), j = q / D, rem = q % D;
        pj[i] = (int32_t)j;
        pt[i] = (double)rem / (double)D;
        const double pa = 1.0 - pt[i];
        if (!feed(j, i, s * pa)) return GS_EINVAL;
        if (rem > 0 && !feed(j + 1, i, s * pt[i])) return GS_EINVAL;
    }
    return 0;
}

int gs_fmg_axis(int64_t nf, int64_t nc, int32_t* cj, double* cw)
{
    if (nf < 2 || nf > INT32_MAX / 2 || nc != nf / 2 || !cj || !cw) return GS_EINVAL;
    const int64_t D = nf + 1, P = nc + 2;
    cj[0] = cj[nf + 1] = 0;
    for (int k = 0; k < 4; k++) cw[k] = cw[4 * (nf + 1) + k] = 0.0;
    for (int64_t i = 1; i <= nf; i++) {
        const int64_t q = i * (nc + 1), pj = q / D, rem = q % D;
        const int64_t c = P >= 4 ? std::min(std::max(pj - 1, (int64_t)0), P - 4) : 0;
        const double t = (double)(pj - c) + (double)rem / (double)D;
        double* w = cw + 4 * i;
        cj[i] = (int32_t)c;
        if (P >= 4) {
            w[0] = -(((t - 1) * (t - 2)) * (t - 3)) / 6;
            w[1] = ((t * (t - 2)) * (t - 3)) / 2;
            w[2] = -((t * (t - 1)) * (t - 3)) / 2;
            w[3] = ((t * (t - 1)) * (t - 2)) / 6;
        } else {
            w[0] = ((t - 1) * (t - 2)) / 2;
            w[1] = -(t * (t - 2));
            w[2] = (t * (t - 1)) / 2;
            w[3] = 0.0;
        }
    }
    return 0;
}

int gs_fmg_prolong_pa(const double* coarse, const gs_level* cl, double* fine, const gs_level* fl,
                      const gs_fmg_tables* T, hipStream_t st)
{
    if (!coarse || !fine || bad_fmg_transfer(fl, cl, T)) return GS_EINVAL;
    const FqPlan plan = fq_plan(fl);
    const auto fn = plan.nt ? k_fmg_prolong_pa<true> : k_fmg_prolong_pa<false>;
    const int zc = plan.zc;
    const dim3 g = plan.grid, b(FQ_TX, FQ_TY);
    if (g.y > 65535u || g.z > 65535u) return GS_EINVAL;
    FqTables d;
    for (int a = 0; a < 3; a++) {
        d.cj[a] = T->cj[a];
        d.cw[a] = T->cw[a];
    }
    // the fine pair (x odd, x + 1) as one 16-byte store where the layout aligns it (gs_field_layout does)
    const int al = ((reinterpret_cast<uintptr_t>(fine + 1) & 15) == 0 && fl->ldy % 2 == 0 && fl->ldz % 2 == 0) ? 1 : 0;
    launch(fn, g, b, st, d, coarse, fine, (int)cl->nx, (int)cl->ny, (int)cl->nz, (int)fl->nx, (int)fl->ny,
                       (int)fl->nz, cl->ldy, cl->ldz, fl->ldy, fl->ldz, zc, al);
    return launch_status();
}

int gs_restrict_pa(const double* fine, const gs_level* fl, double* coarse_a, double* coarse_b, const gs_level* cl,
                   const gs_transfer_tables* T, hipStream_t st)
{
    if (!fine || !coarse_a || bad_transfer(fl, cl, T)) return GS_EINVAL;
    const dim3 g((unsigned)((cl->nx + 63) / 64), (unsigned)((cl->ny + 3) / 4), (unsigned)cl->nz), b(64, 4);
    launch(k_restrict_pa, g, b, st, device_tables(T), fine, coarse_a, coarse_b, (int)cl->nx, (int)cl->ny,
                       (int)fl->nx, (int)fl->ny, (int)fl->nz, fl->ldy, fl->ldz, cl->ldy, cl->ldz);
    return launch_status();
}

int gs_prolong_add_pa(const double* coarse_v, const double* coarse_sub, const gs_level* cl, double* fine_v,
                      const gs_level* fl, const gs_transfer_tables* T, hipStream_t st)
{
    if (!coarse_v || !fine_v || bad_transfer(fl, cl, T)) return GS_EINVAL;
    const dim3 g((unsigned)((fl->nx + 127) / 128), (unsigned)((fl->ny + 3) / 4), (unsigned)fl->nz), b(64, 4);
    with_bools([&](auto SUB) {
        launch(k_prolong_add_pa<SUB>, g, b, st, device_tables(T), coarse_v, coarse_sub, fine_v, (int)fl->nx,
                           (int)fl->ny, (int)cl->nx, (int)cl->ny, (int)cl->nz, fl->ldy, fl->ldz, cl->ldy, cl->ldz);
    }, coarse_sub != nullptr);
    return launch_status();
}

int gs_residual_restrict_pa(const gs_stencil* S, const gs_level* fl, int mode, double gamma, const double* v,
                            const double* f, const double* w, double* coarse_f, const gs_level* cl,
                            const gs_transfer_tables* T, hipStream_t st)
{
    mode = base_mode(mode); // (GS_NEWTON_G: the factor field is read; it holds gamma)
    if (!S || !valid_stencil(S) || !v || !f || !coarse_f || mode < GS_LINEAR || mode > GS_NEWTON_B ||
        (newtonish(mode) && !w) || bad_transfer(fl, cl, T))
        return GS_EINVAL;
    const Coef k = make_coef(S, fl, 0.0, gamma);
    PaStencil so;
    for (int t = 0; t < 7; t++) {
        so.lds[t] = S->ox[t] + S->oy[t] * PA_VX;
        so.oz[t] = S->oz[t];
    }
    const PaPlan plan = pa_plan(cl);
    const int zc = plan.zc;
    const dim3 g = plan.grid, b(PA_T);
    with_mode([&](auto M) {
        launch(k_resrestrict_pa<M>, g, b, st, k, so, device_tables(T), v, f, w, coarse_f, (int)fl->nx,
                           (int)fl->ny, (int)fl->nz, fl->ldy, fl->ldz, (int)cl->nx, (int)cl->ny, (int)cl->nz, cl->ldy,
                           cl->ldz, (int)zc);
    }, mode);
    return launch_status();
}

int gs_residual_restrict_pa_chunk(const gs_level* fl, const gs_level* cl)
{
    if (bad_pair(fl, cl) || bad_pa_grid(fl)) return 0;
    return pa_plan(cl).zc;
}

int gs_fmg_prolong_pa_chunk(const gs_level* fl, const gs_level* cl)
{
    if (bad_fmg_pair(fl, cl)) return 0;
    const FqPlan plan = fq_plan(fl);
    return plan.grid.y > 65535u || plan.grid.z > 65535u ? 0 : plan.zc;
}

int gs_transfer_launch_dry_run(int on) { return launch_dry_run(on); }

int64_t gs_transfer_launch_record(char* buf, int64_t cap) { return launch_record_take(buf, cap); }

} // extern "C"
