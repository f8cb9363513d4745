// gs_krylov.hip — libgpusolve_krylov.so: the launchers of include/gpusolve_krylov.h (semantics and evaluation order
// there). Its own library and header: libgpusolve_hip.so's export list and its kernels stay what they are.
// gs_device.hpp gives Coef, the point expressions, the one-point passes' launch plan and the launch helpers. As in
// libgpusolve_transfer.so, the include brings two things along: that header's non-template kernels (k_restrict,
// k_copy, k_sumsq_finish, ...) are compiled into this library as code objects nothing here launches, and its Knobs
// are read from the environment once, when the library is loaded. pass_plan and make_coef consult them, so
// GS_RB_ZC and GS_NO_UNIT_STENCIL steer gs_pcg_dir's instance and chunk as they steer the one-point passes; no
// launcher reads the environment itself.
#include "gs_krylov_device.hpp"

namespace {

// whole levels only; the kernels index planes with 32-bit z and the grids' y / z extents are 16-bit
bool bad_krylov_level(const gs_level* L) { return bad_level(L) || L->z0 != 0; }

bool empty_level(const gs_level* L) { return L->nx == 0 || L->ny == 0 || L->nz == 0; }

// the padded boxes [a, a + span) and [b, b + span) share a word
bool overlap(const gs_level* L, const double* a, const double* b)
{
    const int64_t span = (L->nz + 2) * L->ldz;
    return a < b + span && b < a + span;
}

// gs_pcg_dir takes the z-march where the one-point passes of gpusolve_hip.h do (pass_plan: canonical stencil order
// and at least 1024 blocks of 4-plane chunks), with their chunk rule
PassPlan dir_plan(const gs_stencil* S, const gs_level* L) { return pass_plan(S, L); }

// the element-wise passes: 128 x KV_BY points per block and plane, chunks of 1..16 planes for ~4096 blocks
struct VecPlan {
    int zc;
    dim3 grid;
};
VecPlan vec_plan(const gs_level* L)
{
    const int64_t tiles = ((L->nx + 2 * WAVE - 1) / (2 * WAVE)) * ((L->ny + KV_BY - 1) / KV_BY);
    int64_t zc = L->nz * tiles / 4096;
    zc = zc < 1 ? 1 : (zc > 16 ? 16 : zc);
    return VecPlan{(int)zc, dim3((unsigned)((L->nx + 2 * WAVE - 1) / (2 * WAVE)), (unsigned)((L->ny + KV_BY - 1) / KV_BY),
                                 (unsigned)((L->nz + zc - 1) / zc))};
}
int64_t blocks(dim3 g) { return (int64_t)g.x * g.y * g.z; }
bool bad_grid(dim3 g) { return g.y > 65535u || g.z > 65535u; }

} // namespace

extern "C" {

int64_t gs_pcg_dir_num_partials(const gs_stencil* S, const gs_level* L)
{
    if (!S || !valid_stencil(S) || bad_krylov_level(L) || empty_level(L)) return 0;
    return blocks(dir_plan(S, L).grid);
}

const char* gs_pcg_dir_kernel(const gs_stencil* S, const gs_level* L, int first)
{
    if (!S || !valid_stencil(S) || bad_krylov_level(L) || empty_level(L)) return "";
    const PassPlan plan = dir_plan(S, L);
    if (bad_grid(plan.grid)) return "";
    if (!plan.rb) return first ? "k_pcg_dir_gen<true>" : "k_pcg_dir_gen<false>";
    const Coef k = make_coef(S, L, 0.0, 0.0);
    if (k.unit) return first ? "k_pcg_dir_rb<true, true>" : "k_pcg_dir_rb<true, false>";
    return first ? "k_pcg_dir_rb<false, true>" : "k_pcg_dir_rb<false, false>";
}

int gs_pcg_dir(const gs_stencil* S, const gs_level* L, const double* z, const double* p_in, double* p_out, double* q,
               const double* beta_dev, double* partials, hipStream_t st)
{
    if (!S || !valid_stencil(S) || bad_krylov_level(L) || !z || !p_out || !q || !partials || (p_in && !beta_dev))
        return GS_EINVAL;
    if (overlap(L, p_out, z) || overlap(L, q, z) || overlap(L, p_out, q) ||
        (p_in && (overlap(L, p_out, p_in) || overlap(L, q, p_in))))
        return GS_EINVAL;
    if (empty_level(L)) return 0;
    const PassPlan plan = dir_plan(S, L);
    if (bad_grid(plan.grid)) return GS_EINVAL;
    const Coef k = make_coef(S, L, 0.0, 0.0);
    const int nx = (int)L->nx, ny = (int)L->ny, nz = (int)L->nz;
    if (plan.rb) {
        with_bools([&](auto U, auto F) {
            launch((k_pcg_dir_rb<U, F, RB_RY, RB_W>), plan.grid, dim3(WAVE, RB_W), st, k, z, p_in, p_out, q, beta_dev,
                   partials, nx, ny, nz, L->ldy, L->ldz, plan.zc);
        }, k.unit != 0, p_in == nullptr);
    } else {
        with_bools([&](auto F) {
            launch((k_pcg_dir_gen<F>), plan.grid, dim3(GN_BX, GN_BY), st, k, z, p_in, p_out, q, beta_dev, partials, nx,
                   ny, nz, L->ldy, L->ldz);
        }, p_in == nullptr);
    }
    return launch_status();
}

int64_t gs_pcg_step_num_partials(const gs_level* L)
{
    if (bad_krylov_level(L) || empty_level(L)) return 0;
    return blocks(vec_plan(L).grid);
}

int gs_pcg_step(const gs_level* L, double* x, double* r, const double* p, const double* q, const double* alpha_dev,
                double* partials, hipStream_t st)
{
    if (bad_krylov_level(L) || !x || !r || !p || !q || !alpha_dev || !partials) return GS_EINVAL;
    if (overlap(L, x, r) || overlap(L, x, p) || overlap(L, x, q) || overlap(L, r, p) || overlap(L, r, q))
        return GS_EINVAL;
    if (empty_level(L)) return 0;
    const VecPlan plan = vec_plan(L);
    if (bad_grid(plan.grid)) return GS_EINVAL;
    launch(k_pcg_step, plan.grid, dim3(WAVE, KV_BY), st, x, r, p, q, alpha_dev, partials, (int)L->nx, (int)L->ny,
           (int)L->nz, L->ldy, L->ldz, plan.zc);
    return launch_status();
}

int64_t gs_dot_num_partials(const gs_level* L) { return gs_pcg_step_num_partials(L); }

int gs_krylov_vec_chunk(const gs_level* L)
{
    if (bad_krylov_level(L) || empty_level(L)) return 0;
    const VecPlan plan = vec_plan(L);
    return bad_grid(plan.grid) ? 0 : plan.zc;
}

int gs_dot(const gs_level* L, const double* a, const double* b, double* partials, hipStream_t st)
{
    if (bad_krylov_level(L) || !a || !b || !partials) return GS_EINVAL;
    if (empty_level(L)) return 0;
    const VecPlan plan = vec_plan(L);
    if (bad_grid(plan.grid)) return GS_EINVAL;
    launch(k_dot, plan.grid, dim3(WAVE, KV_BY), st, a, b, partials, (int)L->nx, (int)L->ny, (int)L->nz, L->ldy, L->ldz,
           plan.zc);
    return launch_status();
}

int gs_pcg_scalars(int what, const double* partials, int64_t n, double* rec, double* slot, hipStream_t st)
{
    if (what < GS_PCG_PQ || what > GS_PCG_RZ_FIRST || n < 0 || (n > 0 && !partials) || !rec) return GS_EINVAL;
    launch(k_pcg_scalars, dim3(1), dim3(FIN_T), st, what, partials, n, rec, slot);
    return launch_status();
}

} // extern "C"
