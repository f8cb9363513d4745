/* gpusolve_semi.h — XY semi-coarsening (libgpusolve_semi.so). Added; not reference operators. The driver calls it on
 * grids created with GS_COARSEN_XY (gs_grid_create_coarsen of include/gpusolve_driver.h); nothing
 * else in the product does.
 *
 * An XY hierarchy coarsens x and y by two per level (n -> n / 2, integer division) and keeps nz. Two things follow:
 * every level has its own stencil (gs_semi_level_stencil), and the grid transfers do not touch z (the _xy launchers).
 *
 * Level stencils. For a level of mesh width hl under a level 0 of mesh width h0 (gs_level.h: 1 / (ny + 1)), and S the
 * configuration's stencil with centre s0, z weights up (at (0,0,+1)) and lo (at (0,0,-1)) and x / y weights
 * w_a .. w_d in config order, evaluated in double as written, every operation rounded once:
 *     q = hl / h0          r = q * q
 *     up_l = r * up        lo_l = r * lo        the x / y weights: S's words
 *     s0_l = r * s0 + (r - 1.0) * (((w_a + w_b) + w_c) + w_d)
 * Entry order and offsets are S's. Level 0 (r = 1.0) is S word for word: r * x = x, and (r - 1.0) * sum is a zero,
 * which added to r * s0 leaves it (s0 = -0.0 aside). This is the re-discretisation of Lx + Ly at hl with Lz and the
 * zeroth-order part of the centre kept at h0, in units of 1 / hl^2: the operator of level l is stencil_l . u / hl^2.
 * On sizes 2^k - 1 in y, q = 2^l and r = 4^l exactly.
 *
 * Transfers, for a transition fine (nx, ny, nz) -> coarse (nx / 2, ny / 2, nz): the tables, weights and evaluation
 * order of include/gpusolve_transfer.h on axes 0 and 1, X pass then Y pass, and no Z pass — plane z of the coarse
 * level comes from plane z of the fine level alone and the other way round. A gs_transfer_tables describes the
 * transition: axes 0 and 1 as there (gs_transfer_axis' arrays, uploaded); axis 2 must have nf = nc = nz and NULL
 * arrays. By-position tables make every size work; on an aligned axis (n = 2m + 1) the weights are (1/4, 1/2, 1/4)
 * and (1/2, 1/2) exactly.
 *
 * Launchers: whole levels (z0 = 0); the conventions of gpusolve_hip.h — asynchronous on `stream`, no allocation, no
 * synchronisation, no environment variable, 0 or GS_EINVAL / a hipError_t — and its layout contract: any legal pitch
 * and any 8-byte-aligned field pointer, results depend only on the padded boxes (of f: interior points only), exactly
 * the documented set is written, reads stay inside planes 0 .. nz+1, rows 0 .. ny+1, columns 0 .. nx+1 of every
 * field. A bad level, a null pointer, a coarse level that is not (nx / 2, ny / 2, nz), nx or ny below 2, nz above
 * 65535, z0 != 0 or tables that do not match the levels as described: GS_EINVAL and nothing is written. nz = 0: 0 and
 * nothing is launched.
 */
#ifndef GPUSOLVE_SEMI_H
#define GPUSOLVE_SEMI_H

#include <stdint.h>
#include "gpusolve_hip.h"
#include "gpusolve_transfer.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Pure host code (no device): *out = the stencil of a level of mesh width hl, by the rule above. GS_EINVAL, nothing
 * written: a NULL pointer, h0 or hl not a positive finite number, or a stencil whose seven entries are not the seven
 * offsets (0,0,0), (+-1,0,0), (0,+-1,0), (0,0,+-1) once each (gs_zline_supported's shape test, without its dominance
 * test). out may be S. */
int gs_semi_level_stencil(const gs_stencil* S, double h0, double hl, gs_stencil* out);

/* coarse interior = R_xy fine (a stored field to a stored field). */
int gs_restrict_xy(const double* fine, const gs_level* fl, double* coarse, const gs_level* cl,
                   const gs_transfer_tables* T, hipStream_t stream);

/* fine_v interior += P_xy coarse_v: per fine point the X pass  pa_x * c[jx] + pt_x * c[jx + 1]  on coarse rows jy and
 * jy + 1, then the Y pass  pa_y * (row jy) + pt_y * (row jy + 1), both products and the add as written. The coarse
 * ring takes part as data (it holds zeros). */
int gs_prolong_add_xy(const double* coarse_v, const gs_level* cl, double* fine_v, const gs_level* fl,
                      const gs_transfer_tables* T, hipStream_t stream);

/* coarse_f interior = R_xy (f - A v), A the LINEAR operator of S on fl (stencil . v / h^2), the fine residual never
 * stored: gs_residual's point expression, gs_restrict_xy's sums — bit-identical to gs_residual (mode GS_LINEAR)
 * followed by gs_restrict_xy. S: any stencil gs_residual takes. v's ring is read (it holds zeros), f's is not. */
int gs_residual_restrict_xy(const gs_stencil* S, const gs_level* fl, const double* v, const double* f,
                            double* coarse_f, const gs_level* cl, const gs_transfer_tables* T, hipStream_t stream);
/* The z-chunk gs_residual_restrict_xy launches with on (fl, cl): planes per block, 8..64, from the plan function the
 * launcher takes its grid from (block z index b covers planes b * chunk + 1 .. min(nz, (b + 1) * chunk)). Launches
 * nothing and needs no device; 0 for levels the launcher refuses and for nz = 0. */
int gs_residual_restrict_xy_chunk(const gs_level* fl, const gs_level* cl);

/* The kernel a launcher enqueues for (fl, cl): each has one instance, for every shape.
 *   GS_SEMI_RESIDUAL_RESTRICT  "k_resrestrict_xy"  a block owns 64 x 4 coarse columns and marches a chunk of planes:
 *                              v tile with a one-point halo in a three-plane LDS ring, the next plane's loads in
 *                              flight in registers, the residual plane and the x-pass plane in LDS
 *   GS_SEMI_RESTRICT           "k_restrict_xy"     a thread per coarse point
 *   GS_SEMI_PROLONG_ADD        "k_prolong_add_xy"  a thread per pair of fine points (x odd, x + 1)
 * "" for an unknown `op`, for levels the launchers refuse and for nz = 0. */
enum { GS_SEMI_RESIDUAL_RESTRICT = 0, GS_SEMI_RESTRICT = 1, GS_SEMI_PROLONG_ADD = 2 };
const char* gs_semi_kernel(int op, const gs_level* fl, const gs_level* cl);

/* This library's launch record: gs_launch_dry_run / gs_launch_record of include/gpusolve_hip.h for the launchers
 * above (each library keeps its own record and its own dry-run flag). */
int gs_semi_launch_dry_run(int on);
int64_t gs_semi_launch_record(char* buf, int64_t cap);

#ifdef __cplusplus
}
#endif
#endif /* GPUSOLVE_SEMI_H */
