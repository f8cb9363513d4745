/* gpusolve_krylov.h — the level-0 passes of multigrid-preconditioned conjugate gradients (libgpusolve_krylov.so).
 * Added; not reference operators. The driver composes them with the V-cycle as preconditioner (gs_grid_pcg of
 * include/gpusolve_driver.h); nothing else in the product calls them.
 *
 * One PCG iteration, for A the LINEAR operator (stencil . u / h^2, no gamma term) and M^-1 one V-cycle from zero:
 *     p = z + beta p_old,  q = A p,  pq = p . q                    gs_pcg_dir       32 B per point
 *     alpha = rz / pq                                              gs_pcg_scalars(GS_PCG_PQ)
 *     x += alpha p,  r -= alpha q,  rr = r . r                     gs_pcg_step      48 B per point
 *     (record the iteration, hand rr to the host)                  gs_pcg_scalars(GS_PCG_RR)
 *     z = M^-1 r                                                   (the caller's cycle)
 *     rz' = r . z                                                  gs_dot           16 B per point
 *     beta = rz' / rz,  rz = rz'                                   gs_pcg_scalars(GS_PCG_RZ)
 *
 * Conventions of gpusolve_hip.h: asynchronous on `stream`, no allocation, no copy, no synchronisation, no environment
 * variable; 0, GS_EINVAL or a hipError_t. Layout contract: any legal pitch and any 8-byte-aligned field pointer; inputs
 * are read inside their padded boxes only (a pair load may touch the one element after a padded row, as the one-point
 * passes of gpusolve_hip.h do, and its value reaches no result) and their rings must hold zeros; exactly the interior
 * points of the outputs are written. Whole levels (z0 = 0). A level with an empty axis: 0, nothing launched, and its
 * partial count is 0.
 *
 * Arithmetic, as written, no contraction: p_out = z + (beta * p_in); q = S(p_out) / h^2 with S the stencil sum of
 * gs_apply_op (config order, the unit-neighbour form where it applies, the same division); x + (alpha * p);
 * r - (alpha * q). Every dot product is summed in a fixed order — per lane, per wave, per block into partials[block],
 * then by gs_pcg_scalars in the strided order of gs_sumsq_finish — so a run repeats bit for bit. No atomics.
 */
#ifndef GPUSOLVE_KRYLOV_H
#define GPUSOLVE_KRYLOV_H

#include <stdint.h>
#include "gpusolve_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The device-resident record gs_pcg_scalars keeps (GS_PCG_REC doubles), and the layout of a history slot. */
enum { GS_PCG_RZ_I = 0, GS_PCG_PQ_I = 1, GS_PCG_ALPHA_I = 2, GS_PCG_BETA_I = 3, GS_PCG_RR_I = 4, GS_PCG_FLAG_I = 5,
       GS_PCG_REC = 8 };
/* flag bits (the flag is stored as a double holding a small integer; it is sticky until GS_PCG_RZ_FIRST):
 * p . q, r . z not a positive finite number; r . r not finite (the updated residual overflowed or holds a NaN) */
enum { GS_PCG_BAD_PQ = 1, GS_PCG_BAD_RZ = 2, GS_PCG_BAD_RR = 4 };
/* what gs_pcg_scalars does with the sum s of the partials */
enum {
    GS_PCG_PQ = 0,       /* pq = s; alpha = rz / pq */
    GS_PCG_RR = 1,       /* rr = s (0 and GS_PCG_BAD_RR if s is not finite); the record is copied to `slot` */
    GS_PCG_RZ = 2,       /* beta = s / rz; rz = s */
    GS_PCG_RZ_FIRST = 3  /* a new run: flag = 0, rz = s, beta = 0, pq = alpha = rr = 0 */
};

/* p_out = z + beta p_in (beta = *beta_dev, read on the device; p_in == NULL: p_out = z, neither p_in nor beta_dev
 * is read), q = A p_out, partials[b] = block b's part of p_out . q (gs_pcg_dir_num_partials of them). The neighbours
 * of a point are formed from z and p_in, so p_out and q must not alias z, p_in or each other: GS_EINVAL. Any stencil
 * with offsets in {-1, 0, 1}^3. */
int gs_pcg_dir(const gs_stencil* S, const gs_level* L, const double* z, const double* p_in, double* p_out, double* q,
               const double* beta_dev, double* partials, hipStream_t stream);
int64_t gs_pcg_dir_num_partials(const gs_stencil* S, const gs_level* L);
/* the kernel instance gs_pcg_dir launches for (S, L, p_in == NULL ? first : !first): "k_pcg_dir_rb<unit, first>" (the
 * register-blocked z-march) or "k_pcg_dir_gen<first>" (one point per thread); "" for arguments it refuses. */
const char* gs_pcg_dir_kernel(const gs_stencil* S, const gs_level* L, int first);

/* x += alpha p, r -= alpha q in place (alpha = *alpha_dev), partials[b] = block b's part of the new r . r. With
 * alpha == 0 no word of x or r is written. x and r must not alias each other, p or q: GS_EINVAL. */
int gs_pcg_step(const gs_level* L, double* x, double* r, const double* p, const double* q, const double* alpha_dev,
                double* partials, hipStream_t stream);
int64_t gs_pcg_step_num_partials(const gs_level* L);

/* partials[b] = block b's part of a . b over the interior (a == b allowed). */
int gs_dot(const gs_level* L, const double* a, const double* b, double* partials, hipStream_t stream);
int64_t gs_dot_num_partials(const gs_level* L);

/* The z-chunk gs_pcg_step and gs_dot launch with on L: planes per block, 1..16, from the plan function the two
 * launchers take their grid from. Block (bx, by, bz) covers planes bz * chunk + 1 .. min(nz, (bz + 1) * chunk) and
 * writes partials[(bz * gy + by) * gx + bx]. Launches nothing and needs no device; 0 for a level they refuse or an
 * empty one. */
int gs_krylov_vec_chunk(const gs_level* L);

/* One block: s = the sum of partials[0 .. n-1] (n >= 0), then the update of `rec` (GS_PCG_REC doubles of device
 * memory) that `what` names. Quotients are IEEE divisions. A sum that decides a quotient (p . q, r . z) must be a
 * positive finite number: otherwise, or once the flag is set, the quotient is stored as 0 and the sum's flag bit is
 * set — alpha and beta never hold a NaN or an infinity. A sum that is not finite is recorded as 0 and sets its flag
 * bit, r . r's GS_PCG_BAD_RR included: a reader of the record tells that 0 from a residual that vanished by the flag.
 * GS_PCG_RR also copies the record to slot[0 .. GS_PCG_REC-1] unless slot is NULL (device-visible memory: the
 * driver passes a slot of its mapped, coherent pinned history). */
int gs_pcg_scalars(int what, const double* partials, int64_t n, double* rec, double* slot, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GPUSOLVE_KRYLOV_H */
