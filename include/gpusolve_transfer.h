/* gpusolve_transfer.h — position-aware grid transfers (libgpusolve_transfer.so). Added; not reference operators.
 *
 * The hierarchy coarsens a level of n points per axis to m = n / 2 (integer division) with h_c = 1/(m + 1): a coarse
 * grid spanning the same domain. The reference's restrict / interpolate (gs_restrict, gs_prolong_add of
 * gpusolve_hip.h) assume that fine index 2i sits on coarse index i, which holds only for n = 2m + 1. The operators
 * here interpolate by POSITION instead, and restrict with the scaled transpose, so a V-cycle converges on every size
 * (512^3 as well as 511^3). On an aligned axis (n = 2m + 1) they are the reference's operators.
 *
 * Definitions, per axis, for a transition fine n -> coarse m = n / 2; indices are padded indices (0 and n+1 the ring),
 * D = n + 1. For a fine index i = 1..n, in int64:
 *     q = i * (m + 1);  pj[i] = q / D;  rem = q % D;  pt[i] = (double)rem / (double)D;  pa[i] = 1.0 - pt[i]
 * (pj[i] + 1 <= m + 1). Aligned axis: pj = i / 2, pt = (i % 2) / 2.
 *
 * Prolongation with correction, fine_v += P d, d = coarse_v (or coarse_v - coarse_sub, formed per coarse point
 * first): separable, X then Y then Z, per axis  pa[i] * d[pj[i]] + pt[i] * d[pj[i] + 1]  — both products and the add
 * as written, no contraction. The coarse ring takes part as data (it holds zeros). Only interior fine points are
 * written.
 *
 * Restriction, with s = (double)(m + 1) / (double)D: coarse J = 1..m gathers, in ascending i, the fine interior points
 * with pj[i] = J (weight s * pa[i]) or with pj[i] = J - 1 and rem > 0 (weight s * pt[i]); each weight one multiply.
 * They are rcnt[J] <= 4 consecutive indices from rlo[J], weights rw[4 * J + k]. The axis sum is
 *     ((w0 * r0 + w1 * r1) + w2 * r2) + w3 * r3        truncated to rcnt terms, the first product starting the sum;
 * separable, X then Y then Z. No ring value of the fine field is read. Aligned axis: (1/4, 1/2, 1/4) exactly.
 *
 * Tables. gs_transfer_axis fills HOST arrays for one axis; a caller uploads them and describes them to the launchers
 * with a gs_transfer_tables: nf / nc say which transition each axis' arrays were built for (checked against the levels
 * of every call), the pointers are DEVICE pointers. Array sizes per axis: pj, pt: nf + 2 entries (index = fine padded
 * index; entries 0 and nf + 1 are 0 / 0.0 and never used); rlo, rcnt: nc + 2 entries (0 and nc + 1 unused, rcnt 0);
 * rw: 4 * (nc + 2) doubles (unused weights 0.0).
 *
 * Launchers: whole levels (z0 = 0); the conventions of gpusolve_hip.h — asynchronous on `stream`, no allocation, no
 * synchronisation, no environment variable, 0 or GS_EINVAL / a hipError_t — and its layout contract: any legal pitch,
 * results depend only on the padded boxes (of f and w: interior points only), exactly the documented set is written,
 * reads stay inside planes 0 .. nz+1, rows 0 .. ny+1, columns 0 .. nx+1 of every field. A bad level, a null pointer, a
 * coarse level that is not fine / 2 per axis, z0 != 0 or tables whose nf / nc do not match the levels: GS_EINVAL and
 * nothing is written.
 */
#ifndef GPUSOLVE_TRANSFER_H
#define GPUSOLVE_TRANSFER_H

#include <stdint.h>
#include "gpusolve_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    int64_t nf[3], nc[3];  /* per axis (x, y, z): the transition the arrays were built for */
    const int32_t* pj[3];  /* device pointers, see above */
    const double* pt[3];
    const int32_t* rlo[3];
    const int32_t* rcnt[3];
    const double* rw[3];
} gs_transfer_tables;

/* One axis' tables into host arrays of the sizes above. Pure host code (no device). GS_EINVAL unless nf >= 2,
 * nc == nf / 2 and every pointer is non-null. */
int gs_transfer_axis(int64_t nf, int64_t nc, int32_t* pj, double* pt, int32_t* rlo, int32_t* rcnt, double* rw);

/* coarse_a (and coarse_b unless NULL) interior = R fine (a stored field; gs_restrict2's role). */
int gs_restrict_pa(const double* fine, const gs_level* fl, double* coarse_a, double* coarse_b, const gs_level* cl,
                   const gs_transfer_tables* T, hipStream_t stream);

/* fine_v interior += P (coarse_v - coarse_sub) (coarse_sub may be NULL; gs_prolong_add's role). */
int gs_prolong_add_pa(const double* coarse_v, const double* coarse_sub, const gs_level* cl, double* fine_v,
                      const gs_level* fl, const gs_transfer_tables* T, hipStream_t stream);

/* coarse_f interior = R (f - A v) with the fine residual never stored (gs_residual_restrict's role): every mode
 * gs_residual takes, its point expressions; w as there. LINEAR: bit-identical to gs_residual followed by
 * gs_restrict_pa. */
int gs_residual_restrict_pa(const gs_stencil* S, const gs_level* fl, int mode, double gamma, const double* v,
                            const double* f, const double* w, double* coarse_f, const gs_level* cl,
                            const gs_transfer_tables* T, hipStream_t stream);
/* The z-chunk gs_residual_restrict_pa launches with on (fl, cl): COARSE planes per block, 4..32, from the plan
 * function the launcher takes its grid from (block z index b covers coarse planes b * chunk + 1 ..
 * min(cnz, (b + 1) * chunk)). Launches nothing and needs no device; 0 for levels the launcher refuses. */
int gs_residual_restrict_pa_chunk(const gs_level* fl, const gs_level* cl);

/* ---- Full multigrid's prolongation of a SOLUTION by position (gs_fmg_prolong's role on transitions that are not
 * aligned). Tricubic, separable, X then Y then Z. Per axis, with q, pj, rem, D as above and
 * P = m + 2 the number of padded coarse values:
 *     P >= 4: K = 4, cj[i] = clamp(pj - 1, 0, P - 4);      P = 3 (m = 1): K = 3, cj[i] = 0
 *     t = (double)(pj - cj[i]) + (double)rem / (double)D      the point's coordinate in the nodes cj .. cj + K - 1
 * and the Lagrange weights, each evaluated in double as written, left to right:
 *     K = 4: w0 = -(((t-1)*(t-2))*(t-3))/6   w1 = ((t*(t-2))*(t-3))/2   w2 = -((t*(t-1))*(t-3))/2   w3 = ((t*(t-1))*(t-2))/6
 *     K = 3: w0 = ((t-1)*(t-2))/2            w1 = -(t*(t-2))            w2 = (t*(t-1))/2            w3 = 0.0
 * The axis value is  ((w0 * c[cj] + w1 * c[cj+1]) + w2 * c[cj+2]) + w3 * c[cj+3]  truncated to K terms, the first
 * product starting the sum, no contraction. The coarse ring takes part as data; only interior fine points are written;
 * no read leaves the padded coarse box. On an aligned axis this is gs_fmg_prolong's cubic up to rounding (not bit for
 * bit: the weights are evaluated, not the constants 5/16, 15/16, ...).
 *
 * gs_fmg_axis fills HOST arrays for one axis: cj, nf + 2 entries, and cw, 4 * (nf + 2) doubles (w0..w3 of fine index
 * i at cw[4 * i]); entries 0 and nf + 1 are zero. gs_fmg_tables describes uploaded copies as gs_transfer_tables does. */
typedef struct {
    int64_t nf[3], nc[3]; /* per axis (x, y, z): the transition the arrays were built for */
    const int32_t* cj[3]; /* device pointers */
    const double* cw[3];
} gs_fmg_tables;

/* Pure host code (no device). GS_EINVAL, with nothing written, unless nf >= 2, nc == nf / 2 and both pointers are
 * non-null. */
int gs_fmg_axis(int64_t nf, int64_t nc, int32_t* cj, double* cw);

/* fine interior = P coarse (whole levels; any transition with coarse = fine / 2 per axis, aligned axes included).
 * The launchers' conventions and layout contract above. */
int gs_fmg_prolong_pa(const double* coarse, const gs_level* cl, double* fine, const gs_level* fl,
                      const gs_fmg_tables* T, hipStream_t stream);
/* The z-chunk gs_fmg_prolong_pa launches with on (fl, cl): FINE planes per block, an even number in 16..128, from the
 * plan function the launcher takes its grid from. Above 16 only where the level's blocks at 16 planes fill the
 * device, and then the device's choice (the kernel's occupancy x its compute units; without a device 256 units of
 * one block each are assumed). Launches nothing; 0 for levels the launcher refuses. */
int gs_fmg_prolong_pa_chunk(const gs_level* fl, const gs_level* cl);

/* This library's launch record: gs_launch_dry_run / gs_launch_record of include/gpusolve_hip.h for the launchers
 * above (each library keeps its own record and its own dry-run flag). */
int gs_transfer_launch_dry_run(int on);
int64_t gs_transfer_launch_record(char* buf, int64_t cap);

#ifdef __cplusplus
}
#endif
#endif /* GPUSOLVE_TRANSFER_H */
