/* gpusolve_line.h — the z-line Jacobi smoother (libgpusolve_line.so). Added; not a reference operator. The driver
 * runs it in place of the point sweeps when a grid's smoother is GS_SMOOTHER_ZLINE (gs_grid_set_smoother of
 * include/gpusolve_driver.h); nothing else in the product calls it.
 *
 * One sweep solves, for every column (x, y), the tridiagonal system the stencil's centre and its two z-neighbours
 * form along z, with the four x / y neighbours taken from the input iterate (Jacobi across columns), and relaxes
 * towards that solution with omega. For A the LINEAR operator (stencil . u / h^2, no gamma term), s0 the centre
 * weight, `up` the weight at (0, 0, +1) and `lo` the weight at (0, 0, -1):
 *
 *     tables (gs_zline_factors, host):   den[1] = s0,  cp[k] = up / den[k],  den[k+1] = s0 - lo * cp[k]
 *     per column, k = 1 .. nz:
 *       g_k = the four products s_i * v_in(neighbour i) of the entries with oz = 0 other than the centre, in
 *             config order; the first product starts the sum, each further one is added to it
 *       b_k = (h*h) * f_k - g_k
 *       d_1 = b_1 / den[1],   d_k = (b_k - lo * d_{k-1}) / den[k]            (forward pass, k ascending)
 *       u_nz = d_nz,          u_k = d_k - cp[k] * u_{k+1}                    (backward pass, k descending)
 *       v_out_k = v_k + omega * (u_k - v_k)
 *     zero iterate (v_in == NULL):  b_k = (h*h) * f_k  and  v_out_k = omega * u_k
 *
 * as written: every product, sum and quotient is rounded once (the library is built with -ffp-contract=off), the
 * quotients are IEEE divisions, no reciprocal is tabulated. tests/zline_ref.py restates it word for word and the
 * device equals it bit for bit. The zero iterate gives the values a zeroed field gives under ==; the SIGN of a zero
 * may differ (a zeroed field's g_k is a signed zero and v + omega * u adds +0: -0 results become +0 there).
 *
 * d lives in v_out between the two passes: each element is written in the forward pass and read back, then
 * overwritten with the result, by the lane that wrote it. One launch per sweep; no field beyond v_in's ping-pong
 * partner is needed. The instance for few, long columns (k_zline_lds, below) keeps d in LDS instead: it never reads
 * v_out and writes each interior element once, with the result.
 *
 * Conventions of gpusolve_hip.h: asynchronous on `stream`, no allocation, no copy, no synchronisation, no environment
 * variable; 0, GS_EINVAL or a hipError_t. Layout contract: any legal pitch and any 8-byte-aligned field pointer;
 * v_in and f are read inside the readable extent of gpusolve_hip.h only (clamped indices; a pair load may touch the
 * one element after a padded row), as is v_out where it is read back; the ring of v_in must hold zeros, f's ring may
 * hold anything; exactly the interior points of v_out are written. Whole levels (z0 = 0). A level with an empty
 * axis: 0, nothing launched.
 */
#ifndef GPUSOLVE_LINE_H
#define GPUSOLVE_LINE_H

#include <stdint.h>
#include "gpusolve_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The factors of one level, in device memory: nz + 2 doubles each (entries 0 and nz + 1 are 0), as gs_zline_factors
 * fills them for the stencil the sweep is called with, and the nz they were built for. */
typedef struct {
    const double* cp;
    const double* den;
    int64_t nz;
} gs_zline_tables;

/* 1 when a z-line sweep of S is defined: the seven entries are the seven offsets (0,0,0), (+-1,0,0), (0,+-1,0),
 * (0,0,+-1), once each, in any order, and s0 != 0, |s0| >= |up| + |lo| (a NaN weight there fails the comparison).
 * Elimination without pivoting then never meets a zero denominator: |den_k| >= |s0| - |lo| >= |up| keeps
 * |cp[k]| <= 1, so |den_{k+1}| >= |s0| - |lo| again (and den_k != 0 even where up = lo = 0). Else 0. */
int gs_zline_supported(const gs_stencil* S);

/* Pure host code: cp[0 .. nz+1] and den[0 .. nz+1] by the recurrence above (nz >= 0). GS_EINVAL, nothing written,
 * for a NULL pointer, nz < 0 or a stencil gs_zline_supported refuses. */
int gs_zline_factors(const gs_stencil* S, int64_t nz, double* cp, double* den);

/* One sweep, v_in -> v_out. v_in == NULL: the zero iterate, not read. GS_EINVAL, nothing written: a stencil
 * gs_zline_supported refuses, a bad level or z0 != 0, NULL v_out / f / tables / table pointers, tables->nz != L->nz,
 * v_out sharing a word of its padded box with v_in or f. */
int gs_zline_sweep(const gs_stencil* S, const gs_level* L, double omega, const double* v_in, double* v_out,
                   const double* f, const gs_zline_tables* tables, hipStream_t stream);

/* The kernel instance gs_zline_sweep launches for (S, L, v_in == NULL ? zero : !zero): "k_zline_march<zero>" — a lane
 * owns a pair of columns and marches up, then down, with a register ring of planes in flight; canonical stencil
 * order and at least 32 * 32 columns — "k_zline_lds<zero>" — a block owns eight columns, keeps their state in LDS
 * and runs the two recurrences out of it; fewer than 32 * 32 columns and 64 <= nz <= 1536, in any order — or
 * "k_zline_col<zero>" (a thread owns one column: every other level); "" for arguments the sweep refuses and for a
 * level with an empty axis. The three compute the same words. */
const char* gs_zline_kernel(const gs_stencil* S, const gs_level* L, int zero);

#ifdef __cplusplus
}
#endif
#endif /* GPUSOLVE_LINE_H */
