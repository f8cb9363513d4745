/* gpusolve_driver.h — C ABI of the GpuSolve-hip host driver (libgpusolve_driver.so).
 *
 * The reference's backend contract is a C++ one (a grid object + static solver functions selected
 * at compile time, src/main.cpp:5-13,88-111). This header exposes the same objects through a
 * plain C ABI (opaque handle, plain pointers and sizes) so non-C++ hosts (ctypes tests, bench.py,
 * a cgo/JNI wrapper) can drive the identical code path the GpuSolve-hip executable runs:
 *
 *   gs_grid_create         CpuGridData(const GridParams&)   src/cpu/CpuGridData.cpp:15-79
 *   gs_grid_solve          main's dispatch: NewtonSolver::solve (mode 2) else CpuSolver::solve
 *                                                          src/main.cpp:88-94
 *   gs_grid_vcycle         CpuSolver::vcycle                src/cpu/CpuSolver.cpp:85-139
 *   gs_grid_jacobi         CpuSolver::jacobi                src/cpu/CpuSolver.cpp:141-180
 *   gs_grid_residual_norm  CpuSolver::compResidual          src/cpu/CpuSolver.cpp:45-83
 *
 * Errors: functions return 0 / a non-NULL handle on success; otherwise gs_last_error() holds the
 * message the GpuSolve-hip executable would print after "Exception: ".
 */
#ifndef GPUSOLVE_DRIVER_H
#define GPUSOLVE_DRIVER_H

#include <stdint.h>
#include "gpusolve_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* GridParams (src/gridParams.h:29-47) in plain C. */
typedef struct {
    int64_t maxiter;
    double tol;
    int64_t dims[3];
    int mode; /* GS_LINEAR / GS_NONLINEAR / GS_NEWTON */
    int64_t pre, post;
    double omega, gamma;
    gs_stencil stencil;
} gs_params;

/* Parses the reference's 14-line config text. Returns 0, 1 (invalid mode), 2 (bad stencil). */
int gs_parse_config(const char* text, gs_params* out);

void* gs_grid_create(const gs_params* p); /* device-resident hierarchy on the current HIP device */
/* The coarsening, a creation-time choice (added). GS_COARSEN_XYZ: gs_grid_create, launch for launch.
 * GS_COARSEN_XY: semi-coarsening for a stencil whose z coupling is weak — level l has (nx_{l-1} / 2, ny_{l-1} / 2, nz)
 * points, nlev = floor(log2(min(nx, ny))) + 1, and its own stencil, re-discretised by gs_semi_level_stencil of
 * gpusolve_semi.h (gs_grid_level_stencil reads it; on an XYZ grid every level reports the configuration's). Every
 * transition takes the general path with that header's _xy launchers (by-position tables in x and y, built and
 * uploaded once, at creation; every size works) between the level's ordinary sweeps: point levels keep their fused
 * pairs and triples, line levels their z-line sweeps (gs_grid_set_smoother; GS_SMOOTHER_AUTO picks per level). The
 * fused prolongation pair, the tiled steps and the one-launch coarse cycle are not taken, gs_grid_set_transfer changes
 * nothing and gs_grid_fmg is refused with a reason. gs_grid_solve, gs_grid_vcycle, gs_grid_vcycle_level,
 * gs_grid_pcg (R_xy is the scaled transpose of P_xy: its conditions on the transfers hold on every size), per-sweep
 * weights, gs_grid_jacobi and gs_grid_residual_norm work as on any grid. NULL, with the reason in gs_last_error() and
 * nothing allocated: any other `coarsen`; XY with a mode other than LINEAR, a stencil that is not the seven axis
 * offsets once each, or min(nx, ny) < 2 (XY on a Z-slab / RCCL or schedule-trace grid is refused the same way where
 * GS_COARSEN asks for it). GS_COARSEN=xy|xyz in the environment when a grid is created chooses for gs_grid_create and
 * GpuSolve-hip; any other value fails the creation. gs_grid_create_coarsen does not read the variable. */
enum { GS_COARSEN_XYZ = 0, GS_COARSEN_XY = 1 };
void* gs_grid_create_coarsen(const gs_params* p, int coarsen);
int gs_grid_get_coarsen(void* grid);
/* The stencil level `level` runs with. 1 for a bad level or a NULL `out`. */
int gs_grid_level_stencil(void* grid, int level, gs_stencil* out);
void gs_grid_destroy(void* grid);

/* Runs the solve selected by the mode. print: 0 silent, 1 reference stdout lines.
 * Writes up to cap residual values (initial, then one per V-cycle / Newton iteration) into hist
 * and their total count into *count.
 *
 * What a grid holds between calls (tests/session_ref.py is this rule as a CPU model, tests/test_gpu_sessions.py holds
 * the driver to it; the model covers the operations declared below too — gs_grid_pcg, gs_grid_set_smoother, XY grids,
 * gs_grid_set_fmg_prolong, gs_grid_import / gs_grid_export and the refusals "with nothing changed" — and
 * tests/test_gpu_feature_sessions.py holds the driver to those in sequence). Level 0's v (NEWTON: newtonV) and f are
 * always the reference's. On the levels below:
 *   - gs_grid_vcycle, gs_grid_fmg and a solve that ran all its cycles (or stopped on its last one) leave every level's
 *     v and f as that last V-cycle left them: f the restricted residual (FAS: + A(restV)), v the post-smoothed iterate.
 *     NONLINEAR: v is the FAS iterate itself; the reference overwrites it with the correction v - restV
 *     (CpuSolver.cpp:121-124), which the driver only forms on the fly.
 *   - a LINEAR / NONLINEAR solve that stopped on tol BEFORE its last cycle leaves v and f of the levels >= 1
 *     unspecified: with the cycles pipelined, the next cycle's down-leg has run on them already (level 0 is restored
 *     exactly: the adoption of the speculative sweeps is undone); with GS_NO_PIPELINE or GS_NO_SPECULATION it has not.
 *     Upload a level's v and f (gs_grid_upload) or run a V-cycle from above it before reading it.
 *   - gs_grid_vcycle_level(l) reads level l's v and f and defines the levels below l; the levels above are not touched.
 *   - gs_grid_pcg (and a gs_grid_solve that GS_SOLVER=pcg sends there) leaves level 0's v = x, the last complete
 *     iteration's iterate, and level 0's f the caller's, word for word; v and f of the levels >= 1 are unspecified,
 *     exactly as after a tol-stopped solve (the preconditioner's cycles ran on them, from the residual, not from f).
 *   - NEWTON: after a solve only level 0's newtonV is defined; v and f of every level are the inner solves' work fields.
 *   - every field is handed back stored: a zero iterate the driver keeps as a flag is never visible to gs_grid_download,
 *     and gs_grid_upload of a level's v is what the next operation on that level reads. */
int gs_grid_solve(void* grid, int print, double* hist, int cap, int* count);

int gs_grid_vcycle(void* grid, double* residual);
/* One V-cycle rooted at `level` (added): the down-leg, coarse end and up-leg of gs_grid_vcycle with level `level`
 * in level 0's place — its f and v are the caller's, the levels above it are not touched, no norm is taken. The
 * same fused, tiled and coarse-launch paths as inside a whole V-cycle. Single-GPU grids. */
int gs_grid_vcycle_level(void* grid, int level);
/* Full multigrid start (added; nested iteration): every level's f becomes the full-weighting restriction of level
 * 0's f as it stands (an uploaded f is honoured); the start level (gs_grid_fmg_start_level) is iterated from zero
 * and every finer level from the tricubic prolongation (gs_fmg_prolong) of the level below, cycles_per_level
 * V-cycles each. Overwrites v on every level; *residual = the level-0 residual norm. LINEAR and NONLINEAR (FAS)
 * grids. Fails, with nothing done and the reason in gs_last_error(): a grid whose coarse grids do not align (any
 * axis not 2^k - 1: e.g. every power-of-two size), NEWTON mode, a Z-slab / RCCL grid, cycles_per_level < 1.
 * GS_FMG=k in the environment when the grid is created makes gs_grid_solve / GpuSolve-hip run this pass after the
 * initial-residual line. */
int gs_grid_fmg(void* grid, int cycles_per_level, double* residual);
/* Conjugate gradients preconditioned by the V-cycle (added). x0 = level 0's v as it stands (an
 * upload or a preceding gs_grid_fmg is honoured), r = f - A x0, hist[0] = ||r||; then at most maxiter iterations
 * (the grid's maxiter and tol; gs_grid_solve's stopping rule, history and *count semantics, and with `print` its
 * "iter: k residual: r Took Nms" lines), each one V-cycle from a zero iterate on the residual (every fused, tiled,
 * coarse-launch, weighted and POSITION path as gs_grid_vcycle takes it) plus three passes over level 0
 * (gpusolve_krylov.h). hist[k] is the square root of the recurrence residual's r . r. The scalars stay on the device;
 * the host waits once per iteration, for that norm. The first call allocates four more level-0 fields (r, z and two
 * directions; q lives in the cycle's ping-pong partner); if that fails the call fails with nothing changed.
 * Returns 0; GS_PCG_BREAKDOWN when p . q or r . z was not a positive finite number (a zero right-hand side, or a
 * residual already at rounding level): the loop ends there, v and the history are those of the last complete
 * iteration, nothing is NaN. The same code when an iteration's r . r is not finite (GS_PCG_BAD_RR: the iterate
 * overflowed; v holds it and the history ends before it, so the 0 recorded for r . r never counts as converged).
 * 1 (gs_last_error(), nothing touched) for a grid PCG cannot run on: a mode other than LINEAR, a Z-slab / RCCL or
 * trace grid, pre != post or pre = 0, weights whose post weights are not a permutation of
 * the pre weights, a stencil whose weight at offset o is not its weight at -o, a transition that is not aligned while
 * the transfers are REFERENCE — each makes the cycle a non-symmetric or indefinite preconditioner.
 * GS_SOLVER=pcg|vcycle in the environment when the grid is created makes gs_grid_solve / GpuSolve-hip on a LINEAR
 * grid run this instead of the V-cycle loop (after GS_FMG=k: from FMG's iterate); an ineligible grid then fails the
 * solve before any work, any other value fails the creation. */
enum { GS_PCG_BREAKDOWN = 2 };
int gs_grid_pcg(void* grid, int print, double* hist, int cap, int* count);
/* 1 if gs_grid_pcg can run on the grid as it is configured now, else 0 and the reason in gs_last_error(). */
int gs_grid_pcg_supported(void* grid);
/* The last gs_grid_pcg run's scalars: returns the number n of iterations it started (a breakdown's included; -1 and
 * gs_last_error() before any run) and writes, for k < min(n, cap_iters), rec[6k .. 6k+5] = r.z and p.q of iteration
 * k, alpha = rz / pq, the beta its direction used (0 for k = 0, else rz_k / rz_(k-1)), the new r . r, and the flag
 * (0, or GS_PCG_BAD_PQ | GS_PCG_BAD_RZ | GS_PCG_BAD_RR of gpusolve_krylov.h). rec may be NULL with cap_iters 0. */
int gs_grid_pcg_record(void* grid, double* rec, int cap_iters);
/* The level FMG starts on: the deepest level with every transition above it aligned (fine n = 2 coarse n + 1 per
 * axis); 0 when FMG is not applicable to the grid. */
int gs_grid_fmg_start_level(void* grid);
/* Per-sweep relaxation weights (added; Chebyshev-Jacobi smoothing). With weights set, on every
 * level the k-th pre-smoothing sweep of every V-cycle takes pre[k] and the k-th post-smoothing sweep post[k] in place
 * of the grid's omega; the coarsest level's pre + post sweeps take the pre weights, then the post weights. They apply
 * to gs_grid_solve in all three modes (NEWTON: its inner V-cycles), gs_grid_vcycle, gs_grid_vcycle_level,
 * gs_grid_fmg and Z-slab grids, through the same fused launches (the `_w` launchers of gpusolve_hip.h): equal
 * weights give the unweighted solve bit for bit. npre / npost must equal the grid's pre / post, each at most
 * GS_MAX_WEIGHTS, every weight finite; (NULL, 0, NULL, 0) clears the weights. On error (return 1) nothing changes
 * and gs_last_error() holds the reason. gs_grid_jacobi / gs_grid_time_jacobi are stand-alone sweeps and keep omega.
 * GS_OMEGAS in the environment when the grid is created sets them: "w1,w2/w3,w4" (pre weights, a slash, post
 * weights) or "cheb" (gs_chebyshev_weights on [1/3, 2] for the grid's own counts); a malformed value or a count
 * mismatch fails the creation. */
int gs_grid_set_weights(void* grid, const double* pre, int npre, const double* post, int npost);
/* 1 and the weights (pre: the grid's pre values, post: its post values; either may be NULL) when weights are set,
 * else 0. */
int gs_grid_get_weights(void* grid, double* pre, double* post);
/* out[k-1] = 1 / ((hi+lo)/2 + (hi-lo)/2 * cos(pi (2k-1) / (2 nu))), k = 1..nu: the weights whose error polynomial
 * prod (1 - w_k x) is the scaled Chebyshev polynomial of degree nu on [lo, hi]. Pure host code. 1 (and
 * gs_last_error()) unless nu >= 1 and 0 < lo < hi. */
int gs_chebyshev_weights(int nu, double lo, double hi, double* out);
/* GS_OMEGAS's parser on its own (pure host code): the value `text` for a grid of pre / post smoothing sweeps, as
 * pre + post weights into out (which may be NULL: validation only). 1 (and gs_last_error()) on a malformed value, a
 * count mismatch, a non-finite weight or more than GS_MAX_WEIGHTS weights per leg. */
int gs_parse_omegas(const char* text, int pre, int post, double* out);
/* Grid transfers (added). GS_TRANSFER_REFERENCE, the default: the reference's index-aligned restrict /
 * interpolate on every transition — exact only where fine n = 2 coarse n + 1, so V-cycles on even sizes (every power
 * of two) do not converge. GS_TRANSFER_POSITION: every transition that is not aligned takes the position-aware
 * operators of gpusolve_transfer.h (gs_residual_restrict_pa, gs_restrict_pa, gs_prolong_add_pa between the level's
 * ordinary sweeps; the tiled steps, the fused prolongation pairs and the one-launch coarse cycle are not taken there),
 * aligned transitions are unchanged launch for launch: on sizes 2^k - 1 the two modes give the same bits. Applies to
 * gs_grid_solve in all three modes, gs_grid_vcycle and gs_grid_vcycle_level; gs_grid_fmg keeps its alignment
 * requirement in either mode unless gs_grid_set_fmg_prolong lifts it (below). The tables of the non-aligned transitions are built and uploaded when POSITION is first
 * switched on. Fails (return 1, gs_last_error(), nothing changed) for any other mode value and for POSITION on a
 * Z-slab / RCCL grid. GS_TRANSFER=position|reference in the environment when the grid is created sets the mode; any
 * other value fails the creation. */
enum { GS_TRANSFER_REFERENCE = 0, GS_TRANSFER_POSITION = 1 };
int gs_grid_set_transfer(void* grid, int mode);
int gs_grid_get_transfer(void* grid);
/* The smoother (added). GS_SMOOTHER_JACOBI, the default: damped point Jacobi, every launch as
 * before. GS_SMOOTHER_ZLINE: every sweep solves each z-column's tridiagonal system exactly and stays Jacobi across
 * columns (gs_zline_sweep of gpusolve_line.h, one launch per sweep) — the smoother for a stencil whose z weights
 * dominate (thin cells in z), where point Jacobi V-cycles stall; on an isotropic stencil, or one whose weak axis is z,
 * it gains nothing and costs about four point cycles per cycle. A strong x or y axis: order the axes so that it is z.
 * In ZLINE mode nothing that embeds point Jacobi is taken (the fused pairs and triples, the fused prolongation pair,
 * the tiled steps, the one-launch coarse cycle, the speculative closing norm and with it the overlap of the norm wait
 * with the next cycle: the norm comes from a residual pass); the residual + restriction, the prolongation, the
 * POSITION transfers and the zero-guess flag are unchanged. gs_grid_solve, gs_grid_vcycle, gs_grid_vcycle_level,
 * gs_grid_jacobi, gs_grid_fmg and gs_grid_pcg follow the grid's smoother (per-sweep weights apply to line sweeps as
 * to point sweeps; a z-line cycle with pre = post is symmetric, so gs_grid_pcg's conditions are unchanged). Switching
 * back to JACOBI restores every launch of the default path. The factors of every level are built and uploaded when
 * ZLINE is first switched on and freed with the grid. Fails (return 1, gs_last_error(), nothing changed) for any
 * other mode value and for ZLINE on a grid that is not LINEAR, on a Z-slab / RCCL or schedule-trace grid (the lines
 * cross the slabs) and for a stencil gs_zline_supported refuses. GS_SMOOTHER=zline|jacobi in the environment when the
 * grid is created sets the mode; any other value, and zline on such a grid, fails the creation.
 * GS_SMOOTHER_AUTO (added; "auto" in GS_SMOOTHER) chooses per level: level l runs z-line sweeps where
 * the largest |z weight| of its stencil (gs_grid_level_stencil) is strictly greater than its largest |x / y weight|,
 * and the point path otherwise (gs_grid_level_smoother reports the choice). On an XYZ grid all levels share one
 * stencil, so AUTO is all or nothing; on an XY grid every coarsening multiplies the z weights by four against the
 * others, so the fine levels stay on the fused point kernels and the levels below run lines. JACOBI and ZLINE still
 * mean every level; on an XY grid ZLINE builds each level's factors from that level's stencil. A point level keeps
 * its fused pairs and triples, a line level takes nothing that embeds point Jacobi; one line level anywhere rules out
 * the one-launch coarse cycle. The closing norm: speculation, and with it the overlap of the norm wait, is off
 * whenever level 0 is a line level (the norm comes from a residual pass) and unchanged otherwise. AUTO needs a LINEAR
 * single-GPU grid, as ZLINE does, and is refused, with nothing changed, when a level that would run line sweeps has a
 * stencil gs_zline_supported refuses. */
enum { GS_SMOOTHER_JACOBI = 0, GS_SMOOTHER_ZLINE = 1, GS_SMOOTHER_AUTO = 2 };
int gs_grid_set_smoother(void* grid, int mode);
int gs_grid_get_smoother(void* grid);
/* 1 if level `level` runs z-line sweeps, 0 if it runs the point path, -1 for a bad level. */
int gs_grid_level_smoother(void* grid, int level);
/* Full multigrid's prolongation (added; DESIGN.md §4.7 "FMG on every size"). GS_FMG_PROLONG_ALIGNED, the default:
 * gs_grid_fmg as described above, unchanged launch for launch. GS_FMG_PROLONG_POSITION: gs_grid_fmg_start_level is the
 * coarsest level on every LINEAR / NONLINEAR single-GPU grid (NEWTON, Z-slab and trace grids: still 0, still refused);
 * f is restricted by gs_restrict_pa and v prolonged by gs_fmg_prolong_pa (gpusolve_transfer.h: the tricubic operator by
 * position) on every transition that is not aligned, aligned transitions keep gs_restrict / gs_fmg_prolong — on a grid
 * whose transitions are all aligned the setting changes nothing, bit for bit. A grid with a non-aligned transition
 * must also run the POSITION transfers (gs_grid_set_transfer): otherwise gs_grid_fmg fails with nothing done. The
 * tables are built and uploaded when POSITION is first set. Fails (return 1, gs_last_error(), nothing changed) for any
 * other mode value. GS_FMG_PROLONG=position|aligned in the environment when the grid is created sets the mode; any
 * other value fails the creation. */
enum { GS_FMG_PROLONG_ALIGNED = 0, GS_FMG_PROLONG_POSITION = 1 };
int gs_grid_set_fmg_prolong(void* grid, int mode);
int gs_grid_get_fmg_prolong(void* grid);
/* 1 if the transition from `level` to `level + 1` is aligned (fine n = 2 coarse n + 1 on all three axes; on an XY
 * grid: on x and y), 0 if not, -1 if there is no such transition. */
int gs_grid_level_aligned(void* grid, int level);
int gs_grid_jacobi(void* grid, int level, int sweeps);
int gs_grid_residual_norm(void* grid, int level, double* norm);
int gs_grid_num_levels(void* grid);
/* 1 if the level's smoothing runs as fused sweep pairs (gs_jacobi_sweep2), else 0. */
int gs_grid_level_fused(void* grid, int level);
/* The number of fused three-sweep launches (gs_jacobi_sweep3) issued on the level since the grid was created. */
int64_t gs_grid_level_triples(void* grid, int level);
int gs_grid_level(void* grid, int level, gs_level* out);
/* field: 0 v (current iterate), 1 restV, 2 newtonV, 3 f, 4 r, 5 newtonF (level 0). NULL if absent. */
double* gs_grid_field(void* grid, int level, int field);
hipStream_t gs_grid_stream(void* grid);
/* Synchronous copies of a whole padded field to / from a dense host array laid out
 * [nz+2][ny+2][nx+2] (x fastest). */
int gs_grid_download(void* grid, int level, int field, double* host);
int gs_grid_upload(void* grid, int level, int field, const double* host);
/* Device-side import / export of a field's interior (added; include/gpusolve_io.h has the semantics: `dev` is a device
 * array of dtype GS_IO_F64 / GS_IO_F32 addressed by three element strides, one per grid axis, scaled by `scale`; the
 * arithmetic, the accepted strides and the instances are gs_io_import's / gs_io_export's). No host copy and no host
 * synchronisation: the call returns with the work enqueued.
 *   Field state: the field ids and the rules of gs_grid_upload / gs_grid_download — an imported v or f of a level is
 *   what the next operation on that level reads, an import of newtonV invalidates what the driver derived from it, every
 *   field is exported stored. Only interior points are written: the ring keeps its values (v's: the zero Dirichlet
 *   value), so unlike an upload an import cannot set it.
 *   Ordering: `user` is the stream on which the caller produced (import) or will consume (export) `dev`. The copy runs
 *   on the grid's stream after everything enqueued on `user` so far, and work enqueued on `user` after the call runs
 *   after the copy — two events per grid, in both directions, so `dev` may be overwritten or freed on `user` straight
 *   away. With `user` the grid's own stream (gs_grid_stream) no event is used.
 *   Refused (1, the reason in gs_last_error(), nothing touched): a Z-slab / RCCL or schedule-trace grid (a rank holds a
 *   slab whose ghost planes would need an exchange), no such level or field, a null `dev`, and whatever gs_io_import /
 *   gs_io_export answer with GS_EINVAL. */
int gs_grid_import(void* grid, int level, int field, const void* dev, int dtype, const int64_t stride[3], double scale,
                   hipStream_t user);
int gs_grid_export(void* grid, int level, int field, void* dev, int dtype, const int64_t stride[3], double scale,
                   hipStream_t user);
int gs_grid_sync(void* grid);
/* Host cost of the ghost exchanges issued so far (Z-slab grids): total wall milliseconds spent inside
 * the exchange calls (RCCL: group start/end and the settle poll of the non-blocking communicator) and
 * the number of calls. Zero for single-GPU grids. */
int gs_grid_comm_stats(void* grid, double* halo_host_ms, int64_t* halo_calls);
/* The largest host cost of ONE exchange so far (issue + polls + settle; the pipelined sweep sequence
 * settles an exchange only before the next boundary planes, after the next interior is enqueued). */
int gs_grid_comm_stats_max(void* grid, double* halo_host_max_ms);
/* With GS_METRICS=1 in the environment when the grid was created: the "[gs] mlups=... gbps=...
 * pct_peak=... vcycle_ms=... cycles=... level_ms=..." line GpuSolve-hip prints after its solve (over
 * the V-cycles run so far), and the device ms per level and V-cycle. Non-zero if metrics are off. */
int gs_grid_metrics(void* grid, char* line, int cap, double* level_ms, int levels_cap);
/* Vector3::dump (src/cpu/Vector3.cpp:56-78) of a padded field: header "Px Py Pz" then "x y z value"
 * per point, x outermost, z innermost, values in the iostream default format (%g). path NULL or
 * empty (or not openable): the lines go to stdout without the header, as in the reference.
 * gs_dump_write formats a dense host array [pz][py][px] (x fastest); gs_grid_dump downloads first. */
int gs_dump_write(const double* host, int64_t px, int64_t py, int64_t pz, const char* path);
int gs_grid_dump(void* grid, int level, int field, const char* path);

/* Times `sweeps` level-`level` Jacobi sweeps with hipEvents on the grid's stream (after `warmup`
 * untimed sweeps); *ms = elapsed milliseconds of the timed sweeps. */
int gs_grid_time_jacobi(void* grid, int level, int warmup, int sweeps, float* ms);
/* Times `cycles` V-cycles (each including its norm readback) with a host clock; *ms total. */
int gs_grid_time_vcycles(void* grid, int cycles, double* ms, double* last_residual);

/* ---- Z-slab multi-GPU (new) ----
 * Ownership plan of every level for `nranks` ranks (pure host logic): distributed[l] = 1 when
 * level l is Z-slab partitioned; lo/hi[l*nranks + r] = rank r's owned global interior planes
 * (1-based, inclusive). min_points < 0 selects the default agglomeration threshold. Returns the
 * level count (at most max_levels entries are written). */
int gs_zslab_plan(const int64_t dims[3], int nranks, int64_t min_points, int max_levels, int* distributed,
                  int64_t* lo, int64_t* hi);
/* The Z-slab schedule of rank `rank` of `nranks` for the solve of p (construction, initial norm,
 * p->maxiter V-cycles / Newton iterations), produced by the driver's own V-cycle code in its trace mode
 * (no device touched): one line per kernel launch, ghost exchange, gather, norm reduction, swap and
 * zeroing, "op field=.. key=value ..." (ops: rhs pair sweep pro swap zero halo gather norm residual
 * resrestrict restrict prolongadd applyadd coarse copy newtonF axpy; L = level, z1..z2 = local planes,
 * c1..c2 = global coarse planes). Writes at most cap-1 bytes + NUL; *len = the full length. */
int gs_zslab_schedule(const gs_params* p, int nranks, int rank, int64_t min_points, char* buf, int64_t cap,
                      int64_t* len);
/* 128-byte RCCL unique id (rank 0 creates it, every rank passes the same bytes). */
int gs_rccl_unique_id(unsigned char uid[128]);
/* Grid whose levels are Z-slab partitioned over an RCCL communicator (one GPU per rank; the
 * current HIP device). The other gs_grid_* calls then run the distributed solver; fields and
 * levels describe this rank's slab; rank 0 prints. */
void* gs_grid_create_rccl(const gs_params* p, int rank, int nranks, const unsigned char uid[128]);
/* The same with an explicit RCCL CTA budget for this grid's communicator (ncclConfig_t::minCTAs = maxCTAs =
 * ctas: the workgroups RCCL's send/recv kernels take beside the interior sweep; 0: RCCL's own choice; -1: the
 * process default, GS_RCCL_CTAS or 64). gs_grid_create_rccl is ctas = -1. */
void* gs_grid_create_rccl_ctas(const gs_params* p, int rank, int nranks, const unsigned char uid[128], int ctas);
/* The CTA budget of the grid's RCCL communicator; -1 for single-GPU / loopback grids. */
int gs_grid_comm_ctas(void* grid);
/* NCCL_NCHANNELS_PER_PEER that gives one grouped ghost exchange (four send/recv per rank) the whole CTA budget
 * `ctas` (-1: the process default): ctas / 4, 0 for RCCL's default. RCCL reads the variable once per process,
 * so the LAUNCHER sets it (unless already set) before its first communicator — GpuSolve-hip's main and bench.py
 * do; the library never writes the process environment. */
int gs_rccl_channels_per_peer_hint(int ctas);
/* The id's file hand-off of a multi-process GpuSolve-hip run (one launcher, one node): rank 0
 * publishes (temporary file renamed into place), the others wait up to timeout_s for all 128 bytes.
 * 0 on success, else non-zero with gs_last_error(). */
int gs_uid_publish(const char* path, const unsigned char uid[128]);
int gs_uid_await(const char* path, double timeout_s, unsigned char uid[128]);
/* The id file GpuSolve-hip uses when GS_UID_FILE is unset: /tmp/gpusolve-uid-<parent pid>-<MASTER_PORT>,
 * plus -<TORCHELASTIC_RUN_ID>-a<TORCHELASTIC_RESTART_COUNT> under torchrun, so that each restart attempt
 * has its own file. Writes at most cap-1 bytes + NUL; returns the full length. */
int gs_uid_default_path(char* buf, int cap);
/* Single-process emulation of an nranks Z-slab run on the current device: nranks threads, each a
 * rank with its own slab and streams, device-to-device copies as the exchange. Runs `sweeps`
 * level-0 Jacobi sweeps, then (solve != 0) the solve of p. Writes rank 0's residual history and
 * the assembled level-0 v (dense [nz+2][ny+2][nx+2], interior planes only; NULL to skip).
 * min_points as in gs_zslab_plan. For testing the distributed path on one GPU. */
int gs_zslab_loopback_run(const gs_params* p, int nranks, int64_t min_points, int sweeps, int solve, double* hist,
                          int cap, int* count, double* v_host);

/* ---- failure-detection self-tests (host logic only; no GPU) ----
 * gs_debug_bounded_wait: the bounded wait that settles every RCCL call and sync (gs_comm.hpp),
 * driven by a fake poll: scenario 0 completes at poll k, 1 reports ncclInternalError at poll k,
 * 2 never completes (times out after timeout_s). Returns 0 on completion, 1 with the message in msg.
 * gs_debug_loopback_abort: nranks threads meet at loopback-hub barriers and failing_rank throws;
 * returns how many threads unwound (nranks = none left hanging); gs_last_error() = the first error. */
int gs_debug_bounded_wait(int scenario, int k, double timeout_s, char* msg, int cap);
int gs_debug_loopback_abort(int nranks, int failing_rank);

const char* gs_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* GPUSOLVE_DRIVER_H */
