/* gpusolve_io.h — device-side field import / export (libgpusolve_io.so). Added; not reference operators. The driver
 * calls it from gs_grid_import / gs_grid_export (include/gpusolve_driver.h); nothing else in the
 * product does.
 *
 * A field of the kernel ABI (include/gpusolve_hip.h: padded, pitched, fp64) on one side, a caller's device array on
 * the other: fp64 or fp32, addressed by three ELEMENT strides, one per grid axis. Interior point (x, y, z), each
 * index from 1, corresponds to ext[(x-1)*stride[0] + (y-1)*stride[1] + (z-1)*stride[2]], elements of the external
 * type counted from `ext`. A torch-contiguous [z][y][x] tensor is stride = {1, nx, nx*ny}; the reference's [x][y][z]
 * order is {ny*nz, nz, 1}; a strong x axis that should become the grid's z is a matter of which stride goes where.
 *
 * Arithmetic, as written, no contraction, per point and independent of the instance that moves it:
 *     import:  d = (double)e            fp32 -> fp64 is the exact widening; an fp64 e is taken as it is
 *              field = scale == 1.0 ? d : scale * d        one multiply in double, rounded once
 *     export:  p = scale == 1.0 ? f : scale * f
 *              ext = (type)p            fp64 -> fp32 is ONE round-to-nearest-even conversion of p; fp64 stores p
 * With scale == 1.0 nothing is multiplied: fp64 <-> fp64 moves the bits, NaN payloads included; the conversions treat
 * a NaN as IEEE 754 conversions do (quiet, the payload's leading bits kept). numpy reproduces every word:
 * np.float64(e), np.float64(scale) * d, p.astype(np.float32).
 *
 * What is read and written. Import writes exactly the interior points of `field` — ring, pitch padding and `ext` are
 * untouched — and reads exactly the addressed elements of `ext`. Export writes exactly the addressed elements of
 * `ext` and reads only the interior of `field`.
 *
 * Strides. Import takes strides >= 0; stride 0 broadcasts (stride[2] = 0: one plane into every z). Export takes
 * strides >= 1 that do not alias: of the axes with more than one point, sorted by stride, each stride must be >= the
 * previous stride times the previous extent (an axis of one point addresses nothing twice whatever its stride).
 *
 * Launchers: the conventions of gpusolve_hip.h — asynchronous on `stream`, no allocation, no synchronisation, no
 * environment variable; 0, GS_EINVAL or a hipError_t; whole levels (z0 = 0); for the FIELD side its layout contract:
 * any legal pitch and any 8-byte-aligned field pointer. `ext` must be aligned to its element size. GS_EINVAL, nothing
 * written and nothing launched: a null pointer, a bad level or z0 != 0, an unknown dtype, a scale that is not finite,
 * a negative stride, (export) a zero or aliasing stride, more than 2^31 - 1 blocks, ny or nz above 65535 with
 * stride[0] == 1. A level with an empty axis: 0, nothing launched.
 *
 * Instances (gs_io_kernel names the one a call launches; DIR, DT are the direction and dtype below):
 *   rows  "k_io_rows<DIR, DT, W, NT>"  stride[0] == 1. A wave moves a row segment of 128 points (fp32: 256); a block,
 *                                   four of them; rows are the launch grid's y and z. W = 1: 16-byte accesses on both
 *                                   sides (fp32: 16 bytes of four floats against two 16-byte field accesses), taken
 *                                   where both sides allow it — interior x = 1 of the field 16-byte aligned with even
 *                                   pitches (gs_field_layout's layout is), and `ext`, stride[1] and stride[2]
 *                                   multiples of 16 bytes; the ragged end of a row goes point by point. NT = 1: those
 *                                   accesses are non-temporal, on levels of 2^25 points and more (as gs_copy's are).
 *                                   W = 0 (then NT = 0): 8-byte accesses (4 on an fp32 side), lanes on consecutive
 *                                   points. The torch-contiguous case, and the one built to run at copy speed.
 *   tile  "k_io_tile<DIR, DT>"      stride[0] != 1 and stride[1] == 1 or stride[2] == 1. A block transposes a tile of
 *                                   64 x by 64 points of the unit-stride axis (y if stride[1] == 1, else z) through
 *                                   LDS, rows padded to 65 doubles against bank conflicts: the global read and the
 *                                   global write are both coalesced. The "make my strong axis z" and [x][y][z] case.
 *   gen   "k_io_gen<DIR, DT>"       anything else. One point per thread, x fastest. Correct for every stride triple,
 *                                   not fast: the external side is as uncoalesced as the strides make it.
 */
#ifndef GPUSOLVE_IO_H
#define GPUSOLVE_IO_H

#include <stdint.h>
#include "gpusolve_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { GS_IO_F64 = 0, GS_IO_F32 = 1 };       /* dtype: the external array's element type */
enum { GS_IO_IMPORT = 0, GS_IO_EXPORT = 1 }; /* dir of gs_io_kernel */

/* field interior (x,y,z = 1..n) = scale * ext[(x-1)*sx + (y-1)*sy + (z-1)*sz] — element strides */
int gs_io_import(double* field, const gs_level* L, const void* ext, int dtype, const int64_t stride[3], double scale,
                 hipStream_t stream);
/* ext[...] = (dtype)(scale * field interior) */
int gs_io_export(const double* field, const gs_level* L, void* ext, int dtype, const int64_t stride[3], double scale,
                 hipStream_t stream);

/* The kernel instance a call with these arguments launches, for 16-byte-aligned `field + 1` and `ext` (the W of a rows
 * instance is then decided by the pitches and strides alone; a launcher looks at its pointers as well): one of the
 * names above with its numbers filled in, e.g. "k_io_rows<0, 1, 1, 0>". "" for arguments the launchers refuse and for a
 * level with an empty axis. */
const char* gs_io_kernel(int dir, int dtype, const gs_level* L, const int64_t stride[3]);

/* This library's launch record: gs_launch_dry_run / gs_launch_record of include/gpusolve_hip.h for the launchers
 * above (each library keeps its own record and its own dry-run flag). */
int gs_io_launch_dry_run(int on);
int64_t gs_io_launch_record(char* buf, int64_t cap);

#ifdef __cplusplus
}
#endif
#endif /* GPUSOLVE_IO_H */
