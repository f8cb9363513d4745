// gs_io.hip — libgpusolve_io.so: device-side field import / export (include/gpusolve_io.h: semantics, arithmetic,
// instances). Its own library and header: the other libraries' export lists and kernels stay what they are.
// gs_device.hpp gives bad_level and the launch helpers; as in the transfer, line and semi libraries its non-template
// kernels come along as code objects nothing here launches, and its Knobs are read from the environment once, when
// the library is loaded. No launcher reads the environment.
#include "gs_device.hpp"
#include "gs_io_device.hpp"

#include "gpusolve_io.h"

#include <algorithm>
#include <cstdio>

namespace {

enum { IO_NONE = 0, IO_ROWS, IO_TILE_Y, IO_TILE_Z, IO_GEN };

// rows: levels of at least this many points stream through non-temporal 16-byte accesses, k_fmg_prolong's threshold
// (profiles/io/summary.md: the A/B at 512^3 and the measurement on either side of the threshold)
constexpr int64_t IO_NT_POINTS = int64_t(1) << 25;

struct IoPlan {
    int kind = IO_NONE; // IO_NONE with rc == 0: an empty axis
    int rc = 0;
    int wide = 0;       // rows: the strides and pitches allow 16-byte accesses (the pointers are the launcher's to add)
    int nt = 0;         // rows: the level is large enough for non-temporal accesses to pay (IO_NT_POINTS)
    IoGeom g{};
    int64_t blocks = 0; // (rows: per row)
    int tx = 0, tu = 0;
    int64_t points = 0;
};

// every check that does not need the pointers, and the instance with its launch shape
IoPlan io_plan(int dir, int dtype, const gs_level* L, const int64_t* s, double scale)
{
    IoPlan p;
    p.rc = GS_EINVAL;
    if ((dir != GS_IO_IMPORT && dir != GS_IO_EXPORT) || (dtype != GS_IO_F64 && dtype != GS_IO_F32) || !s ||
        bad_level(L) || L->z0 != 0 || !std::isfinite(scale))
        return p;
    const int64_t n[3] = {L->nx, L->ny, L->nz};
    for (int a = 0; a < 3; a++)
        if (s[a] < (dir == GS_IO_EXPORT ? 1 : 0)) return p;
    if (n[0] == 0 || n[1] == 0 || n[2] == 0) {
        p.rc = 0;
        return p;
    }
    if (dir == GS_IO_EXPORT) {
        // no two points on one element: the axes of more than one point by stride, each past the span of the last
        int ax[3], m = 0;
        for (int a = 0; a < 3; a++)
            if (n[a] > 1) ax[m++] = a;
        std::sort(ax, ax + m, [&](int a, int b) { return s[a] < s[b]; });
        for (int i = 1; i < m; i++) {
            const int64_t prev = s[ax[i - 1]], ext = n[ax[i - 1]];
            if (prev > INT64_MAX / ext || s[ax[i]] < prev * ext) return p;
        }
    }
    p.g = IoGeom{(int)L->nx, (int)L->ny, (int)L->nz, L->ldy, L->ldz, s[0], s[1], s[2]};
    if (s[0] == 1) {
        p.kind = IO_ROWS;
        const int pts = 64 * (dtype == GS_IO_F32 ? 4 : 2);
        const int64_t mod = dtype == GS_IO_F32 ? 4 : 2;
        p.wide = (L->ldy % 2 == 0 && L->ldz % 2 == 0 && s[1] % mod == 0 && s[2] % mod == 0) ? 1 : 0;
        p.nt = n[0] * n[1] * n[2] >= IO_NT_POINTS ? 1 : 0;
        p.blocks = (n[0] + pts * IO_ROW_WAVES - 1) / (pts * IO_ROW_WAVES);
        if (n[1] > 65535 || n[2] > 65535) { // rows are the launch grid's y and z extents
            p.kind = IO_NONE;
            return p;
        }
    } else if (s[1] == 1 || s[2] == 1) {
        p.kind = s[1] == 1 ? IO_TILE_Y : IO_TILE_Z;
        const int64_t nu = s[1] == 1 ? n[1] : n[2], nw = s[1] == 1 ? n[2] : n[1];
        p.tx = (int)((n[0] + IO_TILE - 1) / IO_TILE);
        p.tu = (int)((nu + IO_TILE - 1) / IO_TILE);
        p.blocks = (int64_t)p.tx * p.tu * nw;
    } else {
        p.kind = IO_GEN;
        p.points = n[0] * n[1] * n[2];
        p.blocks = (p.points + 255) / 256;
    }
    if (p.blocks > INT32_MAX) {
        p.kind = IO_NONE;
        return p;
    }
    p.rc = 0;
    return p;
}

template <int DIR, int DT>
void io_launch(const IoPlan& p, int wide, double* field, void* ext, double scale, hipStream_t st)
{
    const dim3 g((unsigned)p.blocks);
    switch (p.kind) {
    case IO_ROWS: {
        const dim3 gr((unsigned)p.blocks, (unsigned)p.g.ny, (unsigned)p.g.nz), b(64 * IO_ROW_WAVES);
        if (!wide) launch(k_io_rows<DIR, DT, 0, 0>, gr, b, st, field, ext, p.g, scale);
        else if (p.nt) launch(k_io_rows<DIR, DT, 1, 1>, gr, b, st, field, ext, p.g, scale);
        else launch(k_io_rows<DIR, DT, 1, 0>, gr, b, st, field, ext, p.g, scale);
        break;
    }
    case IO_TILE_Y:
    case IO_TILE_Z:
        launch(k_io_tile<DIR, DT>, g, dim3(256), st, field, ext, p.g, scale, p.kind == IO_TILE_Y ? 1 : 2, p.tx, p.tu);
        break;
    default: launch(k_io_gen<DIR, DT>, g, dim3(256), st, field, ext, p.g, scale, p.points); break;
    }
}

int io_run(int dir, double* field, const gs_level* L, void* ext, int dtype, const int64_t* stride, double scale,
           hipStream_t st)
{
    if (!field || !ext) return GS_EINVAL;
    const IoPlan p = io_plan(dir, dtype, L, stride, scale);
    if (p.rc != 0 || p.kind == IO_NONE) return p.rc;
    const int wide = (p.wide && (reinterpret_cast<uintptr_t>(field + 1) & 15) == 0 &&
                      (reinterpret_cast<uintptr_t>(ext) & 15) == 0) ? 1 : 0;
    if (dir == GS_IO_IMPORT) {
        if (dtype == GS_IO_F64) io_launch<GS_IO_IMPORT, GS_IO_F64>(p, wide, field, ext, scale, st);
        else io_launch<GS_IO_IMPORT, GS_IO_F32>(p, wide, field, ext, scale, st);
    } else {
        if (dtype == GS_IO_F64) io_launch<GS_IO_EXPORT, GS_IO_F64>(p, wide, field, ext, scale, st);
        else io_launch<GS_IO_EXPORT, GS_IO_F32>(p, wide, field, ext, scale, st);
    }
    return launch_status();
}

// the names as the launch record spells them
struct IoNames {
    char rows[2][2][3][24], tile[2][2][24], gen[2][2][24]; // rows: W = 0, W = 1, W = 1 non-temporal
    IoNames()
    {
        for (int d = 0; d < 2; d++)
            for (int t = 0; t < 2; t++) {
                for (int w = 0; w < 3; w++)
                    std::snprintf(rows[d][t][w], 24, "k_io_rows<%d, %d, %d, %d>", d, t, w ? 1 : 0, w == 2 ? 1 : 0);
                std::snprintf(tile[d][t], 24, "k_io_tile<%d, %d>", d, t);
                std::snprintf(gen[d][t], 24, "k_io_gen<%d, %d>", d, t);
            }
    }
};
const IoNames kIoNames;

} // namespace

extern "C" {

int gs_io_import(double* field, const gs_level* L, const void* ext, int dtype, const int64_t stride[3], double scale,
                 hipStream_t st)
{
    return io_run(GS_IO_IMPORT, field, L, const_cast<void*>(ext), dtype, stride, scale, st);
}

int gs_io_export(const double* field, const gs_level* L, void* ext, int dtype, const int64_t stride[3], double scale,
                 hipStream_t st)
{
    return io_run(GS_IO_EXPORT, const_cast<double*>(field), L, ext, dtype, stride, scale, st);
}

const char* gs_io_kernel(int dir, int dtype, const gs_level* L, const int64_t stride[3])
{
    const IoPlan p = io_plan(dir, dtype, L, stride, 1.0);
    switch (p.kind) {
    case IO_ROWS: return kIoNames.rows[dir][dtype][p.wide ? 1 + p.nt : 0];
    case IO_TILE_Y:
    case IO_TILE_Z: return kIoNames.tile[dir][dtype];
    case IO_GEN: return kIoNames.gen[dir][dtype];
    default: return "";
    }
}

int gs_io_launch_dry_run(int on) { return launch_dry_run(on); }

int64_t gs_io_launch_record(char* buf, int64_t cap) { return launch_record_take(buf, cap); }

} // extern "C"
