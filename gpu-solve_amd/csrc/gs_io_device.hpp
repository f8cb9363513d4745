// gs_io_device.hpp — the kernels of libgpusolve_io.so (include/gpusolve_io.h: what they move and the arithmetic).
// Included by gs_io.hip after gs_device.hpp. Every kernel is a template on the direction (GS_IO_IMPORT / GS_IO_EXPORT)
// and the external dtype (GS_IO_F64 / GS_IO_F32); `field` is written by imports only and `ext` by exports only.
#pragma once

#include "gpusolve_io.h"

namespace {

struct IoGeom {
    int nx, ny, nz;
    int64_t ldy, ldz; // field pitches
    int64_t sx, sy, sz; // external element strides
};

template <int DT> struct IoExt;
template <> struct IoExt<GS_IO_F64> { using T = double; };
template <> struct IoExt<GS_IO_F32> { using T = float; };

typedef double io_d2 __attribute__((ext_vector_type(2)));
typedef float io_f4 __attribute__((ext_vector_type(4)));

// the two point expressions of the header; scale == 1.0 multiplies nothing
template <class T>
__device__ __forceinline__ double io_in(T e, double scale)
{
    const double d = (double)e;
    return scale == 1.0 ? d : scale * d;
}

template <class T>
__device__ __forceinline__ T io_out(double f, double scale)
{
    const double p = scale == 1.0 ? f : scale * f;
    return (T)p;
}

constexpr int IO_ROW_WAVES = 4; // waves per block of k_io_rows

// 16-byte accesses of the rows instance; NT: non-temporal (a level that no cache holds is streamed past them)
template <int NT, class V>
__device__ __forceinline__ V io_ldv(const void* p)
{
    return NT ? __builtin_nontemporal_load(static_cast<const V*>(p)) : *static_cast<const V*>(p);
}

template <int NT, class V>
__device__ __forceinline__ void io_stv(void* p, V v)
{
    if (NT) __builtin_nontemporal_store(v, static_cast<V*>(p));
    else *static_cast<V*>(p) = v;
}

// rows: sx == 1. Block (bx, y, z) owns IO_ROW_WAVES segments of row (y, z), one per wave; a segment is 64 * P points,
// P = 2 (fp64) or 4 (fp32). WIDE: lane l moves points P*l .. P*l + P-1 of the segment with 16-byte accesses, the
// group that crosses the row's end point by point. Otherwise lane l moves points l, 64 + l, ... No index is divided.
template <int DIR, int DT, int WIDE, int NT>
__global__ __launch_bounds__(64 * IO_ROW_WAVES) void k_io_rows(double* __restrict__ field, void* __restrict__ ext,
                                                                IoGeom g, double scale)
{
    using T = typename IoExt<DT>::T;
    constexpr int P = DT == GS_IO_F32 ? 4 : 2;
    const int lane = threadIdx.x & 63;
    const int64_t xb = ((int64_t)blockIdx.x * IO_ROW_WAVES + (threadIdx.x >> 6)) * (64 * P);
    if (xb >= g.nx) return;
    const int64_t y = blockIdx.y, z = blockIdx.z;
    double* f = field + (z + 1) * g.ldz + (y + 1) * g.ldy + 1;
    T* e = static_cast<T*>(ext) + z * g.sz + y * g.sy;
    if (WIDE) {
        const int x = (int)xb + lane * P;
        if (x + P <= g.nx) {
            if (DIR == GS_IO_IMPORT) {
                if (DT == GS_IO_F64) {
                    const io_d2 s = io_ldv<NT, io_d2>(e + x);
                    io_d2 d;
                    d.x = io_in(s.x, scale);
                    d.y = io_in(s.y, scale);
                    io_stv<NT>(f + x, d);
                } else {
                    const io_f4 s = io_ldv<NT, io_f4>(e + x);
                    io_d2 d0, d1;
                    d0.x = io_in(s.x, scale);
                    d0.y = io_in(s.y, scale);
                    d1.x = io_in(s.z, scale);
                    d1.y = io_in(s.w, scale);
                    io_stv<NT>(f + x, d0);
                    io_stv<NT>(f + x + 2, d1);
                }
            } else {
                if (DT == GS_IO_F64) {
                    const io_d2 s = io_ldv<NT, io_d2>(f + x);
                    io_d2 d;
                    d.x = io_out<double>(s.x, scale);
                    d.y = io_out<double>(s.y, scale);
                    io_stv<NT>(e + x, d);
                } else {
                    const io_d2 s0 = io_ldv<NT, io_d2>(f + x);
                    const io_d2 s1 = io_ldv<NT, io_d2>(f + x + 2);
                    io_f4 d;
                    d.x = io_out<float>(s0.x, scale);
                    d.y = io_out<float>(s0.y, scale);
                    d.z = io_out<float>(s1.x, scale);
                    d.w = io_out<float>(s1.y, scale);
                    io_stv<NT>(e + x, d);
                }
            }
        } else {
            for (int k = x; k < g.nx; k++) {
                if (DIR == GS_IO_IMPORT) f[k] = io_in(e[k], scale);
                else e[k] = io_out<T>(f[k], scale);
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < P; k++) {
            const int64_t x = xb + k * 64 + lane;
            if (x < g.nx) {
                if (DIR == GS_IO_IMPORT) f[x] = io_in(e[x], scale);
                else e[x] = io_out<T>(f[x], scale);
            }
        }
    }
}

constexpr int IO_TILE = 64;     // a tile is IO_TILE x by IO_TILE points of the external side's unit-stride axis
constexpr int IO_TILE_LD = 65;  // LDS row pitch in doubles: the column read t[lane][i] is lane * 130 + 2 i dwords,
                                // every bank pair of a 32-lane half once (ds_read_b64: bank = dword mod 64)

// tile: the external side has unit stride along u (uaxis 1: y, 2: z) and not along x. Block b owns tile (b % tx,
// (b / tx) % tu) of the plane w = b / (tx * tu) of the third axis. The tile holds the field-side values as doubles,
// [row][lane] as the coalesced read delivers them; the write side reads it [lane][row].
template <int DIR, int DT>
__global__ __launch_bounds__(256) void k_io_tile(double* __restrict__ field, void* __restrict__ ext, IoGeom g,
                                                 double scale, int uaxis, int tx, int tu)
{
    using T = typename IoExt<DT>::T;
    __shared__ double t[IO_TILE][IO_TILE_LD];
    unsigned b = blockIdx.x; // (the launcher keeps the block count below 2^31)
    const int x0 = (int)(b % (unsigned)tx) * IO_TILE;
    b /= (unsigned)tx;
    const int u0 = (int)(b % (unsigned)tu) * IO_TILE;
    const int64_t w = b / (unsigned)tu;
    const int nu = uaxis == 1 ? g.ny : g.nz;
    const int64_t fu = uaxis == 1 ? g.ldy : g.ldz, fw = uaxis == 1 ? g.ldz : g.ldy;
    const int64_t sw = uaxis == 1 ? g.sz : g.sy;
    double* f = field + g.ldz + g.ldy + 1 + w * fw; // + x + u * fu
    T* e = static_cast<T*>(ext) + w * sw;           // + x * sx + u
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (DIR == GS_IO_IMPORT) {
        for (int i = wv; i < IO_TILE; i += 4) {
            const int x = x0 + i, u = u0 + lane;
            if (x < g.nx && u < nu) t[i][lane] = io_in(e[x * g.sx + u], scale);
        }
        __syncthreads();
        for (int i = wv; i < IO_TILE; i += 4) {
            const int u = u0 + i, x = x0 + lane;
            if (x < g.nx && u < nu) f[x + u * fu] = t[lane][i];
        }
    } else {
        for (int i = wv; i < IO_TILE; i += 4) {
            const int u = u0 + i, x = x0 + lane;
            if (x < g.nx && u < nu) t[i][lane] = f[x + u * fu];
        }
        __syncthreads();
        for (int i = wv; i < IO_TILE; i += 4) {
            const int x = x0 + i, u = u0 + lane;
            if (x < g.nx && u < nu) e[x * g.sx + u] = io_out<T>(t[lane][i], scale);
        }
    }
}

// gen: one interior point per thread, x fastest
template <int DIR, int DT>
__global__ __launch_bounds__(256) void k_io_gen(double* __restrict__ field, void* __restrict__ ext, IoGeom g,
                                                double scale, int64_t points)
{
    using T = typename IoExt<DT>::T;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= points) return;
    const int64_t x = i % g.nx, r = i / g.nx;
    const int64_t y = r % g.ny, z = r / g.ny;
    double* f = field + (z + 1) * g.ldz + (y + 1) * g.ldy + (x + 1);
    T* e = static_cast<T*>(ext) + x * g.sx + y * g.sy + z * g.sz;
    if (DIR == GS_IO_IMPORT) *f = io_in(*e, scale);
    else *e = io_out<T>(*f, scale);
}

} // namespace
