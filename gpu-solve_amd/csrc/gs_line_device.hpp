// gs_line_device.hpp — the kernels of libgpusolve_line.so (include/gpusolve_line.h): one z-line Jacobi sweep per
// launch. gs_device.hpp gives the lane shifts, the pair loads / stores, the XCD tile order and the launch helpers;
// no kernel of it is launched from here. Internal linkage. Built with -ffp-contract=off: every expression rounds as
// written, and the expressions are the header's, in its order.
#pragma once
#include "gs_device.hpp"

#include "gpusolve_line.h"

namespace {

// What a sweep needs of the stencil, by value (SGPRs): the four x / y entries in config order (weights, and their
// linear element offsets for the one-column kernel), the weight at (0, 0, -1), h*h and the relaxation weight.
struct ZlCoef {
    double s[4];
    int64_t off[4];
    double lo, hh, omega;
};

// g_k's sum: the first product starts it
__device__ __forceinline__ double zl_g(const ZlCoef& k, double a0, double a1, double a2, double a3)
{
    double g = k.s[0] * a0;
    g = g + k.s[1] * a1;
    g = g + k.s[2] * a2;
    g = g + k.s[3] * a3;
    return g;
}
// one forward step: d_k from b_k, d_{k-1} and den[k] (FIRST: k = 1)
__device__ __forceinline__ double zl_fwd(const ZlCoef& k, double b, double dprev, double den, bool first)
{
    const double t = k.lo * dprev;
    const double num = first ? b : b - t;
    return num / den;
}
// one backward step: u_k from d_k, u_{k+1} and cp[k] (LAST: k = nz)
__device__ __forceinline__ double zl_bwd(double d, double unext, double cp, bool last)
{
    const double t = cp * unext;
    return last ? d : d - t;
}
template <bool ZV>
__device__ __forceinline__ double zl_relax(const ZlCoef& k, double v, double u)
{
    if (ZV) return k.omega * u;
    const double w = u - v;
    const double t = k.omega * w;
    return v + t;
}

// ---------------------------------------------------------------------------------------------
// The marching instance. k_rb's lane shape (gs_device.hpp): a lane owns one dwordx4 pair (x, x+1) of ONE row, a wave
// 128 columns of it, ZL_W waves stack in y; there is no z-chunk — the block's columns are marched from plane 1 to nz
// (forward elimination, d stored into v_out) and back (substitution, the relaxed result stored non-temporally over
// d). x-neighbours come by DPP wave shift with wave-uniform edge loads, y-neighbours are two more row loads (the
// rows of the neighbour waves: L1 / L2 hits, which is why y-adjacent tiles share an XCD, xcd_tile).
//
// The recurrence is one dependent multiply-subtract-divide per plane, but no load depends on it: both passes keep
// ZL_R planes of loads in flight in a register ring (slot s is consumed, then refilled with the plane ZL_R steps
// ahead; the loops are unrolled by ZL_R so that the slot index is static, every load is unconditional with its plane
// clamped into 0 .. nz+1, and the steps past the level's end are computed and discarded, as in k_rb). den[k] and
// cp[k] travel in the ring too. Canonical stencil order only (k_zline_col takes the rest). Columns and rows are
// clamped into the padded box; only x <= nx, y <= ny is stored.
constexpr int ZL_W = 4; // waves (rows) per block
// Ring depth (planes in flight: ZL_R - 1 behind the one being consumed). The columns are all the parallelism there is
// — two waves per SIMD at 512^2, half a wave at 256^2 — so registers are spent on depth: 8 slots are 151 VGPRs, three
// waves per SIMD, no scratch (4 slots: 86 VGPRs, five waves, which the columns cannot fill; profiles/zline/).
constexpr int ZL_R = 8;

template <bool ZV>
__global__ __launch_bounds__(WAVE* ZL_W) void k_zline_march(ZlCoef k, const double* __restrict__ v,
                                                            const double* __restrict__ f, double* __restrict__ out,
                                                            const double* __restrict__ cp,
                                                            const double* __restrict__ den, int nx, int ny, int nz,
                                                            int64_t ldy, int64_t ldz)
{
    const int lane = threadIdx.x;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.y);
    const int nbx = (nx + 2 * WAVE - 1) / (2 * WAVE);
    const int64_t tile = xcd_tile(blockIdx.x, gridDim.x);
    const int bx = (int)(tile % nbx), by = (int)(tile / nbx);
    const int x0 = 1 + bx * (2 * WAVE);
    const int x = x0 + 2 * lane;
    const int xl = min(x, nx + 1);
    const int y = 1 + by * ZL_W + wv;
    const int xle = x0 - 1;
    const int xre = min(x0 + 2 * WAVE, nx + 1);
    const bool okx0 = x <= nx && y <= ny, okx1 = x + 1 <= nx && y <= ny;
    const int64_t rm = (int64_t)min(y - 1, ny + 1) * ldy, rc = (int64_t)min(y, ny + 1) * ldy,
                  rp = (int64_t)min(y + 1, ny + 1) * ldy;

    // ---- forward: d_k into v_out ----
    {
        double2 C[ZL_R], HM[ZL_R], HP[ZL_R], F[ZL_R];
        double EL[ZL_R], ER[ZL_R], DN[ZL_R];
        auto load_slot = [&](const int s, const int kk) {
            const int64_t zo = (int64_t)kk * ldz;
            F[s] = ld2(f + xl + rc + zo);
            DN[s] = den[kk];
            if (!ZV) {
                C[s] = ld2(v + xl + rc + zo);
                HM[s] = ld2(v + xl + rm + zo);
                HP[s] = ld2(v + xl + rp + zo);
                EL[s] = v[xle + rc + zo];
                ER[s] = v[xre + rc + zo];
            }
        };
#pragma unroll
        for (int s = 0; s < ZL_R; s++) load_slot(s, min(1 + s, nz + 1));
        double d0 = 0.0, d1 = 0.0;
        for (int k0 = 1; k0 <= nz; k0 += ZL_R) {
#pragma unroll
            for (int s = 0; s < ZL_R; s++) {
                const int kz = k0 + s;
                double b0 = k.hh * F[s].x, b1 = k.hh * F[s].y;
                if (!ZV) {
                    const double2 c = C[s];
                    const double xm0 = lane_from_left<true>(c.y, EL[s]);
                    const double xp1 = lane_from_right<true>(c.x, ER[s]);
                    b0 = b0 - zl_g(k, c.y, xm0, HP[s].x, HM[s].x);
                    b1 = b1 - zl_g(k, xp1, c.x, HP[s].y, HM[s].y);
                }
                d0 = zl_fwd(k, b0, d0, DN[s], kz == 1);
                d1 = zl_fwd(k, b1, d1, DN[s], kz == 1);
                if (kz <= nz) {
                    double* q = out + x + rc + (int64_t)kz * ldz;
                    if (okx1) st2s<false>(q, d0, d1);
                    else if (okx0) *q = d0;
                }
                load_slot(s, min(kz + ZL_R, nz + 1));
            }
        }
    }
    // ---- backward: u_k, and the relaxed iterate over d ----
    {
        double2 D[ZL_R], V[ZL_R];
        double CP[ZL_R];
        auto load_slot = [&](const int s, const int kk) {
            const int64_t zo = (int64_t)kk * ldz;
            D[s] = ld2(out + xl + rc + zo);
            CP[s] = cp[kk];
            if (!ZV) V[s] = ld2(v + xl + rc + zo);
        };
#pragma unroll
        for (int s = 0; s < ZL_R; s++) load_slot(s, max(nz - s, 0));
        double u0 = 0.0, u1 = 0.0;
        for (int k0 = nz; k0 >= 1; k0 -= ZL_R) {
#pragma unroll
            for (int s = 0; s < ZL_R; s++) {
                const int kz = k0 - s;
                u0 = zl_bwd(D[s].x, u0, CP[s], kz == nz);
                u1 = zl_bwd(D[s].y, u1, CP[s], kz == nz);
                const double o0 = zl_relax<ZV>(k, ZV ? 0.0 : V[s].x, u0);
                const double o1 = zl_relax<ZV>(k, ZV ? 0.0 : V[s].y, u1);
                if (kz >= 1) {
                    double* q = out + x + rc + (int64_t)kz * ldz;
                    if (okx1) st2s<true>(q, o0, o1);
                    else if (okx0) *q = o0;
                }
                load_slot(s, max(kz - ZL_R, 0));
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// One column per thread (k_generic's block shape): the seven axis offsets in any order, and the levels too small for
// the marching instance. The neighbours are plain loads at the entries' linear offsets. The plane loop is unrolled so
// that the loads of four planes are issued ahead of the dependent chain.
template <bool ZV>
__global__ __launch_bounds__(256) void k_zline_col(ZlCoef k, const double* __restrict__ v, const double* __restrict__ f,
                                                   double* __restrict__ out, const double* __restrict__ cp,
                                                   const double* __restrict__ den, int nx, int ny, int nz, int64_t ldy,
                                                   int64_t ldz)
{
    const int x = 1 + blockIdx.x * GN_BX + threadIdx.x;
    const int y = 1 + blockIdx.y * GN_BY + threadIdx.y;
    if (x > nx || y > ny) return;
    const int64_t base = x + (int64_t)y * ldy;
    double d = 0.0;
#pragma unroll 4
    for (int kz = 1; kz <= nz; kz++) {
        const int64_t p = base + (int64_t)kz * ldz;
        double b = k.hh * f[p];
        if (!ZV) b = b - zl_g(k, v[p + k.off[0]], v[p + k.off[1]], v[p + k.off[2]], v[p + k.off[3]]);
        d = zl_fwd(k, b, d, den[kz], kz == 1);
        out[p] = d;
    }
    double u = 0.0;
#pragma unroll 4
    for (int kz = nz; kz >= 1; kz--) {
        const int64_t p = base + (int64_t)kz * ldz;
        u = zl_bwd(out[p], u, cp[kz], kz == nz);
        out[p] = zl_relax<ZV>(k, ZV ? 0.0 : v[p], u);
    }
}

// ---------------------------------------------------------------------------------------------
// Few, long columns (fewer than 32 * 32 of them, ZF_MIN_NZ .. ZF_MAX_NZ planes; any stencil order): k_zline_col's
// 2 nz dependent steps each wait for a global load there, on levels that fill a fraction of one CU. Here a block of
// four waves owns ZF_CB columns (consecutive in the flattened index x - 1 + nx * (y - 1), so the tiles are full
// whatever nx is) and keeps their state in LDS, [plane][column]:
//   A  all threads, one (plane, column) each per pass of ZF_T / ZF_CB planes: b_k into LDS, k_zline_col's expression
//      with the neighbours at the entries' linear offsets; den[1 .. nz] and cp[1 .. nz] into LDS beside it
//   B  lanes 0 .. ZF_CB - 1 of wave 0, a column each: d over b, k ascending, then u over d, k descending. As in
//      k_zline_march the operands of the next planes wait in a register ring (a slot is consumed, then refilled from
//      LDS with the plane one ring length ahead; the loops are unrolled by the ring length), so that no step waits
//      for memory: the step is the chain itself (multiply, subtract, IEEE divide; multiply, subtract)
//   C  all threads: the relaxed iterate from u (LDS) and v (global) to the interior of v_out
// d never leaves LDS and v_out is never read: 24 B per point (16 on the zero iterate) where k_zline_col moves 48.
// The steps of B past the level's end are computed and discarded, as in k_zline_march: their operands are read at
// the plane clamped into 1 .. nz, and their results land in spare rows below plane 1 and above plane nz.
// Every thread reaches both barriers: a thread without a column, or a wave without a chain, only skips its work.
constexpr int ZF_T = 256;     // threads per block
constexpr int ZF_CB = 8;      // columns per block
// Ring lengths. Forward: a step is a dozen dependent fp64 instructions, three steps cover an LDS read many times
// over, and the 3 * (2 reads + 1 write) behind a slot's read stay under lgkmcnt's 15: its waits are exact. Backward: a
// step is two operations, so the ring is longer.
constexpr int ZF_UF = 4, ZF_UB = 8;
constexpr int ZF_MIN_NZ = 64; // below: a launch is mostly phases A and C, and k_zline_col's is as short
constexpr int ZF_MAX_NZ = 1536;
constexpr int ZF_ROWS = ZF_MAX_NZ + ZF_UB + ZF_UF - 2;    // planes 2 - ZF_UB .. ZF_MAX_NZ + ZF_UF - 1
constexpr int ZF_WORDS = ZF_ROWS * ZF_CB + 2 * ZF_MAX_NZ; // state, den[1 ..], cp[1 ..]: 123,520 B
static_assert(ZF_WORDS * sizeof(double) <= 160 * 1024, "k_zline_lds: static LDS beyond a CU's 160 KiB");

template <bool ZV>
__global__ __launch_bounds__(ZF_T) void k_zline_lds(ZlCoef k, const double* __restrict__ v, const double* __restrict__ f,
                                                    double* __restrict__ out, const double* __restrict__ cp,
                                                    const double* __restrict__ den, int nx, int ny, int nz, int64_t ldy,
                                                    int64_t ldz)
{
    __shared__ double lds[ZF_WORDS]; // one array: state rows, then the two tables
    double* const S = lds + (ZF_UB - 2) * ZF_CB; // S[kz * ZF_CB + c]: plane kz (2 - ZF_UB .. nz + ZF_UF - 1), column c
    double* const DEN = lds + ZF_ROWS * ZF_CB - 1; // DEN[kz], CP[kz]: kz = 1 .. nz
    double* const CP = DEN + ZF_MAX_NZ;
    const int t = threadIdx.x;
    const int c = t % ZF_CB, pz = t / ZF_CB;
    const int col = blockIdx.x * ZF_CB + c;
    const bool has = col < nx * ny;
    const int64_t base = (1 + col % nx) + (int64_t)(1 + col / nx) * ldy;

    // ---- A ----
    if (has) {
#pragma unroll 4
        for (int kz = 1 + pz; kz <= nz; kz += ZF_T / ZF_CB) {
            const int64_t p = base + (int64_t)kz * ldz;
            double b = k.hh * f[p];
            if (!ZV) b = b - zl_g(k, v[p + k.off[0]], v[p + k.off[1]], v[p + k.off[2]], v[p + k.off[3]]);
            S[kz * ZF_CB + c] = b;
        }
    }
    for (int kz = 1 + t; kz <= nz; kz += ZF_T) {
        DEN[kz] = den[kz];
        CP[kz] = cp[kz];
    }
    __syncthreads();

    // ---- B ----
    if (t < ZF_CB && has) {
        {
            double X[ZF_UF], W[ZF_UF]; // the ring: b_k and den[k] of the next ZF_UF planes
#pragma unroll
            for (int s = 0; s < ZF_UF; s++) {
                const int q = min(1 + s, nz);
                X[s] = S[q * ZF_CB + c];
                W[s] = DEN[q];
            }
            double d = 0.0;
            for (int k0 = 1; k0 <= nz; k0 += ZF_UF) {
#pragma unroll
                for (int s = 0; s < ZF_UF; s++) {
                    const int kz = k0 + s, q = min(kz + ZF_UF, nz);
                    d = zl_fwd(k, X[s], d, W[s], kz == 1);
                    X[s] = S[q * ZF_CB + c];
                    W[s] = DEN[q];
                    S[kz * ZF_CB + c] = d;
                }
            }
        }
        {
            double X[ZF_UB], W[ZF_UB]; // d_k and cp[k]
#pragma unroll
            for (int s = 0; s < ZF_UB; s++) {
                const int q = max(nz - s, 1);
                X[s] = S[q * ZF_CB + c];
                W[s] = CP[q];
            }
            double u = 0.0;
            for (int k0 = nz; k0 >= 1; k0 -= ZF_UB) {
#pragma unroll
                for (int s = 0; s < ZF_UB; s++) {
                    const int kz = k0 - s, q = max(kz - ZF_UB, 1);
                    u = zl_bwd(X[s], u, W[s], kz == nz);
                    X[s] = S[q * ZF_CB + c];
                    W[s] = CP[q];
                    S[kz * ZF_CB + c] = u;
                }
            }
        }
    }
    __syncthreads();

    // ---- C ----
    if (has) {
#pragma unroll 4
        for (int kz = 1 + pz; kz <= nz; kz += ZF_T / ZF_CB) {
            const int64_t p = base + (int64_t)kz * ldz;
            out[p] = zl_relax<ZV>(k, ZV ? 0.0 : v[p], S[kz * ZF_CB + c]);
        }
    }
}

} // namespace
