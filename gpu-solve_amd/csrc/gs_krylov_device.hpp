// gs_krylov_device.hpp — the kernels of libgpusolve_krylov.so (include/gpusolve_krylov.h): the three level-0 passes
// of preconditioned conjugate gradients and the one-block scalar update. gs_device.hpp gives Coef, the stencil's
// point expressions (stencil_sum, div_hh), the lane shifts, the streamed loads / stores and block_sum; no kernel of
// it is launched from here. Internal linkage. Built with -ffp-contract=off: every expression rounds as written.
#pragma once
#include "gs_device.hpp"

#include "gpusolve_krylov.h"

namespace {

// the new direction at one point: fl(z + fl(beta * p)); FIRST: the first direction, p_out = z (no p is read)
template <bool FIRST>
__device__ __forceinline__ double pcg_comb(double z, double p, double beta)
{
    if (FIRST) return z;
    const double t = beta * p;
    return z + t;
}
template <bool FIRST>
__device__ __forceinline__ double2 pcg_comb2(double2 z, double2 p, double beta)
{
    return make_double2(pcg_comb<FIRST>(z.x, p.x, beta), pcg_comb<FIRST>(z.y, p.y, beta));
}

// ---------------------------------------------------------------------------------------------
// gs_pcg_dir, register-blocked z-march: k_rb's shape (gs_device.hpp: a lane owns one dwordx4 pair of RY rows, a wave
// a 128 x RY tile, W waves stack in y, the block walks ZC planes; x-neighbours by DPP wave shift with wave-uniform
// edge loads, two halo rows per wave and plane, the loads of plane z+1 issued before plane z's arithmetic,
// non-temporal stores) with TWO input streams: every value the stencil reads — the lane's rows of three planes, the
// halo rows, the tile edges — is the new direction formed from the loaded z and p_in where it is consumed, so p_out
// is written once and never read back. The slots hold raw z / p_in; P and C hold formed directions.
// Canonical stencil order only (k_pcg_dir_gen takes the rest). Columns, rows and planes are clamped into the padded
// box as in k_rb; the ring holds zeros, so a direction formed there is +0, the value p_out's ring has.
template <bool UN, bool FIRST, int RY, int W>
__global__ __launch_bounds__(WAVE* W) void k_pcg_dir_rb(Coef k, const double* __restrict__ zf,
                                                         const double* __restrict__ pf, double* __restrict__ pout,
                                                         double* __restrict__ qout, const double* __restrict__ beta_dev,
                                                         double* __restrict__ partials, int nx, int ny, int nz,
                                                         int64_t ldy, int64_t ldz, int ZC)
{
    __shared__ double red[W];
    const int lane = threadIdx.x;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.y);
    const int64_t tile = blockIdx.x + gridDim.x * ((int64_t)blockIdx.y + gridDim.y * (int64_t)blockIdx.z);
    const int x0 = 1 + blockIdx.x * (2 * WAVE);
    const int x = x0 + 2 * lane;
    const int xl = min(x, nx + 1);
    const int y0 = 1 + (blockIdx.y * W + wv) * RY;
    const int zb = 1 + blockIdx.z * ZC;
    const int ze = min(zb + ZC - 1, nz);
    const int xle = x0 - 1;
    const int xre = min(x0 + 2 * WAVE, nx + 1);
    const bool okx0 = x <= nx, okx1 = x + 1 <= nx;
    const double beta = FIRST ? 0.0 : *beta_dev;

    int64_t roff[RY + 2]; // rows y0-1 .. y0+RY (clamped into the padded range)
#pragma unroll
    for (int r = 0; r < RY + 2; r++) roff[r] = (int64_t)min(y0 - 1 + r, ny + 1) * ldy;

    double2 P[RY], C[RY];
    double2 NZ[2][RY], NP[2][RY], HZ[2][2], HP[2][2];
    double EZ[2][RY], EP[2][RY], FZ[2][RY], FP[2][RY]; // left (E) and right (F) tile-edge values
    double dot = 0.0;
    auto ld2p = [&](int64_t o) { return FIRST ? make_double2(0.0, 0.0) : ld2(pf + o); };
    auto ld1p = [&](int64_t o) { return FIRST ? 0.0 : pf[o]; };
    // slot s <- plane z1's halo rows and edges, plane z2's own rows (plane offsets)
    auto load_slot = [&](const int s, const int64_t z1, const int64_t z2) {
#pragma unroll
        for (int r = 0; r < RY; r++) {
            NZ[s][r] = ld2(zf + xl + roff[r + 1] + z2);
            NP[s][r] = ld2p(xl + roff[r + 1] + z2);
            EZ[s][r] = zf[xle + roff[r + 1] + z1];
            EP[s][r] = ld1p(xle + roff[r + 1] + z1);
            FZ[s][r] = zf[xre + roff[r + 1] + z1];
            FP[s][r] = ld1p(xre + roff[r + 1] + z1);
        }
        HZ[s][0] = ld2(zf + xl + roff[0] + z1);
        HP[s][0] = ld2p(xl + roff[0] + z1);
        HZ[s][1] = ld2(zf + xl + roff[RY + 1] + z1);
        HP[s][1] = ld2p(xl + roff[RY + 1] + z1);
    };
    if (zb <= ze) {
        const int64_t zo = (int64_t)zb * ldz;
#pragma unroll
        for (int r = 0; r < RY; r++) {
            P[r] = pcg_comb2<FIRST>(ld2(zf + xl + roff[r + 1] + zo - ldz), ld2p(xl + roff[r + 1] + zo - ldz), beta);
            C[r] = pcg_comb2<FIRST>(ld2(zf + xl + roff[r + 1] + zo), ld2p(xl + roff[r + 1] + zo), beta);
        }
        load_slot(1, zo, zo + ldz);
    }
    // both halves always run and every load is unconditional (indices clamped), as in k_rb
    for (int z0 = zb; z0 <= ze; z0 += 2) {
#pragma unroll
        for (int ph = 0; ph < 2; ph++) {
            const int z = z0 + ph;
            const bool real = z <= ze;
            const int cs = ph ^ 1; // slot holding plane z
            const int64_t zo = (int64_t)z * ldz;
            load_slot(ph, (int64_t)min(z + 1, nz + 1) * ldz, (int64_t)min(z + 2, nz + 1) * ldz);
            double2 N[RY];
#pragma unroll
            for (int r = 0; r < RY; r++) N[r] = pcg_comb2<FIRST>(NZ[cs][r], NP[cs][r], beta);
            const double2 h0 = pcg_comb2<FIRST>(HZ[cs][0], HP[cs][0], beta);
            const double2 h1 = pcg_comb2<FIRST>(HZ[cs][1], HP[cs][1], beta);
#pragma unroll
            for (int r = 0; r < RY; r++) {
                const double2 c = C[r], ym = r == 0 ? h0 : C[r - 1], yp = r == RY - 1 ? h1 : C[r + 1];
                const double2 zm = P[r], zp = N[r];
                const double xm0 = lane_from_left<true>(c.y, pcg_comb<FIRST>(EZ[cs][r], EP[cs][r], beta));
                const double xp1 = lane_from_right<true>(c.x, pcg_comb<FIRST>(FZ[cs][r], FP[cs][r], beta));
                const double q0 = div_hh(k, stencil_sum<UN>(k, c.x, c.y, xm0, yp.x, ym.x, zp.x, zm.x));
                const double q1 = div_hh(k, stencil_sum<UN>(k, c.y, xp1, c.x, yp.y, ym.y, zp.y, zm.y));
                const bool rowok = real && y0 + r <= ny;
                if (rowok && okx0) dot += c.x * q0;
                if (rowok && okx1) dot += c.y * q1;
                if (rowok) {
                    const int64_t o = x + roff[r + 1] + zo;
                    if (okx1) {
                        st2s<true>(pout + o, c.x, c.y);
                        st2s<true>(qout + o, q0, q1);
                    } else if (okx0) {
                        pout[o] = c.x;
                        qout[o] = q0;
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < RY; r++) {
                P[r] = C[r];
                C[r] = N[r];
            }
        }
    }
    const double t = block_sum<W>(dot, red);
    if (threadIdx.x == 0 && threadIdx.y == 0) partials[tile] = t;
}

// gs_pcg_dir, one point per thread (k_generic's shape): any 7 offsets in {-1,0,1}^3 in any order, and the levels too
// small for the z-march. The sum's form is k_generic's, term by term in the stencil's order.
template <bool FIRST>
__global__ __launch_bounds__(256) void k_pcg_dir_gen(Coef k, const double* __restrict__ zf,
                                                     const double* __restrict__ pf, double* __restrict__ pout,
                                                     double* __restrict__ qout, const double* __restrict__ beta_dev,
                                                     double* __restrict__ partials, int nx, int ny, int nz,
                                                     int64_t ldy, int64_t ldz)
{
    __shared__ double red[GN_BY];
    const int x = 1 + blockIdx.x * GN_BX + threadIdx.x;
    const int y = 1 + blockIdx.y * GN_BY + threadIdx.y;
    const int z = 1 + blockIdx.z;
    const double beta = FIRST ? 0.0 : *beta_dev;
    double dot = 0.0;
    if (x <= nx && y <= ny) {
        const int64_t p = x + y * ldy + (int64_t)z * ldz;
        auto at = [&](int64_t o) { return pcg_comb<FIRST>(zf[o], FIRST ? 0.0 : pf[o], beta); };
        double s = 0.0;
        if (k.unit) {
            s = __builtin_fma(k.s[0], at(p + k.off[0]), 0.0);
#pragma unroll
            for (int i = 1; i < 7; i++) s = s - at(p + k.off[i]);
        } else {
#pragma unroll
            for (int i = 0; i < 7; i++) s += k.s[i] * at(p + k.off[i]);
        }
        const double qv = div_hh(k, s);
        const double c = at(p);
        pout[p] = c;
        qout[p] = qv;
        dot = c * qv;
    }
    const double t = block_sum<GN_BY>(dot, red);
    if (threadIdx.x == 0 && threadIdx.y == 0)
        partials[blockIdx.x + gridDim.x * ((int64_t)blockIdx.y + gridDim.y * (int64_t)blockIdx.z)] = t;
}

// ---------------------------------------------------------------------------------------------
// The two element-wise passes: a lane owns one pair (x, x+1) of one row, a block 128 columns x KV_BY rows, and walks
// ZC planes. Only interior pairs are loaded (x <= nx, so x+1 <= nx+1 stays inside the padded row).
constexpr int KV_BY = 4;

// x += alpha p, r -= alpha q, partial sums of the new r . r. alpha == 0 (a breakdown): nothing is stored
__global__ __launch_bounds__(WAVE* KV_BY) void k_pcg_step(double* __restrict__ xf, double* __restrict__ rf,
                                                          const double* __restrict__ pf, const double* __restrict__ qf,
                                                          const double* __restrict__ alpha_dev,
                                                          double* __restrict__ partials, int nx, int ny, int nz,
                                                          int64_t ldy, int64_t ldz, int ZC)
{
    __shared__ double red[KV_BY];
    const int x = 1 + (blockIdx.x * WAVE + threadIdx.x) * 2;
    const int y = 1 + blockIdx.y * KV_BY + threadIdx.y;
    const int zb = 1 + blockIdx.z * ZC, ze = min(zb + ZC - 1, nz);
    const double alpha = *alpha_dev;
    const bool store = alpha != 0.0;
    const bool ok0 = x <= nx && y <= ny, ok1 = x + 1 <= nx;
    double rr = 0.0;
    if (ok0) {
        int64_t o = x + (int64_t)y * ldy + (int64_t)zb * ldz;
        for (int z = zb; z <= ze; z++, o += ldz) {
            const double2 xv = ld2(xf + o), rv = ld2(rf + o), pv = ld2s<true>(pf + o), qv = ld2s<true>(qf + o);
            const double ap0 = alpha * pv.x, ap1 = alpha * pv.y, aq0 = alpha * qv.x, aq1 = alpha * qv.y;
            const double x0 = xv.x + ap0, x1 = xv.y + ap1;
            const double r0 = store ? rv.x - aq0 : rv.x, r1 = store ? rv.y - aq1 : rv.y;
            rr += r0 * r0;
            if (ok1) rr += r1 * r1;
            if (store) {
                if (ok1) {
                    st2s<true>(xf + o, x0, x1);
                    st2s<true>(rf + o, r0, r1);
                } else {
                    xf[o] = x0;
                    rf[o] = r0;
                }
            }
        }
    }
    const double t = block_sum<KV_BY>(rr, red);
    if (threadIdx.x == 0 && threadIdx.y == 0)
        partials[blockIdx.x + gridDim.x * ((int64_t)blockIdx.y + gridDim.y * (int64_t)blockIdx.z)] = t;
}

__global__ __launch_bounds__(WAVE* KV_BY) void k_dot(const double* __restrict__ af, const double* __restrict__ bf,
                                                     double* __restrict__ partials, int nx, int ny, int nz, int64_t ldy,
                                                     int64_t ldz, int ZC)
{
    __shared__ double red[KV_BY];
    const int x = 1 + (blockIdx.x * WAVE + threadIdx.x) * 2;
    const int y = 1 + blockIdx.y * KV_BY + threadIdx.y;
    const int zb = 1 + blockIdx.z * ZC, ze = min(zb + ZC - 1, nz);
    const bool ok0 = x <= nx && y <= ny, ok1 = x + 1 <= nx;
    double s = 0.0;
    if (ok0) {
        int64_t o = x + (int64_t)y * ldy + (int64_t)zb * ldz;
        for (int z = zb; z <= ze; z++, o += ldz) {
            const double2 a = ld2(af + o), b = ld2(bf + o);
            s += a.x * b.x;
            if (ok1) s += a.y * b.y;
        }
    }
    const double t = block_sum<KV_BY>(s, red);
    if (threadIdx.x == 0 && threadIdx.y == 0)
        partials[blockIdx.x + gridDim.x * ((int64_t)blockIdx.y + gridDim.y * (int64_t)blockIdx.z)] = t;
}

// ---------------------------------------------------------------------------------------------
// The scalar update: k_sumsq_finish's fixed strided sum, then thread 0 updates the record (gpusolve_krylov.h).
__global__ __launch_bounds__(FIN_T) void k_pcg_scalars(int what, const double* __restrict__ partials, int64_t n,
                                                       double* __restrict__ rec, double* __restrict__ slot)
{
    __shared__ double red[FIN_T / WAVE];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += FIN_T) s += partials[i];
    const double t = block_sum<FIN_T / WAVE>(s, red);
    if (threadIdx.x != 0) return;
    const bool finite = __builtin_fabs(t) < __builtin_inf(); // (false for a NaN)
    const bool pos = finite && t > 0.0;
    const double kept = finite ? t : 0.0;
    if (what == GS_PCG_RZ_FIRST) {
        rec[GS_PCG_RZ_I] = kept;
        rec[GS_PCG_PQ_I] = 0.0;
        rec[GS_PCG_ALPHA_I] = 0.0;
        rec[GS_PCG_BETA_I] = 0.0;
        rec[GS_PCG_RR_I] = 0.0;
        rec[GS_PCG_FLAG_I] = pos ? 0.0 : (double)GS_PCG_BAD_RZ;
        for (int i = GS_PCG_FLAG_I + 1; i < GS_PCG_REC; i++) rec[i] = 0.0;
        return;
    }
    int flag = (int)rec[GS_PCG_FLAG_I];
    if (what == GS_PCG_PQ) {
        double a = pos ? rec[GS_PCG_RZ_I] / t : 0.0;
        if (!pos || !(__builtin_fabs(a) < __builtin_inf())) flag |= GS_PCG_BAD_PQ; // (a quotient that overflows too)
        rec[GS_PCG_PQ_I] = kept;
        rec[GS_PCG_ALPHA_I] = flag ? 0.0 : a;
        rec[GS_PCG_FLAG_I] = (double)flag;
    } else if (what == GS_PCG_RZ) {
        double b = pos ? t / rec[GS_PCG_RZ_I] : 0.0;
        if (!pos || !(__builtin_fabs(b) < __builtin_inf())) flag |= GS_PCG_BAD_RZ;
        rec[GS_PCG_BETA_I] = flag ? 0.0 : b;
        rec[GS_PCG_RZ_I] = kept;
        rec[GS_PCG_FLAG_I] = (double)flag;
    } else {
        if (!finite) flag |= GS_PCG_BAD_RR; // (r overflowed or holds a NaN: the 0 stored is not a norm)
        rec[GS_PCG_RR_I] = kept;
        rec[GS_PCG_FLAG_I] = (double)flag;
        if (slot)
            for (int i = 0; i < GS_PCG_REC; i++) slot[i] = rec[i];
    }
}

} // namespace
