// gs_semi_device.hpp — kernels of the XY semi-coarsening transfers (include/gpusolve_semi.h holds the definitions;
// tables and evaluation order are include/gpusolve_transfer.h's on axes 0 and 1). Included after gs_device.hpp by
// gs_semi.hip only. Built with -ffp-contract=off: every product and sum below is rounded once, in the order written.
// The kernels are gs_transfer_device.hpp's with the z pass taken out: plane z of one level pairs with plane z of the
// other, so nothing is carried from plane to plane.
#pragma once

namespace {

// the device tables of the two coarsened axes (gs_transfer_tables' pointers), by value in the kernel arguments
struct XyTables {
    const int32_t* pj[2];
    const double* pt[2];
    const int32_t* rlo[2];
    const int32_t* rcnt[2];
    const double* rw[2];
};

__device__ __forceinline__ int xy_clamp(int v, int lo, int hi) { return min(max(v, lo), hi); }

// ---------------------------------------------------------------------------------------------
// Restriction of a stored field: one coarse point per thread; the separable sum X, then Y over the point's rcnt <= 4
// fine indices per axis (all interior: no ring value is read). Table values are clamped into the fine interior, so
// tables that do not belong to the levels cannot take a load out of the field.
__global__ __launch_bounds__(256) void k_restrict_xy(XyTables T, const double* __restrict__ fine,
                                                     double* __restrict__ coarse, int cnx, int cny, int fnx, int fny,
                                                     int64_t fldy, int64_t fldz, int64_t cldy, int64_t cldz)
{
    const int X = 1 + blockIdx.x * 64 + threadIdx.x;
    const int Y = 1 + blockIdx.y * 4 + threadIdx.y;
    const int Z = 1 + blockIdx.z;
    if (X > cnx || Y > cny) return;
    const int x0 = xy_clamp(T.rlo[0][X], 1, fnx), nxw = xy_clamp(T.rcnt[0][X], 0, min(4, fnx - x0 + 1));
    const int y0 = xy_clamp(T.rlo[1][Y], 1, fny), nyw = xy_clamp(T.rcnt[1][Y], 0, min(4, fny - y0 + 1));
    double wx[4], wy[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        wx[k] = T.rw[0][4 * X + k];
        wy[k] = T.rw[1][4 * Y + k];
    }
    double ay = 0.0;
#pragma unroll
    for (int b = 0; b < 4; b++) {
        if (b >= nyw) break;
        const double* row = fine + x0 + (int64_t)(y0 + b) * fldy + (int64_t)Z * fldz;
        double ax = 0.0;
#pragma unroll
        for (int a = 0; a < 4; a++) {
            if (a >= nxw) break;
            const double t = wx[a] * row[a];
            ax = a == 0 ? t : ax + t;
        }
        const double t = wy[b] * ax;
        ay = b == 0 ? t : ay + t;
    }
    coarse[X + Y * cldy + (int64_t)Z * cldz] = ay;
}

// ---------------------------------------------------------------------------------------------
// fine_v += P_xy c: two fine interior x-points per thread (x odd, x + 1), each the X, then Y pass over the 2 x 2
// coarse points around it on the point's own plane (the coarse ring included, as data). The pair goes as one 16-byte
// load / store where the layout aligns it (al), else as two words.
__global__ __launch_bounds__(256) void k_prolong_add_xy(XyTables T, const double* __restrict__ c,
                                                        double* __restrict__ fv, int fnx, int fny, int cnx, int cny,
                                                        int64_t fldy, int64_t fldz, int64_t cldy, int64_t cldz, int al)
{
    const int x = 1 + 2 * (blockIdx.x * 64 + threadIdx.x);
    const int y = 1 + blockIdx.y * 4 + threadIdx.y;
    const int z = 1 + blockIdx.z;
    if (x > fnx || y > fny) return;
    const bool two = x + 1 <= fnx;
    const int x1 = two ? x + 1 : x;
    const int jy = xy_clamp(T.pj[1][y], 0, cny);
    const double ty = T.pt[1][y];
    const double ay = 1.0 - ty;
    auto point = [&](int xx) -> double {
        const int jx = xy_clamp(T.pj[0][xx], 0, cnx);
        const double tx = T.pt[0][xx], ax = 1.0 - tx;
        auto X = [&](int yy) -> double {
            const int64_t q = jx + yy * cldy + (int64_t)z * cldz;
            return ax * c[q] + tx * c[q + 1];
        };
        return ay * X(jy) + ty * X(jy + 1);
    };
    const double e0 = point(x), e1 = point(x1);
    const int64_t p = x + y * fldy + (int64_t)z * fldz;
    if (two && al) {
        const double2 v = ld2(fv + p);
        st2s<false>(fv + p, v.x + e0, v.y + e1);
    } else {
        fv[p] = fv[p] + e0;
        if (two) fv[p + 1] = fv[p + 1] + e1;
    }
}

// ---------------------------------------------------------------------------------------------
// coarse f = R_xy (f - A v), LINEAR, the fine residual never stored: gs_transfer_device.hpp's k_resrestrict_pa
// without its z pass. A block owns XY_TXC x XY_TYC coarse columns and marches a chunk of planes (fine plane z feeds
// coarse plane z):
//  - the fine region starts at (rlo_x[X0], rlo_y[Y0]) and is at most (2 XY_TXC + 2) x (2 XY_TYC + 2) points per plane
//    (the windows of T + 1 coarse points span less than (T + 1) * 2 fine indices);
//  - the v tile of the region with a one-point halo lives in a three-plane LDS ring (planes z-1 .. z+1), loads
//    coalesced along x and one plane ahead in registers, as are f's;
//  - per plane the residual of the region goes to LDS, the x-pass (every thread's own coarse column: its <= 4
//    x-weights are read once) writes coarse-x by fine-y sums to LDS, the y-pass (<= 4 y-weights, read once) leaves
//    one value per thread, which is the coarse point: stored at once.
// Every sum is the one gs_restrict_xy forms and every residual gs_residual's expression. Every table value is clamped
// into the fine interior and the LDS tile, so tables that do not belong to the levels cannot take an access out of
// either.
constexpr int XY_TXC = 64, XY_TYC = 4, XY_T = XY_TXC * XY_TYC;
constexpr int XY_FX = 2 * XY_TXC + 2, XY_FY = 2 * XY_TYC + 2; // residual region per plane, at most
constexpr int XY_VX = XY_FX + 2, XY_VY = XY_FY + 2;           // v tile per plane (one-point halo)
constexpr int XY_VP = XY_VX * XY_VY, XY_RP = XY_FX * XY_FY, XY_XP = XY_TXC * XY_FY;
constexpr int XY_NV = (XY_VP + XY_T - 1) / XY_T; // v tile points per thread and plane
constexpr int XY_NR = (XY_RP + XY_T - 1) / XY_T; // residual points per thread and plane
constexpr int XY_NX = (XY_FY + XY_TYC - 1) / XY_TYC; // x-pass rows per thread and plane

struct XyStencil {
    int lds[7]; // ox + oy * XY_VX (in-plane LDS offset)
    int oz[7];
};

__global__ __launch_bounds__(XY_T) void k_resrestrict_xy(Coef k, XyStencil so, XyTables T, const double* __restrict__ v,
                                                         const double* __restrict__ f, double* __restrict__ cf, int fnx,
                                                         int fny, int nz, int64_t fldy, int64_t fldz, int cnx, int cny,
                                                         int64_t cldy, int64_t cldz, int ZC)
{
    // one LDS array addressed with integer offsets: v ring slots 0..2, then the residual plane, then the x-pass plane
    constexpr int R0 = 3 * XY_VP, X0L = R0 + XY_RP;
    __shared__ double lds[3 * XY_VP + XY_RP + XY_XP];
    const int tid = threadIdx.x;
    const int X0 = 1 + blockIdx.x * XY_TXC, Y0 = 1 + blockIdx.y * XY_TYC;
    const int zb = 1 + blockIdx.z * ZC, ze = min(zb + ZC - 1, nz);
    if (zb > ze) return;
    const int Xe = min(X0 + XY_TXC - 1, cnx), Ye = min(Y0 + XY_TYC - 1, cny);
    // the fine region of this block (clamped into the fine interior and the LDS tile whatever the tables hold)
    const int fx0 = xy_clamp(T.rlo[0][X0], 1, fnx), fy0 = xy_clamp(T.rlo[1][Y0], 1, fny);
    const int fxw = xy_clamp(T.rlo[0][Xe] + T.rcnt[0][Xe] - fx0, 0, min(XY_FX, fnx - fx0 + 1));
    const int fyw = xy_clamp(T.rlo[1][Ye] + T.rcnt[1][Ye] - fy0, 0, min(XY_FY, fny - fy0 + 1));

    // this thread's v-tile points (clamped into the padded level: clamped copies are never used)
    int64_t voff[XY_NV];
#pragma unroll
    for (int i = 0; i < XY_NV; i++) {
        const int e = min(tid + i * XY_T, XY_VP - 1);
        const int ly = e / XY_VX, lx = e - ly * XY_VX;
        voff[i] = min(fx0 - 1 + lx, fnx + 1) + (int64_t)min(fy0 - 1 + ly, fny + 1) * fldy;
    }
    // this thread's residual points: global offset, LDS position, whether the point is in the region
    int64_t roff[XY_NR];
    int rpos[XY_NR];
    bool rin[XY_NR];
#pragma unroll
    for (int i = 0; i < XY_NR; i++) {
        const int e = min(tid + i * XY_T, XY_RP - 1);
        const int ry = e / XY_FX, rx = e - ry * XY_FX;
        rin[i] = tid + i * XY_T < XY_RP && rx < fxw && ry < fyw;
        roff[i] = min(fx0 + rx, fnx) + (int64_t)min(fy0 + ry, fny) * fldy;
        rpos[i] = (ry + 1) * XY_VX + rx + 1;
    }
    // this thread's coarse column (x- and y-pass): table rows read once
    const int cx = tid % XY_TXC, cy = tid / XY_TXC;
    const int X = X0 + cx, Y = Y0 + cy;
    const bool xin = X <= cnx, yin = Y <= cny;
    const int Xc = min(X, cnx), Yc = min(Y, cny);
    const int xlo = xy_clamp(T.rlo[0][Xc] - fx0, 0, XY_FX - 1), xn = xy_clamp(T.rcnt[0][Xc], 0, min(4, XY_FX - xlo));
    const int ylo = xy_clamp(T.rlo[1][Yc] - fy0, 0, XY_FY - 1), yn = xy_clamp(T.rcnt[1][Yc], 0, min(4, XY_FY - ylo));
    double wx[4], wy[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        wx[q] = T.rw[0][4 * Xc + q];
        wy[q] = T.rw[1][4 * Yc + q];
    }

    auto load_v = [&](double (&dst)[XY_NV], int fz) {
        const int64_t o = (int64_t)xy_clamp(fz, 0, nz + 1) * fldz;
#pragma unroll
        for (int i = 0; i < XY_NV; i++) dst[i] = v[voff[i] + o];
    };
    auto store_v = [&](const double (&src)[XY_NV], int fz) {
        const int d = (fz % 3) * XY_VP;
#pragma unroll
        for (int i = 0; i < XY_NV; i++)
            if (tid + i * XY_T < XY_VP) lds[d + tid + i * XY_T] = src[i];
    };
    auto load_f = [&](double (&F)[XY_NR], int fz) {
        const int64_t o = (int64_t)xy_clamp(fz, 1, nz) * fldz;
#pragma unroll
        for (int i = 0; i < XY_NR; i++) F[i] = __builtin_nontemporal_load(f + roff[i] + o);
    };
    // r on plane fz (interior) from the v ring, which holds planes fz-1 .. fz+1
    auto residual_plane = [&](const double (&F)[XY_NR], int fz) {
        int toff[7];
#pragma unroll
        for (int t = 0; t < 7; t++) toff[t] = ((fz + so.oz[t]) % 3) * XY_VP + so.lds[t];
        const int coff = (fz % 3) * XY_VP;
#pragma unroll
        for (int i = 0; i < XY_NR; i++) {
            if (tid + i * XY_T >= XY_RP) continue;
            double r = 0.0;
            if (rin[i]) {
                double sum;
                if (k.unit) { // stencil_sum<true>'s form, term by term (as k_generic)
                    sum = __builtin_fma(k.s[0], lds[rpos[i] + toff[0]], 0.0);
#pragma unroll
                    for (int t = 1; t < 7; t++) sum = sum - lds[rpos[i] + toff[t]];
                } else {
                    sum = 0.0;
#pragma unroll
                    for (int t = 0; t < 7; t++) sum += k.s[t] * lds[rpos[i] + toff[t]];
                }
                const double c = lds[rpos[i] + coff];
                const double q = op_finish<GS_LINEAR>(k, div_hh(k, sum), c, 0.0);
                r = F[i] - q;
            }
            lds[R0 + tid + i * XY_T] = r;
        }
    };

    double VN[XY_NV], FN[XY_NR];
    // prologue: v planes zb-1 .. zb+1 into the ring, f of plane zb in registers
    load_v(VN, zb - 1);
    store_v(VN, zb - 1);
    load_v(VN, zb);
    store_v(VN, zb);
    load_v(VN, zb + 1);
    store_v(VN, zb + 1);
    load_f(FN, zb);
    __syncthreads();

    for (int fz = zb; fz <= ze; fz++) {
        double FC[XY_NR];
#pragma unroll
        for (int i = 0; i < XY_NR; i++) FC[i] = FN[i];
        if (fz < ze) { // the next plane's operands, in flight during this plane's arithmetic
            load_v(VN, fz + 2);
            load_f(FN, fz + 1);
        }
        residual_plane(FC, fz);
        __syncthreads(); // the residual plane is complete; nobody reads v plane fz-1 any more
        if (fz < ze) store_v(VN, fz + 2); // into the slot of plane fz-1
        // x-pass: coarse column cx, fine rows cy, cy + XY_TYC, ...
#pragma unroll
        for (int i = 0; i < XY_NX; i++) {
            const int ry = cy + i * XY_TYC;
            if (ry >= XY_FY) continue;
            double a = 0.0;
            if (xin && ry < fyw) {
                const int o = R0 + ry * XY_FX + xlo;
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    if (q >= xn) break;
                    const double t = wx[q] * lds[o + q];
                    a = q == 0 ? t : a + t;
                }
            }
            lds[X0L + ry * XY_TXC + cx] = a;
        }
        __syncthreads(); // the x-pass plane is complete; the next v plane is in the ring
        // y-pass: the coarse point
        if (xin && yin) {
            double a = 0.0;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                if (q >= yn) break;
                const double t = wy[q] * lds[X0L + (ylo + q) * XY_TXC + cx];
                a = q == 0 ? t : a + t;
            }
            cf[X + Y * cldy + (int64_t)fz * cldz] = a;
        }
        // (the next step's x-pass writes follow its own barrier: no thread still reads this plane's sums then)
    }
}

} // namespace
