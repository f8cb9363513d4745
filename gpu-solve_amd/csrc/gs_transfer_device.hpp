// gs_transfer_device.hpp — kernels of the position-aware grid transfers (include/gpusolve_transfer.h holds the
// definitions: tables, evaluation order). Included after gs_device.hpp by gs_transfer.hip only. Built with
// -ffp-contract=off: every product and sum below is rounded once, in the order written.
#pragma once

namespace {

// the device tables of one transition (gs_transfer_tables' pointers), by value in the kernel arguments
struct PaTables {
    const int32_t* pj[3];
    const double* pt[3];
    const int32_t* rlo[3];
    const int32_t* rcnt[3];
    const double* rw[3];
};

__device__ __forceinline__ int pa_clamp(int v, int lo, int hi) { return min(max(v, lo), hi); }

// ---------------------------------------------------------------------------------------------
// Restriction of a stored field: one coarse point per thread; the separable sum X, then Y, then Z over the point's
// rcnt <= 4 fine indices per axis (all interior: no ring value is read). Table values are clamped into the fine
// interior, so tables that do not belong to the levels cannot take a load out of the field.
__global__ __launch_bounds__(256) void k_restrict_pa(PaTables T, const double* __restrict__ fine,
                                                     double* __restrict__ ca, double* __restrict__ cb, int cnx, int cny,
                                                     int fnx, int fny, int fnz, int64_t fldy, int64_t fldz,
                                                     int64_t cldy, int64_t cldz)
{
    const int X = 1 + blockIdx.x * 64 + threadIdx.x;
    const int Y = 1 + blockIdx.y * 4 + threadIdx.y;
    const int Z = 1 + blockIdx.z;
    if (X > cnx || Y > cny) return;
    const int x0 = pa_clamp(T.rlo[0][X], 1, fnx), nxw = pa_clamp(T.rcnt[0][X], 0, min(4, fnx - x0 + 1));
    const int y0 = pa_clamp(T.rlo[1][Y], 1, fny), nyw = pa_clamp(T.rcnt[1][Y], 0, min(4, fny - y0 + 1));
    const int z0 = pa_clamp(T.rlo[2][Z], 1, fnz), nzw = pa_clamp(T.rcnt[2][Z], 0, min(4, fnz - z0 + 1));
    double wx[4], wy[4], wz[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        wx[k] = T.rw[0][4 * X + k];
        wy[k] = T.rw[1][4 * Y + k];
        wz[k] = T.rw[2][4 * Z + k];
    }
    double az = 0.0;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        if (c >= nzw) break;
        double ay = 0.0;
#pragma unroll
        for (int b = 0; b < 4; b++) {
            if (b >= nyw) break;
            const double* row = fine + x0 + (int64_t)(y0 + b) * fldy + (int64_t)(z0 + c) * fldz;
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
        const double t = wz[c] * ay;
        az = c == 0 ? t : az + t;
    }
    const int64_t q = X + Y * cldy + (int64_t)Z * cldz;
    ca[q] = az;
    if (cb) cb[q] = az;
}

// ---------------------------------------------------------------------------------------------
// fine_v += P (c - sub): two fine interior x-points per thread (x odd, x + 1: one pair load / store of v, as
// k_prolong_add), each the X, then Y, then Z pass over the 2 x 2 x 2 coarse points around it (the coarse ring
// included, as data).
template <bool SUB>
__global__ __launch_bounds__(256) void k_prolong_add_pa(PaTables T, const double* __restrict__ c,
                                                        const double* __restrict__ sub, double* __restrict__ fv, int fnx,
                                                        int fny, int cnx, int cny, int cnz, int64_t fldy, int64_t fldz,
                                                        int64_t cldy, int64_t cldz)
{
    const int x = 1 + 2 * (blockIdx.x * 64 + threadIdx.x);
    const int y = 1 + blockIdx.y * 4 + threadIdx.y;
    const int z = 1 + blockIdx.z;
    if (x > fnx || y > fny) return;
    const bool two = x + 1 <= fnx;
    const int x1 = two ? x + 1 : x;
    const int jy = pa_clamp(T.pj[1][y], 0, cny), jz = pa_clamp(T.pj[2][z], 0, cnz);
    const double ty = T.pt[1][y], tz = T.pt[2][z];
    const double ay = 1.0 - ty, az = 1.0 - tz;
    auto point = [&](int xx) -> double {
        const int jx = pa_clamp(T.pj[0][xx], 0, cnx);
        const double tx = T.pt[0][xx], ax = 1.0 - tx;
        auto X = [&](int yy, int zz) -> double {
            const int64_t q = jx + yy * cldy + (int64_t)zz * cldz;
            const double d0 = SUB ? c[q] - sub[q] : c[q], d1 = SUB ? c[q + 1] - sub[q + 1] : c[q + 1];
            return ax * d0 + tx * d1;
        };
        auto Y = [&](int zz) -> double { return ay * X(jy, zz) + ty * X(jy + 1, zz); };
        return az * Y(jz) + tz * Y(jz + 1);
    };
    const double e0 = point(x), e1 = point(x1);
    const int64_t p = x + y * fldy + (int64_t)z * fldz;
    if (two) {
        const double2 v = ld2(fv + p);
        st2s<true>(fv + p, v.x + e0, v.y + e1);
    } else {
        fv[p] = fv[p] + e0;
    }
}

// ---------------------------------------------------------------------------------------------
// coarse f = R (f - A v) with the fine residual never stored. The shape of gs_device.hpp's k_resrestrict — a block
// owns PA_TXC x PA_TYC coarse columns and marches a chunk of coarse planes, v tile with a one-point halo in an LDS
// ring, loads coalesced along x and one plane ahead in registers — with the table-driven operator:
//  - the fine region starts at (rlo_x[X0], rlo_y[Y0]) and is at most (2 PA_TXC + 2) x (2 PA_TYC + 2) points per plane
//    (the windows of T + 1 coarse points span less than (T + 1) * 2 fine indices);
//  - the march is over FINE planes: per plane, the residual of the region goes to LDS, the x-pass (every thread's own
//    coarse column: its <= 4 x-weights are read once) writes coarse-x by fine-y sums to LDS, the y-pass (<= 4
//    y-weights, read once) leaves one value per thread, kept in a four-plane register window;
//  - a coarse plane Z is written at the last fine plane of its window, from the window and its <= 4 z-weights.
// The windows of consecutive coarse planes overlap, so a chunk starts at rlo_z of its first coarse plane (planes
// shared with the chunk before are evaluated by both). Every sum is the one gs_restrict_pa forms and every residual
// gs_residual's expression.
constexpr int PA_TXC = 64, PA_TYC = 4, PA_T = PA_TXC * PA_TYC;
constexpr int PA_FX = 2 * PA_TXC + 2, PA_FY = 2 * PA_TYC + 2; // residual region per plane, at most
constexpr int PA_VX = PA_FX + 2, PA_VY = PA_FY + 2;           // v tile per plane (one-point halo)
constexpr int PA_VP = PA_VX * PA_VY, PA_RP = PA_FX * PA_FY, PA_XP = PA_TXC * PA_FY;
constexpr int PA_NV = (PA_VP + PA_T - 1) / PA_T; // v tile points per thread and plane
constexpr int PA_NR = (PA_RP + PA_T - 1) / PA_T; // residual points per thread and plane
constexpr int PA_NX = (PA_FY + PA_TYC - 1) / PA_TYC; // x-pass rows per thread and plane

struct PaStencil {
    int lds[7]; // ox + oy * PA_VX (in-plane LDS offset)
    int oz[7];
};

template <int MODE>
__global__ __launch_bounds__(PA_T) void k_resrestrict_pa(Coef k, PaStencil so, PaTables T, const double* __restrict__ v,
                                                         const double* __restrict__ f, const double* __restrict__ w,
                                                         double* __restrict__ cf, int fnx, int fny, int fnz,
                                                         int64_t fldy, int64_t fldz, int cnx, int cny, int cnz,
                                                         int64_t cldy, int64_t cldz, int ZC)
{
    // one LDS array addressed with integer offsets: v ring slots 0..2, then the residual plane, then the x-pass plane
    constexpr int R0 = 3 * PA_VP, X0L = R0 + PA_RP;
    __shared__ double lds[3 * PA_VP + PA_RP + PA_XP];
    const int tid = threadIdx.x;
    const int X0 = 1 + blockIdx.x * PA_TXC, Y0 = 1 + blockIdx.y * PA_TYC;
    const int Zb = 1 + blockIdx.z * ZC, Ze = min(Zb + ZC - 1, cnz);
    if (Zb > Ze) return;
    const int Xe = min(X0 + PA_TXC - 1, cnx), Ye = min(Y0 + PA_TYC - 1, cny);
    // the fine region of this block (clamped into the fine interior and the LDS tile whatever the tables hold)
    const int fx0 = pa_clamp(T.rlo[0][X0], 1, fnx), fy0 = pa_clamp(T.rlo[1][Y0], 1, fny);
    const int fxw = pa_clamp(T.rlo[0][Xe] + T.rcnt[0][Xe] - fx0, 0, min(PA_FX, fnx - fx0 + 1));
    const int fyw = pa_clamp(T.rlo[1][Ye] + T.rcnt[1][Ye] - fy0, 0, min(PA_FY, fny - fy0 + 1));
    const int fzb = pa_clamp(T.rlo[2][Zb], 1, fnz);
    const int fze = pa_clamp(T.rlo[2][Ze] + T.rcnt[2][Ze] - 1, 1, fnz);

    // this thread's v-tile points (clamped into the padded level: clamped copies are never used)
    int64_t voff[PA_NV];
#pragma unroll
    for (int i = 0; i < PA_NV; i++) {
        const int e = min(tid + i * PA_T, PA_VP - 1);
        const int ly = e / PA_VX, lx = e - ly * PA_VX;
        voff[i] = min(fx0 - 1 + lx, fnx + 1) + (int64_t)min(fy0 - 1 + ly, fny + 1) * fldy;
    }
    // this thread's residual points: global offset, LDS position, whether the point is in the region
    int64_t roff[PA_NR];
    int rpos[PA_NR];
    bool rin[PA_NR];
#pragma unroll
    for (int i = 0; i < PA_NR; i++) {
        const int e = min(tid + i * PA_T, PA_RP - 1);
        const int ry = e / PA_FX, rx = e - ry * PA_FX;
        rin[i] = tid + i * PA_T < PA_RP && rx < fxw && ry < fyw;
        roff[i] = min(fx0 + rx, fnx) + (int64_t)min(fy0 + ry, fny) * fldy;
        rpos[i] = (ry + 1) * PA_VX + rx + 1;
    }
    // this thread's coarse column (x- and y-pass): table rows read once
    const int cx = tid % PA_TXC, cy = tid / PA_TXC;
    const int X = X0 + cx, Y = Y0 + cy;
    const bool xin = X <= cnx, yin = Y <= cny;
    const int Xc = min(X, cnx), Yc = min(Y, cny);
    const int xlo = pa_clamp(T.rlo[0][Xc] - fx0, 0, PA_FX - 1), xn = pa_clamp(T.rcnt[0][Xc], 0, min(4, PA_FX - xlo));
    const int ylo = pa_clamp(T.rlo[1][Yc] - fy0, 0, PA_FY - 1), yn = pa_clamp(T.rcnt[1][Yc], 0, min(4, PA_FY - ylo));
    double wx[4], wy[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        wx[q] = T.rw[0][4 * Xc + q];
        wy[q] = T.rw[1][4 * Yc + q];
    }

    auto zo = [&](int fz) { return (int64_t)pa_clamp(fz, 0, fnz + 1) * fldz; };
    auto load_v = [&](double (&dst)[PA_NV], int fz) {
        const int64_t o = zo(fz);
#pragma unroll
        for (int i = 0; i < PA_NV; i++) dst[i] = v[voff[i] + o];
    };
    auto store_v = [&](const double (&src)[PA_NV], int fz) {
        const int d = (fz % 3) * PA_VP;
#pragma unroll
        for (int i = 0; i < PA_NV; i++)
            if (tid + i * PA_T < PA_VP) lds[d + tid + i * PA_T] = src[i];
    };
    auto load_fw = [&](double (&F)[PA_NR], double (&W)[PA_NR], int fz) {
        const int64_t o = (int64_t)pa_clamp(fz, 1, fnz) * fldz;
#pragma unroll
        for (int i = 0; i < PA_NR; i++) {
            F[i] = f[roff[i] + o];
            if (newtonish(MODE)) W[i] = w[roff[i] + o];
        }
    };
    // r on fine plane fz (interior) from the v ring, which holds planes fz-1 .. fz+1
    auto residual_plane = [&](const double (&F)[PA_NR], const double (&W)[PA_NR], int fz) {
        int toff[7];
#pragma unroll
        for (int t = 0; t < 7; t++) toff[t] = ((fz + so.oz[t]) % 3) * PA_VP + so.lds[t];
        const int coff = (fz % 3) * PA_VP;
#pragma unroll
        for (int i = 0; i < PA_NR; i++) {
            if (tid + i * PA_T >= PA_RP) continue;
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
                const double q = op_finish<MODE>(k, div_hh(k, sum), c, newtonish(MODE) ? W[i] : 0.0);
                r = F[i] - q;
            }
            lds[R0 + tid + i * PA_T] = r;
        }
    };

    double VN[PA_NV], FN[PA_NR], WN[PA_NR];
    // prologue: v planes fzb-1 .. fzb+1 into the ring, f (w) of plane fzb in registers
    load_v(VN, fzb - 1);
    store_v(VN, fzb - 1);
    load_v(VN, fzb);
    store_v(VN, fzb);
    load_v(VN, fzb + 1);
    store_v(VN, fzb + 1);
    load_fw(FN, WN, fzb);
    __syncthreads();

    double p0 = 0.0, p1 = 0.0, p2 = 0.0, p3 = 0.0; // the y-pass values of fine planes fz-3 .. fz
    int Z = Zb, zend = T.rlo[2][Zb] + T.rcnt[2][Zb] - 1;
    for (int fz = fzb; fz <= fze; fz++) {
        double FC[PA_NR], WC[PA_NR];
#pragma unroll
        for (int i = 0; i < PA_NR; i++) {
            FC[i] = FN[i];
            WC[i] = WN[i];
        }
        if (fz < fze) { // the next plane's operands, in flight during this plane's arithmetic
            load_v(VN, fz + 2);
            load_fw(FN, WN, fz + 1);
        }
        residual_plane(FC, WC, fz);
        __syncthreads(); // the residual plane is complete; nobody reads v plane fz-1 any more
        if (fz < fze) store_v(VN, fz + 2); // into the slot of plane fz-1
        // x-pass: coarse column cx, fine rows cy, cy + PA_TYC, ...
#pragma unroll
        for (int i = 0; i < PA_NX; i++) {
            const int ry = cy + i * PA_TYC;
            if (ry >= PA_FY) continue;
            double a = 0.0;
            if (xin && ry < fyw) {
                const int o = R0 + ry * PA_FX + xlo;
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    if (q >= xn) break;
                    const double t = wx[q] * lds[o + q];
                    a = q == 0 ? t : a + t;
                }
            }
            lds[X0L + ry * PA_TXC + cx] = a;
        }
        __syncthreads(); // the x-pass plane is complete; the next v plane is in the ring
        // y-pass
        double a = 0.0;
        if (xin && yin) {
#pragma unroll
            for (int q = 0; q < 4; q++) {
                if (q >= yn) break;
                const double t = wy[q] * lds[X0L + (ylo + q) * PA_TXC + cx];
                a = q == 0 ? t : a + t;
            }
        }
        p0 = p1;
        p1 = p2;
        p2 = p3;
        p3 = a;
        if (fz == zend) { // (block-uniform) the last fine plane of coarse plane Z's window
            const int zn = T.rcnt[2][Z];
            const double w0 = T.rw[2][4 * Z], w1 = T.rw[2][4 * Z + 1], w2 = T.rw[2][4 * Z + 2], w3 = T.rw[2][4 * Z + 3];
            double out;
            if (zn >= 4) out = ((w0 * p0 + w1 * p1) + w2 * p2) + w3 * p3;
            else if (zn == 3) out = (w0 * p1 + w1 * p2) + w2 * p3;
            else if (zn == 2) out = w0 * p2 + w1 * p3;
            else out = w0 * p3;
            if (xin && yin) cf[X + Y * cldy + (int64_t)Z * cldz] = out;
            Z++;
            zend = Z <= Ze ? T.rlo[2][Z] + T.rcnt[2][Z] - 1 : -1;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Full multigrid's prolongation by position (gs_fmg_prolong_pa): gs_device.hpp's k_fmg_prolong with the window start
// cj and the four Lagrange weights of every fine index read from tables instead of following from 2i / 2i + 1.
// One block: a fine tile of 2 FQ_TX x-points (a wave: the lane's points x, x + 1, x odd, as one 16-byte store) by
// 2 FQ_TY rows (two per wave), marching a chunk of fine planes. Per coarse plane the block stages the columns
// cj_x[first] .. cj_x[last] + K - 1 and rows cj_y[first] .. cj_y[last] + K - 1 of its tile in LDS (three buffers, one
// barrier per plane; plane p + 1, loaded a step earlier, is written at the top of step p, then plane p + 2's loads
// are issued into the same registers); each thread forms the x- and then y-interpolated values of its 2 x 2 fine
// columns on that plane; the z pass runs on a register window of the last four such planes. cj_z is non-decreasing in
// the fine plane and moves by 0 or 1, so after coarse plane p the fine planes with cj_z + K - 1 = p are complete, in
// order.
//  - 128 consecutive fine indices span at most 64 + K coarse ones, 8 at most 4 + K (pj advances by (m + 1) / (n + 1)
//    per index: at most 130 / 258 where a tile is full in x, at most 5 / 9 where it is full in y): FQ_LW, FQ_LR.
//  - A lane's 2 x 4 x-weights and the wave's 2 x 4 y-weights are loop invariants; the z-weights are wave-uniform,
//    read when the plane before theirs has been emitted (the window start one plane further ahead).
//  - K = 3 (one coarse point on the axis): the fourth operand is neither used nor, in global memory, read.
//  - Every table value is clamped to the staged tile and the padded coarse array, so tables that do not belong to
//    the levels cannot take an access out of either field.
constexpr int FQ_TX = 64, FQ_TY = 4, FQ_T = FQ_TX * FQ_TY;
constexpr int FQ_LW = FQ_TX + 4, FQ_LR = 2 * FQ_TY; // staged columns, rows
constexpr int FQ_NE = (FQ_LW * FQ_LR + FQ_T - 1) / FQ_T; // staged elements per thread and plane

struct FqTables {
    const int32_t* cj[3];
    const double* cw[3];
};

__device__ __forceinline__ double fq_sum(bool k3, const double (&w)[4], double c0, double c1, double c2, double c3)
{
    const double s = (w[0] * c0 + w[1] * c1) + w[2] * c2;
    return k3 ? s : s + w[3] * c3;
}

template <bool NT>
__global__ __launch_bounds__(FQ_T, 5) void k_fmg_prolong_pa(FqTables T, const double* __restrict__ c,
                                                         double* __restrict__ f, int cnx, int cny, int cnz, int fnx,
                                                         int fny, int fnz, int64_t cldy, int64_t cldz, int64_t fldy,
                                                         int64_t fldz, int zc, int al)
{
    __shared__ double pl[3][FQ_LR * FQ_LW];
    // (the wave's rows in SGPRs: their windows and weights are then scalar)
    const int lane = threadIdx.x, wv = __builtin_amdgcn_readfirstlane(threadIdx.y), tid = wv * FQ_TX + lane;
    const bool k3x = cnx < 2, k3y = cny < 2, k3z = cnz < 2;
    const int x0 = 1 + blockIdx.x * 2 * FQ_TX, y0 = 1 + blockIdx.y * 2 * FQ_TY, zb = 1 + blockIdx.z * zc;
    const int xe = min(x0 + 2 * FQ_TX - 1, fnx), ye = min(y0 + 2 * FQ_TY - 1, fny), ze = min(zb + zc - 1, fnz);
    // staged columns / rows / planes: what the tile's windows cover, inside the padded coarse array
    const int clo = pa_clamp(T.cj[0][x0], 0, cnx + 1);
    const int ncol = pa_clamp(T.cj[0][xe] + (k3x ? 3 : 4) - clo, 1, min(FQ_LW, cnx + 2 - clo));
    const int rlo = pa_clamp(T.cj[1][y0], 0, cny + 1);
    const int nrow = pa_clamp(T.cj[1][ye] + (k3y ? 3 : 4) - rlo, 1, min(FQ_LR, cny + 2 - rlo));
    const int pstart = pa_clamp(T.cj[2][zb], 0, cnz + 1);
    const int pend = pa_clamp(T.cj[2][ze] + (k3z ? 2 : 3), pstart, cnz + 1);
    // the lane's two x-points and the wave's two rows: window positions in the staged plane, weights
    const int x = x0 + 2 * lane, ya = y0 + 2 * wv;
    const bool okx = x <= fnx, x2 = x + 1 <= fnx, oka = ya <= fny, okb = ya + 1 <= fny;
    const int xa = min(x, fnx), xb = min(x + 1, fnx), yA = min(ya, fny), yB = min(ya + 1, fny);
    const int lca = pa_clamp(T.cj[0][xa] - clo, 0, FQ_LW - 4), lcb = pa_clamp(T.cj[0][xb] - clo, 0, FQ_LW - 4);
    const int lra = pa_clamp(T.cj[1][yA] - rlo, 0, FQ_LR - 4);
    const bool dy = T.cj[1][yB] - rlo > lra; // row b's window starts one staged row later
    double wxa[4], wxb[4], wya[4], wyb[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        wxa[k] = T.cw[0][4 * xa + k];
        wxb[k] = T.cw[0][4 * xb + k];
        wya[k] = T.cw[1][4 * yA + k];
        wyb[k] = T.cw[1][4 * yB + k];
    }
    // the staged elements this thread loads per plane (offsets from cb: the launcher keeps FQ_LR * cldy inside an int)
    const int n = nrow * ncol;
    const double* const cb = c + clo + (int64_t)rlo * cldy;
    int goff[FQ_NE], loff[FQ_NE];
    bool gok[FQ_NE];
#pragma unroll
    for (int m = 0; m < FQ_NE; m++) {
        const int e = tid + m * FQ_T;
        gok[m] = e < n;
        const int r = gok[m] ? e / ncol : 0, col = gok[m] ? e - r * ncol : 0;
        goff[m] = col + r * (int)cldy;
        loff[m] = r * FQ_LW + col;
    }
    // plane pstart goes to LDS now; g: the thread's elements of the plane after the one being computed, loaded a step
    // earlier and written to the third buffer at the top of the step
    double g[FQ_NE];
#pragma unroll
    for (int m = 0; m < FQ_NE; m++) g[m] = gok[m] ? cb[goff[m] + (int64_t)pstart * cldz] : 0.0;
#pragma unroll
    for (int m = 0; m < FQ_NE; m++)
        if (gok[m]) pl[0][loff[m]] = g[m];
#pragma unroll
    for (int m = 0; m < FQ_NE; m++) g[m] = gok[m] && pstart < pend ? cb[goff[m] + (int64_t)(pstart + 1) * cldz] : 0.0;
    __syncthreads();

    // the z tables of the fine plane to emit next: window start (and that of the plane after it), weights
    auto zidx = [&](int z) { return min(z, fnz + 1); };
    int z = zb, cjc = T.cj[2][zidx(zb)], cjn = T.cj[2][zidx(zb + 1)];
    double wz[4];
#pragma unroll
    for (int k = 0; k < 4; k++) wz[k] = T.cw[2][4 * zidx(zb) + k];

    // [plane of the window][row a: x, x + 1; row b: x, x + 1]
    double W[4][4];
#pragma unroll
    for (int m = 0; m < 4; m++)
#pragma unroll
        for (int q = 0; q < 4; q++) W[m][q] = 0.0;
    double* const frow = f + x + (int64_t)ya * fldy;
    auto store = [&](double* p, double a, double b) {
        if (x2) {
            if (al) st2s<NT>(p, a, b);
            else {
                p[0] = a;
                p[1] = b;
            }
        } else {
            p[0] = a;
        }
    };

    int cur = 0;
    for (int p = pstart; p <= pend; p++) {
        // plane p + 1 into the buffer last read two steps ago; plane p + 2's loads are in flight during this step
        const int nxt = cur == 2 ? 0 : cur + 1;
        if (p < pend) {
#pragma unroll
            for (int m = 0; m < FQ_NE; m++)
                if (gok[m]) pl[nxt][loff[m]] = g[m];
        }
#pragma unroll
        for (int m = 0; m < FQ_NE; m++) g[m] = gok[m] && p + 2 <= pend ? cb[goff[m] + (int64_t)(p + 2) * cldz] : 0.0;
#pragma unroll
        for (int m = 0; m < 3; m++)
#pragma unroll
            for (int q = 0; q < 4; q++) W[m][q] = W[m + 1][q];
        // x pass on the five staged rows the two windows cover (the fifth only where they differ); every row's values go
        // straight into the y sums, which take their terms in window order: row a's term m, row b's term m - dy
#pragma unroll
        for (int m = 0; m < 5; m++) {
            if (m == 4 && (!dy || k3y)) continue;
            const double* row = pl[cur] + min(lra + m, FQ_LR - 1) * FQ_LW;
            const double va = fq_sum(k3x, wxa, row[lca], row[lca + 1], row[lca + 2], row[lca + 3]);
            const double vb = fq_sum(k3x, wxb, row[lcb], row[lcb + 1], row[lcb + 2], row[lcb + 3]);
            if (m == 0) {
                W[3][0] = wya[0] * va;
                W[3][1] = wya[0] * vb;
            } else if (m < 3 || (m == 3 && !k3y)) {
                W[3][0] = W[3][0] + wya[m] * va;
                W[3][1] = W[3][1] + wya[m] * vb;
            }
            if (m == 0) {
                if (!dy) {
                    W[3][2] = wyb[0] * va;
                    W[3][3] = wyb[0] * vb;
                }
            } else {
                const int t = dy ? m - 1 : m; // (wave-uniform)
                const double w = dy ? wyb[m - 1] : wyb[m < 4 ? m : 3];
                if (t == 0) {
                    W[3][2] = w * va;
                    W[3][3] = w * vb;
                } else if (t < 3 || (t == 3 && !k3y)) {
                    W[3][2] = W[3][2] + w * va;
                    W[3][3] = W[3][3] + w * vb;
                }
            }
        }
        // the fine planes complete with coarse plane p (W[m] holds plane p - 3 + m)
        while (z <= ze && cjc + (k3z ? 2 : 3) == p) {
            if (okx && oka) {
                double o[4];
#pragma unroll
                for (int q = 0; q < 4; q++)
                    o[q] = k3z ? (wz[0] * W[1][q] + wz[1] * W[2][q]) + wz[2] * W[3][q]
                               : ((wz[0] * W[0][q] + wz[1] * W[1][q]) + wz[2] * W[2][q]) + wz[3] * W[3][q];
                double* const q0 = frow + (int64_t)z * fldz;
                store(q0, o[0], o[1]);
                if (okb) store(q0 + fldy, o[2], o[3]);
            }
            z++;
            cjc = cjn;
            cjn = T.cj[2][zidx(z + 1)];
#pragma unroll
            for (int k = 0; k < 4; k++) wz[k] = T.cw[2][4 * zidx(z) + k];
        }
        __syncthreads();
        cur = nxt;
    }
}

} // namespace
