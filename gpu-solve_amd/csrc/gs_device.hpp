// gs_device.hpp — the CDNA4 (gfx950) device code of the GMG V-cycle and its launch plans: point
// formulas, the stencil / restriction / prolongation / coarse-cycle kernels and the host-side planning
// helpers. Included by gs_kernels.hip (the product library, include/gpusolve_hip.h) and by gs_diag.hip
// (libgpusolve_diag.so: tuning variants, bandwidth probes and the measured-and-rejected k_prr, which only
// tools/, tests/ and bench.py's measured-ceiling leg load; include/gpusolve_diag.h). Internal linkage.
//
// Numerics follow the reference CPU backend operator by operator (src/cpu/CpuSolver.cpp,
// src/cpu/NewtonSolver.cpp, src/cpu/CpuGridData.cpp of Bricktricker/gpu-solve): every expression
// keeps the reference's evaluation order and the libraries are built with -ffp-contract=off, so in
// LINEAR mode every field is bit-identical to the CPU path; only the l2-norm summation order
// (deterministic here: fixed per-block partials + fixed-order finish) and, in the non-linear
// modes, ocml's exp vs glibc's exp (<= 1 ulp) differ.
//
// Layout: x unit-stride, z slowest (include/gpusolve_hip.h), so Z-slabs are contiguous planes and
// a wave64 row load along x is one coalesced 1 KiB (dwordx4 per lane) access.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include <cmath>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <cxxabi.h>
#include <map>
#include <mutex>
#include <string>
#include <type_traits>
#include <utility>

#include "gpusolve_hip.h"

// Timing-only experiment builds (tools/exp_builds.sh; never the product, results are wrong):
//   GS_EXP_NOBAR  the pair's and k_rr2's per-plane LDS barriers removed (what the lock-step costs)
//   GS_EXP_NOEXP  exp(x) replaced by one multiplication (what the exponentials cost)
//   GS_EXP_NODIV  NEWTON's r / den replaced by a multiplication (what the divisions cost)
//   GS_EXP_EFIELD k_tb2y's NEWTON sweep-1 rows load E = exp(w) from a second field instead of evaluating it
//                 (the field lies gs_exp_set_efoff(n) elements past newtonV; tools/newton_kprobe.py sets it)
//   GS_EXP_T3_FLIGHT k_tb3y's sweep 1 takes its z+ operand, row -2 and f from planes already in registers, so no stage
//                 waits on the newest loads (bounds what more flight time for the loads can buy)
//   GS_EXP_T3_SYM    k_tb3y's whole-wave-rows instance keeps the symmetric step (both y-waves in phase: what the
//                    stagger of waves 4-7 is worth)
//   GS_EXP_T3_CHAIN  k_tb3y's sweeps 2 and 3 take their z+ operand from the previous step's plane instead of the stage
//                 before them (bounds what breaking the stage-to-stage chain can buy)
// Alternative-arithmetic builds (A/B only; correct results, not the product's choice):
//   GS_EXP_NB_IEEE   GS_NEWTON_B's Jacobi quotient as the IEEE division instead of nb_quot (r05p)
#ifdef GS_EXP_NOEXP
#define exp(x) ((x) * 1.0000001)
#endif
#ifdef GS_EXP_NOBAR
#define GS_LDS_BARRIER() __builtin_amdgcn_s_waitcnt(0xc07f)
#else
#define GS_LDS_BARRIER()                                                                                               \
    do {                                                                                                               \
        __builtin_amdgcn_s_waitcnt(0xc07f);                                                                            \
        __builtin_amdgcn_s_barrier();                                                                                  \
    } while (0)
#endif

namespace {

constexpr int WAVE = 64;

// NEWTON's two forms (include/gpusolve_hip.h): GS_NEWTON reads newtonV as w, GS_NEWTON_B reads the precomputed
// linearisation factor B = gamma (1 + newtonV) exp(newtonV) (gs_newton_bfac) as w. Both carry a w operand.
constexpr bool newtonish(int m) { return m == GS_NEWTON || m == GS_NEWTON_B; }
// GS_NEWTON_G (the first Newton iteration: B = gamma everywhere) launches the GS_NEWTON_B kernels with Coef::bconst
constexpr int base_mode(int m) { return m == GS_NEWTON_G ? GS_NEWTON_B : m; }

// compile-time / run-time booleans for code specialised per wave (BoolC) or selected per use (RtBool)
template <bool B>
struct BoolC {
    __device__ static constexpr bool get() { return B; }
};
struct RtBool {
    bool b;
    __device__ bool get() const { return b; }
};

// ---------------------------------------------------------------------------------------------
// Stencil coefficients by value (they land in SGPRs).
struct Coef {
    double s[7];
    double hh;     // h*h
    double omega[3]; // relaxation weight of each fused stage (sweep) of a pass; equal unless weights were given
    double gamma;
    double alpha;  // h*h / s0          (CpuSolver.cpp:145)
    double preFac; // s0 / (h*h)        (CpuSolver.cpp:144)
    int fastdiv;   // 2^-120 <= hh <= 1: div_hh may take its 3-operation path
    int unit;      // s[1..6] == -1 and |s[0]| >= 1: the unit-neighbour stencil sum applies (stencil_sum<true>)
    int swz;       // column-block pairs: x-waves of the mirrored row rotated by two (GS_XH_SWIZZLE)
    int zq;        // every s[i] finite and hh a positive normal number: the stencil sum of an identically zero
                   // iterate over hh is exactly +0 (each s[i] * 0 is a signed zero, +0 plus a signed zero is
                   // +0, +0 / hh is +0), so zero-iterate sweeps take q = +0 without evaluating it
    int bconst;     // GS_NEWTON_B with B = gamma at every point (the first Newton iteration's factor): the pair and
                    // k_rr2 take k.gamma instead of loading w (which still holds gamma for every other kernel)
    int64_t off[7]; // generic kernel: linear element offsets of the 7 entries
#ifdef GS_EXP_EFIELD
    int64_t efoff;
#endif
};

bool canonical_order(const gs_stencil* S)
{
    static const int cx[7] = {0, 1, -1, 0, 0, 0, 0};
    static const int cy[7] = {0, 0, 0, 1, -1, 0, 0};
    static const int cz[7] = {0, 0, 0, 0, 0, 1, -1};
    for (int i = 0; i < 7; i++)
        if (S->ox[i] != cx[i] || S->oy[i] != cy[i] || S->oz[i] != cz[i]) return false;
    return true;
}

bool valid_stencil(const gs_stencil* S)
{
    for (int i = 0; i < 7; i++)
        if (S->ox[i] < -1 || S->ox[i] > 1 || S->oy[i] < -1 || S->oy[i] > 1 || S->oz[i] < -1 || S->oz[i] > 1)
            return false;
    return true;
}

// A/B switches of the launch plans, read ONCE when the library is loaded (a namespace-scope object,
// initialised at load time: no getenv is reachable from a launch). Defaults are the measured choices
// (DESIGN.md §9); the switches serve tools/ A/B runs and the tests that pin every alternative path:
//   GS_NO_UNIT_STENCIL   the general 14-operation stencil sum instead of the unit-neighbour form
//   GS_FIT_ROUNDS=0      no round-fitted chunk lengths for the zero-iterate pairs
//   GS_SLAB_ZC=n         z-chunk (planes; even, >= 2) of pair launches past a slab's first plane
//   GS_PAIR_ZC=n         z-chunk of pair launches from a level's first plane (>= 2^26 points)
//   GS_PAIR_MIN_BLOCKS=n blocks of 4-plane chunks from which a level smooths in pairs (default 128)
//   GS_PAIR_BIG_CHUNKS=0 64-plane chunks on >= 2^26-point levels
//   GS_PAIR_ONE_ROUND=0  no one-round / four-round chunking on >= 2^26-point levels
//   GS_RR_LDS            residual + restriction through the LDS kernel (k_resrestrict) only
//   GS_RR_NR=1|2         coarse rows per k_rr2 block (default: 2 on LINEAR levels of >= 2^26 points)
//   GS_RR_REVERSE=0|1    k_rr2 z-chunks in ascending (0) or descending (1, default: r04e, -1% on 512^3) order
//   GS_NO_ZERO_Q         zero-iterate sweeps evaluate the stencil of their zeros instead of taking q = +0
//   GS_XH_SWIZZLE=0|1    column-block pairs: the mirrored row's x-waves rotated by two (1, default) or not (0)
//   GS_MID_ZC=n          z-chunk of pair launches over whole levels of < 2^26 points (A/B)
//   GS_RR_ZC=n           z-chunk (coarse planes) of k_rr2 launches from fine levels of < 2^26 points (A/B)
//   GS_RR_ZC_BIG=n       the same for fine levels of >= 2^26 points (A/B)
//   GS_RB_ZC=n           z-chunk of the one-point passes (k_rb sweeps / residuals, the Newton update pass) (A/B)
//   GS_PAIR_FX=0         LINEAR plain pairs always through the instance with per-lane range selects (A/B, r06)
//   GS_FMG_NT=0|1        gs_fmg_prolong's fine stores never / always non-temporal (default: from 2^25 fine points) (A/B)
//   GS_T3_SADDR=0        the fused triple's unit-stencil instances with per-lane 64-bit addresses (A/B)
struct Knobs {
    bool unitStencil, fitRounds, bigChunks, oneRound, rrLds, zeroQ;
    int xhSwizzle, midZc, rrZc, rrZcBig, rbZc;
    int slabZc, pairZc, rrNr, rrReverse;
    bool pairFx, t3Saddr;
    int fmgNt;
    int64_t pairMinBlocks;
    static int num(const char* name, int dflt)
    {
        const char* e = getenv(name);
        return e && *e ? atoi(e) : dflt;
    }
    Knobs()
        : unitStencil(getenv("GS_NO_UNIT_STENCIL") == nullptr), fitRounds(num("GS_FIT_ROUNDS", 1) != 0),
          bigChunks(num("GS_PAIR_BIG_CHUNKS", 1) != 0), oneRound(num("GS_PAIR_ONE_ROUND", 1) != 0),
          rrLds(getenv("GS_RR_LDS") != nullptr), zeroQ(getenv("GS_NO_ZERO_Q") == nullptr),
          xhSwizzle(num("GS_XH_SWIZZLE", 1)), midZc(num("GS_MID_ZC", 0)), rrZc(num("GS_RR_ZC", 0)),
          rrZcBig(num("GS_RR_ZC_BIG", 0)), rbZc(num("GS_RB_ZC", 0)), slabZc(num("GS_SLAB_ZC", 0)),
          pairZc(num("GS_PAIR_ZC", 0)), rrNr(num("GS_RR_NR", 0)), rrReverse(num("GS_RR_REVERSE", 1)),
          pairFx(num("GS_PAIR_FX", 1) != 0), t3Saddr(num("GS_T3_SADDR", 1) != 0), fmgNt(num("GS_FMG_NT", -1)),
          pairMinBlocks(num("GS_PAIR_MIN_BLOCKS", 128))
    {
    }
};
const Knobs kKnobs;

#ifdef GS_EXP_EFIELD
int64_t gs_exp_efoff = 0; // set by gs_exp_set_efoff (gs_kernels.hip, this build only)
#endif

Coef make_coef(const gs_stencil* S, const gs_level* L, double omega, double gamma, int bconst = 0)
{
    Coef k;
    for (int i = 0; i < 7; i++) {
        k.s[i] = S->s[i];
        k.off[i] = S->ox[i] + S->oy[i] * L->ldy + S->oz[i] * L->ldz;
    }
    k.hh = L->h * L->h;
    for (int i = 0; i < 3; i++) k.omega[i] = omega;
    k.gamma = gamma;
    k.alpha = k.hh / S->s[0];
    k.preFac = S->s[0] / k.hh;
    k.fastdiv = k.hh >= 0x1p-120 && k.hh <= 1.0;
    k.unit = kKnobs.unitStencil && (S->s[0] >= 1.0 || S->s[0] <= -1.0);
    for (int i = 1; i < 7; i++) k.unit = k.unit && S->s[i] == -1.0;
    k.swz = kKnobs.xhSwizzle;
    k.zq = kKnobs.zeroQ && std::isnormal(k.hh) && k.hh > 0.0;
    for (int i = 0; i < 7; i++) k.zq = k.zq && std::isfinite(S->s[i]);
    k.bconst = bconst;
#ifdef GS_EXP_EFIELD
    k.efoff = gs_exp_efoff;
#endif
    return k;
}

// the same with one relaxation weight per fused stage (n <= 3 of them; the remaining stages repeat the last)
Coef make_coef_w(const gs_stencil* S, const gs_level* L, const double* omegas, int n, double gamma, int bconst = 0)
{
    Coef k = make_coef(S, L, omegas[0], gamma, bconst);
    for (int i = 1; i < 3; i++) k.omega[i] = omegas[i < n ? i : n - 1];
    return k;
}

// ---------------------------------------------------------------------------------------------
// Point formulas (reference evaluation order; built with -ffp-contract=off).

// s / hh, bit-identical to the compiler's IEEE division, in 3 FP64 operations instead of ~11.
// The gfx950 division sequence is: D = div_scale(hh), y = rcp(D) refined by two Newton steps,
// N = div_scale(s), q = N*y, r = fma(-D, q, N), q' = div_fmas(r, y, q), div_fixup(q', hh, s). When
// neither operand is scaled (s and hh normal, s != 0, exponent(s) - exponent(hh) < 768, the quotient
// normal and exponent(s) > 53) div_scale returns its operand, div_fmas is a plain fma and div_fixup
// returns q' — and y depends on hh alone, so it is loop-invariant. The fast path is taken for
// 2^-899 <= |s| < 2^601 with the host guaranteeing 2^-120 <= hh <= 1 (Coef::fastdiv); anything
// else (zero, denormals, inf/nan, extreme magnitudes) takes the ordinary division.
__device__ __forceinline__ double hh_recip(double hh)
{
    const double y0 = __builtin_amdgcn_rcp(hh);
    const double y1 = __builtin_fma(y0, __builtin_fma(-hh, y0, 1.0), y0);
    return __builtin_fma(y1, __builtin_fma(-hh, y1, 1.0), y1);
}

__device__ __forceinline__ double div_hh(const Coef& k, double s)
{
    const unsigned e = ((unsigned)__double2hiint(s) >> 20) & 0x7ffu; // biased exponent
    if (k.fastdiv && e - 124u < 1500u) {                              // 124 <= e <= 1623
        const double y = hh_recip(k.hh);
        const double q = s * y;
        const double r = __builtin_fma(-k.hh, q, s);
        return __builtin_fma(r, y, q);
    }
    return s / k.hh;
}

// The same division for N values at once: the operand-range test of every value is combined first
// and ONE branch picks the 3-operation path for all N (or the IEEE division for all N when any value
// is outside the range), so a sweep over several rows has one exec branch instead of one per point
// and the scheduler can interleave the rows' arithmetic.
__device__ __forceinline__ bool div_hh_fast_ok(double s)
{
    const unsigned e = ((unsigned)__double2hiint(s) >> 20) & 0x7ffu;
    return e - 124u < 1500u;
}
template <int N>
__device__ __forceinline__ void div_hh_n(const Coef& k, double (&s)[N])
{
    bool ok = k.fastdiv;
#pragma unroll
    for (int i = 0; i < N; i++) ok &= div_hh_fast_ok(s[i]);
    if (ok) {
        const double y = hh_recip(k.hh);
#pragma unroll
        for (int i = 0; i < N; i++) {
            const double q = s[i] * y;
            const double r = __builtin_fma(-k.hh, q, s[i]);
            s[i] = __builtin_fma(r, y, q);
        }
    } else {
#pragma unroll
        for (int i = 0; i < N; i++) s[i] = s[i] / k.hh;
    }
}

// div_hh_n with the operand-range test taken on the minimum and the maximum of the N exponent fields (three-input
// integer min / max: about two operations per value instead of four): the same predicate — every exponent in
// 124..1623 — so the same path and the same quotients as div_hh_n
template <int N>
__device__ __forceinline__ void div_hh_mm(const Coef& k, double (&s)[N])
{
    unsigned lo = 0x7ffu, hi = 0u;
#pragma unroll
    for (int i = 0; i < N; i++) {
        const unsigned e = ((unsigned)__double2hiint(s[i]) >> 20) & 0x7ffu;
        lo = min(lo, e);
        hi = max(hi, e);
    }
    if (k.fastdiv && lo >= 124u && hi <= 1623u) {
        const double y = hh_recip(k.hh);
#pragma unroll
        for (int i = 0; i < N; i++) {
            const double q = s[i] * y;
            const double r = __builtin_fma(-k.hh, q, s[i]);
            s[i] = __builtin_fma(r, y, q);
        }
    } else {
#pragma unroll
        for (int i = 0; i < N; i++) s[i] = s[i] / k.hh;
    }
}

// one row's two points: batched, except in GS_NEWTON mode whose kernels run at the VGPR limit (the batch
// keeps both sums live across the branch). GS_NEWTON_B's pairs have the room since r05: batched, NEWTON_B pair
// 0.840-0.853 vs 0.872-0.885 ms, prolongation pair 0.924-0.930 vs 0.964-0.975 ms, Newton iteration -0.8 ms (r05r)
template <int MODE>
__device__ __forceinline__ void div_hh_row(const Coef& k, double (&q)[2])
{
    if (MODE == GS_NEWTON) {
        q[0] = div_hh(k, q[0]);
        q[1] = div_hh(k, q[1]);
    } else {
        div_hh_n(k, q);
    }
}

// stencil sum in config order (before the division by h^2) — CpuSolver.cpp:56-62.
// UN (Coef::unit: the six neighbour weights are exactly -1, |s0| >= 1 — every reference config): the
// same value in 7 instead of 14 operations, bit for bit. s += (-1) * x is s - x exactly (the product
// by -1 is a sign flip, and IEEE subtraction is the addition of the negation), and the first term
// 0.0 + s0 * c equals fma(s0, c, 0.0): both round the product once and add an exact zero, and with
// |s0| >= 1 a non-zero product never underflows to a signed zero (the one case where they differ).
// (A NaN operand's sign is the one thing that differs: s - x negates it, s + (-1) * x does not. Every kernel,
// k_generic included, takes this form for a unit stencil, so they agree with one another on those bits too.)
template <bool UN = false>
__device__ __forceinline__ double stencil_sum(const Coef& k, double c, double xp, double xm, double yp, double ym,
                                              double zp, double zm)
{
    if constexpr (UN) {
        double s = __builtin_fma(k.s[0], c, 0.0);
        s = s - xp;
        s = s - xm;
        s = s - yp;
        s = s - ym;
        s = s - zp;
        s = s - zm;
        return s;
    }
    double s = 0.0;
    s += k.s[0] * c;
    s += k.s[1] * xp;
    s += k.s[2] * xm;
    s += k.s[3] * yp;
    s += k.s[4] * ym;
    s += k.s[5] * zp;
    s += k.s[6] * zm;
    return s;
}

// stencil_sum<false> with each addition's operands held in the source order (sum, product): where both are NaNs the
// hardware returns the first operand's, and the compiler is free to commute an addition, which it does in k_tb3y and
// does not in the one-point kernel; every other value is the same either way. (The unit form needs no such care:
// a - b keeps its operand order.) k_tb3y's general-stencil instance only.
__device__ __forceinline__ double add_in_order(double a, double b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    double r;
    asm("v_add_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
#else
    return a + b;
#endif
}
__device__ __forceinline__ double stencil_sum_in_order(const Coef& k, double c, double xp, double xm, double yp,
                                                       double ym, double zp, double zm)
{
    double s = 0.0;
    s += k.s[0] * c;
    s = add_in_order(s, k.s[1] * xp);
    s = add_in_order(s, k.s[2] * xm);
    s = add_in_order(s, k.s[3] * yp);
    s = add_in_order(s, k.s[4] * ym);
    s = add_in_order(s, k.s[5] * zp);
    s = add_in_order(s, k.s[6] * zm);
    return s;
}

// the non-linear term added after the division — CpuSolver.cpp:63-76
template <int MODE>
__device__ __forceinline__ double op_finish(const Coef& k, double q, double c, double w)
{
    if (MODE == GS_NEWTON) {
        const double ew = exp(w);
        q += k.gamma * (1 + w) * c * ew;
    } else if (MODE == GS_NEWTON_B) {
        q += w * c; // w = B = gamma (1 + newtonV) exp(newtonV)
    } else if (MODE == GS_NONLINEAR) {
        const double ev = exp(c);
        const double nl = k.gamma * c * ev;
        q += nl;
    }
    return q;
}

// stencil sum in config order, then /h^2 and the non-linear term  — CpuSolver.cpp:56-76
template <int MODE, bool UN = false>
__device__ __forceinline__ double op_value(const Coef& k, double c, double xp, double xm, double yp, double ym,
                                           double zp, double zm, double w)
{
    double s = stencil_sum<UN>(k, c, xp, xm, yp, ym, zp, zm);
    s = div_hh(k, s);
    return op_finish<MODE>(k, s, c, w);
}

// GS_NEWTON_B's Jacobi quotient r / den (den = preFac + B, the reference's denominator bit for bit): r times den's
// reciprocal refined by two Newton steps (the reciprocal the IEEE division sequence forms, see div_hh), without the
// division's final correction, scaling and fix-up: 7 FP64 operations instead of ~11, branch-free, and within 1 ulp
// of r / den (tests/test_gpu_newton_b.py::test_nb_quotient_ulps: 26 % of the quotients differ, by one ulp). NEWTON's
// parity is a tolerance — 1e-6 relative on the residual norms (north_star), 1e-9 / 1e-10 in the tests — and its exp
// already differs by an ulp between ocml and glibc. A denominator above 2^1000 (inf included) is clamped there so the
// reciprocal stays normal: r / inf comes out below |r| 2^-999 instead of 0; NaN stays NaN, den = 0 gives NaN where the
// IEEE quotient is inf — both non-finite. Per 512^3 launch: pair 0.871-0.873 vs 0.897-0.914 ms, prolongation pair
// 0.960-0.965 vs 0.989-0.997 ms; Newton iteration -0.5 ms (r05p, profiles/r05/r05p_newton_b_quotient_ab.txt; one
// Newton step only: 18 ulp, 1 % faster; a range branch around it: r05o). GS_EXP_NB_IEEE: the IEEE division (A/B).
// The clamp is symmetric (r06): B = gamma (1 + w) e^w is negative for w < -1, so preFac + B can be negative; a
// denominator of magnitude above 2^1000 (-inf included) keeps its sign. Denominators of magnitude 2^-1000 .. 2^1000
// of either sign stay within the 1 ulp (test_nb_quotient_ulps); below that the reciprocal overflows to inf, where the
// IEEE quotient may still be finite (a point whose denominator cancels to ~1e-301 has left the contract anyway).
__device__ __forceinline__ double nb_recip(double den)
{
    const double d = __builtin_fabs(den) > 0x1p1000 ? __builtin_copysign(0x1p1000, den) : den;
    return hh_recip(d);
}
__device__ __forceinline__ double nb_quot(double r, double den)
{
#ifdef GS_EXP_NB_IEEE
    return r / den;
#else
    return r * nb_recip(den);
#endif
}

// Jacobi point update from the old value and its residual — CpuSolver.cpp:157-171
// (om: the relaxation weight of the sweep the point belongs to, a wave-uniform scalar: k.omega[stage])
template <int MODE>
__device__ __forceinline__ double jacobi_update(const Coef& k, double v, double r, double w, double om)
{
    if (MODE == GS_LINEAR) return v + om * (k.alpha * r);
    if (MODE == GS_NEWTON_B) return v + om * nb_quot(r, k.preFac + w); // preFac + B: the reference's den
    const double u = (MODE == GS_NONLINEAR) ? v : w;
    const double eu = exp(u);
    const double den = k.preFac + k.gamma * (1 + u) * eu;
    return v + om * (r / den);
}
template <int MODE>
__device__ __forceinline__ double jacobi_update(const Coef& k, double v, double r, double w)
{
    return jacobi_update<MODE>(k, v, r, w, k.omega[0]);
}

// NEWTON's linearisation terms of a point, A = gamma (1 + w) and E = exp(w), computed ONCE per point
// and pass and shared by the operator and the update of both sweeps of a fused pair: bit-identical to
// op_finish / jacobi_update, whose reference expressions evaluate gamma * (1 + w) first and multiply
// by exp(w) last (CpuSolver.cpp:63-66, :157-171).
__device__ __forceinline__ double newton_op(double q, double c, double A, double E) { return q + A * c * E; }
template <int MODE>
__device__ __forceinline__ double newton_update(const Coef& k, double v, double r, double A, double E, double om)
{
    const double den = k.preFac + A * E;
    if constexpr (MODE == GS_NEWTON_B) return v + om * nb_quot(r, den); // (E = 1: den = preFac + B exactly)
#ifdef GS_EXP_NODIV
    return v + om * (r * den);
#else
    return v + om * (r / den);
#endif
}

// GS_NEWTON_B's linearisation factor of a point, b = gamma (1 + w) exp(w), evaluated as the reference's Jacobi
// denominator evaluates its product, (gamma * (1 + w)) * exp(w) (CpuSolver.cpp:166-172)
__device__ __forceinline__ double bfac_of(double gamma, double w) { return gamma * (1 + w) * exp(w); }

// A and E of a point from its w operand: GS_NEWTON_B's w is B itself, so A = B and E = 1 (A * c * E = B * c and
// preFac + A * E = preFac + B exactly: the products by 1.0 fold away)
template <int MODE>
__device__ __forceinline__ double newton_A(const Coef& k, double w)
{
    return MODE == GS_NEWTON_B ? w : k.gamma * (1 + w);
}
template <int MODE>
__device__ __forceinline__ double newton_E(double w)
{
    return MODE == GS_NEWTON_B ? 1.0 : exp(w);
}

__device__ __forceinline__ double wave_sum(double x)
{
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) x += __shfl_down(x, o, WAVE);
    return x;
}

// Block-wide fixed-order sum of nw <= NWAVES waves (default: all); result valid in thread 0.
template <int NWAVES>
__device__ __forceinline__ double block_sum(double x, double* lds, int nw = NWAVES)
{
    const int tid = threadIdx.x + threadIdx.y * blockDim.x;
    x = wave_sum(x);
    if ((tid & (WAVE - 1)) == 0) lds[tid / WAVE] = x;
    __syncthreads();
    double t = 0.0;
    if (tid == 0) {
#pragma unroll
        for (int i = 0; i < NWAVES; i++)
            if (i < nw) t += lds[i];
    }
    return t;
}

// ---------------------------------------------------------------------------------------------
// Stencil passes come in three kinds:
//   KIND 0: Jacobi sweep         out = v_new (partials: sum r^2 of the input's residual, nullable)
//   KIND 1: residual             out = r (nullable), partials = per-block sum r^2 (nullable)
//   KIND 2: FAS coarse operator  out = A(u) (ADD=false) or out += A(u) (ADD=true)
// ---------------------------------------------------------------------------------------------
// Register-blocked z-march ("rb"): each lane owns 2 consecutive x-points (one dwordx4) of RY
// consecutive y-rows, a wave owns a 128 x RY tile, W waves stack in y, the block walks ZC planes.
//  - y-neighbours come from the lane's own registers (plus 2 halo rows per wave and plane),
//  - x-neighbours from the adjacent lane by a DPP wave shift (wave_shr:1 / wave_shl:1); the two
//    tile-edge values per row are wave-uniform scalar loads,
//  - z-neighbours are the previous / next plane held in registers,
//  - every load of plane z+1 (next-next v rows, halo rows, f, edges) is issued before plane z is
//    computed, so a full plane of HBM traffic is in flight behind the arithmetic.
// Loads use a clamped column min(x, nx+1); a pair load there reads one element past the padded
// row, which the allocation recipe of gs_field_layout (+32 elements) keeps in bounds.
template <bool DPP>
__device__ __forceinline__ double lane_from_left(double src, double edge)
{
    // lane i <- src of lane i-1; lane 0 <- edge
    if (DPP) {
        const long long s = __double_as_longlong(src), e = __double_as_longlong(edge);
        const int lo = __builtin_amdgcn_update_dpp((int)e, (int)s, 0x138, 0xf, 0xf, false);
        const int hi = __builtin_amdgcn_update_dpp((int)(e >> 32), (int)(s >> 32), 0x138, 0xf, 0xf, false);
        return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
    } else {
        const double t = __shfl_up(src, 1, WAVE);
        return (threadIdx.x & (WAVE - 1)) == 0 ? edge : t;
    }
}

template <bool DPP>
__device__ __forceinline__ double lane_from_right(double src, double edge)
{
    // lane i <- src of lane i+1; lane 63 <- edge
    if (DPP) {
        const long long s = __double_as_longlong(src), e = __double_as_longlong(edge);
        const int lo = __builtin_amdgcn_update_dpp((int)e, (int)s, 0x130, 0xf, 0xf, false);
        const int hi = __builtin_amdgcn_update_dpp((int)(e >> 32), (int)(s >> 32), 0x130, 0xf, 0xf, false);
        return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
    } else {
        const double t = __shfl_down(src, 1, WAVE);
        return (threadIdx.x & (WAVE - 1)) == WAVE - 1 ? edge : t;
    }
}

// a value every lane holds identically (an LDS broadcast read), moved to SGPRs
__device__ __forceinline__ double uniform_d(double x)
{
    const long long b = __double_as_longlong(x);
    const int lo = __builtin_amdgcn_readfirstlane((int)b), hi = __builtin_amdgcn_readfirstlane((int)(b >> 32));
    return __longlong_as_double(((long long)(unsigned)hi << 32) | (unsigned)lo);
}

__device__ __forceinline__ double2 ld2(const double* __restrict__ p) { return *reinterpret_cast<const double2*>(p); }

typedef double dv2 __attribute__((ext_vector_type(2)));
// streamed-once operands (f, the output) optionally bypass the caches' retention (nt)
template <bool NT>
__device__ __forceinline__ double2 ld2s(const double* __restrict__ p)
{
    if (NT) {
        const dv2 t = __builtin_nontemporal_load(reinterpret_cast<const dv2*>(p));
        return make_double2(t.x, t.y);
    }
    return ld2(p);
}
template <bool NT>
__device__ __forceinline__ void st2s(double* __restrict__ p, double a, double b)
{
    if (NT) {
        const dv2 t = {a, b};
        __builtin_nontemporal_store(t, reinterpret_cast<dv2*>(p));
    } else {
        *reinterpret_cast<double2*>(p) = make_double2(a, b);
    }
}

// Scalar-base addressing (k_tb3y): a wave-uniform 64-bit byte address held in SGPRs plus one 32-bit lane offset, the
// `global_load_dwordx4 v, v_off, s[base:base+1]` form, so that no lane keeps a 64-bit address. Two things keep the
// compiler from undoing it. (1) The uniform base goes through an empty asm statement with an SGPR constraint: without it
// base + row + lane offset is reassociated, the loop-invariant part (row + lane offset) hoisted into a 64-bit VGPR pair
// per row, and the plane offset added per step with v_lshl_add_u64. The INTEGER is laundered and then cast to a
// global (address_space(1)) pointer: laundering a pointer loses its address space and gives flat_load. (2) The lane
// offset stays a 32-bit value that is redefined in the loop (sa_lane, once per plane step), so its zero-extension is
// formed where the access is selected; hoisted out of the loop it is a 64-bit VGPR again and selection falls back to
// v_lshl_add_u64 plus `off`. Neither statement emits an instruction (not volatile: the scheduler moves them freely).
typedef __attribute__((address_space(1))) const dv2 sa_cdv2;
typedef __attribute__((address_space(1))) dv2 sa_dv2;
typedef __attribute__((address_space(1))) double sa_d;
__device__ __forceinline__ uint64_t sa_base(const double* p)
{
    uint64_t a = reinterpret_cast<uint64_t>(p);
    asm("" : "+s"(a));
    return a;
}
__device__ __forceinline__ unsigned sa_lane(unsigned off)
{
    asm("" : "+v"(off));
    return off;
}
__device__ __forceinline__ double2 sa_ld2(uint64_t base, unsigned off)
{
    const dv2 t = *reinterpret_cast<sa_cdv2*>(base + off);
    return make_double2(t.x, t.y);
}
__device__ __forceinline__ void sa_st2nt(uint64_t base, unsigned off, double a, double b)
{
    const dv2 t = {a, b};
    __builtin_nontemporal_store(t, reinterpret_cast<sa_dv2*>(base + off));
}
__device__ __forceinline__ void sa_st1(uint64_t base, unsigned off, double a) { *reinterpret_cast<sa_d*>(base + off) = a; }

// A copy the register coalescer cannot fold (k_tb3y's staggered instance): the value moves into registers of its own (the
// early-clobber output), so the source's registers stay the source's. Where a load slot's rows are handed over to the
// plane state with plain assignments, the state takes over the slot's registers, the refill lands in others, and the
// loop-carried slot is put back under its header name by copies on the back-edge that wait for the refill.
__device__ __forceinline__ double2 mov_fresh(const double2 a)
{
    double2 r;
    asm("v_mov_b64 %0, %1" : "=&v"(r.x) : "v"(a.x));
    asm("v_mov_b64 %0, %1" : "=&v"(r.y) : "v"(a.y));
    return r;
}

// Loads of the iterate; ZV: the iterate is identically zero (a coarse level's first sweep after
// the reference's v = 0) and is not read at all. Multiplying the literal zeros keeps the arithmetic,
// and so every bit of the result, that of loaded zeros (no fast-math folding).
template <bool ZV, bool NT = false>
__device__ __forceinline__ double2 ldv2(const double* __restrict__ p)
{
    if (ZV) return make_double2(0.0, 0.0);
    return ld2s<NT>(p);
}
template <bool ZV>
__device__ __forceinline__ double ldv1(const double* __restrict__ p)
{
    return ZV ? 0.0 : *p;
}

// Bijective XCD-aware tile order (cdna_hip_programming.md T1): hardware block b runs on XCD b % 8;
// give each XCD a contiguous run of tiles so y-neighbour tiles share an L2 while they run.
__device__ __forceinline__ int64_t xcd_tile(int64_t b, int64_t nb)
{
    const int64_t q = nb / 8, r = nb % 8, x = b % 8, k = b / 8;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + k;
}

template <int MODE, int KIND, bool ADD, int RY, int W, bool DPP, bool NT = false, bool XCD = false, bool NTV = false,
          bool ZV = false, bool UN = false>
__global__ __launch_bounds__(WAVE* W) void k_rb(Coef k, const double* __restrict__ v, const double* __restrict__ f,
                                                 const double* __restrict__ w, double* __restrict__ out,
                                                 double* __restrict__ partials, int nx, int ny, int nz, int64_t ldy,
                                                 int64_t ldz, int ZC)
{
    __shared__ double red[W];
    const int lane = threadIdx.x;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.y);
    int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
    int64_t tile = blockIdx.x + gridDim.x * ((int64_t)blockIdx.y + gridDim.y * (int64_t)blockIdx.z);
    if (XCD) {
        const int nbx = (nx + 2 * WAVE - 1) / (2 * WAVE), nby = (ny + RY * W - 1) / (RY * W);
        tile = xcd_tile(blockIdx.x, gridDim.x);
        bx = (int)(tile % nbx);
        by = (int)((tile / nbx) % nby);
        bz = (int)(tile / ((int64_t)nbx * nby));
    }
    const int x0 = 1 + bx * (2 * WAVE);
    const int x = x0 + 2 * lane;
    const int xl = min(x, nx + 1);
    const int y0 = 1 + (by * W + wv) * RY;
    const int zb = 1 + bz * ZC;
    const int ze = min(zb + ZC - 1, nz);
    const int xle = x0 - 1;
    const int xre = min(x0 + 2 * WAVE, nx + 1);
    const bool okx0 = x <= nx, okx1 = x + 1 <= nx;
    const double* fin = (KIND == 2) ? out : f;

    int64_t roff[RY + 2]; // rows y0-1 .. y0+RY (clamped into the padded range)
#pragma unroll
    for (int r = 0; r < RY + 2; r++) roff[r] = (int64_t)min(y0 - 1 + r, ny + 1) * ldy;

    // Planes z-1 (P) and z (C) of the wave's rows live in registers. Everything of plane z+1 (its
    // halo rows, f, w, tile edges) and the v rows of plane z+2 is loaded into slot ph of a two-slot
    // ring while plane z is computed from the other slot, and only moved out after it was consumed:
    // a load's destination is never copied before its first use, so its wait lands one full plane
    // of arithmetic after the issue (the loop is unrolled by two to make the slot index static).
    double2 P[RY], C[RY], NL[2][RY], FL[2][RY], WL[2][RY], HL[2][2];
    double EL[2][RY], ER[2][RY];
    double sumsq = 0.0;
    // slot s <- plane z1's halo rows, f, w, edges and plane z2's v rows (plane offsets)
    auto load_slot = [&](const int s, const int64_t z1, const int64_t z2) {
#pragma unroll
        for (int r = 0; r < RY; r++) {
            NL[s][r] = ldv2<ZV, NTV>(v + xl + roff[r + 1] + z2);
            if (KIND != 2 || ADD) FL[s][r] = ld2s<NT>(fin + xl + roff[r + 1] + z1);
            if (newtonish(MODE)) WL[s][r] = ld2(w + xl + roff[r + 1] + z1);
            EL[s][r] = ldv1<ZV>(v + xle + roff[r + 1] + z1);
            ER[s][r] = ldv1<ZV>(v + xre + roff[r + 1] + z1);
        }
        HL[s][0] = ldv2<ZV>(v + xl + roff[0] + z1);
        HL[s][1] = ldv2<ZV>(v + xl + roff[RY + 1] + z1);
    };
    if (zb <= ze) {
        const int64_t zo = (int64_t)zb * ldz;
#pragma unroll
        for (int r = 0; r < RY; r++) {
            P[r] = ldv2<ZV>(v + xl + roff[r + 1] + zo - ldz);
            C[r] = ldv2<ZV>(v + xl + roff[r + 1] + zo);
        }
        load_slot(1, zo, zo + ldz);
    }
    // Both halves always run (an odd chunk ends with one step whose results are discarded), and
    // the loads of every step are unconditional (plane indices clamped into the padded range), so
    // the slots keep fixed registers around the loop.
    for (int z0 = zb; z0 <= ze; z0 += 2) {
#pragma unroll
        for (int ph = 0; ph < 2; ph++) {
            const int z = z0 + ph;
            const bool real = z <= ze;
            const int cs = ph ^ 1; // slot holding plane z
            const int64_t zo = (int64_t)z * ldz;
            load_slot(ph, (int64_t)min(z + 1, nz + 1) * ldz, (int64_t)min(z + 2, nz + 1) * ldz);
#pragma unroll
            for (int r = 0; r < RY; r++) {
                const double2 c = C[r], ym = r == 0 ? HL[cs][0] : C[r - 1], yp = r == RY - 1 ? HL[cs][1] : C[r + 1];
                const double2 zm = P[r], zp = NL[cs][r];
                const double xm0 = lane_from_left<DPP>(c.y, EL[cs][r]);
                const double xp1 = lane_from_right<DPP>(c.x, ER[cs][r]);
                const double wx = newtonish(MODE) ? WL[cs][r].x : 0.0;
                const double wy = newtonish(MODE) ? WL[cs][r].y : 0.0;
                // NEWTON sweep: exp(w) once per point, shared by the operator and the update
                constexpr bool NS = newtonish(MODE) && KIND == 0;
                const double Ax = NS ? newton_A<MODE>(k, wx) : 0.0, Ay = NS ? newton_A<MODE>(k, wy) : 0.0;
                const double Ex = NS ? newton_E<MODE>(wx) : 0.0, Ey = NS ? newton_E<MODE>(wy) : 0.0;
                const double a0 = NS ? newton_op(div_hh(k, stencil_sum<UN>(k, c.x, c.y, xm0, yp.x, ym.x, zp.x, zm.x)), c.x, Ax, Ex)
                                     : op_value<MODE, UN>(k, c.x, c.y, xm0, yp.x, ym.x, zp.x, zm.x, wx);
                const double a1 = NS ? newton_op(div_hh(k, stencil_sum<UN>(k, c.y, xp1, c.x, yp.y, ym.y, zp.y, zm.y)), c.y, Ay, Ey)
                                     : op_value<MODE, UN>(k, c.y, xp1, c.x, yp.y, ym.y, zp.y, zm.y, wy);
                double r0 = 0.0, r1 = 0.0; // residual of the input iterate
                if (KIND != 2 || ADD) {
                    r0 = FL[cs][r].x - a0;
                    r1 = FL[cs][r].y - a1;
                }
                double o0, o1;
                if (NS) {
                    o0 = newton_update<MODE>(k, c.x, r0, Ax, Ex, k.omega[0]);
                    o1 = newton_update<MODE>(k, c.y, r1, Ay, Ey, k.omega[0]);
                } else if (KIND == 0) {
                    o0 = jacobi_update<MODE>(k, c.x, r0, wx);
                    o1 = jacobi_update<MODE>(k, c.y, r1, wy);
                } else if (KIND == 1) {
                    o0 = r0;
                    o1 = r1;
                } else {
                    o0 = ADD ? FL[cs][r].x + a0 : a0;
                    o1 = ADD ? FL[cs][r].y + a1 : a1;
                }
                const bool rowok = real && y0 + r <= ny;
                if (KIND != 2 && partials) {
                    if (rowok && okx0) sumsq += r0 * r0;
                    if (rowok && okx1) sumsq += r1 * r1;
                }
                if (rowok && (KIND != 1 || out)) {
                    double* q = out + x + roff[r + 1] + zo;
                    if (okx1) st2s<NT>(q, o0, o1);
                    else if (okx0) *q = o0;
                }
            }
#pragma unroll
            for (int r = 0; r < RY; r++) {
                P[r] = C[r];
                C[r] = NL[cs][r];
            }
        }
    }
    if (KIND != 2 && partials) {
        const double t = block_sum<W>(sumsq, red);
        if (threadIdx.x == 0 && threadIdx.y == 0) partials[tile] = t;
    }
}

// compF right after findError's update (NewtonSolver.cpp:105-107 then :48-81): w' = w + e (newtonV +=
// v, the expression of k_axpy with a = 1) is formed from both operands wherever the stencil reads it and
// stored once for the block's own points, and the NONLINEAR residual f = F - N(w') with its per-block
// sum of squares is written in the same pass: 40 instead of 48 B per point (k_axpy + k_rb KIND 1).
// Same shape, grid, term order and partial-sum order as k_rb<NONLINEAR, 1> under pass_plan, so f, the
// partials and the norm are bit-identical to the two launches; the caller guarantees that wout's
// non-interior cells already hold what k_axpy would leave there (zeros on a whole level).
// RS: findError's restriction of the new newtonV onto level 1 (NewtonSolver.cpp:88-92, CpuSolver.cpp:211-238) in
// the same pass: a wave's two rows are the fine rows 2Y-1, 2Y of coarse row Y (its upper halo row is 2Y+1), a
// lane's pair the fine columns 2X-1, 2X (2X+1 from the next lane), and coarse plane Z is summed at step 2Z+1 from
// the register window of planes 2Z-1 .. 2Z+1 (never from the slot in flight), in the reference's term order:
// bit-identical to gs_restrict of the stored newtonV, whose 1.1 GB re-read at 512^3 it saves. The chunk of
// planes is even; the last chunk runs one step past the level when nz is even (coarse plane nz / 2).
// (three waves per SIMD, as the plain pass has: <= 168 VGPRs for the restriction's rings)
// BF: the next inner solve's GS_NEWTON_B factor of this level in the same pass — bout = bfac_of(w') at the
// block's own points, from the exp(w') of compF's term (evaluated once): that level's gs_newton_bfac pass is not
// needed (the coarse level's factor stays a gs_newton_bfac pass: its exp inside the restriction's register rings
// spilled ~90 B per lane at three waves per SIMD). RS + BF runs at two waves per SIMD (at three it spills 20 B)
template <int RY, int W, bool UN, bool RS = false, bool BF = false>
__global__ __launch_bounds__(WAVE* W, (RS && BF) ? 2 : 3) void k_newton_upd(Coef k, const double* __restrict__ w,
                                                         const double* __restrict__ e, const double* __restrict__ F,
                                                         double* __restrict__ wout, double* __restrict__ fout,
                                                         double* __restrict__ partials, int nx, int ny, int nz,
                                                         int64_t ldy, int64_t ldz, int ZC, double* __restrict__ cw,
                                                         int cnx, int cny, int cnz, int64_t cldy, int64_t cldz,
                                                         double* __restrict__ bout)
{
    static_assert(!RS || RY == 2, "the restriction takes two fine rows per wave");
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
    const int zlast = (RS && ze == nz) ? nz + 1 : ze;
    const int xle = x0 - 1;
    const int xre = min(x0 + 2 * WAVE, nx + 1);
    const bool okx0 = x <= nx, okx1 = x + 1 <= nx;
    int64_t roff[RY + 2];
#pragma unroll
    for (int r = 0; r < RY + 2; r++) roff[r] = (int64_t)min(y0 - 1 + r, ny + 1) * ldy;
    auto lw2 = [&](int64_t o) {
        const double2 a = ld2(w + o), b = ld2(e + o);
        return make_double2(a.x + b.x, a.y + b.y);
    };
    auto lw1 = [&](int64_t o) { return w[o] + e[o]; };
    // the ring of k_rb: plane z+1's halo rows, F, edges and plane z+2's rows in slot ph
    double2 P[RY], C[RY], NL[2][RY], FL[2][RY], HL[2][2];
    double EL[2][RY], ER[2][RY];
    // RS: own rows at plane z-2, the upper halo row at planes z-1 / z-2, and the right-edge column (rows 2Y-1,
    // 2Y, 2Y+1) at planes z-1 / z-2; EH: the halo row's right edge in the slot
    double2 PP[RS ? RY : 1], Hh1, Hh2;
    double EH[2], E1[3], E2[3];
    double sumsq = 0.0;
    auto load_slot = [&](const int s, const int64_t z1, const int64_t z2) {
#pragma unroll
        for (int r = 0; r < RY; r++) {
            NL[s][r] = lw2(xl + roff[r + 1] + z2);
            FL[s][r] = ld2s<true>(F + xl + roff[r + 1] + z1);
            EL[s][r] = lw1(xle + roff[r + 1] + z1);
            ER[s][r] = lw1(xre + roff[r + 1] + z1);
        }
        HL[s][0] = lw2(xl + roff[0] + z1);
        HL[s][1] = lw2(xl + roff[RY + 1] + z1);
        if constexpr (RS) EH[s] = lw1(xre + roff[RY + 1] + z1);
    };
    if (zb <= ze) {
        const int64_t zo = (int64_t)zb * ldz;
#pragma unroll
        for (int r = 0; r < RY; r++) {
            P[r] = lw2(xl + roff[r + 1] + zo - ldz);
            C[r] = lw2(xl + roff[r + 1] + zo);
        }
        if constexpr (RS) {
#pragma unroll
            for (int r = 0; r < RY; r++) {
                PP[r] = lw2(xl + roff[r + 1] + zo - 2 * ldz);
                E1[r] = lw1(xre + roff[r + 1] + zo - ldz);
                E2[r] = lw1(xre + roff[r + 1] + zo - 2 * ldz);
            }
            Hh1 = lw2(xl + roff[RY + 1] + zo - ldz);
            Hh2 = lw2(xl + roff[RY + 1] + zo - 2 * ldz);
            E1[2] = lw1(xre + roff[RY + 1] + zo - ldz);
            E2[2] = lw1(xre + roff[RY + 1] + zo - 2 * ldz);
        }
        load_slot(1, zo, zo + ldz);
    }
    const int X = 1 + (int)blockIdx.x * WAVE + lane, Yc = (y0 + 1) / 2;
    for (int z0 = zb; z0 <= zlast; z0 += 2) {
#pragma unroll
        for (int ph = 0; ph < 2; ph++) {
            const int z = z0 + ph;
            const bool real = z <= ze;
            const int cs = ph ^ 1;
            const int64_t zo = (int64_t)z * ldz;
            load_slot(ph, (int64_t)min(z + 1, nz + 1) * ldz, (int64_t)min(z + 2, nz + 1) * ldz);
#pragma unroll
            for (int r = 0; r < RY; r++) {
                const double2 c = C[r], ym = r == 0 ? HL[cs][0] : C[r - 1], yp = r == RY - 1 ? HL[cs][1] : C[r + 1];
                const double2 zm = P[r], zp = NL[cs][r];
                const double xm0 = lane_from_left<true>(c.y, EL[cs][r]);
                const double xp1 = lane_from_right<true>(c.x, ER[cs][r]);
                // (compF's non-linear term gamma w' exp(w'), NewtonSolver.cpp:63-72, and B share exp(w'))
                double a0 = div_hh(k, stencil_sum<UN>(k, c.x, c.y, xm0, yp.x, ym.x, zp.x, zm.x));
                double a1 = div_hh(k, stencil_sum<UN>(k, c.y, xp1, c.x, yp.y, ym.y, zp.y, zm.y));
                double b0 = 0.0, b1 = 0.0;
                {
                    const double E0 = exp(c.x), E1 = exp(c.y);
                    const double nl0 = k.gamma * c.x * E0, nl1 = k.gamma * c.y * E1;
                    a0 += nl0;
                    a1 += nl1;
                    if constexpr (BF) {
                        b0 = k.gamma * (1 + c.x) * E0;
                        b1 = k.gamma * (1 + c.y) * E1;
                    }
                }
                const double r0 = FL[cs][r].x - a0, r1 = FL[cs][r].y - a1;
                const bool rowok = real && y0 + r <= ny;
                if (rowok && okx0) sumsq += r0 * r0;
                if (rowok && okx1) sumsq += r1 * r1;
                if (rowok) {
                    const int64_t q = x + roff[r + 1] + zo;
                    if (okx1) {
                        st2s<true>(fout + q, r0, r1);
                        st2s<true>(wout + q, c.x, c.y);
                        if constexpr (BF) st2s<true>(bout + q, b0, b1);
                    } else if (okx0) {
                        fout[q] = r0;
                        wout[q] = c.x;
                        if constexpr (BF) bout[q] = b0;
                    }
                }
            }
            if constexpr (RS) {
                // coarse plane Z = (z - 1) / 2 from planes z-2 (PP), z-1 (P), z (C): fine (2X+ii, 2Y+jj, 2Z+kk)
                const int Zc = (z - 1) >> 1;
                const bool odd = z & 1;
                // the fine column 2X+1 of each (row, plane): the next lane's 2X-1, the edge column for lane 63
                const double2 rows[3][3] = {{PP[0], PP[1], Hh2}, {P[0], P[1], Hh1}, {C[0], C[1], HL[cs][1]}};
                const double eg[3][3] = {{E2[0], E2[1], E2[2]}, {E1[0], E1[1], E1[2]}, {ER[cs][0], ER[cs][1], EH[cs]}};
                if (odd && Zc >= 1 && Zc <= cnz) { // (wave-uniform; the DPP shifts need every lane)
                    double acc = 0.0;
#pragma unroll
                    for (int ii = -1; ii <= 1; ii++)
#pragma unroll
                        for (int jj = -1; jj <= 1; jj++)
#pragma unroll
                            for (int kk = -1; kk <= 1; kk++) {
                                const double fac = 0.125 * ((2.0 - (ii < 0 ? -ii : ii)) / 2.0) *
                                                   ((2.0 - (jj < 0 ? -jj : jj)) / 2.0) *
                                                   ((2.0 - (kk < 0 ? -kk : kk)) / 2.0);
                                const double2 v2 = rows[kk + 1][jj + 1];
                                const double t = ii < 0 ? v2.x
                                                        : (ii == 0 ? v2.y
                                                                   : lane_from_right<true>(v2.x, eg[kk + 1][jj + 1]));
                                acc += fac * t;
                            }
                    if (X <= cnx && Yc <= cny) cw[X + (int64_t)Yc * cldy + (int64_t)Zc * cldz] = acc;
                }
                Hh2 = Hh1;
                Hh1 = HL[cs][1];
#pragma unroll
                for (int i = 0; i < 3; i++) E2[i] = E1[i];
                E1[0] = ER[cs][0];
                E1[1] = ER[cs][1];
                E1[2] = EH[cs];
#pragma unroll
                for (int r = 0; r < RY; r++) PP[r] = P[r];
            }
#pragma unroll
            for (int r = 0; r < RY; r++) {
                P[r] = C[r];
                C[r] = NL[cs][r];
            }
        }
    }
    if (partials) {
        const double t = block_sum<W>(sumsq, red);
        if (threadIdx.x == 0 && threadIdx.y == 0) partials[tile] = t;
    }
}

dim3 rb_grid(const gs_level* L, int RY, int W, int ZC, bool oneD = false)
{
    const dim3 g((unsigned)((L->nx + 2 * WAVE - 1) / (2 * WAVE)), (unsigned)((L->ny + RY * W - 1) / (RY * W)),
                 (unsigned)((L->nz + ZC - 1) / ZC));
    return oneD ? dim3(g.x * g.y * g.z) : g;
}

// ---------------------------------------------------------------------------------------------
// Generic-stencil pass (any 7 offsets in {-1,0,1}^3, any order): one point per thread.
constexpr int GN_BX = 64, GN_BY = 4;

template <int MODE, int KIND, bool ADD>
__global__ __launch_bounds__(256) void k_generic(Coef k, const double* __restrict__ v, const double* __restrict__ f,
                                                 const double* __restrict__ w, double* __restrict__ out,
                                                 double* __restrict__ partials, int nx, int ny, int nz, int64_t ldy,
                                                 int64_t ldz)
{
    __shared__ double red[GN_BY];
    const int x = 1 + blockIdx.x * GN_BX + threadIdx.x;
    const int y = 1 + blockIdx.y * GN_BY + threadIdx.y;
    const int z = 1 + blockIdx.z;
    double sumsq = 0.0;
    if (x <= nx && y <= ny) {
        const int64_t p = x + y * ldy + (int64_t)z * ldz;
        double s = 0.0;
        if (k.unit) {
            // stencil_sum<true>'s form, term by term in the stencil's order: the same value bit for bit (see there), and
            // the NaN bits too are then those of the unit-stencil kernels of the large levels, the pairs and the
            // triples: s - x negates a NaN operand's sign, s + (-1) * x does not
            s = __builtin_fma(k.s[0], v ? v[p + k.off[0]] : 0.0, 0.0);
#pragma unroll
            for (int i = 1; i < 7; i++) s = s - (v ? v[p + k.off[i]] : 0.0);
        } else {
#pragma unroll
            for (int i = 0; i < 7; i++) s += k.s[i] * (v ? v[p + k.off[i]] : 0.0);
        }
        s = div_hh(k, s);
        const double c = v ? v[p] : 0.0;
        const double wv = newtonish(MODE) ? w[p] : 0.0;
        s = op_finish<MODE>(k, s, c, wv);
        if (KIND == 0) {
            const double r = f[p] - s;
            sumsq = r * r;
            out[p] = jacobi_update<MODE>(k, c, r, wv, k.omega[0]);
        } else if (KIND == 1) {
            const double r = f[p] - s;
            sumsq = r * r;
            if (out) out[p] = r;
        } else {
            out[p] = ADD ? out[p] + s : s;
        }
    }
    if (KIND != 2 && partials) {
        const double t = block_sum<GN_BY>(sumsq, red);
        if (threadIdx.x == 0 && threadIdx.y == 0)
            partials[blockIdx.x + gridDim.x * ((int64_t)blockIdx.y + gridDim.y * (int64_t)blockIdx.z)] = t;
    }
}

dim3 gn_grid(const gs_level* L)
{
    return dim3((unsigned)((L->nx + GN_BX - 1) / GN_BX), (unsigned)((L->ny + GN_BY - 1) / GN_BY), (unsigned)L->nz);
}

// ---------------------------------------------------------------------------------------------
// Deterministic finish of the per-block partial sums: one block, fixed strided order.
constexpr int FIN_T = 1024;
__global__ __launch_bounds__(FIN_T) void k_sumsq_finish(const double* __restrict__ partials, int64_t n,
                                                        double* __restrict__ out, int accumulate)
{
    __shared__ double red[FIN_T / WAVE];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += FIN_T) s += partials[i];
    const double t = block_sum<FIN_T / WAVE>(s, red);
    if (threadIdx.x == 0) *out = accumulate ? t : sqrt(t);
}

// ---------------------------------------------------------------------------------------------
// 27-point full weighting (CpuSolver.cpp:211-238): coarse interior point per thread, terms summed
// with ii outermost, kk innermost. The weights are exact powers of two.
// Z-slabs: coarse local plane z is global z + cz0, its centre fine plane global 2(z + cz0), local
// 2(z + cz0) - fz0 (both z0 = 0 on an unpartitioned level).
__global__ __launch_bounds__(256) void k_restrict(const double* __restrict__ fine, double* __restrict__ ca,
                                                  double* __restrict__ cb, int cnx, int cny, int cnz, int64_t fldy,
                                                  int64_t fldz, int64_t cldy, int64_t cldz, int zoff)
{
    const int x = 1 + blockIdx.x * 64 + threadIdx.x;
    const int y = 1 + blockIdx.y * 4 + threadIdx.y;
    const int z = 1 + blockIdx.z;
    if (x > cnx || y > cny) return;
    const double* c0 = fine + 2 * x + (int64_t)(2 * y) * fldy + (int64_t)(2 * z + zoff) * fldz;
    double acc = 0.0;
#pragma unroll
    for (int a = -1; a <= 1; a++)
#pragma unroll
        for (int b = -1; b <= 1; b++)
#pragma unroll
            for (int c = -1; c <= 1; c++) {
                const double wgt = 0.125 * ((2.0 - (a < 0 ? -a : a)) / 2.0) * ((2.0 - (b < 0 ? -b : b)) / 2.0) *
                                   ((2.0 - (c < 0 ? -c : c)) / 2.0);
                acc += wgt * c0[a + b * fldy + c * fldz];
            }
    const int64_t q = x + y * cldy + (int64_t)z * cldz;
    ca[q] = acc;
    if (cb) cb[q] = acc;
}

// ---------------------------------------------------------------------------------------------
// Residual fused into the full-weighting restriction: coarse f = R(f - A v) without writing the fine
// residual to memory (CpuSolver.cpp:45-83 then :211-238; the reference stores r and re-reads it).
// A block owns RR_TXC x RR_TYC coarse columns and marches a chunk of coarse planes. The fine region
// its 27-point stencils touch is (2 RR_TXC + 1) x (2 RR_TYC + 1) points per plane; the v tile with its
// one-point halo is staged in a 4-plane LDS ring (loaded once, coalesced along x), the residual of
// that region in a 3-plane LDS ring. Per coarse plane Z: the two new v planes and the f values of the
// next plane pair are loaded into registers while the current ones are computed (software pipeline),
// r is evaluated on fine planes 2Z and 2Z+1 (2Z-1 is kept from the previous plane), then every
// thread sums its coarse point's 27 terms in the reference's order. Fine points outside the interior
// hold r = 0, as the reference's never-written boundary does. Each residual is the gs_residual
// expression and each sum the gs_restrict one: bit-identical to the unfused pair.
constexpr int RR_TXC = 64, RR_TYC = 4, RR_T = RR_TXC * RR_TYC;
constexpr int RR_FX = 2 * RR_TXC + 1, RR_FY = 2 * RR_TYC + 1; // residual region per plane
constexpr int RR_VX = RR_FX + 2, RR_VY = RR_FY + 2;           // v tile per plane (one-point halo)
constexpr int RR_NR = (RR_FX * RR_FY + RR_T - 1) / RR_T;      // residual points per thread and plane
constexpr int RR_NV = (RR_VX * RR_VY + RR_T - 1) / RR_T;      // v tile points per thread and plane

struct StencilOffsets {
    int lds[7]; // ox + oy * RR_VX (in-plane LDS offset)
    int oz[7];
};

template <int MODE>
__global__ __launch_bounds__(RR_T) void k_resrestrict(Coef k, StencilOffsets so, const double* __restrict__ v,
                                                      const double* __restrict__ f, const double* __restrict__ w,
                                                      double* __restrict__ ca, double* __restrict__ cb, int fnx,
                                                      int fny, int fnz, int64_t fldy, int64_t fldz, int cnx, int cny,
                                                      int cnz, int64_t cldy, int64_t cldz, int zoff, int ZC)
{
    // one LDS array addressed with integer offsets (pointers into it would become flat accesses):
    // v ring slots 0..3 at s * RR_VP, residual ring slots 0..2 at 4 RR_VP + s * RR_RP
    constexpr int RR_VP = RR_VY * RR_VX, RR_RP = RR_FY * RR_FX;
    __shared__ double lds[4 * RR_VP + 3 * RR_RP];
    const int tid = threadIdx.x;
    // (an XCD-aware tile order, as k_tb2y uses, measured 3% slower here: tools/ab_session.sh)
    const int X0 = 1 + blockIdx.x * RR_TXC, Y0 = 1 + blockIdx.y * RR_TYC;
    const int Zb = 1 + blockIdx.z * ZC, Ze = min(Zb + ZC - 1, cnz);
    if (Zb > Ze) return;
    const int fx0 = 2 * X0 - 1, fy0 = 2 * Y0 - 1; // residual region origin (fine)

    // this thread's v-tile points (clamped into the padded level: clamped copies are never used)
    int64_t voff[RR_NV];
#pragma unroll
    for (int i = 0; i < RR_NV; i++) {
        const int e = min(tid + i * RR_T, RR_VX * RR_VY - 1);
        const int ly = e / RR_VX, lx = e - ly * RR_VX;
        voff[i] = min(fx0 - 1 + lx, fnx + 1) + (int64_t)min(fy0 - 1 + ly, fny + 1) * fldy;
    }
    // this thread's residual points: global offset, LDS position, interior flag
    int64_t roff[RR_NR];
    int rpos[RR_NR];
    bool rin[RR_NR];
#pragma unroll
    for (int i = 0; i < RR_NR; i++) {
        const int e = tid + i * RR_T;
        const int ry = min(e, RR_FX * RR_FY - 1) / RR_FX, rx = min(e, RR_FX * RR_FY - 1) - ry * RR_FX;
        const int x = fx0 + rx, y = fy0 + ry;
        rin[i] = e < RR_FX * RR_FY && x <= fnx && y <= fny;
        roff[i] = min(x, fnx + 1) + (int64_t)min(y, fny + 1) * fldy;
        rpos[i] = (ry + 1) * RR_VX + rx + 1;
    }
    auto zc = [&](int fz) { return (int64_t)min(max(fz, -1), fnz + 2) * fldz; };
    auto load_v = [&](double (&dst)[RR_NV], int fz) {
        const int64_t zo = zc(fz);
#pragma unroll
        for (int i = 0; i < RR_NV; i++) dst[i] = v[voff[i] + zo];
    };
    auto store_v = [&](const double (&src)[RR_NV], int fz) {
        const int d = ((fz + 4) & 3) * RR_VP;
#pragma unroll
        for (int i = 0; i < RR_NV; i++)
            if (tid + i * RR_T < RR_VP) lds[d + tid + i * RR_T] = src[i];
    };
    auto load_fw = [&](double (&F)[RR_NR], double (&W)[RR_NR], int fz) {
        const int64_t zo = zc(fz);
#pragma unroll
        for (int i = 0; i < RR_NR; i++) {
            F[i] = f[roff[i] + zo];
            if (newtonish(MODE)) W[i] = w[roff[i] + zo];
        }
    };
    // r on fine plane fz from the v ring (needs planes fz-1 .. fz+1 staged)
    auto residual_plane = [&](const double (&F)[RR_NR], const double (&W)[RR_NR], int fz) {
        int toff[7]; // LDS offset of each stencil term relative to the point's in-plane position
#pragma unroll
        for (int t = 0; t < 7; t++) toff[t] = ((fz + 4 + so.oz[t]) & 3) * RR_VP + so.lds[t];
        const int coff = ((fz + 4) & 3) * RR_VP;
        const int dst = 4 * RR_VP + ((fz + 3) % 3) * RR_RP;
        const bool zin = fz >= 1 && fz <= fnz;
#pragma unroll
        for (int i = 0; i < RR_NR; i++) {
            if (tid + i * RR_T >= RR_FX * RR_FY) continue;
            double r = 0.0;
            if (zin && rin[i]) {
                double sum = 0.0;
#pragma unroll
                for (int t = 0; t < 7; t++) sum += k.s[t] * lds[rpos[i] + toff[t]];
                const double c = lds[rpos[i] + coff];
                const double q = op_finish<MODE>(k, div_hh(k, sum), c, newtonish(MODE) ? W[i] : 0.0);
                r = F[i] - q;
            }
            lds[dst + tid + i * RR_T] = r;
        }
    };

    double VA[RR_NV], VB[RR_NV], FA[RR_NR], FB[RR_NR], WA[RR_NR], WB[RR_NR];
    // prologue: v planes P-2 .. P (P = 2 Zb + zoff) into the ring, r(P-1)
    const int P0 = 2 * Zb + zoff;
    load_v(VA, P0 - 2);
    load_v(VB, P0 - 1);
    load_fw(FA, WA, P0 - 1);
    store_v(VA, P0 - 2);
    store_v(VB, P0 - 1);
    load_v(VA, P0);
    store_v(VA, P0);
    __syncthreads();
    residual_plane(FA, WA, P0 - 1);
    // staged for the first step: v(P+1), v(P+2), f(P), f(P+1)
    load_v(VA, P0 + 1);
    load_v(VB, P0 + 2);
    load_fw(FA, WA, P0);
    load_fw(FB, WB, P0 + 1);
    __syncthreads(); // v(P+2) goes to the slot of v(P-2), which r(P-1) just read
    const int cx = tid % RR_TXC, cy = tid / RR_TXC;
    const int X = X0 + cx, Y = Y0 + cy;
    for (int Z = Zb; Z <= Ze; Z++) {
        const int P = 2 * Z + zoff;
        store_v(VA, P + 1);
        store_v(VB, P + 2);
        __syncthreads();
        double F0[RR_NR], F1[RR_NR], W0[RR_NR], W1[RR_NR];
#pragma unroll
        for (int i = 0; i < RR_NR; i++) {
            F0[i] = FA[i];
            F1[i] = FB[i];
            W0[i] = WA[i];
            W1[i] = WB[i];
        }
        if (Z < Ze) { // the next step's operands, in flight during this step's arithmetic
            load_v(VA, P + 3);
            load_v(VB, P + 4);
            load_fw(FA, WA, P + 2);
            load_fw(FB, WB, P + 3);
        }
        residual_plane(F0, W0, P);
        residual_plane(F1, W1, P + 1);
        __syncthreads();
        if (X <= cnx && Y <= cny) {
            double acc = 0.0;
#pragma unroll
            for (int a = -1; a <= 1; a++)
#pragma unroll
                for (int b = -1; b <= 1; b++)
#pragma unroll
                    for (int c = -1; c <= 1; c++) {
                        const double wgt = 0.125 * ((2.0 - (a < 0 ? -a : a)) / 2.0) * ((2.0 - (b < 0 ? -b : b)) / 2.0) *
                                           ((2.0 - (c < 0 ? -c : c)) / 2.0);
                        acc += wgt * lds[4 * RR_VP + ((P + c + 3) % 3) * RR_RP + (2 * cy + 1 + b) * RR_FX + 2 * cx + 1 + a];
                    }
            const int64_t q = X + Y * cldy + (int64_t)Z * cldz;
            ca[q] = acc;
            if (cb) cb[q] = acc;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Residual + full weighting in registers ("rr2": canonical stencil order, all three modes, levels
// or Z-slabs (zhi) of rows <= 1024 points). A block is the whole row of coarse columns of ONE
// coarse row Y (WX waves of 64 lanes; lane = coarse column X, its fine pair x = 2X-1, 2X one dwordx4)
// and marches a chunk of coarse planes. Per coarse plane Z it evaluates the residual on fine planes 2Z
// and 2Z+1 (2Z-1 is kept from the previous plane) for the three fine rows 2Y-1 .. 2Y+1 the 27-point sum
// reads (row 2Y+1 is also the next row's first: recomputed there, its loads hit L2) the way k_rb's
// residual pass does: x-neighbours by DPP lane shifts with the wave-edge columns exchanged through LDS
// (zero beyond the level's x-boundaries, which hold v = 0), y-neighbours from the lane's own rows plus
// two halo rows, z-neighbours from the register window. r at the next coarse column's first fine
// column (2X+1) is one more DPP shift (the right wave's lane 0 through LDS). The 27 terms are summed in
// the reference's order (CpuSolver.cpp:225-231): 16 B of compulsory HBM reads per fine point (v, f)
// plus 1 B of coarse writes, the residual never stored, and no LDS staging of the operands (the
// LDS-tiled k_resrestrict, kept for the other cases, is latency-bound at 2 blocks per CU). A step's
// operands are loaded at the top of the step into one slot (154 VGPRs and 3 waves per SIMD: measured
// faster than a two-slot ring that keeps the next plane's loads in flight). Blocks go in
// XCD-aware order, y fastest, so the neighbouring rows that share 3 of a block's 5 v rows run on the
// same XCD at the same time.
constexpr int RR2_WXMAX = 8, RR2_NR2_LOG2_POINTS = 26;

// NR: coarse rows per block (1: fine rows 2Y-1..2Y+1 computed; 2: 2Y-1..2Y+3, the shared row 2Y+1 and three
// of the seven v rows once instead of twice)
template <int MODE, int NR, bool UN>
__global__ __launch_bounds__(WAVE* RR2_WXMAX) void k_rr2(Coef k, const double* __restrict__ v,
                                                         const double* __restrict__ f, const double* __restrict__ w,
                                                         double* __restrict__ ca,
                                                         double* __restrict__ cb, int fnx, int fny, int fnz,
                                                         int64_t fldy, int64_t fldz, int cnx, int cny, int cnz, int64_t cldy,
                                                         int64_t cldz, int ZC, int zhi, int rev)
{
    constexpr int RR = 2 * NR + 1; // computed fine rows; v rows 0 .. RR+1 (0 and RR+1: halo rows)
    // wave-edge columns [parity][1 + wave][side][plane * 3 + row] of v, and r at each wave's first fine
    // column [parity][1 + wave][plane * 3 + row]; slots 0 and WX+1 are the zero x-boundary
    __shared__ double ve[2][RR2_WXMAX + 2][2][2 * RR];
    __shared__ double re[2][RR2_WXMAX + 2][2 * RR];
    const int lane = threadIdx.x;
    const int wx = __builtin_amdgcn_readfirstlane(threadIdx.y);
    const int WX = blockDim.y;
    const int tid = lane + WAVE * wx;
    for (int i = tid; i < 2 * (RR2_WXMAX + 2) * 2 * 2 * RR; i += WAVE * WX) (&ve[0][0][0][0])[i] = 0.0;
    for (int i = tid; i < 2 * (RR2_WXMAX + 2) * 2 * RR; i += WAVE * WX) (&re[0][0][0])[i] = 0.0;
    __syncthreads();
    const int64_t tile = xcd_tile(blockIdx.x + (int64_t)gridDim.x * blockIdx.y, (int64_t)gridDim.x * gridDim.y);
    const int Y = 1 + NR * (int)(tile % gridDim.x);
    // rev (GS_RR_REVERSE): the z-chunks in descending order, so the first blocks read the planes the
    // preceding pair launch touched last
    const int zi = (int)(tile / gridDim.x);
    const int Zb = 1 + (rev ? (int)gridDim.y - 1 - zi : zi) * ZC, Ze = min(Zb + ZC - 1, cnz);
    const int X = 1 + wx * WAVE + lane;
    const int x = 2 * X - 1, xl = min(x, fnx + 1);
    const bool okx0 = x <= fnx, okx1 = x + 1 <= fnx;
    int64_t roff[RR + 2]; // fine rows 2Y-2 .. 2Y+2NR (computed: 1..RR)
    bool rowc[RR + 2];
#pragma unroll
    for (int j = 0; j < RR + 2; j++) {
        const int y = 2 * Y - 2 + j;
        roff[j] = (int64_t)min(max(y, 0), fny + 1) * fldy;
        rowc[j] = y >= 1 && y <= fny;
    }
    // zhi: plane fnz+1 is an internal Z-slab boundary (current ghost planes fnz+1 of v, f, w and
    // fnz+2 of v): the residual there is real, not the zero of a level boundary
    auto at = [&](const double* b, int j, int p) {
        return b + xl + roff[j] + (int64_t)min(max(p, 0), fnz + 1 + zhi) * fldz;
    };
    // one step's operands: v planes 2Z+1 (A), 2Z+2 (B) of rows 1..3; halo rows 0 / 4 of planes 2Z (H0)
    // and 2Z+1 (H1); f of planes 2Z (F0), 2Z+1 (F1) rows 1..3
    double2 VA[RR], VB[RR], H0[2], H1[2], F0[RR], F1[RR], W0[RR], W1[RR];
    auto load_slot = [&](const int Z) {
        const int p = 2 * Z;
        // the step's halo rows first (the rows the y-neighbour blocks read too), then row by row: k_rr2 0.442-0.443 vs
        // 0.458-0.459 ms LINEAR, 0.7085-0.7088 vs 0.7254-0.7259 ms NEWTON_B per 512^3 launch (r06x / r06y,
        // interleaved, profiles/r06/r06x_load_order_ab.txt; f rows first: 0.449 / 0.726-0.740, plane by plane: 0.484-0.485 /
        // 0.754-0.760, v / f / w grouped: 0.481-0.485 / 0.747-0.750, halos then v then f / w: 0.476-0.478 / 0.751)
        H0[0] = ld2(at(v, 0, p));
        H0[1] = ld2(at(v, RR + 1, p));
        H1[0] = ld2(at(v, 0, p + 1));
        H1[1] = ld2(at(v, RR + 1, p + 1));
#pragma unroll
        for (int j = 0; j < RR; j++) {
            // rows no neighbouring block reads (v: 2Y+1 .. 2Y+2NR-3, f: 2Y .. 2Y+2NR-2) are non-temporal loads:
            // they bypass L2 retention, leaving it to the shared halo rows
            const bool uv = j >= 2 && j <= RR - 3, uf = j >= 1 && j <= RR - 2;
            VA[j] = uv ? ld2s<true>(at(v, j + 1, p + 1)) : ld2(at(v, j + 1, p + 1));
            VB[j] = uv ? ld2s<true>(at(v, j + 1, p + 2)) : ld2(at(v, j + 1, p + 2));
            F0[j] = uf ? ld2s<true>(at(f, j + 1, p)) : ld2(at(f, j + 1, p));
            F1[j] = uf ? ld2s<true>(at(f, j + 1, p + 1)) : ld2(at(f, j + 1, p + 1));
            if (MODE == GS_NEWTON_B && k.bconst) {
                W0[j] = make_double2(k.gamma, k.gamma);
                W1[j] = W0[j];
            } else if (newtonish(MODE)) {
                W0[j] = uf ? ld2s<true>(at(w, j + 1, p)) : ld2(at(w, j + 1, p));
                W1[j] = uf ? ld2s<true>(at(w, j + 1, p + 1)) : ld2(at(w, j + 1, p + 1));
            }
        }
    };
    // LDS-only barrier
    auto lds_barrier = [] { GS_LDS_BARRIER(); }; // lgkmcnt(0), s_barrier
    // the columns left of lane 0 / right of lane 63 on two planes: v(x-1) of lane 0, v(x+2) of lane 63
    auto edges_v = [&](int par, const double2 (&P)[RR], const double2 (&Q)[RR], double (&CLp)[RR], double (&CRp)[RR],
                       double (&CLq)[RR], double (&CRq)[RR]) {
        if (lane == 0) {
#pragma unroll
            for (int j = 0; j < RR; j++) {
                ve[par][wx + 1][0][j] = P[j].x;
                ve[par][wx + 1][0][RR + j] = Q[j].x;
            }
        }
        if (lane == WAVE - 1) {
#pragma unroll
            for (int j = 0; j < RR; j++) {
                ve[par][wx + 1][1][j] = P[j].y;
                ve[par][wx + 1][1][RR + j] = Q[j].y;
            }
        }
        lds_barrier();
#pragma unroll
        for (int j = 0; j < RR; j++) {
            CLp[j] = uniform_d(ve[par][wx][1][j]);
            CRp[j] = uniform_d(ve[par][wx + 2][0][j]);
            CLq[j] = uniform_d(ve[par][wx][1][RR + j]);
            CRq[j] = uniform_d(ve[par][wx + 2][0][RR + j]);
        }
    };
    // r(2X+1) of every lane for two planes: the right neighbour lane's r.x (lane 63: the right wave's)
    auto edges_r = [&](int par, const double2 (&R)[RR], const double2 (&S)[RR], double (&NQ)[RR], double (&NS)[RR]) {
        if (lane == 0) {
#pragma unroll
            for (int j = 0; j < RR; j++) {
                re[par][wx + 1][j] = R[j].x;
                re[par][wx + 1][RR + j] = S[j].x;
            }
        }
        lds_barrier();
#pragma unroll
        for (int j = 0; j < RR; j++) {
            NQ[j] = lane_from_right<true>(R[j].x, uniform_d(re[par][wx + 2][j]));
            NS[j] = lane_from_right<true>(S[j].x, uniform_d(re[par][wx + 2][RR + j]));
        }
    };
    // r = f - A v on fine plane p, rows 1..3 (k_rb KIND 1: same expression, same term order); 0 outside
    // the interior, as the reference's never-written boundary of r
    auto resid = [&](const double2 (&Vm)[RR], const double2 (&Vc)[RR], const double2 (&H)[2], const double2 (&Vp)[RR],
                     const double2 (&F)[RR], const double2 (&W)[RR], const double (&CL)[RR], const double (&CR)[RR], int p,
                     double2 (&R)[RR]) {
        const bool pin = p >= 1 && (p <= fnz || (zhi && p == fnz + 1));
#pragma unroll
        for (int j = 0; j < RR; j++) {
            const double2 c = Vc[j];
            const double2 ym = j == 0 ? H[0] : Vc[j - 1], yp = j == RR - 1 ? H[1] : Vc[j + 1];
            const double xm0 = lane_from_left<true>(c.y, CL[j]);
            const double xp1 = lane_from_right<true>(c.x, CR[j]);
            const double w0 = newtonish(MODE) ? W[j].x : 0.0, w1 = newtonish(MODE) ? W[j].y : 0.0;
            const double a0 = op_value<MODE, UN>(k, c.x, c.y, xm0, yp.x, ym.x, Vp[j].x, Vm[j].x, w0);
            const double a1 = op_value<MODE, UN>(k, c.y, xp1, c.x, yp.y, ym.y, Vp[j].y, Vm[j].y, w1);
            const bool ok = pin && rowc[j + 1];
            R[j] = make_double2((ok && okx0) ? F[j].x - a0 : 0.0, (ok && okx1) ? F[j].y - a1 : 0.0);
        }
    };

    // prologue: r on fine plane 2Zb-1 (the top plane of the previous coarse plane's stencil)
    double2 Vm[RR], V0[RR], Rm[RR];
    double Nm[RR];
    {
        const int p = 2 * Zb - 1;
        double2 Vq[RR], Hq[2], Fq[RR], Wq[RR];
#pragma unroll
        for (int j = 0; j < RR; j++) {
            Vm[j] = ld2(at(v, j + 1, p - 1));
            Vq[j] = ld2(at(v, j + 1, p));
            V0[j] = ld2(at(v, j + 1, p + 1));
            Fq[j] = ld2(at(f, j + 1, p));
            Wq[j] = (MODE == GS_NEWTON_B && k.bconst) ? make_double2(k.gamma, k.gamma)
                    : newtonish(MODE)                  ? ld2(at(w, j + 1, p))
                                                       : make_double2(0.0, 0.0);
        }
        Hq[0] = ld2(at(v, 0, p));
        Hq[1] = ld2(at(v, RR + 1, p));
        double CL[RR], CR[RR], CL2[RR], CR2[RR], N2[RR];
        edges_v(1, Vq, Vq, CL, CR, CL2, CR2);
        resid(Vm, Vq, Hq, V0, Fq, Wq, CL, CR, p, Rm);
        edges_r(1, Rm, Rm, Nm, N2);
#pragma unroll
        for (int j = 0; j < RR; j++) Vm[j] = Vq[j]; // window: Vm = v(2Zb-1), V0 = v(2Zb)
    }
    // Both halves always run (an odd chunk ends with a step whose results are discarded), and every
    // load is unconditional (plane indices clamped), so the slot keeps fixed registers.
    for (int z0 = Zb; z0 <= Ze; z0 += 2) {
#pragma unroll
        for (int ph = 0; ph < 2; ph++) {
            const int Z = z0 + ph;
            load_slot(Z);
            double CL0[RR], CR0[RR], CL1[RR], CR1[RR];
            edges_v(ph, V0, VA, CL0, CR0, CL1, CR1);
            double2 R0[RR], R1[RR];
            resid(Vm, V0, H0, VA, F0, W0, CL0, CR0, 2 * Z, R0);
            resid(V0, VA, H1, VB, F1, W1, CL1, CR1, 2 * Z + 1, R1);
            double N0[RR], N1[RR];
            edges_r(ph, R0, R1, N0, N1);
#pragma unroll
            for (int i = 0; i < NR; i++) {
                if (Z <= Ze && X <= cnx && Y + i <= cny) {
                    double acc = 0.0;
#pragma unroll
                    for (int a = -1; a <= 1; a++)
#pragma unroll
                        for (int b = -1; b <= 1; b++)
#pragma unroll
                            for (int c = -1; c <= 1; c++) {
                                const double wgt = 0.125 * ((2.0 - (a < 0 ? -a : a)) / 2.0) *
                                                   ((2.0 - (b < 0 ? -b : b)) / 2.0) *
                                                   ((2.0 - (c < 0 ? -c : c)) / 2.0);
                                const int j = 2 * i + b + 1;
                                const double2 rp = c < 0 ? Rm[j] : (c == 0 ? R0[j] : R1[j]);
                                const double rn = c < 0 ? Nm[j] : (c == 0 ? N0[j] : N1[j]);
                                acc += wgt * (a < 0 ? rp.x : (a == 0 ? rp.y : rn));
                            }
                    const int64_t q = X + (Y + i) * cldy + (int64_t)Z * cldz;
                    ca[q] = acc;
                    if (cb) cb[q] = acc;
                }
            }
#pragma unroll
            for (int j = 0; j < RR; j++) {
                Vm[j] = VA[j];
                V0[j] = VB[j];
                Rm[j] = R1[j];
                Nm[j] = N1[j];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Trilinear prolongation, closed form per fine point (the reference's inject + X, Y, Z passes,
// CpuSolver.cpp:240-290, combined in the same X -> Y -> Z order). Fine index P-1 is never written by
// the reference (stays 0) and coarse index Pc-1 is the zero boundary, so along each axis:
//   i even -> c(i/2);  i odd -> 0.5*c(i/2) + 0.5*c(i/2+1).
template <bool SUB>
__device__ __forceinline__ double coarse_at(const double* __restrict__ c, const double* __restrict__ sub, int64_t q)
{
    return SUB ? c[q] - sub[q] : c[q];
}

// (x, y, gz) are fine indices, gz global along z; the coarse field's local plane 0 is global cz0.
template <bool SUB>
__device__ __forceinline__ double prolong_value(const double* __restrict__ c, const double* __restrict__ sub, int x,
                                                int y, int gz, int64_t cldy, int64_t cldz, int cz0)
{
    const int cx = x >> 1, cy = y >> 1, cz = (gz >> 1) - cz0;
    const bool ox = x & 1, oy = y & 1, oz = gz & 1;
    auto X = [&](int jy, int jz) -> double {
        const int64_t q = cx + jy * cldy + (int64_t)jz * cldz;
        const double a = coarse_at<SUB>(c, sub, q);
        if (!ox) return a;
        const double b = coarse_at<SUB>(c, sub, q + 1);
        return 0.5 * a + 0.5 * b;
    };
    auto Y = [&](int jz) -> double {
        const double a = X(cy, jz);
        if (!oy) return a;
        const double b = X(cy + 1, jz);
        return 0.5 * a + 0.5 * b;
    };
    const double a = Y(cz);
    if (!oz) return a;
    const double b = Y(cz + 1);
    return 0.5 * a + 0.5 * b;
}

// Fused correction, two fine x-points per lane (x odd, x+1 even): one pair load / store of v, and
// per coarse row the two coarse values c(x>>1), c(x>>1 + 1) that both points interpolate from.
template <bool SUB>
__global__ __launch_bounds__(256) void k_prolong_add(const double* __restrict__ c, const double* __restrict__ sub,
                                                     double* __restrict__ fv, int fnx, int fny, int fnz, int64_t fldy,
                                                     int64_t fldz, int64_t cldy, int64_t cldz, int fz0, int cz0)
{
    const int t = blockIdx.x * 64 + threadIdx.x;
    const int x = 1 + 2 * t;
    const int y = 1 + blockIdx.y * 4 + threadIdx.y;
    const int z = 1 + blockIdx.z;
    if (x > fnx || y > fny) return;
    const int gz = z + fz0;
    const int cx = x >> 1, cy = y >> 1, cz = (gz >> 1) - cz0;
    const bool oy = y & 1, oz = gz & 1;
    // X pass: e0 at fine x (odd: average of c(cx), c(cx+1)), e1 at x+1 (even: injection of c(cx+1))
    auto X2 = [&](int jy, int jz, double& e0, double& e1) {
        const int64_t q = cx + jy * cldy + (int64_t)jz * cldz;
        const double a = coarse_at<SUB>(c, sub, q), b = coarse_at<SUB>(c, sub, q + 1);
        e0 = 0.5 * a + 0.5 * b;
        e1 = b;
    };
    // Y pass on top of X
    auto Y2 = [&](int jz, double& e0, double& e1) {
        double a0, a1;
        X2(cy, jz, a0, a1);
        if (!oy) {
            e0 = a0;
            e1 = a1;
            return;
        }
        double b0, b1;
        X2(cy + 1, jz, b0, b1);
        e0 = 0.5 * a0 + 0.5 * b0;
        e1 = 0.5 * a1 + 0.5 * b1;
    };
    double e0, e1;
    Y2(cz, e0, e1);
    if (oz) { // Z pass
        double g0, g1;
        Y2(cz + 1, g0, g1);
        e0 = 0.5 * e0 + 0.5 * g0;
        e1 = 0.5 * e1 + 0.5 * g1;
    }
    const int64_t p = x + y * fldy + (int64_t)z * fldz;
    if (x + 1 <= fnx) {
        const double2 v = ld2(fv + p);
        st2s<true>(fv + p, v.x + e0, v.y + e1);
    } else {
        fv[p] = fv[p] + e0;
    }
}

// The corrected iterate v + P v^2h on the four fine columns around every interior column-block
// boundary of the prolongation pair (k_tb2y XH + PRO): columns xb-2 .. xb+1 of the boundary at xb (the
// first column of the right block), rows 0..ny+1, local planes -1..nz+2 — what the blocks on either side
// read of the neighbour's columns. A point gets the correction where the pair's lanes correct it (x, y
// interior; the plane interior or a ghost plane of an internal slab side: pok) and keeps v elsewhere,
// with the reference's X, Y, Z pass arithmetic (prolong_value), so the strip holds bit for bit what the
// neighbour block's lanes compute in registers. Layout: es[((b * (nz + 4) + p + 1) * 4 + c) * (ny + 2) + y].
// The coarse field is indexed from the plane under fine local plane 0 (z0 even: local parities are global).
template <bool SUB>
__global__ __launch_bounds__(256) void k_pro_strip(const double* __restrict__ v, const double* __restrict__ c,
                                                   const double* __restrict__ sub, double* __restrict__ es, int nx,
                                                   int ny, int nz, int64_t ldy, int64_t ldz, int64_t cldy,
                                                   int64_t cldz, int bw, int zlo, int zhi)
{
    // four lanes per row (one per column), 64 rows per block: a wave's v load touches 16 rows' 32-B runs
    // and its coarse loads ~8 rows' lines (one thread per row and four columns, r03j: 159 us per 1024^3
    // launch, address-unit bound — every lane of a load on its own cache line)
    const int col = (int)threadIdx.x & 3;
    const int y = blockIdx.x * 64 + ((int)threadIdx.x >> 2);
    if (y > ny + 1) return;
    const int p = (int)blockIdx.y - 1;
    const int b = (int)blockIdx.z;
    const int x = 1 + (b + 1) * bw - 2 + col;
    const bool pok = (p >= 1 && p <= nz) || (zlo && p <= 0) || (zhi && p > nz);
    double val = v[x + (int64_t)y * ldy + (int64_t)p * ldz];
    if (pok && y >= 1 && y <= ny && x >= 1 && x <= nx) val = val + prolong_value<SUB>(c, sub, x, y, p, cldy, cldz, 0);
    es[(((int64_t)b * (nz + 4) + p + 1) * 4 + col) * (ny + 2) + y] = val;
}

// ---------------------------------------------------------------------------------------------
// Small levels (LINEAR, canonical stencil): a level's whole down-leg step or up-leg step in ONE launch
// of LDS-tiled blocks that recompute their halos instead of exchanging them. A 32^3 or 16^3 level is
// pure launch latency (~4.5 us per operator on a chip it cannot fill): the reference's pre-smoothing
// (2 sweeps), residual and restriction take one launch instead of three to five, the prolongation,
// correction and 2 post-smoothing sweeps one instead of three. A block owns a TS^3 tile of fine points
// (TS = 8: a 4^3 tile of coarse points) and evaluates every stage on the tile plus the halo the later
// stages read (v: 15^3 -> sweep 1: 13^3 -> sweep 2: 11^3 -> residual: 9^3 -> restriction), every point
// with the expression of the kernel it replaces (op_value / jacobi_update / the restriction's 27 terms
// in the reference's order / prolong_value), so every output is bit-identical to the unfused sequence.
// Points outside the level's interior keep their loaded value (a stored sweep leaves boundary values
// as they are) and have r = 0 (the reference never writes r there); loads are clamped to the padded
// array, whose clamped copies only ever feed such boundary points.
constexpr int TS = 8, TS_T = 1024; // 1024 threads: ~3 points per thread and stage (256: 12-14 us per launch, latency-bound)

// one Jacobi sweep over a tile: dst (edge dN) from src (edge dN + 2; dst i <-> src i + 1), f (and, NEWTON,
// the linearisation point w) from tiles of edge fN (dst i <-> f i + fo); global index of dst point 0: g0
template <int MODE, bool UN>
__device__ __forceinline__ void tile_sweep(const Coef& k, double om, const double* src, double* dst, int dN,
                                           const double* F, const double* W, int fN, int fo, int gx0, int gy0, int gz0,
                                           int nx, int ny, int nz)
{
    const int sN = dN + 2, total = dN * dN * dN;
    for (int t = threadIdx.x; t < total; t += TS_T) {
        const int i = t % dN, j = (t / dN) % dN, l = t / (dN * dN);
        const int gx = gx0 + i, gy = gy0 + j, gz = gz0 + l;
        const int q = (i + 1) + sN * ((j + 1) + sN * (l + 1));
        const double c = src[q];
        double nv = c;
        if (gx >= 1 && gx <= nx && gy >= 1 && gy <= ny && gz >= 1 && gz <= nz) {
            const int qf = (i + fo) + fN * ((j + fo) + fN * (l + fo));
            const double w = newtonish(MODE) ? W[qf] : 0.0;
            const double a = op_value<MODE, UN>(k, c, src[q + 1], src[q - 1], src[q + sN], src[q - sN],
                                                 src[q + sN * sN], src[q - sN * sN], w);
            nv = jacobi_update<MODE>(k, c, F[qf] - a, w, om);
        }
        dst[t] = nv;
    }
}

// a tile of a padded field, clamped to the padded array (ZV: identically zero)
template <bool ZV>
__device__ __forceinline__ void tile_load(const double* __restrict__ g, double* dst, int N, int gx0, int gy0, int gz0,
                                          int nx, int ny, int nz, int64_t ldy, int64_t ldz)
{
    for (int t = threadIdx.x; t < N * N * N; t += TS_T) {
        if (ZV) {
            dst[t] = 0.0;
            continue;
        }
        const int i = t % N, j = (t / N) % N, l = t / (N * N);
        const int x = min(max(gx0 + i, 0), nx + 1), y = min(max(gy0 + j, 0), ny + 1), z = min(max(gz0 + l, 0), nz + 1);
        dst[t] = g[x + (int64_t)y * ldy + (int64_t)z * ldz];
    }
}

// pre-smoothing pair + residual + full weighting of a small level: v_out = S(S(v)) on the tile's fine
// points, coarse f = R(f - A v_out) on its coarse points (CpuSolver.cpp:88-99 with preSmoothing 2; ZV:
// v = 0, the coarse level's first sweeps after CpuSolver.cpp:100-101). MODE LINEAR, or NEWTON with the
// level's newtonV as w (the operator and the update linearised there, CpuSolver.cpp:63-66, :166-172).
template <int MODE, bool ZV, bool UN>
__global__ __launch_bounds__(TS_T) void k_tile_pre_rr(Coef k, const double* __restrict__ v, const double* __restrict__ f,
                                                      const double* __restrict__ w, double* __restrict__ vout,
                                                      double* __restrict__ cf, int nx, int ny, int nz, int64_t ldy,
                                                      int64_t ldz, int cnx, int cny, int cnz, int64_t cldy, int64_t cldz)
{
    constexpr int NV = TS + 7, N1 = TS + 5, N2 = TS + 3, NR = TS + 1, NF = TS + 5;
    constexpr int NW = newtonish(MODE) ? NF : 1;
    __shared__ double sv[NV * NV * NV], s1[N1 * N1 * N1], s2[N2 * N2 * N2], sf[NF * NF * NF], sw[NW * NW * NW];
    double* sr = sv; // the residual tile reuses v's storage once sweep 1 is done
    const int tx = 1 + TS * (int)blockIdx.x, ty = 1 + TS * (int)blockIdx.y, tz = 1 + TS * (int)blockIdx.z;
    tile_load<ZV>(v, sv, NV, tx - 3, ty - 3, tz - 3, nx, ny, nz, ldy, ldz);
    tile_load<false>(f, sf, NF, tx - 2, ty - 2, tz - 2, nx, ny, nz, ldy, ldz);
    if (newtonish(MODE)) tile_load<false>(w, sw, NF, tx - 2, ty - 2, tz - 2, nx, ny, nz, ldy, ldz);
    __syncthreads();
    tile_sweep<MODE, UN>(k, k.omega[0], sv, s1, N1, sf, sw, NF, 0, tx - 2, ty - 2, tz - 2, nx, ny, nz);
    __syncthreads();
    tile_sweep<MODE, UN>(k, k.omega[1], s1, s2, N2, sf, sw, NF, 1, tx - 1, ty - 1, tz - 1, nx, ny, nz);
    __syncthreads();
    // the tile's own fine points of v'' (interior only)
    for (int t = threadIdx.x; t < TS * TS * TS; t += TS_T) {
        const int i = t % TS, j = (t / TS) % TS, l = t / (TS * TS);
        const int x = tx + i, y = ty + j, z = tz + l;
        if (x <= nx && y <= ny && z <= nz)
            vout[x + (int64_t)y * ldy + (int64_t)z * ldz] = s2[(i + 1) + N2 * ((j + 1) + N2 * (l + 1))];
    }
    // r = f - A v'' on fine points tx .. tx + TS (the restriction's 3-point windows); 0 off the interior
    for (int t = threadIdx.x; t < NR * NR * NR; t += TS_T) {
        const int i = t % NR, j = (t / NR) % NR, l = t / (NR * NR);
        const int gx = tx + i, gy = ty + j, gz = tz + l;
        double r = 0.0;
        if (gx >= 1 && gx <= nx && gy >= 1 && gy <= ny && gz >= 1 && gz <= nz) {
            const int q = (i + 1) + N2 * ((j + 1) + N2 * (l + 1));
            const int qf = (i + 2) + NF * ((j + 2) + NF * (l + 2));
            const double c = s2[q];
            const double a = op_value<MODE, UN>(k, c, s2[q + 1], s2[q - 1], s2[q + N2], s2[q - N2], s2[q + N2 * N2],
                                                 s2[q - N2 * N2], newtonish(MODE) ? sw[qf] : 0.0);
            r = sf[qf] - a;
        }
        sr[t] = r;
    }
    __syncthreads();
    // coarse points X = (tx + 1) / 2 + 0..TS/2-1 (fine centre 2X = tx + 1 + 2u): the 27 terms in the
    // reference's order (CpuSolver.cpp:225-231)
    constexpr int TC = TS / 2;
    if (threadIdx.x < TC * TC * TC) {
        const int u = threadIdx.x % TC, o2 = (threadIdx.x / TC) % TC, o = threadIdx.x / (TC * TC);
        const int X = (tx + 1) / 2 + u, Y = (ty + 1) / 2 + o2, Z = (tz + 1) / 2 + o;
        if (X <= cnx && Y <= cny && Z <= cnz) {
            double acc = 0.0;
#pragma unroll
            for (int a = -1; a <= 1; a++)
#pragma unroll
                for (int b = -1; b <= 1; b++)
#pragma unroll
                    for (int c = -1; c <= 1; c++) {
                        const double wgt = 0.125 * ((2.0 - (a < 0 ? -a : a)) / 2.0) * ((2.0 - (b < 0 ? -b : b)) / 2.0) *
                                           ((2.0 - (c < 0 ? -c : c)) / 2.0);
                        acc += wgt * sr[(1 + 2 * u + a) + NR * ((1 + 2 * o2 + b) + NR * (1 + 2 * o + c))];
                    }
            cf[X + (int64_t)Y * cldy + (int64_t)Z * cldz] = acc;
        }
    }
}

// prolongation + correction + 2 post-smoothing sweeps of a small level: v_out = S(S(v + P c)) on the tile's
// fine points (CpuSolver.cpp:127-134 with the first two post-smoothing sweeps); MODE as above
template <int MODE, bool UN>
__global__ __launch_bounds__(TS_T) void k_tile_pro2(Coef k, const double* __restrict__ v, const double* __restrict__ c,
                                                    const double* __restrict__ f, const double* __restrict__ w,
                                                    double* __restrict__ vout, int nx, int ny, int nz, int64_t ldy,
                                                    int64_t ldz, int64_t cldy, int64_t cldz)
{
    constexpr int NU = TS + 4, N1 = TS + 2, NF = TS + 2;
    constexpr int NW = newtonish(MODE) ? NF : 1;
    __shared__ double su[NU * NU * NU], s1[N1 * N1 * N1], sf[NF * NF * NF], sw[NW * NW * NW];
    const int tx = 1 + TS * (int)blockIdx.x, ty = 1 + TS * (int)blockIdx.y, tz = 1 + TS * (int)blockIdx.z;
    for (int t = threadIdx.x; t < NU * NU * NU; t += TS_T) {
        const int i = t % NU, j = (t / NU) % NU, l = t / (NU * NU);
        const int gx = tx - 2 + i, gy = ty - 2 + j, gz = tz - 2 + l;
        const int x = min(max(gx, 0), nx + 1), y = min(max(gy, 0), ny + 1), z = min(max(gz, 0), nz + 1);
        double u = v[x + (int64_t)y * ldy + (int64_t)z * ldz];
        if (gx >= 1 && gx <= nx && gy >= 1 && gy <= ny && gz >= 1 && gz <= nz)
            u = u + prolong_value<false>(c, nullptr, gx, gy, gz, cldy, cldz, 0);
        su[t] = u;
    }
    tile_load<false>(f, sf, NF, tx - 1, ty - 1, tz - 1, nx, ny, nz, ldy, ldz);
    if (newtonish(MODE)) tile_load<false>(w, sw, NF, tx - 1, ty - 1, tz - 1, nx, ny, nz, ldy, ldz);
    __syncthreads();
    tile_sweep<MODE, UN>(k, k.omega[0], su, s1, N1, sf, sw, NF, 0, tx - 1, ty - 1, tz - 1, nx, ny, nz);
    __syncthreads();
    for (int t = threadIdx.x; t < TS * TS * TS; t += TS_T) {
        const int i = t % TS, j = (t / TS) % TS, l = t / (TS * TS);
        const int gx = tx + i, gy = ty + j, gz = tz + l;
        if (gx > nx || gy > ny || gz > nz) continue;
        const int q = (i + 1) + N1 * ((j + 1) + N1 * (l + 1));
        const int qf = (i + 1) + NF * ((j + 1) + NF * (l + 1));
        const double cc = s1[q];
        const double wv = newtonish(MODE) ? sw[qf] : 0.0;
        const double a = op_value<MODE, UN>(k, cc, s1[q + 1], s1[q - 1], s1[q + N1], s1[q - N1], s1[q + N1 * N1],
                                             s1[q - N1 * N1], wv);
        vout[gx + (int64_t)gy * ldy + (int64_t)gz * ldz] = jacobi_update<MODE>(k, cc, sf[qf] - a, wv, k.omega[1]);
    }
}

// Unfused reference-shaped interpolate (whole padded fine array), used by parity tests.
__global__ __launch_bounds__(256) void k_interpolate(const double* __restrict__ c, double* __restrict__ e, int fPx,
                                                     int fPy, int fPz, int64_t fldy, int64_t fldz, int64_t cldy,
                                                     int64_t cldz)
{
    const int x = blockIdx.x * 64 + threadIdx.x;
    const int y = blockIdx.y * 4 + threadIdx.y;
    const int z = blockIdx.z;
    if (x >= fPx || y >= fPy) return;
    const int64_t p = x + y * fldy + (int64_t)z * fldz;
    if (x == fPx - 1 || y == fPy - 1 || z == fPz - 1) {
        e[p] = 0.0;
        return;
    }
    e[p] = prolong_value<false>(c, nullptr, x, y, z, cldy, cldz, 0);
}

// ---------------------------------------------------------------------------------------------
// Level-0 right-hand side, CpuGridData.cpp:7-12, 44-78 (same expression order).
__device__ __forceinline__ double rhs_f0(double x)
{
    return 100 * x * (x - 1.0) * x * (x - 1.0) * x * (x - 1.0) * x * (x - 1.0);
}
__device__ __forceinline__ double rhs_f2(double x)
{
    return 100.0 * 4.0 * (x - 1.0) * (x - 1.0) * x * x * (14.0 * x * x - 14.0 * x + 3);
}

__global__ __launch_bounds__(256) void k_rhs(double* __restrict__ f, int mode, double h, double gamma, int nx, int ny,
                                             int nz, int64_t z0, int64_t ldy, int64_t ldz)
{
    const int X = blockIdx.x * 64 + threadIdx.x; // padded indices
    const int Y = blockIdx.y * 4 + threadIdx.y;
    const int Z = blockIdx.z;
    if (X > nx + 1 || Y > ny + 1) return;
    const int64_t p = X + Y * ldy + (int64_t)Z * ldz;
    const int64_t Zg = Z + z0;
    if (mode == GS_LINEAR) {
        if (X < 1 || X > nx || Y < 1 || Y > ny || Z < 1 || Z > nz) return;
        const double x = (int)(X - 1) * h, y = (int)(Y - 1) * h, z = (int)(Zg - 1) * h;
        f[p] = -(rhs_f2(x) * rhs_f0(y) * rhs_f0(z) + rhs_f0(x) * rhs_f2(y) * rhs_f0(z) +
                 rhs_f0(x) * rhs_f0(y) * rhs_f2(z));
    } else {
        const double x = (int)X * h, y = (int)Y * h, z = (int)Zg * h;
        const double ux = x - x * x, uy = y - y * y, uz = z - z * z;
        f[p] = 2.0 * ((y - y * y) * (z - z * z) + (x - x * x) * (z - z * z) + (x - x * x) * (y - y * y)) +
               gamma * ux * uy * uz * exp(ux * uy * uz);
    }
}

// dst = src over n doubles (Vector3 copy-assignment): one dwordx4 per thread and iteration, both
// streams non-temporal (the 1 GB newtonF copy of a 512^3 Newton solve at the box's copy rate instead of
// hipMemcpyAsync's ~2.7 TB/s). head (0 or 1) leading elements bring both pointers to 16 B (a field's
// origin is 8 B past a 16-B boundary); they and an odd tail are copied by thread 0
__global__ __launch_bounds__(256) void k_copy(double* __restrict__ dst, const double* __restrict__ src, int64_t n,
                                              int head)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, n2 = (n - head) / 2;
    const double* s = src + head;
    double* d = dst + head;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n2; i += stride) {
        const double2 t = ld2s<true>(s + 2 * i);
        st2s<true>(d + 2 * i, t.x, t.y);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (head) dst[0] = src[0];
        if ((n - head) & 1) dst[n - 1] = src[n - 1];
    }
}

// GS_NEWTON_B's linearisation factor (bfac_of) elementwise over n elements, dwordx4 streams when both arrays
// share an alignment (head: 0 or 1 leading element), else one per thread (-1)
__global__ __launch_bounds__(256) void k_bfac(double* __restrict__ b, const double* __restrict__ w, int64_t n,
                                              double gamma, int head)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, t0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (head < 0) {
        for (int64_t i = t0; i < n; i += stride) b[i] = bfac_of(gamma, w[i]);
        return;
    }
    const int64_t n2 = (n - head) / 2;
    for (int64_t i = t0; i < n2; i += stride) {
        const double2 t = ld2s<true>(w + head + 2 * i);
        st2s<true>(b + head + 2 * i, bfac_of(gamma, t.x), bfac_of(gamma, t.y));
    }
    if (t0 == 0) {
        if (head) b[0] = bfac_of(gamma, w[0]);
        if ((n - head) & 1) b[n - 1] = bfac_of(gamma, w[n - 1]);
    }
}

__global__ __launch_bounds__(256) void k_fill(double* __restrict__ dst, double value, int64_t n)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += stride) dst[i] = value;
}

__global__ __launch_bounds__(256) void k_axpy(double* __restrict__ y, const double* __restrict__ x, double a,
                                              int64_t n)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += stride) {
        if (a == 1.0) y[i] = y[i] + x[i];
        else if (a == -1.0) y[i] = y[i] - x[i];
        else y[i] = y[i] + a * x[i];
    }
}

// ---------------------------------------------------------------------------------------------
// Full multigrid's prolongation of a SOLUTION (gs_fmg_prolong; not a reference operator): tricubic, separable,
// evaluated x, then y, then z, on aligned levels (fine n = 2 coarse n + 1 per axis, so padded fine index 2i is coarse
// index i; the boundary ring takes part as data). Per axis, "cell" i = 0..c produces the odd fine index 2i+1 from
// four consecutive coarse values (three when c = 1) and, for i < c, the even index 2i+2 by injection:
//   1 <= i <= c-1   (((-w[i-1] + 9 w[i]) + 9 w[i+1]) - w[i+2]) / 16
//   i = 0           (((5 w[0] + 15 w[1]) - 5 w[2]) + w[3]) / 16           i = c: the mirror image from the top end
//   c = 1           ((3 w[0] + 6 w[1]) - w[2]) / 8                          and its mirror
// fmg_axis gives the first index q of the cell's window, which formula it takes (kind 0 / 1 / 2), whether the
// operands run downwards from the window's top (rev) and where the injected value sits in the window (ev: 1 or 2).
__device__ __forceinline__ void fmg_axis(int i, int c, int& q, int& kind, bool& rev, int& ev)
{
    if (c == 1) {
        q = 0;
        kind = 2;
        rev = i != 0;
    } else if (i <= 0) {
        q = 0;
        kind = 1;
        rev = false;
    } else if (i >= c) {
        q = c - 2;
        kind = 1;
        rev = true;
    } else {
        q = i - 1;
        kind = 0;
        rev = false;
    }
    ev = i + 1 - q;
}

__device__ __forceinline__ double fmg_interp(int kind, bool rev, double w0, double w1, double w2, double w3)
{
    if (kind == 0) return (((-w0 + 9.0 * w1) + 9.0 * w2) - w3) / 16.0;
    if (kind == 1) {
        const double a = rev ? w3 : w0, b = rev ? w2 : w1, c = rev ? w1 : w2, d = rev ? w0 : w3;
        return (((5.0 * a + 15.0 * b) - 5.0 * c) + d) / 16.0;
    }
    const double a = rev ? w2 : w0, c = rev ? w0 : w2; // three values: w3 is not read
    return ((3.0 * a + 6.0 * w1) - c) / 8.0;
}

// One block: FP_TX x-cells (a wave: one 16-byte store of the fine pair 2i+1, 2i+2 per lane, 1 KiB per row) by FP_TY
// y-cells (one wave each), marching a chunk of z-cells. Per coarse plane the block stages the tile's rows and
// columns with their -1 / +2 halo in LDS (two buffers, one barrier per plane: plane p+1, loaded a step earlier, is
// written while plane p is computed, and plane p+2's loads are in flight), each thread forms the x- then
// y-interpolated values of its 2 x 2 fine columns on that plane, and the z pass runs on a sliding window of four such
// planes in registers. Loads stay inside the padded coarse array: the staged index ranges are clamped to it, and so
// are the windows.
constexpr int FP_TX = 64, FP_TY = 4, FP_LW = FP_TX + 4, FP_LR = FP_TY + 3;

template <bool NT>
__global__ __launch_bounds__(FP_TX* FP_TY) void k_fmg_prolong(const double* __restrict__ c, double* __restrict__ f,
                                                               int cnx, int cny, int cnz, int64_t cldy, int64_t cldz,
                                                               int64_t fldy, int64_t fldz, int zc, int al)
{
    __shared__ double pl[2][FP_LR][FP_LW];
    // (the wave's y-cell in an SGPR: its formula and window rows are then chosen by scalar branches)
    const int lane = threadIdx.x, wy = __builtin_amdgcn_readfirstlane(threadIdx.y), tid = wy * FP_TX + lane;
    const int i0 = blockIdx.x * FP_TX, j0 = blockIdx.y * FP_TY, k0 = blockIdx.z * zc, k1 = min(k0 + zc, cnz + 1);
    // staged columns / rows / planes: what the tile's windows cover, inside the padded coarse array
    const int clo = min(max(i0 - 1, 0), max(cnx - 2, 0)), chi = min(i0 + FP_TX + 1, cnx + 1), ncol = chi - clo + 1;
    const int rlo = min(max(j0 - 1, 0), max(cny - 2, 0)), rhi = min(j0 + FP_TY + 1, cny + 1), nrow = rhi - rlo + 1;
    const int pstart = min(max(k0 - 1, 0), max(cnz - 2, 0)), pend = min(k1 + 1, cnz + 1);
    const int i = i0 + lane, j = j0 + wy;
    const bool okx = i <= cnx, oky = j <= cny, x2 = i < cnx, y2 = j < cny;
    int qx, kx, ex, qy, ky, ey;
    bool rx, ry;
    fmg_axis(min(i, cnx), cnx, qx, kx, rx, ex);
    fmg_axis(min(j, cny), cny, qy, ky, ry, ey);
    const bool xedge_wave = __any(kx != 0) != 0;
    // window positions in the staged plane (a three-value axis repeats its last index; that operand is not used)
    int lc[4], lr[4];
#pragma unroll
    for (int m = 0; m < 4; m++) {
        lc[m] = min(qx + m, cnx + 1) - clo;
        lr[m] = min(qy + m, cny + 1) - rlo;
    }
    // the (at most two) staged elements this thread loads per plane
    const int n = nrow * ncol;
    int64_t goff[2];
    int loff[2];
    bool gok[2];
#pragma unroll
    for (int m = 0; m < 2; m++) {
        const int e = tid + m * FP_TX * FP_TY;
        gok[m] = e < n;
        const int r = gok[m] ? e / ncol : 0, col = gok[m] ? e - r * ncol : 0;
        goff[m] = (clo + col) + (int64_t)(rlo + r) * cldy;
        loff[m] = r * FP_LW + col;
    }
    static_assert(FP_LR * (FP_TX + 3) <= 2 * FP_TX * FP_TY, "two staged elements per thread cover a plane");
    double g[2], gn[2]; // the thread's elements of plane p + 1 (loaded a step ago) and p + 2 (in flight)
#pragma unroll
    for (int m = 0; m < 2; m++) g[m] = gok[m] ? c[goff[m] + (int64_t)pstart * cldz] : 0.0;
#pragma unroll
    for (int m = 0; m < 2; m++)
        if (gok[m]) (&pl[0][0][0])[loff[m]] = g[m];
#pragma unroll
    for (int m = 0; m < 2; m++) g[m] = gok[m] && pstart < pend ? c[goff[m] + (int64_t)(pstart + 1) * cldz] : 0.0;
    __syncthreads();

    // fine pairs (x odd, x even) of the thread's two fine rows on the last four coarse planes
    double2 wo[4], we[4]; // [plane]: row 2j+1, row 2j+2
#pragma unroll
    for (int m = 0; m < 4; m++) wo[m] = we[m] = make_double2(0.0, 0.0);
    double* const frow = f + (2 * i + 1) + (int64_t)(2 * j + 1) * fldy;
    auto store = [&](int64_t off, double2 v) {
        double* p = frow + off;
        if (x2) {
            if (al) st2s<NT>(p, v.x, v.y);
            else {
                p[0] = v.x;
                p[1] = v.y;
            }
        } else {
            p[0] = v.x;
        }
    };
    // fine planes 2k+1 (kind, rev over the window a..d) and, with ev, 2k+2 (the window's plane ev)
    auto emit = [&](int k, int kind, bool rev, const double2& ao, const double2& ae, const double2& bo,
                    const double2& be, const double2& co, const double2& ce, const double2& d_o, const double2& de,
                    int ev) {
        if (!(okx && oky)) return;
        const int64_t z = (int64_t)(2 * k + 1) * fldz;
        store(z, make_double2(fmg_interp(kind, rev, ao.x, bo.x, co.x, d_o.x), fmg_interp(kind, rev, ao.y, bo.y, co.y, d_o.y)));
        if (y2)
            store(z + fldy,
                  make_double2(fmg_interp(kind, rev, ae.x, be.x, ce.x, de.x), fmg_interp(kind, rev, ae.y, be.y, ce.y, de.y)));
        if (ev) {
            store(z + fldz, ev == 1 ? bo : co);
            if (y2) store(z + fldz + fldy, ev == 1 ? be : ce);
        }
    };

    int cur = 0;
    for (int p = pstart; p <= pend; p++) {
        const bool more = p < pend;
#pragma unroll
        for (int m = 0; m < 2; m++) gn[m] = gok[m] && p + 2 <= pend ? c[goff[m] + (int64_t)(p + 2) * cldz] : 0.0;
        // x pass on the window's four rows, then the y pass
        double xo[4], xe[4];
#pragma unroll
        for (int m = 0; m < 4; m++) {
            const double* row = pl[cur][lr[m]];
            const double a = row[lc[0]], b = row[lc[1]], cc = row[lc[2]], d = row[lc[3]];
            // every lane takes the interior formula; the waves holding x-cell 0 or cnx redo that one lane
            double o = fmg_interp(0, false, a, b, cc, d);
            if (xedge_wave) {
                if (kx != 0) o = fmg_interp(kx, rx, a, b, cc, d);
            }
            xo[m] = o;
            xe[m] = ex == 1 ? b : cc;
        }
#pragma unroll
        for (int m = 0; m < 3; m++) {
            wo[m] = wo[m + 1];
            we[m] = we[m + 1];
        }
        wo[3] = make_double2(fmg_interp(ky, ry, xo[0], xo[1], xo[2], xo[3]), fmg_interp(ky, ry, xe[0], xe[1], xe[2], xe[3]));
        we[3] = make_double2(ey == 1 ? xo[1] : xo[2], ey == 1 ? xe[1] : xe[2]);
        // the z-cells complete with plane p (wo / we [m] hold plane p - 3 + m)
        if (cnz == 1) {
            if (p == 2) {
                emit(0, 2, false, wo[1], we[1], wo[2], we[2], wo[3], we[3], wo[3], we[3], 1);
                emit(1, 2, true, wo[1], we[1], wo[2], we[2], wo[3], we[3], wo[3], we[3], 0);
            }
        } else {
            if (p == 3 && k0 == 0) emit(0, 1, false, wo[0], we[0], wo[1], we[1], wo[2], we[2], wo[3], we[3], 1);
            const int k = p - 2;
            if (k >= 1 && k <= cnz - 1 && k >= k0 && k < k1)
                emit(k, 0, false, wo[0], we[0], wo[1], we[1], wo[2], we[2], wo[3], we[3], 2);
            if (p == cnz + 1 && k1 > cnz) emit(cnz, 1, true, wo[0], we[0], wo[1], we[1], wo[2], we[2], wo[3], we[3], 0);
        }
        if (more) {
#pragma unroll
            for (int m = 0; m < 2; m++)
                if (gok[m]) (&pl[cur ^ 1][0][0])[loff[m]] = g[m];
        }
        __syncthreads();
        cur ^= 1;
        g[0] = gn[0];
        g[1] = gn[1];
    }
}

// ---------------------------------------------------------------------------------------------
// The coarse end of the V-cycle in ONE launch of ONE workgroup (gs_coarse_cycle). A level of a few
// hundred points is pure launch latency per operator on a chip it cannot fill (~4.5 us a sweep);
// here the whole recursion of CpuSolver::vcycle below level lv[0] (CpuSolver.cpp:92-135) runs in one
// 1024-thread workgroup whose levels stay in L2, with a workgroup barrier between operators instead
// of a kernel boundary (the waves of a workgroup share one CU's L1, so the barrier's workgroup-scope
// fences order every store before the next operator's loads). Each point is computed by the
// expression of the per-operator kernel it replaces (k_generic KIND 0 / 1 / 2, k_restrict,
// k_prolong_add), so every field is bit-identical to the per-operator launch sequence.
constexpr int CC_T = 1024, CC_MAXLEV = 8;

struct CcLevel {
    double *v, *va, *f, *r, *rv, *w; // iterate, ping-pong partner, rhs, residual, restV (FAS), newtonV
    int64_t ldy, ldz;
    int nx, ny, nz, vz; // vz: the iterate is the zero iterate, not stored
    Coef k;
};
struct CcPlan {
    CcLevel L[CC_MAXLEV];
    int n, pre, post;
    // per-sweep relaxation weights (gs_coarse_cycle_w), by value: the k-th pre-smoothing sweep of every level takes
    // wpre[k], the k-th post-smoothing sweep wpost[k], the coarsest level's pre + post sweeps wpre then wpost.
    // weighted == 0: every sweep takes its level's Coef::omega[0]
    int weighted;
    double wpre[GS_MAX_WEIGHTS], wpost[GS_MAX_WEIGHTS];
};

__device__ __forceinline__ int64_t cc_at(const CcLevel& L, int x, int y, int z)
{
    return x + y * L.ldy + (int64_t)z * L.ldz;
}

// dst[p] (and dst2[p]) = fn(x, y, z, p) for every interior point p of a level, x fastest, strided
// over the workgroup, B points per thread and pass: all B values are computed before any is stored,
// so a phase reading the field it writes (prolongation, f += A u) sees only old values.
template <int B, class F>
__device__ __forceinline__ void cc_map_b(const CcLevel& L, double* dst, double* dst2, F& fn)
{
    const int n = L.nx * L.ny * L.nz;
    for (int i0 = threadIdx.x; i0 < n; i0 += B * CC_T) {
        double val[B];
        int64_t q[B];
        bool ok[B];
#pragma unroll
        for (int b = 0; b < B; b++) {
            const int i = i0 + b * CC_T;
            ok[b] = i < n;
            const int ii = ok[b] ? i : i0; // a valid point; its value is discarded
            const int t = ii / L.nx, z = t / L.ny;
            const int x = 1 + ii - t * L.nx, y = 1 + t - z * L.ny;
            q[b] = cc_at(L, x, y, 1 + z);
            val[b] = fn(x, y, 1 + z, q[b]);
        }
#pragma unroll
        for (int b = 0; b < B; b++)
            if (ok[b]) {
                dst[q[b]] = val[b];
                if (dst2) dst2[q[b]] = val[b];
            }
    }
}
template <class F>
__device__ __forceinline__ void cc_map(const CcLevel& L, double* dst, double* dst2, F&& fn)
{
    cc_map_b<1>(L, dst, dst2, fn); // 2 points per pass measured no faster (the levels it runs are tiny)
}

// A(u) at p in config order (k_generic): the stencil sum, / h^2, the non-linear term; c = u(p),
// wv = w(p) (NEWTON). uz: u is the zero iterate (literal zeros, as k_generic's v == NULL).
template <int MODE>
__device__ __forceinline__ double cc_op(const Coef& k, const double* __restrict__ u, bool uz,
                                        const double* __restrict__ w, int64_t p, double& c, double& wv)
{
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 7; i++) s += k.s[i] * (uz ? 0.0 : u[p + k.off[i]]);
    s = div_hh(k, s);
    c = uz ? 0.0 : u[p];
    wv = newtonish(MODE) ? w[p] : 0.0;
    return op_finish<MODE>(k, s, c, wv);
}

template <int MODE>
__global__ __launch_bounds__(CC_T) void k_coarse_cycle(CcPlan P)
{
    unsigned alt = 0, zero = 0; // per level bit: the iterate is in va / is the unstored zero
    for (int l = 0; l < P.n; l++)
        if (P.L[l].vz) zero |= 1u << l;
    auto cur = [&](int l) { return ((alt >> l) & 1) ? P.L[l].va : P.L[l].v; };
    // v = 0 made real (HipSolver::materialize)
    auto materialize = [&](int l) {
        if (!((zero >> l) & 1)) return;
        const CcLevel& L = P.L[l];
        double* v = cur(l);
        cc_map(L, v, nullptr, [&](int, int, int, int64_t) { return 0.0; });
        __syncthreads();
        zero &= ~(1u << l);
    };
    // `sweeps` Jacobi sweeps, residual and update fused (k_generic KIND 0), ping-pong v <-> va
    // (post: the sweeps are post-smoothing sweeps; otherwise pre-smoothing sweeps, continued by the post-smoothing
    // ones past P.pre — the coarsest level)
    auto smooth = [&](int l, int sweeps, bool post) {
        const CcLevel& L = P.L[l];
        if (sweeps == 0) materialize(l);
        for (int s = 0; s < sweeps; s++) {
            const int ws = post ? s + P.pre : s;
            const double om = !P.weighted ? L.k.omega[0] : ws < P.pre ? P.wpre[ws] : P.wpost[ws - P.pre];
            const bool uz = (zero >> l) & 1;
            const double* in = cur(l);
            double* out = ((alt >> l) & 1) ? L.v : L.va;
            cc_map(L, out, nullptr, [&](int, int, int, int64_t p) {
                double c, wv;
                const double a = cc_op<MODE>(L.k, in, uz, L.w, p, c, wv);
                const double r = L.f[p] - a;
                return jacobi_update<MODE>(L.k, c, r, wv, om);
            });
            __syncthreads();
            alt ^= 1u << l;
            zero &= ~(1u << l);
        }
    };
    // coarse interior of C <- 27-point full weighting of the fine field src of F (k_restrict)
    auto restrict_to = [&](const double* __restrict__ src, const CcLevel& F, double* ca, double* cb,
                           const CcLevel& C) {
        cc_map(C, ca, cb, [&](int x, int y, int z, int64_t) {
            const double* c0 = src + 2 * x + (int64_t)(2 * y) * F.ldy + (int64_t)(2 * z) * F.ldz;
            double acc = 0.0;
#pragma unroll
            for (int a = -1; a <= 1; a++)
#pragma unroll
                for (int b = -1; b <= 1; b++)
#pragma unroll
                    for (int c = -1; c <= 1; c++) {
                        const double wgt = 0.125 * ((2.0 - (a < 0 ? -a : a)) / 2.0) *
                                           ((2.0 - (b < 0 ? -b : b)) / 2.0) * ((2.0 - (c < 0 ? -c : c)) / 2.0);
                        acc += wgt * c0[a + b * F.ldy + c * F.ldz];
                    }
            return acc;
        });
    };

    // ---- down: pre-smoothing, f^2h = R(f - A v) [FAS: restV = v^2h = R v, f^2h += A(restV)] ----
    for (int l = 0; l + 1 < P.n; l++) {
        const CcLevel &F = P.L[l], &C = P.L[l + 1];
        smooth(l, P.pre, false);
        const double* u = cur(l);
        cc_map(F, F.r, nullptr, [&](int, int, int, int64_t p) { // residual (k_generic KIND 1)
            double c, wv;
            const double a = cc_op<MODE>(F.k, u, false, F.w, p, c, wv);
            return F.f[p] - a;
        });
        __syncthreads();
        restrict_to(F.r, F, C.f, nullptr, C);
        if (MODE == GS_NONLINEAR) restrict_to(u, F, C.rv, cur(l + 1), C);
        __syncthreads();
        if (MODE == GS_NONLINEAR) { // f += A(restV)  (k_generic KIND 2, ADD)
            cc_map(C, C.f, nullptr, [&](int, int, int, int64_t p) {
                double c, wv;
                const double a = cc_op<GS_NONLINEAR>(C.k, C.rv, false, nullptr, p, c, wv);
                return C.f[p] + a;
            });
            __syncthreads();
        }
    }
    // ---- the coarsest level: pre + post sweeps (CpuSolver.cpp:117) ----
    smooth(P.n - 1, P.pre + P.post, false);
    // ---- up: v^h += P(v^2h [- restV^2h]) (k_prolong_add), post-smoothing ----
    for (int l = P.n - 1; l > 0; l--) {
        const CcLevel &C = P.L[l], &F = P.L[l - 1];
        materialize(l);
        const double* cv = cur(l);
        double* fv = cur(l - 1);
        cc_map(F, fv, nullptr, [&](int x, int y, int z, int64_t p) {
            const double e = MODE == GS_NONLINEAR ? prolong_value<true>(cv, C.rv, x, y, z, C.ldy, C.ldz, 0)
                                                  : prolong_value<false>(cv, nullptr, x, y, z, C.ldy, C.ldz, 0);
            return fv[p] + e;
        });
        __syncthreads();
        smooth(l - 1, P.post, true);
    }
}

// The launch record (gs_launch_dry_run / gs_launch_record and the transfer library's pair): every kernel launch of a
// product library goes through launch(), which notes the host function it is about to launch in a thread-local ring
// and, while the calling thread's dry-run flag is set, skips the launch and nothing else. launch_record_take resolves
// the noted functions to kernel names (hipKernelNameRefByPtr, demangled, without `(anonymous namespace)::`, the return
// type and the argument list: `k_rb<0, 0, false, ...>`), newline-separated, and clears the record.
struct LaunchRecord {
    static constexpr int CAP = 16; // a call enqueues at most two kernels; an unread record keeps the latest CAP
    const void* fn[CAP];
    int64_t n;
    bool dry;
};
thread_local LaunchRecord tlLaunches{};

template <class... P, class... A>
inline void launch(void (*fn)(P...), dim3 grid, dim3 block, hipStream_t st, A&&... args)
{
    LaunchRecord& r = tlLaunches;
    r.fn[r.n++ % LaunchRecord::CAP] = reinterpret_cast<const void*>(fn);
    if (r.dry) return;
    hipLaunchKernelGGL(fn, grid, block, 0, st, static_cast<P>(args)...);
}

// dry-run: the launchers' runtime calls that stand in for a kernel (a memset of one partial, gs_copy's memcpy) are
// skipped as a launch is, and record nothing
bool launch_dry() { return tlLaunches.dry; }

int launch_dry_run(int on)
{
    const int was = tlLaunches.dry ? 1 : 0;
    tlLaunches.dry = on != 0;
    return was;
}

int64_t launch_record_take(char* buf, int64_t cap)
{
    LaunchRecord& r = tlLaunches;
    const int64_t n = r.n < LaunchRecord::CAP ? r.n : LaunchRecord::CAP;
    std::string out;
    for (int64_t i = r.n - n; i < r.n; i++) {
        const void* fn = r.fn[i % LaunchRecord::CAP];
        const char* mangled = fn ? hipKernelNameRefByPtr(fn, nullptr) : nullptr;
        std::string name = mangled ? mangled : "?";
        int status = -1;
        char* d = mangled ? abi::__cxa_demangle(mangled, nullptr, nullptr, &status) : nullptr;
        if (d && status == 0) name = d;
        free(d);
        const std::string anon = "(anonymous namespace)::";
        for (size_t p = name.find(anon); p != std::string::npos; p = name.find(anon)) name.erase(p, anon.size());
        if (name.compare(0, 5, "void ") == 0) name.erase(0, 5);
        // the argument list: from the first '(' outside the template arguments
        int depth = 0;
        for (size_t p = 0; p < name.size(); p++) {
            if (name[p] == '<') depth++;
            else if (name[p] == '>') depth--;
            else if (name[p] == '(' && depth == 0) {
                name.erase(p);
                break;
            }
        }
        out += name;
        out += '\n';
    }
    (void)hipGetLastError(); // without a device hipKernelNameRefByPtr leaves hipErrorNoDevice behind: not the caller's
    if (!buf || cap < (int64_t)out.size() + 1) return -1; // (the record is kept)
    memcpy(buf, out.c_str(), out.size() + 1);
    r.n = 0;
    return n;
}

int launch_status()
{
    if (tlLaunches.dry) return 0; // nothing was enqueued, and no device may exist to ask
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

bool bad_level(const gs_level* L)
{
    return !L || L->nx < 0 || L->ny < 0 || L->nz < 0 || L->ldy < L->nx + 2 || L->ldz < L->ldy * (L->ny + 2) ||
           L->nx > INT32_MAX / 2 || L->ny > INT32_MAX / 2 || L->nz > INT32_MAX / 2;
}

// ---------------------------------------------------------------------------------------------
// Two fused Jacobi sweeps (temporal blocking): out = S(S(v)) reading v and f once and writing once
// (24 B per two lattice updates instead of 48). Wavefront along z: at step z the block computes
// sweep 1 at plane z — rows y0-1..y0+RY, i.e. one recomputed halo row per side — and sweep 2 at
// plane z-1 for rows y0..y0+RY-1. A block spans the whole x-row: WX waves of 128 columns whose
// outside columns (of v, and of the sweep-1 values) come from the neighbour waves through LDS, so
// nothing is recomputed along x. Where a sweep-1 point is a level boundary (x or y index 0 / n+1,
// z index 0 / nz+1 unless zlo / zhi says that side is an internal Z-slab boundary whose two ghost
// planes are current) its value is the boundary value itself, exactly as a stored sweep would leave
// it. Per point the arithmetic is the single sweep's, so the result is bit-identical to two
// gs_jacobi_sweep calls.
//
// The kernel ("tb2y") has two wave-rows per block: the block is WX waves along x (the whole row)
// times 2 waves along y; the y-wave 0 owns output rows y0..y0+RY-1, the y-wave 1 rows
// y0+RY..y0+2RY-1. Between the two, the rows they need of each other (v of plane z and sweep-1 of
// plane z-1 at the shared edge) pass through LDS instead of being re-read and recomputed, so a block
// of 2RY output rows recomputes only ONE sweep-1 halo row per side and reads v rows y0-2..y0+2RY+1,
// f rows y0-1..y0+2RY: v 1 + 4/(2RY), f 1 + 2/(2RY) times the compulsory bytes before any L2 reuse
// (blocks of one y-wave: 1 + 4/RY and 1 + 2/RY).
// Both y-waves run the same code on a local row index j = -1..RY+1: wave 0 maps j to y0-1+j, wave 1
// to the mirror image y0+2RY-j, so for both j = 0 is the recomputed halo row, j = 1..RY the own rows,
// j = RY the row published to the other wave, j = RY+1 the row received from it and j = -1 the one
// halo row of v loaded from memory. On wave 1 local j+1 is global y-1: the two y-neighbours are
// swapped back before the stencil sum, which keeps the reference's term order.
// PRO = 1 / 2: the input iterate is v + P(c) / v + P(c - sub) — the prolongation and correction of
// the V-cycle's up-leg (CpuSolver.cpp:121-132, gs_prolong_add) fused into the first post-smoothing
// pair, so the corrected iterate is never stored. The correction is added to every v value when it
// is consumed (the loads stay in flight as before): X-pass values of the two coarse planes under the
// current fine planes live in registers (W0, W1) and the next coarse plane is prefetched one step
// ahead; the z-chunk is even, so every fine plane's parity, hence its Y/Z combination, is static.
//
// XH (rows of more than 2 * WAVE * WX points): the row is split into column blocks of 2 * WAVE * WX
// points, one per block. The column just outside a block edge that is interior belongs to the
// neighbouring block; the edge wave computes what its LDS slot would hold there itself: v of plane z at
// that column (loads) and sweep 1 of plane z-1 at that column, evaluated lane-parallel one local row per
// lane (lane j <-> local row j, y-neighbours by lane shifts, x-neighbours loaded) with the same point
// expression, so every output is bit-identical to two gs_jacobi_sweep calls.
// TS (diagnostics only, gs_debug_pair_timestamps): es is a buffer of 4 doubles per tile that receives the
// block's start and end wall clock (100 MHz), its hardware block index and its HW_ID register
// WPE: waves per SIMD the register allocation must allow (0: the default, one; 4: <= 128 VGPRs, two 8-wave blocks per CU)
// FX (r06): every lane's two points lie inside the row (the host launches it where nx is a whole number of 128-point
// waves, 512-point column blocks for XH): the per-lane range selects of the new values, the norm partials and the stores
// fold away — the same values from fewer VALU instructions per step
template <int MODE, int RY, int WXMAX, bool NT, bool NTF = false, bool ZV = false, bool SPEC = false, int PRO = 0,
          int PFD = 1, bool XH = false, bool UN = false, bool TS = false, int WPE = 0, bool FX = false>
__global__ __launch_bounds__(WAVE* WXMAX * 2, WPE > 0 ? WPE : 1) void k_tb2y(Coef k, const double* __restrict__ v,
                                                           const double* __restrict__ f, const double* __restrict__ w,
                                                           double* __restrict__ out, double* __restrict__ partials,
                                                           int nx, int ny, int nz, int64_t ldy, int64_t ldz, int ZC,
                                                           int zlo, int zhi, const double* __restrict__ pc,
                                                           const double* __restrict__ ps, int cnx, int cny, int cnz,
                                                           int64_t cldy, int64_t cldz, const double* __restrict__ es)
{
    static_assert(PRO == 0 || (SPEC && !ZV && RY % 2 == 0), "fused prolongation: per-wave code, even RY");
    static_assert(!TS || (PRO == 0 && !XH), "timestamps: plain pairs (es carries the buffer)");
    const uint64_t tstart = TS ? wall_clock64() : 0;
    static_assert(!XH || ((PRO == 0 || MODE == GS_LINEAR || newtonish(MODE)) && RY + 2 <= WAVE),
                  "column blocks: every pair, LINEAR / NEWTON prolongation pairs");
    constexpr int NV = RY + 1;  // sweep-1 rows j = 0..RY
    constexpr int NE = NV + RY; // x-edge values per wave side: v rows 0..RY, sweep-1 rows 1..RY
    __shared__ double red[2 * WXMAX];
    // x-edges: [parity][y-wave][1 + x-wave][side][value]; x-wave slots 0 and WX+1 are the zero
    // x-boundary columns (the reference's homogeneous Dirichlet boundary)
    __shared__ double edge[2][2][WXMAX + 2][2][NE];
    // y-edge rows: [parity][y-wave][x-wave][v | sweep-1][lane]
    __shared__ double2 yrow[2][2][WXMAX][2][WAVE];
    const int lane = threadIdx.x;
    const int wy = __builtin_amdgcn_readfirstlane(threadIdx.z);
    const int WX = blockDim.y;
    // XH (Coef::swz): the mirrored y-wave row runs its x-waves rotated by two, so that the two waves a SIMD
    // hosts (hardware wave i -> SIMD i mod 4) are never both edge waves (the edge column's extra work)
    // (not in the prolongation pairs: there the rotation costs the LINEAR column-block form 3 VGPRs, 8-12 B
    // spilled per lane, where it fits 253 without)
    const int wx = __builtin_amdgcn_readfirstlane(XH && PRO == 0 && k.swz && wy && WX == 4 ? (threadIdx.y + 2) & 3
                                                                                            : threadIdx.y);
    const int tid = threadIdx.x + WAVE * (threadIdx.y + WX * threadIdx.z);
    for (int i = tid; i < 2 * 2 * (WXMAX + 2) * 2 * NE; i += WAVE * WX * 2) (&edge[0][0][0][0][0])[i] = 0.0;
    __syncthreads();
    const int64_t tile = xcd_tile(blockIdx.x + (int64_t)gridDim.x * blockIdx.y, (int64_t)gridDim.x * gridDim.y);
    // XH: column blocks fastest (the two edges a pair of neighbours share are read on one XCD)
    const int BW = 2 * WAVE * WX; // columns per block
    const int nh = XH ? (nx + BW - 1) / BW : 1;
    const int hx = XH ? (int)((tile % gridDim.x) % nh) : 0;
    const int xb = 1 + hx * BW;
    const int x0 = xb + wx * (2 * WAVE);
    const int x = x0 + 2 * lane;
    const int xl = min(x, nx + 1);
    const bool bx0 = !FX && x > nx, bx1 = !FX && x + 1 > nx;
    const bool okx0 = FX || x <= nx, okx1 = FX || x + 1 <= nx;
    const int y0 = 1 + (int)((tile % gridDim.x) / nh) * (2 * RY);
    const int zb = 1 + (int)(tile / gridDim.x) * ZC;
    const int ze = min(zb + ZC - 1, nz);
    const bool mir = wy != 0;
    auto yof = [&](int j) { return mir ? y0 + 2 * RY - j : y0 - 1 + j; };

    int64_t roff[RY + 2]; // local rows j = -1..RY at index j+1
    bool rowc[RY + 2];
#pragma unroll
    for (int j = -1; j <= RY; j++) {
        const int y = yof(j);
        roff[j + 1] = (int64_t)min(max(y, 0), ny + 1) * ldy;
        rowc[j + 1] = y >= 1 && y <= ny;
    }
    auto planeok = [&](int z) { return (z >= 1 && z <= nz) || (z == 0 && zlo) || (z == nz + 1 && zhi); };
    auto at = [&](const double* base, int j, int z) { return base + xl + roff[j + 1] + (int64_t)z * ldz; };
    // XH edge column xe (wave 0: left of the block, wave WX-1: right of it) when it is interior
    const bool eL = XH && wx == 0 && hx > 0;
    const bool eR = XH && wx == WX - 1 && xb + BW <= nx;
    const bool edg = eL || eR; // wave-uniform
    const int xe = eL ? xb - 1 : xb + BW;
    int64_t eroff = 0; // lane j <-> local row j = 0..RY+1
    bool erowc = false;
    if (XH) {
        const int y = yof(min(lane, RY + 1));
        eroff = (int64_t)min(max(y, 0), ny + 1) * ldy;
        erowc = y >= 1 && y <= ny;
    }
    auto eat = [&](const double* base, int dx, int z) { return base + (xe + dx) + eroff + (int64_t)z * ldz; };
    // XH + PRO: the edge column's corrected iterate v + P v^2h (columns xe-1..xe+1) comes from the strip
    // k_pro_strip wrote for this launch (layout there): [boundary][plane -1..nz+2][column xb-2..xb+1][row]
    const double* esr = es;
    if (XH && PRO != 0 && edg) {
        const int hb = eL ? hx - 1 : hx; // the block boundary the edge column lies at
        const int y = yof(min(lane, RY + 1));
        esr = es + (int64_t)hb * (nz + 4) * 4 * (ny + 2) + (eL ? 1 : 2) * (ny + 2) + min(max(y, 0), ny + 1);
    }
    auto sat = [&](int dx, int z) { return esr + ((int64_t)(z + 1) * 4 + dx) * (ny + 2); };

    // PFD: prefetch distance in plane steps. 1: two operand slots (this step's, the next one's in
    // flight); 2: four named slots, three live (this step's and the next two in flight), the z loop
    // unrolled by 4 so every slot index is static
    static_assert(PFD == 1 || PFD == 2, "prefetch distance 1 or 2");
    constexpr int NS = PFD == 2 ? 4 : 2, UNR = PFD == 2 ? 4 : 2;
    double2 Vp[NV], Vc[NV], VL[NS][NV], FL[NS][NV], WL[NS][NV], HL[NS];
    double2 V1p[RY], V1c[NV], Fprev[RY], Aprev[RY], Eprev[RY]; // Aprev, Eprev: NEWTON terms at z-1
    // YSH (GS_NEWTON_B plain pairs): the E slots (E = 1 there) carry the point's Jacobi reciprocal nb_recip(preFac + B),
    // formed in sweep 1 and reused by sweep 2 one plane step later — the same value, so bit-identical to nb_quot at
    // both sweeps (232-238 VGPRs, no spill): pair 0.806-0.829 vs 0.829-0.840 ms, Newton iteration 27.74-28.07 vs
    // 28.21-28.48 ms (r05t; in the prolongation pairs too: the same Newton time, 255 VGPRs, and the two-x-wave
    // instance falls to one wave per SIMD, r05s)
    // (the zero-iterate pairs too, though it costs them their third wave per SIMD: 166 -> 177 VGPRs; without them
    // 28.54-28.81 vs 28.08-28.43 ms per Newton iteration, r05u)
    // (and the four-x-wave prolongation pair, 255 VGPRs, no spill: 0.906-0.918 vs 0.935-0.943 ms per 512^3 launch,
    // Newton iteration 27.74-28.04 vs 27.99-28.25 ms, r05z; the two-x-wave instance of 256-point rows keeps
    // recomputing: at 255 VGPRs it would fall to one wave per SIMD, r05s)
    constexpr bool YSH = MODE == GS_NEWTON_B && !XH && (PRO == 0 || WXMAX > 2);
#ifdef GS_EXP_EFIELD
    double2 XL[NS][NV];
#endif
    // NEWTON with the fused prolongation: no room for Aprev / Eprev, so sweep 2 recomputes A from the
    // newtonV rows at z-1 and reads E = exp(w) from LDS (same expressions, same values)
    // NEWTON column blocks (XH) likewise: their edge-column state leaves no room for Aprev / Eprev / Fprev
    // (GS_NEWTON_B prolongation pairs keep them in registers: A = B, E = 1, 246 VGPRs without spill; 0.968-0.979 vs
    // 0.986-0.990 ms per 512^3 launch with the LDS state, profiles/r05/r05g_newton_b_norecomp_touch_ab.txt)
    constexpr bool RECOMP = newtonish(MODE) && ((PRO != 0 && MODE == GS_NEWTON) || XH);
    constexpr bool ELDS = RECOMP && MODE == GS_NEWTON; // E in LDS (GS_NEWTON_B: E = 1, A = B from wprev_l)
    constexpr bool WLDS = newtonish(MODE) && PRO != 0; // the coarse X-pass rows in LDS (prolongation pairs)
    // (Wprev, Fprev: sweep 2's newtonV / f rows at z-1, in LDS like the coarse rows below)
    __shared__ double2 wprev_l[RECOMP ? RY : 1][RECOMP ? 2 * WXMAX : 1][RECOMP ? WAVE : 1];
    __shared__ double2 fprev_l[RECOMP ? RY : 1][RECOMP ? 2 * WXMAX : 1][RECOMP ? WAVE : 1];
    // exp(w) of sweep 1's own rows, by plane parity: sweep 2 reads the previous plane's (each lane its own
    // values, no barrier) instead of evaluating exp a second time (+32 KB: 148 KB, one block per CU as before)
    __shared__ double2 eprev_l[ELDS ? 2 : 1][ELDS ? RY : 1][ELDS ? 2 * WXMAX : 1][ELDS ? WAVE : 1];
#pragma unroll
    for (int j = 0; j < NV; j++) V1c[j] = make_double2(0.0, 0.0);
#pragma unroll
    for (int j = 0; j < RY; j++) V1p[j] = make_double2(0.0, 0.0);
    // XH edge column: v at plane z+1 (EA), its x-neighbours (EXm, EXp) and f at plane z, per slot;
    // EP / EC: v at planes z-1 / z; ES1c: sweep 1 at plane z-1
    // NEWTON (EPK): the five edge values of a step share ONE register per slot: lane 8 f + r holds field f
    // (0 v or the corrected v at plane z+1, 1 / 2 its x-neighbours at plane z, 3 f, 4 newtonV) of local row r,
    // and the edge computation takes them with lane permutes. The prefetch distance stays one step, at 2
    // VGPRs per slot instead of 10 (the NEWTON column-block pairs spilled with five slot arrays)
    constexpr bool EPK = XH && newtonish(MODE);
    constexpr int NES = (XH && !EPK) ? NS : 1;
    double EA[NES], EXm[NES], EXp[NES], EF[NES], EP = 0.0, EC = 0.0, ES1c = 0.0;
    double EPS[EPK ? NS : 1]; // EPK: the packed slots
    auto load_edge = [&](const int s, const int z, const int zv) {
        if constexpr (PRO != 0) {
            EA[s] = *sat(0, zv);
            EXm[s] = *sat(-1, z);
            EXp[s] = *sat(1, z);
        } else {
            EA[s] = ldv1<ZV>(eat(v, 0, zv));
            EXm[s] = ldv1<ZV>(eat(v, -1, z));
            EXp[s] = ldv1<ZV>(eat(v, 1, z));
        }
        EF[s] = *eat(f, 0, z);
    };
    // EPK: lane 8 f + r's row offset (row r = 0..7 clamped to the edge rows 0..RY+1) and field f
    const int pfld = EPK ? lane >> 3 : 0;
    int64_t proff = 0;
    const double* psr = es;
    if constexpr (EPK) {
        const int y = yof(min(lane & 7, RY + 1));
        proff = (int64_t)min(max(y, 0), ny + 1) * ldy;
        if (PRO != 0 && edg) {
            const int hb = eL ? hx - 1 : hx;
            psr = es + (int64_t)hb * (nz + 4) * 4 * (ny + 2) + (eL ? 1 : 2) * (ny + 2) + min(max(y, 0), ny + 1);
        }
    }
    auto load_packed = [&](const int s, const int z, const int zv) {
        const int dx = pfld == 1 ? -1 : (pfld == 2 ? 1 : 0);
        const int zz = pfld == 0 ? zv : z;
        double val = 0.0;
        if (pfld <= 2) {
            if constexpr (PRO != 0) val = psr[((int64_t)(zz + 1) * 4 + dx) * (ny + 2)];
            else if constexpr (!ZV) val = v[(xe + dx) + proff + (int64_t)zz * ldz];
        } else if (pfld == 3) {
            val = f[xe + proff + (int64_t)z * ldz];
        } else if (pfld == 4) {
            val = (MODE == GS_NEWTON_B && k.bconst) ? k.gamma : w[xe + proff + (int64_t)z * ldz];
        }
        EPS[s] = val;
    };
    // field fl of this lane's edge row from packed slot s (a lane permute; every lane of the wave active)
    auto efld = [&](const int s, const int fl) { return __shfl(EPS[s], fl * 8 + (lane & 7), WAVE); };
    // GRP (LINEAR plain pairs, r06): a step's loads grouped by field and plane, rows ascending — v's halo row and rows
    // 0..RY, then f's rows — instead of row by row alternating between the two streams: pair 0.5831-0.5998 vs
    // 0.5935-0.6013 ms per 512^3 launch, 5 of 6 interleaved rounds faster (profiles/r06/r06v_pair_load_order_ab.txt,
    // r06u); the NEWTON pairs and every prolongation pair measured slower with it (r06u / r06v) and keep the row order
    constexpr bool GRP = MODE == GS_LINEAR && PRO == 0;
    auto load_slot = [&](const int s, const int z, const int zv) {
        if constexpr (GRP) {
            HL[s] = ldv2<ZV>(at(v, -1, z));
#pragma unroll
            for (int j = 0; j < NV; j++) VL[s][j] = ldv2<ZV>(at(v, j, zv));
#pragma unroll
            for (int j = 0; j < NV; j++) FL[s][j] = ld2s<NTF>(at(f, j, z));
        } else {
#pragma unroll
            for (int j = 0; j < NV; j++) {
                VL[s][j] = ldv2<ZV>(at(v, j, zv));
                FL[s][j] = ld2s<NTF>(at(f, j, z));
                if (MODE == GS_NEWTON_B && k.bconst) WL[s][j] = make_double2(k.gamma, k.gamma);
                else if (newtonish(MODE)) WL[s][j] = ld2(at(w, j, z));
#ifdef GS_EXP_EFIELD
                if (MODE == GS_NEWTON) XL[s][j] = ld2(at(w, j, z) + k.efoff);
#endif
            }
            HL[s] = ldv2<ZV>(at(v, -1, z));
        }
        if constexpr (XH && !EPK) {
            if (edg) load_edge(s, z, zv);
        }
        if constexpr (EPK) {
            if (edg) load_packed(s, z, zv);
        }
    };
#pragma unroll
    for (int j = 0; j < NV; j++) {
        Vp[j] = ldv2<ZV>(at(v, j, zb - 2));
        Vc[j] = ldv2<ZV>(at(v, j, zb - 1));
    }
    if (XH && edg) {
        EP = PRO != 0 ? *sat(0, zb - 2) : ldv1<ZV>(eat(v, 0, zb - 2));
        EC = PRO != 0 ? *sat(0, zb - 1) : ldv1<ZV>(eat(v, 0, zb - 1));
    }
    // ---- fused prolongation (PRO): coarse rows cyb .. cyb+NCR-1 lie under the wave's fine rows ----
    constexpr int NCR = RY / 2 + 2;
    // RBDPP (NEWTON column blocks, where every VGPR counts): b = c(cx+1) is the next lane's a (one DPP shift; lane
    // 63 takes the next wave's first column as a wave-uniform load), so a is clamped to cnx+1 instead of cnx —
    // the same b for every lane, a different a only for lanes past the row's end, which correct nothing
    constexpr bool RBDPP = newtonish(MODE) && XH && PRO == 1;
    const int cxl = min(x >> 1, max(RBDPP ? cnx + 1 : cnx, 0)); // the lane's coarse column (fine pair x odd, x+1 even)
    const int cxe = min((x0 >> 1) + WAVE, cnx + 1);             // RBDPP: lane 63's b column
    const int cyb = mir ? ((y0 - 1) >> 1) + RY / 2 : ((y0 - 1) >> 1) - 1;
    int64_t crow[NCR];
#pragma unroll
    for (int r = 0; r < NCR; r++) crow[r] = (int64_t)min(max(cyb + r, 0), cny + 1) * cldy;
    double2 W0[NCR], W1[NCR], Wm[NCR]; // X-pass values of coarse planes K, K+1 (Wm: K-1, first step)
    // HALF: the same rows times 0.5, the product every Y and Z pass of the reference takes of them first
    // (0.5 * fine(y-1) + 0.5 * fine(y+1) with fine(y+-1) an X-pass value; 0.5 * fine(z) + 0.5 * fine(z+2)
    // with fine(z), fine(z+2) X-pass values on even rows): formed once per coarse row instead of at every
    // fine point that reads it — the same products, so the same bits
    constexpr bool HALF = !WLDS;
    double2 H0[HALF ? NCR : 1], H1[HALF ? NCR : 1], Hm[HALF ? NCR : 1];
    // NEWTON (RECOMP): the X-pass rows of planes K, K+1 live in LDS, slot wsl / wsl^1 — each lane
    // reads back only what it wrote, so no barrier; this keeps the variant inside 256 VGPRs
    __shared__ double2 wlds[WLDS ? 2 : 1][WLDS ? 2 * WXMAX : 1][WLDS ? NCR : 1][WLDS ? WAVE : 1];
    int wsl = 0;
    const int wid_l = WLDS ? wx + WX * wy : 0;
    // coarse X-pass row r of plane slot s (0: K, 1: K+1, 2: K-1 on the first step)
    auto wget = [&](int s, int r) -> double2 {
        if (s == 2) return Wm[r];
        if constexpr (WLDS) return wlds[s ^ wsl][wid_l][r][lane];
        else return s == 0 ? W0[r] : W1[r];
    };
    auto hget = [&](int s, int r) -> double2 { return s == 2 ? Hm[HALF ? r : 0] : (s == 0 ? H0[HALF ? r : 0] : H1[HALF ? r : 0]); };
    double RA[NCR], RB[RBDPP ? 1 : NCR], RE[RBDPP ? NCR : 1], SA[NCR], SB[NCR]; // raw c (and sub) of plane K+2, in flight
    auto craw = [&](int cz) {
        // coarse planes -1 .. cnz+2 exist in the layout; only those under corrected fine planes matter
        const int64_t zp = (int64_t)min(max(cz, -1), cnz + 2) * cldz, zo = zp + cxl;
#pragma unroll
        for (int r = 0; r < NCR; r++) {
            RA[r] = pc[zo + crow[r]];
            if constexpr (RBDPP) RE[r] = pc[zp + crow[r] + cxe];
            else RB[r] = pc[zo + crow[r] + 1];
            if (PRO == 2) {
                SA[r] = ps[zo + crow[r]];
                SB[r] = ps[zo + crow[r] + 1];
            }
        }
    };
    // X pass of gs_prolong_add: e(x odd) = 0.5 a + 0.5 b, e(x+1 even) = b, a / b = c(cx) / c(cx+1)
    auto xpass = [&](int s) {
#pragma unroll
        for (int r = 0; r < NCR; r++) {
            const double a = PRO == 2 ? RA[r] - SA[r] : RA[r];
            const double b = RBDPP ? lane_from_right<true>(RA[r], RE[RBDPP ? r : 0])
                                   : (PRO == 2 ? RB[r] - SB[r] : RB[RBDPP ? 0 : r]);
            const double2 X = make_double2(0.5 * a + 0.5 * b, b);
            if constexpr (HALF) {
                const double2 Hh = make_double2(0.5 * X.x, 0.5 * X.y);
                if (s == 2) Hm[r] = Hh;
                else if (s == 0) H0[r] = Hh;
                else H1[r] = Hh;
            }
            if (s == 2) Wm[r] = X;
            else if constexpr (WLDS) wlds[s ^ wsl][wid_l][r][lane] = X;
            else if (s == 0) W0[r] = X;
            else W1[r] = X;
        }
    };
    // the correction of local row j on a plane whose coarse neighbours are Wa (and Wb when the fine
    // plane is odd), Y pass then Z pass; added where the fine point is interior
    auto correct = [&](double2& val, int j, bool zodd, bool zin, int sa, int sb, auto mirc) {
        constexpr bool M = decltype(mirc)::get();
        const int u = M ? 2 * RY + 1 - j : j + 2; // fine row = 2 (coarse base) + u
        const int ri = M ? (u >> 1) - RY / 2 : (u >> 1);
        const bool yodd = u & 1;
        auto ypass = [&](int s) {
            const double2 X0 = wget(s, ri);
            if (!yodd) return X0;
            const double2 X1 = wget(s, ri + 1);
            return make_double2(0.5 * X0.x + 0.5 * X1.x, 0.5 * X0.y + 0.5 * X1.y);
        };
        double2 e;
        if constexpr (HALF) {
            auto hsum = [](double2 p, double2 q) { return make_double2(p.x + q.x, p.y + q.y); };
            if (!zodd) {
                e = yodd ? hsum(hget(sa, ri), hget(sa, ri + 1)) : wget(sa, ri);
            } else if (!yodd) {
                e = hsum(hget(sa, ri), hget(sb, ri));
            } else {
                const double2 ea = hsum(hget(sa, ri), hget(sa, ri + 1)), eb = hsum(hget(sb, ri), hget(sb, ri + 1));
                e = make_double2(0.5 * ea.x + 0.5 * eb.x, 0.5 * ea.y + 0.5 * eb.y);
            }
        } else {
            e = ypass(sa);
            if (zodd) {
                const double2 g = ypass(sb);
                e = make_double2(0.5 * e.x + 0.5 * g.x, 0.5 * e.y + 0.5 * g.y);
            }
        }
        if (zin && rowc[j + 1]) {
            if (okx0) val.x = val.x + e.x;
            if (okx1) val.y = val.y + e.y;
        }
    };
    // a fine plane gets the correction when it is interior or a ghost plane of an internal slab side
    auto pok = [&](int p) { return (p >= 1 && p <= nz) || (zlo && p <= 0) || (zhi && p > nz); };
    if (PRO) {
        const int m0 = (zb - 1) >> 1; // zb is odd: planes zb-2 = 2 m0 - 1, zb - 1 = 2 m0
        craw(m0 - 1);
        xpass(2);
        craw(m0);
        xpass(0);
        craw(m0 + 1);
        xpass(1);
        auto pro_init = [&](auto mirc) {
#pragma unroll
            for (int j = 0; j < NV; j++) {
                correct(Vp[j], j, true, pok(zb - 2), 2, 0, mirc);
                correct(Vc[j], j, false, pok(zb - 1), 0, 0, mirc);
            }
        };
        if (mir) pro_init(BoolC<true>{});
        else pro_init(BoolC<false>{});
    }
    if (PFD == 1) {
        load_slot(1, zb - 1, zb);
    } else {
        load_slot(0, zb - 1, zb);
        load_slot(1, zb, zb + 1);
    }
    double sumsq = 0.0;
    for (int z0 = zb - 1; z0 <= ze + 1; z0 += UNR) {
#pragma unroll
        for (int ph4 = 0; ph4 < UNR; ph4++) {
            // the last two steps of a 4-step round are skipped past the chunk (uniform branch)
            if (UNR == 4 && ph4 == 2 && z0 + 2 > ze + 1) break;
            const int ph = ph4 & 1; // plane parity (z0 is even): LDS double buffers, PRO combinations
            const int z = z0 + ph4;
            const int cs = PFD == 1 ? ph ^ 1 : ph4; // slot holding this step's operands
            if (PFD == 1) load_slot(ph, min(z + 1, nz + 1), min(z + 2, nz + 2));
            else load_slot((ph4 + 2) & 3, min(z + 2, nz + 1), min(z + 3, nz + 2));
            if (PRO && ph == 0) craw((z >> 1) + 2); // consumed at the end of the next step
            // ---- publish: x-edge columns (v(z) rows 0..RY, sweep-1(z-1) rows 1..RY) and the y-edge row
            if (lane == 0) {
#pragma unroll
                for (int j = 0; j < NV; j++) edge[ph][wy][wx + 1][0][j] = Vc[j].x;
#pragma unroll
                for (int j = 1; j <= RY; j++) edge[ph][wy][wx + 1][0][NV + j - 1] = V1c[j].x;
            }
            if (lane == WAVE - 1) {
#pragma unroll
                for (int j = 0; j < NV; j++) edge[ph][wy][wx + 1][1][j] = Vc[j].y;
#pragma unroll
                for (int j = 1; j <= RY; j++) edge[ph][wy][wx + 1][1][NV + j - 1] = V1c[j].y;
            }
            yrow[ph][wy][wx][0][lane] = Vc[RY];
            yrow[ph][wy][wx][1][lane] = V1c[RY];
            // LDS-only barrier: the outstanding prefetch stays in flight across it
            GS_LDS_BARRIER(); // lgkmcnt(0), s_barrier
            double CL[NE], CR[NE];
            // VEDGE (r06: LINEAR plain and prolongation pairs on whole rows, the GS_NEWTON_B FX plain pair): the edge
            // values stay in the VGPRs the LDS broadcast read fills, and each DPP shift takes its edge as the old value
            // in place — no readfirstlane to SGPRs and no copy back to a VGPR per shift (20 fewer VALU instructions per
            // plane step, +20 VGPRs: 230 / 248 / 252, no spill). Pair 0.557-0.568 vs 0.574-0.583 ms, LINEAR prolongation
            // pair 0.652-0.661 vs 0.665-0.674 ms, Newton iteration 27.54-27.65 vs 27.65-28.04 ms (rotated rounds,
            // profiles/r06/r06ad_pair_vedge_ab.txt, r06ag_vedge_pro_newton_ab.txt); the other pairs keep them in SGPRs
            // (the extra VGPRs would spill or cost them a wave per SIMD)
            constexpr bool VEDGE = !XH && (MODE == GS_LINEAR || (MODE == GS_NEWTON_B && PRO == 0 && FX));
#pragma unroll
            for (int i = 0; i < NE; i++) { // wave-uniform: kept in SGPRs (VEDGE: VGPRs)
                if constexpr (VEDGE) {
                    CL[i] = edge[ph][wy][wx][1][i];
                    CR[i] = edge[ph][wy][wx + 2][0][i];
                } else {
                    CL[i] = uniform_d(edge[ph][wy][wx][1][i]);
                    CR[i] = uniform_d(edge[ph][wy][wx + 2][0][i]);
                }
            }
            const double2 vY = yrow[ph][wy ^ 1][wx][0][lane]; // v(z) at local row RY+1
            const double2 sY = yrow[ph][wy ^ 1][wx][1][lane]; // sweep-1(z-1) at local row RY+1
            if constexpr (XH) {
                // the edge column beyond an interior block edge: v(z) rows 0..RY, sweep-1(z-1) rows 1..RY
                if (edg) {
#pragma unroll
                    for (int i = 0; i < NE; i++) {
                        const double e = i < NV ? EC : ES1c;
                        const int ln = i < NV ? i : i - NV + 1;
                        const long long b = __double_as_longlong(e);
                        const int lo = __builtin_amdgcn_readlane((int)b, ln), hi = __builtin_amdgcn_readlane((int)(b >> 32), ln);
                        const double u = __longlong_as_double(((long long)(unsigned)hi << 32) | (unsigned)lo);
                        if (eL) CL[i] = u;
                        else CR[i] = u;
                    }
                }
            }

            // ---- the two sweeps; wave 1 (mirrored rows) runs its own copy of the code, so the swap of
            // its y-neighbours costs no selects ----
            double2 V1n[NV];
            double2 Acur[RY], Ecur[RY]; // NEWTON terms of sweep 1's own rows (-> Aprev / Eprev)
            const bool pz = planeok(z);
            double ES1n = 0.0;
            auto sweeps = [&](auto mirc) {
                const bool M = mirc.get();
                if constexpr (XH) {
                    // sweep 1 at plane z on the edge column, local row = lane (rows 1..RY are used)
                    if (edg) {
                        const double c = EC;
                        const double lm = lane_from_left<true>(EC, 0.0), lp = lane_from_right<true>(EC, 0.0);
                        const double ym = M ? lp : lm, yp = M ? lm : lp;
                        double nv;
                        // (zero iterate: q = +0 exactly, Coef::zq)
                        auto qe = [&] {
                            if constexpr (EPK) {
                                const double exm = efld(cs, 1), exq = efld(cs, 2), ea = efld(cs, 0);
                                return (ZV && k.zq) ? 0.0 : div_hh(k, stencil_sum<UN>(k, c, exq, exm, yp, ym, ea, EP));
                            } else {
                                return (ZV && k.zq) ? 0.0 : div_hh(k, stencil_sum<UN>(k, c, EXp[cs], EXm[cs], yp, ym, EA[cs], EP));
                            }
                        };
                        if constexpr (newtonish(MODE)) { // the interior rows' NEWTON expressions, exp once
                            const double we = efld(cs, 4), A = newton_A<MODE>(k, we), E = newton_E<MODE>(we);
                            const double a = newton_op(qe(), c, A, E);
                            nv = newton_update<MODE>(k, c, efld(cs, 3) - a, A, E, k.omega[0]);
                        } else {
                            const double a = op_finish<MODE>(k, qe(), c, 0.0);
                            nv = jacobi_update<MODE>(k, c, EF[cs] - a, 0.0, k.omega[0]);
                        }
                        ES1n = (!pz || !erowc) ? c : nv;
                    }
                }
                if constexpr (PRO != 0) {
                    // the corrected iterate: plane z+1 (VL) and the halo row at plane z (HL); with z0
                    // even, ph 0 has z even (z+1 odd: coarse K, K+1) and ph 1 has z odd
#pragma unroll
                    for (int j = 0; j < NV; j++)
                        correct(VL[cs][j], j, ph == 0, pok(z + 1), ph == 0 ? 0 : 1, 1, mirc);
                    correct(HL[cs], -1, ph == 1, pok(z), 0, 1, mirc);
                }
                // sweep 1 at plane z, local rows 0..RY
#pragma unroll
                for (int j = 0; j < NV; j++) {
                    const double2 c = Vc[j], zm = Vp[j], zp = VL[cs][j];
                    const double2 lm = j == 0 ? HL[cs] : Vc[j - 1], lp = j == RY ? vY : Vc[j + 1];
                    const double2 ym = M ? lp : lm, yp = M ? lm : lp;
                    double q[2];
                    if (ZV && k.zq) { // the stencil of the zero iterate over h^2: +0 exactly (Coef::zq)
                        q[0] = 0.0;
                        q[1] = 0.0;
                    } else {
                        const double xm0 = lane_from_left<true>(c.y, CL[j]);
                        const double xp1 = lane_from_right<true>(c.x, CR[j]);
                        q[0] = stencil_sum<UN>(k, c.x, c.y, xm0, yp.x, ym.x, zp.x, zm.x);
                        q[1] = stencil_sum<UN>(k, c.y, xp1, c.x, yp.y, ym.y, zp.y, zm.y);
                        div_hh_row<MODE>(k, q);
                    }
                    double a0, a1, n0, n1;
                    if constexpr (newtonish(MODE)) {
                        const double2 wv = WL[cs][j];
                        const double2 A = make_double2(newton_A<MODE>(k, wv.x), newton_A<MODE>(k, wv.y));
#ifdef GS_EXP_EFIELD
                        const double2 E = XL[cs][j];
#else
                        const double2 E = YSH ? make_double2(nb_recip(k.preFac + A.x), nb_recip(k.preFac + A.y))
                                              : make_double2(newton_E<MODE>(wv.x), newton_E<MODE>(wv.y));
#endif
                        if (!RECOMP && j >= 1) {
                            Acur[j - 1] = A;
                            Ecur[j - 1] = E;
                        }
                        if (ELDS && j >= 1) eprev_l[ph][j - 1][wx + WX * wy][lane] = E;
                        if constexpr (YSH) {
                            a0 = newton_op(q[0], c.x, A.x, 1.0);
                            a1 = newton_op(q[1], c.y, A.y, 1.0);
                            n0 = c.x + k.omega[0] * ((FL[cs][j].x - a0) * E.x);
                            n1 = c.y + k.omega[0] * ((FL[cs][j].y - a1) * E.y);
                        } else {
                            a0 = newton_op(q[0], c.x, A.x, E.x);
                            a1 = newton_op(q[1], c.y, A.y, E.y);
                            n0 = newton_update<MODE>(k, c.x, FL[cs][j].x - a0, A.x, E.x, k.omega[0]);
                            n1 = newton_update<MODE>(k, c.y, FL[cs][j].y - a1, A.y, E.y, k.omega[0]);
                        }
                    } else {
                        a0 = op_finish<MODE>(k, q[0], c.x, 0.0);
                        a1 = op_finish<MODE>(k, q[1], c.y, 0.0);
                        n0 = jacobi_update<MODE>(k, c.x, FL[cs][j].x - a0, 0.0, k.omega[0]);
                        n1 = jacobi_update<MODE>(k, c.y, FL[cs][j].y - a1, 0.0, k.omega[0]);
                    }
                    const double r0 = FL[cs][j].x - a0, r1 = FL[cs][j].y - a1;
                    if (partials && j >= 1 && z >= zb && z <= ze && rowc[j + 1]) {
                        if (okx0) sumsq += r0 * r0;
                        if (okx1) sumsq += r1 * r1;
                    }
                    const bool keep = !pz || !rowc[j + 1];
                    V1n[j] = make_double2((keep || bx0) ? c.x : n0, (keep || bx1) ? c.y : n1);
                }
                // sweep 2 at plane z-1, own rows 1..RY
                if (z - 1 >= zb && z - 1 <= ze) {
                    const int64_t zo = (int64_t)(z - 1) * ldz;
#pragma unroll
                    for (int j = 1; j <= RY; j++) {
                        const double2 c = V1c[j], zm = V1p[j - 1], zp = V1n[j];
                        const double2 lm = V1c[j - 1], lp = j == RY ? sY : V1c[j + 1];
                        const double2 ym = M ? lp : lm, yp = M ? lm : lp;
                        const double xm0 = lane_from_left<true>(c.y, CL[NV + j - 1]);
                        const double xp1 = lane_from_right<true>(c.x, CR[NV + j - 1]);
                        double q[2] = {stencil_sum<UN>(k, c.x, c.y, xm0, yp.x, ym.x, zp.x, zm.x),
                                       stencil_sum<UN>(k, c.y, xp1, c.x, yp.y, ym.y, zp.y, zm.y)};
                        div_hh_row<MODE>(k, q);
                        double o0, o1;
                        if constexpr (newtonish(MODE)) {
                            double2 A, E;
                            if constexpr (RECOMP) {
                                const double2 wv = wprev_l[j - 1][wx + WX * wy][lane];
                                A = make_double2(newton_A<MODE>(k, wv.x), newton_A<MODE>(k, wv.y));
                                if constexpr (ELDS) E = eprev_l[ph ^ 1][j - 1][wx + WX * wy][lane];
                                else E = make_double2(1.0, 1.0);
                            } else {
                                A = Aprev[j - 1];
                                E = Eprev[j - 1];
                            }
                            const double a0 = newton_op(q[0], c.x, A.x, YSH ? 1.0 : E.x);
                            const double a1 = newton_op(q[1], c.y, A.y, YSH ? 1.0 : E.y);
                            const double2 fp = RECOMP ? fprev_l[j - 1][wx + WX * wy][lane] : Fprev[j - 1];
                            if constexpr (YSH) {
                                o0 = c.x + k.omega[1] * ((fp.x - a0) * E.x);
                                o1 = c.y + k.omega[1] * ((fp.y - a1) * E.y);
                            } else {
                                o0 = newton_update<MODE>(k, c.x, fp.x - a0, A.x, E.x, k.omega[1]);
                                o1 = newton_update<MODE>(k, c.y, fp.y - a1, A.y, E.y, k.omega[1]);
                            }
                        } else {
                            const double a0 = op_finish<MODE>(k, q[0], c.x, 0.0);
                            const double a1 = op_finish<MODE>(k, q[1], c.y, 0.0);
                            o0 = jacobi_update<MODE>(k, c.x, Fprev[j - 1].x - a0, 0.0, k.omega[1]);
                            o1 = jacobi_update<MODE>(k, c.y, Fprev[j - 1].y - a1, 0.0, k.omega[1]);
                        }
                        if (yof(j) <= ny) {
                            double* qo = out + x + roff[j + 1] + zo;
                            if (okx1) st2s<NT>(qo, o0, o1);
                            else if (okx0) *qo = o0;
                        }
                    }
                }
            };
            if constexpr (!SPEC) {
                sweeps(RtBool{mir});
            } else {
                if (mir) sweeps(BoolC<true>{});
                else sweeps(BoolC<false>{});
            }
            // ---- rotate ----
#pragma unroll
            for (int j = 1; j <= RY; j++) {
                V1p[j - 1] = V1c[j];
                if (!RECOMP) Fprev[j - 1] = FL[cs][j];
                if constexpr (RECOMP) {
                    wprev_l[j - 1][wx + WX * wy][lane] = WL[cs][j];
                    fprev_l[j - 1][wx + WX * wy][lane] = FL[cs][j];
                } else if (newtonish(MODE)) {
                    Aprev[j - 1] = Acur[j - 1];
                    Eprev[j - 1] = Ecur[j - 1];
                }
            }
#pragma unroll
            for (int j = 0; j < NV; j++) {
                V1c[j] = V1n[j];
                Vp[j] = Vc[j];
                Vc[j] = VL[cs][j];
            }
            if constexpr (XH) {
                EP = EC;
                if constexpr (EPK) {
                    if (edg) EC = efld(cs, 0);
                } else {
                    EC = EA[cs];
                }
                ES1c = ES1n;
            }
            if (PRO && ph == 1) { // next step: coarse planes K+1, K+2
                if constexpr (WLDS) {
                    wsl ^= 1;
                } else {
#pragma unroll
                    for (int r = 0; r < NCR; r++) W0[r] = W1[r];
                    if constexpr (HALF) {
#pragma unroll
                        for (int r = 0; r < NCR; r++) H0[r] = H1[r];
                    }
                }
                xpass(1);
            }
        }
    }
    if (partials) {
        // fixed-order block sum: waves in (x, y) order
        sumsq = wave_sum(sumsq);
        const int wid = wx + WX * wy;
        if (lane == 0) red[wid] = sumsq;
        __syncthreads();
        if (tid == 0) {
            double t = 0.0;
            for (int i = 0; i < 2 * WX; i++) t += red[i];
            partials[tile] = t;
        }
    }
    if constexpr (TS) {
        if (tid == 0) {
            double* t = const_cast<double*>(es) + 4 * tile;
            t[0] = (double)tstart;
            t[1] = (double)wall_clock64();
            t[2] = (double)(blockIdx.x + (int64_t)gridDim.x * blockIdx.y);
            t[3] = (double)(unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 4); // HW_ID: CU / SH / SE
        }
    }
}

// Shape of the fused pair: k_tb2y, 2 y-waves of TBY_RY rows each under the 4 x-waves of a row or of a
// 512-point column block (8 waves, ~218 VGPRs: two waves per SIMD; NEWTON carries the w rows too and takes
// 2 rows per wave to stay clear of spills; measured on MI355X with tools/kbench.py --pairs: two waves
// that share a SIMD and hide each other's latency beat the lower halo overhead of 3-6 rows at one wave
// per SIMD by 20-25%).
constexpr int TBY_RY = 2, TBY_RY_NEWTON = 2, TBY_WX = 4;
// prefetch distance of k_tb2y (plane steps): LINEAR keeps two steps in flight (215 VGPRs, still two
// waves per SIMD; 0.662 vs 0.673 ms per 512^3 pair, profiles/r01m_summary.md), the other modes and
// the fused prolongation one (VGPR budget: the LINEAR prolongation pair at distance 2 spills)
constexpr int tby_pfd(int mode) { return mode == GS_LINEAR ? 2 : 1; }
// column blocks (XH): LINEAR with a real input iterate at distance 2 too (247 VGPRs, no spill)

// The fused triple ("tb3y"): three LINEAR sweeps per pass in k_tb2y's whole-row tile (4 x-waves x 2 mirrored y-waves
// x TBY_RY rows, one 8-wave block per CU, XCD-aware tile order, z-chunks of tb2_plan). At plane step z a block
// evaluates sweep 2 at plane z-1, then sweep 3 at plane z-2, which it stores, then sweep 1 at plane z+1, so a sequence
// of K sweeps takes K/3 passes over memory instead of K/2. Sweep 1 runs one plane ahead of the wavefront and last in
// the step: it reads only v and f, so the planes loaded at the top of step z-1 are first read after sweeps 2 and 3 of
// step z (about one and a half steps of flight on the same two operand slots), and its result crosses the step
// boundary (S1a = sweep 1 at plane z on entry, S1c at z-1, plane z-2 in LDS). Local rows as in k_tb2y (wave 0:
// j -> y0-1+j, wave 1 the mirror image y0+2RY-j): own rows j = 1..RY, row RY+1 received from the other y-wave through
// `yrow` (v(z+1), sweep-1(z-1), sweep-2(z-2)), rows <= 0 recomputed halo. v is loaded on rows -2..RY (row -2 at plane
// z+1 only), f on rows -1..RY; sweep 1 is evaluated on rows -1..RY, sweep 2 on rows 0..RY, sweep 3 on rows 1..RY: 9
// row evaluations per y-wave and step for 2 output rows. Loads grouped by field, one LDS-only barrier per step, the
// x-edge columns of every stage through `edge`: each row reads its two edge values where it uses them, straight into
// the VGPRs the DPP shift takes as its old operand (no readfirstlane, no copy back).
// State a lane only re-reads itself one or more steps later lives in LDS, not in registers (k_tb2y's wprev_l / fprev_l
// pattern, no barrier): the previous-plane rows of sweeps 1 / 2 and f. Sweep 1 leaves f(z+1) in the slot of the step's
// parity, where sweep 2 finds it as f(z-1) two steps later (no copy); sweep 2 hands it on to sweep 3's rows. With that
// state in registers, or with all the edge values read into VGPRs up front as the LINEAR pair keeps them, every
// instance with per-lane addresses spills.
// SA: every load and store as a wave-uniform row base on the scalar unit plus one 32-bit lane offset (sa_base above):
// no lane holds a 64-bit address, which gives 20 VGPRs back. They hold the previous-plane rows of sweeps 1 and 2 and
// sweep 3's f (S1p, S2p, F2: 7 LDS writes and 7 LDS reads of 16 B per lane and step less; f1_l stays in LDS), and
// sweep 1 is divided in one batch of its four rows. The unit-stencil instances (246 / 252 VGPRs); the general-stencil
// instance would spill 13 SGPRs to VGPR lanes and keeps SA = false, which is also what GS_T3_SADDR=0 selects (A/B).
// A chunk recomputes four prologue steps (z = zb-3 .. zb), whose stage values are formed from whatever the
// zero-initialised state gives and are never consumed by a stored value. Boundary rows, columns and planes keep the
// input value at every stage; plane addresses are clamped to 0..nz+1. Every point goes through the expressions of the
// one-sweep kernels in the same operand order, so the output is bit-identical to three gs_jacobi_sweep calls.
// Whole non-distributed levels only (no ghost-plane sides), a real input iterate, no prolongation, no norm partials.
// DB: the stencil sums of several rows are divided by h^2 in ONE batch (div_hh_mm over two rows of sweep 1, all four
// with SA, and every row of sweep 2: five (four) range branches per step instead of nine, and the rows' dependent
// chains interleave); else row by row.
// Sweep 3 is divided row by row in every instance: it is where the registers peak (both carried sweep-1
// planes, both sweep-2 planes and both load slots are live), and batched there the unit-stencil instances spill.
// Each quotient is the same value either way. The unit-stencil instances are batched (254 / 256 VGPRs with per-lane
// addresses), the general-stencil instance is not (256, its sums through stencil_sum_in_order).
// ST (the scalar-base instance for rows of whole waves, the 512^3 benchmark's): the two y-waves that share a SIMD (waves
// i and i+4, the same wx) run out of phase. wy = 0 keeps the step above. wy = 1 lags by half a step: between barriers z
// and z+1 it runs sweep 1 at plane z FIRST (the plane wy = 0 evaluated at the end of the previous interval), issues its
// loads into the slot that sweep 1 consumed, then runs sweep 2 at z-1 (its z+ operand is the sweep 1 just computed)
// and sweep 3 at z-2; so one half's load issue, load wait and store burst sit beside the other's arithmetic. Still one
// barrier per step and publish -> barrier -> read; at barrier z both halves hold sweep-1(z-1) and sweep-2(z-2) as
// before. Only the exchanged v row differs: wy = 0 publishes v(z) (its Vp), wy = 1 v(z+1) from the load slot it has not
// consumed yet. The lagging half runs its own copy of the whole z loop (`half` below): in one loop with a branch per
// step each half carries the other's state through its steps as live values, the two do not fit 256 VGPRs together,
// and loads issued on one path only turn the compiler's counted vmcnt waits into vmcnt(0) where the paths join.
// ST also hands a load slot's v rows over to the plane state with a real move (mov_fresh) and keeps f's two parity slots
// in registers (FR: 24 VGPRs, moved out of the load slot the same way; no f1_l, 49,152 B of LDS and 3 of a lane's 6
// ds_write_b128 / ds_read_b128 per step less). With plain assignments the plane state takes over the slot's registers,
// the refill lands in others, and the copies that put the loop-carried slot back on the back-edge waited for loads
// half a step old (vmcnt(4) in the lagging loop). Now every vmcnt wait of both z loops leaves the newest slot's nine
// loads in flight and the back-edge blocks hold none (tools/waits_table.py prints them; 230 VGPRs, 52,608 B LDS).
// GS_EXP_T3_FLIGHT / GS_EXP_T3_CHAIN: the two timing-only probes of the step's shape (top of this file).
#ifdef GS_EXP_T3_CHAIN
#define GS_T3_ZP(n, c) c
#else
#define GS_T3_ZP(n, c) n
#endif
template <bool UN, bool FX, bool DB, bool SA>
__global__ __launch_bounds__(WAVE* TBY_WX * 2) void k_tb3y(Coef k, const double* __restrict__ v,
                                                           const double* __restrict__ f, double* __restrict__ out,
                                                           int nx, int ny, int nz, int64_t ldy, int64_t ldz, int ZC)
{
    constexpr int MODE = GS_LINEAR, RY = TBY_RY, WXMAX = TBY_WX;
    static_assert(RY == 2, "k_tb3y: two rows per y-wave (the boundary tests below name the rows)");
    constexpr int N0 = RY + 2;       // v, f, sweep-1 rows j = -1..RY at index j+1
    constexpr int N1 = RY + 1;       // sweep-2 rows j = 0..RY at index j
    constexpr int NE = N0 + N1 + RY; // x-edge values per wave side: v rows -1..RY, sweep-1 rows 0..RY, sweep-2 rows 1..RY
    constexpr int B1 = DB ? (SA ? N0 : 2) : 1, B2 = DB ? N1 : 1, B3 = 1; // rows per division batch of sweeps 1, 2, 3
    constexpr bool RS = SA; // the previous-plane rows of sweeps 1 / 2 and sweep 3's f in registers, not in LDS
#ifdef GS_EXP_T3_SYM
    constexpr bool ST = false;
#else
    constexpr bool ST = SA && FX; // the staggered step: the mirrored y-waves (wy = 1) run half a step behind (above)
#endif
    constexpr bool FR = ST; // f's two parity slots (f1_l below) in registers, not in LDS: this instance has the room
    // x-edges: [parity][y-wave][1 + x-wave][side][value]; x-wave slots 0 and WX+1 are the zero x-boundary columns
    __shared__ double edge[2][2][WXMAX + 2][2][NE];
    // y-edge rows: [parity][y-wave][x-wave][v | sweep-1 | sweep-2][lane]
    __shared__ double2 yrow[2][2][WXMAX][3][WAVE];
    // per-lane state, [row][wave][lane]: f at planes z-1 / z (rows 0..RY) and z-2 (rows 1..RY), sweep 1 at plane z-2
    // (rows 0..RY), sweep 2 at plane z-3 (rows 1..RY)
    // (f1_l: two slots by step parity; sweep 1 writes f(z+1) into the slot sweep 2 reads two steps later. FR: in
    // registers, F1s below; the array is not referenced then and takes no LDS)
    __shared__ double2 f1_l[2][N1][2 * WXMAX][WAVE];
    __shared__ double2 f2_l[RY][2 * WXMAX][WAVE];
    __shared__ double2 s1p_l[N1][2 * WXMAX][WAVE];
    __shared__ double2 s2p_l[RY][2 * WXMAX][WAVE];
    const int lane = threadIdx.x;
    const int wy = __builtin_amdgcn_readfirstlane(threadIdx.z);
    const int WX = blockDim.y;
    const int wx = __builtin_amdgcn_readfirstlane(threadIdx.y);
    const int wid = wx + WXMAX * wy;
    const int tid = threadIdx.x + WAVE * (threadIdx.y + WX * threadIdx.z);
    for (int i = tid; i < 2 * 2 * (WXMAX + 2) * 2 * NE; i += WAVE * WX * 2) (&edge[0][0][0][0][0])[i] = 0.0;
    __syncthreads();
    const int64_t tile = xcd_tile(blockIdx.x + (int64_t)gridDim.x * blockIdx.y, (int64_t)gridDim.x * gridDim.y);
    const int x = 1 + wx * (2 * WAVE) + 2 * lane;
    const int xl = min(x, nx + 1);
    const bool bx0 = !FX && x > nx, bx1 = !FX && x + 1 > nx;
    const bool okx0 = FX || x <= nx, okx1 = FX || x + 1 <= nx;
    const int y0 = 1 + (int)(tile % gridDim.x) * (2 * RY);
    const int zb = 1 + (int)(tile / gridDim.x) * ZC;
    const int ze = min(zb + ZC - 1, nz);
    // The rest of the kernel once per half: the lagging waves (ST: the mirrored y-waves) run their own copy of the z
    // loop around the same barriers, so that neither half carries the other's state through its steps; what joins
    // the halves is the LDS protocol alone
    auto half = [&](auto lagc) {
        constexpr bool LAG = decltype(lagc)::get();
        const bool mir = LAG || (!ST && wy != 0);
        auto yof = [&](int j) { return mir ? y0 + 2 * RY - j : y0 - 1 + j; };

        int64_t roff[RY + 3]; // local rows j = -2..RY at index j+2
        bool rowc[RY + 3];
#pragma unroll
        for (int j = -2; j <= RY; j++) {
            const int y = yof(j);
            roff[j + 2] = (int64_t)min(max(y, 0), ny + 1) * ldy;
            rowc[j + 2] = y >= 1 && y <= ny;
        }
        const bool in1 = rowc[1] && rowc[2] && rowc[3] && rowc[4]; // every sweep-1 / sweep-2 row is an interior row
        const bool in2 = rowc[2] && rowc[3] && rowc[4];
        auto planeok = [&](int z) { return z >= 1 && z <= nz; };
        auto cz = [&](int z) { return min(max(z, 0), nz + 1); }; // planes below 0 / above nz+1 are never dereferenced
        auto at = [&](const double* base, int j, int z) { return base + xl + roff[j + 2] + (int64_t)z * ldz; };
        // SA: the row's base on the scalar unit, the lane's byte offset in one VGPR (sa_base above). A lane that stores
        // has x <= nx, so xl == x there and the stores take the loads' offset.
        unsigned xo = 8u * (unsigned)xl;
        auto ldrow = [&](const double* base, int j, int z) {
            if constexpr (SA) return sa_ld2(sa_base(base + roff[j + 2] + (int64_t)z * ldz), xo);
            else return ld2(at(base, j, z));
        };

        double2 Vp[N0], Vc[N0], VL[2][N0], FL[2][N0], HL[2]; // v(z), v(z+1); per slot: v(z+2), f(z+1), v(z+1) at row -2
        double2 S1a[N0], S1c[N0], S2c[N1];                   // sweep 1 at planes z and z-1, sweep 2 at plane z-2
        double2 S1p[N1], S2p[RY], F2[RY];                    // RS: sweep 1 at plane z-2, sweep 2 at plane z-3, f at plane z-2
        double2 F1s[2][N1];                                  // FR: f1_l's two slots
#pragma unroll
        for (int i = 0; i < N0; i++) S1a[i] = S1c[i] = make_double2(0.0, 0.0);
#pragma unroll
        for (int i = 0; i < N1; i++) {
            S2c[i] = make_double2(0.0, 0.0);
            if constexpr (FR) F1s[0][i] = F1s[1][i] = make_double2(0.0, 0.0);
            else f1_l[0][i][wid][lane] = f1_l[1][i][wid][lane] = make_double2(0.0, 0.0);
            if constexpr (RS) S1p[i] = make_double2(0.0, 0.0);
            else s1p_l[i][wid][lane] = make_double2(0.0, 0.0);
        }
#pragma unroll
        for (int i = 0; i < RY; i++) {
            if constexpr (RS) {
                S2p[i] = F2[i] = make_double2(0.0, 0.0);
            } else {
                f2_l[i][wid][lane] = make_double2(0.0, 0.0);
                s2p_l[i][wid][lane] = make_double2(0.0, 0.0);
            }
        }
        // a step's loads grouped by field, rows ascending (as the LINEAR plain pair, GRP)
        auto load_slot = [&](const int s, const int z, const int zv) {
            HL[s] = ldrow(v, -2, z);
#pragma unroll
            for (int i = 0; i < N0; i++) VL[s][i] = ldrow(v, i - 1, zv);
#pragma unroll
            for (int i = 0; i < N0; i++) FL[s][i] = ldrow(f, i - 1, z);
        };
        // (a lagging wave enters one plane behind and with both slots filled: its first sweep 1 consumes slot 1, the
        // second slot 0, and each refills the slot it has consumed)
        constexpr int zl = LAG ? 1 : 0;
#pragma unroll
        for (int i = 0; i < N0; i++) {
            Vp[i] = ldrow(v, i - 1, cz(zb - 3 - zl));
            Vc[i] = ldrow(v, i - 1, cz(zb - 2 - zl));
        }
        // (the scheduling fences keep the row bases of the prologue's 26 loads from being formed all at once: together
        // they do not fit the SGPRs)
        if constexpr (ST) __builtin_amdgcn_sched_barrier(0);
        load_slot(1, cz(zb - 2 - zl), cz(zb - 1 - zl));
        if constexpr (LAG) {
            __builtin_amdgcn_sched_barrier(0);
            load_slot(0, cz(zb - 1 - zl), cz(zb - zl));
        }
        // The lagging half is also the younger half of the block (waves 4-7), which loses the VALU arbitration against its
        // SIMD partner at equal priority (priority first, then age), and its sweep 1 -> sweep 2 chain is the longer one:
        // one static priority raise, no flips inside the loop. Worth 2.4 % on top of the stagger at 512^3 and 0.5 %
        // without it (profiles/sweep3_stagger/summary.md)
        if constexpr (LAG) __builtin_amdgcn_s_setprio(1);
        for (int z0 = zb - 3; z0 <= ze + 2; z0 += 2) {
#pragma unroll
            for (int ph = 0; ph < 2; ph++) {
                const int z = z0 + ph; // (a step past ze+2 loads clamped planes and stores nothing)
                const int cs = ph ^ 1; // slot holding this step's operands
                if constexpr (SA) xo = sa_lane(xo);
                if constexpr (!LAG) load_slot(ph, cz(z + 2), cz(z + 3));
                // ---- publish: x-edge columns of the three stages and the y-edge rows
                if (lane == 0) {
#pragma unroll
                    for (int i = 0; i < N0; i++) edge[ph][wy][wx + 1][0][i] = Vc[i].x;
#pragma unroll
                    for (int i = 0; i < N1; i++) edge[ph][wy][wx + 1][0][N0 + i] = S1c[i + 1].x;
#pragma unroll
                    for (int i = 0; i < RY; i++) edge[ph][wy][wx + 1][0][N0 + N1 + i] = S2c[i + 1].x;
                }
                if (lane == WAVE - 1) {
#pragma unroll
                    for (int i = 0; i < N0; i++) edge[ph][wy][wx + 1][1][i] = Vc[i].y;
#pragma unroll
                    for (int i = 0; i < N1; i++) edge[ph][wy][wx + 1][1][N0 + i] = S1c[i + 1].y;
#pragma unroll
                    for (int i = 0; i < RY; i++) edge[ph][wy][wx + 1][1][N0 + N1 + i] = S2c[i + 1].y;
                }
                // ST: the other half's sweep 1 runs one plane off this wave's. The leading wave hands over v(z), the
                // lagging wave v(z+1) from the slot its next sweep 1 consumes (issued more than a step ago: the counted
                // wait in front of this write leaves the newer slot's loads in flight)
                if constexpr (LAG) yrow[ph][wy][wx][0][lane] = VL[cs][N0 - 1];
                else yrow[ph][wy][wx][0][lane] = ST ? Vp[N0 - 1] : Vc[N0 - 1];
                yrow[ph][wy][wx][1][lane] = S1c[N0 - 1];
                yrow[ph][wy][wx][2][lane] = S2c[N1 - 1];
                // LDS-only barrier: the outstanding prefetch stays in flight across it
                GS_LDS_BARRIER();
                // the x-edge values of the neighbour waves: read where a row uses them (an LDS broadcast read straight into
                // the VGPRs the DPP shift takes as its old operand; all NE pairs read up front spill)
                const double* const CL = edge[ph][wy][wx][1];
                const double* const CR = edge[ph][wy][wx + 2][0];
                // local row RY+1 of v(z+1) (a lagging wave: v(z)), sweep-1(z-1) and sweep-2(z-2): read here, ahead of their
                // use (read by the sweep that uses them the staggered step is 7 % slower); the general-stencil instance
                // reads each where it is used, up front it spills 2 VGPRs
                constexpr bool YL = !UN;
                const double2(&YR)[3][WAVE] = yrow[ph][wy ^ 1][wx];
                double2 vY, s1Y, s2Y;
                if constexpr (!YL) vY = YR[0][lane], s1Y = YR[1][lane], s2Y = YR[2][lane];

                // one row of one stage in two halves around the division: the stencil sums of the lane's two points from
                // the row's centre, its y- and z-neighbour rows and the x-edge values of the wave; then the new values
                auto row_sums = [&](auto mirc, const double2 c, const double2 lm, const double2 lp, const double2 zm,
                                    const double2 zp, const double el, const double er, double& q0, double& q1) {
                    constexpr bool M = decltype(mirc)::get();
                    const double2 ym = M ? lp : lm, yp = M ? lm : lp;
                    const double xm0 = lane_from_left<true>(c.y, el);
                    const double xp1 = lane_from_right<true>(c.x, er);
                    if constexpr (UN) {
                        q0 = stencil_sum<true>(k, c.x, c.y, xm0, yp.x, ym.x, zp.x, zm.x);
                        q1 = stencil_sum<true>(k, c.y, xp1, c.x, yp.y, ym.y, zp.y, zm.y);
                    } else {
                        q0 = stencil_sum_in_order(k, c.x, c.y, xm0, yp.x, ym.x, zp.x, zm.x);
                        q1 = stencil_sum_in_order(k, c.y, xp1, c.x, yp.y, ym.y, zp.y, zm.y);
                    }
                };
                auto row_finish = [&](const double om, const double2 c, const double q0, const double q1, const double2 fv) {
                    const double a0 = op_finish<MODE>(k, q0, c.x, 0.0);
                    const double a1 = op_finish<MODE>(k, q1, c.y, 0.0);
                    return make_double2(jacobi_update<MODE>(k, c.x, fv.x - a0, 0.0, om),
                                        jacobi_update<MODE>(k, c.y, fv.y - a1, 0.0, om));
                };
                auto kept = [&](const bool keep, const double2 c, const double2 n) {
                    return make_double2((keep || bx0) ? c.x : n.x, (keep || bx1) ? c.y : n.y);
                };
                // ---- the three sweeps; wave 1 (mirrored rows) runs its own copy of the code. The keep selects run only
                // where some row, column or the plane is a boundary (a wave-uniform branch)
                // sweep 1 at plane z+1 (a lagging wave: at plane z), sweep 2 at plane z-1; F1: f at plane z-1 as sweep 2
                // read it (-> f2_l)
                double2 S1n[N0], S2n[N1], F1[N1];
                const bool pz0 = planeok(LAG ? z : z + 1), pz1 = planeok(z - 1);
                static_assert(N0 % B1 == 0 && N1 % B2 == 0 && RY % B3 == 0, "whole division batches");
                // sweep 1 at plane z+1 (z), local rows -1..RY, into S1o
                auto sweep1 = [&](auto mirc, double2(&S1o)[N0]) {
                    if constexpr (YL) vY = YR[0][lane];
#pragma unroll
                    for (int b = 0; b < N0; b += B1) {
                        double q[2 * B1];
#pragma unroll
                        for (int i = b; i < b + B1; i++)
#ifdef GS_EXP_T3_FLIGHT
                            row_sums(mirc, Vc[i], i == 0 ? Vc[1] : Vc[i - 1], i == N0 - 1 ? vY : Vc[i + 1], Vp[i], Vp[i],
                                     CL[i], CR[i], q[2 * (i - b)], q[2 * (i - b) + 1]);
#else
                            row_sums(mirc, Vc[i], i == 0 ? HL[cs] : Vc[i - 1], i == N0 - 1 ? vY : Vc[i + 1], Vp[i], VL[cs][i],
                                     CL[i], CR[i], q[2 * (i - b)], q[2 * (i - b) + 1]);
#endif
                        div_hh_mm(k, q);
#pragma unroll
                        for (int i = b; i < b + B1; i++)
#ifdef GS_EXP_T3_FLIGHT
                            S1o[i] = row_finish(k.omega[0], Vc[i], q[2 * (i - b)], q[2 * (i - b) + 1], Vp[i]);
#else
                            S1o[i] = row_finish(k.omega[0], Vc[i], q[2 * (i - b)], q[2 * (i - b) + 1], FL[cs][i]);
#endif
                    }
                    if (!FX || !pz0 || !in1) {
#pragma unroll
                        for (int i = 0; i < N0; i++) S1o[i] = kept(!pz0 || !rowc[i + 1], Vc[i], S1o[i]);
                    }
                };
                // sweep 2 at plane z-1, local rows 0..RY; a lagging wave takes its z+ operand from the sweep 1 it has just
                // run, and f(z-1) from the slot that sweep 1 wrote one step ago
                auto sweep2 = [&](auto mirc) {
                    if constexpr (YL) s1Y = YR[1][lane];
#pragma unroll
                    for (int b = 0; b < N1; b += B2) {
                        double q[2 * B2];
#pragma unroll
                        for (int i = b; i < b + B2; i++) {
                            if constexpr (FR) F1[i] = F1s[LAG ? cs : ph][i];
                            else F1[i] = f1_l[LAG ? cs : ph][i][wid][lane];
                            row_sums(mirc, S1c[i + 1], S1c[i], i == N1 - 1 ? s1Y : S1c[i + 2],
                                     RS ? S1p[i] : s1p_l[i][wid][lane],
                                     GS_T3_ZP(S1a[i + 1], S1c[i + 1]),
                                     CL[N0 + i], CR[N0 + i], q[2 * (i - b)], q[2 * (i - b) + 1]);
                        }
                        div_hh_mm(k, q);
#pragma unroll
                        for (int i = b; i < b + B2; i++)
                            S2n[i] = row_finish(k.omega[1], S1c[i + 1], q[2 * (i - b)], q[2 * (i - b) + 1], F1[i]);
                    }
                    if (!FX || !pz1 || !in2) {
#pragma unroll
                        for (int i = 0; i < N1; i++) S2n[i] = kept(!pz1 || !rowc[i + 2], S1c[i + 1], S2n[i]);
                    }
                };
                // sweep 3 at plane z-2, own rows 1..RY
                auto sweep3 = [&](auto mirc) {
                    if (z - 2 >= zb && z - 2 <= ze) {
                        if constexpr (YL) s2Y = YR[2][lane];
                        const int64_t zo = (int64_t)(z - 2) * ldz;
#pragma unroll
                        for (int b = 1; b <= RY; b += B3) {
                            double q[2 * B3];
                            double2 fv[B3];
#pragma unroll
                            for (int j = b; j < b + B3; j++) {
                                fv[j - b] = RS ? F2[j - 1] : f2_l[j - 1][wid][lane];
                                row_sums(mirc, S2c[j], S2c[j - 1], j == RY ? s2Y : S2c[j + 1],
                                         RS ? S2p[j - 1] : s2p_l[j - 1][wid][lane],
                                         GS_T3_ZP(S2n[j], S2c[j]), CL[N0 + N1 + j - 1], CR[N0 + N1 + j - 1], q[2 * (j - b)],
                                         q[2 * (j - b) + 1]);
                            }
                            div_hh_mm(k, q);
#pragma unroll
                            for (int j = b; j < b + B3; j++) {
                                const double2 o = row_finish(k.omega[2], S2c[j], q[2 * (j - b)], q[2 * (j - b) + 1], fv[j - b]);
                                if (yof(j) <= ny) {
                                    if constexpr (SA) {
                                        xo = sa_lane(xo); // (redefined in the store's own block: sa_base above)
                                        const uint64_t qb = sa_base(out + roff[j + 2] + zo);
                                        if (okx1) sa_st2nt(qb, xo, o.x, o.y);
                                        else if (okx0) sa_st1(qb, xo, o.x);
                                    } else {
                                        double* qo = out + x + roff[j + 2] + zo;
                                        if (okx1) st2s<true>(qo, o.x, o.y);
                                        else if (okx0) *qo = o.x;
                                    }
                                }
                            }
                        }
                    }
                };
                // ---- rotate the state of sweeps 2 and 3 (each lane's LDS rows are read by this lane alone) ...
                auto rotate23 = [&] {
#pragma unroll
                    for (int j = 1; j <= RY; j++) {
                        if constexpr (RS) {
                            S2p[j - 1] = S2c[j];
                            F2[j - 1] = F1[j];
                        } else {
                            s2p_l[j - 1][wid][lane] = S2c[j];
                            f2_l[j - 1][wid][lane] = F1[j];
                        }
                    }
#pragma unroll
                    for (int i = 0; i < N1; i++) {
                        S2c[i] = S2n[i];
                        if constexpr (RS) S1p[i] = S1c[i + 1];
                        else s1p_l[i][wid][lane] = S1c[i + 1];
                    }
#pragma unroll
                    for (int i = 0; i < N0; i++) S1c[i] = S1a[i];
                };
                // ---- ... and of sweep 1: f into the slot sweep 2 reads, v one plane on
                auto rotate1 = [&] {
#pragma unroll
                    for (int i = 0; i < N1; i++) {
                        if constexpr (FR) F1s[ph][i] = mov_fresh(FL[cs][i + 1]); // (a real move, as v's below)
                        else f1_l[ph][i][wid][lane] = FL[cs][i + 1];
                    }
#pragma unroll
                    for (int i = 0; i < N0; i++) {
                        Vp[i] = Vc[i];
                        // (ST: a real move. The slot keeps its registers from one iteration to the next, its refill
                        // writes them, and nothing reads them before the refill's first consumer, so no copy on the
                        // back-edge waits for loads in flight. The other instances are at the register limit and keep
                        // the assignment, `if constexpr` so that their code is the same to the instruction)
                        if constexpr (ST) Vc[i] = mov_fresh(VL[cs][i]);
                        else Vc[i] = VL[cs][i];
                    }
                };
                if constexpr (LAG) {
                    // the lagging half: sweep 1 first (the plane the leading half evaluated at the end of the previous
                    // step; its result is sweep 2's z+ operand at once), then the loads into the slot it has just
                    // consumed, then sweeps 2 and 3
                    sweep1(BoolC<true>{}, S1a);
                    rotate1();
                    load_slot(cs, cz(z + 2), cz(z + 3));
                    sweep2(BoolC<true>{}), sweep3(BoolC<true>{});
                    rotate23();
                } else {
                    if (mir) sweep2(BoolC<true>{}), sweep3(BoolC<true>{});
                    else sweep2(BoolC<false>{}), sweep3(BoolC<false>{});
                    rotate23();
                    // sweep 1 last: it reads only v and f, the second, independent chain of the step
                    if (mir) sweep1(BoolC<true>{}, S1n);
                    else sweep1(BoolC<false>{}, S1n);
#pragma unroll
                    for (int i = 0; i < N0; i++) S1a[i] = S1n[i];
                    rotate1();
                }
            }
        }
    };
    if constexpr (ST) {
        if (wy != 0) half(BoolC<true>{});
        else half(BoolC<false>{});
    } else {
        half(BoolC<false>{});
    }
}

// Run-time selectors as compile-time constants, for the launchers' choice of a kernel instance:
// with_bools(f, b...) calls f(std::bool_constant<b>{}...), with_mode(f, mode, b...) the same behind the mode's
// std::integral_constant (mode: a base mode the caller has range-checked). f is a generic lambda that names the
// instance; a combination that has no instance is excluded there with `if constexpr`, so none is built for it.
template <class F>
auto with_bools(F&& f)
{
    return f();
}
template <class F, class... B>
auto with_bools(F&& f, bool b, B... bs)
{
    return b ? with_bools([&](auto... c) { return f(std::true_type{}, c...); }, bs...)
             : with_bools([&](auto... c) { return f(std::false_type{}, c...); }, bs...);
}
template <class F, class... B>
auto with_mode(F&& f, int mode, B... bs)
{
    if (mode == GS_LINEAR)
        return with_bools([&](auto... c) { return f(std::integral_constant<int, GS_LINEAR>{}, c...); }, bs...);
    if (mode == GS_NONLINEAR)
        return with_bools([&](auto... c) { return f(std::integral_constant<int, GS_NONLINEAR>{}, c...); }, bs...);
    if (mode == GS_NEWTON_B)
        return with_bools([&](auto... c) { return f(std::integral_constant<int, GS_NEWTON_B>{}, c...); }, bs...);
    return with_bools([&](auto... c) { return f(std::integral_constant<int, GS_NEWTON>{}, c...); }, bs...);
}

// Blocks of `threads` threads kernel `fn` keeps resident on the whole GPU (occupancy x CUs, cached).
int64_t resident_blocks(const void* fn, int threads)
{
    static std::mutex m;
    static std::map<std::pair<const void*, int>, int64_t> cache;
    std::lock_guard<std::mutex> lk(m);
    const auto key = std::make_pair(fn, threads);
    auto it = cache.find(key);
    if (it != cache.end()) return it->second;
    int per = 0, dev = 0, cus = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, fn, threads, 0) != hipSuccess || per < 1) per = 1;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1)
        cus = 256;
    (void)hipGetLastError();
    return cache[key] = (int64_t)per * cus;
}

// Round-aware chunking for levels whose grid is a few rounds of resident blocks: the chunk length c
// in [lo, hi] (even if `even`) maximising (blocks / (rounds x capacity)) x c / (c + halo) — whole
// rounds, long chunks (each recomputes ~halo planes) — among those that still fill the GPU.
// GS_FIT_ROUNDS=0 keeps the callers' rules (A/B). Returns 0 for "keep".
int fit_chunk(int64_t tiles, int64_t planes, int64_t cap, int lo, int hi, bool even, double halo)
{
    if (!kKnobs.fitRounds || tiles < 1 || planes < 1 || cap < 1) return 0;
    double best = -1.0;
    int bc = 0;
    for (int c = lo; c <= hi; c++) {
        if (even && (c & 1)) continue;
        const int64_t blocks = tiles * ((planes + c - 1) / c);
        if (blocks < cap && bc != 0) continue; // would leave CUs idle where a shorter chunk does not
        const int64_t rounds = (blocks + cap - 1) / cap;
        const double score = (double)blocks / (double)(rounds * cap) * c / (c + halo);
        if (score > best) {
            best = score;
            bc = c;
        }
    }
    return bc;
}

// refit a plan's z-chunk (grid.y) for kernel `fn` at `threads` threads
template <class K>
void refit_chunks(K* fn, int threads, int64_t planes, int lo, int hi, bool even, double halo, int* zc, dim3* g)
{
    const int c = fit_chunk(g->x, planes, resident_blocks((const void*)fn, threads), lo, hi, even, halo);
    if (c > 0) {
        *zc = c;
        g->y = (unsigned)((planes + c - 1) / c);
    }
}

// compute units of the current device (cached per device)
int64_t device_cus()
{
    static std::mutex m;
    static std::map<int, int64_t> cache;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    std::lock_guard<std::mutex> lk(m);
    auto it = cache.find(dev);
    if (it != cache.end()) return it->second;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 256;
    (void)hipGetLastError();
    return cache[dev] = cus;
}

// Geometry rule of the fused pair: the whole x-row in one block (or, XH, one column block of 512
// points) and enough work for >= 128 blocks of 4-plane chunks; the z-chunk is then chosen for >= 1024
// blocks (4..64 planes: at 512^3, 64-plane chunks measured 5-8% faster than 32 — fewer re-read
// chunk-boundary planes). fills: 0 (impossible), 1 (possible) or 2 (possible and fills the GPU);
// colb: the k_tb2y column-block shape (XH: rows of more than 512 points, up to 2^20), else its whole-row shape.
struct PairPlan {
    int fills;
    int zc;
    dim3 grid, block;
    bool colb;
};

PairPlan tb2_plan(const gs_stencil* S, const gs_level* L, int mode = GS_LINEAR)
{
    const PairPlan none{0, 0, dim3(1), dim3(1), false};
    if (!S || !L || !canonical_order(S) || L->nx < 1 || L->ny < 1 || L->nz < 1) return none;
    const bool two = L->nx <= 2 * WAVE * TBY_WX;
    // longer rows: column blocks in every mode (NEWTON since r04: sweep 2's rows in LDS, edge values loaded
    // per step: 255 VGPRs, no spill; profiles/r04/r04i_newton_1023.txt)
    const bool colb = !two;
    if (colb && L->nx > (int64_t)1 << 20) return none;
    const int64_t nh = colb ? (L->nx + 2 * WAVE * TBY_WX - 1) / (2 * WAVE * TBY_WX) : 1;
    const int rows = 2 * (newtonish(mode) ? TBY_RY_NEWTON : TBY_RY); // output rows per block
    const int64_t tiles = (L->ny + rows - 1) / rows * nh;
    // the block count (of 4-plane chunks) from which the pair is the level's smoother: 128 takes 64^3
    // (256 blocks: ZV pair + prolongation pair 23.5 us vs 4 one-point sweeps + prolongation 24.7 us) and
    // leaves 32^3 (64 blocks: 25.2 vs 23.9 us) to the one-point kernel (rocprofv3 V-cycle traces, r02:
    // tools/rr_ab_session.sh pmb GS_PAIR_MIN_BLOCKS 512 128);
    // GS_PAIR_MIN_BLOCKS overrides it (A/B)
    const int64_t minBlocks = kKnobs.pairMinBlocks;
    const int fills = tiles * ((L->nz + 3) / 4) >= minBlocks ? 2 : 1;
    int64_t c = tiles * L->nz / 1024;
    c = c < 4 ? 4 : (c > 64 ? 64 : c);
    // levels of >= 2^26 points: chunks for ~512 blocks, up to 128 planes (one 8-wave block per CU, two
    // rounds at 512^3; fewer re-read chunk-boundary planes): 0.658 vs 0.674 ms per 512^3 pair
    // (tools/kbench.py --pairs --zc 64,96,128). GS_PAIR_BIG_CHUNKS=0 keeps the 64-plane rule (A/B).
    const bool big_chunks = kKnobs.bigChunks;
    if (big_chunks && L->nx * L->ny * L->nz >= ((int64_t)1 << 26)) {
        const int64_t b = tiles * L->nz / 512;
        c = b < 64 ? 64 : (b > 128 ? 128 : b);
        // k_tb2y shapes whose tiles fit the CUs: chunks long enough for ONE round of blocks (every
        // k_tb2y variant at this size runs one 8-wave block per CU). 512^3: 256 blocks of 256 planes,
        // pair 0.587 vs 0.602 ms, V-cycle 2.16 vs 2.18 ms (tools/ab_multi.sh; 170- and 192-plane
        // chunks, i.e. uneven rounds, are far slower). Only for plane ranges from the level's first plane
        // (z0 = 0: whole single-GPU levels): the interior launch of an overlapped Z-slab sweep keeps two
        // rounds, so that the ghost exchange running beside it (RCCL kernels on the comm stream) finds
        // free CUs halfway through instead of waiting for every block of the interior to retire.
        // GS_PAIR_ONE_ROUND=0 keeps the rule above (A/B).
        const bool one_round = kKnobs.oneRound;
        const int64_t cus = device_cus();
        if (one_round && tiles <= cus && L->z0 == 0) {
            const int64_t per = cus / tiles; // chunks per tile
            int64_t c1 = (L->nz + per - 1) / per;
            c1 += c1 & 1;
            if (c1 > c) c = c1;
        } else if (one_round && colb && tiles > cus && L->z0 == 0) {
            // more tiles than CUs (1024^3: 512 column-block tiles): chunks for four rounds of blocks where
            // that lengthens them (1024^3: 512 planes, pair 4.90 vs 5.00-5.06 ms, tools/zc_sweep.sh,
            // profiles/r02k; a 1024x1024x128 slab keeps its 128-plane chunks, 0.622 vs 0.641 ms at 64)
            const int64_t per = std::max<int64_t>(1, 4 * cus / tiles);
            int64_t c1 = (L->nz + per - 1) / per;
            c1 += c1 & 1;
            if (c1 > c) c = c1;
        }
        // plane ranges past a slab's first plane (the interior launch of an overlapped Z-slab sweep):
        // GS_SLAB_ZC-plane chunks, so that blocks retire often and the ghost exchange's kernels
        // (RCCL's need a whole SIMD's registers) find a free CU soon after they are enqueued; GS_PAIR_ZC: the
        // same for plane ranges from a level's first plane (A/B)
        const int fz = L->z0 != 0 ? kKnobs.slabZc : kKnobs.pairZc;
        if (fz > 0) c = std::max(2, fz); // >= 2: the even rounding below must not reach 0
    }
    if (kKnobs.midZc > 0 && L->z0 == 0 && L->nx * L->ny * L->nz < ((int64_t)1 << 26)) c = std::max(2, kKnobs.midZc);
    c &= ~(int64_t)1; // even: every chunk starts on an odd plane (the fused prolongation's parities)
    return PairPlan{fills, (int)c, dim3((unsigned)tiles, (unsigned)((L->nz + c - 1) / c)),
                    dim3(WAVE, colb ? (unsigned)TBY_WX : (unsigned)((L->nx + 2 * WAVE - 1) / (2 * WAVE)), 2), colb};
}

// k_tb2y's signature, and the one place that writes its argument list: kernel `fn` (an instance of the launcher's
// selector, or one of the diagnostics' variants) over plan `p`. PairOperands: what the plain pairs leave empty — the
// prolongation pairs' coarse iterate and subtrahend (from the plane under fine local plane 0), the coarse level's
// extents and pitches, and `es`, their edge-column workspace (diagnostics: the timestamp buffer).
using PairKernel = void (*)(Coef, const double*, const double*, const double*, double*, double*, int, int, int, int64_t,
                            int64_t, int, int, int, const double*, const double*, int, int, int, int64_t, int64_t,
                            const double*);
struct PairOperands {
    const double *pc, *ps;
    int cnx, cny, cnz;
    int64_t cldy, cldz;
    const double* es;
};

int launch_tb2y(PairKernel fn, const PairPlan& p, const Coef& k, const gs_level* L, const double* v_in, const double* f,
                const double* w, double* v_out, double* partials, int zlo, int zhi, hipStream_t st,
                const PairOperands& o = PairOperands{})
{
    launch(fn, p.grid, p.block, st, k, v_in, f, w, v_out, partials, (int)L->nx, (int)L->ny, (int)L->nz,
                       L->ldy, L->ldz, p.zc, zlo ? 1 : 0, zhi ? 1 : 0, o.pc, o.ps, o.cnx, o.cny, o.cnz, o.cldy, o.cldz,
                       o.es);
    return launch_status();
}

// Production shape of the register-blocked kernel (chosen by tools/kbench.py on MI355X,
// profiles/r01a_kbench.json): 8 rows x 128 columns per wave, 2 waves per block, non-temporal f /
// output streams. The z-chunk is chosen per launch so the grid keeps >= 2048 blocks (at most 32
// planes, at least 4); a level too small for that many 4-plane chunks runs the one-point-per-thread
// kernel instead (coarse levels are latency-bound: parallelism beats register blocking there).
constexpr int RB_RY = 2, RB_W = 4, RB_ZCMAX = 32, RB_ZCMIN = 4;
constexpr bool RB_NT = true;

struct PassPlan {
    bool rb;
    int zc;
    dim3 grid;
};

PassPlan pass_plan(const gs_stencil* S, const gs_level* L)
{
    PassPlan p{false, 0, dim3(1)};
    if (!canonical_order(S)) {
        p.grid = gn_grid(L);
        return p;
    }
    const int64_t tiles = ((L->nx + 2 * WAVE - 1) / (2 * WAVE)) * ((L->ny + RB_RY * RB_W - 1) / (RB_RY * RB_W));
    if (tiles * ((L->nz + RB_ZCMIN - 1) / RB_ZCMIN) < 1024) {
        p.grid = gn_grid(L);
        return p;
    }
    int64_t zc = L->nz * tiles / 2048;
    zc = zc < RB_ZCMIN ? RB_ZCMIN : (zc > RB_ZCMAX ? RB_ZCMAX : zc);
    if (kKnobs.rbZc > 0) zc = kKnobs.rbZc + (kKnobs.rbZc & 1); // (A/B; even: the fused restriction's plane parity)
    p.rb = true;
    p.zc = (int)zc;
    p.grid = rb_grid(L, RB_RY, RB_W, p.zc);
    return p;
}

// Dispatch a stencil pass over (mode, kind) to the fast or the generic kernel.
template <int KIND, bool ADD>
int launch_pass(const gs_stencil* S, const gs_level* L, int mode, double omega, double gamma, const double* v,
                const double* f, const double* w, double* out, double* partials, hipStream_t st)
{
    // v == NULL: the zero iterate (sweeps only, not in NONLINEAR mode, whose coarse iterates are
    // restrictions, never zero)
    mode = base_mode(mode); // (GS_NEWTON_G: the one-point passes read the factor field, which holds gamma)
    if (!S || bad_level(L) || !valid_stencil(S) || (!v && (KIND != 0 || mode == GS_NONLINEAR))) return GS_EINVAL;
    if (mode < GS_LINEAR || mode > GS_NEWTON_B || (KIND == 2 && mode != GS_NONLINEAR)) return GS_EINVAL;
    if (L->nx == 0 || L->ny == 0 || L->nz == 0) return 0;
    const Coef k = make_coef(S, L, omega, gamma);
    const int nx = (int)L->nx, ny = (int)L->ny, nz = (int)L->nz;
    const PassPlan plan = pass_plan(S, L);
    if (plan.rb) {
        const dim3 g = plan.grid, b(WAVE, RB_W);
        // k_rb per (mode, zero iterate, unit stencil): the zero iterate for sweeps outside NONLINEAR, KIND 2 (the FAS
        // operator) for NONLINEAR only, as checked above
        with_mode([&](auto M, auto Z, auto U) {
            if constexpr ((!Z || (KIND == 0 && !ADD && M != GS_NONLINEAR)) && (KIND != 2 || M == GS_NONLINEAR))
                launch((k_rb<M, KIND, ADD, RB_RY, RB_W, true, RB_NT, false, false, Z, U>), g, b, st, k, v,
                                   f, w, out, partials, nx, ny, nz, L->ldy, L->ldz, plan.zc);
        }, mode, !v, k.unit);
    } else {
        const dim3 g = plan.grid, b(GN_BX, GN_BY);
        with_mode([&](auto M) {
            if constexpr (KIND != 2 || M == GS_NONLINEAR)
                launch((k_generic<M, KIND, ADD>), g, b, st, k, v, f, w, out, partials, nx, ny, nz, L->ldy,
                                   L->ldz);
        }, mode);
    }
    return launch_status();
}

} // namespace
