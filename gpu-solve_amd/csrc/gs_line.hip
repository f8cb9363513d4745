// gs_line.hip — libgpusolve_line.so: the launchers of include/gpusolve_line.h (semantics and evaluation order there).
// Its own library and header: libgpusolve_hip.so's export list and its kernels stay what they are. As in
// libgpusolve_transfer.so and libgpusolve_krylov.so, including gs_device.hpp brings two things along: that header's
// non-template kernels are compiled into this library as code objects nothing here launches, and its Knobs are read
// from the environment once, when the library is loaded. None of them steers anything here; no launcher reads the
// environment.
#include "gs_line_device.hpp"

namespace {

// the seven axis offsets once each: index of the centre, of (0,0,+1), of (0,0,-1), and the four x / y entries in
// config order; false for any other set
struct ZlShape {
    int c, up, lo, xy[4];
};
bool zl_shape(const gs_stencil* S, ZlShape* out)
{
    ZlShape z{-1, -1, -1, {-1, -1, -1, -1}};
    int nxy = 0;
    bool seen[7] = {};
    for (int i = 0; i < 7; i++) {
        const int ox = S->ox[i], oy = S->oy[i], oz = S->oz[i];
        if (ox < -1 || ox > 1 || oy < -1 || oy > 1 || oz < -1 || oz > 1) return false;
        if ((ox != 0) + (oy != 0) + (oz != 0) > 1) return false; // a diagonal offset
        // 0: centre, 1 / 2: +-x, 3 / 4: +-y, 5 / 6: +-z
        const int id = ox ? (ox > 0 ? 1 : 2) : oy ? (oy > 0 ? 3 : 4) : oz ? (oz > 0 ? 5 : 6) : 0;
        if (seen[id]) return false; // a repeated offset
        seen[id] = true;
        if (id == 0) z.c = i;
        else if (id == 5) z.up = i;
        else if (id == 6) z.lo = i;
        else z.xy[nxy++] = i;
    }
    *out = z;
    return true;
}

bool zl_supported(const gs_stencil* S, ZlShape* z)
{
    if (!S || !zl_shape(S, z)) return false;
    const double s0 = S->s[z->c], up = S->s[z->up], lo = S->s[z->lo];
    return s0 != 0.0 && std::fabs(s0) >= std::fabs(up) + std::fabs(lo); // (false for a NaN)
}

// whole levels only; the kernels index planes with 32-bit z
bool bad_line_level(const gs_level* L) { return bad_level(L) || L->z0 != 0; }
bool empty_level(const gs_level* L) { return L->nx == 0 || L->ny == 0 || L->nz == 0; }

// the padded boxes [a, a + span) and [b, b + span) share a word
bool overlap(const gs_level* L, const double* a, const double* b)
{
    const int64_t span = (L->nz + 2) * L->ldz;
    return a < b + span && b < a + span;
}

// the marching instance: canonical order (its x / y operands come from registers and lane shifts) from 32 * 32 columns
// on. Its ring of loads in flight matters more than full waves on the coarse levels, which are load latency times
// 2 nz steps: with the threshold at 128 * 128 the 127^3 and 63^3 levels made a 255^3 cycle 2.11 ms
constexpr int64_t ZL_MARCH_COLUMNS = 32 * 32;
// the LDS instance: below that column count, in any order, where the planes fit its static array (ZF_MAX_NZ) and are
// enough to pay for its two barriers (ZF_MIN_NZ). Such a level is 2 nz dependent global loads in k_zline_col, a
// fraction of one CU's lanes wide: five of them were 9.6 of a 15.4 ms XY cycle at 511^3
struct ZlPlan {
    bool march, lds;
    dim3 grid;
    bool ok; // the grid is launchable
};
ZlPlan zl_plan(const gs_stencil* S, const gs_level* L)
{
    const int64_t columns = L->nx * L->ny;
    ZlPlan p{canonical_order(S) && columns >= ZL_MARCH_COLUMNS, false, dim3(1), true};
    p.lds = columns < ZL_MARCH_COLUMNS && L->nz >= ZF_MIN_NZ && L->nz <= ZF_MAX_NZ;
    if (p.lds) {
        p.grid = dim3((unsigned)((columns + ZF_CB - 1) / ZF_CB)); // at most 128 blocks
    } else if (p.march) {
        const int64_t nb = ((L->nx + 2 * WAVE - 1) / (2 * WAVE)) * ((L->ny + ZL_W - 1) / ZL_W);
        p.ok = nb <= INT32_MAX;
        p.grid = dim3((unsigned)nb);
    } else {
        const int64_t gx = (L->nx + GN_BX - 1) / GN_BX, gy = (L->ny + GN_BY - 1) / GN_BY;
        p.ok = gy <= 65535;
        p.grid = dim3((unsigned)gx, (unsigned)gy);
    }
    return p;
}

} // namespace

extern "C" {

int gs_zline_supported(const gs_stencil* S)
{
    ZlShape z;
    return zl_supported(S, &z) ? 1 : 0;
}

int gs_zline_factors(const gs_stencil* S, int64_t nz, double* cp, double* den)
{
    ZlShape z;
    if (!zl_supported(S, &z) || nz < 0 || !cp || !den) return GS_EINVAL;
    const double s0 = S->s[z.c], up = S->s[z.up], lo = S->s[z.lo];
    cp[0] = den[0] = 0.0;
    cp[nz + 1] = den[nz + 1] = 0.0;
    double dk = s0; // den[1]
    for (int64_t k = 1; k <= nz; k++) {
        den[k] = dk;
        cp[k] = up / dk;
        const double t = lo * cp[k];
        dk = s0 - t;
    }
    return 0;
}

const char* gs_zline_kernel(const gs_stencil* S, const gs_level* L, int zero)
{
    ZlShape z;
    if (!zl_supported(S, &z) || bad_line_level(L) || empty_level(L)) return "";
    const ZlPlan p = zl_plan(S, L);
    if (!p.ok) return "";
    if (p.lds) return zero ? "k_zline_lds<true>" : "k_zline_lds<false>";
    if (p.march) return zero ? "k_zline_march<true>" : "k_zline_march<false>";
    return zero ? "k_zline_col<true>" : "k_zline_col<false>";
}

int gs_zline_sweep(const gs_stencil* S, const gs_level* L, double omega, const double* v_in, double* v_out,
                   const double* f, const gs_zline_tables* T, hipStream_t st)
{
    ZlShape z;
    if (!zl_supported(S, &z) || bad_line_level(L) || !v_out || !f || !T || !T->cp || !T->den || T->nz != L->nz)
        return GS_EINVAL;
    if (overlap(L, v_out, f) || (v_in && overlap(L, v_out, v_in))) return GS_EINVAL;
    if (empty_level(L)) return 0;
    const ZlPlan p = zl_plan(S, L);
    if (!p.ok) return GS_EINVAL;
    ZlCoef k;
    for (int i = 0; i < 4; i++) {
        k.s[i] = S->s[z.xy[i]];
        k.off[i] = S->ox[z.xy[i]] + S->oy[z.xy[i]] * L->ldy;
    }
    k.lo = S->s[z.lo];
    k.hh = L->h * L->h;
    k.omega = omega;
    const int nx = (int)L->nx, ny = (int)L->ny, nz = (int)L->nz;
    with_bools([&](auto ZV) {
        if (p.lds)
            launch((k_zline_lds<ZV>), p.grid, dim3(ZF_T), st, k, v_in, f, v_out, T->cp, T->den, nx, ny, nz, L->ldy,
                   L->ldz);
        else if (p.march)
            launch((k_zline_march<ZV>), p.grid, dim3(WAVE, ZL_W), st, k, v_in, f, v_out, T->cp, T->den, nx, ny, nz,
                   L->ldy, L->ldz);
        else
            launch((k_zline_col<ZV>), p.grid, dim3(GN_BX, GN_BY), st, k, v_in, f, v_out, T->cp, T->den, nx, ny, nz,
                   L->ldy, L->ldz);
    }, v_in == nullptr);
    return launch_status();
}

} // extern "C"
