// gs_grid.cpp — HipGridData, HipSolver, NewtonSolver (see gs_grid.hpp).
#include "gs_grid.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <utility>

#include <hip/hip_runtime.h>

#include "gpusolve_driver.h"
#include "gpusolve_krylov.h"

namespace gs {

void check(int code, const char* what)
{
    if (code != 0) throw Error(std::string(what) + ": " + gs_strerror(code));
}

// ---------------------------------------------------------------------------------------------
DeviceField::DeviceField(int64_t nx, int64_t ny, int64_t nz, hipStream_t s, bool dry) : dry_(dry)
{
    int64_t origin = 0;
    check(gs_field_layout(nx, ny, nz, &ldy_, &ldz_, &alloc_, &origin), "gs_field_layout");
    span_ = ldz_ * (nz + 2);
    if (dry) return;
    void* p = nullptr;
    check((int)hipMalloc(&p, sizeof(double) * alloc_), "hipMalloc");
    base_ = static_cast<double*>(p);
    origin_ = base_ + origin;
    span_ = ldz_ * (nz + 2);
    zero(s);
}

DeviceField::~DeviceField()
{
    if (base_) (void)hipFree(base_);
}

DeviceField& DeviceField::operator=(DeviceField&& o) noexcept
{
    if (this != &o) {
        if (base_) (void)hipFree(base_);
        base_ = std::exchange(o.base_, nullptr);
        origin_ = std::exchange(o.origin_, nullptr);
        ldy_ = o.ldy_;
        ldz_ = o.ldz_;
        span_ = o.span_;
        alloc_ = o.alloc_;
        dry_ = o.dry_;
    }
    return *this;
}

bool HipGridData::allRanks(bool flag)
{
    if (trace || !comm_ || comm_->size() <= 1) return flag;
    const hipStream_t s = stream();
    const double on = flag ? 1.0 : 0.0;
    std::vector<double> all((std::size_t)comm_->size(), 0.0);
    check((int)hipMemcpyAsync(dNorm_, &on, sizeof(double), hipMemcpyHostToDevice, s), "hipMemcpyAsync");
    comm_->allgather1(dNorm_, dRankSums_, s);
    check((int)hipMemcpyAsync(all.data(), dRankSums_, sizeof(double) * all.size(), hipMemcpyDeviceToHost, s),
          "hipMemcpyAsync");
    comm_->sync(s);
    for (const double a : all) flag = flag && a != 0.0;
    return flag;
}

void DeviceField::zero(hipStream_t s)
{
    if (base_) check((int)hipMemsetAsync(base_, 0, sizeof(double) * alloc_, s), "hipMemsetAsync");
}

void DeviceField::swap(DeviceField& o) noexcept
{
    std::swap(base_, o.base_);
    std::swap(origin_, o.origin_);
    std::swap(ldy_, o.ldy_);
    std::swap(ldz_, o.ldz_);
    std::swap(span_, o.span_);
    std::swap(alloc_, o.alloc_);
    std::swap(dry_, o.dry_);
}

DeviceBuf::~DeviceBuf()
{
    if (p_) (void)hipFree(p_);
}

double* DeviceBuf::get(int64_t elems)
{
    if (elems <= n_) return p_;
    if (p_) check((int)hipFree(p_), "hipFree");
    p_ = nullptr;
    n_ = 0;
    void* q = nullptr;
    check((int)hipMalloc(&q, sizeof(double) * (size_t)elems), "hipMalloc(workspace)");
    p_ = static_cast<double*>(q);
    n_ = elems;
    return p_;
}

StreamGuard::StreamGuard(bool create, bool high)
{
    if (!create) return;
    int least = 0, greatest = 0;
    if (high && hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess)
        check((int)hipStreamCreateWithPriority(&s, hipStreamNonBlocking, greatest), "hipStreamCreateWithPriority");
    else
        check((int)hipStreamCreateWithFlags(&s, hipStreamNonBlocking), "hipStreamCreate");
}
StreamGuard::~StreamGuard()
{
    if (s) (void)hipStreamDestroy(s);
}

// ---------------------------------------------------------------------------------------------
void LevelClock::mark(hipStream_t s, int level, bool begin)
{
    if (!on) return;
    const std::size_t k = segLevel.size();
    if (begin) {
        if (ev.size() < 2 * (k + 1)) {
            for (int j = 0; j < 2; j++) {
                hipEvent_t e = nullptr;
                check((int)hipEventCreate(&e), "hipEventCreate");
                ev.push_back(e);
            }
        }
        segLevel.push_back(level);
        check((int)hipEventRecord(ev[2 * k], s), "hipEventRecord");
    } else if (k > 0) {
        check((int)hipEventRecord(ev[2 * k - 1], s), "hipEventRecord");
    }
}

void LevelClock::collect()
{
    if (!on) return;
    for (std::size_t k = 0; k < segLevel.size(); k++) {
        float ms = 0.f;
        check((int)hipEventSynchronize(ev[2 * k + 1]), "hipEventSynchronize");
        check((int)hipEventElapsedTime(&ms, ev[2 * k], ev[2 * k + 1]), "hipEventElapsedTime");
        const std::size_t l = (std::size_t)segLevel[k];
        if (levelMs.size() <= l) levelMs.resize(l + 1, 0.0);
        levelMs[l] += ms;
    }
    segLevel.clear();
}

LevelClock::~LevelClock()
{
    for (hipEvent_t e : ev) (void)hipEventDestroy(e);
}

int64_t proWsElems(const HipGridData& g, std::size_t l); // below

static const char* const kTransferSingleGpu =
    "transfer: POSITION needs a single-GPU grid (not a Z-slab / RCCL or schedule-trace grid)";

// ---------------------------------------------------------------------------------------------
// Level hierarchy: L = floor(log2(min dim)) + 1, dims halve per level, h_l = 1/(ny_l+1)
// (src/cpu/CpuGridData.cpp:19-41). Fields a mode never touches are not allocated.
HipGridData::HipGridData(const GridParams& grid, Comm* comm, int64_t agglomeratePoints,
                         std::vector<std::string>* traceLog, int coarsenArg)
    : GridParams(grid), trace(traceLog), comm_(comm), stream_(traceLog == nullptr),
      // the exchange path at high priority: when the interior sweep's blocks retire, the dispatcher
      // hands the freed CUs to the boundary planes and the ghost exchange first
      commStream_(traceLog == nullptr, true), bndStream_(traceLog == nullptr && comm != nullptr && comm->size() > 1, true)
{
    const bool dry = traceLog != nullptr;
    if (std::min(std::min(gridDim[0], gridDim[1]), gridDim[2]) == 0) throw Error("grid dimensions must be positive");
    for (int i = 0; i < 7; i++) {
        stencilAbi.s[i] = stencil.values[i];
        stencilAbi.ox[i] = stencil.getXOffset(i);
        stencilAbi.oy[i] = stencil.getYOffset(i);
        stencilAbi.oz[i] = stencil.getZOffset(i);
    }
    // GS_COARSEN=xy|xyz: the coarsening where the caller leaves it open; anything else, and XY on a grid that cannot
    // take it, throws here, before any work or collective
    coarsen = coarsenArg;
    if (coarsen < 0) {
        coarsen = 0;
        if (const char* e = std::getenv("GS_COARSEN")) {
            const std::string t = e;
            if (t == "xy") coarsen = 1;
            else if (t != "xyz")
                throw Error("GS_COARSEN=" + t + ": the value must be xy or xyz");
        }
    }
    if (coarsen != 0 && coarsen != 1) throw Error("coarsen: the value must be GS_COARSEN_XYZ (0) or GS_COARSEN_XY (1)");
    if (xy()) {
        gs_stencil t;
        if (mode != LINEAR)
            throw Error("coarsen: XY needs a LINEAR grid (NONLINEAR and NEWTON semi-coarsening are not built)");
        if (nranks() > 1 || traceLog)
            throw Error("coarsen: XY needs a single-GPU grid (not a Z-slab / RCCL or schedule-trace grid: every level "
                        "keeps all planes)");
        if (gs_semi_level_stencil(&stencilAbi, 1.0, 1.0, &t) != 0)
            throw Error("coarsen: XY needs a stencil of the seven axis offsets, once each (the level stencils "
                        "re-discretise its x / y part)");
        if (std::min(gridDim[0], gridDim[1]) < 2) throw Error("coarsen: XY needs at least 2 points in x and in y");
    }
    const std::size_t mn = xy() ? std::min(gridDim[0], gridDim[1]) : std::min(std::min(gridDim[0], gridDim[1]), gridDim[2]);
    const int nlev = (int)std::floor(std::log((double)mn) / std::log(2.0)) + 1;
    levels_.resize(nlev);
    {
        auto on = [](const char* name) { return std::getenv(name) != nullptr; };
        sw.fusedSweeps = !on("GS_NO_FUSED_SWEEPS");
        sw.speculation = !on("GS_NO_SPECULATION");
        sw.fusedProlong = !on("GS_NO_FUSED_PROLONG");
        sw.fusedRR = !on("GS_NO_FUSED_RR");
        sw.zeroGuess = !on("GS_NO_ZERO_GUESS");
        sw.pipeline = !on("GS_NO_PIPELINE");
        sw.newtonFusedUpdate = !on("GS_NO_NEWTON_FUSED_UPDATE");
        sw.newtonB = !on("GS_NO_NEWTON_B");
        if (const char* e = std::getenv("GS_NEWTON_B_FUSED")) sw.newtonBFused = std::atoi(e) != 0;
        sw.newtonG = !on("GS_NO_NEWTON_G");
        if (const char* e = std::getenv("GS_NEWTON_PRO_POINTS")) sw.newtonProPoints = std::strtoll(e, nullptr, 10);
        if (const char* e = std::getenv("GS_TILE_POINTS")) sw.tilePoints = std::strtoll(e, nullptr, 10);
        if (const char* e = std::getenv("GS_HALO_ORDER")) sw.haloOrder = std::atoi(e);
        sw.sweep3 = !on("GS_NO_SWEEP3");
        if (const char* e = std::getenv("GS_SWEEP3_MIN_POINTS")) sw.sweep3MinPoints = std::strtoll(e, nullptr, 10);
        if (const char* e = std::getenv("GS_FMG")) sw.fmg = std::max(0, std::atoi(e));
        // GS_SOLVER=pcg|vcycle: what HipSolver::solve runs on a LINEAR grid; anything else throws here
        if (const char* e = std::getenv("GS_SOLVER")) {
            const std::string t = e;
            if (t == "pcg") sw.solver = 1;
            else if (t != "vcycle")
                throw Error("GS_SOLVER=" + t + ": the value must be pcg or vcycle");
        }
        // GS_OMEGAS: per-sweep relaxation weights; a malformed value or a count mismatch throws here, before any work
        if (const char* e = std::getenv("GS_OMEGAS")) weights = parseOmegas(e, preSmoothing, postSmoothing);
    }
    // GS_TRANSFER=position|reference: the grid transfers (setTransfer, once the levels exist); anything else throws here
    int transferEnv = 0;
    if (const char* e = std::getenv("GS_TRANSFER")) {
        const std::string t = e;
        if (t == "position") transferEnv = 1;
        else if (t != "reference")
            throw Error("GS_TRANSFER=" + t + ": the value must be position or reference");
    }
    if (transferEnv == 1 && (nranks() > 1 || traceLog)) throw Error(kTransferSingleGpu); // before any work or collective
    // GS_SMOOTHER=zline|jacobi: the smoother (setSmoother, once the levels exist); anything else, and zline on a grid
    // that cannot take it, throws here, before any work or collective
    int smootherEnv = 0;
    if (const char* e = std::getenv("GS_SMOOTHER")) {
        const std::string t = e;
        if (t == "zline") smootherEnv = 1;
        else if (t == "auto") smootherEnv = 2;
        else if (t != "jacobi")
            throw Error("GS_SMOOTHER=" + t + ": the value must be zline, auto or jacobi");
    }
    if (smootherEnv == 1) zlineCheck();
    if (smootherEnv == 2) zlineCheck("AUTO");
    // GS_FMG_PROLONG=position|aligned: full multigrid's prolongation (setFmgProlong, once the levels exist)
    int fmgProlongEnv = 0;
    if (const char* e = std::getenv("GS_FMG_PROLONG")) {
        const std::string t = e;
        if (t == "position") fmgProlongEnv = 1;
        else if (t != "aligned")
            throw Error("GS_FMG_PROLONG=" + t + ": the value must be position or aligned");
    }
    std::vector<int64_t> nzs, pts;
    for (int l = 0; l < nlev; l++) {
        LevelData& L = levels_[l];
        L.levelDim = l == 0 ? gridDim
                            : std::array<std::size_t, 3>{levels_[l - 1].levelDim[0] / 2, levels_[l - 1].levelDim[1] / 2,
                                                         xy() ? levels_[l - 1].levelDim[2] : levels_[l - 1].levelDim[2] / 2};
        nzs.push_back((int64_t)L.levelDim[2]);
        pts.push_back((int64_t)(L.levelDim[0] * L.levelDim[1] * L.levelDim[2]));
    }
    if (agglomeratePoints < 0) {
        const char* e = std::getenv("GS_ZSLAB_MIN_POINTS");
        agglomeratePoints = e ? std::atoll(e) : 32768;
    }
    const SlabPlan plan = planZSlabs(nzs, pts, nranks(), agglomeratePoints);

    const hipStream_t s = stream_.s;
    int64_t maxParts = 1;
    for (int l = 0; l < nlev; l++) {
        LevelData& L = levels_[l];
        const int64_t nx = (int64_t)L.levelDim[0], ny = (int64_t)L.levelDim[1];
        L.distributed = plan.distributed[l];
        L.ranksLo = plan.lo[l];
        L.ranksHi = plan.hi[l];
        if (L.distributed) {
            L.lo = plan.lo[l][rank()];
            L.hi = plan.hi[l][rank()];
        } else {
            L.lo = 1;
            L.hi = (int64_t)L.levelDim[2];
        }
        const int64_t nz = L.hi - L.lo + 1;
        L.h = 1.0 / (L.levelDim[1] + 1);
        L.v = DeviceField(nx, ny, nz, s, dry);
        L.vAlt = DeviceField(nx, ny, nz, s, dry);
        L.f = DeviceField(nx, ny, nz, s, dry);
        if (l + 1 < nlev) L.r = DeviceField(nx, ny, nz, s, dry); // restriction source
        if (mode == NONLINEAR && l > 0) L.restV = DeviceField(nx, ny, nz, s, dry);
        if (mode == NEWTON) L.newtonV = DeviceField(nx, ny, nz, s, dry);
        if (mode == NEWTON && sw.newtonB && dry) L.bfac = DeviceField(nx, ny, nz, s, dry); // (else: below)
        if (mode == NEWTON && l == 1 && nlev >= 3 && !L.distributed) L.newtonVNext = DeviceField(nx, ny, nz, s, dry);
        L.geom = gs_level{nx, ny, nz, L.v.ldy(), L.v.ldz(), L.lo - 1, L.h};
        L.sten = stencilAbi;
        if (xy()) check(gs_semi_level_stencil(&stencilAbi, levels_[0].h, L.h, &L.sten), "gs_semi_level_stencil");
        maxParts = std::max(maxParts, gs_residual_num_partials(&L.sten, &L.geom));
        maxParts = std::max(maxParts, gs_jacobi_sweep2_num_partials(&L.sten, &L.geom, (int)mode));
        L.minPlanes = nz;
        if (L.distributed)
            for (int q = 0; q < nranks(); q++) L.minPlanes = std::min(L.minPlanes, L.ranksHi[q] - L.ranksLo[q] + 1);
        // rank-uniform on a Z-slab level (the smoothing schedule decides the ghost exchanges): judged
        // on the thinnest slab, as the kernel's fill count grows with the plane count
        gs_level thin = L.geom;
        thin.nz = L.minPlanes;
        L.fusedPairs = sw.fusedSweeps && gs_jacobi_sweep2_supported_mode(&L.sten, &thin, (int)mode) == 2 &&
                       (!L.distributed || L.minPlanes >= 2);
        L.fusedTriples = sw.sweep3 && sw.fusedSweeps && mode == LINEAR && !L.distributed && pts[l] >= sw.sweep3MinPoints &&
                         gs_jacobi_sweep3_supported(&L.sten, &L.geom) == 2;
        // (the tiled steps embed the 3-D transfers: not on an XY hierarchy)
        L.tiled = !xy() && !L.distributed && pts[l] <= sw.tilePoints &&
                  gs_tiled_supported(&L.sten, &L.geom, (int)mode) != 0;
    }
    // The coarse end of the V-cycle runs as one gs_coarse_cycle launch from the first level of at
    // most GS_COARSE_POINTS points that is not Z-slab partitioned; 0 = off. Default 512 = 8^3: a 16^3
    // level costs 42 us inside the one workgroup (a single CU's L2 bandwidth: ~6 us per operator)
    // against 30 us as six chip-wide launches; from 8^3 down the launch wins (tools/ab_coarse.sh).
    coarseFrom = levels_.size();
    {
        const char* e = std::getenv("GS_COARSE_POINTS");
        const int64_t thr = e ? std::atoll(e) : 512;
        if (thr > 0 && preSmoothing + postSmoothing < (1u << 20) && !xy()) // (XY: one stencil per level, 2-D transfers)
            for (int l = nlev - 1; l >= 1; l--) {
                if (levels_[l].distributed || pts[l] > thr || nlev - l > gs_coarse_cycle_max_levels()) break;
                coarseFrom = (std::size_t)l;
            }
    }
    coarseFromRef_ = coarseFrom;
    xferT_.assign(levels_.size(), gs_transfer_tables{});
    fmgT_.assign(levels_.size(), gs_fmg_tables{});
    zlineT_.assign(levels_.size(), gs_zline_tables{});
    if (mode == NEWTON) newtonF = DeviceField(levels_[0].geom.nx, levels_[0].geom.ny, levels_[0].geom.nz, s, dry);
    newtonVZero_ = mode == NEWTON; // (every field is created zero-filled)
    {
        const char* e = std::getenv("GS_METRICS");
        clock.on = !dry && e && *e && *e != '0';
        clock.levelMs.assign(nlev, 0.0);
    }
    if (dry) {
        dryParts_.assign(16, 0.0); // the partial-sum pointers the solvers pass mark normed launches
        partials_ = dryParts_.data();
        rec("rhs", {{"L", 0}}, "f");
        halo(levels_[0], levels_[0].f, s);
        if (fmgProlongEnv) setFmgProlong(fmgProlongEnv);
        return;
    }
    // the overlapped sweep splits a level into 3 launches, each with its own partials region
    maxParts = 2 * maxParts + 4096;
    check((int)hipMalloc((void**)&partials_, sizeof(double) * maxParts), "hipMalloc(partials)");
    check((int)hipMalloc((void**)&dNorm_, sizeof(double)), "hipMalloc(norm)");
    check((int)hipMalloc((void**)&dRankSums_, sizeof(double) * nranks()), "hipMalloc(rank sums)");
    // the final norm goes straight from the finishing kernel to this pinned word (no D2H copy launch)
    check((int)hipHostMalloc((void**)&hNorm_, sizeof(double), hipHostMallocMapped | hipHostMallocCoherent),
          "hipHostMalloc");
    check((int)hipHostGetDevicePointer((void**)&hNormDev_, hNorm_, 0), "hipHostGetDevicePointer");
    check((int)hipEventCreateWithFlags(&evA_, hipEventDisableTiming), "hipEventCreate");
    check((int)hipEventCreateWithFlags(&evB_, hipEventDisableTiming), "hipEventCreate");
    check((int)hipEventCreateWithFlags(&evC_, hipEventDisableTiming), "hipEventCreate");
    for (auto& e : evBnd_) check((int)hipEventCreateWithFlags(&e, hipEventDisableTiming), "hipEventCreate");
    check((int)hipEventCreateWithFlags(&evNorm_, hipEventDisableTiming), "hipEventCreate");
    // level-0 right-hand side on the device (src/cpu/CpuGridData.cpp:44-78), h = 1/(Y+1) (main.cpp:84);
    // a slab evaluates it at its global plane indices (geom.z0)
    check(gs_rhs_init(&levels_[0].geom, levels_[0].f.data(), (int)mode, 1.0 / (gridDim[1] + 1), gamma, s),
          "gs_rhs_init");
    halo(levels_[0], levels_[0].f, s); // the fused pair's first sweep reads f on a ghost plane
    // GS_METRICS is read by each process, but the per-level clock changes the collective schedule (no
    // pipelined cycles; the last closing norm is kept): a distributed grid runs it only if EVERY rank has it
    // on, so that all ranks issue the same exchanges and collectives
    clock.on = allRanks(clock.on);
    // GS_NEWTON_B's factor fields: one more level-sized array per NEWTON level (~8.6 GB at 1023^3). If they do not
    // fit, the grid runs the reference-expression inner solves (mode 2, GS_NO_NEWTON_B) instead of failing; the
    // choice is agreed across ranks (it changes which kernels run, never the exchanges, but stays uniform)
    if (mode == NEWTON && sw.newtonB) {
        bool ok = true;
        try {
            for (auto& L : levels_) L.bfac = DeviceField(L.geom.nx, L.geom.ny, L.geom.nz, s, dry);
        } catch (const Error&) {
            ok = false;
            (void)hipGetLastError(); // (the failed hipMalloc's sticky error)
        }
        if (!allRanks(ok)) {
            sw.newtonB = false;
            for (auto& L : levels_) L.bfac = DeviceField();
        }
    }
    // the fused prolongation pair's edge-column workspaces (column-block rows), one per stream, at their
    // largest size now: proPlanes never reallocates them
    for (int l = 0; l + 1 < nlev; l++) {
        const int64_t need = proWsElems(*this, (std::size_t)l);
        if (need <= 0) continue;
        levels_[l].proWs[0].get(need);
        if (bndStream_.s) levels_[l].proWs[1].get(need);
    }
    check((int)hipStreamSynchronize(s), "hipStreamSynchronize");
    if (xy()) buildXyTables();
    if (transferEnv) setTransfer(transferEnv);
    if (fmgProlongEnv) setFmgProlong(fmgProlongEnv);
    if (smootherEnv) setSmoother(smootherEnv);
}

bool HipGridData::levelAligned(std::size_t l) const
{
    if (l + 1 >= levels_.size()) return true;
    const auto &f = levels_[l].levelDim, &c = levels_[l + 1].levelDim;
    return f[0] == 2 * c[0] + 1 && f[1] == 2 * c[1] + 1 && (xy() || f[2] == 2 * c[2] + 1);
}

// One transition's tables (gs_transfer_axis per axis) in one device allocation: per axis pt, rw, then per axis pj, rlo,
// rcnt (the doubles first, so that every array is 8-byte aligned). axes = 3: a POSITION transition; axes = 2: a
// transition of an XY hierarchy (axis 2: nf = nc = nz, no arrays).
gs_transfer_tables HipGridData::uploadTransferTables(std::size_t l, int axes)
{
    gs_transfer_tables T{};
    std::vector<std::vector<int32_t>> pj(axes), rlo(axes), rcnt(axes);
    std::vector<std::vector<double>> pt(axes), rw(axes);
    std::size_t bytes = 0;
    for (int a = 0; a < axes; a++) {
        const int64_t nf = (int64_t)levels_[l].levelDim[a], nc = (int64_t)levels_[l + 1].levelDim[a];
        T.nf[a] = nf;
        T.nc[a] = nc;
        pj[a].resize(nf + 2);
        pt[a].resize(nf + 2);
        rlo[a].resize(nc + 2);
        rcnt[a].resize(nc + 2);
        rw[a].resize(4 * (nc + 2));
        check(gs_transfer_axis(nf, nc, pj[a].data(), pt[a].data(), rlo[a].data(), rcnt[a].data(), rw[a].data()),
              "gs_transfer_axis");
        bytes += sizeof(double) * (pt[a].size() + rw[a].size()) +
                 sizeof(int32_t) * (pj[a].size() + rlo[a].size() + rcnt[a].size() + 2);
    }
    if (axes == 2) T.nf[2] = T.nc[2] = (int64_t)levels_[l].levelDim[2];
    char* base = nullptr;
    check((int)hipMalloc((void**)&base, bytes), "hipMalloc(transfer tables)");
    xferMem_.push_back(base);
    std::size_t off = 0;
    auto put = [&](const void* src, std::size_t n) {
        check((int)hipMemcpy(base + off, src, n, hipMemcpyHostToDevice), "hipMemcpy(transfer tables)");
        const void* p = base + off;
        off += n;
        return p;
    };
    for (int a = 0; a < axes; a++) {
        T.pt[a] = (const double*)put(pt[a].data(), sizeof(double) * pt[a].size());
        T.rw[a] = (const double*)put(rw[a].data(), sizeof(double) * rw[a].size());
    }
    for (int a = 0; a < axes; a++) {
        T.pj[a] = (const int32_t*)put(pj[a].data(), sizeof(int32_t) * pj[a].size());
        T.rlo[a] = (const int32_t*)put(rlo[a].data(), sizeof(int32_t) * rlo[a].size());
        T.rcnt[a] = (const int32_t*)put(rcnt[a].data(), sizeof(int32_t) * rcnt[a].size());
    }
    return T;
}

// The x / y tables of every transition of an XY hierarchy: at creation, once.
void HipGridData::buildXyTables()
{
    for (std::size_t l = 0; l + 1 < levels_.size(); l++) xferT_[l] = uploadTransferTables(l, 2);
}

void HipGridData::setTransfer(int m)
{
    if (m != 0 && m != 1) throw Error("transfer: the mode must be GS_TRANSFER_REFERENCE (0) or GS_TRANSFER_POSITION (1)");
    if (m == 1 && (nranks() > 1 || trace))
        throw Error(kTransferSingleGpu);
    const std::size_t nl = levels_.size();
    for (std::size_t l = 0; m == 1 && l + 1 < nl; l++) {
        if (levelAligned(l) || xferT_[l].pj[0]) continue;
        xferT_[l] = uploadTransferTables(l, 3);
    }
    transferMode = m;
    updateCoarseFrom();
}

// The one-launch coarse cycle embeds the index-aligned transfers and point Jacobi: in POSITION mode it starts at the
// first level, from the reference rule's on, below which every transition is aligned (none: no coarse launch); in
// ZLINE mode there is none.
void HipGridData::updateCoarseFrom()
{
    const std::size_t nl = levels_.size();
    coarseFrom = coarseFromRef_;
    if (transferMode == 1 && coarseFromRef_ < nl) {
        std::size_t c = nl - 1;
        while (c > coarseFromRef_ && levelAligned(c - 1)) c--;
        coarseFrom = c;
    }
    if (anyLine || xy()) coarseFrom = nl;
}

static const char* const kZlineStencil =
    " needs a stencil of the seven axis offsets, once each, whose centre weight s0 is "
    "not 0 and has |s0| >= |weight at (0,0,+1)| + |weight at (0,0,-1)|";

void HipGridData::zlineCheck(const char* name) const
{
    const std::string who = std::string("smoother: ") + name;
    if (mode != LINEAR)
        throw Error(who + " needs a LINEAR grid (NONLINEAR and NEWTON line sweeps are not built: their diagonal "
                          "is a field)");
    if (nranks() > 1 || trace)
        throw Error(who + " needs a single-GPU grid (not a Z-slab / RCCL or schedule-trace grid: the lines "
                          "cross the slabs)");
    // (AUTO judges every level that would run line sweeps by its own stencil: setSmoother)
    if (std::string(name) == "ZLINE" && !gs_zline_supported(&stencilAbi)) throw Error(who + kZlineStencil);
}

void HipGridData::setSmoother(int m)
{
    if (m < 0 || m > 2)
        throw Error("smoother: the mode must be GS_SMOOTHER_JACOBI (0), GS_SMOOTHER_ZLINE (1) or GS_SMOOTHER_AUTO (2)");
    const std::size_t nl = levels_.size();
    std::vector<char> want(nl, 0);
    if (m != 0) {
        zlineCheck(m == 1 ? "ZLINE" : "AUTO");
        for (std::size_t l = 0; l < nl; l++) {
            const gs_stencil& S = levels_[l].sten;
            if (m == 2) {
                // (AUTO on a grid ZLINE's shape test would refuse: no weight counts as a z weight twice; a stencil
                // with a diagonal offset has its level refused below only if the rule picks lines for it)
                double mz = 0.0, mxy = 0.0;
                for (int i = 0; i < 7; i++) {
                    if (S.ox[i] == 0 && S.oy[i] == 0 && S.oz[i] != 0) mz = std::max(mz, std::fabs(S.s[i]));
                    else if (S.ox[i] != 0 || S.oy[i] != 0) mxy = std::max(mxy, std::fabs(S.s[i]));
                }
                want[l] = mz > mxy;
            } else {
                want[l] = 1;
            }
            if (want[l] && !gs_zline_supported(&S))
                throw Error(std::string("smoother: ") + (m == 1 ? "ZLINE" : "AUTO") + kZlineStencil + " (level " +
                            std::to_string(l) + ")");
        }
        // one allocation for the line levels that have no factors yet: per level cp, then den (nz + 2 doubles each)
        std::vector<double> host;
        std::vector<std::size_t> at(nl, 0);
        for (std::size_t l = 0; l < nl; l++) {
            if (!want[l] || zlineT_[l].cp) continue;
            const auto& L = levels_[l];
            const std::size_t n = (std::size_t)L.geom.nz + 2;
            at[l] = host.size();
            host.resize(host.size() + 2 * n);
            check(gs_zline_factors(&L.sten, L.geom.nz, host.data() + at[l], host.data() + at[l] + n), "gs_zline_factors");
        }
        if (!host.empty()) {
            double* base = nullptr;
            check((int)hipMalloc((void**)&base, sizeof(double) * host.size()), "hipMalloc(z-line factors)");
            xferMem_.push_back(base);
            check((int)hipMemcpy(base, host.data(), sizeof(double) * host.size(), hipMemcpyHostToDevice),
                  "hipMemcpy(z-line factors)");
            for (std::size_t l = 0; l < nl; l++) {
                if (!want[l] || zlineT_[l].cp) continue;
                const int64_t nz = levels_[l].geom.nz;
                zlineT_[l] = gs_zline_tables{base + at[l], base + at[l] + nz + 2, nz};
            }
        }
    }
    anyLine = false;
    for (std::size_t l = 0; l < nl; l++) {
        levels_[l].line = want[l] != 0;
        anyLine = anyLine || levels_[l].line;
    }
    smootherMode = m;
    updateCoarseFrom();
}

void HipGridData::setFmgProlong(int m)
{
    if (m != 0 && m != 1)
        throw Error("fmg prolong: the mode must be GS_FMG_PROLONG_ALIGNED (0) or GS_FMG_PROLONG_POSITION (1)");
    if (m == 1) buildFmgTables();
    fmgProlongMode = m;
}

void HipGridData::buildFmgTables()
{
    if (mode == NEWTON || nranks() > 1 || trace || xy()) return; // FMG is refused there: no table is ever read
    for (std::size_t l = 0; l + 1 < levels_.size(); l++) {
        if (levelAligned(l) || fmgT_[l].cj[0]) continue;
        // one allocation per transition: per axis cw (4 (nf + 2) doubles), then per axis cj (nf + 2)
        gs_fmg_tables T{};
        std::vector<std::vector<int32_t>> cj(3);
        std::vector<std::vector<double>> cw(3);
        std::size_t bytes = 0;
        for (int a = 0; a < 3; a++) {
            const int64_t nf = (int64_t)levels_[l].levelDim[a], nc = (int64_t)levels_[l + 1].levelDim[a];
            T.nf[a] = nf;
            T.nc[a] = nc;
            cj[a].resize(nf + 2);
            cw[a].resize(4 * (nf + 2));
            check(gs_fmg_axis(nf, nc, cj[a].data(), cw[a].data()), "gs_fmg_axis");
            bytes += sizeof(double) * cw[a].size() + sizeof(int32_t) * cj[a].size();
        }
        char* base = nullptr;
        check((int)hipMalloc((void**)&base, bytes), "hipMalloc(fmg tables)");
        xferMem_.push_back(base);
        std::size_t off = 0;
        auto put = [&](const void* src, std::size_t n) {
            check((int)hipMemcpy(base + off, src, n, hipMemcpyHostToDevice), "hipMemcpy(fmg tables)");
            const void* p = base + off;
            off += n;
            return p;
        };
        for (int a = 0; a < 3; a++) T.cw[a] = (const double*)put(cw[a].data(), sizeof(double) * cw[a].size());
        for (int a = 0; a < 3; a++) T.cj[a] = (const int32_t*)put(cj[a].data(), sizeof(int32_t) * cj[a].size());
        fmgT_[l] = T;
    }
}

HipGridData::~HipGridData()
{
    if (stream_.s) (void)hipStreamSynchronize(stream_.s);
    if (commStream_.s) (void)hipStreamSynchronize(commStream_.s);
    if (bndStream_.s) (void)hipStreamSynchronize(bndStream_.s);
    for (void* p : xferMem_) (void)hipFree(p);
    if (partials_ && !trace) (void)hipFree(partials_);
    if (dNorm_) (void)hipFree(dNorm_);
    if (dRankSums_) (void)hipFree(dRankSums_);
    if (hNorm_) (void)hipHostFree(hNorm_);
    if (evA_) (void)hipEventDestroy(evA_);
    if (evB_) (void)hipEventDestroy(evB_);
    if (evC_) (void)hipEventDestroy(evC_);
    for (auto e : evBnd_)
        if (e) (void)hipEventDestroy(e);
    if (evNorm_) (void)hipEventDestroy(evNorm_);
    if (pcg.rec) (void)hipFree(pcg.rec);
    if (pcg.parts) (void)hipFree(pcg.parts);
    if (pcg.slots) (void)hipHostFree(pcg.slots);
    if (pcg.ev) (void)hipEventDestroy(pcg.ev);
}

void HipGridData::rec(const char* op, std::initializer_list<std::pair<const char*, long long>> kv, const char* field)
{
    std::string line = op;
    if (field) line += std::string(" field=") + field;
    for (const auto& p : kv) line += " " + std::string(p.first) + "=" + std::to_string(p.second);
    trace->push_back(line);
}

const char* HipGridData::fieldName(const LevelData& L, const DeviceField& f)
{
    if (&f == &L.v) return "v";
    if (&f == &L.vAlt) return "vAlt";
    if (&f == &L.f) return "f";
    if (&f == &L.r) return "r";
    if (&f == &L.restV) return "restV";
    if (&f == &L.newtonV) return "newtonV";
    if (&f == &L.bfac) return "bfac";
    return "?";
}

// Trace mode has no device: the norms are placeholders (1.0, never a stop), except that
// GS_TRACE_STOP_AFTER=k makes the norm closing cycle k read 0.0, so that the loop stops there and the
// schedule records an early stop (tests replay it: the undo of the overlapped next cycle's adoption).
double HipGridData::traceNorm()
{
    const char* e = std::getenv("GS_TRACE_STOP_AFTER"); // read per call: tests switch it
    const long stopAfter = e ? std::strtol(e, nullptr, 10) : -1;
    const long read = traceNorms_++; // 0: the initial norm, i + 1: cycle i's closing norm
    return (stopAfter >= 0 && read == stopAfter + 1) ? 0.0 : 1.0;
}

double HipGridData::readNorm()
{
    if (trace) return traceNorm();
    sync();
    return *(volatile double*)hNorm_;
}

void HipGridData::readNormBegin()
{
    if (trace) return;
    check((int)hipEventRecord(evNorm_, stream_.s), "hipEventRecord");
}

double HipGridData::readNormEnd()
{
    if (trace) return traceNorm();
    // distributed: a bounded wait that also polls the communicator's error state (gs_comm.hpp)
    if (comm_ && comm_->size() > 1) comm_->syncEvent(evNorm_);
    else check((int)hipEventSynchronize(evNorm_), "hipEventSynchronize");
    return *(volatile double*)hNorm_;
}

void HipGridData::sync()
{
    if (trace) return;
    // distributed: a bounded wait that also polls the communicator's error state (gs_comm.hpp)
    if (comm_ && comm_->size() > 1) comm_->sync(stream_.s);
    else check((int)hipStreamSynchronize(stream_.s), "hipStreamSynchronize");
}

void HipGridData::halo(LevelData& L, DeviceField& fld, hipStream_t s, int depth)
{
    if (!(L.distributed && nranks() > 1)) return;
    if (trace) {
        rec("halo", {{"L", (long long)levelIndex(L)}, {"depth", depth}}, fieldName(L, fld));
        return;
    }
    haloSettle(); // (an exchange of the pipelined sequence is settled before anything else is issued)
    // host cost of issuing + settling the exchange (RCCL: group start/end and the async-error poll)
    const auto t0 = std::chrono::steady_clock::now();
    comm_->halo(fld.data(), fld.ldz(), L.geom.nz, depth, s);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    haloHostMs += ms;
    haloHostMaxMs = std::max(haloHostMaxMs, ms);
    haloCalls++;
}

void HipGridData::haloIssue(LevelData& L, DeviceField& fld, hipStream_t s, int depth)
{
    if (!(L.distributed && nranks() > 1)) return;
    if (trace) {
        rec("halo", {{"L", (long long)levelIndex(L)}, {"depth", depth}}, fieldName(L, fld));
        return;
    }
    haloSettle();
    const auto t0 = std::chrono::steady_clock::now();
    comm_->haloIssue(fld.data(), fld.ldz(), L.geom.nz, depth, s);
    haloCurMs_ = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    haloPending_ = true;
}

bool HipGridData::haloReady()
{
    if (trace) return sw.haloOrder != 1;
    if (!haloPending_) return sw.haloOrder != 1;
    const auto t0 = std::chrono::steady_clock::now();
    const bool ok = comm_->haloReady();
    haloCurMs_ += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (sw.haloOrder == 1) return false;
    return sw.haloOrder == 2 || ok;
}

void HipGridData::haloSettle()
{
    if (!haloPending_) return;
    const auto t0 = std::chrono::steady_clock::now();
    comm_->haloSettle();
    haloCurMs_ += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    haloPending_ = false;
    haloHostMs += haloCurMs_;
    haloHostMaxMs = std::max(haloHostMaxMs, haloCurMs_);
    haloCalls++;
}

void HipGridData::gather(LevelData& L, DeviceField& fld)
{
    if (trace) rec("gather", {{"L", (long long)levelIndex(L)}}, fieldName(L, fld));
    else comm_->gatherPlanes(fld.data(), fld.ldz(), L.ranksLo, L.ranksHi, stream_.s);
}

gs_level HipGridData::ownedGeom(const LevelData& L, int64_t* off) const
{
    gs_level g = L.geom;
    *off = 0;
    const std::size_t l = &L - levels_.data();
    const bool transition = l > 0 && !L.distributed && levels_[l - 1].distributed;
    if (transition) {
        const int64_t lo = L.ranksLo[rank()], hi = L.ranksHi[rank()];
        g.nz = std::max<int64_t>(0, hi - lo + 1);
        g.z0 = lo - 1;
        *off = (lo - 1) * L.geom.ldz;
    }
    return g;
}

// ---------------------------------------------------------------------------------------------
// Per-sweep relaxation weights (pure host code)

// omega_k = 1 / ((hi+lo)/2 + (hi-lo)/2 cos(pi (2k-1) / (2 nu))), k = 1..nu: the reciprocals of the roots of the
// degree-nu Chebyshev polynomial on [lo, hi], so that prod (1 - omega_k x) is the polynomial of least maximum there
std::vector<double> chebyshevWeights(int nu, double lo, double hi)
{
    if (nu < 1) throw Error("chebyshev weights: nu must be at least 1");
    if (!(lo > 0.0) || !(hi > lo) || !std::isfinite(hi)) throw Error("chebyshev weights: need 0 < lo < hi");
    const double pi = 3.14159265358979323846;
    std::vector<double> w((std::size_t)nu);
    for (int k = 1; k <= nu; k++)
        w[(std::size_t)k - 1] = 1.0 / ((hi + lo) / 2 + (hi - lo) / 2 * std::cos(pi * (2 * k - 1) / (2.0 * nu)));
    return w;
}

std::vector<double> checkedWeights(const double* pre, int npre, const double* post, int npost, std::size_t gridPre,
                                   std::size_t gridPost)
{
    if (npre == 0 && npost == 0 && !pre && !post) return {}; // cleared
    if (npre < 0 || npost < 0 || (npre > 0 && !pre) || (npost > 0 && !post))
        throw Error("weights: a count is negative or its array is missing");
    if (npre > GS_MAX_WEIGHTS || npost > GS_MAX_WEIGHTS)
        throw Error("weights: at most " + std::to_string(GS_MAX_WEIGHTS) + " weights per leg");
    if ((std::size_t)npre != gridPre || (std::size_t)npost != gridPost)
        throw Error("weights: " + std::to_string(npre) + " pre / " + std::to_string(npost) +
                    " post weights for a grid with " + std::to_string(gridPre) + " pre / " +
                    std::to_string(gridPost) + " post smoothing sweeps");
    std::vector<double> w;
    for (int i = 0; i < npre; i++) w.push_back(pre[i]);
    for (int i = 0; i < npost; i++) w.push_back(post[i]);
    for (double x : w)
        if (!std::isfinite(x)) throw Error("weights: every weight must be finite");
    return w;
}

// GS_OMEGAS: "w1,w2/w3,w4" (pre weights, a slash, post weights; either side may be empty for a count of 0) or
// "cheb" (Chebyshev weights on [1/3, 2], the 7-point operator's high-frequency band, for the grid's own counts)
std::vector<double> parseOmegas(const char* text, std::size_t gridPre, std::size_t gridPost)
{
    const std::string t(text);
    if (t == "cheb") {
        if (gridPre > (std::size_t)GS_MAX_WEIGHTS || gridPost > (std::size_t)GS_MAX_WEIGHTS)
            throw Error("GS_OMEGAS: at most " + std::to_string(GS_MAX_WEIGHTS) + " weights per leg");
        std::vector<double> w;
        if (gridPre > 0) w = chebyshevWeights((int)gridPre, 1.0 / 3.0, 2.0);
        if (gridPost > 0) {
            const std::vector<double> q = chebyshevWeights((int)gridPost, 1.0 / 3.0, 2.0);
            w.insert(w.end(), q.begin(), q.end());
        }
        return w;
    }
    const std::size_t slash = t.find('/');
    if (slash == std::string::npos || t.find('/', slash + 1) != std::string::npos)
        throw Error("GS_OMEGAS: expected \"w1,w2/w3,w4\" or \"cheb\", got \"" + t + "\"");
    auto list = [&](const std::string& part) {
        std::vector<double> v;
        std::size_t pos = 0;
        while (!part.empty()) {
            const std::size_t comma = part.find(',', pos);
            const std::string item = part.substr(pos, comma == std::string::npos ? std::string::npos : comma - pos);
            char* end = nullptr;
            const double x = std::strtod(item.c_str(), &end);
            if (item.empty() || end == item.c_str() || *end != '\0')
                throw Error("GS_OMEGAS: \"" + item + "\" is not a number (in \"" + t + "\")");
            v.push_back(x);
            if (comma == std::string::npos) break;
            pos = comma + 1;
        }
        return v;
    };
    const std::vector<double> pre = list(t.substr(0, slash)), post = list(t.substr(slash + 1));
    if (pre.empty() && post.empty()) throw Error("GS_OMEGAS: no weights in \"" + t + "\"");
    return checkedWeights(pre.data(), (int)pre.size(), post.data(), (int)post.size(), gridPre, gridPost);
}

void HipGridData::setWeights(const double* pre, int npre, const double* post, int npost)
{
    weights = checkedWeights(pre, npre, post, npost, preSmoothing, postSmoothing); // (throws before assigning)
}

// ---------------------------------------------------------------------------------------------
thread_local std::vector<double>* HipSolver::history = nullptr;
thread_local std::vector<double>* NewtonSolver::history = nullptr;

namespace {

// one fused sweep over local planes [z1, z2] of level L: reads L.v, writes L.vAlt; with partials,
// also the per-block r^2 sums of the input's residual. Returns the partial count written.
// w: the sweep's relaxation weight (per-sweep weights, HipGridData::weights); NULL: the grid's omega
int64_t sweepPlanes(HipGridData& g, HipGridData::LevelData& L, int64_t z1, int64_t z2, hipStream_t s,
                    double* partials = nullptr, const double* w = nullptr)
{
    if (z2 < z1) return 0;
    gs_level sub = L.geom;
    sub.nz = z2 - z1 + 1;
    sub.z0 += z1 - 1;
    const int64_t off = (z1 - 1) * L.geom.ldz;
    if (g.trace) {
        g.rec("sweep", {{"L", (long long)g.levelIndex(L)}, {"z1", z1}, {"z2", z2}, {"vzero", L.vZero}, {"norm", partials != nullptr}});
        return partials ? 1 : 0;
    }
    check(gs_jacobi_sweep_norm(&L.sten, &sub, g.kmode(), w ? w[0] : g.omega, g.gamma,
                               L.vZero ? nullptr : L.v.data() + off,
                               L.vAlt.data() + off, L.f.data() + off, g.wOf(L) ? g.wOf(L) + off : nullptr,
                               partials, s),
          "gs_jacobi_sweep");
    return partials ? gs_residual_num_partials(&L.sten, &sub) : 0;
}

// two fused sweeps over local planes [z1, z2]: reads L.v (two ghost planes deep where a side is an
// internal boundary), writes L.vAlt; with partials, also the per-block r^2 sums of the input's
// residual. Returns the partial count written.
// w: the two sweeps' relaxation weights; NULL: the grid's omega for both
int64_t pairPlanes(HipGridData& g, HipGridData::LevelData& L, int64_t z1, int64_t z2, hipStream_t s,
                   double* partials = nullptr, const double* w = nullptr)
{
    if (z2 < z1) return 0;
    gs_level sub = L.geom;
    sub.nz = z2 - z1 + 1;
    sub.z0 += z1 - 1;
    const int64_t off = (z1 - 1) * L.geom.ldz;
    const bool dist = L.distributed && g.nranks() > 1;
    const int zlo = z1 > 1 || (dist && g.rank() > 0);
    const int zhi = z2 < L.geom.nz || (dist && g.rank() + 1 < g.nranks());
    if (g.trace) {
        g.rec("pair", {{"L", (long long)g.levelIndex(L)}, {"z1", z1}, {"z2", z2}, {"zlo", zlo}, {"zhi", zhi},
                       {"vzero", L.vZero}, {"norm", partials != nullptr}});
        return partials ? 1 : 0;
    }
    const double om[2] = {w ? w[0] : g.omega, w ? w[1] : g.omega};
    check(gs_jacobi_sweep2_norm_w(&L.sten, &sub, g.kmode(), om, g.gamma, L.vZero ? nullptr : L.v.data() + off,
                                  L.vAlt.data() + off, L.f.data() + off, g.wOf(L) ? g.wOf(L) + off : nullptr,
                                  zlo, zhi, partials, s),
          "gs_jacobi_sweep2");
    return partials ? gs_jacobi_sweep2_num_partials(&L.sten, &sub, (int)g.mode) : 0;
}

// three fused LINEAR sweeps over a whole non-distributed level (gs_jacobi_sweep3): reads L.v, writes L.vAlt
void tripleLevel(HipGridData& g, HipGridData::LevelData& L, hipStream_t s, const double* w)
{
    const double om[3] = {w ? w[0] : g.omega, w ? w[1] : g.omega, w ? w[2] : g.omega};
    check(gs_jacobi_sweep3_w(&L.sten, &L.geom, om, g.gamma, L.v.data(), L.vAlt.data(), L.f.data(), s),
          "gs_jacobi_sweep3");
}

// The first post-smoothing pair of v^h + P v^2h (gs_jacobi_sweep2_prolong) on planes z1..z2 of F
// into F.vAlt. Every plane range starts on an odd plane (the kernel's parities are global ones) and
// ends two planes below the level's top or on it: the planes past an internal range end are
// interior planes (or a neighbour's ghost copies), which the kernel corrects as it reads them.
void proPlanes(HipGridData& g, HipGridData::LevelData& F, HipGridData::LevelData& C, int64_t z1, int64_t z2,
               hipStream_t s)
{
    if (z2 < z1) return;
    gs_level sub = F.geom;
    sub.nz = z2 - z1 + 1;
    sub.z0 += z1 - 1;
    const int64_t off = (z1 - 1) * F.geom.ldz;
    const bool dist = F.distributed && g.nranks() > 1;
    const int zlo = z1 > 1 || (dist && g.rank() > 0);
    const int zhi = z2 < F.geom.nz || (dist && g.rank() + 1 < g.nranks());
    if (g.trace) {
        g.rec("pro", {{"L", (long long)g.levelIndex(F)}, {"z1", z1}, {"z2", z2}, {"zlo", zlo}, {"zhi", zhi}});
        return;
    }
    // rows > 512 points (column blocks): the corrected edge columns go through a workspace, one per
    // stream (the boundary planes' launch runs beside the interior's)
    const int64_t wsn = gs_jacobi_sweep2_prolong_ws_elems(&F.sten, &sub, (int)g.mode);
    // (allocated once, at grid creation, for the largest plane range upLeg requests: never reallocated —
    // a hipFree / hipMalloc here would synchronise the device inside the overlapped sequence)
    DeviceBuf& wb = F.proWs[s == g.stream() ? 0 : 1];
    if (wsn > wb.size()) throw Error("gs_jacobi_sweep2_prolong: workspace not sized at grid creation");
    double* ws = wsn > 0 ? wb.get(wsn) : nullptr;
    // (the prolongation pair is the first two post-smoothing sweeps: post[0..1] of the per-sweep weights)
    const double* w = g.wPost();
    const double om[2] = {w ? w[0] : g.omega, w ? w[1] : g.omega};
    check(gs_jacobi_sweep2_prolong_ws_w(&F.sten, &sub, g.kmode(), om, g.gamma, F.v.data() + off,
                                        C.v.data(), nullptr, &C.geom, F.vAlt.data() + off, F.f.data() + off,
                                        g.wOf(F) ? g.wOf(F) + off : nullptr, zlo, zhi, ws, wsn, s),
          "gs_jacobi_sweep2_prolong");
}

} // namespace

// Workspace elements of the largest plane range upLeg's fused prolongation pair requests on level l
// (the whole level, or the boundary / interior ranges of the overlapped Z-slab sequence).
int64_t proWsElems(const HipGridData& g, std::size_t l)
{
    if (g.xy()) return 0; // (the fused prolongation pair embeds the 3-D interpolation: never taken)
    const gs_level& G = g.getLevel(l).geom;
    const int64_t nz = G.nz, zt = nz % 2 == 0 ? nz - 1 : nz - 2;
    const int64_t ranges[4][2] = {{1, nz}, {1, 2}, {zt, nz}, {3, zt - 1}};
    int64_t need = 0;
    for (const auto& r : ranges) {
        if (r[1] < r[0] || r[0] < 1) continue;
        gs_level sub = G;
        sub.nz = r[1] - r[0] + 1;
        sub.z0 += r[0] - 1;
        need = std::max(need, gs_jacobi_sweep2_prolong_ws_elems(&g.getLevel(l).sten, &sub, (int)g.mode));
    }
    return need;
}

namespace {

bool transitionLevel(HipGridData& g, std::size_t l)
{
    return l > 0 && g.nranks() > 1 && !g.getLevel(l).distributed && g.getLevel(l - 1).distributed;
}

// fine level l -> coarse level l+1 (one or two coarse outputs), then ghost refresh / gather
void restrictTo(HipGridData& g, const DeviceField& src, std::size_t l, DeviceField& a, DeviceField* b,
                bool needGhosts)
{
    auto& F = g.getLevel(l);
    auto& C = g.getLevel(l + 1);
    const hipStream_t s = g.stream();
    int64_t off = 0;
    const gs_level cg = g.ownedGeom(C, &off);
    if (g.trace) {
        if (cg.nz > 0)
            g.rec("restrict", {{"L", (long long)l}, {"c1", cg.z0 + 1}, {"c2", cg.z0 + cg.nz}, {"two", b != nullptr}},
                  (std::string(HipGridData::fieldName(F, src)) + ">" + HipGridData::fieldName(C, a) +
                   (b ? std::string(",") + HipGridData::fieldName(C, *b) : std::string())).c_str());
    } else if (g.xy())
        check(gs_restrict_xy(src.data(), &F.geom, a.data(), &C.geom, g.xfer(l), s), "gs_restrict_xy");
    else if (g.pa(l))
        check(gs_restrict_pa(src.data(), &F.geom, a.data(), b ? b->data() : nullptr, &C.geom, g.xfer(l), s),
              "gs_restrict_pa");
    else if (cg.nz > 0)
        check(gs_restrict2(src.data(), &F.geom, a.data() + off, b ? b->data() + off : nullptr, &cg, s), "gs_restrict");
    if (transitionLevel(g, l + 1)) {
        g.gather(C, a);
        if (b) g.gather(C, *b);
    } else if (needGhosts) {
        g.halo(C, a, s);
        if (b) g.halo(C, *b, s, g.vDepth(C)); // b is the coarse iterate (FAS)
    }
}

} // namespace

// The overlapped exchange of a Z-slab sweep: the boundary planes run on their own stream (forked
// from the compute stream), the exchange on the comm stream after them, and the interior planes on
// the compute stream concurrently with both; the compute stream waits for the exchange (join,
// recorded after it, waited on after the interior launch) before the next sweep. The boundary and
// interior launches write disjoint planes of vAlt and only read v. Nothing to order in trace mode.
hipStream_t HipSolver::forkBoundary(HipGridData& grid)
{
    if (grid.trace) return grid.stream();
    check((int)hipEventRecord(grid.evA_, grid.stream()), "hipEventRecord");
    check((int)hipStreamWaitEvent(grid.bndStream_.s, grid.evA_, 0), "hipStreamWaitEvent");
    return grid.bndStream_.s;
}

void HipSolver::forkComm(HipGridData& grid)
{
    if (grid.trace) return;
    check((int)hipEventRecord(grid.evC_, grid.bndStream_.s), "hipEventRecord");
    check((int)hipStreamWaitEvent(grid.commStream(), grid.evC_, 0), "hipStreamWaitEvent");
}

void HipSolver::joinComm(HipGridData& grid, bool wait)
{
    if (grid.trace) return;
    if (!wait) check((int)hipEventRecord(grid.evB_, grid.commStream()), "hipEventRecord");
    else check((int)hipStreamWaitEvent(grid.stream(), grid.evB_, 0), "hipStreamWaitEvent");
}

// the pipelined sequence's pending exchange settled on the host (its kernels are on the comm stream),
// then the event the next boundary planes and the final join wait on
void HipSolver::settleExchange(HipGridData& grid)
{
    grid.haloSettle();
    if (!grid.trace) check((int)hipEventRecord(grid.evB_, grid.commStream()), "hipEventRecord");
}

// (the speculative step is a level-0 point sweep or pair: not where level 0 runs z-line sweeps)
bool HipSolver::speculationEnabled(const HipGridData& grid)
{
    return grid.sw.speculation && grid.preSmoothing > 0 && grid.numLevels() > 1 && !grid.lineAt(0);
}

// src/cpu/CpuSolver.cpp:12-43. Every norm the loop reads (the initial one and each V-cycle's closing
// one) is the residual of the current level-0 iterate, which the next cycle's first pre-smoothing
// sweep computes anyway: that sweep runs speculatively into vAlt and reports the norm; if the loop
// stops there, vAlt is dropped and v is the final iterate, exactly as in the reference.
void HipSolver::solve(HipGridData& grid)
{
    const bool print = grid.printProgress && grid.rank() == 0;
    const bool spec = speculationEnabled(grid);
    if (grid.sw.solver == 1 && grid.mode == GridParams::LINEAR) pcgCheck(grid); // GS_SOLVER=pcg: likewise
    if (grid.sw.fmg > 0) fmgCheck(grid, grid.sw.fmg); // GS_FMG on a grid FMG cannot run on: before any work
    if (grid.sw.solver == 1 && grid.mode == GridParams::LINEAR) {
        // GS_SOLVER=pcg: the same lines and history from conjugate gradients; after GS_FMG=k from FMG's iterate, whose
        // residual is PCG's first norm and has FMG's line
        if (grid.sw.fmg > 0) {
            const double initial = compResidual(grid, 0, false, true);
            if (history) history->push_back(initial);
            if (print) std::cout << "Inital residual: " << initial << '\n';
            if (print) Timer::start();
            fmgRun(grid, grid.sw.fmg);
            grid.clock.segLevel.clear();
            pcg(grid, &initial);
        } else {
            pcg(grid);
        }
        return;
    }
    int pending = 0;
    const double initialResidual = spec ? speculativeSweep(grid, &pending) : compResidual(grid, 0, false, true);
    if (history) history->push_back(initialResidual);
    if (print) std::cout << "Inital residual: " << initialResidual << '\n';
    if (print) Timer::start();
    if (grid.sw.fmg > 0) {
        // GS_FMG=k: the full-multigrid start replaces level 0's iterate (the speculative sweep of the old one is
        // dropped); its residual is the next cycle's speculative step's, like every closing norm, has its own line
        // (which the reference harness's regex does not match), enters the history and is held against tol
        fmgRun(grid, grid.sw.fmg);
        grid.clock.segLevel.clear(); // (the per-level clock times the V-cycles of the loop below only)
        pending = 0;
        const double res = spec ? speculativeSweep(grid, &pending) : compResidual(grid, 0, false, true);
        if (history) history->push_back(res);
        if (print) {
            std::cout << "fmg: cycles: " << grid.sw.fmg << " residual: " << res << ' ';
            Timer::stop();
            Timer::start();
        }
        if (res <= initialResidual / (1.0 / grid.tol)) return;
    }
    auto onNorm = [&](std::size_t i, double res) {
        if (history) history->push_back(res);
        if (print) {
            std::cout << "iter: " << i << " residual: " << res << ' ';
            Timer::stop(); // "Took Nms": from the previous norm to this one (the cycles overlap)
            Timer::start();
        }
        return res <= initialResidual / (1.0 / grid.tol);
    };
    // The closing norm of the LAST cycle decides nothing (the loop ends at maxiter either way): when nobody
    // reads it — no progress print, no history, no per-level clock; NewtonSolver::findError's inner solves — that
    // cycle ends with its up-leg and the norm's pass (a whole level-0 pair at 512^3) is not run
    // (rank-uniform: every rank must run the same exchanges and collectives, so the decision rests on the
    // grid's printProgress, not on `print`, which only rank 0 has, and on clock.on, which a distributed grid
    // agrees across ranks at creation)
    const bool lastNormDead = !grid.printProgress && history == nullptr && !grid.clock.on;
    if (spec) {
        runCycles(grid, &pending, grid.maxiter, onNorm, lastNormDead);
    } else {
        for (std::size_t i = 0; i < grid.maxiter; i++) {
            if (lastNormDead && i + 1 == grid.maxiter) {
                cycleDown(grid, nullptr);
                cycleUpNoNorm(grid);
                break;
            }
            if (onNorm(i, vcycle(grid))) break;
        }
    }
}

// level 0's up-leg without the closing norm (the last cycle of a solve whose final norm nobody reads)
void HipSolver::cycleUpNoNorm(HipGridData& grid)
{
    if (std::min(grid.coarseFrom, grid.numLevels() - 1) >= 1) upLeg(grid, 1);
    if (grid.trace) grid.rec("nonorm", {{"L", 0}});
}

// Global ||.|| from this rank's per-block partials: fixed-order sums per rank, then over ranks in
// rank order, so every rank (and every run) gets the same bits.
double HipSolver::finishNorm(HipGridData& grid, int64_t nparts, bool wait)
{
    const hipStream_t s = grid.stream();
    if (grid.trace) {
        grid.rec("norm", {{"allgather", grid.nranks() > 1 && grid.getLevel(0).distributed}});
        return wait ? grid.readNorm() : std::nan(""); // (!wait: readNormEnd reads it)
    }
    if (grid.nranks() > 1 && grid.getLevel(0).distributed) {
        check(gs_sumsq_finish(grid.partials(), nparts, grid.dNorm(), 1, s), "gs_sumsq_finish");
        grid.comm()->allgather1(grid.dNorm(), grid.dRankSums(), s);
        check(gs_sumsq_finish(grid.dRankSums(), grid.nranks(), grid.hNormDev(), 0, s), "gs_sumsq_finish");
    } else {
        check(gs_sumsq_finish(grid.partials(), nparts, grid.hNormDev(), 0, s), "gs_sumsq_finish");
    }
    if (wait) return grid.readNorm();
    grid.readNormBegin();
    return std::nan("");
}

// compResidual (src/cpu/CpuSolver.cpp:45-83): r is written only when a restriction consumes it,
// the norm only when a caller reads it (level 0).
double HipSolver::compResidual(HipGridData& grid, std::size_t l, bool storeR, bool norm)
{
    materialize(grid, l);
    auto& L = grid.getLevel(l);
    const hipStream_t s = grid.stream();
    if (grid.trace)
        grid.rec("residual", {{"L", (long long)l}, {"store", storeR}, {"norm", norm}});
    else
        check(gs_residual(&L.sten, &L.geom, grid.kmode(), grid.gamma, L.v.data(), L.f.data(),
                          grid.wOf(L), storeR ? L.r.data() : nullptr,
                          norm ? grid.partials() : nullptr, s),
              "gs_residual");
    if (storeR) grid.halo(L, L.r, s);
    if (!norm) return 0.0;
    return finishNorm(grid, gs_residual_num_partials(&L.sten, &L.geom));
}

// Whether level l's first post-smoothing pair can take the prolongation from level l+1 (rank-uniform:
// the pair's ghost exchange is collective). A Z-slab level needs every slab to start on an even global
// plane (the kernel's plane parities) and, under a Z-slab coarse level, each rank's coarse planes over
// its fine ones with two coarse ghost planes (the bottom ghost fine plane interpolates from coarse
// plane -1); a replicated coarse level holds every plane.
static bool proSlabOk(HipGridData& grid, std::size_t l)
{
    auto& F = grid.getLevel(l);
    auto& C = grid.getLevel(l + 1);
    if (!(F.distributed && grid.nranks() > 1)) return true;
    for (int q = 0; q < grid.nranks(); q++) {
        if ((F.ranksLo[q] - 1) % 2 != 0) return false;
        if (C.distributed && 2 * (C.ranksLo[q] - 1) != F.ranksLo[q] - 1) return false;
    }
    return !C.distributed || grid.vDepth(C) == 2;
}

// NEWTON's fused prolongation pair keeps part of its state in LDS and recomputes exp(newtonV) for
// its second sweep: on 512^3 it saves 0.14 ms per V-cycle against gs_prolong_add + the plain pair, on
// 256^3 / 128^3 it cost 0.065 / 0.05 ms more (profiles/r01l_summary.md). Since r04 levels of at most
// two 256-point y-blocks launch a two-x-wave instance (74 KB of LDS, two blocks per CU), which wins on
// 512^3's level 1 and 256^3's level 0 too (Newton iteration 36.5-36.6 against 36.7-36.75 ms at 512^3,
// 6.32-6.36 against 6.58-6.62 ms at 256^3: profiles/r04/r04e_newton_ab_swizzle_rrreverse.txt,
// r04f_newton_pro_threshold.txt),
// so NEWTON levels take it from GS_NEWTON_PRO_POINTS points per rank on (judged on the thinnest slab: rank-uniform).
// Since r06 the default is 2^21, so 512^3's 128^3 level fuses too: its two-x-wave GS_NEWTON_B prolongation pair
// (34.7 us) replaces gs_prolong_add (39 us) + the plain pair (22 us), one launch fewer per inner V-cycle; a Newton
// iteration's kernel time 29.09 vs 29.22 ms, wall 27.63-27.80 vs 27.69-27.84 ms (3 interleaved rounds,
// profiles/r06/r06p_newton_pro_points_ab.txt). LINEAR levels always do.
static bool proWorthIt(HipGridData& grid, std::size_t l)
{
    if (grid.mode != GridParams::NEWTON) return true;
    const int64_t minPoints = grid.sw.newtonProPoints;
    const auto& F = grid.getLevel(l);
    return (int64_t)F.levelDim[0] * (int64_t)F.levelDim[1] * F.minPlanes >= minPoints;
}

// k sweeps (src/cpu/CpuSolver.cpp:141-180). Each reads v and writes vAlt, then the two swap. Where
// the level allows, sweeps run in fused pairs (gs_jacobi_sweep2: one read of v and f, one write, for
// two sweeps), an odd one as a single sweep.
//
// On a Z-slab the outermost planes of each step (one per side for a sweep, two for a pair) run on the
// boundary stream, their ghost exchange follows on the comm stream, and the interior planes run on the
// compute stream beside both. The steps of one call are pipelined so that the compute stream never waits
// for an exchange: step k's interior reads only v's owned planes (k-1's interior, k-1's boundary
// planes), never its ghost planes, so it needs boundary k-1 but not exchange k-1. Only the boundary
// planes of step k wait for exchange k-1 (the ghosts they read) and for interior k-1 (whose input planes
// they overwrite); exchange k then hides under interior k+1 instead of sitting between two interiors.
// The last exchange is joined into the compute stream before returning. Writes never meet a read of the
// same planes: interior k writes the buffer exchange k-2 sent from (its boundary planes only) and that
// boundary k-1 read planes 3-4 of before it (event), boundary k writes planes exchange k-2 sent (comm is
// in order, boundary k waits exchange k-1). The interior launch is enqueued before the exchange is issued:
// RCCL's non-blocking group is settled on the host (gs_comm.cpp), and the GPU must not wait on that host
// round-trip between the boundary planes and the interior.
//
// w: a cursor into the per-sweep relaxation weights (HipGridData::weights), one weight per sweep of this call:
// every triple, pair and single sweep takes its slice and moves the cursor on. NULL: the grid's omega throughout.
void HipSolver::jacobi(HipGridData& grid, std::size_t l, std::size_t sweeps, const double* w)
{
    auto& L = grid.getLevel(l);
    const hipStream_t s = grid.stream();
    if (L.line) {
        // one z-line sweep per sweep (single GPU, whole levels: setSmoother): no pairs, no triples
        for (; sweeps > 0; sweeps--) {
            check(gs_zline_sweep(&L.sten, &L.geom, w ? *w++ : grid.omega, L.vZero ? nullptr : L.v.data(),
                                 L.vAlt.data(), L.f.data(), grid.zlineTables(l), s),
                  "gs_zline_sweep");
            L.v.swap(L.vAlt);
            L.vZero = false;
        }
        return;
    }
    const bool dist = L.distributed && grid.nranks() > 1;
    const int64_t nz = L.geom.nz;
    const int depth = grid.vDepth(L);
    int step = 0; // overlapped steps issued in this call
    while (sweeps > 0) {
        // a fused triple where the level takes them and the rest of the sequence still splits into triples and
        // pairs (3: T, 4: P P, 5: T P, 6: T T, 7: T P P, ...): never on a Z-slab, in the schedule trace or on
        // the zero iterate, which keep the pair schedule
        if (L.fusedTriples && !dist && !grid.trace && !L.vZero && (sweeps == 3 || sweeps >= 5)) {
            tripleLevel(grid, L, s, w);
            L.triplesRun++;
            L.v.swap(L.vAlt);
            sweeps -= 3;
            if (w) w += 3;
            continue;
        }
        const bool pair = L.fusedPairs && sweeps >= 2;
        const int64_t b = pair ? 2 : depth; // outermost planes whose ghost copies the neighbours need
        auto run = [&](int64_t z1, int64_t z2, hipStream_t st) {
            if (pair) pairPlanes(grid, L, z1, z2, st, nullptr, w);
            else sweepPlanes(grid, L, z1, z2, st, nullptr, w);
        };
        if (!dist) {
            run(1, nz, s);
        } else if (grid.overlapHalo && nz >= 2 * b + 1) {
            hipStream_t bs = s;
            // interior k reads boundary k-1's planes (boundary k's event slot is recorded below, k-1's still
            // holds) and interior k-1's, but no ghost plane: it may go before exchange k-1 has settled. When
            // that exchange is still being settled on the host (RCCL's non-blocking group), interior k is
            // enqueued first, so the GPU never idles behind the host; otherwise boundary k goes first, so its
            // exchange starts as early as possible (GS_HALO_ORDER forces either order)
            const bool interiorFirst = step > 0 && !grid.haloReady();
            if (!grid.trace) {
                bs = grid.bndStream_.s;
                check((int)hipEventRecord(grid.evA_, s), "hipEventRecord"); // after interior k-1
            }
            auto interior = [&] {
                if (!grid.trace && step > 0)
                    check((int)hipStreamWaitEvent(s, grid.evBnd_[(step - 1) & 1], 0), "hipStreamWaitEvent");
                run(b + 1, nz - b, s);
            };
            if (interiorFirst) interior();
            if (step > 0) settleExchange(grid); // exchange k-1's kernels on the comm stream, then evB
            if (!grid.trace) {
                // boundary k after interior k-1 (whose input planes it overwrites) and after exchange k-1
                // (the ghost planes it reads; on the comm stream, after every earlier exchange)
                check((int)hipStreamWaitEvent(bs, grid.evA_, 0), "hipStreamWaitEvent");
                if (step > 0) check((int)hipStreamWaitEvent(bs, grid.evB_, 0), "hipStreamWaitEvent");
            }
            run(1, b, bs);
            run(nz - b + 1, nz, bs);
            if (!grid.trace) {
                hipEvent_t bnd = grid.evBnd_[step & 1];
                check((int)hipEventRecord(bnd, bs), "hipEventRecord");
                check((int)hipStreamWaitEvent(grid.commStream(), bnd, 0), "hipStreamWaitEvent");
            }
            if (!interiorFirst) interior();
            grid.haloIssue(L, L.vAlt, grid.commStream(), depth); // settled at the next step or below
            step++;
        } else {
            if (step > 0) {
                settleExchange(grid);
                joinComm(grid, true); // an earlier overlapped step's exchange
            }
            step = 0;
            run(1, nz, s);
            grid.halo(L, L.vAlt, s, depth);
        }
        L.v.swap(L.vAlt);
        if (grid.trace) grid.rec("swap", {{"L", (long long)l}});
        L.vZero = false;
        sweeps -= pair ? 2 : 1;
        if (w) w += pair ? 2 : 1;
    }
    if (step > 0) {
        // the last exchange (and through it the last boundary planes) before anything else on the level
        settleExchange(grid);
        joinComm(grid, true);
        if (!grid.trace) check((int)hipStreamWaitEvent(s, grid.evBnd_[(step - 1) & 1], 0), "hipStreamWaitEvent");
    }
}

// v = 0 made real (the zero-iterate sweeps had no chance to replace it)
void HipSolver::materialize(HipGridData& grid, std::size_t l)
{
    auto& L = grid.getLevel(l);
    if (!L.vZero) return;
    if (grid.trace) grid.rec("zero", {{"L", (long long)l}}, "v");
    L.v.zero(grid.stream());
    L.vZero = false;
}

// CpuSolver.cpp:92-135 below level `from` in one launch (gs_coarse_cycle): the caller has set
// f^from (and, FAS, restV / v); on return every level from..nl-1 holds its post-smoothed iterate.
void HipSolver::coarseCycle(HipGridData& grid, std::size_t from)
{
    const std::size_t nl = grid.numLevels();
    gs_coarse_level lv[16] = {};
    const int n = (int)(nl - from);
    if (n < 1 || n > 16) throw Error("coarseCycle: bad level range");
    for (int j = 0; j < n; j++) {
        auto& L = grid.getLevel(from + j);
        lv[j] = gs_coarse_level{L.v.data(), L.vAlt.data(), L.f.data(), L.r ? L.r.data() : nullptr,
                                L.restV ? L.restV.data() : nullptr, const_cast<double*>(grid.wOf(L)),
                                L.geom, j == 0 ? (L.vZero ? 1 : 0) : (grid.mode != GridParams::NONLINEAR ? 1 : 0)};
    }
    if (grid.trace)
        grid.rec("coarse", {{"from", (long long)from}, {"vzero", lv[0].v_zero}});
    else if (grid.weighted())
        check(gs_coarse_cycle_w(&grid.getLevel(from).sten, lv, n, grid.kmode(), grid.wPre(), grid.gamma, (int)grid.preSmoothing,
                                (int)grid.postSmoothing, grid.stream()),
              "gs_coarse_cycle");
    else
        check(gs_coarse_cycle(&grid.getLevel(from).sten, lv, n, grid.kmode(), grid.omega, grid.gamma, (int)grid.preSmoothing,
                              (int)grid.postSmoothing, grid.stream()),
              "gs_coarse_cycle");
    const bool odd = ((grid.preSmoothing + grid.postSmoothing) & 1) != 0; // every level swept pre+post times
    for (int j = 0; j < n; j++) {
        auto& L = grid.getLevel(from + j);
        if (odd) {
            L.v.swap(L.vAlt);
            if (grid.trace) grid.rec("swap", {{"L", (long long)(from + j)}});
        }
        L.vZero = false;
    }
}

// The first pre-smoothing step of the next cycle, run into vAlt (v untouched) with the norm of the
// residual of v: a fused pair when level 0 smooths in pairs and pre-smoothing has two sweeps, else
// one sweep. *sweeps = how many sweeps vAlt holds.
double HipSolver::speculativeSweep(HipGridData& grid, int* sweeps, bool wait)
{
    auto& L = grid.getLevel(0);
    const hipStream_t s = grid.stream();
    const int64_t nz = L.geom.nz;
    double* P = grid.partials();
    int64_t n = 0;
    const bool pair = L.fusedPairs && grid.preSmoothing >= 2;
    const int depth = grid.vDepth(L);
    const int64_t b = pair ? 2 : depth;
    auto run = [&](int64_t z1, int64_t z2, hipStream_t st) {
        // (the first pre-smoothing sweeps: pre[0..] of the per-sweep weights)
        n += pair ? pairPlanes(grid, L, z1, z2, st, P + n, grid.wPre())
                  : sweepPlanes(grid, L, z1, z2, st, P + n, grid.wPre());
    };
    if (!(L.distributed && grid.nranks() > 1)) {
        run(1, nz, s);
    } else if (grid.overlapHalo && nz >= 2 * b + 1) {
        const hipStream_t bs = forkBoundary(grid);
        run(1, b, bs);
        run(nz - b + 1, nz, bs);
        forkComm(grid);
        run(b + 1, nz - b, s); // interior enqueued before the RCCL group is issued and settled
        grid.halo(L, L.vAlt, grid.commStream(), depth);
        joinComm(grid, false);
        joinComm(grid, true);
    } else {
        run(1, nz, s);
        grid.halo(L, L.vAlt, s, depth);
    }
    if (sweeps) *sweeps = pair ? 2 : 1;
    grid.clock.mark(s, 0, false); // closes the caller's segment before the norm's host sync
    return finishNorm(grid, n, wait);
}

void HipSolver::restrict(HipGridData& grid, const DeviceField& src, std::size_t srcLevel, DeviceField& dst)
{
    restrictTo(grid, src, srcLevel, dst, nullptr, true);
}

double HipSolver::vcycle(HipGridData& grid) { return vcycleSpeculative(grid, nullptr); }

// The up-leg of level i-1 from level i (CpuSolver.cpp:121-135): v^(i-1) += P v^i, post-smoothing.
void HipSolver::upLeg(HipGridData& grid, std::size_t i)
{
    const hipStream_t s = grid.stream();
    auto& C = grid.getLevel(i);
    auto& F = grid.getLevel(i - 1);
    grid.clock.mark(s, (int)(i - 1), true);
    materialize(grid, i); // only if the level had no sweep at all
    // (the tiled step fuses the prolongation with a pair: the GS_NO_FUSED_SWEEPS / GS_NO_FUSED_PROLONG
    // alternatives take the general path below)
    const bool xy = grid.xy(); // XY hierarchy: the general path below, with gs_prolong_add_xy
    const bool pa = xy || grid.pa(i - 1); // position-aware transfers: the general path below, with gs_prolong_add_pa
    const bool zl = F.line; // z-line sweeps: neither fused step below, both embed point Jacobi
    if (!pa && !zl && i - 1 >= 1 && F.tiled && !C.distributed && grid.postSmoothing >= 2 && grid.sw.fusedSweeps &&
        grid.sw.fusedProlong) {
        // a small level: prolongation, correction and the first two post-smoothing sweeps in one launch
        materialize(grid, i - 1);
        if (grid.trace)
            grid.rec("tiledpro", {{"L", (long long)(i - 1)}});
        else {
            const double* w = grid.wPost();
            const double om[2] = {w ? w[0] : grid.omega, w ? w[1] : grid.omega};
            check(gs_prolong_smooth2_tiled_w(&F.sten, &F.geom, grid.kmode(), om, grid.gamma, F.v.data(),
                                             C.v.data(), &C.geom, F.vAlt.data(), F.f.data(), grid.wOf(F), s),
                  "gs_prolong_smooth2_tiled");
        }
        F.v.swap(F.vAlt);
        if (grid.trace) grid.rec("swap", {{"L", (long long)(i - 1)}});
        F.vZero = false;
        jacobi(grid, i - 1, grid.postSmoothing - 2, grid.wPost(2));
        grid.clock.mark(s, (int)(i - 1), false);
        return;
    }
    if (!pa && !zl && grid.sw.fusedProlong && F.fusedPairs && grid.postSmoothing >= 2 && proWorthIt(grid, i - 1) && proSlabOk(grid, i - 1) &&
        gs_jacobi_sweep2_prolong_supported(&F.sten, &F.geom, (int)grid.mode)) {
        // the first two post-smoothing sweeps of v^h + P v^2h in one pass (the corrected
        // iterate is never stored), then the remaining ones. On a Z-slab each rank corrects its
        // ghost planes itself, from the coarse planes under them, and the pair's outermost planes
        // go first so that their exchange overlaps the interior (as in jacobi())
        materialize(grid, i - 1);
        const int64_t nz = F.geom.nz;
        if (!(F.distributed && grid.nranks() > 1)) {
            proPlanes(grid, F, C, 1, nz, s);
        } else if (grid.overlapHalo && nz >= 5) {
            const int64_t zt = nz % 2 == 0 ? nz - 1 : nz - 2; // odd start: 2 or 3 top planes
            const hipStream_t bs = forkBoundary(grid);
            proPlanes(grid, F, C, 1, 2, bs);
            proPlanes(grid, F, C, zt, nz, bs);
            forkComm(grid);
            proPlanes(grid, F, C, 3, zt - 1, s); // interior first (see jacobi())
            grid.halo(F, F.vAlt, grid.commStream(), grid.vDepth(F));
            joinComm(grid, false);
            joinComm(grid, true);
        } else {
            proPlanes(grid, F, C, 1, nz, s);
            grid.halo(F, F.vAlt, s, grid.vDepth(F));
        }
        F.v.swap(F.vAlt);
        if (grid.trace) grid.rec("swap", {{"L", (long long)(i - 1)}});
        F.vZero = false;
        jacobi(grid, i - 1, grid.postSmoothing - 2, grid.wPost(2));
        grid.clock.mark(s, (int)(i - 1), false);
        return;
    }
    // v^h += P (v^2h [- restV^2h])   (CpuSolver.cpp:121-132, interpolate + v += e fused)
    if (grid.trace)
        grid.rec("prolongadd", {{"L", (long long)(i - 1)}, {"sub", grid.mode == GridParams::NONLINEAR}});
    else if (xy) {
        materialize(grid, i - 1);
        check(gs_prolong_add_xy(C.v.data(), &C.geom, F.v.data(), &F.geom, grid.xfer(i - 1), s), "gs_prolong_add_xy");
    } else if (pa) {
        materialize(grid, i - 1);
        check(gs_prolong_add_pa(C.v.data(), grid.mode == GridParams::NONLINEAR ? C.restV.data() : nullptr, &C.geom,
                                F.v.data(), &F.geom, grid.xfer(i - 1), s),
              "gs_prolong_add_pa");
    } else
        check(gs_prolong_add(C.v.data(), grid.mode == GridParams::NONLINEAR ? C.restV.data() : nullptr, &C.geom,
                             F.v.data(), &F.geom, s),
              "gs_prolong_add");
    grid.halo(F, F.v, s, grid.vDepth(F));
    jacobi(grid, i - 1, grid.postSmoothing, grid.wPost());
    grid.clock.mark(s, (int)(i - 1), false);
}

// src/cpu/CpuSolver.cpp:85-139, in two halves (see gs_grid.hpp)
void HipSolver::cycleDown(HipGridData& grid, int* pending) { downFrom(grid, 0, pending); }

void HipSolver::downFrom(HipGridData& grid, std::size_t from, int* pending)
{
    const std::size_t nl = grid.numLevels();
    const hipStream_t s = grid.stream();
    // levels lc.. run as one gs_coarse_cycle launch (lc == nl: none); the host loops descend to lc
    // (a cycle rooted at or below coarseFrom is that one launch from its root on)
    const std::size_t lc = std::max(grid.coarseFrom, from), last = std::min(lc, nl - 1);
    for (std::size_t i = from; i < last; i++) {
        grid.clock.mark(s, (int)i, true);
        std::size_t pre = grid.preSmoothing;
        if (i == 0 && pending && *pending > 0 && pre >= (std::size_t)*pending) {
            grid.getLevel(0).v.swap(grid.getLevel(0).vAlt); // adopt the speculative first sweep(s)
            grid.getLevel(0).vZero = false;
            if (grid.trace) grid.rec("swap", {{"L", 0}});
            pre -= (std::size_t)*pending;
            *pending = 0;
        }
        auto& L = grid.getLevel(i);
        auto& C = grid.getLevel(i + 1);
        // (the tiled step fuses a pair, the residual and the restriction and leaves v^2h = 0 as a flag: the
        // GS_NO_FUSED_SWEEPS / GS_NO_FUSED_RR / GS_NO_ZERO_GUESS alternatives take the general path below)
        const bool xy = grid.xy(); // XY hierarchy: the general path below with the _xy launchers
        const bool pa = xy || grid.pa(i); // position-aware transfers: the general path below with the _pa launchers
        if (!pa && !L.line && i >= 1 && pre == 2 && L.tiled && !C.distributed && grid.sw.fusedSweeps &&
            grid.sw.fusedRR && grid.sw.zeroGuess) {
            // a small level: the pre-smoothing pair, residual and restriction in one tiled launch
            if (grid.trace)
                grid.rec("tiledpre", {{"L", (long long)i}, {"vzero", L.vZero}});
            else {
                const double* w = grid.wPre(); // (i >= 1: no speculative sweeps, the pair is pre[0..1])
                const double om[2] = {w ? w[0] : grid.omega, w ? w[1] : grid.omega};
                check(gs_smooth2_restrict_tiled_w(&L.sten, &L.geom, grid.kmode(), om, grid.gamma,
                                                  L.vZero ? nullptr : L.v.data(), L.vAlt.data(), L.f.data(),
                                                  grid.wOf(L), C.f.data(), &C.geom, s),
                      "gs_smooth2_restrict_tiled");
            }
            L.v.swap(L.vAlt);
            if (grid.trace) grid.rec("swap", {{"L", (long long)i}});
            L.vZero = false;
            C.vZero = true; // LINEAR / NEWTON: v^2h = 0 (CpuSolver.cpp:100-101), not stored
            grid.clock.mark(s, (int)i, false);
            continue;
        }
        jacobi(grid, i, pre, grid.wPre(grid.preSmoothing - pre)); // (past the adopted speculative sweeps)
        // f^2h = R (f^h - A v^h) in one pass: the fine residual is never stored
        bool fused = false;
        if (grid.sw.fusedRR) {
            materialize(grid, i);
            const double* w = grid.wOf(L);
            if (xy) {
                check(gs_residual_restrict_xy(&L.sten, &L.geom, L.v.data(), L.f.data(), C.f.data(), &C.geom,
                                              grid.xfer(i), s),
                      "gs_residual_restrict_xy");
                fused = true;
            } else if (pa) {
                if (HipGridData::paFusedRR) {
                    check(gs_residual_restrict_pa(&L.sten, &L.geom, grid.kmode(), grid.gamma, L.v.data(),
                                                  L.f.data(), w, C.f.data(), &C.geom, grid.xfer(i), s),
                          "gs_residual_restrict_pa");
                    fused = true;
                }
            } else if (!(L.distributed && grid.nranks() > 1)) {
                if (grid.trace)
                    grid.rec("resrestrict", {{"L", (long long)i}, {"c1", 1}, {"c2", C.geom.nz}, {"zhi", 0}});
                else
                    check(gs_residual_restrict(&L.sten, &L.geom, grid.kmode(), grid.gamma, L.v.data(),
                                               L.f.data(), w, C.f.data(), nullptr, &C.geom, s),
                          "gs_residual_restrict");
                fused = true;
            } else {
                // Z-slab: this rank's coarse planes from its fine slab, whose top ghost planes are current
                // (v after the sweep's exchange, f / newtonV after theirs); then the coarse ghosts / gather
                // every rank must take the same branch (the ghost exchanges are collective): the slab
                // kernel needs each rank's coarse planes over its even fine planes
                bool slabOk = true;
                for (int q = 0; q < grid.nranks(); q++)
                    if (C.ranksHi[q] >= C.ranksLo[q]) slabOk = slabOk && 2 * (C.ranksLo[q] - 1) == L.ranksLo[q] - 1;
                int64_t off = 0;
                const gs_level cg = grid.ownedGeom(C, &off);
                const int zhi = grid.rank() + 1 < grid.nranks();
                // (the residual on the top ghost plane reads v two planes deep)
                slabOk = slabOk && grid.vDepth(L) == 2 &&
                         gs_residual_restrict_slab_supported(&L.sten, &L.geom) != 0;
                if (slabOk) {
                    if (cg.nz > 0 && grid.trace)
                        grid.rec("resrestrict", {{"L", (long long)i}, {"c1", cg.z0 + 1}, {"c2", cg.z0 + cg.nz}, {"zhi", zhi}});
                    else if (cg.nz > 0)
                        check(gs_residual_restrict_slab(&L.sten, &L.geom, grid.kmode(), grid.gamma,
                                                        L.v.data(), L.f.data(), w, C.f.data() + off, nullptr, &cg,
                                                        zhi, s),
                              "gs_residual_restrict_slab");
                    if (transitionLevel(grid, i + 1)) grid.gather(C, C.f);
                    else grid.halo(C, C.f, s);
                    fused = true;
                }
            }
        }
        if (!fused) {
            compResidual(grid, i, true, false);
            restrictTo(grid, L.r, i, C.f, nullptr, true); // f^2h = R r^h (ghosts: the fused pair reads them)
        }
        if (grid.mode != GridParams::NONLINEAR) {
            // v^2h = 0 (CpuSolver.cpp:114-116): not stored; the first sweep on the level reads no v
            if (!grid.sw.zeroGuess) {
                if (grid.trace) grid.rec("zero", {{"L", (long long)(i + 1)}}, "v");
                C.v.zero(s);
            } else {
                C.vZero = true;
            }
        } else {
            // FAS: restV = v^2h = R v^h, then f^2h += A^2h(restV)  (CpuSolver.cpp:104-113)
            restrictTo(grid, L.v, i, C.restV, &C.v, true);
            if (grid.trace)
                grid.rec("applyadd", {{"L", (long long)(i + 1)}});
            else
                check(gs_apply_op_add(&C.sten, &C.geom, grid.gamma, C.restV.data(), C.f.data(), s),
                      "gs_apply_op_add");
            grid.halo(C, C.f, s);
        }
        grid.clock.mark(s, (int)i, false);
    }
    grid.clock.mark(s, (int)std::min(lc, nl - 1), true);
    if (lc < nl) coarseCycle(grid, lc);
    else jacobi(grid, nl - 1, grid.preSmoothing + grid.postSmoothing, grid.wPre()); // coarsest "solve": pre, then post weights
    grid.clock.mark(s, (int)std::min(lc, nl - 1), false);
    for (std::size_t i = last; i > from + 1; i--) upLeg(grid, i);
}

void HipSolver::vcycleFrom(HipGridData& grid, std::size_t level)
{
    const std::size_t nl = grid.numLevels();
    if (level >= nl) throw Error("vcycleFrom: no such level");
    if (grid.nranks() > 1)
        throw Error("vcycleFrom: single-GPU grids only (a Z-slab grid's coarse levels are gathered from level 0 down)");
    downFrom(grid, level, nullptr);
    // the root's own up-leg (level 0's is cycleUp0's / cycleUpNoNorm's); none when the root is the coarse end
    if (std::min(std::max(grid.coarseFrom, level), nl - 1) > level) upLeg(grid, level + 1);
}

std::size_t HipSolver::fmgStartLevel(const HipGridData& grid)
{
    if (grid.mode == GridParams::NEWTON || grid.nranks() > 1 || grid.trace || grid.xy()) return 0;
    if (grid.fmgProlongMode == 1) return grid.numLevels() - 1; // every transition can be prolonged
    std::size_t s = 0;
    while (s + 1 < grid.numLevels() && gs_fmg_prolong_supported(&grid.getLevel(s + 1).geom, &grid.getLevel(s).geom)) s++;
    return s;
}

void HipSolver::fmgCheck(const HipGridData& grid, int cyclesPerLevel)
{
    if (grid.mode == GridParams::NEWTON)
        throw Error("FMG: NEWTON mode is not supported (LINEAR and NONLINEAR grids only)");
    if (grid.nranks() > 1 || grid.trace)
        throw Error("FMG: single-GPU grids only (not a Z-slab / RCCL or schedule-trace grid)");
    if (grid.xy())
        throw Error("FMG: not on an XY semi-coarsened grid (gs_fmg_prolong interpolates in z too; an XY full-multigrid "
                    "start is not built)");
    if (cyclesPerLevel < 1) throw Error("FMG: cycles per level must be at least 1");
    if (grid.fmgProlongMode == 1 && grid.transferMode == 0)
        for (std::size_t l = 0; l + 1 < grid.numLevels(); l++)
            if (!grid.levelAligned(l)) {
                const auto& d = grid.getLevel(0).levelDim;
                throw Error("FMG: the position-aware prolongation (GS_FMG_PROLONG=position) on " + std::to_string(d[0]) +
                            " x " + std::to_string(d[1]) + " x " + std::to_string(d[2]) +
                            ", whose coarse grids do not all align, needs the position-aware transfers for its V-cycles: "
                            "gs_grid_set_transfer(GS_TRANSFER_POSITION) / GS_TRANSFER=position");
            }
    if (fmgStartLevel(grid) == 0) {
        const auto& d = grid.getLevel(0).levelDim;
        throw Error("FMG: the coarse grids of " + std::to_string(d[0]) + " x " + std::to_string(d[1]) + " x " +
                    std::to_string(d[2]) +
                    " do not align with the fine grid (n/2 points per axis instead of (n-1)/2): full multigrid needs "
                    "sizes 2^k - 1 (31, 63, 127, 255, 511, ...) on every axis");
    }
}

void HipSolver::fmgRun(HipGridData& grid, int cyclesPerLevel)
{
    fmgCheck(grid, cyclesPerLevel);
    const hipStream_t s = grid.stream();
    const std::size_t start = fmgStartLevel(grid);
    if (grid.fmgProlongMode == 1) grid.buildFmgTables();
    // f^(l+1) = R f^l from level 0's f as it stands (a V-cycle rooted at level l only writes f below l); restrict()
    // takes gs_restrict_pa on the transitions the grid's POSITION transfers cover
    for (std::size_t l = 0; l < start; l++) restrict(grid, grid.getLevel(l).f, l, grid.getLevel(l + 1).f);
    for (std::size_t l = start + 1; l-- > 0;) {
        auto& L = grid.getLevel(l);
        if (l == start) {
            // the zero iterate: a flag where the first sweep can take it (as the V-cycle's coarse v = 0), else stored
            if (grid.mode != GridParams::NONLINEAR && grid.sw.zeroGuess) {
                L.vZero = true;
            } else {
                L.v.zero(s);
                L.vZero = false;
            }
        } else {
            auto& C = grid.getLevel(l + 1);
            materialize(grid, l + 1);
            if (grid.fmgProlongMode == 1 && !grid.levelAligned(l))
                check(gs_fmg_prolong_pa(C.v.data(), &C.geom, L.v.data(), &L.geom, grid.fmgTables(l), s),
                      "gs_fmg_prolong_pa");
            else
                check(gs_fmg_prolong(C.v.data(), &C.geom, L.v.data(), &L.geom, s), "gs_fmg_prolong");
            L.vZero = false;
        }
        for (int c = 0; c < cyclesPerLevel; c++) vcycleFrom(grid, l);
    }
}

double HipSolver::fmg(HipGridData& grid, int cyclesPerLevel)
{
    fmgRun(grid, cyclesPerLevel);
    return compResidual(grid, 0, false, true);
}

// ---------------------------------------------------------------------------------------------
// Conjugate gradients preconditioned by the V-cycle.

void HipGridData::pcgAlloc()
{
    const std::size_t need = maxiter + 1;
    const gs_level& g0 = levels_[0].geom;
    const char* const what = "PCG: allocating its level-0 fields and scalar record failed";
    double *slots = nullptr, *slotsDev = nullptr;
    if (pcg.slotCap < need) {
        if (hipHostMalloc((void**)&slots, sizeof(double) * GS_PCG_REC * need, hipHostMallocMapped | hipHostMallocCoherent) !=
                hipSuccess ||
            hipHostGetDevicePointer((void**)&slotsDev, slots, 0) != hipSuccess) {
            if (slots) (void)hipHostFree(slots);
            (void)hipGetLastError();
            throw Error(what);
        }
    }
    if (!pcg.rec) {
        double *rec = nullptr, *parts = nullptr;
        hipEvent_t ev = nullptr;
        try {
            DeviceField r(g0.nx, g0.ny, g0.nz, stream_.s), z(g0.nx, g0.ny, g0.nz, stream_.s),
                p0(g0.nx, g0.ny, g0.nz, stream_.s), p1(g0.nx, g0.ny, g0.nz, stream_.s);
            const int64_t np = std::max<int64_t>(
                1, std::max(gs_pcg_dir_num_partials(&stencilAbi, &g0),
                            std::max(gs_pcg_step_num_partials(&g0), gs_dot_num_partials(&g0))));
            if (hipMalloc((void**)&rec, sizeof(double) * GS_PCG_REC) != hipSuccess ||
                hipMalloc((void**)&parts, sizeof(double) * np) != hipSuccess ||
                hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess)
                throw Error(what);
            pcg.r = std::move(r);
            pcg.z = std::move(z);
            pcg.p[0] = std::move(p0);
            pcg.p[1] = std::move(p1);
        } catch (const Error&) {
            if (rec) (void)hipFree(rec);
            if (parts) (void)hipFree(parts);
            if (ev) (void)hipEventDestroy(ev);
            if (slots) (void)hipHostFree(slots);
            (void)hipGetLastError(); // (the failed allocation's sticky error)
            throw Error(what);
        }
        pcg.rec = rec;
        pcg.parts = parts;
        pcg.ev = ev;
    }
    if (slots) {
        if (pcg.slots) {
            check((int)hipStreamSynchronize(stream_.s), "hipStreamSynchronize"); // (no kernel still writes the old one)
            (void)hipHostFree(pcg.slots);
        }
        pcg.slots = slots;
        pcg.slotsDev = slotsDev;
        pcg.slotCap = need;
        pcg.started = -1;
    }
}

// The cycle is a symmetric positive definite preconditioner only under these conditions (tests/test_pcg_cpu.py
// measures the symmetry defect of the model cycle: 1e-15 where they hold, 4.3e-3 with pre = 2, post = 1)
void HipSolver::pcgCheck(const HipGridData& grid)
{
    if (grid.mode != GridParams::LINEAR)
        throw Error("PCG: LINEAR grids only (NONLINEAR and NEWTON are not linear systems)");
    if (grid.nranks() > 1 || grid.trace)
        throw Error("PCG: single-GPU grids only (not a Z-slab / RCCL or schedule-trace grid)");
    if (grid.preSmoothing != grid.postSmoothing || grid.preSmoothing == 0)
        throw Error("PCG: the cycle must smooth symmetrically: pre = post >= 1 (pre = " +
                    std::to_string(grid.preSmoothing) + ", post = " + std::to_string(grid.postSmoothing) + ")");
    if (grid.weighted()) {
        std::vector<double> a(grid.wPre(), grid.wPre() + grid.preSmoothing),
            b(grid.wPost(), grid.wPost() + grid.postSmoothing);
        std::sort(a.begin(), a.end());
        std::sort(b.begin(), b.end());
        if (a != b)
            throw Error("PCG: the post-smoothing weights must be the pre-smoothing weights in some order (the cycle is "
                        "not symmetric otherwise)");
    }
    double wgt[27] = {};
    const gs_stencil& S = grid.stencilAbi;
    for (int i = 0; i < 7; i++) wgt[(S.ox[i] + 1) + 3 * (S.oy[i] + 1) + 9 * (S.oz[i] + 1)] += S.s[i];
    for (int o = 0; o < 27; o++)
        if (!(wgt[o] == wgt[26 - o]))
            throw Error("PCG: the stencil must be symmetric: the weight at every offset o must be the weight at -o");
    // (an XY hierarchy's transfers are by position on every transition: R_xy is the scaled transpose of P_xy)
    if (grid.transferMode == 0 && !grid.xy())
        for (std::size_t l = 0; l + 1 < grid.numLevels(); l++)
            if (!grid.levelAligned(l)) {
                const auto& d = grid.getLevel(0).levelDim;
                throw Error("PCG: the coarse grids of " + std::to_string(d[0]) + " x " + std::to_string(d[1]) + " x " +
                            std::to_string(d[2]) +
                            " do not align and the reference transfers diverge there: "
                            "gs_grid_set_transfer(GS_TRANSFER_POSITION) / GS_TRANSFER=position");
            }
}

namespace {
// level 0's f and v stand in for the residual and the preconditioned residual while the cycle runs; put back on
// every exit
struct PcgSwap {
    HipGridData::LevelData& L;
    HipGridData::PcgState& st;
    const bool vz;
    PcgSwap(HipGridData::LevelData& l, HipGridData::PcgState& s) : L(l), st(s), vz(l.vZero)
    {
        L.f.swap(st.r);
        L.v.swap(st.z);
    }
    ~PcgSwap()
    {
        L.f.swap(st.r);
        L.v.swap(st.z);
        L.vZero = vz;
    }
};
} // namespace

bool HipSolver::pcg(HipGridData& grid, const double* fmgInitial)
{
    pcgCheck(grid);
    grid.pcgAlloc();
    auto& st = grid.pcg;
    auto& L0 = grid.getLevel(0);
    const hipStream_t s = grid.stream();
    const gs_stencil* S = &grid.stencilAbi;
    const gs_level* G = &L0.geom;
    const bool print = grid.printProgress;
    materialize(grid, 0);
    st.started = 0;
    st.breakdown = false;
    // r = f - A x0 and its norm
    check(gs_residual(S, G, GS_LINEAR, grid.gamma, L0.v.data(), L0.f.data(), nullptr, st.r.data(), grid.partials(), s),
          "gs_residual");
    const double res0 = finishNorm(grid, gs_residual_num_partials(S, G));
    const double initialResidual = fmgInitial ? *fmgInitial : res0;
    if (history) history->push_back(res0);
    if (fmgInitial) {
        if (print) {
            std::cout << "fmg: cycles: " << grid.sw.fmg << " residual: " << res0 << ' ';
            Timer::stop();
            Timer::start();
        }
        if (res0 <= initialResidual / (1.0 / grid.tol)) return false;
    } else {
        if (print) std::cout << "Inital residual: " << res0 << '\n';
        if (print) Timer::start();
    }
    // z = M^-1 r (one V-cycle from the zero iterate with r as right-hand side), r . z, and the scalars it decides
    auto tail = [&](bool first) {
        {
            PcgSwap sw(L0, st);
            if (grid.sw.zeroGuess) {
                L0.vZero = true;
            } else {
                L0.v.zero(s);
                L0.vZero = false;
            }
            vcycleFrom(grid, 0);
            materialize(grid, 0);
            grid.clock.segLevel.clear(); // (the per-level clock times the V-cycle loop only)
        }
        check(gs_dot(G, st.r.data(), st.z.data(), st.parts, s), "gs_dot");
        check(gs_pcg_scalars(first ? GS_PCG_RZ_FIRST : GS_PCG_RZ, st.parts, gs_dot_num_partials(G), st.rec, nullptr, s),
              "gs_pcg_scalars");
    };
    tail(true);
    bool tailDone = true;
    int cur = 0; // p[cur]: the direction this iteration writes; p[cur ^ 1]: the previous one
    for (std::size_t k = 0; k < grid.maxiter; k++) {
        if (!tailDone) tail(false);
        double* q = L0.vAlt.data();
        check(gs_pcg_dir(S, G, st.z.data(), k == 0 ? nullptr : st.p[cur ^ 1].data(), st.p[cur].data(), q,
                         st.rec + GS_PCG_BETA_I, st.parts, s),
              "gs_pcg_dir");
        check(gs_pcg_scalars(GS_PCG_PQ, st.parts, gs_pcg_dir_num_partials(S, G), st.rec, nullptr, s), "gs_pcg_scalars");
        check(gs_pcg_step(G, L0.v.data(), st.r.data(), st.p[cur].data(), q, st.rec + GS_PCG_ALPHA_I, st.parts, s),
              "gs_pcg_step");
        check(gs_pcg_scalars(GS_PCG_RR, st.parts, gs_pcg_step_num_partials(G), st.rec, st.slotsDev + GS_PCG_REC * k, s),
              "gs_pcg_scalars");
        check((int)hipEventRecord(st.ev, s), "hipEventRecord");
        st.started = (int)k + 1;
        // the next iteration's cycle, dot product and beta behind the norm the host waits for: they write z, the
        // record and the coarse levels only, so stopping here leaves x and r this iteration's
        const bool ahead = grid.sw.pipeline && k + 1 < grid.maxiter;
        if (ahead) tail(false);
        tailDone = ahead;
        check((int)hipEventSynchronize(st.ev), "hipEventSynchronize");
        const volatile double* slot = st.slots + GS_PCG_REC * k;
        // a breakdown: alpha was 0, so this iteration changed nothing (GS_PCG_BAD_RR: r . r is not finite, the iterate
        // overflowed; the slot's 0 is no norm and must not count as converged)
        if (slot[GS_PCG_FLAG_I] != 0.0) {
            st.breakdown = true;
            break;
        }
        const double res = std::sqrt(slot[GS_PCG_RR_I]);
        if (history) history->push_back(res);
        if (print) {
            std::cout << "iter: " << k << " residual: " << res << ' ';
            Timer::stop();
            Timer::start();
        }
        if (res <= initialResidual / (1.0 / grid.tol)) break;
        cur ^= 1;
    }
    return st.breakdown;
}

double HipSolver::cycleUp0(HipGridData& grid, int* pending, bool wait)
{
    const std::size_t nl = grid.numLevels();
    const hipStream_t s = grid.stream();
    if (std::min(grid.coarseFrom, nl - 1) >= 1) upLeg(grid, 1);
    // the closing norm: the next cycle's first pre-smoothing step (speculative) or a residual pass
    grid.clock.mark(s, 0, true);
    double res;
    if (pending && speculationEnabled(grid)) {
        res = speculativeSweep(grid, pending, wait); // closes the segment before its host sync
    } else {
        res = compResidual(grid, 0, false, true);
        grid.clock.mark(s, 0, false); // after the norm's host sync: over-counts by the sync latency
    }
    return res;
}

double HipSolver::vcycleSpeculative(HipGridData& grid, int* pending)
{
    const auto tWall = std::chrono::steady_clock::now();
    cycleDown(grid, pending);
    const double res = cycleUp0(grid, pending, true);
    if (grid.clock.on) {
        grid.clock.collect();
        grid.clock.cycles++;
        grid.clock.wallMs += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tWall).count();
    }
    return res;
}

// Overlapping cycle i+1's cycleDown with the wait for cycle i's norm is exact only if that work
// leaves level 0's iterate alone: every pre-smoothing sweep is the speculative step's (pre ==
// pending), level 0 is not part of the coarse-cycle launch, and no per-level clock is running.
bool HipSolver::pipelinable(const HipGridData& grid, int pending)
{
    return grid.sw.pipeline && !grid.clock.on && speculationEnabled(grid) && pending > 0 &&
           (std::size_t)pending == grid.preSmoothing && std::min(grid.coarseFrom, grid.numLevels() - 1) >= 1;
}

std::size_t HipSolver::runCycles(HipGridData& grid, int* pending, std::size_t maxCycles,
                                 const std::function<bool(std::size_t, double)>& onNorm, bool lastNormDead)
{
    // (cycle-invariant: every closing speculative step leaves the same number of sweeps pending)
    const bool pipe = pipelinable(grid, *pending);
    bool downDone = false; // this cycle's cycleDown was enqueued during the previous cycle's wait
    for (std::size_t i = 0; i < maxCycles; i++) {
        if (lastNormDead && i + 1 == maxCycles) {
            // the last cycle's closing norm decides nothing and nobody reads it: no speculative pass
            if (!downDone) cycleDown(grid, pending);
            cycleUpNoNorm(grid);
            *pending = 0;
            return maxCycles;
        }
        if (!pipe) {
            if (onNorm(i, vcycleSpeculative(grid, pending))) return i + 1;
            continue;
        }
        if (!downDone) cycleDown(grid, pending);
        cycleUp0(grid, pending, false); // cycle i's closing norm in flight; *pending = its sweeps
        const int next = *pending;
        const bool ahead = i + 1 < maxCycles;
        if (ahead) cycleDown(grid, pending); // adopts the speculative sweeps: *pending = 0
        const double res = grid.readNormEnd();
        if (onNorm(i, res)) {
            if (ahead) { // undo the adoption: level 0 holds cycle i's iterate, vAlt the speculation
                auto& L0 = grid.getLevel(0);
                L0.v.swap(L0.vAlt);
                if (grid.trace) grid.rec("swap", {{"L", 0}});
                *pending = next;
            }
            return i + 1;
        }
        downDone = ahead;
    }
    return maxCycles;
}

void NewtonSolver::solve(HipGridData& grid)
{
    auto& L0 = grid.getLevel(0);
    const hipStream_t s = grid.stream();
    // the reference prints unconditionally (NewtonSolver.cpp:16,27); printProgress defaults to true,
    // so GpuSolve-hip does too, and library callers silence it without touching std::cout
    const bool print = grid.printProgress && grid.rank() == 0;
    if (grid.sw.fmg > 0) HipSolver::fmgCheck(grid, grid.sw.fmg); // GS_FMG: NEWTON throws, before any work
    if (grid.trace)
        grid.rec("copy", {{"L", 0}}, "f>newtonF");
    else
        check(gs_copy(grid.newtonF.data(), L0.f.data(), L0.f.span(), s), "gs_copy");
    const double initialResidual = compF(grid);
    // fields may have been set since the last solve: the first findError restricts level 1 and forms level 0's factor
    // itself, and skips the restrictions of a zero newtonV only if EVERY rank still has it (a rank that handed its
    // newtonV pointer out would restrict, and restrictions exchange ghost planes on distributed levels)
    grid.newtonR1_ = false;
    grid.bfacFresh_ = 0;
    grid.newtonVZero_ = grid.allRanks(grid.newtonVZero_);
    if (history) history->push_back(initialResidual);
    if (print) std::cout << "Inital newton residual: " << initialResidual << '\n';

    for (std::size_t i = 0; i < grid.maxiter; i++) {
        if (print) Timer::start();
        // The reference recomputes compF here (NewtonSolver.cpp:21); f^0 already holds exactly that
        // value from the previous compF and nothing wrote it since, so the pass is skipped.
        // v = 0 (NewtonSolver.cpp:22), not stored: the inner solve's first (speculative) sweep is a
        // zero-iterate kernel that reads no v; anything else that reads v materializes it first
        L0.vZero = true;
        const double res = findError(grid) ? compFUpdate(grid) : compF(grid);
        if (history) history->push_back(res);
        if (print) {
            std::cout << "newton iter: " << i << " residual: " << res << ' ';
            Timer::stop();
        }
        if (res <= initialResidual / (1.0 / grid.tol)) return;
    }
}

// f^0 = newtonF - N(newtonV^0), returns ||f^0||  (NewtonSolver.cpp:48-81)
double NewtonSolver::compF(HipGridData& grid)
{
    auto& L0 = grid.getLevel(0);
    if (grid.trace)
        grid.rec("newtonF", {{"L", 0}});
    else
        check(gs_newton_F(&grid.stencilAbi, &L0.geom, grid.gamma, L0.newtonV.data(), grid.newtonF.data(),
                          L0.f.data(), grid.partials(), grid.stream()),
              "gs_newton_F");
    grid.halo(L0, L0.f, grid.stream());
    return HipSolver::finishNorm(grid, gs_residual_num_partials(&grid.stencilAbi, &L0.geom));
}

// newtonV += v and the compF after it as one pass (gs_newton_F_update) on a level this rank holds whole:
// the sum goes to level 0's vAlt — zero outside the interior like newtonV + v, and dead once the inner
// solve has returned (its pending speculative sweep is dropped; the next inner solve starts from the
// zero iterate) — which then becomes newtonV. Bit-identical to gs_axpy + gs_newton_F.
// On a Z-slab rank the pass reads w and e on the ghost planes 0 and nz+1 (both current: newtonV's from the
// previous update, v's from the inner solve's last exchange) but stores w' only on the owned planes, so
// the new newtonV's ghost planes are formed afterwards as k_axpy would leave them (newtonV + 1.0 v, two
// planes: a copy and an axpy each) — no exchange, bit-identical to the whole-array gs_axpy of the
// two-pass path.
bool NewtonSolver::fusedUpdate(const HipGridData& grid)
{
    const auto& L0 = grid.getLevel(0);
    return grid.sw.newtonFusedUpdate && gs_newton_F_update_supported(&grid.stencilAbi, &L0.geom) != 0;
}

double NewtonSolver::compFUpdate(HipGridData& grid)
{
    auto& L0 = grid.getLevel(0);
    // single GPU: the next findError's restriction of newtonV onto level 1 (NewtonSolver.cpp:88-92) comes out of
    // the same pass (gs_newton_F_update_restrict), so findError skips that 1.1 GB re-read at 512^3
    // (gs_newton_F_update_restrict embeds the index-aligned restriction: not where level 0's transition is position-aware)
    const bool r1 = grid.numLevels() >= 3 && !(L0.distributed && grid.nranks() > 1) && !grid.pa(0) &&
                    (grid.trace || grid.getLevel(1).newtonVNext.data() != nullptr) &&
                    gs_newton_F_update_restrict_supported(&grid.stencilAbi, &L0.geom, &grid.getLevel(1).geom) != 0;
    // the same pass also writes the next inner solve's GS_NEWTON_B factor of level 0 (from the exp(w') compF
    // evaluates anyway): findError then skips that level's gs_newton_bfac pass
    const bool bf = r1 && grid.sw.newtonB && grid.sw.newtonBFused;
    if (grid.trace)
        grid.rec("newtonFupdate", {{"L", 0}, {"restrict", r1}, {"bfac", bf}});
    else if (r1)
        check(gs_newton_F_update_restrict_bfac(&grid.stencilAbi, &L0.geom, grid.gamma, L0.newtonV.data(), L0.v.data(),
                                               grid.newtonF.data(), L0.vAlt.data(), L0.f.data(), grid.partials(),
                                               grid.getLevel(1).newtonVNext.data(), &grid.getLevel(1).geom,
                                               bf ? L0.bfac.data() : nullptr, grid.stream()),
              "gs_newton_F_update_restrict");
    else
        check(gs_newton_F_update(&grid.stencilAbi, &L0.geom, grid.gamma, L0.newtonV.data(), L0.v.data(),
                                 grid.newtonF.data(), L0.vAlt.data(), L0.f.data(), grid.partials(), grid.stream()),
              "gs_newton_F_update");
    grid.newtonR1_ = r1;
    grid.bfacFresh_ = bf ? 1u : 0u;
    grid.newtonVZero_ = false;
    if (L0.distributed && grid.nranks() > 1) {
        // the ghost planes of w' = newtonV + v (see fusedUpdate)
        const int64_t ldz = L0.v.ldz();
        for (const int64_t p : {(int64_t)0, L0.geom.nz + 1}) {
            if (grid.trace) {
                grid.rec("ghostsum", {{"L", 0}, {"plane", (long long)p}}, "vAlt=newtonV+v");
                continue;
            }
            check(gs_copy(L0.vAlt.data() + p * ldz, L0.newtonV.data() + p * ldz, ldz, grid.stream()), "gs_copy");
            check(gs_axpy(L0.vAlt.data() + p * ldz, L0.v.data() + p * ldz, 1.0, ldz, grid.stream()), "gs_axpy");
        }
    }
    L0.newtonV.swap(L0.vAlt);
    if (grid.trace) grid.rec("swapnewton", {{"L", 0}});
    grid.halo(L0, L0.f, grid.stream());
    return HipSolver::finishNorm(grid, gs_residual_num_partials(&grid.stencilAbi, &L0.geom));
}

// NewtonSolver.cpp:83-108
bool NewtonSolver::findError(HipGridData& grid)
{
    // newtonV is still the zero every level's field was created with (the first Newton iteration): its
    // restrictions are those zeros (nothing to compute) and every factor is B = gamma (1 + 0) exp(0) = gamma
    const bool zeroW = grid.newtonVZero_;
    for (std::size_t i = 1; !zeroW && i + 1 < grid.numLevels(); i++) {
        if (i == 1 && grid.newtonR1_) { // restricted by the last compFUpdate; level 0's newtonV unchanged since
            grid.getLevel(1).newtonV.swap(grid.getLevel(1).newtonVNext);
            if (grid.trace) grid.rec("swapnewton", {{"L", 1}});
            grid.newtonR1_ = false;
            continue;
        }
        HipSolver::restrict(grid, grid.getLevel(i - 1).newtonV, i - 1, grid.getLevel(i).newtonV);
    }
    // GS_NEWTON_B: every level's factor B = gamma (1 + w) exp(w) of the newtonV the inner solve linearises at
    // (whole local arrays, ghost planes included: each level's newtonV ghosts are current here), so its ten
    // V-cycles evaluate no exp(newtonV) (include/gpusolve_hip.h)
    if (grid.sw.newtonB) {
        for (std::size_t i = 0; i < grid.numLevels(); i++) {
            auto& L = grid.getLevel(i);
            if (i < 32 && (grid.bfacFresh_ >> i) & 1u) continue; // written by the last compFUpdate pass
            if (grid.trace) grid.rec("bfac", {{"L", (long long)i}});
            else if (zeroW) // (planes -1 .. nz+2, as gs_newton_bfac covers)
                check(gs_fill(L.bfac.data() - L.bfac.ldz(), grid.gamma * (1 + 0.0) * std::exp(0.0),
                              L.bfac.ldz() * (L.geom.nz + 4), grid.stream()),
                      "gs_fill");
            else check(gs_newton_bfac(&L.geom, grid.gamma, L.newtonV.data(), L.bfac.data(), grid.stream()), "gs_newton_bfac");
        }
        grid.newtonB_ = true;
        grid.bconst_ = zeroW && grid.sw.newtonG; // B = gamma everywhere: GS_NEWTON_G
    }
    grid.bfacFresh_ = 0;

    const bool keepPrint = grid.printProgress;
    grid.printProgress = false;
    const std::size_t origIter = grid.maxiter;
    const double origTol = grid.tol;
    grid.maxiter = 10;
    grid.tol = 0.1;
    std::vector<double>* keep = HipSolver::history;
    HipSolver::history = nullptr;
    try {
        HipSolver::solve(grid);
    } catch (...) {
        grid.newtonB_ = grid.bconst_ = false;
        throw;
    }
    grid.newtonB_ = grid.bconst_ = false; // newtonV changes next (newtonV += v): the factors are stale from here on
    HipSolver::history = keep;
    grid.printProgress = keepPrint;
    grid.maxiter = origIter;
    grid.tol = origTol;

    if (fusedUpdate(grid)) return true; // compFUpdate adds v
    auto& L0 = grid.getLevel(0);
    // whole local array, ghost planes included: both operands' ghosts are current, so the sum's are
    if (grid.trace) grid.rec("axpy", {{"L", 0}}, "newtonV+=v");
    else check(gs_axpy(L0.newtonV.data(), L0.v.data(), 1.0, L0.v.span(), grid.stream()), "gs_axpy");
    grid.newtonR1_ = false;
    grid.newtonVZero_ = false;
    return false;
}

// "[gs] mlups=... gbps=... pct_peak=... vcycle_ms=... cycles=... level_ms=a,b,..." over the V-cycles
// timed so far (GS_METRICS). mlups: level-0 smoother updates ((pre+post) x N0 per cycle) per second of
// V-cycle wall time; gbps: SURVEY.md §8(d)'s compulsory V-cycle traffic model, per level N_l points
// ((pre+post) x 24 B + 16 B residual/restriction + 16 B prolongation/correction + 2 B coarse, the
// coarsest level only its sweeps) + 16 B x N0 for the closing norm, per second; pct_peak against
// 8000 GB/s. level_ms: device time per level and cycle. Does not match runExperiments.py:46's regex.
std::string metricsLine(const HipGridData& grid)
{
    const LevelClock& c = grid.clock;
    if (c.cycles == 0) return "[gs] no V-cycle timed";
    const double ms = c.wallMs / c.cycles;
    const double sweeps = (double)(grid.preSmoothing + grid.postSmoothing);
    double bytes = 0.0;
    const std::size_t nl = grid.numLevels();
    for (std::size_t l = 0; l < nl; l++) {
        const auto& d = grid.getLevel(l).levelDim;
        const double n = (double)d[0] * (double)d[1] * (double)d[2];
        bytes += n * (sweeps * 24.0 + (l + 1 < nl ? 34.0 : 0.0));
    }
    const auto& d0 = grid.getLevel(0).levelDim;
    const double n0 = (double)d0[0] * (double)d0[1] * (double)d0[2];
    bytes += 16.0 * n0;
    const double gbps = bytes / (ms * 1e-3) / 1e9;
    char buf[256];
    std::snprintf(buf, sizeof buf, "[gs] mlups=%.1f gbps=%.1f pct_peak=%.1f vcycle_ms=%.3f cycles=%d level_ms=",
                  sweeps * n0 / (ms * 1e-3) / 1e6, gbps, 100.0 * gbps / 8000.0, ms, c.cycles);
    std::string out = buf;
    for (std::size_t l = 0; l < c.levelMs.size(); l++) {
        std::snprintf(buf, sizeof buf, "%s%.4f", l ? "," : "", c.levelMs[l] / c.cycles);
        out += buf;
    }
    return out;
}

void dumpField(HipGridData& grid, std::size_t level, const std::string& path)
{
    auto& L = grid.getLevel(level);
    HipSolver::materialize(grid, level);
    const gs_level& g = L.geom;
    const std::size_t px = (std::size_t)g.nx + 2, py = (std::size_t)g.ny + 2, pz = (std::size_t)g.nz + 2;
    std::vector<double> host(px * py * pz);
    check((int)hipStreamSynchronize(grid.stream()), "hipStreamSynchronize");
    check((int)hipMemcpy2D(host.data(), sizeof(double) * px, L.v.data(), sizeof(double) * (std::size_t)g.ldy,
                           sizeof(double) * px, py * pz, hipMemcpyDeviceToHost),
          "hipMemcpy2D");
    if (gs_dump_write(host.data(), (int64_t)px, (int64_t)py, (int64_t)pz, path.c_str()) != 0)
        throw Error(gs_last_error());
}

} // namespace gs
