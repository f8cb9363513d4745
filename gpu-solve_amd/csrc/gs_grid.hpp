// gs_grid.hpp — device-resident level hierarchy (HipGridData) and the V-cycle / Newton drivers.
//
// Mirrors the reference backend contract:
//   CpuGridData  (src/cpu/CpuGridData.{h,cpp})  -> gs::HipGridData
//   CpuSolver    (src/cpu/CpuSolver.{h,cpp})     -> gs::HipSolver   (solve, restrict public)
//   NewtonSolver (src/cpu/NewtonSolver.{h,cpp})  -> gs::NewtonSolver
// All fields live in HBM for the whole solve; the only device->host traffic per V-cycle is the
// 8-byte residual norm.
//
// Multi-GPU (new; the reference has none): with a Comm of size > 1 each level is either Z-slab
// partitioned (local planes + one ghost plane per side, kept current after every write of a field
// that is read with neighbours) or replicated below the agglomeration threshold.
#pragma once
#include <array>
#include <cstddef>
#include <cstdint>
#include <initializer_list>
#include <memory>
#include <string>
#include <functional>
#include <vector>

#include "gpusolve_hip.h"
#include "gpusolve_transfer.h"
#include "gpusolve_line.h"
#include "gpusolve_semi.h"
#include "gs_comm.hpp"
#include "gs_params.hpp"

namespace gs {

void check(int code, const char* what); // throws gs::Error with gs_strerror(code)

// One padded fp64 field in the pitched x-fastest layout of include/gpusolve_hip.h.
class DeviceField {
public:
    DeviceField() = default;
    DeviceField(int64_t nx, int64_t ny, int64_t nz, hipStream_t s, bool dry = false); // zero-filled
    // dry: the layout without device memory (schedule tracing, HipGridData's trace mode)
    ~DeviceField();
    DeviceField(const DeviceField&) = delete;
    DeviceField& operator=(const DeviceField&) = delete;
    DeviceField(DeviceField&& o) noexcept { *this = std::move(o); }
    DeviceField& operator=(DeviceField&& o) noexcept;

    double* data() const { return origin_; }
    int64_t ldy() const { return ldy_; }
    int64_t ldz() const { return ldz_; }
    int64_t span() const { return span_; } // elements from origin covering every padded point
    explicit operator bool() const { return base_ != nullptr || dry_; }
    void zero(hipStream_t s);
    void swap(DeviceField& o) noexcept;

private:
    double* base_ = nullptr;
    double* origin_ = nullptr;
    int64_t ldy_ = 0, ldz_ = 0, span_ = 0, alloc_ = 0;
    bool dry_ = false;
};

// A plain device buffer of doubles (workspaces), grown on demand.
class DeviceBuf {
public:
    DeviceBuf() = default;
    ~DeviceBuf();
    DeviceBuf(const DeviceBuf&) = delete;
    DeviceBuf& operator=(const DeviceBuf&) = delete;
    double* get(int64_t elems); // at least elems doubles (reallocated when larger; contents not kept)
    int64_t size() const { return n_; }

private:
    double* p_ = nullptr;
    int64_t n_ = 0;
};

struct StreamGuard {
    hipStream_t s = nullptr;
    // high: the device's greatest stream priority (the exchange path: boundary planes, ghost copies)
    explicit StreamGuard(bool create = true, bool high = false);
    ~StreamGuard();
};

// Per-level device time of the V-cycles (GS_METRICS=1 when the grid is created): HIP events around every level's
// down-leg (smoothing, residual + restriction) and up-leg (prolongation + smoothing) work on the
// compute stream, read back after each cycle's norm sync. Off: no event is recorded.
struct LevelClock {
    bool on = false;
    int cycles = 0;
    double wallMs = 0.0;         // host wall time of the V-cycles (norm readbacks included)
    std::vector<double> levelMs; // device ms per level, summed over cycles
    std::vector<hipEvent_t> ev;  // ev[2k], ev[2k+1] bracket segment k of the current cycle
    std::vector<int> segLevel;   // level of segment k
    void mark(hipStream_t s, int level, bool begin);
    void collect();              // after a host sync: add this cycle's segments
    ~LevelClock();
};

class HipGridData final : public GridParams {
public:
    struct LevelData {
        DeviceField v;       // current iterate
        DeviceField vAlt;    // Jacobi ping-pong partner (the fused sweep reads v, writes vAlt)
        DeviceField restV;   // restricted v (FAS)
        DeviceField newtonV; // Newton linearisation point
        DeviceField newtonVNext; // (level 1, single GPU) R(level 0's newtonV) from the last compF update, swapped
                                 // in by the next findError — until then newtonV keeps the reference's value
        DeviceField f;       // right-hand side
        DeviceField r;       // residual (restriction source)
        DeviceField bfac;    // NEWTON (GS_NEWTON_B): B = gamma (1 + newtonV) exp(newtonV) of the inner solve's
                             // linearisation point, set by findError (gs_newton_bfac)
        std::array<std::size_t, 3> levelDim{}; // global interior extents
        double h = 0.0;
        gs_level geom{};     // kernel-side geometry of the stored array (slab or full level)
        gs_stencil sten{};   // the level's stencil: the configuration's on every level of an XYZ hierarchy, the
                             // re-discretised one (gs_semi_level_stencil) on level l of an XY hierarchy
        bool line = false;   // the level smooths with z-line sweeps (setSmoother)
        bool distributed = false;
        bool fusedPairs = false; // smoothing runs as fused sweep pairs (gs_jacobi_sweep2)
        bool fusedTriples = false; // long LINEAR sweep sequences run as fused triples (gs_jacobi_sweep3)
        int64_t triplesRun = 0;    // fused triples launched on this level so far (gs_grid_level_triples)
        bool vZero = false;      // v is identically zero but not stored: the next sweep reads no v
        bool tiled = false;      // small LINEAR level: down- and up-leg steps as one tiled launch each
        int64_t lo = 1, hi = 0; // this rank's owned global planes (== 1..nz when not distributed)
        int64_t minPlanes = 0;  // fewest planes any rank owns on this level
        std::vector<int64_t> ranksLo, ranksHi; // every rank's owned planes (gather of replicated levels)
        // workspaces of the fused prolongation pair on column-block rows (gs_jacobi_sweep2_prolong_ws):
        // [0] for launches on the compute stream, [1] on the boundary stream (they run concurrently)
        std::unique_ptr<DeviceBuf[]> proWs = std::make_unique<DeviceBuf[]>(2);
    };

    // comm == nullptr or comm->size() == 1: the single-GPU path. The grid does not own comm.
    // trace != nullptr: schedule-trace mode — no device is touched; every kernel launch, ghost
    // exchange, gather, norm reduction, swap and zeroing the solvers would issue is appended to *trace
    // as one "op key=value ..." line instead (gs_zslab_schedule; replayed by tests/test_zslab_cpu.py
    // with the oracle's arithmetic on gloo ranks).
    // coarsen: GS_COARSEN_XYZ (0), GS_COARSEN_XY (1), or -1: what GS_COARSEN says (xyz without it).
    explicit HipGridData(const GridParams& grid, Comm* comm = nullptr, int64_t agglomeratePoints = -1,
                         std::vector<std::string>* trace = nullptr, int coarsen = -1);
    ~HipGridData();

    LevelData& getLevel(std::size_t l) { return levels_[l]; }
    const LevelData& getLevel(std::size_t l) const { return levels_[l]; }
    std::size_t numLevels() const { return levels_.size(); }

    DeviceField newtonF;  // Newton: the original right-hand side (src/cpu/CpuGridData.h:36)
    gs_stencil stencilAbi{};
    hipStream_t stream() const { return stream_.s; }
    hipStream_t commStream() const { return commStream_.s; }
    Comm* comm() const { return comm_; }
    int rank() const { return comm_ ? comm_->rank() : 0; }
    int nranks() const { return comm_ ? comm_->size() : 1; }
    bool overlapHalo = true; // boundary planes first, halo on the comm stream beside the interior
    // Alternative-path switches, read from the environment once, when the grid is created (never on a
    // launch path); the defaults are the measured choices. Tests pin every alternative bit-identical.
    struct Switches {
        bool fusedSweeps = true;   // GS_NO_FUSED_SWEEPS: one-sweep kernels only
        bool speculation = true;   // GS_NO_SPECULATION: the closing norm from a residual pass
        bool fusedProlong = true;  // GS_NO_FUSED_PROLONG: gs_prolong_add + the plain pair
        bool fusedRR = true;       // GS_NO_FUSED_RR: residual stored, then restricted
        bool zeroGuess = true;     // GS_NO_ZERO_GUESS: coarse v = 0 stored instead of flagged
        bool pipeline = true;      // GS_NO_PIPELINE: no overlap of the norm wait with the next cycle
        bool newtonFusedUpdate = true; // GS_NO_NEWTON_FUSED_UPDATE: newtonV += v, then compF (two passes)
        bool newtonB = true; // GS_NO_NEWTON_B: inner Newton solves read newtonV (GS_NEWTON) instead of the
                             // precomputed factor B (GS_NEWTON_B: exp(newtonV) once per point and Newton iteration)
        bool newtonBFused = true; // GS_NEWTON_B_FUSED=0: level 0's factor from its own gs_newton_bfac pass instead
                                  // of the compF update pass (bit-identical)
        bool newtonG = true; // GS_NO_NEWTON_G: the first Newton iteration's inner solve reads its factor fields (all
                             // gamma) instead of taking gamma in the pairs and k_rr2 (GS_NEWTON_G; bit-identical)
        int64_t tilePoints = (int64_t)1 << 18; // GS_TILE_POINTS: levels of at most this many points (replicated,
                                               // LINEAR) run the tiled one-launch down/up-leg steps; 0 = off
        int64_t newtonProPoints = (int64_t)1 << 21; // GS_NEWTON_PRO_POINTS: NEWTON levels take the fused
                                                     // prolongation pair from this many points per rank (r06: 2^21,
                                                     // 128^3 too, was 2^24)
        bool sweep3 = true; // GS_NO_SWEEP3: no fused triples (gs_jacobi_sweep3) in LINEAR sweep sequences
        int64_t sweep3MinPoints = (int64_t)1 << 26; // GS_SWEEP3_MIN_POINTS: levels take triples from this many points
                                                     // (2^26: the levels whose pair runs one round of blocks)
        // GS_HALO_ORDER: in a pipelined Z-slab sweep sequence, interior k goes before boundary k when
        // exchange k-1 has not settled on the host yet (0, adaptive), always (1), or never (2: boundary first)
        int haloOrder = 0;
        // GS_FMG=k (default 0, off): HipSolver::solve starts with a full-multigrid pass of k V-cycles per level
        // (HipSolver::fmg) before its first V-cycle — with GS_OMEGAS (weights, below) the switches that change the
        // iterate
        int fmg = 0;
        // GS_SOLVER=pcg|vcycle (default vcycle): HipSolver::solve on a LINEAR grid runs HipSolver::pcg — conjugate
        // gradients preconditioned by the V-cycle — instead of the V-cycle loop (after GS_FMG: from FMG's iterate)
        int solver = 0;
    } sw;
    // Per-sweep relaxation weights (gs_grid_set_weights, GS_OMEGAS): preSmoothing pre weights followed by
    // postSmoothing post weights; empty (the default): every sweep takes omega. On every level the k-th
    // pre-smoothing sweep of a V-cycle takes pre[k], the k-th post-smoothing sweep post[k], the coarsest level's
    // pre + post sweeps the whole sequence. HipSolver::jacobi called without a cursor (gs_grid_jacobi) keeps omega.
    std::vector<double> weights;
    bool weighted() const { return !weights.empty(); }
    const double* wPre(std::size_t k = 0) const { return weights.empty() ? nullptr : weights.data() + k; }
    const double* wPost(std::size_t k = 0) const { return weights.empty() ? nullptr : weights.data() + preSmoothing + k; }
    // counts must equal preSmoothing / postSmoothing and be at most GS_MAX_WEIGHTS, every weight finite;
    // (NULL, 0, NULL, 0) clears. Throws, leaving the weights as they were.
    void setWeights(const double* pre, int npre, const double* post, int npost);
    // Grid transfers (gs_grid_set_transfer, GS_TRANSFER). 0, the default: the reference's index-aligned restrict /
    // interpolate on every transition. 1 (POSITION): every transition that is not aligned (fine n = 2 coarse n + 1 on
    // all three axes) takes the position-aware operators of include/gpusolve_transfer.h through the general path
    // (sweeps, gs_residual_restrict_pa, gs_restrict_pa, gs_prolong_add_pa, sweeps); the tiled steps, k_rr2, the fused
    // prolongation pairs and gs_newton_F_update_restrict embed the index-aligned operator and are not taken there,
    // and the one-launch coarse cycle starts only where every transition below is aligned. Aligned transitions are
    // unchanged launch for launch. With the other two (GS_FMG, GS_OMEGAS) the switches that change the iterate.
    int transferMode = 0;
    // single-GPU grids only; builds and uploads the tables of every non-aligned transition the first time POSITION is
    // switched on. Throws, leaving the grid as it was.
    void setTransfer(int mode);
    bool levelAligned(std::size_t l) const; // the transition l -> l + 1 (l + 1 < numLevels())
    bool pa(std::size_t l) const { return !xy() && transferMode == 1 && !levelAligned(l); }
    const gs_transfer_tables* xfer(std::size_t l) const { return &xferT_[l]; }
    // The smoother (gs_grid_set_smoother, GS_SMOOTHER). 0, the default (JACOBI): damped point Jacobi,
    // every launch as before. 1 (ZLINE): HipSolver::jacobi runs one gs_zline_sweep (include/gpusolve_line.h) per sweep,
    // v -> vAlt and a swap, NULL while vZero holds, omega from the weight cursor where weights are set. Everything that
    // embeds point Jacobi is then not taken — the fused pairs and triples, the fused prolongation pair, the tiled
    // steps, the one-launch coarse cycle (coarseFrom = numLevels()) and the speculative closing norm, with it the
    // overlap of the norm wait with the next cycle: the norm comes from a residual pass, as under GS_NO_SPECULATION.
    // What does not depend on the smoother stays: gs_residual_restrict, gs_prolong_add, the _pa launchers, the
    // zero-guess flag. LINEAR single-GPU grids whose stencil gs_zline_supported accepts; with GS_TRANSFER, GS_FMG and
    // GS_OMEGAS the switches that change the iterate.
    // 2 (AUTO): level l runs z-line sweeps where the largest |z weight| of its stencil (LevelData::sten) is strictly
    // greater than its largest |x / y weight|, the point path otherwise: all or nothing on an XYZ hierarchy, whose
    // levels share one stencil; on an XY hierarchy typically the point kernels on the fine levels and lines below.
    // A line level takes none of the steps that embed point Jacobi, a point level keeps its fused pairs and triples;
    // the fused prolongation pair and the tiled steps are taken where the level they smooth is a point level (and the
    // hierarchy is XYZ). One line level anywhere: no one-launch coarse cycle. The closing norm is speculated, and the
    // norm wait overlapped, exactly when level 0 is a point level (the speculative step is a level-0 point sweep).
    int smootherMode = 0;
    bool anyLine = false; // some level is a line level
    bool lineAt(std::size_t l) const { return levels_[l].line; }
    // builds (gs_zline_factors, from the level's own stencil) and uploads the factors of every line level that has
    // none yet; they are freed with the grid. Throws, leaving the grid as it was (zlineCheck: what a refusal says).
    void setSmoother(int mode);
    void zlineCheck(const char* name = "ZLINE") const; // LINEAR, single GPU, level 0's stencil supported (ZLINE)
    // The coarsening (gs_grid_create_coarsen, GS_COARSEN), fixed at creation. 0 (XYZ), the default:
    // every axis halves per level. 1 (XY): x and y halve, nz stays; nlev = floor(log2(min(nx, ny))) + 1; level l has
    // the stencil gs_semi_level_stencil gives for its h; every transition takes the general path with the _xy
    // launchers of include/gpusolve_semi.h (tables of axes 0 and 1 built and uploaded at creation), whatever
    // transferMode says — the fused prolongation pair, the tiled steps and the one-launch coarse cycle embed 3-D
    // transfers and one stencil for several levels and are not taken; FMG is refused. LINEAR single-GPU grids whose
    // stencil is the seven axis offsets, min(nx, ny) >= 2.
    int coarsen = 0;
    bool xy() const { return coarsen == 1; }
    const gs_zline_tables* zlineTables(std::size_t l) const { return &zlineT_[l]; }
    // Full multigrid's prolongation (gs_grid_set_fmg_prolong, GS_FMG_PROLONG). 0, the default (ALIGNED): gs_fmg_prolong
    // on aligned transitions only, so FMG starts at the deepest level above which every transition is aligned and is
    // refused where that is level 0. 1 (POSITION): FMG starts at the coarsest level; an aligned transition keeps
    // gs_fmg_prolong, every other one takes gs_fmg_prolong_pa (and needs the POSITION transfers for its V-cycles:
    // fmgCheck). NEWTON, Z-slab and trace grids keep the mode and stay refused by FMG.
    int fmgProlongMode = 0;
    // builds and uploads the tables of every non-aligned transition the first time POSITION is switched on (on a grid
    // FMG can run on). Throws, leaving the grid as it was.
    void setFmgProlong(int mode);
    void buildFmgTables(); // (no-op once built, or where FMG is refused anyway)
    const gs_fmg_tables* fmgTables(std::size_t l) const { return &fmgT_[l]; }
    // where the position-aware path is taken, f^2h = R(f^h - A v^h) in one pass (gs_residual_restrict_pa) rather
    // than gs_residual with a stored r followed by gs_restrict_pa (DESIGN.md §4.9 has the A/B)
    static constexpr bool paFusedRR = true;
    // levels coarseFrom .. numLevels()-1 run as ONE gs_coarse_cycle launch in every V-cycle
    // (numLevels(): none); set from GS_COARSE_POINTS at construction
    std::size_t coarseFrom = 0;
    // HipSolver::pcg's state, allocated by its first call (pcgAlloc: all of it or nothing): four
    // level-0 fields beside the hierarchy's — the residual r, the preconditioned residual z, the direction and the
    // previous direction (q = A p lives in level 0's vAlt, which is dead outside a cycle) —, the device-resident
    // scalar record, its own partial sums and the mapped, coherent pinned history (one slot per iteration: the
    // norm-word pattern of hNorm_), from which gs_grid_pcg_record reads the last run
    struct PcgState {
        DeviceField r, z, p[2];
        double* rec = nullptr;      // device: GS_PCG_REC doubles
        double* parts = nullptr;    // device: the three passes' partial sums
        double* slots = nullptr;    // pinned host: GS_PCG_REC doubles per iteration
        double* slotsDev = nullptr; // ... as the device sees it
        std::size_t slotCap = 0;
        int started = -1;           // iterations the last run started (-1: no run yet)
        bool breakdown = false;     // ... and whether it ended in a breakdown
        hipEvent_t ev = nullptr;
    } pcg;
    void pcgAlloc(); // throws, leaving the state as it was
    LevelClock clock; // per-level timing (GS_METRICS)
    std::vector<std::string>* trace = nullptr; // schedule-trace mode (see the constructor)
    void rec(const char* op, std::initializer_list<std::pair<const char*, long long>> kv, const char* field = nullptr);
    std::size_t levelIndex(const LevelData& L) const { return (std::size_t)(&L - levels_.data()); }
    static const char* fieldName(const LevelData& L, const DeviceField& f);

    // residual-norm plumbing: per-block partials, device scalars, pinned host scalar
    double* partials() const { return partials_; }
    double* dNorm() const { return dNorm_; }       // this rank's sum of squares (distributed norms)
    double* hNormDev() const { return hNormDev_; } // the pinned norm word, as the finishing kernel writes it
    double* dRankSums() const { return dRankSums_; }
    double readNorm(); // stream sync + the pinned norm word: the one host sync per V-cycle
    // the same in two halves: an event now, the (bounded) wait for the event later, so
    // that more work can be enqueued in between
    void readNormBegin();
    double readNormEnd();
    void sync();       // stream sync (bounded, error-polling when distributed over RCCL)

    // the mode and the w operand the V-cycle's kernels take: GS_NEWTON_B and B while findError's inner solve runs
    // with the factor fields current (newtonB_), else the grid's mode and newtonV (reference expressions)
    int kmode() const { return newtonB_ ? (bconst_ ? (int)GS_NEWTON_G : (int)GS_NEWTON_B) : (int)mode; }
    const double* wOf(const LevelData& L) const
    {
        return newtonB_ ? L.bfac.data() : (L.newtonV ? L.newtonV.data() : nullptr);
    }
    // newtonV may have been written from outside the solvers (the C ABI's writable field pointer or an upload):
    // nothing derived from it may be reused — not the zero-field shortcut (newtonVZero_), nor level 1's restriction
    // (newtonR1_) or level 0's factor (bfacFresh_) that the last update pass wrote
    void newtonVTouched()
    {
        newtonVZero_ = false;
        newtonR1_ = false;
        bfacFresh_ = 0;
    }
    // AND of `flag` over every rank of a distributed grid (an allgather of one word; the flag itself elsewhere), so
    // that a schedule decision taken from per-process state issues the same collectives on every rank
    bool allRanks(bool flag);
    // ghost planes of a distributed level's field (no-op otherwise); depth 2 where possible for
    // iterate fields (the fused pair reads two ghost planes of v)
    void halo(LevelData& L, DeviceField& fld, hipStream_t s, int depth = 1);
    // the same in halves (the pipelined sweep sequence, HipSolver::jacobi): haloIssue starts the exchange,
    // haloSettle() returns once its kernels are on s (only then may an event be recorded after it);
    // haloReady(): one poll of an issued exchange (trace mode: GS_HALO_ORDER decides, see Switches)
    void haloIssue(LevelData& L, DeviceField& fld, hipStream_t s, int depth);
    bool haloReady();
    void haloSettle();
    double haloHostMs = 0.0;    // host wall time spent issuing and settling ghost exchanges, summed
    double haloHostMaxMs = 0.0; // ... the largest for one exchange (issue + polls + settle)
    int64_t haloCalls = 0;
    int vDepth(const LevelData& L) const { return L.minPlanes >= 2 ? 2 : 1; }
    // replicated level fed from a distributed parent: assemble every rank's owned planes
    void gather(LevelData& L, DeviceField& fld);
    // geometry + pointer offset of the planes this rank computes on level L
    gs_level ownedGeom(const LevelData& L, int64_t* planeOffset) const;

private:
    std::vector<LevelData> levels_;
    Comm* comm_ = nullptr;
    StreamGuard stream_;
    StreamGuard commStream_;
    StreamGuard bndStream_; // boundary planes of an overlapped Z-slab sweep (distributed grids only)
    double* partials_ = nullptr;
    double* dNorm_ = nullptr;
    double* dRankSums_ = nullptr;
    double* hNorm_ = nullptr;
    double* hNormDev_ = nullptr;
    hipEvent_t evA_ = nullptr, evB_ = nullptr, evC_ = nullptr, evNorm_ = nullptr;
    hipEvent_t evBnd_[2] = {nullptr, nullptr}; // boundary planes of sweep k (k & 1) in a pipelined sequence
    std::vector<double> dryParts_;
    long traceNorms_ = 0;
    std::size_t coarseFromRef_ = 0;          // coarseFrom of the REFERENCE transfers (GS_COARSE_POINTS' rule)
    std::vector<gs_transfer_tables> xferT_;  // per transition l -> l + 1; null pointers where aligned or not built
    std::vector<gs_fmg_tables> fmgT_;        // the same for gs_fmg_prolong_pa
    std::vector<gs_zline_tables> zlineT_;    // per level: the z-line factors (null pointers until ZLINE is first set)
    std::vector<void*> xferMem_;             // the device allocations behind all three
    gs_transfer_tables uploadTransferTables(std::size_t l, int axes); // transition l -> l + 1 (3 axes, or x / y)
    void buildXyTables();                    // the x / y tables of every transition of an XY hierarchy (creation)
    void updateCoarseFrom();                 // coarseFrom from coarseFromRef_, the transfers and the smoother
    bool haloPending_ = false; // an exchange issued by haloIssue, not settled
    friend class NewtonSolver;
    bool newtonR1_ = false;    // level 1's newtonVNext holds R(level 0's newtonV) (gs_newton_F_update_restrict)
    bool newtonB_ = false;     // every level's bfac holds B of its current newtonV (set for the inner solve)
    bool bconst_ = false;      // ... and that B is gamma everywhere (newtonV = 0, the first iteration): GS_NEWTON_G
    unsigned bfacFresh_ = 0;   // bit l: level l's bfac already holds B of the newtonV the next findError uses
    bool newtonVZero_ = false; // every level's newtonV is still the zero of grid creation (the first findError)
    double haloCurMs_ = 0.0;   // host ms spent on that exchange so far
    double traceNorm();
    friend class HipSolver;
};

class HipSolver {
public:
    static void solve(HipGridData& grid);
    static void restrict(HipGridData& grid, const DeviceField& src, std::size_t srcLevel, DeviceField& dst);

    // exposed for benchmarks / the C ABI
    static double compResidual(HipGridData& grid, std::size_t level, bool storeR, bool norm);
    static double vcycle(HipGridData& grid);
    // The solve loop's V-cycle: with speculation on, a cycle's closing norm comes out of the first
    // pre-smoothing step of the next cycle (same residual, computed by that step anyway: one sweep
    // or a fused pair), run into vAlt without swapping; *pending = how many sweeps vAlt holds (0:
    // none), and the next cycle adopts them.
    static double vcycleSpeculative(HipGridData& grid, int* pending);
    // vcycleSpeculative in two halves: cycleDown enqueues everything that leaves level 0's iterate
    // untouched (adopting the pending speculative sweeps, every down-leg, the coarse end, the up-legs
    // of levels >= 1); cycleUp0 enqueues level 0's up-leg and the closing norm, and waits for the norm
    // only if `wait` (else the caller collects it with grid.readNormEnd()).
    static void cycleDown(HipGridData& grid, int* pending);
    static double cycleUp0(HipGridData& grid, int* pending, bool wait);
    // cycleDown rooted at level `from` (cycleDown is from = 0): the down-legs from..., the coarse end — the one
    // gs_coarse_cycle launch from max(from, coarseFrom) on, or the coarsest level's sweeps — and the up-legs of the
    // levels above from + 1
    static void downFrom(HipGridData& grid, std::size_t from, int* pending);
    // One V-cycle rooted at `level` (its f and v set): the levels above it are not touched, no norm is taken and
    // nothing is speculated or pipelined. The levels take the fused, tiled and coarse-launch paths they take in a
    // whole V-cycle.
    static void vcycleFrom(HipGridData& grid, std::size_t level);
    // Full multigrid (nested iteration; not in the reference): every level's f becomes the full-weighting
    // restriction of level 0's f as it stands; the start level s (fmgStartLevel) is iterated from zero and each
    // finer level from the tricubic prolongation (gs_fmg_prolong) of the level below, cyclesPerLevel V-cycles
    // each. Overwrites v on every level; returns the level-0 residual norm. LINEAR and NONLINEAR (FAS) grids on
    // one GPU whose coarse grids align (sizes 2^k - 1); otherwise throws before any work (fmgCheck). With
    // grid.fmgProlongMode POSITION: every size, from the coarsest level, non-aligned transitions prolonged by
    // gs_fmg_prolong_pa and restricted by gs_restrict_pa (the grid's transfers must be POSITION where one exists).
    static double fmg(HipGridData& grid, int cyclesPerLevel);
    // Conjugate gradients preconditioned by one V-cycle (vcycleFrom(0) from a zero iterate on the residual) on a
    // LINEAR single-GPU grid whose cycle is symmetric (pcgCheck throws otherwise, before any work): from level 0's
    // v as it stands, at most maxiter iterations, solve's stopping rule, history and print lines. fmgInitial: the
    // norm solve() took before its GS_FMG pass (the tolerance's reference; the first norm then has FMG's line).
    // Returns whether the run ended in a breakdown (p.q or r.z not a positive finite number).
    static bool pcg(HipGridData& grid, const double* fmgInitial = nullptr);
    static void pcgCheck(const HipGridData& grid);
    // the deepest level such that every transition above it is gs_fmg_prolong_supported (POSITION prolongation: the
    // coarsest level); 0: FMG not applicable
    static std::size_t fmgStartLevel(const HipGridData& grid);
    static void fmgCheck(const HipGridData& grid, int cyclesPerLevel); // throws what fmg would
    static void fmgRun(HipGridData& grid, int cyclesPerLevel);         // fmg without the closing norm
    // Up to maxCycles V-cycles with the host's wait for cycle i's norm overlapped with cycle i+1's
    // cycleDown (when pipelinable): onNorm(i, res) gets each closing norm in order and returns true
    // to stop — the early-enqueued work then only wrote coarse levels and scratch, and the adoption
    // of the speculative level-0 sweeps is undone, so level 0 holds cycle i's iterate exactly as
    // without the overlap. *pending: the speculative sweeps vAlt holds on entry and on return.
    // lastNormDead: the last cycle's closing norm is not computed (nobody reads it, see solve())
    static std::size_t runCycles(HipGridData& grid, int* pending, std::size_t maxCycles,
                                 const std::function<bool(std::size_t, double)>& onNorm, bool lastNormDead = false);
    static void cycleUpNoNorm(HipGridData& grid);
    static bool pipelinable(const HipGridData& grid, int pending);
    static void upLeg(HipGridData& grid, std::size_t level); // level-1 -> level-1 up-leg (from `level`)
    // level-0 sweep or pair v -> vAlt (no swap) + norm of f - A v; *sweeps = sweeps run; !wait: the
    // norm is left in flight (grid.readNormEnd())
    static double speculativeSweep(HipGridData& grid, int* sweeps, bool wait = true);
    static bool speculationEnabled(const HipGridData& grid);
    static void jacobi(HipGridData& grid, std::size_t level, std::size_t sweeps, const double* weights = nullptr);
    static void materialize(HipGridData& grid, std::size_t level); // store a pending v = 0
    // the V-cycle below level `from` (its f set) in one gs_coarse_cycle launch
    static void coarseCycle(HipGridData& grid, std::size_t from);
    static double finishNorm(HipGridData& grid, int64_t nparts, bool wait = true);
    static hipStream_t forkBoundary(HipGridData& grid);
    static void forkComm(HipGridData& grid);
    static void joinComm(HipGridData& grid, bool wait);
    static void settleExchange(HipGridData& grid);

    // solve() records its residual history here when non-null (initial, then one per V-cycle)
    static thread_local std::vector<double>* history;
};

class NewtonSolver {
public:
    static void solve(HipGridData& grid);
    static double compF(HipGridData& grid);
    // findError's newtonV += v, left to compFUpdate when fusedUpdate() (returns whether it was deferred)
    static bool findError(HipGridData& grid);
    static double compFUpdate(HipGridData& grid);
    static bool fusedUpdate(const HipGridData& grid);
    static thread_local std::vector<double>* history;
};

// Per-sweep relaxation weights, pure host code (gs_grid.cpp). chebyshevWeights: the nu Chebyshev weights on
// [lo, hi] (throws unless nu >= 1 and 0 < lo < hi). parseOmegas: GS_OMEGAS's value, "w1,w2/w3,w4" or "cheb", as
// pre weights followed by post weights for a grid of pre / post smoothing sweeps (throws on a malformed value, a
// count mismatch, a non-finite weight or more than GS_MAX_WEIGHTS weights per leg).
std::vector<double> chebyshevWeights(int nu, double lo, double hi);
std::vector<double> parseOmegas(const char* text, std::size_t pre, std::size_t post);

// The optional machine-readable metrics line of GpuSolve-hip (GS_METRICS=1), see gs_grid.cpp.
std::string metricsLine(const HipGridData& grid);

// Vector3::dump (src/cpu/Vector3.cpp:56-78) of level `level`'s iterate v (this rank's slab).
void dumpField(HipGridData& grid, std::size_t level, const std::string& path);

} // namespace gs
