// lwhip_host.h -- what the host-side translation units of the C ABI (include/lwhip.h) share: the device-buffer wrapper,
// the context (the HBM-resident copy of a problem, its tables and launch state), the error plumbing and the functions that
// cross file boundaries.
//
//     lwhip_api.hip      create / destroy, one iteration (sweep -> reduce -> [all-reduce by the caller] -> apply), populations
//     lwhip_tables.hip   validation of the descriptor; the structure tables of the sweeps in two halves: plan_tables (device-free:
//                        TableKnobs + compute-unit count -> TablePlan + HostTables) and upload_tables; build_tables drives them
//     lwhip_state.hip    device allocations, kernel argument blocks, the sweep's launch sequence, upload / download
//     lwhip_api2d.hip    the 2D iteration's launch sequence, the 2D primitives
//     lwhip_batch.hip    1.5D column batches
//     lwhip_api_prd.hip  PRD sub-iterations
//     lwhip_rays.hip     emergent spectra along observer rays
//     lwhip_rays2d.hip   ... of a 2D context
//     lwhip_hprd.hip     the hybrid-PRD interpolation tables, built on the device (needs no context)
//
// There is no CPU fallback: without a HIP device every compute entry point fails with LWHIP_ERR_DEVICE.
#pragma once
#include "lwhip_internal.h"
#include "../../include/lwhip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

namespace lwhip
{
// records the message lwhip_last_error() returns (thread-local) and passes the code through
int fail(int code, const std::string& msg);

#define HIP_TRY(expr)                                                                                  \
    do                                                                                                 \
    {                                                                                                  \
        hipError_t err__ = (expr);                                                                     \
        if (err__ != hipSuccess)                                                                       \
            return fail(LWHIP_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(err__));       \
    } while (0)

inline bool debug_knobs_on(); // (LWHIP_DEBUG=1: the diagnosis knobs below are read only then)

// Page-locked host memory out of the library's one pool (lwhip_api.hip).  mapped: host-mapped and coherent, the device reaches it
// through `dev` (the host block, the upload stage, LWHIP_LS_TIMING); otherwise a source or target of copies only.  The block goes
// back to the pool only after `stream` -- the stream whose queued copies or kernels read or write it -- has drained: release()
// waits for it, whatever path the owner leaves by.
struct PinnedBlock
{
    unsigned char* host = nullptr;
    unsigned char* dev = nullptr;
    size_t bytes = 0;
    int device = 0;
    hipStream_t stream = nullptr;
    // at least `need` bytes, used on `s` from now on (a smaller block goes back first)
    hipError_t reserve(int device, size_t need, hipStream_t s, bool mapped = false);
    void release();
    template <typename U> U* as() const { return (U*)host; }
    PinnedBlock() = default;
    PinnedBlock(const PinnedBlock&) = delete;
    PinnedBlock& operator=(const PinnedBlock&) = delete;
    ~PinnedBlock() { release(); }
};

// The state allocations of a context made with lwhip_create_like come out of ONE device allocation (round 6): the owner of the
// tables counts the bytes its own alloc_state asks for (count mode), a borrower gets an arena of that size, cleared with one
// fill, and its DevBufs take consecutive 256-byte-aligned pieces of it -- ~60 hipMalloc and ~13 fills per column of a 1.5D
// batch become one of each.  A piece that does not fit (or any allocation outside lwhip_create) takes the ordinary path.
struct DevArena
{
    unsigned char* base = nullptr;
    size_t size = 0, used = 0;
    size_t counted = 0;   // count mode: bytes asked for
    bool counting = false;
    bool take(size_t bytes, void** p)
    {
        bytes = (bytes + 255) & ~(size_t)255;
        if (counting)
            counted += bytes;
        if (counting || used + bytes > size)
            return false;
        *p = base + used;
        used += bytes;
        return true;
    }
    bool holds(const void* p) const { return !counting && (const unsigned char*)p >= base && (const unsigned char*)p < base + size; }
};

// Host-to-device copies of a batch column's creation, gathered (round 6): while a borrower of a 1.5D batch is created, every
// upload -- the H2D macro, the argument blocks, DevBuf::upload -- is copied into ONE page-locked stage and described by a record;
// lwhip_create then sends the stage to a device inbox with one copy and lets one kernel (h2d_scatter_kernel) move the pieces to
// their buffers.  A column made ~55 copies (several of them from pageable memory, which the runtime stages while holding its
// lock) and one synchronous hipMemcpy that waited 6 ms for the other creating threads' streams; now one copy and one launch.
struct H2DBatch
{
    PinnedBlock stage;              // out of the pinned pool
    unsigned char* inbox = nullptr; // its landing place on the device (a per-device pool of them, lwhip_api.hip)
    int device = 0;
    size_t used = 0;
    std::vector<H2DRec> recs;
    bool inFlight = false; // a flush was queued and the stage not yet known to be free again
    bool open(int device, hipStream_t s); // false: no stage to be had (the ordinary copies)
    bool add(void* dst, const void* src, size_t bytes);
    hipError_t flush();
    hipError_t finish(); // what was gathered goes out, and the stream drains
    void close();        // the stage (after the stream has drained) and the inbox back to their pools
    ~H2DBatch() { close(); }
};

// Everything a context's allocations, fills and host-to-device copies go through (lwhip_context::mem): all of it is queued on
// `stream`, the context's stream; the library queues nothing on the null stream.  The other fields are set only while
// lwhip_create runs.
struct DevMem
{
    hipStream_t stream = nullptr;
    DevArena* arena = nullptr;    // the borrower's arena, or the owner's count
    // alloc(count) leaves out its safety-net clearing (alloc_zero still clears): the state buffers of a context made with
    // lwhip_create_like -- a column of a 1.5D batch: ~40 fills of a few KB each per column, a driver call apiece.  Every byte a
    // kernel reads of such a buffer is written first by an upload or a kernel (tests/test_padding.py runs the column batches
    // under the finite sentinel fills); the owner of the tables, and every ordinary context, keeps the net.
    bool skipSafetyClear = false;
    H2DBatch* batch = nullptr;    // the open gathered upload
    bool unstaged = false;        // a copy since the last settle() reads its source where it lies
    // the one host-to-device copy: into the open gathered upload, else queued on the stream
    hipError_t h2d(void* dst, const void* src, size_t bytes)
    {
        if (bytes == 0 || (batch && batch->add(dst, src, bytes)))
            return hipSuccess;
        unstaged = true;
        return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream);
    }
    // the sources of the copies queued so far may go once this has returned
    hipError_t settle()
    {
        if (batch && !unstaged)
            return hipSuccess;
        unstaged = false;
        return hipStreamSynchronize(stream);
    }
};

// What a fresh allocation holds (lwhip_state.hip): init 0 nothing, 1 the safety net, 2 zeros -- or a diagnosis fill (below)
hipError_t fresh_fill(DevMem& m, void* p, size_t count, size_t elem, bool fp64, int init, int seq);
void released_fill(void* p, size_t bytes);
bool poison_on();
bool sentinel_on();

template <typename T> struct DevBuf
{
    T* p = nullptr;
    size_t n = 0;
    bool owned = true;
    uint64_t sig = 0; // content fingerprint of what upload() put there (see upload_or_borrow)
    // What a fresh allocation holds.  Round 4 handed out CLEARED memory because some kernel read bytes no upload had written and
    // hipMalloc returns whatever the pages' previous owner left there.  Round 5 located such reads with a FINITE sentinel
    // (LWHIP_PAD_SENTINEL, lwhip_state.hip; NaN is swallowed by the fmin / fmax of the Steffen derivative, a finite 6.7e299 is
    // not) and fixed them; what is left of the clearing is listed in DESIGN.md section 4.
    //   alloc(m, count)         state buffer: every byte a kernel reads is written first by an upload or a kernel (asserted by
    //                           the sentinel test); cleared all the same as a safety net unless LWHIP_NO_CLEAR is set
    //   alloc(m, count, false)  the caller overwrites all of it at once (upload)
    //   alloc_zero(m, count)    a buffer that is ACCUMULATED into, or whose zero is a value: always cleared
    // The fills are queued on m.stream, ahead of every copy and kernel that touches the buffer.
    hipError_t alloc(DevMem& m, size_t count, bool clear = true) { return alloc_impl(m, count, clear ? 1 : 0); }
    hipError_t alloc_zero(DevMem& m, size_t count) { return alloc_impl(m, count, 2); }
    hipError_t alloc_impl(DevMem& m, size_t count, int init)
    {
        release();
        n = count;
        if (count == 0)
            return hipSuccess;
        if (m.arena && m.arena->take(count * sizeof(T), (void**)&p))
        {
            owned = false; // (the arena was cleared as a whole: zeros serve alloc_zero and the safety net alike)
            return hipSuccess;
        }
        const hipError_t e = hipMalloc((void**)&p, count * sizeof(T));
        const int seq = alloc_seq()++;
        return e != hipSuccess ? e : fresh_fill(m, p, count, sizeof(T), std::is_same<T, double>::value, init, seq);
    }
    static std::atomic<int>& alloc_seq() // (diagnosis only: the numbers of LWHIP_TRACE_ALLOC / LWHIP_PAD_SENTINEL)
    {
        static std::atomic<int> seq{ 0 };
        return seq;
    }
    // the clearing of a buffer whose zeros only keep its padding finite (not a value): left out under the sentinel, and for a
    // piece of the borrower's arena (cleared as a whole a moment ago)
    hipError_t clear_padding(DevMem& m)
    {
        if (!p || sentinel_on() || (m.arena && m.arena->holds(p)))
            return hipSuccess;
        return hipMemsetAsync(p, 0, n * sizeof(T), m.stream);
    }
    // a window of somebody else's allocation (the depth arena of the lane sweep)
    void view(T* ptr, size_t count)
    {
        release();
        p = ptr;
        n = count;
        owned = false;
    }
    // the table of a structurally identical context instead of a copy of one's own (lwhip_create_like): same size, or upload
    // ... and only if it holds what this context would upload: the structure fingerprint of lwhip_create_like covers the
    // problem, not the layout choices build_tables reads from the environment (LWHIP_SWEEP, the tile / split / tail knobs of
    // tests and tools) -- a borrower made under another environment computes another layout and must not run on the donor's
    // tables.  The fingerprint samples the bytes (size, both ends, ~4 000 words in between): a different layout differs in
    // sizes or in the first records.
    static uint64_t fingerprint(const std::vector<T>& v)
    {
        const size_t nw = v.size() * sizeof(T) / 4;
        const unsigned char* b = (const unsigned char*)v.data();
        uint64_t h = 1469598103934665603ull ^ (uint64_t)(v.size() * sizeof(T));
        auto word = [&](size_t w) {
            uint32_t x;
            std::memcpy(&x, b + 4 * w, 4);
            h = (h ^ x) * 1099511628211ull;
        };
        const size_t step = nw > 8192 ? nw / 4096 : 1;
        for (size_t w = 0; w < nw; w += step)
            word(w);
        for (size_t w = nw > 16 ? nw - 16 : 0; w < nw; ++w)
            word(w);
        return h | 1ull;
    }
    hipError_t upload_or_borrow(DevMem& m, const std::vector<T>& v, const DevBuf<T>* from)
    {
        if (from && from->p && from->n == v.size() && !v.empty() && from->sig == fingerprint(v))
        {
            view(from->p, from->n);
            sig = from->sig;
            return hipSuccess;
        }
        // (a structure table: the owner's copy is what borrowers use, so it is neither counted into the size of a borrower's
        // arena nor -- where a borrower has to keep a copy of its own after all -- taken out of one)
        DevArena* const ar = m.arena;
        m.arena = nullptr;
        const hipError_t e = upload(m, v);
        m.arena = ar;
        return e;
    }
    hipError_t upload(DevMem& m, const std::vector<T>& v)
    {
        hipError_t e = alloc(m, v.size(), poison_on());
        if (e != hipSuccess || v.empty())
            return e;
        sig = fingerprint(v);
        e = m.h2d(p, v.data(), v.size() * sizeof(T));
        return e != hipSuccess ? e : m.settle(); // (v is the caller's: it may go when this returns)
    }
    void release()
    {
        if (p && owned)
        {
            if (poison_on())
                released_fill(p, n * sizeof(T));
            (void)hipFree(p);
        }
        p = nullptr;
        n = 0;
        owned = true;
        sig = 0;
    }
    ~DevBuf() { release(); }
};


struct HostTrans
{
    lwhip_transition t;   // borrowed host pointers
    int atom;
    int NblueLoc, NredLoc; // clipped to the shard, shard-local indices
    int ltStart;           // first own-grid index inside the shard
    int rhoLt0 = 0, rhoRows = 0; // PRD lines: the own-grid rows held in the rho pool (the shard's; hybrid PRD: the whole grid)
    int row;               // wphi row (lines) / ratio row (continua)
    int64_t parOff, phiOff, rhoOff;
    int64_t waveOff; // lines: offset of the full own grid / wlambda in the lineWave / lineWlam pools
};
// The transitions active at each wavelength row, in the reference's order (active atoms, then detailed ones; kr order): row la
// has laTr[laOff[la] .. laOff[la + 1]).  local: the rows of the context's own grid (NblueLoc / NredLoc), or of the global one.
inline void active_trans_lists(const std::vector<HostTrans>& trans, int Nla, bool local, std::vector<int32_t>& laOff,
                               std::vector<int32_t>& laTr)
{
    laOff.assign(Nla + 1, 0);
    laTr.clear();
    for (int la = 0; la < Nla; ++la)
    {
        laOff[la] = (int32_t)laTr.size();
        for (size_t tr = 0; tr < trans.size(); ++tr)
        {
            const HostTrans& h = trans[tr];
            if (la >= (local ? h.NblueLoc : h.t.Nblue) && la < (local ? h.NredLoc : h.t.Nred))
                laTr.push_back((int32_t)tr);
        }
    }
    laOff[Nla] = (int32_t)laTr.size();
    if (laTr.empty())
        laTr.push_back(0); // (never an empty upload)
}
// What forming a line's profile at a point needs beside the point, per transition (the order of `trans`, which is what the lists
// above index): where the pools keep vBroad of the line's atom, its aDamp row and its own wavelength grid, and lambda0.  For the
// kernels that evaluate phi where they gather instead of reading a stored one: the observer rays (lwhip_rays.hip) and the
// full-Stokes observer gather (lwhip_stokes_fs.hip).
struct LineEval
{
    int32_t atom, row, ltStart, _pad; // row: aDamp row (lines) / ratio row (continua); ltStart: own-grid index of the shard's first row
    int64_t waveOff;                   // the line's full own grid in the lineWave pool (0 for a continuum)
    double lambda0;
};
inline std::vector<LineEval> line_eval_records(const std::vector<HostTrans>& trans)
{
    std::vector<LineEval> ev(std::max<size_t>(trans.size(), 1), LineEval{});
    for (size_t tr = 0; tr < trans.size(); ++tr)
    {
        const HostTrans& h = trans[tr];
        ev[tr].atom = h.atom;
        ev[tr].row = h.row;
        ev[tr].ltStart = h.ltStart;
        ev[tr].waveOff = h.waveOff >= 0 ? h.waveOff : 0;
        ev[tr].lambda0 = h.t.lambda0;
    }
    return ev;
}

// ---- the structure tables (lwhip_tables.hip) ----------------------------------------------------------------------------------
// The environment's knobs that shape the tables, read once per lwhip_create (read_table_knobs).  The layout knobs are honoured
// only under LWHIP_DEBUG; the defaults below are what a production process gets.
struct TableKnobs
{
    struct OptInt // a knob whose default is computed where it is used
    {
        bool set = false;
        int v = 0;
        int value_or(int dflt) const { return set ? v : dflt; }
    };
    bool createTiming = false; // LWHIP_CREATE_TIMING: where the host time of the tables goes (stderr)
    bool verbose = false;      // LWHIP_VERBOSE: tile and finish-program histograms (stderr)
    bool sweepGiven = false, sweepLanes = false, sweepMarch = false; // LWHIP_SWEEP=lanes|march forces a sweep
    int tileGeneric = 0;       // LWHIP_TILE_GENERIC > 0: every tile through the guarded generic march (test hook)
    int laneGeneric = 1;       // LWHIP_LANE_GENERIC=0: no generic kind in the lane sweep (such problems take the march)
    int tileL = 16;            // LWHIP_TILE_L: most wavelengths of a march tile
    OptInt tileLH, tileL1;     // LWHIP_TILE_LH / LWHIP_TILE_L1: ... of a tile with two or more slots / with one
    int lWaves = 4, tWaves = 2; // LWHIP_LWAVES / LWHIP_TWAVES: wavefronts per workgroup of the lane sweep / the march
    int tileFuse = 1;          // LWHIP_TILE_FUSE=0: the march's post-pass as a launch of its own
    int laneSplit = 0;         // LWHIP_LANE_SPLIT=1|2|4: wavefronts a tile's rays are split over
    OptInt laneCut;            // LWHIP_LANE_CUT: chunks of the lane sweep's tail cut in two
    int depthSplit = -1;       // LWHIP_DEPTH_SPLIT=1|2|4: wavefronts a direction's depth points are split over on the march
    int detNoWait = 0;         // LWHIP_DET_NOWAIT: fixed-order mode without its waits (measurement only, bit mask)
    int finFast = 1;           // LWHIP_FIN_FAST=0: the finish's general form for every tile
};

// What build_tables decides, as scalars: THE declaration list (type, name, initial value).  lwhip_context derives from
// TablePlan, so a reader says c->laneSweep; plan_tables fills one, upload_tables copies it into the context, and
// lwhip_tables_signature folds the fields in this order.
#define LWHIP_TABLE_PLAN(X)                                                                                                     \
    X(int64_t, gammaTot, 0) X(int64_t, phiTot, 0) X(int64_t, rhoTot, 0) X(int64_t, parTot, 0) /* doubles of the pools */      \
    X(int64_t, rowsTot, 0)     /* rows of the continuum-row buffer (march, 2D) */                                              \
    X(int64_t, rowsTileTot, 0) X(int64_t, momTot, 0) X(int64_t, phiTTot, 0) /* doubles of the tiles' rows / moments / phi */  \
    X(int, NlevTot, 0) X(int, Ntrans, 0) X(int, Nline, 0) X(int, Ncont, 0)                                                    \
    X(int, maxL, 0) X(int, maxC, 0) X(int, maxM, 0) X(int, maxP, 0) /* most lines / continua / mixed / pure at one wavelength */ \
    X(int, nContLa, 0)         /* wavelengths with a continuum */                                                              \
    X(bool, tiled, false)      /* 1D: tiles of structurally identical wavelengths */                                          \
    X(bool, laneSweep, false)  /* the depth-across-lanes sweep (lwhip_lanesweep.hip), else the ray-column march */            \
    X(bool, deterministic, false) /* LWHIP_OPT_DETERMINISTIC as asked for; the plan turns it off on the march */              \
    X(int, laneD, 0) X(int, laneLR, 0) X(int, laneR, 0) /* lane sweep: points per lane, lanes per ray, wavelengths per wavefront */ \
    X(int, tileL, 12)          /* most wavelengths of a tile */                                                                \
    X(int, tileCap, 0)         /* > 0: the guarded generic march, up to this many lines / mixed continua per tile */          \
    X(int, tileWaves, 4)       /* wavefronts per workgroup */                                                                  \
    X(bool, tileFuse, false)   /* march: the workgroup = one tile, finished by the post-pass inside the sweep launch */       \
    X(int, depthSplit, 1)      /* march on deep columns: wavefronts a direction's depth points are split over */              \
    X(int, laneSplit, 1) X(int, laneSplitPrd, 1) /* lane sweep: wavefronts a tile's rays are split over; ... in the PRD rates pass */ \
    X(int, nTiles, 0) X(int, nTilesPrd, 0) X(int, nTileChunks, 0) X(int, nTileChunksPrd, 0) X(int, nPostChunks, 0)            \
    X(int, nPostChunksPrd, 0)                                                                                                  \
    X(int, maxSlotsTile, 0) X(int, maxCTTile, 1) X(int, maxCTPost, 1) /* most slots of a tile; accumulator slots per workgroup */ \
    X(int, preCols, 0)         /* most level-sum columns a tile's rows need (LDS columns of the pre-pass) */                   \
    X(bool, chunkOrderOn, false) X(bool, chunkSplitOn, false) /* lane sweep: chunkOrder / chunkSplit are in use */            \
    X(int, nGenTiles, 0) X(int, momA, 0) /* lane sweep: tiles of the generic kind, moment-scratch rows of their wavefronts */
struct TablePlan
{
#define X(type, name, init) type name = init;
    LWHIP_TABLE_PLAN(X)
#undef X
};

// The device buffers of the structure tables: THE declaration list (element type, name), in upload order.  lwhip_context
// derives from TableBufs; a context made with lwhip_create_like borrows each from its owner where the bytes agree
// (upload_tables), and lwhip_tables_signature folds size and content fingerprint of each in this order.
#define LWHIP_TABLE_BUFS(X)                                                                                                     \
    X(int32_t, detOff) X(int32_t, detEnt) X(int32_t, detOffPrd) X(int32_t, detEntPrd) /* fixed-order mode: (workgroup, slot) lists */ \
    X(double, lineWave) X(double, lineWlam) X(double, par)                                                                     \
    X(DevTrans, dtrans) X(DevLaHeader, laHdr) X(DevSlot, slots) X(int32_t, slotTrD)                                            \
    X(DevProgram, progs) X(DevProgRow, progRows) X(DevProgEnt, progEnts)                                                       \
    X(int32_t, contLa) X(int32_t, rayAll) X(int32_t, rayUp)                                                                    \
    X(DevContRec, contRec) X(DevPostProg, postProg)                                                                            \
    X(DevTile, tiles) X(DevTileSlot, tslots) X(DevTileSlot, tslotsPrd) X(DevTileCopy, tcopies) X(int32_t, tileRemap)           \
    X(int32_t, chunkTile)                                                                                                      \
    X(int32_t, chunkOrder) /* lane sweep: dispatch order of the workgroups' chunks */                                          \
    X(int32_t, chunkSplit) /* ... per chunk, the wavefronts its tiles' rays are split over (the launch's tail) */              \
    /* lane sweep: the flat per-workgroup / per-tile records of a task's setup and finish (lwhip_internal.h) */               \
    X(DevLaneWg, laneWg)                                                                                                       \
    X(uint8_t, laneFeedG)  /* generic tiles: continuum -> slot feed bytes */                                                   \
    X(DevLaneTile, laneTiles) X(DevLaneTile, laneTilesPrd) X(DevLaneWg, laneWgPrd)                                             \
    X(DevLaneRay, laneRays) X(DevLaneFin, laneFin) X(double, laneFinPar)                                                       \
    X(int32_t, chunkTilePrd) X(int32_t, tileListPrd) X(int32_t, tileSlotTr) X(int32_t, tileSlotTrPrd)                          \
    X(int32_t, postChunkTile) X(int32_t, postChunkTilePrd) X(int32_t, postSlotTr) X(int32_t, postCs)                           \
    X(int32_t, transLi) X(int32_t, transLj) X(int32_t, atomNlevel) X(int32_t, atomDetailed) X(int32_t, atomTrOffD)
struct TableBufs
{
#define X(type, name) DevBuf<type> name;
    LWHIP_TABLE_BUFS(X)
#undef X
};

// Everything plan_tables hands upload_tables beside the plan: the bytes of every table, the host vectors the context keeps, and
// the sizes of the few allocations.  A vector left empty is a table this context does not have.
struct HostTables
{
#define X(type, name) std::vector<type> name;
    LWHIP_TABLE_BUFS(X) // (one per buffer of TableBufs, as it is uploaded)
#undef X
    // what the context keeps on the host (lwhip_context's members of the same names)
    std::vector<HostTrans> trans;
    std::vector<int> levelOff, atomTrOff;
    std::vector<int64_t> gammaOff;
    std::vector<int> hLa2prdHost, hLa2hHost;
    std::vector<int64_t> hRhoOffHost;
    // hybrid PRD: never borrowed (the coefficients follow the atmosphere)
    std::vector<lwhip_rho_coeff> hRho;
    std::vector<int32_t> hLa2h;
    std::vector<int64_t> hJOff;
    std::vector<lwhip_j_coeff> hJCoef;
    // elements of the allocations (0: none)
    size_t JRestCount = 0, detSlabCount = 0, detPartCount = 0, momScratchCount = 0;
    // between the stages of the plan only
    std::vector<int> laneCsPure;    // lane sweep: accumulator slot of every pure continuum inside its workgroup chunk
    std::vector<char> ppWide;       // per tile: the finish program's words are in the wide encoding
    std::vector<uint32_t> turnPure; // fixed-order mode: per (tile, continuum) the task's turn at the continuum's slot
};

// the fold of structure_signature, for lwhip_tables_signature's two words
struct SigFold
{
    uint64_t h = 0x9E3779B97F4A7C15ull;
    void mix(uint64_t v)
    {
        h ^= v + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2);
        h *= 0xFF51AFD7ED558CCDull;
        h ^= h >> 33;
    }
};
}
using namespace lwhip;

namespace lwhip
{
// full Stokes (lwhip_stokes.hip, lwhip_stokes_fs.hip): one transition as the Stokes gather reads it
struct StokesTrans
{
    int32_t type, gi, gj, Nblue; // (gi, gj: global level rows into the n pool)
    int32_t prd, row, pol, _pad; // row: ratio row (continua); pol: ordinal among the polarised lines, or -1
    int64_t parOff, phiOff, rhoOff; // (rhoOff: of the line's own-grid row 0)
    int64_t polOff, polStride;   // polarised lines: phiQ of the line in the pol pool; the six arrays are polStride apart
};
// what lwhip_set_stokes borrowed and its device copies
struct StokesState
{
    bool on = false;
    lwhip_stokes desc{};
    std::vector<lwhip_stokes_line> lines;
    std::vector<int> lineTr;       // global transition index of each polarised line
    std::vector<int64_t> polOff;   // offset of each line's six arrays in `pol`
    std::vector<int32_t> laPolHost;// per wavelength: a polarised line is active
    int64_t polTot = 0;
    bool polOnDevice = false;      // phiQ..psiV were computed on the device since the last LWHIP_STOKES transfer
    DevBuf<double> B, proj, pol, Quv, J20, comp;
    DevBuf<int32_t> alpha, laOff, laTr, laPol;
    DevBuf<StokesTrans> tr;
    // for the observer gather, which forms the profiles of a new direction where it needs them: what evaluating each transition's
    // profile takes (indexed as `tr`), and per polarised line the offset of its components in alpha / comp and their number
    DevBuf<LineEval> ev;
    DevBuf<int32_t> polComp;
    int64_t nComp = 0; // all lines' components: `comp` holds the shifts, then the strengths
    DevBuf<PolLineArgs> args;
    std::vector<PolLineArgs> argsHost;
};
int stokes_transfer(lwhip_context* c, bool up); // lwhip_upload / lwhip_download of LWHIP_STOKES
// the refusals the Stokes entry points share, the device check first (lwhip_stokes.hip)
int check_stokes_ctx(lwhip_context* c, const char* what, bool needStokes);
struct StokesBatch; // what a context, or a column batch, keeps for its full-Stokes formal solutions (lwhip_stokes_fs.hip)
void stokes_batch_release(StokesBatch* s);
// observer rays (lwhip_rays.hip, lwhip_rays2d.hip)
// one transition as the gather reads it
struct RayTrans
{
    int32_t type, gi, gj, Nblue; // (gi, gj: global level rows of the n pool; Nblue: first row of the context's grid)
    int32_t prd, row, atom, ltStart; // row: aDamp row (lines) / ratio row (continua); ltStart: own-grid index of Nblue
    int64_t parOff, rhoOff, waveOff; // (rhoOff: of the row of Nblue)
    double lambda0;
    // a line of the context's hybrid-PRD list (lwhip_hprd.lineAtom / lineTrans), read by the hybrid gather alone: its own grid is
    // nlt wavelengths at waveOff, rho of the whole of it [nlt, Ns] at rho0Off (plan_hybrid_prd keeps it resident on every shard)
    int32_t hybrid, nlt;
    int64_t rho0Off;
};

// The structure tables of the gather and the staging of a call.  The tables depend on the structure alone: a context made with
// lwhip_create_like uses its table owner's.
struct RaysState
{
    std::mutex lock;
    bool built = false;
    DevBuf<RayTrans> tr;
    DevBuf<int32_t> laOff, laTr;
    DevBuf<unsigned char> in, out; // [RayCol per column | staged vz | staged lowerBc], [per column: I | chi | eta | I(k)]
    PinnedBlock inPinned, outPinned;
};

void rays_release(RaysState* s);
// the gather tables of `o` (a table owner: a context made with lwhip_create_like uses its owner's), made on first use
int rays_tables(lwhip_context* o, RaysState*& out);
struct Rays2dState; // observer rays of a 2D context (lwhip_rays2d.hip): the geometry of the last view, the staging of its calls
void rays2d_release(Rays2dState* s);

// The geometry tables of a 2D grid on the device, as the 2D formal solver reads them (Fs2dArgs): the context's own grid, and the
// grid of an observer's directions (lwhip_rays2d.hip).  Filled by geom2d_upload (lwhip_state.hip).
struct Geom2dDev
{
    DevBuf<double> mux;
    DevBuf<lwhip_intersection> uw, dw, sub;
    DevBuf<double> uwS, dwS; // the records field by field (fs2d_records_packed), or empty
    DevBuf<int32_t> uwA, dwA, longIdx, subOff, lcOwner;
};
// `g`'s tables into `d`, queued on m's stream: g's arrays must stay until that stream has been waited for
int geom2d_upload(DevMem& m, const lwhip_grid2d& g, Geom2dDev& d);

// Ng acceleration of the populations of n columns (ng_kernel, lwhip_pops.hip), every column's history and call count on the
// device: a batch owns one for its n columns, a lone context one for itself -- a batch of one.  Off: all empty.
struct NgState
{
    bool on = false;
    int order = 0, period = 0, delay = 0; // (delay after the max rule, Ng.hpp:32)
    int64_t histStride = 0;               // doubles of history per column
    int n = 0, Natoms = 0;                // columns; solved atoms of each
    DevBuf<NgCol> columns;                // [n] every column's n pool and status word
    DevBuf<NgAtom> atoms;                 // [Natoms] the solved atoms, offsets inside one column
    DevBuf<double> history;               // [n][Natoms][order + 2][Nlevel * Ns]
    DevBuf<double> out;                   // change [n][Natoms][2], then int32 count [n], accel [n], ticket [n]: one copy
    PinnedBlock pinned;                   // ... lands here (change, count, accel)
    // A lone context has the kernel store change and accel into its host-mapped block instead (no copy per step); else null
    double* mappedChange = nullptr;       // device address of the block's change records, the accel word behind them
    const double* mappedChangeHost = nullptr;
    size_t change_doubles() const { return (size_t)n * Natoms * 2; }
    int32_t* count() const { return (int32_t*)(out.p + change_doubles()); } // (device)
    // where the host reads what ng_fetch brought (or the kernel stored)
    const double* change_host() const { return mappedChange ? mappedChangeHost : pinned.as<double>(); }
    const int32_t* count_host() const { return (const int32_t*)(pinned.as<double>() + change_doubles()); }
    const int32_t* accel_host() const { return mappedChange ? (const int32_t*)(mappedChangeHost + change_doubles()) : count_host() + n; }
};
// cols: the columns (structurally identical; one stream and device: cols[0]'s).  lone -- the one place the two owners differ:
// cols is one context, whose host-mapped block takes change and accel (see NgState) and for which (0, 0, 0) is order 0 (no
// extrapolation, changes tracked); for a batch (0, 0, 0) turns Ng off.  No solved atom: off, LWHIP_OK.
int ng_configure(NgState& s, const std::vector<lwhip_context*>& cols, int Norder, int Nperiod, int Ndelay, bool lone);
int ng_off(NgState& s, hipStream_t stream);
NgArgs ng_args(const NgState& s, const int32_t* activeCols);
// the Ng step of nActive columns (activeCols: their numbers on the device, or null: the first nActive), queued on `stream`
hipError_t ng_step(const NgState& s, const int32_t* activeCols, int nActive, hipStream_t stream);
// after a step: waits for `stream` with every column's change and accel at change_host() / accel_host() (mapped: no copy)
int ng_fetch(NgState& s, hipStream_t stream);
void ng_changes(const NgState& s, int col, double* dPops, int32_t* dPopsMaxIdx); // ... column col's [Natoms] out of them
// lwhip_ng_state / lwhip_batch_ng_state: the options in effect and the device's own count and accel words ([n] each; off: zeros)
int ng_read_state(NgState& s, int n, hipStream_t stream, int32_t opts[3], int32_t* counts, int32_t* lastAccelerated);
}

struct lwhip_context;
namespace lwhip
{
int host_block_init(lwhip_context* c);
void host_block_release(lwhip_context* c);
hipError_t stream_acquire(int device, hipStream_t* out);
void stream_release(int device, hipStream_t s);
hipError_t stream_acquire_shared(int device, hipStream_t* out); // the columns of a batch made by one thread share a stream
void stream_release_shared(int device, hipStream_t s);
void* pinned_acquire(int device, size_t bytes, void** devPtr, bool mapped); // the pinned pool (PinnedBlock: its owner type)
void pinned_release(int device, void* p, size_t bytes);
void peer_release(lwhip_context* c);
int peer_publish(lwhip_context* c);
int fingerprint_J_enqueue(lwhip_context* c);
void fingerprint_J_fold(lwhip_context* c, const void* p);
void peer_apply_args(lwhip_context* c, struct ApplyArgs& a);
}

// (TablePlan, TableBufs: what build_tables decided and put on the device -- one declaration list each, above)
struct lwhip_context : lwhip::TablePlan, lwhip::TableBufs
{
    lwhip_problem prob;             // copy of the descriptor (host pointers borrowed)
    std::vector<lwhip_atom> atoms;
    std::vector<HostTrans> trans;   // global transition list, reference order (these vectors: copies of the HostTables')
    std::vector<int> levelOff, atomTrOff;
    std::vector<int64_t> gammaOff;
    int device = 0;
    int worldSize = 1, worldRank = 0;
    int laStart = 0, laEnd = 0, Nla = 0;
    int Ns = 0, Nrays = 0, Natom = 0;
    bool is2d = false;            // x-periodic 2D geometry (prob.grid2d): batched pipeline of lwhip_2d.hip
    int Nx = 1, batch2d = 1;
    std::vector<DevLaHeader> hdrHost;
    std::vector<int32_t> contLaHost;
    DevBuf<double> geoT;
    // hybrid PRD (lwhip_options.hprd): the tables of configure_hprd_coeffs on the device
    // deterministic mode (LWHIP_OPT_DETERMINISTIC): per-workgroup slabs (the (workgroup, slot) lists of every transition: TableBufs)
    DevBuf<double> detSlab, detPart; // (detPart: partial sums of the fixed-shape reduction, lwhip_lanesweep.hip)
    const lwhip_hprd* hprd = nullptr;
    std::vector<int> hLa2prdHost, hLa2hHost;     // global wavelength -> row of JRest / ordinal among hPrdIdxs, or -1
    std::vector<int64_t> hRhoOffHost;             // per transition: offset of its rho-coefficient block, or -1
    DevBuf<lwhip_rho_coeff> hRho;
    DevBuf<int32_t> hLa2h;
    DevBuf<int64_t> hJOff;
    DevBuf<lwhip_j_coeff> hJCoef;
    DevBuf<double> JRest;
    PinnedBlock lsDbg;           // LWHIP_LS_TIMING: phase clocks of the last sweep, [nTiles][8] (mapped)
    DevBuf<double> depArena; // lane sweep: n | wphi | ratio | geoT in one allocation (one buffer resource in the kernel)
    int ktStride = 4;
    DevBuf<double> bcPlanck;
    DevBuf<double> momScratch;    // the moment scratch of the generic tiles' wavefronts (TileArgs::momS)
    DevBuf<double> geo, kt, rowsTile, momTile, phiT;
    DevBuf<TileArgs> dtargs, dtargsPrd;
    TileArgs htargs{}, htargsPrd{};
    DevMem mem;                   // allocations, fills and uploads: all on the context's stream
    hipStream_t& stream = mem.stream;
    hipStream_t ownStream = nullptr;
    bool ownStreamShared = false;

    DevBuf<double> height, temperature, muz, wmu, wavelength, lowerBcData, upperBcData;
    DevBuf<int32_t> lowerIdx, upperIdx;
    DevBuf<double> bgChi, bgEta, bgSca, J, I, depthChi, depthEta, depthI;
    DevBuf<double> n, nTotal, ratio, wphi, phi, rho, Gamma, Cmat, Rij, Rji;
    DevBuf<double> vlosMu, vBroad, aDamp, Qelast;
    DevBuf<double> prdChange, rowsBuf, popScratch, prdJt, prdJ;
    DevBuf<PrdLineArgs> prdArgsDev;   // argument blocks of the PRD lines of a sub-iteration (one launch for all lines)
    std::vector<PrdLineArgs> prdArgsHost; // what the device copy holds
    DevBuf<double> b2cs, b2I, b2Psi, b2coef, red2d;
    DevBuf<int32_t> b2idx;
    int groups2d = 1, maxRowsLa = 1;
    int kLo = 0, kHi = -1; // depth range of the population updates (lwhip_set_depth_range); kHi < 0: to the end
    int djIdxMode = 0;     // lwhip_set_djmax_index_mode: 1 = the single-thread scheme's index bookkeeping
    double* tailMapped = nullptr; // host-mapped (dJMax, idx) of the one-call iteration (a window of hostBlock)
    double* tailMappedDev = nullptr;
    double tailTicket = 0.0;      // ticket of the last launch that reports through tailMapped
    // line profiles generated on the device (lwhip_compute_profiles): re-derived before the next sweep whenever the
    // inputs they depend on (vlosMu: LWHIP_ATMOS; vBroad, aDamp: LWHIP_NSTAR) are uploaded again
    bool deviceProfiles = false, profilesStale = false;
    DevBuf<VoigtLineArgs> voigtList; // the lines' argument blocks of lwhip_compute_profiles
    DevBuf<double> wphiScratch;   // [16, Ns] wavelength-slice sums of the profile normalisation
    DevBuf<int> wphiTicket;       // arrival counters of its point tiles
    bool lastSweepUpOnly = false; // the last sweep traced the up rays only (lwhip_formal_sol(upOnly))
    bool partsOnly = false;       // fs_partial ran stage 1 of the slab reduce only (one-call iteration)
    int batchHint = 0;            // lwhip_options.flags & 0xffff: contexts expected to share the device (column batch)
    bool prdDetailed = false;     // LWHIP_OPT_PRD_DETAILED: the PRD calls include the detailed atoms' PRD lines
    Geom2dDev g2;                      // 2D: the geometry tables of the context's own grid (geom2d_upload)
    DevBuf<double> xbcLow, xbcUp;      // 2D, fixed x boundaries: [Nla, Nmu, Nz] of the shard
    DevBuf<double> zDown, zUp;         // ZPlaneDecomposition outputs [Nla, Nrays, Nx] (lwhip_set_zplane_outputs)
    double* zDownHost = nullptr;       // their host arrays [Nlambda, Nrays, Nx]
    double* zUpHost = nullptr;
    DevBuf<int32_t> xIdxLow, xIdxUp;   // [Nrays, 2]
    DevBuf<double> b2lc; // [batch2d][NlongChar][3]
    // lwhip_create_like: the structure tables (lwhip_tables.hip) are borrowed from a context of the same structure, which
    // counts its borrowers and cannot be destroyed before them
    lwhip_context* tablesFrom = nullptr;
    std::atomic<int> borrowers{ 0 }; // (contexts are created and destroyed from several host threads: columns, per-GPU workers)
    uint64_t structSig = 0; // fingerprint of everything the structure tables are built from
    bool dJPrdClean = false; // dJ holds zeros outside the wavelengths the PRD rates pass visits (no full sweep since)
    std::vector<int> prdLines;        // PRD lines of the active atoms (global transition indices), reference order
    std::vector<int64_t> prdRowOff;   // first row of each line's grid in the prdJ gather buffer
    int64_t prdRowsTot = 0;
    bool prdPending = false;          // between lwhip_prd_partial and lwhip_prd_finalise
    bool prdFused = false;            // ... and its apply launch reads the stage-1 parts and reduces the lines' changes itself
    std::vector<std::unique_ptr<DevBuf<double>>> gII; // per transition: cached PRD weights (lazily)
    std::vector<char> gIIValid;
    DevBuf<NrAtom> nrAtoms, statEqAtoms;
    NgState ng; // lwhip_ng_configure: this context as a batch of one column
    int statEqKey = -2;
    int32_t* statusHost = nullptr;
    int32_t* statusDev = nullptr;
    double* changeHost = nullptr; // host-mapped per-block population changes of the last reported solve
    double* changeDev = nullptr;
    size_t changeCount = 0;
    DevBuf<int32_t> transType;
    DevBuf<int32_t> prdChangeIdx;
    PinnedBlock prdPinned;
    // pipelined sub-iterations of lwhip_redistribute_prd (one device, 1D, lane sweep): the launches of up to PRD_PIPE_DEPTH
    // sub-iterations are queued without a host round trip in between; the device keeps the loop's stopping rule (prdCtl, see
    // ApplyArgs) and every sub-iteration's results land in its own slot of prdPinnedPipe
    DevBuf<int32_t> prdCtl;
    // every line's profile is the same for the two directions of an angle (static atmosphere): found when the profiles are
    // uploaded (the host's arrays are compared) or generated (all line-of-sight velocities zero); TileDyn::phiSym
    bool phiSym = false, vlosZero = false;
    // ... and, beyond that, the same for every angle (no line-of-sight velocity at all: the Voigt argument does not know the
    // ray), found in the same places: bit-identical blocks [lt][0][down] = [lt][mu][dir]; TileDyn::phiIso
    bool phiIso = false;
    // LWHIP_PAIR_RAYS=0 / LWHIP_PRD_PIPELINE=0 (experiment knobs, read ONCE per context in lwhip_create and only under
    // LWHIP_DEBUG like the other layout knobs: the first changes the order of the arithmetic)
    // LWHIP_ISO_RAYS=0: angle-independent profiles are not made use of (the stencils are formed once per angle as for
    // profiles that are only direction-symmetric; the same arithmetic, so the same bits)
    // LWHIP_LS_PLAIN=0: every launch of the lane sweep takes the full instance (the plain one leaves out code the launch
    // does not need: the same arithmetic, so the same bits); for A/B runs and tests
    bool pairRays = true, isoRays = true, prdPipeline = true, prdGeneral = false, lsPlain = true;
    PinnedBlock prdPinnedPipe;
    int prdPipeIter = 0;     // > 0: the sub-iteration the calls of lwhip_prd_partial / _finalise belong to
    double prdPipeTol = 0.0;
    DevBuf<ContArgs> dargs;      // 2D: argument block of the continuum-row kernel
    ContArgs hargs{};
    bool atomicParts = false;     // the pending iteration's parts were accumulated by atomics
    bool red8Clean = false;       // red8 holds zeros (only the atomic path leaves it so)
    int* zeroCheck = nullptr;     // LWHIP_CHECK_ZERO=1 (diagnosis): host-mapped count of non-zero words found in red8 at sweep entry
    int* zeroCheckDev = nullptr;  // (windows of hostBlock; null unless the knob is set)
    DevBuf<int64_t> atomGammaOff;
    DevBuf<double> red, red8, dJ;
    std::vector<double> gatherHost;
    DevBuf<int32_t> status;
    StokesState stokes;           // lwhip_set_stokes (lwhip_stokes.hip)
    StokesBatch* stokesFs = nullptr; // made by the first lwhip_full_stokes_fs (lwhip_stokes_fs.hip)
    RaysState* rays = nullptr;    // made by the first lwhip_compute_rays (lwhip_rays.hip)
    Rays2dState* rays2d = nullptr; // made by the first lwhip_compute_rays_2d (lwhip_rays2d.hip)

    bool profiling = false;
    int profEvery = 1, profCount = 0; // time every profEvery-th sweep launch (lwhip_profile_enable(ctx, n))
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
    double sweepMs = 0.0;
    int sweepCount = 0;
    bool partialPending = false;
    bool prefillPending = false; // lwhip_gamma_prefill_from_C deferred into the next apply_kernel
    double prefillCrsw = 1.0;
    PinnedBlock gatherPinned;
    // pinned staging for the many small per-atom / per-transition host arrays: they are packed here and
    // cross PCIe as a few large copies (a pageable hipMemcpy per 656-byte row costs ~12 us each); layout: stage_layout
    PinnedBlock stage;

    // ONE pinned, host-mapped block per context holds every word the DEVICE stores into host memory (tailMapped, statusHost,
    // changeHost, zeroCheck point into it) and every target of a small device-to-host copy the API used to aim at a stack
    // variable (popStatusHost, prdCtlHost): made once in lwhip_create (host_block_init), released by the destructor AFTER the
    // stream has drained -- so no kernel and no copy engine can hold an address of host memory that is not this context's own
    // for the context's whole life, whatever path a call returns by.  LWHIP_DEBUG: the block is never given back to the
    // runtime (quarantine, lwhip_api.hip) and its canary words are checked when the process ends.
    // peer exchange of the sharded iteration (lwhip_peer_*, lwhip_api.hip): this rank's window [flags 2 x LWHIP_PEER_MAX |
    // slots 2 x world x peerStride doubles] and the device addresses of every rank's window (own included)
    unsigned char* peerWin = nullptr;
    size_t peerWinBytes = 0, peerStride = 0;
    unsigned char* peerPtr[LWHIP_PEER_MAX] = {};
    bool peerIpc[LWHIP_PEER_MAX] = {};   // opened with hipIpcOpenMemHandle (closed in lwhip_peer_detach)
    bool peerOn = false;
    unsigned long long peerSeq = 0;      // exchanges so far (the next one uses buffer peerSeq & 1 with flag value peerSeq + 1)
    DevBuf<int32_t> peerArrive;
    size_t stateBytes = 0;         // what this context's alloc_state asked for (the size of a borrower's arena)
    unsigned char* stateArena = nullptr;
    // lwhip_map_host_J: the caller's J array page-locked and mapped; the sweep stores J there too
    void* JhostReg = nullptr;      // what was registered (prob.J)
    double* JhostDev = nullptr;    // device address of this shard's first row in it
    DevBuf<double> Jsnap;          // lwhip_j_snapshot
    DevBuf<unsigned long long> fpSums; // lwhip_fingerprint_J: the blocks' sums
    PinnedBlock fpPinned;
    bool fpJValid = false;         // fpJValue is the fingerprint of the device's current J as seen at address fpJPtr
    uint64_t fpJValue = 0;
    const void* fpJPtr = nullptr;
    unsigned char* hostBlock = nullptr;
    size_t hostBlockBytes = 0;
    int32_t* turnLateHost = nullptr;  // fixed-order mode: turn waits that timed out (device-written, TileArgs::turnLate)
    int32_t* turnLateDev = nullptr;
    int32_t* popStatusHost = nullptr; // device-to-host target of the status word of time_dep_update / nr_post_update
    int32_t* prdCtlHost = nullptr;    // ... of the stopping-rule words of the pipelined PRD sub-iterations

    ~lwhip_context()
    {
        // (a context that failed half-way through lwhip_create comes here without lwhip_destroy: nothing of it may be
        // released while its stream still runs)
        if (stream)
            (void)hipStreamSynchronize(stream);
        for (PinnedBlock* b : { &stage, &gatherPinned, &prdPinned, &prdPinnedPipe, &fpPinned, &lsDbg, &ng.pinned })
            b->release(); // (before the stream they were used on goes back to its pool)
        stokes_batch_release(stokesFs);
        rays_release(rays);
        rays2d_release(rays2d);
        for (auto& pr : pending)
        {
            (void)hipEventDestroy(pr.first);
            (void)hipEventDestroy(pr.second);
        }
        if (ownStream && ownStreamShared)
            stream_release_shared(device, ownStream);
        else if (ownStream)
            stream_release(device, ownStream); // (never hipStreamDestroy: see stream_acquire, lwhip_api.hip)
        peer_release(this);
        if (stateArena) // (the DevBufs that point into it do not own their pieces)
            (void)hipFree(stateArena);
        if (JhostReg)
            (void)hipHostUnregister(JhostReg);
        host_block_release(this);
    }
};

#define H2D(dst, src, count)                                                                           \
    HIP_TRY(c->mem.h2d((dst), (src), (size_t)(count) * sizeof(double)))
#define D2H(dst, src, count)                                                                           \
    HIP_TRY(hipMemcpyAsync((dst), (src), (size_t)(count) * sizeof(double), hipMemcpyDeviceToHost, c->stream))

namespace lwhip
{
inline int env_int(const char* name, int dflt)
{
    const char* v = std::getenv(name);
    if (!v || !*v)
        return dflt;
    return std::atoi(v);
}
// The layout / experiment knobs of tests and tools (tile widths, wavefronts per workgroup, split factors, forced kinds: the list
// is in INTEGRATION.md section 5) are read only when LWHIP_DEBUG is set: a production process cannot change the work
// distribution -- or the summation order -- through a stray environment variable.
inline bool debug_knobs_on()
{
    static const bool on = std::getenv("LWHIP_DEBUG") != nullptr;
    return on;
}
inline int dbg_env_int(const char* name, int dflt) { return debug_knobs_on() ? env_int(name, dflt) : dflt; }

inline double trans_wlambda(const lwhip_transition& t, int lt)
{
    // Transition::wlambda, LwTransition.hpp:71-81
    const int len = t.Nred - t.Nblue;
    if (lt == 0)
        return 0.5 * (t.wavelength[1] - t.wavelength[0]) * t.dopplerWidth;
    if (lt == len - 1)
        return 0.5 * (t.wavelength[len - 1] - t.wavelength[len - 2]) * t.dopplerWidth;
    return 0.5 * (t.wavelength[lt + 1] - t.wavelength[lt - 1]) * t.dopplerWidth;
}

// lwhip_tables.hip
int validate(const lwhip_problem* p, std::string& why);
uint64_t structure_signature(const lwhip_context* c);
// the context's host fields from the descriptor and the options (no device needed); refuses a bad shard or rank
int context_init_host(lwhip_context* c, const lwhip_problem* prob, const lwhip_options* opts);
TableKnobs read_table_knobs();
int plan_tables(const lwhip_context& c, const TableKnobs& k, int numCU, TablePlan& p, HostTables& ht); // device-free
int upload_tables(lwhip_context* c, const TablePlan& p, const HostTables& ht);
int build_tables(lwhip_context* c); // knobs, compute-unit count, plan, upload
uint64_t plan_signature(const TablePlan& p); // lwhip_tables_signature's second word
// lwhip_state.hip
int alloc_state(lwhip_context* c);
int build_sweep_args(lwhip_context* c);
int build_tile_args(lwhip_context* c);
int retile_profiles(lwhip_context* c);
bool retile_args(lwhip_context* c, RetileArgs& r);
TileDyn make_dyn(lwhip_context* c, bool upOnly, int lambdaIterate);
hipError_t run_sweep(lwhip_context* c, const TileDyn& dyn, bool rates, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);
int flush_prefill(lwhip_context* c);
int verify_zero_check(lwhip_context* c);
int collect_profile(lwhip_context* c);
// lwhip_api.hip
ReduceArgs make_reduce_args(lwhip_context* c);
ApplyArgs make_apply_args(lwhip_context* c);
int ensure_profiles(lwhip_context* c);
int voigt_line_list(lwhip_context* c, std::vector<VoigtLineArgs>& out);
int stat_equil_impl(lwhip_context* c, int atom, bool wait, double* dPops = nullptr, int32_t* dPopsMaxIdx = nullptr);
int solved_atoms(const lwhip_context* c, int atom, std::vector<NrAtom>& atoms); // atom -1: all that are not detailed; returns maxNl
StatEqArgs stat_eq_args(const lwhip_context* c, int Natoms);                    // ... and their solve over the context's depth range
// the context's phi / wphi were just made on the device from (aDamp, vBroad, vlosMu): the Voigt arguments of the two directions of
// an angle differ by the sign of the line-of-sight velocity alone, those of two angles by its projection alone
inline void profiles_made_on_device(lwhip_context* c)
{
    c->deviceProfiles = true;
    c->profilesStale = false;
    c->phiSym = c->vlosZero;
    c->phiIso = c->vlosZero;
}
// A batch's list of argument blocks goes to `dev` (copy; grown first if need be, once nothing can still read the buffer that is
// replaced) and is launched in pieces: the launch geometry allows 65 535 entries per grid dimension.
// (launch: a function or a closure (const T* dev, const T* host, int n, hipStream_t) -> hipError_t)
template <class T, class F>
int launch_list(lwhip_context* c0, DevBuf<T>& dev, const std::vector<T>& list, bool copy, F launch)
{
    if (list.empty())
        return LWHIP_OK;
    if (copy && dev.n < list.size())
    {
        HIP_TRY(hipStreamSynchronize(c0->stream));
        HIP_TRY(dev.alloc(c0->mem, list.size(), false));
    }
    if (copy)
        HIP_TRY(hipMemcpyAsync(dev.p, list.data(), list.size() * sizeof(T), hipMemcpyHostToDevice, c0->stream));
    for (size_t off = 0; off < list.size(); off += 32768)
        HIP_TRY(launch(dev.p + off, list.data() + off, (int)std::min<size_t>(32768, list.size() - off), c0->stream));
    return LWHIP_OK;
}
// lwhip_api2d.hip
int run_2d(lwhip_context* c, int lambdaIterate, int mode = 0);
// lwhip_api_prd.hip
enum { PRD_PIPE_DEPTH = 4 }; // sub-iterations queued per host round trip (lwhip_redistribute_prd, lwhip_batch_redistribute_prd)
// redistribute_prd needs the collisional rates C of every atom with a PRD line: the refusal of both entry points
int prd_check_collisions(const lwhip_context* c);
// The argument blocks of the context's PRD lines for one sub-iteration, out[Nprd] -- the scratch buffers of the scattering
// integral (grown first), the slices, the gII cache (made, or "recompute" where it cannot be allocated; a line whose block says
// gIIFill is marked filled: the launch that follows fills it) and the change buffers.  stopPos: PrdLineArgs::stopPos of every
// line.  A lone context launches its own list (lwhip_prd_partial), a column batch the columns' lists back to back.
int prd_build_line_args(lwhip_context* c, int stopPos, PrdLineArgs* out);
}

// ---- 1.5D column batches: one iteration of n structurally identical contexts in one set of launches (lwhip_batch.hip;
// their full-Stokes calls: lwhip_stokes_batch.hip, lwhip_stokes_fs.hip) ----------
// One per-column argument list of a batch.  Every batched kernel picks its column by list position, so the entries of the active
// columns alone (lwhip_batch_set_active), position p = column act[p], are all it needs to run a smaller batch -- and all
// columns are the set act = 0 .. n-1.
template <class T> struct ColList
{
    std::vector<T> full;   // every column's entry
    DevBuf<T> dev;         // made once, for all columns: the entries of the active ones, in the order of act
    std::vector<T> staged; // ... as the queued copy reads them
    hipError_t alloc(DevMem& mem, size_t n) // (lwhip_batch_create; every entry a launch reads is copied there first)
    {
        full.resize(n);
        return dev.alloc(mem, n, false);
    }
    hipError_t refresh(const std::vector<int32_t>& act, hipStream_t stream)
    {
        staged.resize(act.size());
        for (size_t p = 0; p < act.size(); ++p)
            staged[p] = full[act[p]];
        return hipMemcpyAsync(dev.p, staged.data(), staged.size() * sizeof(T), hipMemcpyHostToDevice, stream);
    }
};

struct lwhip_batch
{
    std::vector<lwhip_context*> ctxs;
    std::vector<hipStream_t> ownStreams; // what the columns ran on before they joined the batch
    // The active set (lwhip_batch_set_active) and the argument lists of its columns: refreshed together whenever the set
    // changes (batch_refresh_lists), except the apply blocks, which the next iteration rebuilds and uploads (aValid is off).
    std::vector<int32_t> act;            // the active columns, increasing (0 .. n-1 when all are)
    bool allActive = true;               // (then batch_conv_kernel / ng_kernel get no column list: batch_cols)
    DevBuf<int32_t> colsAct;             // act on the device
    ColList<const TileArgs*> ap;
    ColList<ReduceArgs> r;
    ColList<ApplyArgs> a;
    ColList<StatEqArgs> se, seRep;       // stat_equil of all solved atoms of every column; seRep: change -> `change` below
    double aCrsw = 0.0;                  // what the device copy of the apply blocks was built with
    bool aValid = false;
    StatEqArgs se0{};
    int seMaxNl = 0;
    DevBuf<double> tail;                 // [n][2] (dJMax, idx) of every column
    PinnedBlock tailPinned;
    // lwhip_batch_stat_equil_report
    int seBlocks = 0;                    // solve blocks per atom and column
    DevBuf<double> change;               // [n][Natoms][seBlocks][2], what stat_eq_body writes per column
    DevBuf<double> rec;                  // [n][2 + 2 Natoms]: dJMax, idx, then (dPops, idx) per atom
    PinnedBlock recPinned;
    std::vector<int32_t> recCols;        // the columns the last report solved (whose rows of recPinned are its)
    // lwhip_batch_time_dep_update / lwhip_batch_nr_post_update: everything a call sends -- the active columns' argument blocks
    // in list order, then their arrays -- is staged in ONE pinned block and goes up in one copy
    PinnedBlock popStage;
    DevBuf<unsigned char> popIn;         // ... its landing place, laid out as the stage
    int nrBlocks = 0;                    // Newton-Raphson blocks per column (the block size follows Neqn, not seMaxNl)
    DevBuf<double> nrChange;             // [n][Natoms][nrBlocks][2]; zero in the slots of solved atoms the call does not list
    std::vector<int32_t> nrListed;       // the atom list those zeros are right for
    // lwhip_batch_redistribute_prd: the lists of the PRD rates pass, made by the first call and refreshed
    // by a call that finds another active set than the last one did (prdAct); the lines' argument blocks of the active
    // columns back to back, position-major, uploaded when they change; the PRD pass's own (dJMax, idx) tail; the records of a
    // group of sub-iterations [PRD_PIPE_DEPTH][n][2 (1 + Nprd)] with the int32 stop words [n] behind them -- one copy per group
    ColList<const TileArgs*> apPrd;      // the columns' dtargsPrd
    ColList<ReduceArgs> rPrd;            // stage 2 with batchTail -> prdTail
    ColList<ApplyArgs> aPrd;             // the PRD lines' rates out (prdOnly)
    std::vector<int32_t> prdAct;         // the set those lists' device copies hold
    DevBuf<double> prdTail;              // [n][2]
    DevBuf<PrdLineArgs> prdLines;
    std::vector<PrdLineArgs> prdLinesHost; // what the device copy holds
    DevBuf<double> prdRec;
    int prdRecNprd = -1;                 // the line count prdRec was sized for
    PinnedBlock prdRecPinned;
    // hybrid PRD (every column made with lwhip_options.hprd, or none): the columns' wavelength headers and with them their tile
    // lists follow their own velocity fields, so their sweep launches differ in their workgroup counts (batch_sweep_geom); zr:
    // each column's JRest, cleared in one launch in front of every pass that rebuilds it
    bool hybrid = false;
    ColList<ZeroArgs> zr;
    uint64_t zrMax = 0;                  // the longest JRest, in doubles
    NgState ng;                                // lwhip_batch_ng_configure: Ng acceleration of every column
    DevBuf<VoigtLineArgs> voigtList; // lines of the columns whose profiles are being recomputed
    DevBuf<RetileArgs> retileList;   // ... and their retile arguments
    DevBuf<PolLineArgs> polList;     // every column's polarised lines, as polHost (lwhip_batch_compute_polarised_profiles)
    std::vector<PolLineArgs> polHost;
    StokesBatch* stokes = nullptr;   // made by the first lwhip_batch_full_stokes_fs
    RaysState* rays = nullptr;       // made by the first lwhip_batch_compute_rays
};

namespace lwhip
{
// lwhip_batch.hip
int batch_ensure_profiles(lwhip_batch* b);                                  // the columns whose profiles went stale
int batch_retile(lwhip_batch* b, const std::vector<lwhip_context*>& cols); // tile-blocked copies of their phi, one launch list
// lwhip_stokes_batch.hip: the refusals the batch's Stokes entry points share
int check_stokes_batch(lwhip_batch* b, const char* what);
// Every refusal of an observer-ray request, before anything is queued (lwhip_rays.hip); la0 / la1: the rows of the global grid it
// asks for.  anySolver: the full-Stokes observer rays, which like lwhip_full_stokes_fs ignore the context's formal solver.
// hybrid: the calls that serve hybrid-PRD contexts (lwhip_compute_rays_hprd and its kin) -- they need the tables every other
// call refuses.
int rays_check(lwhip_context* c, const lwhip_rays* r, const std::string& what, bool anySolver, int& la0, int& la1,
               bool hybrid = false);
}
