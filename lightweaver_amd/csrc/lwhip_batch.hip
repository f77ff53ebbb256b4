// lwhip_batch.hip -- host side of the C ABI (lwhip_host.h): 1.5D column batches -- one iteration of n structurally identical
// contexts in one set of launches.
#include "lwhip_host.h"

// (struct lwhip_batch: lwhip_host.h)

// device profiles of the batch's columns: every line of every column that needs them (all = the explicit
// lwhip_batch_compute_profiles, else those whose atmosphere was uploaded since) in ONE launch pair on the batch's stream
static int batch_compute_profiles(lwhip_batch* b, bool all)
{
    std::vector<VoigtLineArgs> list;
    std::vector<lwhip_context*> todo;
    for (lwhip_context* c : b->ctxs)
    {
        if (!(all || c->profilesStale))
            continue;
        const int st = voigt_line_list(c, list);
        if (st != LWHIP_OK)
            return st;
        todo.push_back(c);
    }
    if (todo.empty())
        return LWHIP_OK;
    const int st = launch_list(b->ctxs[0], b->voigtList, list, true, launch_voigt_lines);
    if (st != LWHIP_OK)
        return st;
    // ... and their tile-blocked copies, one grid slice per column
    for (lwhip_context* c : todo)
        profiles_made_on_device(c);
    return batch_retile(b, todo);
}

// one sweep launch for all columns: the lane sweep's plain instance only if every column's own launch would take it (the
// rule of the pair flags: lwhip_batch_formal_sol_gamma_matrices)
static bool batch_plain_ok(const lwhip_batch* b, const TileDyn& dyn)
{
    for (const lwhip_context* c : b->ctxs)
        if (!c->lsPlain || !lane_sweep_plain(c->htargs, dyn, b->ctxs[0]->prob.formalSolver, true))
            return false;
    return true;
}

// the geometry of the batch's one lane-sweep launch (prd: of the PRD rates pass): gridDim.x and the dynamic LDS.  Hybrid
// columns differ in both: the largest of the active columns' (TileArgs::nWg ends a column's surplus workgroups; each column lays
// out its LDS from its own maxCT).  Otherwise the first column's, which lwhip_batch_create has compared the others with.
static void batch_sweep_geom(const lwhip_batch* b, bool prd, const std::vector<int32_t>& cols, int& wg, size_t& lds)
{
    const lwhip_context* c0 = b->ctxs[0];
    wg = prd ? c0->nTileChunksPrd : c0->nTileChunks;
    lds = 0;
    if (!b->hybrid)
        return;
    wg = 0;
    for (const int32_t i : cols)
    {
        const lwhip_context* c = b->ctxs[i];
        wg = std::max(wg, prd ? c->nTileChunksPrd : c->nTileChunks);
        lds = std::max(lds, lane_sweep_lds_bytes(prd ? c->htargsPrd : c->htargs, c->tileWaves));
    }
}

// the argument lists of the active set (lwhip_batch_set_active; all columns: lwhip_batch_create) go to the device, ordered on the
// batch's stream behind the launches that read the last set.  (The apply blocks follow in the next
// lwhip_batch_formal_sol_gamma_matrices: aValid is off.)
static int batch_refresh_lists(lwhip_batch* b)
{
    lwhip_context* c0 = b->ctxs[0];
    HIP_TRY(b->ap.refresh(b->act, c0->stream));
    HIP_TRY(b->r.refresh(b->act, c0->stream));
    HIP_TRY(b->se.refresh(b->act, c0->stream));
    HIP_TRY(b->seRep.refresh(b->act, c0->stream));
    if (b->hybrid)
        HIP_TRY(b->zr.refresh(b->act, c0->stream));
    HIP_TRY(hipMemcpyAsync(b->colsAct.p, b->act.data(), b->act.size() * sizeof(int32_t), hipMemcpyHostToDevice, c0->stream));
    HIP_TRY(hipStreamSynchronize(c0->stream)); // (what the copies read changes with the next set; a change of set is rare)
    return LWHIP_OK;
}

// what batch_conv_kernel and ng_kernel get to find a list position's column: nothing when every column is active
static const int32_t* batch_cols(const lwhip_batch* b) { return b->allActive ? nullptr : b->colsAct.p; }

// every entry point's opening: the batch is there, and its device is the current one
static int batch_enter(lwhip_batch* b, const char* what, lwhip_context*& c0)
{
    if (!b || b->ctxs.empty())
        return fail(LWHIP_ERR_INVALID, what);
    c0 = b->ctxs[0];
    HIP_TRY(hipSetDevice(c0->device));
    return LWHIP_OK;
}

// the status words of the columns just solved: the first singular one is reported (and cleared)
static int batch_singular(lwhip_batch* b)
{
    for (const int32_t i : b->act)
    {
        lwhip_context* c = b->ctxs[i];
        if (*c->statusHost == LWHIP_ERR_SINGULAR)
        {
            *c->statusHost = 0;
            return fail(LWHIP_ERR_SINGULAR, "Singular Matrix");
        }
    }
    return LWHIP_OK;
}

// the Ng step of the active columns, queued behind their solve
static hipError_t batch_ng_step(lwhip_batch* b)
{
    return ng_step(b->ng, batch_cols(b), (int)b->act.size(), b->ctxs[0]->stream);
}

// stat_equil of the active columns in one launch, their Ng step behind it when Ng is on, and one stream wait.  report: the
// columns' changes -- with Ng its max_change, taken after any extrapolation (rel_diff_ng_accelerate,
// Source/LwMiddleLayer.pyx:3318-3346), one (value, index) pair per column and atom; else what the solve writes when its arguments
// aim at `change` (seRep) -- become one record per column (batch_conv_kernel), which one copy brings back.
static int batch_solve(lwhip_batch* b, bool report, const char* what, double* dPops, int32_t* dPopsMaxIdx)
{
    lwhip_context* c0 = nullptr;
    if (const int st = batch_enter(b, what, c0); st != LWHIP_OK)
        return st;
    const int Na = b->se0.Natoms, nAct = (int)b->act.size();
    if (Na <= 0)
        return LWHIP_OK;
    for (const int32_t i : b->act)
    {
        lwhip_context* c = b->ctxs[i];
        const int stp = flush_prefill(c);
        if (stp != LWHIP_OK)
            return stp;
        *c->statusHost = 0;
    }
    const bool ownChange = report && !b->ng.on;
    HIP_TRY(launch_stat_eq(b->se0, b->seMaxNl, c0->stream, ownChange ? b->seRep.dev.p : b->se.dev.p, nAct));
    if (b->ng.on)
        HIP_TRY(batch_ng_step(b));
    const size_t stride = 2 + 2 * (size_t)Na;
    if (report)
    {
        BatchConvArgs ca{};
        ca.tail = b->tail.p;
        ca.rec = b->rec.p;
        ca.cols = batch_cols(b);
        ca.Natoms = Na;
        ca.change = ownChange ? b->change.p : b->ng.out.p;
        ca.nBlocks = ownChange ? b->seBlocks : 1;
        HIP_TRY(launch_batch_conv(ca, nAct, c0->stream));
        HIP_TRY(hipMemcpyAsync(b->recPinned.host, b->rec.p, b->ctxs.size() * stride * sizeof(double), hipMemcpyDeviceToHost, c0->stream));
    }
    HIP_TRY(hipStreamSynchronize(c0->stream));
    if (report)
        b->recCols = b->act;
    const int st = batch_singular(b);
    if (st != LWHIP_OK || !report)
        return st;
    const double* rec = b->recPinned.as<double>();
    for (const int32_t i : b->act)
        for (int q = 0; q < Na; ++q)
        {
            dPops[(size_t)i * Na + q] = rec[i * stride + 2 + 2 * q];
            if (dPopsMaxIdx)
                dPopsMaxIdx[(size_t)i * Na + q] = (int32_t)rec[i * stride + 3 + 2 * q];
        }
    return LWHIP_OK;
}

// lwhip_batch_time_dep_update / lwhip_batch_nr_post_update: room for what a call sends, in the pinned stage and on the device
// (both regrown, after a stream wait, when a request is larger; a call ends with a stream wait, so the stage is free here)
static int pop_stage(lwhip_batch* b, size_t bytes, unsigned char*& stage)
{
    lwhip_context* c0 = b->ctxs[0];
    if (b->popIn.n < bytes)
    {
        HIP_TRY(hipStreamSynchronize(c0->stream));
        HIP_TRY(b->popIn.alloc(c0->mem, bytes, false));
    }
    HIP_TRY(b->popStage.reserve(c0->device, bytes, c0->stream));
    stage = b->popStage.host;
    return LWHIP_OK;
}

// ... and what comes before their launch: every active column's pending Gamma pre-fill, its status word cleared
static int pop_begin(lwhip_batch* b)
{
    for (const int32_t i : b->act)
    {
        lwhip_context* c = b->ctxs[i];
        const int stp = flush_prefill(c);
        if (stp != LWHIP_OK)
            return stp;
        *c->statusHost = 0;
    }
    return LWHIP_OK;
}

namespace lwhip
{
int batch_retile(lwhip_batch* b, const std::vector<lwhip_context*>& cols)
{
    std::vector<RetileArgs> rl;
    for (lwhip_context* c : cols)
    {
        RetileArgs r;
        if (retile_args(c, r))
            rl.push_back(r);
    }
    return launch_list(b->ctxs[0], b->retileList, rl, true, launch_retile_list);
}
int batch_ensure_profiles(lwhip_batch* b) { return batch_compute_profiles(b, false); }
}

extern "C"
{
int lwhip_batch_create(lwhip_context* const* ctxs, int n, lwhip_batch** out)
{
    if (!ctxs || n < 1 || !out)
        return fail(LWHIP_ERR_INVALID, "batch_create: null argument");
    lwhip_context* c0 = ctxs[0];
    for (int i = 0; i < n; ++i)
    {
        lwhip_context* c = ctxs[i];
        if (!c)
            return fail(LWHIP_ERR_INVALID, "batch_create: null context");
        if (c->is2d || c->worldSize != 1)
            return fail(LWHIP_ERR_UNSUPPORTED, "batch_create: columns are 1D, unsharded contexts");
        if (c->deterministic)
            return fail(LWHIP_ERR_UNSUPPORTED, "batch_create: the fused batch sums by atomics (a context made with LWHIP_OPT_DETERMINISTIC "
                                               "iterates on its own)");
        // what the one launch fixes for every column ...
        const bool launchDiffers = c->device != c0->device || c->Ns != c0->Ns || c->Nla != c0->Nla || c->Nrays != c0->Nrays
                                   || c->Ntrans != c0->Ntrans || c->Natom != c0->Natom || c->tileCap != c0->tileCap
                                   || c->tileFuse != c0->tileFuse || c->tileWaves != c0->tileWaves || c->laneSweep != c0->laneSweep
                                   || c->maxL != c0->maxL || c->maxC != c0->maxC || c->NlevTot != c0->NlevTot
                                   || c->prob.formalSolver != c0->prob.formalSolver;
        // ... and the counts that follow a hybrid column's own velocity field (hasPrd of its wavelength headers is part of a
        // tile's identity): free when every column is hybrid and on the lane sweep, whose workgroups know their column's count
        const bool countsDiffer = c->nTiles != c0->nTiles || c->nTileChunks != c0->nTileChunks || c->nPostChunks != c0->nPostChunks
                                  || c->maxCTTile != c0->maxCTTile;
        if ((c->hprd != nullptr) != (c0->hprd != nullptr))
            return fail(LWHIP_ERR_INVALID, "batch_create: hybrid-PRD columns (lwhip_options.hprd) and plain ones do not share a "
                                           "batch: the sweep launch runs one instance for every column");
        if (launchDiffers || (countsDiffer && !(c0->hprd && c0->laneSweep)))
            return fail(LWHIP_ERR_INVALID, "batch_create: the columns must share device, model atoms, wavelength grid "
                                           "and solver");
    }
    HIP_TRY(hipSetDevice(c0->device));
    // the batch's launches go to the first column's stream; the other columns move onto it so that their own
    // uploads / downloads stay ordered with the batch
    std::vector<hipStream_t> before(n);
    for (int i = 0; i < n; ++i)
    {
        before[i] = ctxs[i]->stream;
        if (ctxs[i]->stream != c0->stream)
        {
            HIP_TRY(hipStreamSynchronize(ctxs[i]->stream));
            ctxs[i]->stream = c0->stream;
        }
    }
    auto b = std::make_unique<lwhip_batch>();
    b->ctxs.assign(ctxs, ctxs + n);
    b->ownStreams = before;
    b->hybrid = c0->hprd != nullptr && c0->laneSweep;
    if (b->hybrid)
    {
        HIP_TRY(b->zr.alloc(c0->mem, (size_t)n));
        for (int i = 0; i < n; ++i)
        {
            b->zr.full[i] = ZeroArgs{ ctxs[i]->JRest.p, (uint64_t)ctxs[i]->JRest.n };
            b->zrMax = std::max<uint64_t>(b->zrMax, ctxs[i]->JRest.n);
        }
    }
    HIP_TRY(b->ap.alloc(c0->mem, (size_t)n));
    HIP_TRY(b->r.alloc(c0->mem, (size_t)n));
    HIP_TRY(b->a.alloc(c0->mem, (size_t)n));
    HIP_TRY(b->se.alloc(c0->mem, (size_t)n));
    HIP_TRY(b->seRep.alloc(c0->mem, (size_t)n));
    HIP_TRY(b->colsAct.alloc(c0->mem, (size_t)n, false));
    b->act.resize(n);
    HIP_TRY(b->tail.alloc(c0->mem, (size_t)2 * n));
    for (int i = 0; i < n; ++i)
    {
        lwhip_context* c = ctxs[i];
        b->act[i] = i;
        b->ap.full[i] = c->dtargs.p;
        b->r.full[i] = make_reduce_args(c);
        b->r.full[i].batchTail = b->tail.p + 2 * (size_t)i;
        b->r.full[i].zeroParts = 1;
        // the columns' stage-1 buffers start clean (the sweep adds into them, stage 2 zeroes what it has summed)
        if (!c->red8Clean)
            HIP_TRY(hipMemsetAsync(c->red8.p, 0, c->red8.n * sizeof(double), c0->stream));
        c->red8Clean = true;
        // stat_equil of all its solved atoms, at every depth (a batch's solve does not follow lwhip_set_depth_range)
        std::vector<NrAtom> atoms;
        const int maxNl = solved_atoms(c, -1, atoms);
        if (!atoms.empty())
        {
            HIP_TRY(c->statEqAtoms.upload(c->mem, atoms));
            c->statEqKey = -1;
        }
        StatEqArgs& sa = b->se.full[i] = stat_eq_args(c, (int)atoms.size());
        sa.k0 = 0;
        sa.k1 = c->Ns;
        if (i == 0)
        {
            b->se0 = sa;
            b->seMaxNl = maxNl;
        }
        else if (sa.Natoms != b->se0.Natoms || maxNl != b->seMaxNl)
            return fail(LWHIP_ERR_INVALID, "batch_create: the columns must share their active atoms");
    }
    // the reported solve: the change records of all columns, a second list of solve arguments that aims at them (the plain
    // solve keeps launching with `se`, whose change is null), and the records the columns' changes become
    const size_t Na = (size_t)std::max(b->se0.Natoms, 0);
    b->seBlocks = stat_eq_blocks(c0->Ns, b->seMaxNl);
    HIP_TRY(b->change.alloc(c0->mem, (size_t)n * Na * b->seBlocks * 2));
    b->seRep.full = b->se.full;
    for (int i = 0; i < n; ++i)
        b->seRep.full[i].change = b->change.p + (size_t)i * Na * b->seBlocks * 2;
    HIP_TRY(b->rec.alloc(c0->mem, (size_t)n * (2 + 2 * Na)));
    HIP_TRY(b->recPinned.reserve(c0->device, (size_t)n * (2 + 2 * Na) * sizeof(double), c0->stream));
    HIP_TRY(b->tailPinned.reserve(c0->device, (size_t)2 * n * sizeof(double), c0->stream));
    const int st = batch_refresh_lists(b.get());
    if (st != LWHIP_OK)
        return st;
    *out = b.release();
    return LWHIP_OK;
}

void lwhip_batch_destroy(lwhip_batch* b)
{
    if (!b)
        return;
    // the columns go back to their own streams (the first column's may be destroyed before the others)
    if (!b->ctxs.empty())
    {
        (void)hipSetDevice(b->ctxs[0]->device);
        (void)hipStreamSynchronize(b->ctxs[0]->stream);
        b->tailPinned.release();
        b->popStage.release();
        b->prdRecPinned.release();
        stokes_batch_release(b->stokes);
        b->stokes = nullptr;
        rays_release(b->rays);
        b->rays = nullptr;
        for (size_t i = 0; i < b->ctxs.size() && i < b->ownStreams.size(); ++i)
            b->ctxs[i]->stream = b->ownStreams[i];
    }
    delete b;
}

int lwhip_batch_formal_sol_gamma_matrices(lwhip_batch* b, int lambdaIterate, double crsw, lwhip_iter_result* results)
{
    lwhip_context* c0 = nullptr;
    if (const int st = batch_enter(b, "null batch", c0); st != LWHIP_OK)
        return st;
    const int n = (int)b->ctxs.size();
    {
        // columns whose atmosphere was updated: their phi / wphi first, all their lines in one launch pair
        const int stp = batch_ensure_profiles(b);
        if (stp != LWHIP_OK)
            return stp;
    }
    // the columns this call launches: the active set (lwhip_batch_set_active), whose entries the lists' device copies hold
    const int nAct = (int)b->act.size();
    const TileArgs* const* apL = b->ap.dev.p;
    // Gamma <- crsw * C of every column is fused into its slice of the apply launch
    for (const int32_t i : b->act)
    {
        lwhip_context* c = b->ctxs[i];
        if (c->partialPending || c->prdPending)
            return fail(LWHIP_ERR_INVALID, "batch iteration while a split iteration of a column is pending");
        c->prefillCrsw = crsw;
        c->dJPrdClean = false; // (the batch sweep writes every wavelength's dJ)
        c->prefillPending = c->gammaTot > 0 && c->Cmat.p != nullptr;
        b->a.full[i] = make_apply_args(c);
        c->prefillPending = false;
    }
    if (!b->aValid || b->aCrsw != crsw)
    {
        HIP_TRY(b->a.refresh(b->act, c0->stream));
        b->aValid = true;
        b->aCrsw = crsw;
    }
    // one set of launches for all columns: pre-pass, sweep (each workgroup finishes its tile when fused), stage 2
    TileDyn dyn = make_dyn(c0, false, lambdaIterate);
    for (int q = 0; q < n && dyn.phiSym; ++q) // (one launch for all columns: pairs only if every column's profiles are symmetric)
        dyn.phiSym = b->ctxs[q]->phiSym ? 1 : 0;
    for (int q = 0; q < n && dyn.phiIso; ++q) // (... and one stencil set per wavefront only if every column's are angle-independent)
        dyn.phiIso = (b->ctxs[q]->phiIso && dyn.phiSym) ? 1 : 0;
    const bool fuse = c0->tileFuse;
    if (!c0->laneSweep) // (the lane sweep's tasks do their own pre-pass)
        HIP_TRY(launch_tile_pre(c0->dtargs.p, c0->htargs, c0->nTiles, apL, nAct, c0->stream));
    if (c0->laneSweep)
    {
        // hybrid PRD: the rest-frame mean intensity is rebuilt by every pass that updates J (run_sweep of a lone context)
        if (b->hybrid)
            HIP_TRY(launch_batch_zero_jrest(b->zr.dev.p, b->zrMax, nAct, c0->stream));
        int wg = 0;
        size_t lds = 0;
        batch_sweep_geom(b, false, b->act, wg, lds);
        HIP_TRY(launch_lane_sweep(c0->dtargs.p, c0->htargs, dyn, c0->prob.formalSolver, true, wg, c0->tileWaves, apL, nAct, c0->stream,
                                  batch_plain_ok(b, dyn), lds));
    }
    else
    {
        HIP_TRY(launch_tile_sweep(c0->dtargs.p, c0->htargs, dyn, c0->prob.formalSolver, c0->tileCap, true, fuse, c0->nTileChunks,
                                  c0->tileWaves, apL, nAct, c0->stream));
        if (!fuse)
            HIP_TRY(launch_tile_post(c0->dtargs.p, c0->htargs, dyn, c0->nPostChunks, apL, nAct, c0->stream));
    }
    {
        ReduceArgs r0 = make_reduce_args(c0);
        r0.zeroParts = 1;
        HIP_TRY(launch_reduce_sum(r0, c0->stream, b->r.dev.p, nAct));
    }
    if (c0->Natom > 0)
        HIP_TRY(launch_apply(b->a.full[b->act[0]], c0->stream, b->a.dev.p, nAct));
    if (results)
    {
        HIP_TRY(hipMemcpyAsync(b->tailPinned.host, b->tail.p, (size_t)2 * n * sizeof(double), hipMemcpyDeviceToHost, c0->stream));
        HIP_TRY(hipStreamSynchronize(c0->stream));
        for (const int32_t i : b->act) // (entries of inactive columns stay as the caller filled them)
        {
            results[i].updatedJ = 1;
            results[i].dJMax = b->tailPinned.as<double>()[2 * i];
            results[i].dJMaxIdx = (int32_t)b->tailPinned.as<double>()[2 * i + 1];
        }
    }
    return LWHIP_OK;
}

int lwhip_batch_compute_profiles(lwhip_batch* b)
{
    lwhip_context* c0 = nullptr;
    const int st = batch_enter(b, "null batch", c0);
    return st != LWHIP_OK ? st : batch_compute_profiles(b, true);
}

int lwhip_batch_sweep_instance(lwhip_batch* b, int32_t out[4])
{
    if (!b || b->ctxs.empty() || !out)
        return fail(LWHIP_ERR_INVALID, "batch_sweep_instance: null argument");
    // (what lwhip_batch_formal_sol_gamma_matrices passes its one sweep launch; out[1] is not reported for a batch)
    const lwhip_context* c0 = b->ctxs[0];
    const bool lanes = c0->laneSweep && c0->tiled;
    bool sw = true;
    for (const lwhip_context* c : b->ctxs)
        sw = sw && c->lsPlain;
    out[0] = (lanes && batch_plain_ok(b, make_dyn(b->ctxs[0], false, 0))) ? 1 : 0;
    out[1] = 0;
    out[2] = lanes ? 1 : 0;
    out[3] = sw ? 1 : 0;
    return LWHIP_OK;
}

int lwhip_batch_sweep_shape(lwhip_batch* b, int32_t* perColumn, int32_t launch[2])
{
    if (!b || b->ctxs.empty() || !perColumn || !launch)
        return fail(LWHIP_ERR_INVALID, "batch_sweep_shape: null argument");
    const lwhip_context* c0 = b->ctxs[0];
    const bool lanes = c0->laneSweep && c0->tiled;
    for (size_t i = 0; i < b->ctxs.size(); ++i)
    {
        perColumn[2 * i] = b->ctxs[i]->nTileChunks;
        perColumn[2 * i + 1] = b->ctxs[i]->nTileChunksPrd;
    }
    // (what the active set's launches pass as gridDim.x; the fused PRD pass exists on the lane sweep only)
    size_t lds = 0;
    int wg = 0, wgPrd = 0;
    batch_sweep_geom(b, false, b->act, wg, lds);
    batch_sweep_geom(b, true, b->act, wgPrd, lds);
    launch[0] = wg;
    launch[1] = lanes ? wgPrd : 0;
    return LWHIP_OK;
}

int lwhip_batch_stat_equil(lwhip_batch* b) { return batch_solve(b, false, "null batch", nullptr, nullptr); }

int lwhip_batch_stat_equil_report(lwhip_batch* b, double* dPops, int32_t* dPopsMaxIdx)
{
    const char* what = "batch_stat_equil_report: null argument";
    return dPops ? batch_solve(b, true, what, dPops, dPopsMaxIdx) : fail(LWHIP_ERR_INVALID, what);
}

int lwhip_batch_time_dep_update(lwhip_batch* b, const double* const* nOld, const double* dt, double* dPops, int32_t* dPopsMaxIdx)
{
    lwhip_context* c0 = nullptr;
    if (const int st = batch_enter(b, "batch_time_dep_update: null batch", c0); st != LWHIP_OK)
        return st;
    if (!nOld || !dt)
        return fail(LWHIP_ERR_INVALID, "batch_time_dep_update: null argument");
    const int Na = b->se0.Natoms, nAct = (int)b->act.size();
    if (Na <= 0)
        return LWHIP_OK;
    for (const int32_t i : b->act)
        if (!nOld[i])
            return fail(LWHIP_ERR_INVALID, "batch_time_dep_update: column " + std::to_string(i) + " has no nOld");
    const size_t Ns = (size_t)c0->Ns;
    size_t rows = 0; // of nOld, per column: the solved atoms' levels
    for (int ia = 0; ia < c0->Natom; ++ia)
        if (!c0->atoms[ia].detailed)
            rows += (size_t)c0->atoms[ia].Nlevel;
    const size_t per = rows * Ns, oldOff = (size_t)nAct * sizeof(TimeDepArgs);
    unsigned char* stage = nullptr;
    if (const int st = pop_stage(b, oldOff + (size_t)nAct * per * sizeof(double), stage); st != LWHIP_OK)
        return st;
    TimeDepArgs* args = (TimeDepArgs*)stage;
    for (int p = 0; p < nAct; ++p)
    {
        const int32_t i = b->act[p];
        lwhip_context* c = b->ctxs[i];
        TimeDepArgs& a = args[p];
        a.Ns = c->Ns;
        a.Natoms = Na;
        a.atoms = b->se.full[i].atoms;
        a.n = c->n.p;
        a.Gamma = c->Gamma.p;
        a.nOld = (const double*)(b->popIn.p + oldOff) + (size_t)p * per;
        a.dt = dt[i];
        a.status = c->statusDev;
        a.change = b->change.p + (size_t)i * Na * b->seBlocks * 2;
        std::memcpy(stage + oldOff + (size_t)p * per * sizeof(double), nOld[i], per * sizeof(double));
    }
    if (const int st = pop_begin(b); st != LWHIP_OK)
        return st;
    HIP_TRY(hipMemcpyAsync(b->popIn.p, stage, oldOff + (size_t)nAct * per * sizeof(double), hipMemcpyHostToDevice, c0->stream));
    HIP_TRY(launch_time_dep_list((const TimeDepArgs*)b->popIn.p, c0->Ns, Na, b->seMaxNl, nAct, c0->stream));
    BatchConvArgs ca{};
    ca.tail = b->tail.p;
    ca.rec = b->rec.p;
    ca.cols = batch_cols(b);
    ca.Natoms = Na;
    ca.change = b->change.p;
    ca.nBlocks = b->seBlocks;
    HIP_TRY(launch_batch_conv(ca, nAct, c0->stream));
    const size_t stride = 2 + 2 * (size_t)Na;
    HIP_TRY(hipMemcpyAsync(b->recPinned.host, b->rec.p, b->ctxs.size() * stride * sizeof(double), hipMemcpyDeviceToHost, c0->stream));
    HIP_TRY(hipStreamSynchronize(c0->stream));
    b->recCols = b->act;
    if (const int st = batch_singular(b); st != LWHIP_OK)
        return st;
    const double* rec = b->recPinned.as<double>();
    for (const int32_t i : b->act)
        for (int q = 0; q < Na; ++q)
        {
            if (dPops)
                dPops[(size_t)i * Na + q] = rec[i * stride + 2 + 2 * q];
            if (dPopsMaxIdx)
                dPopsMaxIdx[(size_t)i * Na + q] = (int32_t)rec[i * stride + 3 + 2 * q];
        }
    return LWHIP_OK;
}

int lwhip_batch_nr_post_update(lwhip_batch* b, const lwhip_nr_args* perColumn, double* dPops, int32_t* dPopsMaxIdx)
{
    lwhip_context* c0 = nullptr;
    if (const int st = batch_enter(b, "batch_nr_post_update: null batch", c0); st != LWHIP_OK)
        return st;
    if (!perColumn)
        return fail(LWHIP_ERR_INVALID, "batch_nr_post_update: null argument");
    const int Na = b->se0.Natoms, nAct = (int)b->act.size(), n = (int)b->ctxs.size();
    const size_t Ns = (size_t)c0->Ns;
    // ---- every refusal, before anything is queued: the first active column's list, then every column against it ----
    const lwhip_nr_args& f = perColumn[b->act[0]];
    const std::string what = "batch_nr_post_update: column ";
    if (!f.atoms || f.Natoms <= 0)
        return fail(LWHIP_ERR_INVALID, what + std::to_string(b->act[0]) + " lists no atoms");
    const int Nl = f.Natoms;
    std::vector<NrAtom> atoms(Nl);
    std::vector<int32_t> slots(Nl);
    int eq = 0;
    int64_t dcRows = 0;
    for (int q = 0; q < Nl; ++q)
    {
        const int ia = f.atoms[q];
        if (ia < 0 || ia >= c0->Natom || c0->atoms[ia].detailed)
            return fail(LWHIP_ERR_INVALID, "batch_nr_post_update: not an active atom");
        NrAtom& at = atoms[q];
        at.atom = ia;
        at.Nlevel = c0->atoms[ia].Nlevel;
        at.levelOff = c0->levelOff[ia];
        at.eqOff = eq;
        at.trBegin = c0->atomTrOff[ia];
        at.trEnd = c0->atomTrOff[ia + 1];
        at.gammaOff = c0->gammaOff[ia];
        at.dcOff = dcRows;
        eq += at.Nlevel;
        dcRows += (int64_t)at.Nlevel * at.Nlevel;
        slots[q] = 0; // its position among the solved atoms
        for (int ib = 0; ib < ia; ++ib)
            slots[q] += c0->atoms[ib].detailed ? 0 : 1;
    }
    const bool timeDep = f.nPrev != nullptr, fdC = f.dC != nullptr;
    for (const int32_t i : b->act)
    {
        const lwhip_nr_args& g = perColumn[i];
        const lwhip_context* c = b->ctxs[i];
        const std::string col = what + std::to_string(i);
        if (!g.atoms || !g.stages || !g.ne || !g.backgroundNe)
            return fail(LWHIP_ERR_INVALID, col + ": null atoms, stages, ne or backgroundNe");
        if (g.Natoms != Nl || !std::equal(g.atoms, g.atoms + Nl, f.atoms) || (g.nPrev != nullptr) != timeDep || (g.dC != nullptr) != fdC)
            return fail(LWHIP_ERR_INVALID, col + " differs from the first active column in its atom list or in the presence of dC / nPrev");
        for (int q = 0; q < Nl; ++q)
        {
            const NrAtom& at = atoms[q];
            if (!c->atoms[at.atom].C)
                return fail(LWHIP_ERR_INVALID, col + ": nr_post_update needs the collisional rates C of every listed atom");
            if (c->atoms[at.atom].Nlevel != at.Nlevel || c->levelOff[at.atom] != at.levelOff || c->gammaOff[at.atom] != at.gammaOff
                || c->atomTrOff[at.atom] != at.trBegin || c->atomTrOff[at.atom + 1] != at.trEnd)
                return fail(LWHIP_ERR_INVALID, col + ": the listed atoms are not laid out as the first column's");
            if (!g.stages[q] || (timeDep && !g.nPrev[q]) || (fdC && !g.dC[q]))
                return fail(LWHIP_ERR_INVALID, col + ": null stages, nPrev or dC of a listed atom");
        }
    }
    const int Neqn = eq + 1;
    if (Neqn > 64)
        return fail(LWHIP_ERR_UNSUPPORTED, "batch_nr_post_update: more than 63 coupled levels");
    // ---- the call's block: argument blocks | atoms | slots | stages | records | ne | backgroundNe | nPrev | dC ----
    const size_t stride = 2 + 2 * (size_t)Na, D = sizeof(double);
    const size_t atomsOff = (size_t)nAct * sizeof(NrListArgs);
    const size_t slotsOff = atomsOff + (size_t)Nl * sizeof(NrAtom);
    const size_t stagesOff = slotsOff + (((size_t)Nl * sizeof(int32_t) + 7) & ~(size_t)7);
    const size_t recOff = stagesOff + (size_t)nAct * eq * D;
    const size_t neOff = recOff + (size_t)n * stride * D;
    const size_t bgOff = neOff + (size_t)nAct * Ns * D;
    const size_t prevOff = bgOff + (size_t)nAct * Ns * D;
    const size_t dcOff = prevOff + (timeDep ? (size_t)nAct * eq * Ns * D : 0);
    const size_t total = dcOff + (fdC ? (size_t)nAct * dcRows * Ns * D : 0);
    unsigned char* stage = nullptr;
    if (const int st = pop_stage(b, total, stage); st != LWHIP_OK)
        return st;
    // the change records: one set of pairs per column, solved atom and block; the slots of atoms not listed stay zero
    const int nrBlocks = nr_post_blocks(c0->Ns, Neqn);
    if (b->nrBlocks != nrBlocks || !b->nrChange.p)
    {
        HIP_TRY(hipStreamSynchronize(c0->stream));
        HIP_TRY(b->nrChange.alloc_zero(c0->mem, (size_t)n * Na * nrBlocks * 2));
        b->nrBlocks = nrBlocks;
        b->nrListed = slots;
    }
    if (c0->transType.n < (size_t)std::max(c0->Ntrans, 1))
    {
        std::vector<int32_t> tt((size_t)std::max(c0->Ntrans, 1), 0);
        for (int tr = 0; tr < c0->Ntrans; ++tr)
            tt[tr] = c0->trans[tr].t.type;
        HIP_TRY(c0->transType.upload(c0->mem, tt));
    }
    unsigned char* dev = b->popIn.p;
    std::memcpy(stage + atomsOff, atoms.data(), (size_t)Nl * sizeof(NrAtom));
    std::memcpy(stage + slotsOff, slots.data(), (size_t)Nl * sizeof(int32_t));
    NrListArgs* args = (NrListArgs*)stage;
    for (int p = 0; p < nAct; ++p)
    {
        const int32_t i = b->act[p];
        lwhip_context* c = b->ctxs[i];
        const lwhip_nr_args& g = perColumn[i];
        double* hStages = (double*)(stage + stagesOff) + (size_t)p * eq;
        double* hPrev = (double*)(stage + prevOff) + (size_t)p * eq * Ns;
        double* hDC = (double*)(stage + dcOff) + (size_t)p * dcRows * Ns;
        for (int q = 0; q < Nl; ++q)
        {
            const NrAtom& at = atoms[q];
            std::memcpy(hStages + at.eqOff, g.stages[q], (size_t)at.Nlevel * D);
            if (timeDep)
                std::memcpy(hPrev + (size_t)at.eqOff * Ns, g.nPrev[q], (size_t)at.Nlevel * Ns * D);
            if (fdC)
                std::memcpy(hDC + (size_t)at.dcOff * Ns, g.dC[q], (size_t)at.Nlevel * at.Nlevel * Ns * D);
        }
        std::memcpy(stage + neOff + (size_t)p * Ns * D, g.ne, Ns * D);
        std::memcpy(stage + bgOff + (size_t)p * Ns * D, g.backgroundNe, Ns * D);
        NrListArgs& l = args[p];
        NrArgs& a = l.a;
        a = NrArgs{};
        a.Ns = (int32_t)Ns;
        a.Natoms = Nl;
        a.Neqn = Neqn;
        a.timeDep = timeDep ? 1 : 0;
        a.atoms = (const NrAtom*)(dev + atomsOff);
        a.Gamma = c->Gamma.p;
        a.Cmat = c->Cmat.p;
        a.n = c->n.p;
        a.nTotal = c->nTotal.p;
        a.stages = (const double*)(dev + stagesOff) + (size_t)p * eq;
        a.nPrev = timeDep ? (const double*)(dev + prevOff) + (size_t)p * eq * Ns : nullptr;
        a.dC = fdC ? (const double*)(dev + dcOff) + (size_t)p * dcRows * Ns : nullptr;
        a.backgroundNe = (const double*)(dev + bgOff) + (size_t)p * Ns;
        a.ne = (double*)(dev + neOff) + (size_t)p * Ns;
        a.transType = c0->transType.p;
        a.transLi = c->transLi.p;
        a.transLj = c->transLj.p;
        a.dt = g.dt;
        a.crsw = g.crsw;
        a.status = c->statusDev;
        a.k0 = 0;
        a.k1 = (int32_t)Ns;
        l.change = b->nrChange.p + (size_t)i * Na * nrBlocks * 2;
        l.slots = (const int32_t*)(dev + slotsOff);
    }
    if (const int st = pop_begin(b); st != LWHIP_OK)
        return st;
    if (b->nrListed != slots) // (rare: another atom list than the last call's -- what it left in other slots goes)
    {
        HIP_TRY(hipMemsetAsync(b->nrChange.p, 0, b->nrChange.n * sizeof(double), c0->stream));
        b->nrListed = slots;
    }
    HIP_TRY(hipMemcpyAsync(dev, stage, total, hipMemcpyHostToDevice, c0->stream));
    HIP_TRY(launch_nr_post(args[0].a, c0->stream, (const NrListArgs*)dev, nAct));
    BatchConvArgs ca{};
    ca.tail = b->tail.p;
    ca.rec = (double*)(dev + recOff);
    ca.cols = batch_cols(b);
    ca.Natoms = Na;
    ca.change = b->nrChange.p;
    ca.nBlocks = nrBlocks;
    HIP_TRY(launch_batch_conv(ca, nAct, c0->stream));
    // records and ne lie together: one copy back, one wait
    HIP_TRY(hipMemcpyAsync(stage + recOff, dev + recOff, bgOff - recOff, hipMemcpyDeviceToHost, c0->stream));
    HIP_TRY(hipStreamSynchronize(c0->stream));
    const double* rec = (const double*)(stage + recOff);
    double* recOut = b->recPinned.as<double>();
    for (int p = 0; p < nAct; ++p)
    {
        const int32_t i = b->act[p];
        std::memcpy(perColumn[i].ne, stage + neOff + (size_t)p * Ns * D, Ns * D);
        std::memcpy(recOut + i * stride, rec + i * stride, stride * D);
    }
    b->recCols = b->act;
    if (const int st = batch_singular(b); st != LWHIP_OK)
        return st;
    for (const int32_t i : b->act)
        for (int q = 0; q < Nl; ++q)
        {
            if (dPops)
                dPops[(size_t)i * Na + slots[q]] = rec[i * stride + 2 + 2 * slots[q]];
            if (dPopsMaxIdx)
                dPopsMaxIdx[(size_t)i * Na + slots[q]] = (int32_t)rec[i * stride + 3 + 2 * slots[q]];
        }
    return LWHIP_OK;
}

// ---- PRD sub-iterations of the active columns: lwhip_redistribute_prd of each, in one set of launches per sub-iteration --------
// Per sub-iteration: scattering integral over the columns' lines back to back -> (hybrid columns: their JRest to zero) -> PRD rates pass (the BATCH lane sweep over the
// columns' dtargsPrd) -> stage 2 (sums, the pass's dJMax into prdTail) -> apply (the PRD lines' rates out) -> record
// (batch_prd_conv_kernel).  A column stops by its own changes: its stop word, set by the record launch of the sub-iteration
// that met the tolerance, makes its slice of every later launch return at once.
static int batch_prd_lists(lwhip_batch* b, int Nprd)
{
    lwhip_context* c0 = b->ctxs[0];
    const size_t n = b->ctxs.size();
    if (b->apPrd.full.size() != n)
    {
        HIP_TRY(b->apPrd.alloc(c0->mem, n));
        HIP_TRY(b->rPrd.alloc(c0->mem, n));
        HIP_TRY(b->aPrd.alloc(c0->mem, n));
        HIP_TRY(b->prdTail.alloc(c0->mem, 2 * n));
        for (size_t i = 0; i < n; ++i)
        {
            lwhip_context* c = b->ctxs[i];
            b->apPrd.full[i] = c->dtargsPrd.p;
            ReduceArgs& r = b->rPrd.full[i] = make_reduce_args(c);
            r.batchTail = b->prdTail.p + 2 * i; // (b->tail keeps the formal solution's numbers)
            r.zeroParts = 1;
            ApplyArgs& ap = b->aPrd.full[i] = make_apply_args(c);
            ap.crsw = 0.0;
            ap.prefill = 0;
            ap.prdOnly = 1;
        }
        b->prdAct.clear();
    }
    if (b->prdAct != b->act)
    {
        HIP_TRY(hipStreamSynchronize(c0->stream)); // (the staged copies of the last set may still be read)
        HIP_TRY(b->apPrd.refresh(b->act, c0->stream));
        HIP_TRY(b->rPrd.refresh(b->act, c0->stream));
        HIP_TRY(b->aPrd.refresh(b->act, c0->stream));
        b->prdAct = b->act;
    }
    if (b->prdRecNprd != Nprd)
    {
        const size_t stride = 2 * (size_t)(1 + Nprd);
        const size_t doubles = (size_t)PRD_PIPE_DEPTH * n * stride + (n + 1) / 2;
        HIP_TRY(hipStreamSynchronize(c0->stream));
        HIP_TRY(b->prdRec.alloc_zero(c0->mem, doubles));
        HIP_TRY(b->prdRecPinned.reserve(c0->device, doubles * sizeof(double), c0->stream));
        b->prdRecNprd = Nprd;
    }
    return LWHIP_OK;
}

int lwhip_batch_redistribute_prd(lwhip_batch* b, int maxIter, double tol, lwhip_batch_prd_result* res)
{
    lwhip_context* c0 = nullptr;
    if (const int st = batch_enter(b, "batch_redistribute_prd: null batch", c0); st != LWHIP_OK)
        return st;
    if (!res || !res->NprdSubIter)
        return fail(LWHIP_ERR_INVALID, "batch_redistribute_prd: null result");
    // ---- every refusal, before anything is queued ----
    const int Nprd = (int)c0->prdLines.size();
    for (size_t i = 0; i < b->ctxs.size(); ++i)
    {
        const lwhip_context* c = b->ctxs[i];
        if (c->prdDetailed)
            return fail(LWHIP_ERR_UNSUPPORTED, "batch_redistribute_prd: columns made with LWHIP_OPT_PRD_DETAILED iterate as contexts of "
                                               "their own");
        // (columns on one table set share ONE host JRest: their results cannot both be delivered)
        for (size_t j = 0; c->hprd && j < i; ++j)
            if (b->ctxs[j]->hprd == c->hprd)
                return fail(LWHIP_ERR_UNSUPPORTED, "batch_redistribute_prd: columns " + std::to_string(j) + " and " + std::to_string(i)
                                                       + " share one set of hybrid-PRD tables (lwhip_hprd) and with it one JRest: each "
                                                         "column needs tables of its own");
    }
    for (const int32_t i : b->act)
    {
        const lwhip_context* c = b->ctxs[i];
        const std::string col = "batch_redistribute_prd: column " + std::to_string(i);
        if (c->partialPending || c->prdPending)
            return fail(LWHIP_ERR_INVALID, col + " has a split iteration or sub-iteration pending");
        // (hybrid columns: their PRD passes differ in workgroup count and split, which each workgroup reads from its own column)
        if ((int)c->prdLines.size() != Nprd
            || (!b->hybrid && (c->nTileChunksPrd != c0->nTileChunksPrd || c->laneSplitPrd != c0->laneSplitPrd)))
            return fail(LWHIP_ERR_INVALID, col + " does not share the first column's PRD lines");
        for (int q = 0; q < Nprd; ++q)
            if (c->trans[c->prdLines[q]].t.Nred - c->trans[c->prdLines[q]].t.Nblue
                != c0->trans[c0->prdLines[q]].t.Nred - c0->trans[c0->prdLines[q]].t.Nblue)
                return fail(LWHIP_ERR_INVALID, col + " does not share the first column's PRD lines");
        if (const int stc = prd_check_collisions(c); stc != LWHIP_OK)
            return stc;
    }
    res->Nprd = Nprd;
    for (const int32_t i : b->act) // (entries of inactive columns stay as the caller filled them)
        res->NprdSubIter[i] = 0;
    if (Nprd == 0 || maxIter <= 0)
        return LWHIP_OK;
    const int nAct = (int)b->act.size();
    auto out = [&](int32_t i, int it, const double* rec) { // the record of column i's sub-iteration `it` into the caller's arrays
        const size_t row = (size_t)i * maxIter + (it - 1);
        if (res->dJPrdMax)
            res->dJPrdMax[row] = rec[0];
        if (res->dJPrdMaxIdx)
            res->dJPrdMaxIdx[row] = (int32_t)rec[1];
        for (int q = 0; q < Nprd; ++q)
        {
            const int Nl = c0->trans[c0->prdLines[q]].t.Nred - c0->trans[c0->prdLines[q]].t.Nblue;
            if (res->dRho)
                res->dRho[row * Nprd + q] = rec[2 + 2 * q];
            if (res->dRhoMaxIdx) // (modulo Nlambda, as prd_read_results reports it)
                res->dRhoMaxIdx[row * Nprd + q] = (int32_t)rec[3 + 2 * q] % Nl;
        }
    };
    if (!c0->laneSweep)
    {
        // a batch on the ray-column march (deep columns, LWHIP_SWEEP=march): not fused -- each active column's own loop
        std::vector<double> dRho((size_t)maxIter * Nprd), dJ(maxIter), rec(2 * (size_t)(1 + Nprd));
        std::vector<int32_t> dRhoIdx((size_t)maxIter * Nprd), dJIdx(maxIter);
        for (const int32_t i : b->act)
        {
            lwhip_prd_result r1{ 0, 0, dRho.data(), dRhoIdx.data(), dJ.data(), dJIdx.data() };
            if (const int st = lwhip_redistribute_prd(b->ctxs[i], maxIter, tol, &r1); st != LWHIP_OK)
                return st;
            res->NprdSubIter[i] = r1.NprdSubIter;
            for (int it = 1; it <= r1.NprdSubIter; ++it)
            {
                rec[0] = dJ[it - 1];
                rec[1] = dJIdx[it - 1];
                for (int q = 0; q < Nprd; ++q)
                {
                    rec[2 + 2 * q] = dRho[(size_t)(it - 1) * Nprd + q];
                    rec[3 + 2 * q] = dRhoIdx[(size_t)(it - 1) * Nprd + q]; // (below Nlambda already)
                }
                out(i, it, rec.data());
            }
        }
        return LWHIP_OK;
    }
    // ---- the fused route ----
    if (const int stp = batch_ensure_profiles(b); stp != LWHIP_OK)
        return stp;
    if (const int stl = batch_prd_lists(b, Nprd); stl != LWHIP_OK)
        return stl;
    const size_t n = b->ctxs.size(), stride = 2 * (size_t)(1 + Nprd);
    const size_t recDoubles = (size_t)PRD_PIPE_DEPTH * n * stride;
    int32_t* stop = (int32_t*)(b->prdRec.p + recDoubles);
    HIP_TRY(hipMemsetAsync(stop, 0, n * sizeof(int32_t), c0->stream));
    // each column's dJ is zero outside the PRD wavelengths (once per call: every sub-iteration visits the same wavelengths), its
    // stage-1 buffer clean (the sweep adds into it, stage 2 zeroes what it has summed)
    HIP_TRY(launch_batch_zero_dj(b->rPrd.dev.p, c0->Nla, nAct, c0->stream));
    for (const int32_t i : b->act)
    {
        lwhip_context* c = b->ctxs[i];
        c->fpJValid = false; // (the rates pass rewrites J at the PRD wavelengths)
        c->dJPrdClean = true;
        if (!c->red8Clean)
            HIP_TRY(hipMemsetAsync(c->red8.p, 0, c->red8.n * sizeof(double), c0->stream));
        c->red8Clean = true;
    }
    // one sweep launch for all columns: the launch-wide choices over ALL columns, as lwhip_batch_formal_sol_gamma_matrices makes them
    TileDyn dyn = make_dyn(c0, false, 0);
    for (size_t q = 0; q < n && dyn.phiSym; ++q)
        dyn.phiSym = b->ctxs[q]->phiSym ? 1 : 0;
    for (size_t q = 0; q < n && dyn.phiIso; ++q)
        dyn.phiIso = (b->ctxs[q]->phiIso && dyn.phiSym) ? 1 : 0;
    dyn.prdOnly = 1;
    dyn.stopCtl = stop;
    bool plain = true;
    for (const lwhip_context* c : b->ctxs)
        plain = plain && c->lsPlain && lane_sweep_plain(c->htargsPrd, dyn, c0->prob.formalSolver, true);
    ReduceArgs r0 = make_reduce_args(c0);
    r0.zeroParts = 1;
    r0.stopCtl = stop;
    ApplyArgs a0 = b->aPrd.full[b->act[0]];
    a0.prdCtl = stop;
    BatchPrdConvArgs ca{};
    ca.tail = b->prdTail.p;
    ca.cols = batch_cols(b);
    ca.stop = stop;
    ca.tol = tol;
    ca.Nprd = Nprd;
    int wgPrd = 0;
    size_t ldsPrd = 0;
    batch_sweep_geom(b, true, b->act, wgPrd, ldsPrd);
    std::vector<PrdLineArgs> lines((size_t)nAct * Nprd);
    std::vector<int> count(nAct, 0);
    std::vector<char> done(nAct, 0);
    int iter = 0, nDone = 0;
    while (iter < maxIter && nDone < nAct)
    {
        const int nb = std::min((int)PRD_PIPE_DEPTH, maxIter - iter);
        for (int j = 0; j < nb; ++j)
        {
            const int it = iter + j + 1;
            // the lines' blocks change only when a buffer moves or a cache is filled: upload on change
            for (int p = 0; p < nAct; ++p)
                if (const int stb = prd_build_line_args(b->ctxs[b->act[p]], p, lines.data() + (size_t)p * Nprd); stb != LWHIP_OK)
                    return stb;
            if (b->prdLinesHost.size() != lines.size()
                || std::memcmp(b->prdLinesHost.data(), lines.data(), lines.size() * sizeof(PrdLineArgs)) != 0)
            {
                HIP_TRY(hipStreamSynchronize(c0->stream)); // the previous copy may still be read
                b->prdLinesHost = lines;
                if (b->prdLines.n < lines.size())
                    HIP_TRY(b->prdLines.alloc(c0->mem, lines.size(), false));
                HIP_TRY(hipMemcpyAsync(b->prdLines.p, b->prdLinesHost.data(), lines.size() * sizeof(PrdLineArgs), hipMemcpyHostToDevice,
                                       c0->stream));
            }
            const int stsc = launch_list(c0, b->prdLines, b->prdLinesHost, false,
                                         [&](const PrdLineArgs* dev, const PrdLineArgs* host, int nl, hipStream_t s) {
                                             return launch_prd_scatter(dev, host, nl, s, false, stop, it);
                                         });
            if (stsc != LWHIP_OK)
                return stsc;
            dyn.stopIter = it;
            // hybrid PRD: the scatter launch has read JRest, the rates pass rebuilds it (a stopped column keeps its own)
            if (b->hybrid)
                HIP_TRY(launch_batch_zero_jrest(b->zr.dev.p, b->zrMax, nAct, c0->stream, stop, it));
            HIP_TRY(launch_lane_sweep(c0->dtargsPrd.p, c0->htargsPrd, dyn, c0->prob.formalSolver, true, wgPrd, c0->tileWaves,
                                      b->apPrd.dev.p, nAct, c0->stream, plain, ldsPrd));
            r0.stopIter = it;
            HIP_TRY(launch_reduce_sum(r0, c0->stream, b->rPrd.dev.p, nAct));
            a0.prdIter = it;
            if (c0->Natom > 0)
                HIP_TRY(launch_apply(a0, c0->stream, b->aPrd.dev.p, nAct));
            ca.lines = b->prdLines.p;
            ca.rec = b->prdRec.p + (size_t)((it - 1) % PRD_PIPE_DEPTH) * n * stride;
            ca.iter = it;
            HIP_TRY(launch_batch_prd_conv(ca, nAct, c0->stream));
        }
        // the group's records and the stop words: one copy, one wait
        HIP_TRY(hipMemcpyAsync(b->prdRecPinned.host, b->prdRec.p, (recDoubles + (n + 1) / 2) * sizeof(double), hipMemcpyDeviceToHost,
                               c0->stream));
        HIP_TRY(hipStreamSynchronize(c0->stream));
        const double* rec = b->prdRecPinned.as<double>();
        const int32_t* stopHost = (const int32_t*)(rec + recDoubles);
        for (int p = 0; p < nAct; ++p)
        {
            if (done[p])
                continue;
            for (int j = 0; j < nb; ++j)
            {
                const int it = iter + j + 1;
                out(b->act[p], it, rec + ((size_t)((it - 1) % PRD_PIPE_DEPTH) * n + p) * stride);
                count[p] = it;
                if (stopHost[p] == it) // (the sub-iteration that met the tolerance: the later ones did not run for this column)
                {
                    done[p] = 1;
                    ++nDone;
                    break;
                }
            }
        }
        iter += nb;
    }
    for (int p = 0; p < nAct; ++p)
        res->NprdSubIter[b->act[p]] = count[p];
    return LWHIP_OK;
}

int lwhip_batch_conv_records(lwhip_batch* b, double* records, int* strideOut)
{
    if (!b || b->ctxs.empty() || !records)
        return fail(LWHIP_ERR_INVALID, "batch_conv_records: null argument");
    const size_t stride = 2 + 2 * (size_t)std::max(b->se0.Natoms, 0);
    if (strideOut)
        *strideOut = (int)stride;
    const double* rec = b->recPinned.as<double>();
    for (const int32_t i : b->recCols)
        std::memcpy(records + i * stride, rec + i * stride, stride * sizeof(double));
    return LWHIP_OK;
}

int lwhip_batch_set_active(lwhip_batch* b, const int32_t* columns, int nActive)
{
    lwhip_context* c0 = nullptr;
    if (const int st = batch_enter(b, "null batch", c0); st != LWHIP_OK)
        return st;
    const int n = (int)b->ctxs.size();
    if (nActive < 0 || (nActive > 0 && !columns))
        return fail(LWHIP_ERR_INVALID, "batch_set_active: nActive < 0, or a count without a list");
    for (int p = 0; p < nActive; ++p)
        if (columns[p] < 0 || columns[p] >= n || (p > 0 && columns[p] <= columns[p - 1]))
            return fail(LWHIP_ERR_INVALID, "batch_set_active: entry " + std::to_string(p) + " (" + std::to_string(columns[p])
                                               + ") is out of range or not above the one before it");
    const bool all = nActive == 0 || !columns || nActive == n;
    std::vector<int32_t> act(all ? n : nActive);
    for (int p = 0; p < (int)act.size(); ++p)
        act[p] = all ? p : columns[p];
    if (act == b->act)
        return LWHIP_OK;
    b->act = act;
    b->allActive = all;
    b->aValid = false; // (the device copy of the apply blocks is that of another set)
    return batch_refresh_lists(b);
}

int lwhip_batch_active(lwhip_batch* b, int32_t* columns, int* nActive)
{
    if (!b || b->ctxs.empty() || !nActive)
        return fail(LWHIP_ERR_INVALID, "batch_active: null argument");
    *nActive = (int)b->act.size();
    if (columns)
        std::copy(b->act.begin(), b->act.end(), columns);
    return LWHIP_OK;
}

// Ng acceleration of every column: the shared driver (ng_configure ..., lwhip_api.hip) with the batch's n columns.  (0, 0, 0): off.
int lwhip_batch_ng_configure(lwhip_batch* b, int Norder, int Nperiod, int Ndelay)
{
    lwhip_context* c0 = nullptr;
    int st = batch_enter(b, "null batch", c0);
    if (st == LWHIP_OK)
        st = ng_configure(b->ng, b->ctxs, Norder, Nperiod, Ndelay, false);
    if (st == LWHIP_OK && b->ng.on && b->ng.Natoms != b->se0.Natoms) // (batch_conv_kernel reads the change records by se0's count)
    {
        (void)ng_off(b->ng, c0->stream);
        return fail(LWHIP_ERR_INVALID, "batch_ng_configure: the solved atoms are not those of the batch's solve");
    }
    return st;
}

int lwhip_batch_ng_accelerate(lwhip_batch* b, int32_t* accelerated, double* dPops, int32_t* dPopsMaxIdx)
{
    lwhip_context* c0 = nullptr;
    int st = batch_enter(b, "null batch", c0);
    if (st != LWHIP_OK)
        return st;
    if (!b->ng.on)
        return fail(LWHIP_ERR_INVALID, "lwhip_batch_ng_accelerate before lwhip_batch_ng_configure");
    const int Na = b->ng.Natoms;
    for (const int32_t i : b->act)
        *b->ctxs[i]->statusHost = 0;
    HIP_TRY(batch_ng_step(b));
    st = ng_fetch(b->ng, c0->stream);
    if (st == LWHIP_OK)
        st = batch_singular(b);
    if (st != LWHIP_OK)
        return st;
    for (const int32_t i : b->act) // (rows of inactive columns stay as the caller filled them)
    {
        if (accelerated)
            accelerated[i] = b->ng.accel_host()[i];
        ng_changes(b->ng, i, dPops ? dPops + (size_t)i * Na : nullptr, dPopsMaxIdx ? dPopsMaxIdx + (size_t)i * Na : nullptr);
    }
    return LWHIP_OK;
}

int lwhip_batch_ng_state(lwhip_batch* b, int32_t opts[3], int32_t* counts, int32_t* lastAccelerated)
{
    lwhip_context* c0 = nullptr;
    const int st = batch_enter(b, "null batch", c0);
    return st != LWHIP_OK ? st : ng_read_state(b->ng, (int)b->ctxs.size(), c0->stream, opts, counts, lastAccelerated);
}
}
