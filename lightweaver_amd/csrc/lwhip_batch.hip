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
    lwhip_context* c0 = b->ctxs[0];
    if (!list.empty())
    {
        if (b->voigtList.n < list.size())
        {
            HIP_TRY(hipStreamSynchronize(c0->stream)); // nothing may still read the buffer about to be replaced
            HIP_TRY(b->voigtList.alloc(c0->mem, list.size()));
        }
        HIP_TRY(hipMemcpyAsync(b->voigtList.p, list.data(), list.size() * sizeof(VoigtLineArgs), hipMemcpyHostToDevice, c0->stream));
        // the launch geometry allows 65 535 entries per grid dimension
        for (size_t off = 0; off < list.size(); off += 32768)
        {
            const int cnt = (int)std::min<size_t>(32768, list.size() - off);
            HIP_TRY(launch_voigt_lines(b->voigtList.p + off, list.data() + off, cnt, c0->stream));
        }
    }
    // ... and their tile-blocked copies, one grid slice per column
    for (lwhip_context* c : todo)
    {
        c->deviceProfiles = true;
        c->profilesStale = false;
        c->phiSym = c->vlosZero;
        c->phiIso = c->vlosZero;
    }
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

// the compacted argument lists of a proper subset of the columns (lwhip_batch_set_active): position p is column act[p].  The
// buffers are made once, for n columns; the copies are ordered on the batch's stream behind the launches that read the last set.
// (The apply blocks follow in the next lwhip_batch_formal_sol_gamma_matrices: aValid is off.)
template <class T> static hipError_t upload_compact(lwhip_batch* b, DevBuf<T>& dev, std::vector<T>& host, const std::vector<T>& full)
{
    lwhip_context* c0 = b->ctxs[0];
    if (!dev.p)
    {
        const hipError_t e = dev.alloc(c0->mem, full.size(), false);
        if (e != hipSuccess)
            return e;
    }
    host.resize(b->act.size());
    for (size_t p = 0; p < b->act.size(); ++p)
        host[p] = full[b->act[p]];
    return hipMemcpyAsync(dev.p, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice, c0->stream);
}
static int batch_upload_active(lwhip_batch* b)
{
    lwhip_context* c0 = b->ctxs[0];
    HIP_TRY(upload_compact(b, b->apAct, b->apActHost, b->apHost));
    HIP_TRY(upload_compact(b, b->rAct, b->rActHost, b->rHost));
    HIP_TRY(upload_compact(b, b->seAct, b->seActHost, b->seHost));
    if (b->change.p)
        HIP_TRY(upload_compact(b, b->seRepAct, b->seRepActHost, b->seRepHost));
    if (!b->aAct.p)
        HIP_TRY(b->aAct.alloc(c0->mem, b->ctxs.size()));
    b->aActHost.resize(b->act.size());
    if (!b->colsAct.p)
        HIP_TRY(b->colsAct.alloc(c0->mem, b->ctxs.size(), false));
    HIP_TRY(hipMemcpyAsync(b->colsAct.p, b->act.data(), b->act.size() * sizeof(int32_t), hipMemcpyHostToDevice, c0->stream));
    HIP_TRY(hipStreamSynchronize(c0->stream)); // (the host lists may change with the next set; a retirement is rare)
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
    return ng_step(b->ng, b->allActive ? nullptr : b->colsAct.p, (int)b->act.size(), b->ctxs[0]->stream);
}

namespace lwhip
{
int batch_retile(lwhip_batch* b, const std::vector<lwhip_context*>& cols)
{
    lwhip_context* c0 = b->ctxs[0];
    std::vector<RetileArgs> rl;
    for (lwhip_context* c : cols)
    {
        RetileArgs r;
        if (retile_args(c, r))
            rl.push_back(r);
    }
    if (!rl.empty())
    {
        if (b->retileList.n < rl.size())
        {
            HIP_TRY(hipStreamSynchronize(c0->stream));
            HIP_TRY(b->retileList.alloc(c0->mem, rl.size()));
        }
        HIP_TRY(hipMemcpyAsync(b->retileList.p, rl.data(), rl.size() * sizeof(RetileArgs), hipMemcpyHostToDevice, c0->stream));
        for (size_t off = 0; off < rl.size(); off += 32768)
            HIP_TRY(launch_retile_list(b->retileList.p + off, rl.data() + off, (int)std::min<size_t>(32768, rl.size() - off),
                                       c0->stream));
    }
    return LWHIP_OK;
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
        if (c->device != c0->device || c->Ns != c0->Ns || c->Nla != c0->Nla
            || c->Nrays != c0->Nrays || c->Ntrans != c0->Ntrans || c->Natom != c0->Natom || c->nTiles != c0->nTiles
            || c->nTileChunks != c0->nTileChunks || c->nPostChunks != c0->nPostChunks || c->tileCap != c0->tileCap
            || c->tileFuse != c0->tileFuse || c->tileWaves != c0->tileWaves || c->maxCTTile != c0->maxCTTile
            || c->laneSweep != c0->laneSweep
            || c->maxL != c0->maxL || c->maxC != c0->maxC
            || c->NlevTot != c0->NlevTot || c->prob.formalSolver != c0->prob.formalSolver)
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
    std::vector<const TileArgs*> ap(n);
    std::vector<ReduceArgs> rl(n);
    HIP_TRY(b->tail.alloc(c0->mem, (size_t)2 * n));
    for (int i = 0; i < n; ++i)
    {
        ap[i] = ctxs[i]->dtargs.p;
        rl[i] = make_reduce_args(ctxs[i]);
        rl[i].batchTail = b->tail.p + 2 * (size_t)i;
        rl[i].zeroParts = 1;
        // the columns' stage-1 buffers start clean (the sweep adds into them, stage 2 zeroes what it has summed)
        if (!ctxs[i]->red8Clean)
            HIP_TRY(hipMemsetAsync(ctxs[i]->red8.p, 0, ctxs[i]->red8.n * sizeof(double), c0->stream));
        ctxs[i]->red8Clean = true;
    }
    HIP_TRY(b->apList.upload(c0->mem, ap));
    HIP_TRY(b->rList.upload(c0->mem, rl));
    b->apHost = ap;
    b->rHost = rl;
    b->act.resize(n);
    for (int i = 0; i < n; ++i)
        b->act[i] = i;
    HIP_TRY(b->aList.alloc(c0->mem, (size_t)n));
    b->aHost.resize(n);
    {
        std::vector<StatEqArgs> sl(n);
        for (int i = 0; i < n; ++i)
        {
            lwhip_context* c = ctxs[i];
            std::vector<NrAtom> atoms;
            int maxNl = 0;
            for (int ia = 0; ia < c->Natom; ++ia)
            {
                const lwhip_atom& a = c->atoms[ia];
                if (a.detailed)
                    continue;
                NrAtom at{};
                at.atom = ia;
                at.Nlevel = a.Nlevel;
                at.levelOff = c->levelOff[ia];
                at.gammaOff = c->gammaOff[ia];
                atoms.push_back(at);
                maxNl = std::max(maxNl, a.Nlevel);
            }
            if (!atoms.empty())
            {
                HIP_TRY(c->statEqAtoms.upload(c->mem, atoms));
                c->statEqKey = -1;
            }
            StatEqArgs sa{};
            sa.Ns = c->Ns;
            sa.k0 = 0;
            sa.k1 = c->Ns;
            sa.Natoms = (int32_t)atoms.size();
            sa.atoms = c->statEqAtoms.p;
            sa.n = c->n.p;
            sa.nTotal = c->nTotal.p;
            sa.Gamma = c->Gamma.p;
            sa.status = c->statusDev;
            sa.change = nullptr;
            sl[i] = sa;
            if (i == 0)
            {
                b->se0 = sa;
                b->seMaxNl = maxNl;
            }
            else if (sa.Natoms != b->se0.Natoms || maxNl != b->seMaxNl)
                return fail(LWHIP_ERR_INVALID, "batch_create: the columns must share their active atoms");
        }
        HIP_TRY(b->seList.upload(c0->mem, sl));
        b->seHost = sl;
    }
    HIP_TRY(b->tailPinned.reserve(c0->device, (size_t)2 * n * sizeof(double), c0->stream));
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
    if (!b || b->ctxs.empty())
        return fail(LWHIP_ERR_INVALID, "null batch");
    const int n = (int)b->ctxs.size();
    lwhip_context* c0 = b->ctxs[0];
    HIP_TRY(hipSetDevice(c0->device));
    {
        // columns whose atmosphere was updated: their phi / wphi first, all their lines in one launch pair
        const int stp = batch_ensure_profiles(b);
        if (stp != LWHIP_OK)
            return stp;
    }
    // the columns this call launches: all of them, or the compacted lists of the active set (lwhip_batch_set_active)
    const int nAct = (int)b->act.size();
    const TileArgs* const* apL = b->allActive ? b->apList.p : b->apAct.p;
    const ReduceArgs* rL = b->allActive ? b->rList.p : b->rAct.p;
    const ApplyArgs* aL = b->allActive ? b->aList.p : b->aAct.p;
    // Gamma <- crsw * C of every column is fused into its slice of the apply launch
    for (const int32_t i : b->act)
    {
        lwhip_context* c = b->ctxs[i];
        if (c->partialPending || c->prdPending)
            return fail(LWHIP_ERR_INVALID, "batch iteration while a split iteration of a column is pending");
        c->prefillCrsw = crsw;
        c->dJPrdClean = false; // (the batch sweep writes every wavelength's dJ)
        c->prefillPending = c->gammaTot > 0 && c->Cmat.p != nullptr;
        b->aHost[i] = make_apply_args(c);
        c->prefillPending = false;
    }
    if (!b->aValid || b->aCrsw != crsw)
    {
        if (b->allActive)
            HIP_TRY(hipMemcpyAsync(b->aList.p, b->aHost.data(), (size_t)n * sizeof(ApplyArgs), hipMemcpyHostToDevice, c0->stream));
        else
        {
            for (int p = 0; p < nAct; ++p)
                b->aActHost[p] = b->aHost[b->act[p]];
            HIP_TRY(hipMemcpyAsync(b->aAct.p, b->aActHost.data(), (size_t)nAct * sizeof(ApplyArgs), hipMemcpyHostToDevice, c0->stream));
        }
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
        HIP_TRY(launch_lane_sweep(c0->dtargs.p, c0->htargs, dyn, c0->prob.formalSolver, true, c0->nTileChunks, c0->tileWaves, apL, nAct,
                                  c0->stream, batch_plain_ok(b, dyn)));
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
        HIP_TRY(launch_reduce_sum(r0, c0->stream, rL, nAct));
    }
    if (c0->Natom > 0)
        HIP_TRY(launch_apply(b->aHost[b->act[0]], c0->stream, aL, nAct));
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
    if (!b || b->ctxs.empty())
        return fail(LWHIP_ERR_INVALID, "null batch");
    HIP_TRY(hipSetDevice(b->ctxs[0]->device));
    return batch_compute_profiles(b, true);
}

int lwhip_batch_sweep_instance(lwhip_batch* b, int32_t out[4])
{
    if (!b || b->ctxs.empty() || !out)
        return fail(LWHIP_ERR_INVALID, "batch_sweep_instance: null argument");
    // (what lwhip_batch_formal_sol_gamma_matrices passes its one sweep launch; a batch has no PRD rates pass)
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

int lwhip_batch_stat_equil(lwhip_batch* b)
{
    if (!b || b->ctxs.empty())
        return fail(LWHIP_ERR_INVALID, "null batch");
    lwhip_context* c0 = b->ctxs[0];
    HIP_TRY(hipSetDevice(c0->device));
    if (b->se0.Natoms <= 0)
        return LWHIP_OK;
    for (const int32_t i : b->act)
    {
        lwhip_context* c = b->ctxs[i];
        const int stp = flush_prefill(c);
        if (stp != LWHIP_OK)
            return stp;
        *c->statusHost = 0;
    }
    HIP_TRY(launch_stat_eq(b->se0, b->seMaxNl, c0->stream, b->allActive ? b->seList.p : b->seAct.p, (int)b->act.size()));
    if (b->ng.on)
        HIP_TRY(batch_ng_step(b));
    HIP_TRY(hipStreamSynchronize(c0->stream));
    return batch_singular(b);
}

int lwhip_batch_stat_equil_report(lwhip_batch* b, double* dPops, int32_t* dPopsMaxIdx)
{
    if (!b || b->ctxs.empty() || !dPops)
        return fail(LWHIP_ERR_INVALID, "batch_stat_equil_report: null argument");
    lwhip_context* c0 = b->ctxs[0];
    HIP_TRY(hipSetDevice(c0->device));
    const int Na = b->se0.Natoms;
    if (Na <= 0)
        return LWHIP_OK;
    const int n = (int)b->ctxs.size(), nAct = (int)b->act.size();
    const size_t stride = 2 + 2 * (size_t)Na;
    if (!b->rec.p)
    {
        // the records the columns' changes become
        HIP_TRY(b->rec.alloc(c0->mem, (size_t)n * stride));
        HIP_TRY(b->recPinned.reserve(c0->device, (size_t)n * stride * sizeof(double), c0->stream));
    }
    if (!b->ng.on && !b->change.p)
    {
        // the change records of all columns and a second list of solve arguments that aims at them
        b->seBlocks = stat_eq_blocks(c0->Ns, b->seMaxNl);
        HIP_TRY(b->change.alloc(c0->mem, (size_t)n * Na * b->seBlocks * 2));
        b->seRepHost = b->seHost;
        for (int i = 0; i < n; ++i)
            b->seRepHost[i].change = b->change.p + (size_t)i * Na * b->seBlocks * 2;
        HIP_TRY(b->seRepList.upload(c0->mem, b->seRepHost));
        if (!b->allActive)
        {
            const int stu = batch_upload_active(b);
            if (stu != LWHIP_OK)
                return stu;
        }
    }
    for (const int32_t i : b->act)
    {
        lwhip_context* c = b->ctxs[i];
        const int stp = flush_prefill(c);
        if (stp != LWHIP_OK)
            return stp;
        *c->statusHost = 0;
    }
    BatchConvArgs ca{};
    ca.tail = b->tail.p;
    ca.rec = b->rec.p;
    ca.cols = b->allActive ? nullptr : b->colsAct.p;
    ca.Natoms = Na;
    if (b->ng.on)
    {
        // the plain solve, then the Ng step: the reported change is Ng's max_change, taken after any extrapolation
        // (rel_diff_ng_accelerate, Source/LwMiddleLayer.pyx:3318-3346) -- one (value, index) pair per column and atom
        HIP_TRY(launch_stat_eq(b->se0, b->seMaxNl, c0->stream, b->allActive ? b->seList.p : b->seAct.p, nAct));
        HIP_TRY(batch_ng_step(b));
        ca.change = b->ng.out.p;
        ca.nBlocks = 1;
    }
    else
    {
        HIP_TRY(launch_stat_eq(b->se0, b->seMaxNl, c0->stream, b->allActive ? b->seRepList.p : b->seRepAct.p, nAct));
        ca.change = b->change.p;
        ca.nBlocks = b->seBlocks;
    }
    HIP_TRY(launch_batch_conv(ca, nAct, c0->stream));
    HIP_TRY(hipMemcpyAsync(b->recPinned.host, b->rec.p, (size_t)n * stride * sizeof(double), hipMemcpyDeviceToHost, c0->stream));
    HIP_TRY(hipStreamSynchronize(c0->stream));
    b->recCols = b->act;
    const int st = batch_singular(b);
    if (st != LWHIP_OK)
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
    if (!b || b->ctxs.empty())
        return fail(LWHIP_ERR_INVALID, "null batch");
    const int n = (int)b->ctxs.size();
    if (nActive < 0 || (nActive > 0 && !columns))
        return fail(LWHIP_ERR_INVALID, "batch_set_active: nActive < 0, or a count without a list");
    for (int p = 0; p < nActive; ++p)
        if (columns[p] < 0 || columns[p] >= n || (p > 0 && columns[p] <= columns[p - 1]))
            return fail(LWHIP_ERR_INVALID, "batch_set_active: entry " + std::to_string(p) + " (" + std::to_string(columns[p])
                                               + ") is out of range or not above the one before it");
    lwhip_context* c0 = b->ctxs[0];
    HIP_TRY(hipSetDevice(c0->device));
    const bool all = nActive == 0 || !columns || nActive == n;
    std::vector<int32_t> act(all ? n : nActive);
    for (int p = 0; p < (int)act.size(); ++p)
        act[p] = all ? p : columns[p];
    if (act == b->act)
        return LWHIP_OK;
    b->act = act;
    b->allActive = all;
    b->aValid = false; // (the device copy of the apply blocks is that of another set)
    return all ? LWHIP_OK : batch_upload_active(b);
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
    if (!b || b->ctxs.empty())
        return fail(LWHIP_ERR_INVALID, "null batch");
    lwhip_context* c0 = b->ctxs[0];
    HIP_TRY(hipSetDevice(c0->device));
    const int st = ng_configure(b->ng, b->ctxs, Norder, Nperiod, Ndelay, false);
    if (st == LWHIP_OK && b->ng.on && b->ng.Natoms != b->se0.Natoms) // (batch_conv_kernel reads the change records by se0's count)
    {
        (void)ng_off(b->ng, c0->stream);
        return fail(LWHIP_ERR_INVALID, "batch_ng_configure: the solved atoms are not those of the batch's solve");
    }
    return st;
}

int lwhip_batch_ng_accelerate(lwhip_batch* b, int32_t* accelerated, double* dPops, int32_t* dPopsMaxIdx)
{
    if (!b || b->ctxs.empty())
        return fail(LWHIP_ERR_INVALID, "null batch");
    if (!b->ng.on)
        return fail(LWHIP_ERR_INVALID, "lwhip_batch_ng_accelerate before lwhip_batch_ng_configure");
    lwhip_context* c0 = b->ctxs[0];
    HIP_TRY(hipSetDevice(c0->device));
    const int Na = b->ng.Natoms;
    for (const int32_t i : b->act)
        *b->ctxs[i]->statusHost = 0;
    HIP_TRY(batch_ng_step(b));
    int st = ng_fetch(b->ng, c0->stream);
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
    if (!b || b->ctxs.empty())
        return fail(LWHIP_ERR_INVALID, "null batch");
    HIP_TRY(hipSetDevice(b->ctxs[0]->device));
    return ng_read_state(b->ng, (int)b->ctxs.size(), b->ctxs[0]->stream, opts, counts, lastAccelerated);
}
}
