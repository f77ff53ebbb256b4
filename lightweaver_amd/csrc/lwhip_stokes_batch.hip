// lwhip_stokes_batch.hip -- full Stokes for a 1.5D column batch: lwhip_batch_compute_polarised_profiles and
// lwhip_batch_full_stokes_fs, the polarised profiles and formal_sol_full_stokes of every column in one set of launches.
//
// A chunk of (columns x wavelength range) runs as up to three launches on the batch's stream, each over ALL columns of the
// chunk, the column outermost in the work index:
//   stokes_batch_gather_kernel  one workgroup per block of 64 rays: chi[7] and eta[4] of every depth point
//                               (stokes_gather_point), stored as the rays' rows;
//   stokes_batch_march_kernel   one lane per ray, one wavefront per block of 64 rays (stokes_march_ray);
//   stokes_batch_j_kernel       (updateJ) one thread per (column, lambda) (stokes_j_lambda).
// Layout.  A column's rays of the chunk (its nla x Nr x nDir rays, in the single context's order) are cut into blocks of 64,
// the last one padded, so that every wavefront belongs to one column and reads its argument block with scalar loads.  A
// block's rows are [ST_ROWS][Ns][64]: at each depth point the 64 lanes read 64 consecutive doubles (the single context's
// [ray][ST_ROWS][Ns] puts 11 Ns doubles between neighbouring lanes).  The I / Q profiles of updateJ are [2][Ns][64] per
// block.  The device functions are the single context's (lwhip_stokes_dev.h), templated on that addressing only, so each
// column's results are the bits of lwhip_full_stokes_fs on its own context.
// Scratch.  The rows of a chunk are the batch's and capped at 1 GiB: they do not grow with the number of columns.  A chunk
// takes as many whole columns as fit (2 300 wavefronts at 82 depth points without updateJ, more than two per SIMD), or one
// column's wavelength range when a single column does not fit ("Full Stokes").
#include "lwhip_host.h"
#include "lwhip_device.h"

// As in lwhip_stokes.hip: no fused multiply-adds, so that the operations match the reference's one for one.
#pragma clang fp contract(off)

#include "lwhip_stokes_dev.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace lwhip
{
namespace
{
enum { SB_LANES = 64 };

// one chunk: columns [col0, col0 + ncol) x wavelengths [la0, la0 + nla)
struct StokesBatchArgs
{
    const StokesArgs* cols; // [n] the columns' argument blocks
    int32_t col0, ncol, la0, nla;
    int32_t nDir, dir0, blocksPerCol, Ns;
    int32_t Nr, updateJ;
    double* scratch; // [ncol * blocksPerCol][ST_ROWS][Ns][64]
    double* Isc;     // [ncol * blocksPerCol][2][Ns][64] (updateJ)
};

// (la, mu, d) of ray r of a column in the chunk: the single context's order
DEVINL void batch_ray(const StokesBatchArgs& b, int r, int& la, int& mu, int& d)
{
    d = b.dir0 + r % b.nDir;
    mu = (r / b.nDir) % b.Nr;
    la = b.la0 + r / (b.nDir * b.Nr);
}

// one workgroup of 256 threads per block of 64 rays: 64 lanes x 4 depth points at a time
__global__ void __launch_bounds__(256) stokes_batch_gather_kernel(const StokesBatchArgs b)
{
    const int blk = blockIdx.x;
    const int lane = threadIdx.x % SB_LANES;
    const StokesArgs a = b.cols[b.col0 + blk / b.blocksPerCol];
    const int r = (blk % b.blocksPerCol) * SB_LANES + lane;
    if (r >= b.nla * b.Nr * b.nDir)
        return;
    int la, mu, d;
    batch_ray(b, r, la, mu, d);
    const int Ns = b.Ns;
    double* base = b.scratch + (size_t)blk * ST_ROWS * Ns * SB_LANES + lane;
    for (int k = threadIdx.x / SB_LANES; k < Ns; k += blockDim.x / SB_LANES)
        stokes_gather_point(a, la, mu, d, k, LaneRow<double>{ base + (size_t)k * SB_LANES });
}

// one wavefront per block of 64 rays, a lane per ray.  One wavefront per SIMD: held to two (256 registers) the march spills
// 37 VGPRs to scratch memory ("Full Stokes")
__global__ void __launch_bounds__(64) stokes_batch_march_kernel(const StokesBatchArgs b)
{
    const int blk = blockIdx.x;
    const int lane = threadIdx.x;
    const StokesArgs a = b.cols[b.col0 + blk / b.blocksPerCol];
    const int r = (blk % b.blocksPerCol) * SB_LANES + lane;
    if (r >= b.nla * b.Nr * b.nDir)
        return;
    int la, mu, d;
    batch_ray(b, r, la, mu, d);
    const int Ns = b.Ns;
    const LaneRow<const double> row{ b.scratch + (size_t)blk * ST_ROWS * Ns * SB_LANES + lane };
    const LaneRow<double> out0{ b.updateJ ? b.Isc + (size_t)blk * 2 * Ns * SB_LANES + lane : nullptr };
    const LaneRow<double> out1{ b.updateJ ? out0.p + (size_t)Ns * SB_LANES : nullptr };
    stokes_march_ray(a, row, out0, out1, la, mu, d, b.nDir);
}

// J, J20 and dJ: one thread per wavelength of the chunk, blockIdx.y = the column in the chunk
__global__ void stokes_batch_j_kernel(const StokesBatchArgs b)
{
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    const int col = blockIdx.y;
    if (l >= b.nla)
        return;
    const StokesArgs a = b.cols[b.col0 + col];
    const int Ns = b.Ns;
    stokes_j_lambda(a, b.la0 + l, b.nDir, [&](int mu, int dd, int q, int k) {
        const int r = (l * b.Nr + mu) * b.nDir + dd;
        const size_t blk = (size_t)col * b.blocksPerCol + r / SB_LANES;
        return b.Isc[((blk * 2 + q) * Ns + k) * SB_LANES + r % SB_LANES];
    });
}
} // namespace

struct StokesBatch
{
    DevBuf<StokesArgs> args; // the columns' argument blocks, as argsHost
    std::vector<StokesArgs> argsHost;
    DevBuf<double> scratch, Isc; // one chunk's rows and I / Q profiles
    DevBuf<double> tail;         // [n][Nla] dJ of every column, then n int32 singular flags
    PinnedBlock tailPinned;
    DevBuf<PolLineArgs> polList; // every column's polarised lines, as polHost
    std::vector<PolLineArgs> polHost;
};

void stokes_batch_release(StokesBatch* s)
{
    if (s)
        s->tailPinned.release();
    delete s;
}

namespace
{
// the refusals of the batch entry points, before anything is launched: every column as check_stokes_ctx, with the polarised
// lines of column 0 (the same transitions, the same component counts)
int check_stokes_batch(lwhip_batch* b, const char* what)
{
    if (lwhip_device_count() <= 0)
        return fail(LWHIP_ERR_DEVICE, std::string(what) + ": no gfx950 device");
    if (!b || b->ctxs.empty())
        return fail(LWHIP_ERR_INVALID, std::string(what) + ": null batch");
    const StokesState& s0 = b->ctxs[0]->stokes;
    for (size_t i = 0; i < b->ctxs.size(); ++i)
    {
        lwhip_context* c = b->ctxs[i];
        const int chk = check_stokes_ctx(c, what, true);
        if (chk != LWHIP_OK)
            return fail(chk, std::string(lwhip_last_error()) + " (column " + std::to_string(i) + ")");
        const StokesState& s = c->stokes;
        bool same = s.lineTr == s0.lineTr;
        for (size_t q = 0; same && q < s.lines.size(); ++q)
            same = s.lines[q].Ncomp == s0.lines[q].Ncomp;
        if (!same)
            return fail(LWHIP_ERR_INVALID, std::string(what) + ": column " + std::to_string(i)
                                               + " has other polarised lines than column 0 (the same transitions and component "
                                                 "counts are required)");
    }
    return LWHIP_OK;
}
} // namespace
} // namespace lwhip

extern "C"
{
int lwhip_batch_compute_polarised_profiles(lwhip_batch* b)
{
    const char* what = "lwhip_batch_compute_polarised_profiles";
    int chk = check_stokes_batch(b, what);
    if (chk != LWHIP_OK)
        return chk;
    for (size_t i = 0; i < b->ctxs.size(); ++i)
        if (!b->ctxs[i]->stokes.argsHost.empty() && (!b->ctxs[i]->lineWave.p || !b->ctxs[i]->lineWlam.p))
            return fail(LWHIP_ERR_INVALID, std::string(what) + ": column " + std::to_string(i) + " has no line grids on the device");
    lwhip_context* c0 = b->ctxs[0];
    HIP_TRY(hipSetDevice(c0->device));
    // As lwhip_compute_polarised_profiles: device-made profiles whose inputs were uploaded again are regenerated FIRST, or the
    // next sweep or Stokes call would overwrite the polarised lines' phi with the plain Voigt profile.
    {
        const int stp = batch_ensure_profiles(b);
        if (stp != LWHIP_OK)
            return stp;
    }
    if (c0->stokes.argsHost.empty()) // (every column has column 0's polarised lines)
        return LWHIP_OK;
    if (!b->stokes)
        b->stokes = new StokesBatch();
    StokesBatch& sb = *b->stokes;
    std::vector<PolLineArgs> list;
    for (lwhip_context* c : b->ctxs)
        list.insert(list.end(), c->stokes.argsHost.begin(), c->stokes.argsHost.end());
    // (uploaded again only when a column's blocks changed; the host copy is the source of the queued copy)
    if (sb.polHost.size() != list.size() || std::memcmp(sb.polHost.data(), list.data(), list.size() * sizeof(PolLineArgs)) != 0)
    {
        HIP_TRY(hipStreamSynchronize(c0->stream)); // nothing may still read the blocks about to be replaced
        sb.polHost.swap(list);
        if (sb.polList.n < sb.polHost.size())
            HIP_TRY(sb.polList.alloc(c0->mem, sb.polHost.size(), false));
        HIP_TRY(hipMemcpyAsync(sb.polList.p, sb.polHost.data(), sb.polHost.size() * sizeof(PolLineArgs), hipMemcpyHostToDevice,
                               c0->stream));
    }
    const std::vector<PolLineArgs>& pl = sb.polHost;
    // the launch geometry allows 65 535 entries per grid dimension (as batch_compute_profiles)
    for (size_t off = 0; off < pl.size(); off += 32768)
        HIP_TRY(launch_polarised_profiles(sb.polList.p + off, pl.data() + off, (int)std::min<size_t>(32768, pl.size() - off),
                                          c0->stream));
    for (lwhip_context* c : b->ctxs)
    {
        c->stokes.polOnDevice = true;
        c->phiSym = c->phiSym && c->vlosZero;
    }
    return batch_retile(b, b->ctxs);
}

int lwhip_batch_full_stokes_fs(lwhip_batch* b, int updateJ, int upOnly, lwhip_iter_result* results)
{
    const char* what = "lwhip_batch_full_stokes_fs";
    int chk = check_stokes_batch(b, what);
    if (chk != LWHIP_OK)
        return chk;
    const int n = (int)b->ctxs.size();
    for (int i = 0; i < n; ++i)
        if (updateJ && b->ctxs[i]->JhostReg)
            return fail(LWHIP_ERR_UNSUPPORTED, std::string(what) + ": updateJ with a mapped host J in column " + std::to_string(i)
                                                   + " (lwhip_map_host_J(ctx, 0) first)");
    lwhip_context* c0 = b->ctxs[0];
    if (c0->Ns < 3)
        return fail(LWHIP_ERR_INVALID, std::string(what) + ": needs at least 3 depth points");
    HIP_TRY(hipSetDevice(c0->device));
    {
        const int stp = batch_ensure_profiles(b);
        if (stp != LWHIP_OK)
            return stp;
    }
    if (!b->stokes)
        b->stokes = new StokesBatch();
    StokesBatch& sb = *b->stokes;
    const int Ns = c0->Ns, Nr = c0->Nrays, Nla = c0->Nla;
    const int nDir = upOnly ? 1 : 2;
    const size_t tailN = (size_t)n * Nla + (n + 1) / 2; // the dJ rows, then the flags
    if (sb.tail.n < tailN)
    {
        HIP_TRY(hipStreamSynchronize(c0->stream));
        HIP_TRY(sb.tail.alloc(c0->mem, tailN));
        HIP_TRY(sb.tailPinned.reserve(c0->device, tailN * sizeof(double), c0->stream));
    }
    int32_t* flags = (int32_t*)(sb.tail.p + (size_t)n * Nla);
    // the columns' argument blocks (uploaded again only when one of them changed)
    std::vector<StokesArgs> args(n);
    for (int i = 0; i < n; ++i)
    {
        lwhip_context* c = b->ctxs[i];
        StokesState& s = c->stokes;
        StokesArgs a{};
        a.Ns = Ns;
        a.Nr = Nr;
        a.la0 = 0;
        a.nla = Nla;
        a.Nla = Nla;
        a.nDir = nDir;
        a.dir0 = upOnly ? 1 : 0;
        a.updateJ = updateJ ? 1 : 0;
        a.hasJ20 = s.desc.J20 ? 1 : 0;
        a.lowerType = c->prob.zLowerBc.type;
        a.upperType = c->prob.zUpperBc.type;
        a.lowerNmu = c->prob.zLowerBc.Nmu;
        a.upperNmu = c->prob.zUpperBc.Nmu;
        a.height = c->height.p;
        a.temperature = c->temperature.p;
        a.muz = c->muz.p;
        a.wmu = c->wmu.p;
        a.wavelength = c->wavelength.p;
        a.bgChi = c->bgChi.p;
        a.bgEta = c->bgEta.p;
        a.bgSca = c->bgSca.p;
        a.J = c->J.p;
        a.J20 = s.J20.p;
        a.n = c->n.p;
        a.ratio = c->ratio.p;
        a.par = c->par.p;
        a.phi = c->phi.p;
        a.rho = c->rho.p;
        a.pol = s.pol.p;
        a.lowerBc = c->lowerBcData.p;
        a.upperBc = c->upperBcData.p;
        a.lowerIdx = c->lowerIdx.p;
        a.upperIdx = c->upperIdx.p;
        a.laOff = s.laOff.p;
        a.laTr = s.laTr.p;
        a.laPol = s.laPol.p;
        a.tr = s.tr.p;
        a.scratch = nullptr;
        a.Isc = nullptr;
        a.I = c->I.p;
        a.Quv = s.Quv.p;
        a.dJ = sb.tail.p + (size_t)i * Nla;
        a.singular = flags + i;
        args[i] = a;
    }
    if (sb.argsHost.size() != args.size() || std::memcmp(sb.argsHost.data(), args.data(), args.size() * sizeof(StokesArgs)) != 0)
    {
        HIP_TRY(hipStreamSynchronize(c0->stream)); // (nothing queued may still read the blocks about to be replaced)
        sb.argsHost = args;
        if (sb.args.n < (size_t)n)
            HIP_TRY(sb.args.alloc(c0->mem, (size_t)n, false));
        HIP_TRY(hipMemcpyAsync(sb.args.p, sb.argsHost.data(), (size_t)n * sizeof(StokesArgs), hipMemcpyHostToDevice, c0->stream));
    }
    // chunks of (columns x wavelength range) whose rows stay within the cap; LWHIP_STOKES_BATCH_RAYS (LWHIP_DEBUG) caps the
    // rays of a chunk instead, to make small chunks for the tests
    const size_t rowsPerRay = (size_t)ST_ROWS + (updateJ ? 2 : 0);
    size_t maxBlocks = std::max<size_t>(1, ((size_t)1 << 30) / (rowsPerRay * Ns * sizeof(double) * SB_LANES));
    const int dbgRays = dbg_env_int("LWHIP_STOKES_BATCH_RAYS", 0);
    if (dbgRays > 0)
        maxBlocks = std::max<size_t>(1, (size_t)dbgRays / SB_LANES);
    const size_t raysPerLa = (size_t)Nr * nDir;
    const size_t blocksPerColFull = (Nla * raysPerLa + SB_LANES - 1) / SB_LANES;
    int colsChunk = 1, nlaChunk = Nla;
    if (blocksPerColFull <= maxBlocks)
        colsChunk = (int)std::min<size_t>({ (size_t)n, maxBlocks / blocksPerColFull, 65535 });
    else
        nlaChunk = (int)std::max<size_t>(1, maxBlocks * SB_LANES / raysPerLa);
    const size_t blocksMax = (size_t)colsChunk * ((nlaChunk * raysPerLa + SB_LANES - 1) / SB_LANES);
    if (sb.scratch.n < blocksMax * ST_ROWS * Ns * SB_LANES || (updateJ && sb.Isc.n < blocksMax * 2 * Ns * SB_LANES))
    {
        HIP_TRY(hipStreamSynchronize(c0->stream));
        if (sb.scratch.n < blocksMax * ST_ROWS * Ns * SB_LANES)
            HIP_TRY(sb.scratch.alloc(c0->mem, blocksMax * ST_ROWS * Ns * SB_LANES, false));
        if (updateJ && sb.Isc.n < blocksMax * 2 * Ns * SB_LANES)
            HIP_TRY(sb.Isc.alloc(c0->mem, blocksMax * 2 * Ns * SB_LANES, false));
    }
    HIP_TRY(hipMemsetAsync(flags, 0, (size_t)n * sizeof(int32_t), c0->stream));
    StokesBatchArgs ba{};
    ba.cols = sb.args.p;
    ba.nDir = nDir;
    ba.dir0 = upOnly ? 1 : 0;
    ba.Ns = Ns;
    ba.Nr = Nr;
    ba.updateJ = updateJ ? 1 : 0;
    ba.scratch = sb.scratch.p;
    ba.Isc = sb.Isc.p;
    for (int col0 = 0; col0 < n; col0 += colsChunk)
        for (int la0 = 0; la0 < Nla; la0 += nlaChunk)
        {
            ba.col0 = col0;
            ba.ncol = std::min(colsChunk, n - col0);
            ba.la0 = la0;
            ba.nla = std::min(nlaChunk, Nla - la0);
            ba.blocksPerCol = (int)((ba.nla * raysPerLa + SB_LANES - 1) / SB_LANES);
            const unsigned nBlk = (unsigned)ba.ncol * ba.blocksPerCol;
            LWHIP_LAUNCH(stokes_batch_gather_kernel, dim3(nBlk), dim3(256), 0, c0->stream, ba);
            LWHIP_LAUNCH(stokes_batch_march_kernel, dim3(nBlk), dim3(SB_LANES), 0, c0->stream, ba);
            if (updateJ)
                LWHIP_LAUNCH(stokes_batch_j_kernel, dim3((ba.nla + 63) / 64, ba.ncol), dim3(64), 0, c0->stream, ba);
            HIP_TRY(hipGetLastError());
        }
    if (updateJ)
        for (lwhip_context* c : b->ctxs)
            c->fpJValid = false;
    // one copy back: the dJ rows (updateJ) and the flags, then one wait
    const size_t off = updateJ ? 0 : (size_t)n * Nla;
    HIP_TRY(hipMemcpyAsync(sb.tailPinned.as<double>() + off, sb.tail.p + off, (tailN - off) * sizeof(double), hipMemcpyDeviceToHost,
                           c0->stream));
    HIP_TRY(hipStreamSynchronize(c0->stream));
    const double* dJ = sb.tailPinned.as<double>();
    const int32_t* sing = (const int32_t*)(dJ + (size_t)n * Nla);
    for (int i = 0; i < n && results; ++i)
    {
        results[i].updatedJ = updateJ ? 1 : 0;
        results[i].dJMax = 0.0;
        results[i].dJMaxIdx = 0;
        if (!updateJ)
            continue;
        // formal_sol_full_stokes_impl's serial loop: dJMax = max_idx(dJ, dJMax, maxIdx, la) (FormalStokes.cpp:708-714)
        double dJMax = 0.0;
        int maxIdx = 0;
        for (int la = 0; la < Nla; ++la)
        {
            const double v = dJ[(size_t)i * Nla + la];
            if (v < dJMax)
                maxIdx = la;
            else
                dJMax = v;
        }
        results[i].dJMax = dJMax;
        results[i].dJMaxIdx = maxIdx;
    }
    for (int i = 0; i < n; ++i)
        if (sing[i])
            return fail(LWHIP_ERR_SINGULAR, std::string(what) + ": Singular Matrix in the 4 x 4 DELO-Bezier3 step of column "
                                                + std::to_string(i));
    return LWHIP_OK;
}
}
