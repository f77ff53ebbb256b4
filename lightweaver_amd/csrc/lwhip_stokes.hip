// lwhip_stokes.hip -- the full-Stokes formal solution for Zeeman-polarised lines (1D plane-parallel): formal_sol_full_stokes
// (Source/FormalStokes.cpp:166-723) and the entry points of include/lwhip.h that drive it and the polarised profiles
// (whose kernels live with the other Voigt kernels in lwhip_voigt.hip).
//
// Layout.  A wavelength chunk runs as up to three launches on the context's stream:
//   stokes_gather_kernel  one thread per (lambda, mu, direction, depth): chi[7] and eta[4] summed over the transitions
//                         active at lambda (stokes_fs_core :496-602), stored as the ray's rows chi[0..6], S[0..3];
//   stokes_march_kernel   one thread per (lambda, mu, direction): the DELO-Bezier3 march of piecewise_stokes_bezier3_1d_impl
//                         (:166-340) down the ray with a 4 x 4 Crout LU per depth point (lwhip_lu.h), or the scalar
//                         piecewise_bezier3_1d (FormalScalar.cpp:209-325) where the wavelength is not polarised;
//   stokes_j_kernel       (updateJ) one thread per lambda: J, J20 and dJ, the rays added in the reference's order.
// The march is serial in depth, so a ray is one lane.  10 240 x 5 up-going rays are 800 wavefronts, fewer than the chip's
// 1 024 SIMDs: the march is latency-bound whatever its register count, and one lane per ray needs no exchange between
// lanes.  K is carried as its six independent entries (stokes_K :119-142) and expanded where a step uses it; no scratch
// memory ("Full Stokes").  The device functions the kernels call are shared with the column-batch kernels
// (lwhip_stokes_dev.h, lwhip_stokes_batch.hip).
#include "lwhip_host.h"
#include "lwhip_device.h"

// As in lwhip_pops.hip: no fused multiply-adds, so that the operations match the reference's one for one.
#pragma clang fp contract(off)

#include "lwhip_stokes_dev.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace lwhip
{
namespace
{
__global__ void stokes_gather_kernel(const StokesArgs a)
{
    const size_t nRay = (size_t)a.nla * a.Nr * a.nDir;
    const size_t total = nRay * a.Ns;
    for (size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x)
    {
        const int Ns = a.Ns;
        const int k = (int)(idx % Ns);
        const size_t ray = idx / Ns;
        const int d = a.dir0 + (int)(ray % a.nDir);
        const int mu = (int)((ray / a.nDir) % a.Nr);
        const int la = a.la0 + (int)(ray / ((size_t)a.nDir * a.Nr));
        stokes_gather_point(a, la, mu, d, k, a.scratch + ray * ST_ROWS * Ns + k);
    }
}

__global__ void __launch_bounds__(64) stokes_march_kernel(const StokesArgs a)
{
    const size_t nRay = (size_t)a.nla * a.Nr * a.nDir;
    const size_t ray = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (ray >= nRay)
        return;
    const int Ns = a.Ns;
    const int d = a.dir0 + (int)(ray % a.nDir);
    const int mu = (int)((ray / a.nDir) % a.Nr);
    const int la = a.la0 + (int)(ray / ((size_t)a.nDir * a.Nr));
    const double* row = a.scratch + ray * ST_ROWS * Ns;
    double* out0 = a.updateJ ? a.Isc + ray * 2 * Ns : nullptr;
    double* out1 = a.updateJ ? out0 + Ns : nullptr;
    stokes_march_ray(a, row, out0, out1, la, mu, d, a.nDir);
}

// J, J20 and dJ (stokes_j_lambda), one thread per wavelength
__global__ void stokes_j_kernel(const StokesArgs a)
{
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= a.nla)
        return;
    const int Ns = a.Ns;
    stokes_j_lambda(a, a.la0 + l, a.nDir, [&](int mu, int dd, int q, int k) {
        return a.Isc[(((size_t)l * a.Nr + mu) * a.nDir + dd) * 2 * Ns + (size_t)q * Ns + k];
    });
}
} // namespace

int check_stokes_ctx(lwhip_context* c, const char* what, bool needStokes)
{
    if (lwhip_device_count() <= 0)
        return fail(LWHIP_ERR_DEVICE, std::string(what) + ": no gfx950 device");
    if (!c)
        return fail(LWHIP_ERR_INVALID, std::string(what) + ": null context");
    if (c->is2d)
        return fail(LWHIP_ERR_UNSUPPORTED, std::string(what) + ": full Stokes is 1D plane-parallel only (as in the reference, "
                                                               "Source/FormalStokes.cpp:606-623)");
    if (c->laStart != 0 || c->laEnd != c->prob.Nlambda || c->worldSize > 1)
        return fail(LWHIP_ERR_UNSUPPORTED, std::string(what) + ": not on a wavelength shard (the context must hold the whole grid)");
    if (c->hprd)
        return fail(LWHIP_ERR_UNSUPPORTED, std::string(what) + ": not with hybrid PRD tables");
    if (needStokes && !c->stokes.on)
        return fail(LWHIP_ERR_INVALID, std::string(what) + ": no Stokes data (lwhip_set_stokes)");
    return LWHIP_OK;
}

int stokes_transfer(lwhip_context* c, bool up)
{
    StokesState& s = c->stokes;
    if (!s.on)
        return LWHIP_OK;
    HIP_TRY(hipSetDevice(c->device));
    const size_t Ns = c->Ns, Nr = c->Nrays, Nla = c->Nla;
    const hipMemcpyKind kind = up ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost;
    auto copy = [&](double* dev, double* host, size_t n) {
        return up ? hipMemcpyAsync(dev, host, n * sizeof(double), kind, c->stream)
                  : hipMemcpyAsync(host, dev, n * sizeof(double), kind, c->stream);
    };
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (up)
    {
        HIP_TRY(copy(s.B.p, (double*)s.desc.B, Ns));
        HIP_TRY(copy(s.proj.p, (double*)s.desc.cosGamma, Nr * Ns));
        HIP_TRY(copy(s.proj.p + Nr * Ns, (double*)s.desc.cos2chi, Nr * Ns));
        HIP_TRY(copy(s.proj.p + 2 * Nr * Ns, (double*)s.desc.sin2chi, Nr * Ns));
    }
    else
        HIP_TRY(copy(s.Quv.p, s.desc.Quv, 3 * Nla * Nr));
    if (s.desc.J20)
        HIP_TRY(copy(s.J20.p, s.desc.J20, Nla * Ns));
    for (size_t i = 0; i < s.lines.size(); ++i)
    {
        const lwhip_stokes_line& L = s.lines[i];
        const size_t nPer = (size_t)(c->trans[s.lineTr[i]].t.Nred - c->trans[s.lineTr[i]].t.Nblue) * Nr * 2 * Ns;
        double* arrs[6] = { L.phiQ, L.phiU, L.phiV, L.psiQ, L.psiU, L.psiV };
        if (!up && !s.polOnDevice)
            break; // (the host's arrays are what the device holds: nothing to bring back)
        for (int q = 0; q < 6; ++q)
            if (arrs[q])
                HIP_TRY(copy(s.pol.p + s.polOff[i] + q * nPer, arrs[q], nPer));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    s.polOnDevice = false;
    return LWHIP_OK;
}
} // namespace lwhip

extern "C"
{
int lwhip_set_stokes(lwhip_context* c, const lwhip_stokes* st)
{
    int chk = check_stokes_ctx(c, "lwhip_set_stokes", false);
    if (chk != LWHIP_OK)
        return chk;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    StokesState& s = c->stokes;
    s.on = false;
    if (!st)
        return LWHIP_OK;
    const int Ns = c->Ns, Nr = c->Nrays, Nla = c->Nla;
    if (!st->B || !st->cosGamma || !st->cos2chi || !st->sin2chi || !st->Quv || st->Nlines < 0 || (st->Nlines > 0 && !st->lines))
        return fail(LWHIP_ERR_INVALID, "lwhip_set_stokes: B, cosGamma, cos2chi, sin2chi and Quv are required");
    s.desc = *st;
    s.lines.assign(st->lines, st->lines + st->Nlines);
    s.desc.lines = s.lines.data();
    s.lineTr.clear();
    s.polOff.clear();
    s.polTot = 0;
    std::vector<int> polOfTr(c->trans.size(), -1);
    std::vector<int32_t> alpha;
    std::vector<double> comp; // shift then strength, per line back to back
    std::vector<int> compOff;
    for (int i = 0; i < st->Nlines; ++i)
    {
        const lwhip_stokes_line& L = s.lines[i];
        if (L.atom < 0 || L.atom >= c->Natom || L.trans < 0 || L.trans >= c->atoms[L.atom].Ntrans)
            return fail(LWHIP_ERR_INVALID, "lwhip_set_stokes: polarised line " + std::to_string(i) + " is not in the problem");
        const int tr = c->atomTrOff[L.atom] + L.trans;
        const HostTrans& h = c->trans[tr];
        if (h.t.type != LWHIP_LINE)
            return fail(LWHIP_ERR_INVALID, "lwhip_set_stokes: polarised transition " + std::to_string(i) + " is not a line");
        if (polOfTr[tr] >= 0)
            return fail(LWHIP_ERR_INVALID, "lwhip_set_stokes: line " + std::to_string(i) + " listed twice");
        if (L.Ncomp < 0 || (L.Ncomp > 0 && (!L.alpha || !L.shift || !L.strength)))
            return fail(LWHIP_ERR_INVALID, "lwhip_set_stokes: Zeeman components of line " + std::to_string(i));
        if (!h.t.aDamp)
            return fail(LWHIP_ERR_INVALID, "lwhip_set_stokes: polarised line " + std::to_string(i) + " needs aDamp");
        polOfTr[tr] = i;
        s.lineTr.push_back(tr);
        s.polOff.push_back(s.polTot);
        s.polTot += (int64_t)6 * (h.t.Nred - h.t.Nblue) * Nr * 2 * Ns;
        compOff.push_back((int)alpha.size());
        for (int q = 0; q < L.Ncomp; ++q)
            alpha.push_back(L.alpha[q]);
    }
    const size_t nComp = alpha.size();
    comp.resize(2 * std::max<size_t>(nComp, 1), 0.0);
    for (int i = 0; i < st->Nlines; ++i)
        for (int q = 0; q < s.lines[i].Ncomp; ++q)
        {
            comp[compOff[i] + q] = s.lines[i].shift[q];
            comp[nComp + compOff[i] + q] = s.lines[i].strength[q];
        }
    // the transitions active at each wavelength, in the reference's order (active atoms, then detailed ones; kr order)
    std::vector<StokesTrans> trs(c->trans.size());
    std::vector<int32_t> laOff(Nla + 1, 0), laTr, laPol(Nla, 0);
    for (size_t tr = 0; tr < c->trans.size(); ++tr)
    {
        const HostTrans& h = c->trans[tr];
        StokesTrans& t = trs[tr];
        t = StokesTrans{};
        t.type = h.t.type;
        t.gi = c->levelOff[h.atom] + h.t.i;
        t.gj = c->levelOff[h.atom] + h.t.j;
        t.Nblue = h.t.Nblue;
        t.prd = (h.t.type == LWHIP_LINE && h.t.prd && h.rhoOff >= 0) ? 1 : 0;
        t.row = h.row;
        t.pol = polOfTr[tr];
        t.parOff = h.parOff;
        t.phiOff = h.phiOff;
        t.rhoOff = h.rhoOff >= 0 ? h.rhoOff - (int64_t)h.rhoLt0 * Ns : 0;
        if (t.pol >= 0)
        {
            t.polOff = s.polOff[t.pol];
            t.polStride = (int64_t)(h.t.Nred - h.t.Nblue) * Nr * 2 * Ns;
        }
    }
    for (int la = 0; la < Nla; ++la)
    {
        laOff[la] = (int32_t)laTr.size();
        for (size_t tr = 0; tr < c->trans.size(); ++tr)
        {
            const HostTrans& h = c->trans[tr];
            if (la >= h.t.Nblue && la < h.t.Nred)
            {
                laTr.push_back((int32_t)tr);
                if (polOfTr[tr] >= 0)
                    laPol[la] = 1;
            }
        }
    }
    laOff[Nla] = (int32_t)laTr.size();
    if (laTr.empty())
        laTr.push_back(0);
    s.laPolHost = laPol;
    HIP_TRY(s.tr.upload(c->mem, trs));
    HIP_TRY(s.laOff.upload(c->mem, laOff));
    HIP_TRY(s.laTr.upload(c->mem, laTr));
    HIP_TRY(s.laPol.upload(c->mem, laPol));
    if (alpha.empty())
        alpha.push_back(0);
    HIP_TRY(s.alpha.upload(c->mem, alpha));
    HIP_TRY(s.comp.upload(c->mem, comp));
    HIP_TRY(s.B.alloc(c->mem, Ns));
    HIP_TRY(s.proj.alloc(c->mem, (size_t)3 * Nr * Ns));
    HIP_TRY(s.pol.alloc_zero(c->mem, (size_t)std::max<int64_t>(s.polTot, 1)));
    HIP_TRY(s.Quv.alloc_zero(c->mem, (size_t)3 * Nla * Nr));
    if (st->J20)
        HIP_TRY(s.J20.alloc(c->mem, (size_t)Nla * Ns));
    else
        s.J20.release();
    HIP_TRY(s.dJ.alloc_zero(c->mem, (size_t)Nla));
    HIP_TRY(s.singular.alloc_zero(c->mem, 1));
    // the profile kernels' argument blocks
    s.argsHost.clear();
    for (int i = 0; i < st->Nlines; ++i)
    {
        const HostTrans& h = c->trans[s.lineTr[i]];
        PolLineArgs a{};
        a.Ns = Ns;
        a.Nrays = Nr;
        a.nlt = h.t.Nred - h.t.Nblue;
        a.nComp = s.lines[i].Ncomp;
        a.lambda0 = h.t.lambda0;
        a.wave = c->lineWave.p + h.waveOff;
        a.wlam = c->lineWlam.p + h.waveOff;
        a.vlosMu = c->vlosMu.p;
        a.wmu = c->wmu.p;
        a.vBroad = c->vBroad.p + (size_t)h.atom * Ns;
        a.aDamp = c->aDamp.p + (size_t)h.row * Ns;
        a.B = s.B.p;
        a.cosGamma = s.proj.p;
        a.cos2chi = s.proj.p + (size_t)Nr * Ns;
        a.sin2chi = s.proj.p + (size_t)2 * Nr * Ns;
        a.alpha = s.alpha.p + compOff[i];
        a.shift = s.comp.p + compOff[i];
        a.strength = s.comp.p + nComp + compOff[i];
        a.phi = c->phi.p + h.phiOff;
        a.wphi = c->wphi.p + (size_t)h.row * Ns;
        a.pol = s.pol.p + s.polOff[i];
        s.argsHost.push_back(a);
    }
    if (!s.argsHost.empty())
        HIP_TRY(s.args.upload(c->mem, s.argsHost));
    s.on = true;
    return stokes_transfer(c, true);
}

int lwhip_compute_polarised_profiles(lwhip_context* c)
{
    int chk = check_stokes_ctx(c, "lwhip_compute_polarised_profiles", true);
    if (chk != LWHIP_OK)
        return chk;
    HIP_TRY(hipSetDevice(c->device));
    // Device-made profiles whose inputs were uploaded again are regenerated FIRST: done later (by the next sweep or Stokes
    // call) it would overwrite the polarised lines' phi with the plain Voigt profile.
    {
        const int stp = ensure_profiles(c);
        if (stp != LWHIP_OK)
            return stp;
    }
    StokesState& s = c->stokes;
    if (s.argsHost.empty())
        return LWHIP_OK;
    if (!c->lineWave.p || !c->lineWlam.p)
        return fail(LWHIP_ERR_INVALID, "lwhip_compute_polarised_profiles: the context has no line grids on the device");
    HIP_TRY(launch_polarised_profiles(s.args.p, s.argsHost.data(), (int)s.argsHost.size(), c->stream));
    s.polOnDevice = true;
    // phi of the polarised lines changed: the two directions of an angle stay alike only without line-of-sight velocities
    c->phiSym = c->phiSym && c->vlosZero;
    return retile_profiles(c);
}

int lwhip_full_stokes_fs(lwhip_context* c, int updateJ, int upOnly, lwhip_iter_result* res)
{
    int chk = check_stokes_ctx(c, "lwhip_full_stokes_fs", true);
    if (chk != LWHIP_OK)
        return chk;
    HIP_TRY(hipSetDevice(c->device));
    if (updateJ && c->JhostReg)
        return fail(LWHIP_ERR_UNSUPPORTED, "lwhip_full_stokes_fs: updateJ with a mapped host J (lwhip_map_host_J(ctx, 0) first)");
    if (c->Ns < 3)
        return fail(LWHIP_ERR_INVALID, "lwhip_full_stokes_fs: needs at least 3 depth points");
    {
        const int stp = ensure_profiles(c);
        if (stp != LWHIP_OK)
            return stp;
    }
    StokesState& s = c->stokes;
    const int Ns = c->Ns, Nr = c->Nrays, Nla = c->Nla;
    const int nDir = upOnly ? 1 : 2;
    // wavelength chunks: the rows of a chunk's rays stay within 256 MB; LWHIP_STOKES_CHUNK_LA (LWHIP_DEBUG) sets the
    // wavelengths of a chunk instead (the results are the same bits for any chunking, tested)
    const size_t perLa = (size_t)Nr * nDir * (ST_ROWS + (updateJ ? 2 : 0)) * Ns * sizeof(double);
    int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)Nla, ((size_t)256 << 20) / perLa));
    const int dbgChunk = dbg_env_int("LWHIP_STOKES_CHUNK_LA", 0);
    if (dbgChunk > 0)
        chunk = std::max(1, std::min(Nla, dbgChunk));
    const size_t raysChunk = (size_t)chunk * Nr * nDir;
    if (s.scratch.n < raysChunk * ST_ROWS * Ns)
        HIP_TRY(s.scratch.alloc(c->mem, raysChunk * ST_ROWS * Ns));
    if (updateJ && s.Isc.n < raysChunk * 2 * Ns)
        HIP_TRY(s.Isc.alloc(c->mem, raysChunk * 2 * Ns));
    StokesArgs a{};
    a.Ns = Ns;
    a.Nr = Nr;
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
    a.scratch = s.scratch.p;
    a.Isc = s.Isc.p;
    a.I = c->I.p;
    a.Quv = s.Quv.p;
    a.dJ = s.dJ.p;
    a.singular = s.singular.p;
    HIP_TRY(hipMemsetAsync(s.singular.p, 0, sizeof(int32_t), c->stream));
    for (int la0 = 0; la0 < Nla; la0 += chunk)
    {
        a.la0 = la0;
        a.nla = std::min(chunk, Nla - la0);
        const size_t nRay = (size_t)a.nla * Nr * nDir;
        const int gBlocks = (int)std::min<size_t>((nRay * Ns + 255) / 256, 16384);
        LWHIP_LAUNCH(stokes_gather_kernel, dim3(gBlocks), dim3(256), 0, c->stream, a);
        LWHIP_LAUNCH(stokes_march_kernel, dim3((unsigned)((nRay + 63) / 64)), dim3(64), 0, c->stream, a);
        if (updateJ)
            LWHIP_LAUNCH(stokes_j_kernel, dim3((a.nla + 63) / 64), dim3(64), 0, c->stream, a);
        HIP_TRY(hipGetLastError());
    }
    if (updateJ)
        c->fpJValid = false;
    int32_t singular = 0;
    HIP_TRY(hipMemcpyAsync(&singular, s.singular.p, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (res)
    {
        res->updatedJ = updateJ ? 1 : 0;
        res->dJMax = 0.0;
        res->dJMaxIdx = 0;
    }
    if (updateJ)
    {
        // formal_sol_full_stokes_impl's serial loop: dJMax = max_idx(dJ, dJMax, maxIdx, la) (FormalStokes.cpp:708-714)
        std::vector<double> dJ(Nla);
        HIP_TRY(hipMemcpyAsync(dJ.data(), s.dJ.p, Nla * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        double dJMax = 0.0;
        int maxIdx = 0;
        for (int la = 0; la < Nla; ++la)
        {
            if (dJ[la] < dJMax)
                maxIdx = la;
            else
                dJMax = dJ[la];
        }
        if (res)
        {
            res->dJMax = dJMax;
            res->dJMaxIdx = maxIdx;
        }
    }
    else
        HIP_TRY(hipStreamSynchronize(c->stream));
    if (singular)
        return fail(LWHIP_ERR_SINGULAR, "lwhip_full_stokes_fs: Singular Matrix in the 4 x 4 DELO-Bezier3 step");
    return LWHIP_OK;
}
}
