// lwhip_stokes.hip -- the Stokes data of a context for Zeeman-polarised lines (1D plane-parallel): lwhip_set_stokes, its
// transfers, the refusals the Stokes entry points share and lwhip_compute_polarised_profiles (whose kernels live with the
// other Voigt kernels in lwhip_voigt.hip).  The formal solution that reads all this is lwhip_stokes_fs.hip.
#include "lwhip_host.h"

#include <algorithm>
#include <vector>

namespace lwhip
{
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
    std::vector<int32_t> laOff, laTr, laPol(Nla, 0);
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
    active_trans_lists(c->trans, Nla, false, laOff, laTr);
    for (int la = 0; la < Nla; ++la)
        for (int q = laOff[la]; q < laOff[la + 1]; ++q)
            if (polOfTr[laTr[q]] >= 0)
                laPol[la] = 1;
    s.laPolHost = laPol;
    HIP_TRY(s.tr.upload(c->mem, trs));
    HIP_TRY(s.laOff.upload(c->mem, laOff));
    HIP_TRY(s.laTr.upload(c->mem, laTr));
    HIP_TRY(s.laPol.upload(c->mem, laPol));
    {
        std::vector<int32_t> polComp(2 * std::max<size_t>(s.lines.size(), 1), 0);
        for (size_t i = 0; i < s.lines.size(); ++i)
        {
            polComp[2 * i] = compOff[i];
            polComp[2 * i + 1] = s.lines[i].Ncomp;
        }
        HIP_TRY(s.ev.upload(c->mem, line_eval_records(c->trans)));
        HIP_TRY(s.polComp.upload(c->mem, polComp));
        s.nComp = (int64_t)nComp;
    }
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
    c->phiIso = false; // (a Zeeman-split line's phi holds sin^2 gamma of the ray: it depends on the angle even at rest)
    return retile_profiles(c);
}
}
