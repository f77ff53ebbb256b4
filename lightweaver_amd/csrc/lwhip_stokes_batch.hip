// lwhip_stokes_batch.hip -- the polarised profiles of a 1.5D column batch (lwhip_batch_compute_polarised_profiles: every
// column's lines in one list of launches) and the refusals the batch's two Stokes entry points share.  The formal solution,
// lwhip_batch_full_stokes_fs, is lwhip_stokes_fs.hip's: the same driver and kernels as a context on its own.
#include "lwhip_host.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace lwhip
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
    std::vector<PolLineArgs> list;
    for (lwhip_context* c : b->ctxs)
        list.insert(list.end(), c->stokes.argsHost.begin(), c->stokes.argsHost.end());
    // (uploaded again only when a column's blocks changed; the host copy is the source of the queued copy)
    const bool changed = b->polHost.size() != list.size() || std::memcmp(b->polHost.data(), list.data(), list.size() * sizeof(PolLineArgs)) != 0;
    if (changed)
    {
        HIP_TRY(hipStreamSynchronize(c0->stream)); // nothing may still read the blocks about to be replaced
        b->polHost.swap(list);
    }
    const int stl = launch_list(c0, b->polList, b->polHost, changed, launch_polarised_profiles);
    if (stl != LWHIP_OK)
        return stl;
    for (lwhip_context* c : b->ctxs)
    {
        c->stokes.polOnDevice = true;
        c->phiSym = c->phiSym && c->vlosZero;
        c->phiIso = false; // (phi of a Zeeman-split line depends on the angle even at rest: lwhip_stokes.hip)
    }
    return batch_retile(b, b->ctxs);
}
}
