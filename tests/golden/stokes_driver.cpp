// tests/golden/stokes_driver.cpp -- TEST INFRASTRUCTURE: the full-Stokes calls of the REAL Lightweaver core, for
// make_stokes_golden.py.  Compiled by that script into a temporary directory together with the reference's own sources
// (flags of oracle/Makefile); nothing of it or of the reference enters the tree.  The core Context is built by
// oracle/ref_driver.cpp (lwref_create); this adds what a polarised problem needs on top of it:
//
//   lwrefs_stokes(h, st, gammaB, chiB, mux, muy, vz)  Atmosphere B / gammaB / chiB / mux / muy / vz and the projection
//                       arrays (written by Atmosphere::update_projections, Source/Atmosphere.cpp:5-82), every line of
//                       `st` polarised with its components and its phiQ..psiV arrays, Spectrum::Quv = st->Quv;
//   lwrefs_polarised_profiles(h)   Transition::compute_polarised_profiles of every polarised line (FormalStokes.cpp:9-117)
//   lwrefs_full_stokes(h, updateJ, upOnly, J20, res)   formal_sol_full_stokes (:725-729), ExtraParams "J20" if J20 != NULL
#include "../../oracle/ref_driver.cpp"

namespace
{
struct StokesExtra
{
    std::vector<std::pair<int, int>> lines; // (atom, trans)
    std::vector<ZeemanComponents> comps;
};
}

extern "C"
{
int lwrefs_stokes(void* h, const lwhip_stokes* st, const double* gammaB, const double* chiB, const double* mux,
                  const double* muy, const double* vz, void** extra, char* err, int errLen)
{
    try
    {
        auto* rc = (RefContext*)h;
        const lwhip_problem* p = rc->prob;
        const int Ns = p->Nspace, Nr = p->Nrays, Nla = p->Nlambda;
        auto& a = rc->atmos;
        a.B = F64View(const_cast<f64*>(st->B), Ns);
        a.gammaB = F64View(const_cast<f64*>(gammaB), Ns);
        a.chiB = F64View(const_cast<f64*>(chiB), Ns);
        a.mux = F64View(const_cast<f64*>(mux), Nr);
        a.muy = F64View(const_cast<f64*>(muy), Nr);
        a.vz = F64View(const_cast<f64*>(vz), Ns);
        a.cosGamma = F64View2D(const_cast<f64*>(st->cosGamma), Nr, Ns);
        a.cos2chi = F64View2D(const_cast<f64*>(st->cos2chi), Nr, Ns);
        a.sin2chi = F64View2D(const_cast<f64*>(st->sin2chi), Nr, Ns);
        a.update_projections();
        rc->spect.Quv = F64View4D(st->Quv, 3, Nla, Nr, 1);
        auto* ex = new StokesExtra;
        for (int i = 0; i < st->Nlines; ++i)
        {
            const lwhip_stokes_line& L = st->lines[i];
            Transition* t = rc->atoms[L.atom]->trans[L.trans];
            const int Nl = t->Nred - t->Nblue;
            t->polarised = true;
            t->phiQ = F64View4D(L.phiQ, Nl, Nr, 2, Ns);
            t->phiU = F64View4D(L.phiU, Nl, Nr, 2, Ns);
            t->phiV = F64View4D(L.phiV, Nl, Nr, 2, Ns);
            t->psiQ = F64View4D(L.psiQ, Nl, Nr, 2, Ns);
            t->psiU = F64View4D(L.psiU, Nl, Nr, 2, Ns);
            t->psiV = F64View4D(L.psiV, Nl, Nr, 2, Ns);
            ZeemanComponents z;
            z.alpha = I32View(const_cast<i32*>(L.alpha), L.Ncomp);
            z.shift = F64View(const_cast<f64*>(L.shift), L.Ncomp);
            z.strength = F64View(const_cast<f64*>(L.strength), L.Ncomp);
            ex->lines.emplace_back(L.atom, L.trans);
            ex->comps.push_back(z);
        }
        *extra = ex;
        return 0;
    }
    catch (const std::exception& e)
    {
        set_error(err, errLen, e.what());
        return 1;
    }
}

int lwrefs_polarised_profiles(void* h, void* extra, char* err, int errLen)
{
    try
    {
        auto* rc = (RefContext*)h;
        auto* ex = (StokesExtra*)extra;
        for (size_t i = 0; i < ex->lines.size(); ++i)
        {
            Atom* atom = rc->atoms[ex->lines[i].first].get();
            Transition* t = atom->trans[ex->lines[i].second];
            t->compute_polarised_profiles(rc->atmos, t->aDamp, atom->vBroad, ex->comps[i]);
        }
        return 0;
    }
    catch (const std::exception& e)
    {
        set_error(err, errLen, e.what());
        return 1;
    }
}

int lwrefs_full_stokes(void* h, int updateJ, int upOnly, double* J20, lwhip_iter_result* res, char* err, int errLen)
{
    try
    {
        auto* rc = (RefContext*)h;
        ExtraParams params;
        if (J20)
            params.insert<F64View2D>("J20", F64View2D(J20, rc->prob->Nlambda, rc->prob->Nspace));
        IterationResult r = formal_sol_full_stokes(rc->ctx, updateJ != 0, upOnly != 0, params);
        res->updatedJ = r.updatedJ;
        res->dJMax = r.dJMax;
        res->dJMaxIdx = r.dJMaxIdx;
        return 0;
    }
    catch (const std::exception& e)
    {
        set_error(err, errLen, e.what());
        return 1;
    }
}

void lwrefs_free(void* extra)
{
    delete (StokesExtra*)extra;
}
}
