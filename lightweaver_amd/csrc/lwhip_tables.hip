// lwhip_tables.hip -- host side of the C ABI (lwhip_host.h): validation of the problem descriptor and the per-wavelength
// activity tables the sweep kernels walk (tiles, slots, chunks, the lane sweep's flat records, PRD wavelength lists).
//
// lwhip_create's structure tables are made in two halves.  plan_tables is device-free: from the context's host fields
// (context_init_host), the knobs of the environment (TableKnobs) and the device's compute-unit count it decides which sweep the
// context gets and fills a TablePlan (the scalars) and the HostTables (every vector that goes to the device), one named stage
// after the other.  upload_tables sends them, in a fixed order on the context's stream.  build_tables is the driver.
#include "lwhip_host.h"

namespace lwhip
{
int validate(const lwhip_problem* p, std::string& why)
{
    if (!p)
    {
        why = "null problem";
        return LWHIP_ERR_INVALID;
    }
    if (p->abiVersion != LWHIP_ABI_VERSION)
    {
        why = "ABI version mismatch";
        return LWHIP_ERR_INVALID;
    }
    if (p->Nspace < 3 || p->Nrays < 1 || p->Nlambda < 1 || p->Natom < 0)
    {
        why = "need Nspace >= 3, Nrays >= 1, Nlambda >= 1";
        return LWHIP_ERR_INVALID;
    }
    if (p->grid2d)
    {
        const lwhip_grid2d& g = *p->grid2d;
        if (g.Nx < 2 || g.Nz < 2 || g.Nx > 1024 || g.Nx * g.Nz != p->Nspace || g.Nrays != p->Nrays)
        {
            why = "2D grid: 2 <= Nx <= 1024, Nz >= 2, Nx * Nz = Nspace, Nrays matching";
            return LWHIP_ERR_UNSUPPORTED;
        }
        if (g.Nrays > 32)
        {
            // rates2d_kernel keeps the pass's 2 Nrays directions (half weight, ray index) in an LDS table of 64 entries
            why = "2D grid: Nrays <= 32 (rates2d_kernel's ray table in LDS holds the 64 directions of 32 rays)";
            return LWHIP_ERR_UNSUPPORTED;
        }
        if ((g.zLowerBc == LWHIP_BC_CALLABLE) != (p->zLowerBc.type == LWHIP_BC_CALLABLE)
            || (g.zUpperBc == LWHIP_BC_CALLABLE) != (p->zUpperBc.type == LWHIP_BC_CALLABLE))
        {
            why = "2D grid: a CALLABLE z boundary needs lwhip_problem.zLowerBc / zUpperBc of type CALLABLE (bcData [Nlambda, Nmu, Nx])";
            return LWHIP_ERR_INVALID;
        }
        for (int bt : { g.zLowerBc, g.zUpperBc })
            if (bt != LWHIP_BC_ZERO && bt != LWHIP_BC_THERMALISED && bt != LWHIP_BC_CALLABLE)
            {
                why = "2D grid: z boundaries are ZERO, THERMALISED or CALLABLE";
                return LWHIP_ERR_UNSUPPORTED;
            }
        if (!g.periodic)
        {
            // "Mixed boundary types not supported on x-axis!" (Source/FormalScalar2d.cpp:750-759)
            auto ok = [&](const lwhip_boundary* b) {
                return b && b->type == LWHIP_BC_CALLABLE && b->idxs && b->bcData && b->Nmu > 0;
            };
            if (!ok(g.xLowerBc) || !ok(g.xUpperBc) || g.NlongChar != 0)
            {
                why = "2D grid without periodic x: both x boundaries CALLABLE (idxs, bcData [Nlambda, Nmu, Nz]), no long characteristics";
                return LWHIP_ERR_UNSUPPORTED;
            }
            for (int q = 0; q < 2 * g.Nrays; ++q)
                if (g.xLowerBc->idxs[q] < 0 || g.xLowerBc->idxs[q] >= g.xLowerBc->Nmu || g.xUpperBc->idxs[q] < 0
                    || g.xUpperBc->idxs[q] >= g.xUpperBc->Nmu)
                {
                    why = "2D grid: x boundary idxs out of range (\"Error in boundary condition indexing\")";
                    return LWHIP_ERR_INVALID;
                }
        }
        if (!g.mux || !g.uw || !g.dw || !g.longCharIdx || !g.substepOff || (g.NlongChar > 0 && !g.substeps))
        {
            why = "2D grid: incomplete intersection table";
            return LWHIP_ERR_INVALID;
        }
        if (!fs2d_long_chars_ok(&g))
        {
            why = "2D grid: a long characteristic that does not end on a z plane";
            return LWHIP_ERR_UNSUPPORTED;
        }
        if (p->storeDepthData && (!p->depthChi || !p->depthEta || !p->depthI))
        {
            why = "storeDepthData set but depth arrays are null";
            return LWHIP_ERR_INVALID;
        }
    }
    else if (p->Nspace > 1024)
    {
        why = "Nspace > 1024 is not supported by the 1D sweep kernel";
        return LWHIP_ERR_UNSUPPORTED;
    }
    if (!p->grid2d && (p->formalSolver < LWHIP_FS_LINEAR_1D || p->formalSolver > LWHIP_FS_BEZIER3_1D))
    {
        why = "unknown formal solver";
        return LWHIP_ERR_INVALID;
    }
    if (!p->height || !p->temperature || !p->muz || !p->wmu || !p->wavelength || !p->bgChi
        || !p->bgEta || !p->bgSca || !p->J || !p->I)
    {
        why = "null atmosphere / spectrum / background array";
        return LWHIP_ERR_INVALID;
    }
    if (p->storeDepthData && (!p->depthChi || !p->depthEta || !p->depthI))
    {
        why = "storeDepthData set but depth arrays are null";
        return LWHIP_ERR_INVALID;
    }
    const lwhip_boundary* bcs[2] = { &p->zLowerBc, &p->zUpperBc };
    for (auto* b : bcs)
    {
        if (b->type == LWHIP_BC_CALLABLE && (!b->idxs || !b->bcData || b->Nmu < 1))
        {
            why = "CALLABLE boundary needs idxs, bcData, Nmu";
            return LWHIP_ERR_INVALID;
        }
    }
    bool seenDetailed = false;
    for (int ia = 0; ia < p->Natom; ++ia)
    {
        const lwhip_atom& a = p->atoms[ia];
        if (a.Nlevel < 1 || a.Nlevel > 32 || a.Ntrans < 0)
        {
            why = "atom needs 1 <= Nlevel <= 32";
            return a.Nlevel > 32 ? LWHIP_ERR_UNSUPPORTED : LWHIP_ERR_INVALID;
        }
        if (a.detailed)
            seenDetailed = true;
        else if (seenDetailed)
        {
            why = "active atoms must precede detailed atoms";
            return LWHIP_ERR_INVALID;
        }
        if (!a.n || !a.nStar || !a.nTotal || !a.vBroad || (!a.detailed && !a.Gamma))
        {
            why = "null atom array";
            return LWHIP_ERR_INVALID;
        }
        for (int kr = 0; kr < a.Ntrans; ++kr)
        {
            const lwhip_transition& t = a.trans[kr];
            if (t.i < 0 || t.j < 0 || t.i >= a.Nlevel || t.j >= a.Nlevel || t.i == t.j)
            {
                why = "bad transition levels";
                return LWHIP_ERR_INVALID;
            }
            if (t.Nblue < 0 || t.Nred > p->Nlambda || t.Nred - t.Nblue < 2)
            {
                why = "bad transition wavelength range (need >= 2 points inside the grid)";
                return LWHIP_ERR_INVALID;
            }
            if (!t.wavelength || !t.Rij || !t.Rji)
            {
                why = "null transition array";
                return LWHIP_ERR_INVALID;
            }
            if (t.type == LWHIP_LINE)
            {
                if (!t.phi || !t.wphi)
                {
                    why = "line without phi/wphi";
                    return LWHIP_ERR_INVALID;
                }
                if (t.prd && !t.rhoPrd)
                {
                    why = "prd line without rhoPrd";
                    return LWHIP_ERR_INVALID;
                }
            }
            else if (t.type == LWHIP_CONTINUUM)
            {
                if (!t.alpha)
                {
                    why = "continuum without alpha";
                    return LWHIP_ERR_INVALID;
                }
            }
            else
            {
                why = "unknown transition type";
                return LWHIP_ERR_INVALID;
            }
        }
    }
    return LWHIP_OK;
}

// Everything the structure tables depend on, folded into 64 bits: sizes, solver, shard, the wavelength grid, and of every
// transition its levels, wavelength range, Einstein coefficients, own grid and cross-sections.  Two contexts with the same
// fingerprint build the same tables (populations, atmosphere, profiles, boundary data live elsewhere).
uint64_t structure_signature(const lwhip_context* c)
{
    uint64_t h = 0x9E3779B97F4A7C15ull;
    auto mix = [&](uint64_t v) {
        h ^= v + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2);
        h *= 0xFF51AFD7ED558CCDull;
        h ^= h >> 33;
    };
    auto mixd = [&](double v) {
        uint64_t u;
        std::memcpy(&u, &v, 8);
        mix(u);
    };
    auto mixv = [&](const double* p, size_t n) {
        mix(n);
        for (size_t i = 0; p && i < n; ++i)
            mixd(p[i]);
    };
    const lwhip_problem& p = c->prob;
    for (int64_t v : { (int64_t)p.Nlambda, (int64_t)p.Nspace, (int64_t)p.Nrays, (int64_t)p.Natom, (int64_t)p.formalSolver,
                       (int64_t)c->laStart, (int64_t)c->laEnd, (int64_t)c->worldSize, (int64_t)c->batchHint, (int64_t)c->prdDetailed,
                       (int64_t)c->deterministic, (int64_t)(c->hprd != nullptr), (int64_t)c->is2d, (int64_t)p.storeDepthData,
                       (int64_t)c->device })
        mix((uint64_t)v);
    mixv(p.wavelength, (size_t)p.Nlambda);
    for (int ia = 0; ia < p.Natom; ++ia)
    {
        const lwhip_atom& a = c->atoms[ia];
        mix((uint64_t)a.Nlevel);
        mix((uint64_t)a.Ntrans);
        mix((uint64_t)(a.detailed != 0));
        mix((uint64_t)(a.C != nullptr));
        for (int kr = 0; kr < a.Ntrans; ++kr)
        {
            const lwhip_transition& t = a.trans[kr];
            for (int64_t v : { (int64_t)t.type, (int64_t)t.i, (int64_t)t.j, (int64_t)t.Nblue, (int64_t)t.Nred, (int64_t)(t.prd != 0),
                               (int64_t)(t.rhoPrd != nullptr) })
                mix((uint64_t)v);
            mixd(t.Aji);
            mixd(t.Bji);
            mixd(t.Bij);
            mixd(t.lambda0);
            mixd(t.dopplerWidth);
            mixv(t.wavelength, (size_t)std::max(t.Nred - t.Nblue, 0));
            if (t.type != LWHIP_LINE)
                mixv(t.alpha, (size_t)std::max(t.Nred - t.Nblue, 0));
        }
    }
    return h;
}

// The host fields of a context that do not need a device: the copy of the descriptor, the options, the shard, the sizes.
// What lwhip_create does first; with it a program without a device can prepare a context for plan_tables.
int context_init_host(lwhip_context* c, const lwhip_problem* prob, const lwhip_options* opts)
{
    c->prob = *prob;
    c->atoms.assign(prob->atoms, prob->atoms + prob->Natom);
    c->device = opts ? opts->device : 0;
    c->batchHint = opts ? (opts->flags & 0xffff) : 0;
    c->prdDetailed = opts && (opts->flags & LWHIP_OPT_PRD_DETAILED);
    c->hprd = opts ? opts->hprd : nullptr;
    // (as asked for: the plan turns it off where the ray-column march serves the context)
    c->deterministic = ((opts && (opts->flags & LWHIP_OPT_DETERMINISTIC)) || env_int("LWHIP_DETERMINISTIC", 0) == 1)
                       && (!opts || (opts->flags & 0xffff) <= 1);
    c->laStart = 0;
    c->laEnd = prob->Nlambda;
    if (opts && !(opts->laStart == 0 && opts->laEnd == 0))
    {
        c->laStart = opts->laStart;
        c->laEnd = opts->laEnd;
        if (c->laStart < 0 || c->laEnd > prob->Nlambda || c->laEnd <= c->laStart)
            return fail(LWHIP_ERR_INVALID, "lwhip_create: bad wavelength shard");
    }
    if (opts && opts->worldSize > 1)
    {
        c->worldSize = opts->worldSize;
        c->worldRank = opts->worldRank;
        if (c->worldRank < 0 || c->worldRank >= c->worldSize)
            return fail(LWHIP_ERR_INVALID, "lwhip_create: bad worldRank");
    }
    c->is2d = prob->grid2d != nullptr;
    c->Nx = c->is2d ? prob->grid2d->Nx : 1;
    c->Nla = c->laEnd - c->laStart;
    c->Ns = prob->Nspace;
    c->Nrays = prob->Nrays;
    c->Natom = prob->Natom;
    return LWHIP_OK;
}

// Every environment read that shapes the tables.  LWHIP_SWEEP, LWHIP_VERBOSE and LWHIP_CREATE_TIMING are read in any process,
// the layout knobs only under LWHIP_DEBUG (dbg_env_int): the list is in INTEGRATION.md section 5.
TableKnobs read_table_knobs()
{
    auto optional = [](const char* name) {
        const char* v = std::getenv(name);
        TableKnobs::OptInt o;
        o.set = debug_knobs_on() && v && *v;
        o.v = o.set ? std::atoi(v) : 0;
        return o;
    };
    TableKnobs k;
    k.createTiming = std::getenv("LWHIP_CREATE_TIMING") != nullptr;
    k.verbose = std::getenv("LWHIP_VERBOSE") != nullptr;
    const char* sw = std::getenv("LWHIP_SWEEP");
    k.sweepGiven = sw != nullptr;
    k.sweepLanes = sw && std::strcmp(sw, "lanes") == 0;
    k.sweepMarch = sw && std::strcmp(sw, "march") == 0;
    k.tileGeneric = dbg_env_int("LWHIP_TILE_GENERIC", 0);
    k.laneGeneric = dbg_env_int("LWHIP_LANE_GENERIC", 1);
    k.tileL = dbg_env_int("LWHIP_TILE_L", 16);
    k.tileLH = optional("LWHIP_TILE_LH");
    k.tileL1 = optional("LWHIP_TILE_L1");
    k.lWaves = dbg_env_int("LWHIP_LWAVES", 4);
    k.tWaves = dbg_env_int("LWHIP_TWAVES", 2);
    k.tileFuse = dbg_env_int("LWHIP_TILE_FUSE", 1);
    k.laneSplit = dbg_env_int("LWHIP_LANE_SPLIT", 0);
    k.laneCut = optional("LWHIP_LANE_CUT");
    k.depthSplit = dbg_env_int("LWHIP_DEPTH_SPLIT", -1);
    k.detNoWait = dbg_env_int("LWHIP_DET_NOWAIT", 0);
    k.finFast = dbg_env_int("LWHIP_FIN_FAST", 1);
    return k;
}

namespace
{
// LWHIP_CREATE_TIMING=1: where the host time of the tables goes
struct Ticker
{
    bool on;
    std::chrono::steady_clock::time_point prev = std::chrono::steady_clock::now();
    void operator()(const char* what)
    {
        if (!on)
            return;
        const auto now = std::chrono::steady_clock::now();
        std::fprintf(stderr, "  build_tables: %-28s %.3f ms\n", what, std::chrono::duration<double, std::milli>(now - prev).count());
        prev = now;
    }
};

// the kinds of tile the lane sweep has compiled: anything else runs its generic kind (or the march)
bool fast_kind(int nLine, int nMixed)
{
    return (nLine == 0 && nMixed == 0) || (nLine == 1 && nMixed <= 1) || (nLine == 2 && nMixed == 0);
}
// what a tile costs its wavefront, for the order in which workgroups and tasks are taken
double task_cost(const DevTile& td)
{
    return 1.0 + 0.5 * td.nLine + 0.3 * td.nMixed + (td.nLine == 0 ? -0.25 : 0.0);
}

// ---- global transition list, level rows, pools ------------------------------------------
void plan_atom_offsets(const lwhip_context& c, TablePlan& p, HostTables& ht)
{
    const int Ns = c.Ns;
    ht.levelOff.assign(c.Natom + 1, 0);
    ht.atomTrOff.assign(c.Natom + 1, 0);
    ht.gammaOff.assign(c.Natom, 0);
    p.gammaTot = 0;
    for (int ia = 0; ia < c.Natom; ++ia)
    {
        const lwhip_atom& a = c.atoms[ia];
        ht.levelOff[ia + 1] = ht.levelOff[ia] + a.Nlevel;
        ht.atomTrOff[ia + 1] = ht.atomTrOff[ia] + a.Ntrans;
        ht.gammaOff[ia] = p.gammaTot;
        if (!a.detailed)
            p.gammaTot += (int64_t)a.Nlevel * a.Nlevel * Ns;
    }
    p.NlevTot = ht.levelOff[c.Natom];
    p.Ntrans = ht.atomTrOff[c.Natom];
}

// ---- hybrid PRD: the tables of configure_hprd_coeffs (lwhip_options.hprd), checked and laid out for the device ------------
int plan_hybrid_prd(const lwhip_context& c, const TablePlan& p, HostTables& ht)
{
    const int Ns = c.Ns;
    ht.hLa2prdHost.clear();
    ht.hLa2hHost.clear();
    ht.hRhoOffHost.assign(p.Ntrans, -1);
    if (!c.hprd)
        return LWHIP_OK;
    const lwhip_hprd& H = *c.hprd;
    const int Nlam = c.prob.Nlambda, Nr = c.Nrays;
    // On a wavelength shard (round 4) every rank keeps rho of the WHOLE grid of each PRD line (a ray's rho is interpolated
    // between neighbouring wavelengths of the line, which may belong to another shard) and evaluates the scattering
    // integral for all of them; JRest is additive over the wavelengths (Prd.cpp:384-389), so each rank's partial sums
    // ride in the all-reduce of the PRD gather buffer (lwhip_prd_pack).
    if (c.is2d)
        return fail(LWHIP_ERR_UNSUPPORTED, "hybrid PRD: 1D contexts only");
    if (H.NprdLambda < 1 || H.Nlines < 1 || !H.prdIdxs || !H.JRest || !H.lineAtom || !H.lineTrans || !H.rhoCoeffs
        || (H.NhPrd > 0 && (!H.hPrdIdxs || !H.jCoeffOff || !H.jCoeffs)))
        return fail(LWHIP_ERR_INVALID, "hybrid PRD: incomplete lwhip_hprd");
    ht.hLa2prdHost.assign(Nlam, -1);
    ht.hLa2hHost.assign(Nlam, -1);
    for (int i = 0; i < H.NprdLambda; ++i)
    {
        if (H.prdIdxs[i] < 0 || H.prdIdxs[i] >= Nlam)
            return fail(LWHIP_ERR_INVALID, "hybrid PRD: prdIdxs out of range");
        ht.hLa2prdHost[H.prdIdxs[i]] = i;
    }
    for (int i = 0; i < H.NhPrd; ++i)
    {
        if (H.hPrdIdxs[i] < 0 || H.hPrdIdxs[i] >= Nlam)
            return fail(LWHIP_ERR_INVALID, "hybrid PRD: hPrdIdxs out of range");
        ht.hLa2hHost[H.hPrdIdxs[i]] = i;
    }
    std::vector<lwhip_rho_coeff>& rho = ht.hRho;
    for (int q = 0; q < H.Nlines; ++q)
    {
        const int ia = H.lineAtom[q], kr = H.lineTrans[q];
        if (ia < 0 || ia >= c.Natom || kr < 0 || kr >= c.atoms[ia].Ntrans || !H.rhoCoeffs[q])
            return fail(LWHIP_ERR_INVALID, "hybrid PRD: bad line list");
        const lwhip_transition& t = c.atoms[ia].trans[kr];
        if (t.type != LWHIP_LINE || !t.prd || !t.rhoPrd)
            return fail(LWHIP_ERR_INVALID, "hybrid PRD: a listed transition is not a PRD line");
        const int nlt = t.Nred - t.Nblue;
        const size_t n = (size_t)nlt * Nr * 2 * Ns;
        for (size_t i = 0; i < n; ++i)
            if (H.rhoCoeffs[q][i].i0 < 0 || H.rhoCoeffs[q][i].i1 >= nlt || H.rhoCoeffs[q][i].i0 > H.rhoCoeffs[q][i].i1)
                return fail(LWHIP_ERR_INVALID, "hybrid PRD: rho interpolation index outside the line's grid");
        ht.hRhoOffHost[ht.atomTrOff[ia] + kr] = (int64_t)rho.size();
        rho.insert(rho.end(), H.rhoCoeffs[q], H.rhoCoeffs[q] + n);
    }
    rho.resize(rho.size() + 64, lwhip_rho_coeff{ 0, 0, 0.0 }); // (a ray's last block of depths reads past its row)
    ht.hLa2h.assign(ht.hLa2hHost.begin() + c.laStart, ht.hLa2hHost.begin() + c.laEnd); // (indexed by the shard's wavelength)
    if (H.NhPrd > 0)
    {
        const size_t ncell = (size_t)H.NhPrd * Nr * 2 * Ns;
        std::vector<int64_t>& off = ht.hJOff;
        off.assign(H.jCoeffOff, H.jCoeffOff + ncell + 1);
        off.resize(off.size() + 8, off.back());
        const int64_t nj = off[ncell];
        for (int64_t e = 0; e < nj; ++e)
            if (H.jCoeffs[e].idx < 0 || H.jCoeffs[e].idx >= H.NprdLambda)
                return fail(LWHIP_ERR_INVALID, "hybrid PRD: JCoeffs row outside JRest");
        ht.hJCoef.assign(H.jCoeffs, H.jCoeffs + nj);
        ht.hJCoef.resize(ht.hJCoef.size() + 1, lwhip_j_coeff{ 0.0, 0, 0 });
    }
    ht.JRestCount = (size_t)H.NprdLambda * Ns; // (accumulated into by atomics)
    return LWHIP_OK;
}

void plan_transition_list(const lwhip_context& c, TablePlan& p, HostTables& ht)
{
    const int Ns = c.Ns;
    ht.trans.clear();
    p.Nline = p.Ncont = 0;
    p.phiTot = p.rhoTot = p.parTot = 0;
    for (int ia = 0; ia < c.Natom; ++ia)
    {
        const lwhip_atom& a = c.atoms[ia];
        for (int kr = 0; kr < a.Ntrans; ++kr)
        {
            HostTrans h;
            h.t = a.trans[kr];
            h.atom = ia;
            const int b = std::max(h.t.Nblue, c.laStart);
            const int r = std::min(h.t.Nred, c.laEnd);
            if (r > b)
            {
                h.NblueLoc = b - c.laStart;
                h.NredLoc = r - c.laStart;
                h.ltStart = b - h.t.Nblue;
            }
            else
            {
                h.NblueLoc = h.NredLoc = 0;
                h.ltStart = 0;
            }
            const int64_t nlt = h.NredLoc - h.NblueLoc;
            h.parOff = p.parTot;
            p.parTot += 4 * nlt;
            h.phiOff = h.rhoOff = -1;
            if (h.t.type == LWHIP_LINE)
            {
                h.row = p.Nline++;
                h.phiOff = p.phiTot;
                p.phiTot += nlt * c.Nrays * 2 * Ns;
                h.rhoLt0 = h.ltStart;
                h.rhoRows = (int)nlt;
                if (h.t.prd)
                {
                    if (c.hprd && ht.hRhoOffHost[ht.trans.size()] >= 0)
                    {
                        // hybrid PRD: rho of the line's whole grid on every shard
                        h.rhoLt0 = 0;
                        h.rhoRows = h.t.Nred - h.t.Nblue;
                    }
                    h.rhoOff = p.rhoTot;
                    p.rhoTot += (int64_t)h.rhoRows * Ns;
                }
            }
            else
            {
                h.row = p.Ncont++;
            }
            ht.trans.push_back(h);
        }
    }
}

// ---- per-(transition, lt) params -----------------------------------------------------------
void plan_transition_params(const TablePlan& p, HostTables& ht)
{
    std::vector<double>& par = ht.par;
    par.assign((size_t)p.parTot, 0.0);
    for (auto& h : ht.trans)
    {
        const lwhip_transition& t = h.t;
        for (int l = 0; l < h.NredLoc - h.NblueLoc; ++l)
        {
            const int lt = h.ltStart + l;
            double* q = &par[(size_t)h.parOff + 4 * l];
            const double wlambda = trans_wlambda(t, lt);
            if (t.type == LWHIP_LINE)
            {
                const double hnu_4pi = HC_4PI * (t.lambda0 / t.wavelength[lt]);
                q[0] = hnu_4pi * t.Bij;
                q[1] = wlambda;
                q[2] = t.Bji / t.Bij;
                q[3] = t.Aji / t.Bji;
            }
            else
            {
                const double wl = t.wavelength[lt];
                q[0] = t.alpha[lt];
                q[1] = (wlambda / wl) * PI4_H;
                q[2] = TWO_HC_NM3 / (wl * wl * wl);
                q[3] = 0.0;
            }
        }
    }
}

// ---- per-wavelength activity: [lines][mixed continua][pure continua], row programs --------------
int plan_wavelength_activity(const lwhip_context& c, TablePlan& p, HostTables& ht)
{
    const int Ns = c.Ns;
    const std::vector<double>& par = ht.par;
    std::vector<DevLaHeader>& hdr = ht.laHdr;
    std::vector<DevSlot>& slots = ht.slots;
    std::vector<int32_t>& slotTr = ht.slotTrD; // global transition of each slot record
    std::vector<DevProgram>& progs = ht.progs;
    std::vector<DevProgRow>& progRows = ht.progRows;
    std::vector<DevProgEnt>& progEnts = ht.progEnts;
    std::vector<int32_t>& contLaHost = ht.contLa;
    std::map<std::vector<int>, int> progIds;
    hdr.resize(c.Nla);
    p.rowsTot = 0;
    p.maxL = p.maxC = p.maxM = p.maxP = 0;
    const int rowEtaA = 2, rowLevChi = 2 + c.Natom, rowLevU = 2 + c.Natom + p.NlevTot;
    for (int la = 0; la < c.Nla; ++la)
    {
        std::vector<int> lines, conts;
        for (int tr = 0; tr < p.Ntrans; ++tr)
        {
            const HostTrans& h = ht.trans[tr];
            if (la < h.NblueLoc || la >= h.NredLoc)
                continue;
            (h.t.type == LWHIP_LINE ? lines : conts).push_back(tr);
        }
        auto isOp = [&](int tr) { return !c.atoms[ht.trans[tr].atom].detailed; };
        // moment slots: the first two active atoms that have an active line here
        std::vector<int> momentAtoms;
        for (int tr : lines)
            if (isOp(tr) && std::find(momentAtoms.begin(), momentAtoms.end(), ht.trans[tr].atom) == momentAtoms.end())
                momentAtoms.push_back(ht.trans[tr].atom);
        auto msOf = [&](int atom) {
            for (int m = 0; m < (int)momentAtoms.size() && m < 2; ++m)
                if (momentAtoms[m] == atom)
                    return m;
            return -1;
        };
        auto atomHasLines = [&](int atom) {
            return std::find(momentAtoms.begin(), momentAtoms.end(), atom) != momentAtoms.end();
        };
        std::vector<int> mixed, pure;
        for (int tr : conts)
        {
            const HostTrans& h = ht.trans[tr];
            bool isMixed = false;
            if (isOp(tr))
            {
                for (int lt : lines)
                {
                    const HostTrans& l = ht.trans[lt];
                    if (l.atom != h.atom || !isOp(lt))
                        continue;
                    if (l.t.i == h.t.i || l.t.i == h.t.j || l.t.j == h.t.i || l.t.j == h.t.j)
                        isMixed = true;
                }
                if (atomHasLines(h.atom) && msOf(h.atom) < 0)
                    isMixed = true;
            }
            (isMixed ? mixed : pure).push_back(tr);
        }
        std::vector<int> order = lines;
        order.insert(order.end(), mixed.begin(), mixed.end());
        order.insert(order.end(), pure.begin(), pure.end());
        hdr[la].off = (int32_t)slots.size();
        hdr[la].nLine = (int16_t)lines.size();
        hdr[la].nMixed = (int16_t)mixed.size();
        hdr[la].nPure = (int16_t)pure.size();
        hdr[la].hasPrd = 0;
        if (c.hprd && c.hprd->NhPrd > 0)
            hdr[la].hasPrd = ht.hLa2hHost[c.laStart + la] >= 0 ? 1 : 0; // hybrid PRD: the wavelengths that scatter into the PRD region (PrdTemplates.hpp:234-248)
        else
        for (int tr : lines)
            if (ht.trans[tr].t.prd && ht.trans[tr].rhoOff >= 0 && (isOp(tr) || c.prdDetailed))
                hdr[la].hasPrd = 1; // a wavelength the PRD rates pass visits (PrdTemplates.hpp:226-239)
        for (int tr : order)
        {
            const HostTrans& h = ht.trans[tr];
            const int l = la - h.NblueLoc;
            DevSlot sl{};
            sl.cs = 0;
            sl.gi = ht.levelOff[h.atom] + h.t.i;
            sl.gj = ht.levelOff[h.atom] + h.t.j;
            sl.atom = h.atom;
            sl.flags = (isOp(tr) ? 1 : 0) | ((h.t.type == LWHIP_LINE && h.t.prd) ? 2 : 0);
            sl.row = h.row;
            sl.ms = isOp(tr) ? msOf(h.atom) : -1;
            for (int q = 0; q < 4; ++q)
                sl.p[q] = par[(size_t)h.parOff + 4 * l + q];
            sl.phiOff = (h.t.type == LWHIP_LINE) ? h.phiOff + (int64_t)l * c.Nrays * 2 * Ns : -1;
            sl.rhoOff = (h.rhoOff >= 0) ? h.rhoOff + (int64_t)(h.ltStart - h.rhoLt0 + l) * Ns : -1;
            slots.push_back(sl);
            slotTr.push_back(tr);
        }
        {
            // position q of the reference's transition order among this wavelength's continua -> ordinal in the
            // [mixed][pure] slot order (kept in the q-th continuum record's _pad)
            std::vector<int> contOrd = mixed;
            contOrd.insert(contOrd.end(), pure.begin(), pure.end());
            std::vector<int> byTrQ(contOrd.size());
            for (size_t q = 0; q < byTrQ.size(); ++q)
                byTrQ[q] = (int)q;
            std::sort(byTrQ.begin(), byTrQ.end(), [&](int x, int y) { return contOrd[x] < contOrd[y]; });
            for (size_t q = 0; q < byTrQ.size(); ++q)
                slots[hdr[la].off + lines.size() + q]._pad = byTrQ[q];
        }
        p.maxL = std::max(p.maxL, (int)lines.size());
        p.maxC = std::max(p.maxC, (int)conts.size());
        p.maxM = std::max(p.maxM, (int)mixed.size());
        p.maxP = std::max(p.maxP, (int)pure.size());

        // row program of this wavelength's continuum set (deduplicated by signature)
        std::vector<int> contOrder = mixed;
        contOrder.insert(contOrder.end(), pure.begin(), pure.end());
        std::vector<int> rowsNeeded = { 0, 1 };
        for (int tr : order)
        {
            if (!isOp(tr))
                continue;
            const HostTrans& h = ht.trans[tr];
            const int gi = ht.levelOff[h.atom] + h.t.i, gj = ht.levelOff[h.atom] + h.t.j;
            for (int r : { rowEtaA + h.atom, rowLevChi + gi, rowLevChi + gj, rowLevU + gi, rowLevU + gj })
                if (std::find(rowsNeeded.begin(), rowsNeeded.end(), r) == rowsNeeded.end())
                    rowsNeeded.push_back(r);
        }
        std::sort(rowsNeeded.begin(), rowsNeeded.end());
        std::vector<int> key = contOrder;
        key.push_back(-1);
        key.insert(key.end(), rowsNeeded.begin(), rowsNeeded.end());
        auto it = progIds.find(key);
        if (it == progIds.end())
        {
            DevProgram pg{};
            pg.rowOff = (int32_t)progRows.size();
            pg.entOff = (int32_t)progEnts.size();
            // continua contribute in reference (transition index) order
            std::vector<int> byTr(contOrder.size());
            for (size_t q = 0; q < byTr.size(); ++q)
                byTr[q] = (int)q;
            std::sort(byTr.begin(), byTr.end(), [&](int x, int y) { return contOrder[x] < contOrder[y]; });
            for (int r : rowsNeeded)
            {
                DevProgRow pr{};
                pr.row = (int16_t)r;
                pr.entOff = (int32_t)(progEnts.size() - pg.entOff);
                for (int cq : byTr)
                {
                    const int tr = contOrder[cq];
                    const HostTrans& h = ht.trans[tr];
                    const int gi = ht.levelOff[h.atom] + h.t.i, gj = ht.levelOff[h.atom] + h.t.j;
                    const bool op = isOp(tr);
                    if (r == 0)
                        progEnts.push_back(DevProgEnt{ (int16_t)cq, 0 });
                    else if (r == 1)
                        progEnts.push_back(DevProgEnt{ (int16_t)cq, 3 });
                    else if (op && r == rowEtaA + h.atom)
                        progEnts.push_back(DevProgEnt{ (int16_t)cq, 3 });
                    else if (op && r >= rowLevChi && r < rowLevU)
                    {
                        if (r == rowLevChi + gi)
                            progEnts.push_back(DevProgEnt{ (int16_t)cq, 0 });
                        if (r == rowLevChi + gj)
                            progEnts.push_back(DevProgEnt{ (int16_t)cq, 1 });
                    }
                    else if (op && r == rowLevU + gj)
                        progEnts.push_back(DevProgEnt{ (int16_t)cq, 2 });
                }
                pr.nEnt = (int16_t)(progEnts.size() - pg.entOff - pr.entOff);
                progRows.push_back(pr);
            }
            pg.nRows = (int32_t)(progRows.size() - pg.rowOff);
            pg.nEnt = (int32_t)(progEnts.size() - pg.entOff);
            if (pg.nRows > LWHIP_MAX_PROG_ROWS || pg.nEnt > LWHIP_MAX_PROG_ENTS || progs.size() >= 32767)
                return fail(LWHIP_ERR_UNSUPPORTED, "continuum row program exceeds the kernel's LDS tables");
            it = progIds.emplace(key, (int)progs.size()).first;
            progs.push_back(pg);
        }
        hdr[la].prog = (int16_t)it->second;
        // block of this wavelength in the continuum-row buffer (march kernel): the program's rows in
        // rowsNeeded order, then Vji of each continuum
        const int nContHere = (int)contOrder.size();
        hdr[la].nRows = (int32_t)rowsNeeded.size();
        hdr[la].rowBase = -1;
        if (nContHere > 0)
        {
            hdr[la].rowBase = (int32_t)p.rowsTot;
            p.rowsTot += (int64_t)rowsNeeded.size() + nContHere;
            contLaHost.push_back(la);
        }
        auto dense = [&](int r) -> int16_t {
            if (nContHere == 0)
                return -1;
            auto f = std::find(rowsNeeded.begin(), rowsNeeded.end(), r);
            return f == rowsNeeded.end() ? (int16_t)-1 : (int16_t)(f - rowsNeeded.begin());
        };
        for (size_t e = 0; e < order.size(); ++e)
        {
            DevSlot& sl = slots[hdr[la].off + e];
            const HostTrans& htr = ht.trans[order[e]];
            const int gi = ht.levelOff[htr.atom] + htr.t.i, gj = ht.levelOff[htr.atom] + htr.t.j;
            sl.rEtaA = dense(rowEtaA + htr.atom);
            sl.rChiI = dense(rowLevChi + gi);
            sl.rChiJ = dense(rowLevChi + gj);
            sl.rUI = dense(rowLevU + gi);
            sl.rUJ = dense(rowLevU + gj);
            sl.rVji = (int16_t)((int)e >= (int)lines.size() ? (int)rowsNeeded.size() + ((int)e - (int)lines.size()) : -1);
            if (!isOp(order[e]))
                sl.rEtaA = sl.rChiI = sl.rChiJ = sl.rUI = sl.rUJ = -1;
        }
    }
    if (p.maxL > 8)
        return fail(LWHIP_ERR_UNSUPPORTED, "more than 8 lines overlap at one wavelength");
    if (c.is2d && p.maxM > 4)
        return fail(LWHIP_ERR_UNSUPPORTED, "2D: more than 4 continua coupled to the lines of one wavelength (rates2d_kernel's MAXM)");
    if (p.maxC < 1)
        p.maxC = 1;
    p.nContLa = p.rowsTot > 0 ? (int)contLaHost.size() : 0;
    if (contLaHost.empty())
        contLaHost.push_back(0); // (never an empty upload)
    return LWHIP_OK;
}

// LDS of a lane-sweep launch of this problem with `waves` wavefronts per workgroup and maxCT accumulator slots, sized where
// the launches size it (lane_sweep_lds_bytes on the members build_tile_args will set)
size_t lane_lds(const lwhip_context& c, const TablePlan& p, int waves, int maxCT, int D, int LR, int R)
{
    static double fixedOrder; // (only whether detSlab is set is read)
    TileArgs t{};
    t.maxCT = maxCT;
    t.laneD = D;
    t.laneLRD = LR * D;
    t.L = R;
    t.maxC = p.maxC;
    t.depBytes = (uint32_t)(lane_dep_arena_doubles(p.NlevTot, p.Nline, p.Ncont, (int)c.Ns, LR * D) * sizeof(double));
    t.detSlab = p.deterministic ? &fixedOrder : nullptr;
    return lane_sweep_lds_bytes(t, waves);
}
// ... and whether a workgroup can have it: the launch within a workgroup's LDS, the accumulators within their 64 KB
bool lane_fits(const lwhip_context& c, const TablePlan& p, int waves, int maxCT, int D, int LR, int R)
{
    return sizeof(double) * (size_t)maxCT * 4 * (LR * D) <= 64 * 1024 && lane_lds(c, p, waves, maxCT, D, LR, R) <= LWHIP_LDS_WORKGROUP;
}

// The pure continua of a wavelength as the lane sweep integrates them (DevPostProg): which level sums need a
// register ("shared": several contributors, or a foreign one), which are the continuum's own term or zero.
// Two encodings of the program words: the NARROW one (4 bits per field, up to LWHIP_POST_SUMS = 8 shared sums: one- and
// two-atom problems; the finish's fast forms recognise its common words) and the WIDE one (round 5: 8 / 6 bits per field,
// up to LWHIP_POST_SUMS_WIDE = 14 shared sums -- continua of up to four active atoms at one wavelength), chosen per
// tile (DevLaneTile::finFast = 2).
bool post_program(const lwhip_context& c, const TablePlan& p, const HostTables& ht, int la, DevPostProg& pg, bool* wideOut)
{
    const std::vector<DevLaHeader>& hdr = ht.laHdr;
    const std::vector<DevSlot>& slots = ht.slots;
    pg = DevPostProg{};
    if (wideOut)
        *wideOut = false;
    const DevLaHeader& h = hdr[la];
    const int base = h.off + h.nLine, nC = h.nMixed + h.nPure;
    if (nC > LWHIP_POST_MAXC)
        return false;
    // position q of the reference's transition order -> the continuum's slot record
    auto ordOf = [&](int q) { return slots[base + q]._pad; };
    auto rec = [&](int q) -> const DevSlot& { return slots[base + ordOf(q)]; };
    struct Contrib { int q, kind; };
    const int colChi = c.Natom, colU = c.Natom + p.NlevTot;
    auto contributors = [&](int col) {
        std::vector<Contrib> v;
        for (int q = 0; q < nC; ++q)
        {
            const DevSlot& sl = rec(q);
            if (!(sl.flags & 1))
                continue;
            if (col == sl.atom)
                v.push_back({ q, 4 });
            if (col == colChi + sl.gi)
                v.push_back({ q, 1 });
            if (col == colChi + sl.gj)
                v.push_back({ q, 2 });
            if (col == colU + sl.gj)
                v.push_back({ q, 3 });
        }
        return v;
    };
    // per continuum: the entry each of its four terms (+chi, -chi, U, eta) is added to (0: none, 1 .. : a shared sum), and
    // the five operands of a pure continuum (0: zero, 1 .. : a shared sum, -1 .. -4: its own +chi, -chi, U, eta)
    int target[LWHIP_POST_MAXC][4] = {};
    int operand[LWHIP_POST_MAXC][5] = {};
    std::map<int, int> sumOf;
    for (int q = 0; q < nC; ++q)
    {
        const DevSlot& sl = rec(q);
        if (ordOf(q) < h.nMixed || !(sl.flags & 1))
            continue; // mixed continua are integrated ray by ray; detailed atoms have rates only
        const int cols[5] = { sl.atom, colChi + sl.gi, colU + sl.gj, colChi + sl.gj, colU + sl.gi };
        for (int w = 0; w < 5; ++w)
        {
            const auto v = contributors(cols[w]);
            int sel = 0;
            if (v.size() == 1 && v[0].q == q)
                sel = -v[0].kind;
            else if (!v.empty())
            {
                auto it = sumOf.find(cols[w]);
                if (it == sumOf.end())
                {
                    if ((int)sumOf.size() >= LWHIP_POST_SUMS_WIDE)
                        return false;
                    const int m = (int)sumOf.size();
                    it = sumOf.emplace(cols[w], m).first;
                    for (const auto& cb : v)
                        target[cb.q][cb.kind - 1] = m + 1;
                }
                sel = it->second + 1;
            }
            operand[q][w] = sel;
        }
    }
    const bool wide = (int)sumOf.size() > LWHIP_POST_SUMS;
    if (wideOut)
        *wideOut = wide;
    for (int q = 0; q < LWHIP_POST_MAXC; ++q)
    {
        uint32_t code = 0, ops = 0;
        for (int f = 0; f < 4; ++f)
        {
            const int tg = target[q][f];
            code |= wide ? (uint32_t)(tg ? tg : 0xFF) << (8 * f) : (uint32_t)(tg ? tg : 9) << (4 * f);
        }
        for (int w = 0; w < 5; ++w)
        {
            const int sel = operand[q][w];
            // own terms: narrow 9 .. 12, wide 60 .. 63 (+chi, -chi, U, eta)
            const uint32_t field = sel >= 0 ? (uint32_t)sel : (uint32_t)((wide ? 59 : 8) - sel);
            ops |= field << ((wide ? 6 : 4) * w);
        }
        pg.code[q] = code;
        pg.ops[q] = ops;
    }
    return true;
}

// Which sweep: the lane sweep wherever its compiled kinds cover the problem (measured on MI355X:
// tools/size_sweep.sh, tools/cross_exp.sh, profiles/r03_size_sweep.md), the ray-column march otherwise.
// The depth-across-lanes sweep serves the tiles whose line / mixed-continuum counts have a compiled kind and whose
// pure continua fit its register program, where its depth arena fits a workgroup's LDS; anything else runs the
// ray-column march.  LWHIP_SWEEP=lanes|march forces one.
int choose_sweep(const lwhip_context& c, const TableKnobs& k, TablePlan& p, const HostTables& ht)
{
    const int Ns = c.Ns, Nmu = c.Nrays;
    const std::vector<DevLaHeader>& hdr = ht.laHdr;
    if (Nmu > 64 || Ns < 3)
        return fail(LWHIP_ERR_UNSUPPORTED, "the sweep needs Nrays <= 64 and Nspace >= 3");
    p.laneSweep = false;
    int D = 0, LR = 0, R = 0;
    const bool supported = lane_sweep_supported(Ns, Nmu, c.prob.formalSolver, &D, &LR, &R);
    const bool force = k.sweepLanes || c.hprd != nullptr // (hybrid PRD lives in the lane sweep)
                       || p.deterministic;              // (and so does the fixed-order reduction)
    // (End of round 3 -- one tile per wavefront, rays split over two wavefronts for small launches and for the tail of
    // large ones, fixed-register finish: the lane sweep is the faster one at every size measured, 0.076 / 0.142 /
    // 0.187 / 0.217 / 0.315 / 0.426 ms per step at 1 280 / 5 120 / 8 192 / 10 240 / 15 360 / 20 480 wavelengths against
    // the march's 0.171 / 0.205 / 0.225 / 0.223-0.234 / 0.396 / 0.457, and 20 % faster on a 512-column batch.  The
    // march serves what the lane sweep's kinds do not cover, and LWHIP_SWEEP=march.)
    const bool prefer = force || !k.sweepGiven;
    if ((c.hprd || p.deterministic || !k.sweepMarch) && k.tileGeneric == 0 && supported && prefer)
    {
        // (round 5: the choice is per TILE -- a wavelength whose lines / mixed continua have no compiled kind runs the lane
        // sweep's generic kind, lane_rays<-1, -1>: any number of lines up to 8, walked in runs of one line and one partner,
        // any mixed continua up to 8; only hybrid PRD, whose rates are formed ray by ray, is limited to the compiled kinds)
        bool ok = true;
        for (int la = 0; la < c.Nla && ok; ++la)
        {
            const DevLaHeader& h = hdr[la];
            const bool fastKind = fast_kind(h.nLine, h.nMixed);
            const bool genKind = !c.hprd && h.nLine <= 8 && h.nMixed <= 8 && k.laneGeneric != 0;
            DevPostProg pg;
            ok = (fastKind || genKind) && post_program(c, p, ht, la, pg, nullptr);
        }
        if (ok)
        {
            // Every workgroup stages the depth arena -- n, wphi, ratio of every level, line and continuum at every
            // depth -- in its LDS.  The least a launch can ask for is one wavefront with one tile, whose accumulator
            // slots are its wavelengths' transitions: a problem for which even that is more than a workgroup has runs
            // the march (H(6) + Ca II(6), 37 arena rows and 7 slots, fits at 256 points; H + three blended Ca II, 69 rows and
            // 17 slots, does not at 129: its accumulators alone are 71 808 bytes of the 65 536 they may have -- until
            // this check lwhip_create refused that problem instead of taking the march).  The wavefronts per workgroup
            // are chosen below by the same functions.
            int slotsLa = 1;
            for (int la = 0; la < c.Nla; ++la)
                slotsLa = std::max(slotsLa, (int)hdr[la].nLine + (int)hdr[la].nMixed + (int)hdr[la].nPure);
            ok = lane_fits(c, p, 1, slotsLa, D, LR, R);
        }
        if (ok)
        {
            p.laneSweep = true;
            p.laneD = D;
            p.laneLR = LR;
            p.laneR = R;
        }
    }
    if (c.hprd && !p.laneSweep)
        return fail(LWHIP_ERR_UNSUPPORTED, "hybrid PRD needs the depth-across-lanes sweep (1D, 13 <= Nspace <= 256, at most "
                                           "two lines or a line and a mixed continuum per wavelength, its depth arena within "
                                           "a workgroup's LDS)");
    return LWHIP_OK;
}

// ---- tiles of the ray-column sweep (lwhip_raymarch.hip) -----------------------------------------------------
// A tile = up to L consecutive wavelengths with the same slot records (same transitions in the same order, same
// row program): one wavefront marches it, lane = (mu, wavelength).
int plan_tiles(const lwhip_context& c, const TableKnobs& k, int numCU, TablePlan& p, HostTables& ht)
{
    const int Ns = c.Ns, Nmu = c.Nrays;
    const int rowEtaA = 2, rowLevChi = 2 + c.Natom, rowLevU = 2 + c.Natom + p.NlevTot;
    const std::vector<DevLaHeader>& hdr = ht.laHdr;
    const std::vector<DevSlot>& slots = ht.slots;
    const std::vector<int32_t>& slotTr = ht.slotTrD;
    std::vector<DevTile>& tiles = ht.tiles;
    std::vector<DevTileSlot>& tslots = ht.tslots;
    std::vector<DevTileCopy>& tcopies = ht.tcopies;
    std::vector<int32_t>& tileRemap = ht.tileRemap;
    const int L = p.laneSweep ? p.laneR : std::max(1, std::min({ 16, 64 / Nmu, k.tileL }));
    const int LRD = p.laneLR * p.laneD;
    p.tileL = L;
    auto pad16 = [](int64_t v) { return (v + 15) / 16 * 16; };
    auto same_structure = [&](int la, int lb) {
        const DevLaHeader &a = hdr[la], &b = hdr[lb];
        if (a.nLine != b.nLine || a.nMixed != b.nMixed || a.nPure != b.nPure || a.prog != b.prog || a.hasPrd != b.hasPrd)
            return false;
        const int n = a.nLine + a.nMixed + a.nPure;
        for (int e = 0; e < n; ++e)
            if (slotTr[a.off + e] != slotTr[b.off + e])
                return false;
        return true;
    };
    p.rowsTileTot = p.momTot = p.phiTTot = 0;
    p.preCols = 0;
    p.maxSlotsTile = 0;
    p.tileCap = k.tileGeneric; // > 0: every tile through the guarded generic march (test hook)
    // (march, one problem: the launch is one round of workgroups -- one per tile, four per CU -- and lasts as long as its
    // slowest one, march + post-pass.  The tiles with two slots march longest; capping their wavelengths shortens their
    // post-pass, as long as the extra tiles still fit the round: measured 0.196 -> 0.184 ms at 10 240 wavelengths with 10
    // instead of 12, nothing beyond ~0.9 of the slots -- profiles/r03_march_bounds.md)
    auto count_tiles = [&](int capHeavy) {
        int n = 0;
        for (int la = 0; la < c.Nla; ++n)
        {
            const DevLaHeader& h = hdr[la];
            const int Lk = std::min(L, h.nLine + h.nMixed >= 2 ? capHeavy : L);
            int nl = 1;
            while (nl < Lk && la + nl < c.Nla && same_structure(la, la + nl))
                ++nl;
            la += nl;
        }
        return n;
    };
    int autoHeavy = L;
    if (!p.laneSweep && c.batchHint <= 1 && L >= 6)
    {
        const int wfSlots = 4 * numCU; // workgroups of two wavefronts at two wavefronts per SIMD
        for (int cap = L - 1; cap >= L - L / 6; --cap)
            if (count_tiles(cap) * 100 <= wfSlots * 91)
                autoHeavy = cap;
    }
    const int tileLHeavy = std::max(1, k.tileLH.value_or(autoHeavy)), tileLOne = std::max(1, k.tileL1.value_or(L));
    for (int la = 0; la < c.Nla;)
    {
        const DevLaHeader& h = hdr[la];
        // (march: a workgroup lasts its tile's march + post-pass, and the launch as long as its slowest workgroup: tiles
        // whose march is long -- two slots -- take fewer wavelengths, so that their post-pass is shorter)
        const int Lk = p.laneSweep ? L : std::min(L, h.nLine + h.nMixed >= 2 ? tileLHeavy : h.nLine + h.nMixed == 1 ? tileLOne : L);
        int nl = 1;
        while (nl < Lk && la + nl < c.Nla && same_structure(la, la + nl))
            ++nl;
        DevTile td{};
        td.la0 = la;
        td.nl = (int16_t)nl;
        td.nLine = h.nLine;
        td.nMixed = h.nMixed;
        td.hasPrd = (int16_t)h.hasPrd;
        td.slotOff = (int32_t)tslots.size();
        td.copyOff = (int32_t)tcopies.size();
        int nRowsT = 3;
        // the five continuum rows of an active slot (eta_A, chi_i, chi_j, U_i, U_j) are consecutive tile rows,
        // zero-filled where the wavelength has no such term: the march loads them unconditionally
        // which of a slot's five level sums no continuum of this wavelength feeds (the lane sweep does not read them)
        auto zero_mask = [&](const DevSlot& sl) -> int16_t {
            bool fed[5] = { false, false, false, false, false };
            for (int e = h.nLine; e < h.nLine + h.nMixed + h.nPure; ++e)
            {
                const DevSlot& cs = slots[h.off + e];
                if (!(cs.flags & 1))
                    continue;
                fed[0] |= cs.atom == sl.atom;
                fed[1] |= cs.gi == sl.gi || cs.gj == sl.gi;
                fed[2] |= cs.gi == sl.gj || cs.gj == sl.gj;
                fed[3] |= cs.gj == sl.gi;
                fed[4] |= cs.gj == sl.gj;
            }
            int16_t zm = 0;
            for (int q = 0; q < 5; ++q)
                zm |= fed[q] ? 0 : (int16_t)(1 << q);
            return zm;
        };
        auto five_rows = [&](const DevSlot& sl) -> int16_t {
            const int16_t r0 = (int16_t)nRowsT;
            // row ids as the row programs number them (the pre-pass forms the level sums directly)
            // (lane sweep: a row that no continuum of the wavelength feeds is never read -- its zero-mask bit -- and stays
            // the zero the allocation was cleared to: the pre-pass does not write it)
            const int16_t zmS = p.laneSweep ? zero_mask(sl) : (int16_t)0;
            int qi = 0;
            for (int id : { rowEtaA + sl.atom, rowLevChi + sl.gi, rowLevChi + sl.gj, rowLevU + sl.gi, rowLevU + sl.gj })
            {
                if (zmS & (1 << qi++))
                {
                    ++nRowsT;
                    continue;
                }
                if (h.nMixed + h.nPure > 0)
                    tcopies.push_back(DevTileCopy{ 0, (int16_t)id, (int16_t)nRowsT, 0 });
                else
                    tcopies.push_back(DevTileCopy{ 3, 0, (int16_t)nRowsT, 0 });
                ++nRowsT;
            }
            return r0;
        };
        for (int e = 0; e < h.nLine + h.nMixed; ++e)
        {
            const DevSlot& sl = slots[h.off + e];
            DevTileSlot ts{};
            ts.tr = slotTr[h.off + e];
            ts.cs = 0;
            ts.gi = sl.gi;
            ts.gj = sl.gj;
            ts.atom = sl.atom;
            ts.flags = sl.flags;
            ts.row = sl.row;
            ts.ms = sl.ms;
            ts.r0 = (sl.flags & 1) ? five_rows(sl) : (int16_t)0;
            ts.zmask = (sl.flags & 1) ? zero_mask(sl) : (int16_t)31;
            ts.rAux = -1;
            ts.e = (int16_t)e;
            ts.phiOff = -1;
            ts.rhoOff = sl.rhoOff;
            ts.hCoefOff = -1;
            if (c.hprd && e < h.nLine && ht.hRhoOffHost[slotTr[h.off + e]] >= 0)
            {
                // hybrid PRD: the coefficient block of the tile's first wavelength, and the line's first rho row
                const HostTrans& htr = ht.trans[slotTr[h.off + e]];
                const int64_t lt0 = htr.ltStart + la - htr.NblueLoc; // (the coefficient table covers the line's whole grid)
                ts.hCoefOff = ht.hRhoOffHost[slotTr[h.off + e]] + lt0 * c.Nrays * 2 * Ns;
                ts.rhoOff = htr.rhoOff; // row 0 of the line
            }
            if (e < h.nLine && p.laneSweep)
                ts.phiOff = sl.phiOff; // the profiles are read where they lie
            else if (e < h.nLine)
            {
                ts.phiOff = p.phiTTot;
                p.phiTTot += (int64_t)2 * Ns * 64;
            }
            if (e < h.nLine)
            {
                if ((sl.flags & 2) && !p.laneSweep) // (the lane sweep reads rho where it lies)
                {
                    ts.rAux = (int16_t)nRowsT;
                    tcopies.push_back(DevTileCopy{ 2, (int16_t)e, (int16_t)nRowsT++, 0 });
                }
            }
            else
            {
                ts.rAux = (int16_t)nRowsT;
                tcopies.push_back(DevTileCopy{ 1, (int16_t)(e - h.nLine), (int16_t)nRowsT++, 0 });
            }
            tslots.push_back(ts);
            if (!fast_kind(h.nLine, h.nMixed))
                p.tileCap = std::max(p.tileCap, std::max((int)h.nLine, (int)h.nMixed));
        }
        td.nCopy = (int32_t)tcopies.size() - td.copyOff;
        {
            // distinct level-sum columns this tile's rows are copied from (the pre-pass sizes its LDS columns by the max)
            std::vector<int16_t> srcs;
            for (int q = td.copyOff; q < (int)tcopies.size(); ++q)
                if (tcopies[q].kind == 0 && std::find(srcs.begin(), srcs.end(), tcopies[q].src) == srcs.end())
                    srcs.push_back(tcopies[q].src);
            p.preCols = std::max(p.preCols, (int)srcs.size());
            // ... and where each dense level-sum slot lives among them (what the pre-pass's workgroups used to
            // work out for themselves, one thread walking the copy list while 127 waited)
            const int nLev = c.Natom + 2 * p.NlevTot;
            const size_t base = tileRemap.size();
            tileRemap.resize(base + nLev + 1, (int32_t)srcs.size());
            for (size_t q = 0; q < srcs.size(); ++q)
                if (srcs[q] >= 2 && srcs[q] - 2 < nLev)
                    tileRemap[base + (srcs[q] - 2)] = (int32_t)q;
        }
        td.nRowsT = nRowsT;
        td.rowBase = p.rowsTileTot;
        td.momBase = p.momTot;
        if (p.laneSweep)
            p.rowsTileTot += (int64_t)nRowsT * L * LRD; // [row][wavelength][k]
        else
        {
            p.rowsTileTot += (int64_t)nRowsT * Ns * 16; // rows of 16 doubles whatever L (RM_ROW)
            p.momTot += pad16((int64_t)8 * Ns * L);      // [direction][J, M1, Meta0, Meta1][Ns][L]
        }
        p.maxSlotsTile = std::max(p.maxSlotsTile, h.nLine + h.nMixed);
        tiles.push_back(td);
        la += nl;
    }
    p.nTiles = (int)tiles.size();
    if (k.verbose)
    {
        std::map<std::pair<int, int>, std::pair<int, int>> hist;
        for (auto& td : tiles)
        {
            auto& hh = hist[{ td.nLine, td.nMixed }];
            hh.first++;
            hh.second += td.nl;
        }
        for (auto& kv : hist)
            std::fprintf(stderr, "  tiles with %d lines + %d mixed continua: %d (%d wavelengths)\n", kv.first.first, kv.first.second,
                         kv.second.first, kv.second.second);
    }
    for (auto& td : tiles)
        if (td.nLine > 8 || td.nMixed > 8)
            return fail(LWHIP_ERR_UNSUPPORTED, "more than 8 lines (or 8 continua coupled to them) overlap at one wavelength");
    return LWHIP_OK;
}

// ---- workgroups of the sweep: contiguous, cost-balanced runs of tiles; the waves of a workgroup take its tiles in turn ----
struct TileChunking
{
    std::vector<int32_t> chunkTile, slotTr;
    std::vector<int> cs;     // per tile slot (mode 0, 2) or per wavelength slot record (mode 1)
    std::vector<int> csPure; // mode 2: per wavelength slot record, the pure continua
    int maxCT = 1;
};
// mode 0: accumulator slots for the tiles' lines and mixed continua; 1: for the pure continua (post-pass chunks);
// 2: for both (the lane sweep's workgroups finish their tiles themselves)
// fixedCount > 0: every chunk holds that many tiles (lane sweep: one per group of wavefronts -- a workgroup's rounds
// are what a launch of one partial round lasts)
TileChunking chunk_tiles(const HostTables& ht, int Ntrans, const std::vector<int32_t>& list, int tgt, int mode, int fixedCount = 0,
                         const std::vector<int32_t>* bounds = nullptr)
{
    const std::vector<DevLaHeader>& hdr = ht.laHdr;
    const std::vector<DevSlot>& slots = ht.slots;
    const std::vector<int32_t>& slotTr = ht.slotTrD;
    const std::vector<DevTile>& tiles = ht.tiles;
    const std::vector<DevTileSlot>& tslots = ht.tslots;
    auto tile_cost = [](const DevTile& td) { return 1.0 + 0.35 * (td.nLine + td.nMixed); };
    const bool pure = mode == 1;
    TileChunking ck;
    const int n = (int)list.size();
    tgt = std::max(1, std::min(tgt, n));
    if (fixedCount > 0)
        tgt = (n + fixedCount - 1) / fixedCount;
    double total = 0.0;
    for (int ti : list)
        total += tile_cost(tiles[ti]);
    ck.chunkTile.push_back(0);
    double acc = 0.0;
    int made = 0;
    if (bounds) // the chunks are given ([0, ..., n])
        ck.chunkTile.assign(bounds->begin(), bounds->end() - 1);
    for (int i = 0; i < n && !bounds; ++i)
    {
        acc += tile_cost(tiles[list[i]]);
        const int remaining = n - (i + 1), remainingChunks = tgt - (made + 1);
        const bool cut = fixedCount > 0 ? (i + 1) % fixedCount == 0 : (tgt >= n || acc >= total * (made + 1) / tgt || remaining <= remainingChunks);
        if (cut && i + 1 < n && made + 1 < tgt)
        {
            ck.chunkTile.push_back(i + 1);
            ++made;
        }
    }
    ck.chunkTile.push_back(n);
    const int nch = (int)ck.chunkTile.size() - 1;
    std::vector<std::vector<int>> chunkTrans(nch);
    ck.cs.assign(pure ? slots.size() : tslots.size(), 0);
    if (mode == 2)
        ck.csPure.assign(slots.size(), 0);
    for (int ch = 0; ch < nch; ++ch)
    {
        std::vector<int> slotOf(Ntrans, -1);
        auto slot_for = [&](int tr) {
            if (slotOf[tr] < 0)
            {
                slotOf[tr] = (int)chunkTrans[ch].size();
                chunkTrans[ch].push_back(tr);
            }
            return slotOf[tr];
        };
        for (int i = ck.chunkTile[ch]; i < ck.chunkTile[ch + 1]; ++i)
        {
            const DevTile& td = tiles[list[i]];
            if (!pure)
                for (int e = 0; e < td.nLine + td.nMixed; ++e)
                    ck.cs[td.slotOff + e] = slot_for(tslots[td.slotOff + e].tr);
            if (mode != 0)
                for (int q = 0; q < td.nl; ++q)
                {
                    const DevLaHeader& h = hdr[td.la0 + q];
                    for (int e = h.nLine + h.nMixed; e < h.nLine + h.nMixed + h.nPure; ++e)
                        (mode == 2 ? ck.csPure : ck.cs)[h.off + e] = slot_for(slotTr[h.off + e]);
                }
        }
        ck.maxCT = std::max(ck.maxCT, (int)chunkTrans[ch].size());
    }
    ck.slotTr.assign((size_t)nch * ck.maxCT, -1);
    for (int ch = 0; ch < nch; ++ch)
        for (size_t q = 0; q < chunkTrans[ch].size(); ++q)
            ck.slotTr[(size_t)ch * ck.maxCT + q] = chunkTrans[ch][q];
    return ck;
}

// The wavefronts of a workgroup of the lane sweep: halved while the launch asks for more LDS than a workgroup has -- the per-wavefront
// blocks shrink, and so do the accumulator slots, one per transition of the workgroup's tiles.  Counted for whole
// tiles (W per workgroup): the groups of a ray split are parts of those.  H(6) + Ca II(6) with seven slots: four
// wavefronts are 138 656 bytes at 200 points, 162 944 at 244, 164 264 at 245 and 168 680 at 253, where two are
// 154 776.  (Until this check every launch of such a context failed at hipFuncSetAttribute.)  One wavefront fits:
// the sweep was chosen so.
void choose_tile_waves(const lwhip_context& c, const TableKnobs& k, TablePlan& p, const HostTables& ht, const std::vector<int32_t>& all)
{
    p.tileWaves = std::max(1, std::min(8, p.laneSweep ? k.lWaves : k.tWaves));
    // (fixed-order mode: since round 5 with the default's four wavefronts per workgroup -- they add to the workgroup's
    // accumulators in turn, lwhip_lanesweep.hip ls_turn_wait; hybrid PRD adds ray by ray and keeps round 3's form, one
    // wavefront per workgroup, whose LDS sums are formed in program order)
    if (p.laneSweep && p.deterministic && c.hprd)
        p.tileWaves = 1;
    if (!p.laneSweep)
    {
        p.deterministic = false; // (not served by the ray-column march: the flag is ignored there)
        return;
    }
    auto slots_of = [&](const std::vector<int32_t>& list, int mode, int perWg) {
        return list.empty() ? 1 : chunk_tiles(ht, p.Ntrans, list, 0, mode, perWg).maxCT;
    };
    while (p.tileWaves > 1
           && !lane_fits(c, p, p.tileWaves, std::max(slots_of(all, 2, p.tileWaves), slots_of(ht.tileListPrd, 0, p.tileWaves)), p.laneD,
                         p.laneLR, p.laneR))
        p.tileWaves /= 2;
}

// Lane sweep: the wavefronts a tile's rays are split over, in the main sweep and in the PRD rates pass
void choose_lane_split(const lwhip_context& c, const TableKnobs& k, int numCU, TablePlan& p, const HostTables& ht)
{
    const int W = p.tileWaves;
    const std::vector<int32_t>& tileListPrd = ht.tileListPrd;
    // Small problems: the launch is ONE partial round of tasks and lasts as long as its longest task (a tile with two
    // slots: ~0.13 ms alone).  While S wavefronts per tile still fit the round, a tile's rays are split over the S
    // wavefronts of a group (each finishes 1/S of the tile's points): shorter tasks, same round.
    if ((!p.deterministic || !c.hprd) && c.batchHint <= 1 && W == 4)
    {
        const long wfSlots = 2L * 4 * numCU;
        // (measured, tools/split_exp.sh: S = 2 wins while it fits.  S = 4 while IT fits: in round 3 it had the same kernel
        // time at 1 280 wavelengths and a longer step -- four times the workgroups flushing their sums --; with the
        // round-4 kernel (moments, own pre-pass) it is 0.048 against 0.059 ms there, the step 0.059 against 0.074)
        // (a launch that S = 4 fills to the brim -- 1 536 wavelengths, 2 048 wavefronts -- is no faster than with S = 2)
        p.laneSplit = 4L * p.nTiles <= wfSlots * 9 / 10 ? 4 : 2L * p.nTiles <= wfSlots ? 2 : 1;
        const int forced = k.laneSplit;
        if (forced == 1 || forced == 2 || forced == 4)
            p.laneSplit = forced;
    }
    p.laneSplitPrd = p.laneSplit;
    if ((!p.deterministic || !c.hprd) && c.batchHint <= 1 && W == 4 && !tileListPrd.empty() && k.laneSplit == 0)
    {
        // (the PRD rates pass -- every ray forms its line's rates -- gains from S = 4 up to one and a half rounds of
        // wavefronts: 738 tiles, 2 952 wavefronts on 2 048 slots, 0.118 ms per sub-iteration against 0.123 with S = 2)
        const long wfSlots = 2L * 4 * numCU, nT = (long)tileListPrd.size();
        p.laneSplitPrd = 4L * nT <= wfSlots * 3 / 2 ? 4 : 2L * nT <= wfSlots ? 2 : 1;
    }
}

// Lane sweep, more workgroups than the chip holds at once (one problem, 2 workgroups of 4 wavefronts per CU): the
// launch ends with workgroups that started late and have the chip to themselves -- whole tiles of 0.1 ms.  The
// chunks that are dispatched last (the lightest: heaviest go first) are cut into smaller ones whose tiles' rays are
// split over 2 or 4 wavefronts: the same work in shorter pieces, so the tail drains evenly.
// Fills chunkSplit (per chunk: the split factor) and chunkOrder (the dispatch order) where it cuts.
void cut_tail_chunks(const lwhip_context& c, const TableKnobs& k, int numCU, const TablePlan& p, int laneFixed, const std::vector<int32_t>& all,
                     TileChunking& sw, HostTables& ht)
{
    const int W = p.tileWaves;
    const std::vector<DevTile>& tiles = ht.tiles;
    const int slotsWg = 2 * numCU;
    const int nch0 = (int)sw.chunkTile.size() - 1;
    const int tailS = 2; // (the cut chunks' tiles have their rays split over two wavefronts; four measured worse, DESIGN 3.1b vi)
    // (and in a launch of ONE partial round -- more than half a round of whole tiles, so that not every tile can be
    // split -- the heaviest chunks are the ones cut, as many as still fit the round: the launch lasts as long as its
    // longest workgroup)
    const bool oneRound = nch0 <= slotsWg;
    if (!(p.laneSweep && c.batchHint <= 1 && W == 4 && p.laneSplit == 1 && laneFixed == W
          && (nch0 > slotsWg || (oneRound && nch0 > slotsWg / 2)) && (tailS == 2 || tailS == 4)))
        return;
    std::vector<double> cost(nch0, 0.0);
    for (int ch = 0; ch < nch0; ++ch)
        for (int i = sw.chunkTile[ch]; i < sw.chunkTile[ch + 1]; ++i)
            cost[ch] += task_cost(tiles[i]);
    std::vector<int32_t> ord(nch0);
    for (int ch = 0; ch < nch0; ++ch)
        ord[ch] = ch;
    std::stable_sort(ord.begin(), ord.end(), [&](int32_t x, int32_t y) { return cost[x] > cost[y]; });
    std::vector<char> cut(nch0, 0);
    if (nch0 > slotsWg)
    {
        // the first `keep` chunks of the cost order stay whole, the lightest numCU / 2 are cut in two: one pair of
        // half-length workgroups per compute unit to even out the end of the launch.  (Until late in round 4 the rule
        // was "as many as fill the last round of slots exactly", whole + 2 cut = rounds x slots; a sweep over sizes
        // and counts -- tools/keep_rule_exp.sh, profiles/r04_tail_rule.md -- showed a spiky landscape in which that
        // was rarely the minimum: cutting 128 chunks is 3-9 % faster at 6 656 ... 12 288 wavelengths, 3 % at the bench
        // size, 3 % slower at 11 264.)
        // (... and where the last round has room for fewer pairs than that but for some -- 11 264: 85 -- only as many)
        const int rounds = (nch0 + slotsWg - 1) / slotsWg;
        const int room = rounds * slotsWg - nch0;
        int nCut = std::max(1, numCU / 2);
        nCut = std::max(0, k.laneCut.value_or(nCut)); // (experiments: chunks of the tail cut in two)
        if (room >= numCU / 8 && room < nCut)
            nCut = room;
        const int keepAuto = std::max(0, nch0 - nCut);
        const int keep = std::min(nch0, std::max(0, keepAuto));
        for (int q = keep; q < nch0; ++q)
            cut[ord[q]] = 1;
    }
    else
    {
        // one partial round: a cut chunk becomes tailS / 1 workgroups; the heaviest first, while they fit.
        // A round that is (nearly) full does not run as one: the dispatcher does not co-schedule every workgroup
        // (6 144 wavelengths = 512 chunks on 512 slots took two task lengths, 0.115 ms) -- then EVERY chunk is cut
        // and the launch is two rounds of half-length tasks
        const int extra = tailS - 1;
        const int fullPct = 85; // (profiles/r04_tail_rule.md)
        int k = std::min(nch0, std::max(0, (slotsWg - nch0) / extra));
        if (tailS == 2 && nch0 * 100 > slotsWg * fullPct)
            k = nch0;
        for (int q = 0; q < k; ++q)
            cut[ord[q]] = 1;
    }
    const int piece = W / tailS; // tiles per piece
    std::vector<int32_t> bounds, split, firstNew(nch0, 0), nNew(nch0, 0);
    bounds.push_back(0);
    for (int ch = 0; ch < nch0; ++ch)
    {
        firstNew[ch] = (int)bounds.size() - 1;
        const int b0 = sw.chunkTile[ch], b1 = sw.chunkTile[ch + 1];
        if (!cut[ch])
        {
            bounds.push_back(b1);
            split.push_back(1);
        }
        else
            for (int b = b0; b < b1; b += piece)
            {
                bounds.push_back(std::min(b + piece, b1));
                split.push_back(tailS);
            }
        nNew[ch] = (int)bounds.size() - 1 - firstNew[ch];
    }
    sw = chunk_tiles(ht, p.Ntrans, all, 0, 2, 0, &bounds);
    ht.chunkSplit = split;
    for (int q = 0; q < nch0; ++q)
        for (int e = 0; e < nNew[ord[q]]; ++e)
            ht.chunkOrder.push_back(firstNew[ord[q]] + e);
}

// LDS of the march's launches, sized where the launches size it (raymarch_lds_bytes, tile_post_lds_bytes)
TileArgs march_args(const lwhip_context& c, const TablePlan& p, int S)
{
    TileArgs t{};
    t.Ns = c.Ns;
    t.maxCT = p.maxCTTile;
    t.Natom = c.Natom;
    t.NlevTot = p.NlevTot;
    t.depthSplit = S;
    return t;
}

// Deep columns on the march (round 6): a wavefront's march is ~1.6 us per depth point whatever the number of wavelengths,
// so a launch of few tiles over many depth points -- the reference benchmark's 500-point FAL-C: 242 tiles -- leaves most of
// the chip idle for 0.8 ms.  While 2 S wavefronts per tile still fit the chip's two-per-SIMD, a direction's depth points
// are split over S wavefronts of the tile's workgroup (lwhip_raymarch.hip: raymarch_split_kernel, depthSplit).
// LWHIP_DEPTH_SPLIT=1|2|4 (LWHIP_DEBUG) forces it.
// The split launch runs its post-pass on all 128 S threads, each with its level columns in LDS: S is kept only where
// that launch (2 S wavefronts, fused: what run_sweep launches) fits the LDS of a workgroup -- known only now that the
// chunking has fixed maxCTTile.  H(6) + Ca II(6) at 500 points, three slots: 154 624 of 163 840 bytes; a third active
// atom or a fourth slot there is over, and runs unsplit.
void choose_depth_split(const lwhip_context& c, const TableKnobs& k, int numCU, TablePlan& p)
{
    const int Ns = c.Ns;
    p.depthSplit = 1;
    if (p.laneSweep || !p.tileFuse || p.tileCap != 0 || c.batchHint > 1 || p.deterministic)
        return;
    const long wfSlots = 2L * 4 * numCU; // wavefronts the chip holds at the march's two per SIMD
    // (measured at 500 points x 2 908 wavelengths, 242 tiles: S = 1 0.804 ms, S = 2 1.088, S = 4 0.652 per sweep -- every
    // later segment walks its points twice, so the split turns a latency-bound launch (a quarter of the SIMDs busy) into
    // a throughput-bound one with twice the instructions: a gain only where the unsplit launch leaves most of the chip
    // idle and four-way; S = 2 is kept for the tests)
    // (the reference benchmark's grid is 281 tiles = 2 248 wavefronts four-way: 1.10 x the slots, 0.65 against 0.80 ms per sweep)
    auto fits = [&](int S) { return Ns >= 64 * S && raymarch_lds_bytes(march_args(c, p, S), 2 * S, true) <= LWHIP_LDS_WORKGROUP; };
    const int forced = k.depthSplit;
    if (forced == -1)
    {
        // (four-way or not at all: two-way is the measured loss above)
        if (Ns >= 256 && 8L * p.nTiles <= wfSlots * 3 / 2 && fits(4))
            p.depthSplit = 4;
    }
    else if (forced == 2 || forced == 4)
    {
        // a forced value is reduced to the largest one that fits: forcing never produces a launch that fails
        int S = forced;
        while (S > 1 && !fits(S))
            S /= 2;
        p.depthSplit = S;
    }
}

void widen(TileChunking& ck, int maxCT)
{
    if (ck.maxCT == maxCT)
        return;
    const int nch = (int)ck.chunkTile.size() - 1;
    std::vector<int32_t> w((size_t)nch * maxCT, -1);
    for (int ch = 0; ch < nch; ++ch)
        for (int q = 0; q < ck.maxCT; ++q)
            w[(size_t)ch * maxCT + q] = ck.slotTr[(size_t)ch * ck.maxCT + q];
    ck.slotTr.swap(w);
    ck.maxCT = maxCT;
}

// Fixed-order mode, per transition: the (workgroup, slot) pairs that hold its sums, in workgroup order
void det_lists(int Ntrans, int maxCT, const std::vector<int32_t>& slotTrTab, int nch, std::vector<int32_t>& off, std::vector<int32_t>& ent)
{
    std::vector<std::vector<int32_t>> per(Ntrans);
    for (int ch = 0; ch < nch; ++ch)
        for (int q = 0; q < maxCT; ++q)
        {
            const int tr = slotTrTab[(size_t)ch * maxCT + q];
            if (tr >= 0)
                per[tr].push_back(ch * maxCT + q);
        }
    off.assign(1, 0);
    ent.clear();
    for (int tr = 0; tr < Ntrans; ++tr)
    {
        ent.insert(ent.end(), per[tr].begin(), per[tr].end());
        off.push_back((int32_t)ent.size());
    }
    if (ent.empty())
        ent.push_back(0);
}

// LDS of the launches this context will make.  Unsplit (the iteration where the split is off, its PRD rates pass,
// formal_sol, a column batch; W wavefronts, the post-pass fused or a launch of its own): refused beyond the project's
// margin.  The split sweep was chosen above to fit the workgroup.  An accepted context never fails at launch for LDS.
int check_launch_lds(const lwhip_context& c, const TablePlan& p)
{
    const int W = p.tileWaves;
    if (!p.laneSweep)
    {
        const TileArgs t1 = march_args(c, p, 1);
        const size_t ldsUnsplit = std::max(raymarch_lds_bytes(t1, W, p.tileFuse), raymarch_lds_bytes(t1, W, false));
        const size_t ldsPost = p.tileFuse ? 0 : tile_post_lds_bytes(t1);
        const size_t ldsSplit = p.depthSplit > 1 ? raymarch_lds_bytes(march_args(c, p, p.depthSplit), 2 * p.depthSplit, true) : 0;
        if (ldsUnsplit > LWHIP_LDS_BUDGET || ldsPost > LWHIP_LDS_BUDGET || ldsSplit > LWHIP_LDS_WORKGROUP)
            return fail(LWHIP_ERR_UNSUPPORTED, "problem does not fit the 160 KB LDS budget of one workgroup");
    }
    if (p.laneSweep && sizeof(double) * (size_t)p.maxCTTile * 4 * (p.laneLR * p.laneD) > 64 * 1024)
        return fail(LWHIP_ERR_UNSUPPORTED, "more transitions per workgroup than the lane sweep's LDS accumulators hold");
    if (p.laneSweep && lane_lds(c, p, W, p.maxCTTile, p.laneD, p.laneLR, p.laneR) > LWHIP_LDS_WORKGROUP)
        return fail(LWHIP_ERR_UNSUPPORTED, "the lane sweep of this problem does not fit the 160 KB LDS of one workgroup");
    return LWHIP_OK;
}

// Chunking, work distribution and depth split of both sweeps, each LDS rule beside the choice it constrains
int plan_chunks(const lwhip_context& c, const TableKnobs& k, int numCU, TablePlan& p, HostTables& ht)
{
    const int Ns = c.Ns;
    const std::vector<DevSlot>& slots = ht.slots;
    const std::vector<DevTile>& tiles = ht.tiles;
    std::vector<DevTileSlot>& tslots = ht.tslots;
    std::vector<int32_t>& tileListPrd = ht.tileListPrd;
    std::vector<int32_t> all(p.nTiles);
    for (int i = 0; i < p.nTiles; ++i)
    {
        all[i] = i;
        if (tiles[i].hasPrd)
            tileListPrd.push_back(i);
    }
    choose_tile_waves(c, k, p, ht, all);
    const int W = p.tileWaves;
    int wgPerCU = std::max(1, 8 / W);
    if (c.batchHint > 1)
        wgPerCU = 1;
    // (dispatching the lane sweep's long tasks -- tiles with more slots -- first was measured and is WORSE: 0.288 against
    // 0.204 ms at 10 240 wavelengths; co-resident long tasks slow each other down)
    int tgtSweep = std::min((2 * p.nTiles + W - 1) / W, numCU * wgPerCU); // two tasks per tile (down, up)
    // fused post-pass: the workgroup is the two wavefronts of one tile (and every tile is a workgroup)
    // (column batches too: 12.3k -> 16.0k column-iterations/s at 128 columns against a separate post launch)
    p.tileFuse = W == 2 && k.tileFuse != 0 && !p.laneSweep;
    if (c.batchHint > 1 && !p.tileFuse)
        tgtSweep = std::max(1, std::min(tgtSweep, numCU * 4 / c.batchHint));
    if (p.tileFuse)
        tgtSweep = p.nTiles;
    if (!p.tileFuse)
        tgtSweep = std::max(1, tgtSweep);
    p.laneSplit = 1;
    if (p.laneSweep)
    {
        choose_lane_split(c, k, numCU, p, ht);
        tgtSweep = (p.nTiles * p.laneSplit + W - 1) / W; // one tile per group of wavefronts
    }
    // post-pass workgroups: one resident set (LDS: accumulators + the threads' level columns; 8 waves per CU by registers)
    const size_t ldsPostEst = sizeof(double) * ((size_t)7 * 4 * Ns + (size_t)(c.Natom + 2 * p.NlevTot) * 128);
    const int postPerCU = (int)std::max<size_t>(1, std::min<size_t>(4, (size_t)(150 * 1024) / ldsPostEst));
    int tgtPost = std::min(p.nTiles, numCU * postPerCU);
    if (c.batchHint > 1)
        tgtPost = std::max(1, std::min(tgtPost, numCU * 8 / c.batchHint));
    const int laneFixed = p.laneSweep ? std::max(1, W / p.laneSplit) : 0; // (one tile per group of wavefronts)
    TileChunking sw = chunk_tiles(ht, p.Ntrans, all, tgtSweep, p.laneSweep ? 2 : 0, laneFixed);
    cut_tail_chunks(c, k, numCU, p, laneFixed, all, sw, ht);
    TileChunking po = chunk_tiles(ht, p.Ntrans, all, tgtPost, 1);
    TileChunking swPrd, poPrd;
    if (!tileListPrd.empty())
    {
        // (fused post-pass: one tile per workgroup here too)
        swPrd = chunk_tiles(ht, p.Ntrans, tileListPrd,
                            p.laneSweep ? ((int)tileListPrd.size() * p.laneSplitPrd + W - 1) / W
                            : p.tileFuse ? (int)tileListPrd.size()
                                          : std::min((2 * (int)tileListPrd.size() + W - 1) / W, numCU * wgPerCU),
                            0, p.laneSweep ? std::max(1, W / p.laneSplitPrd) : 0);
        poPrd = chunk_tiles(ht, p.Ntrans, tileListPrd, std::min((int)tileListPrd.size(), numCU * postPerCU), 1);
    }
    // both chunkings share one accumulator-slot capacity per kind
    p.maxCTTile = std::max(sw.maxCT, swPrd.maxCT);
    p.maxCTPost = po.maxCT;
    choose_depth_split(c, k, numCU, p); // (deep columns on the march: now that the chunking has fixed maxCTTile)
    widen(sw, p.maxCTTile);
    if (!tileListPrd.empty())
        widen(swPrd, p.maxCTTile);
    for (size_t e = 0; e < tslots.size(); ++e)
        tslots[e].cs = sw.cs[e];
    ht.laneCsPure = sw.csPure;
    ht.chunkTile = sw.chunkTile;
    ht.tileSlotTr = sw.slotTr;
    p.nTileChunks = (int)ht.chunkTile.size() - 1;
    if (p.deterministic)
    {
        det_lists(p.Ntrans, p.maxCTTile, ht.tileSlotTr, p.nTileChunks, ht.detOff, ht.detEnt);
        if (!tileListPrd.empty())
            det_lists(p.Ntrans, p.maxCTTile, swPrd.slotTr, (int)swPrd.chunkTile.size() - 1, ht.detOffPrd, ht.detEntPrd);
        const size_t nch = std::max<size_t>(p.nTileChunks, tileListPrd.empty() ? 0 : swPrd.chunkTile.size() - 1);
        ht.detSlabCount = nch * p.maxCTTile * 4 * Ns;
        ht.detPartCount = det_reduce_scratch_doubles((int)Ns, p.Ntrans);
    }
    ht.postChunkTile = po.chunkTile;
    ht.postSlotTr = po.slotTr;
    ht.postCs.assign(std::max<size_t>(slots.size(), 1), 0);
    for (size_t e = 0; e < slots.size(); ++e)
        ht.postCs[e] = po.cs[e];
    p.nPostChunks = (int)ht.postChunkTile.size() - 1;
    p.nTilesPrd = (int)tileListPrd.size();
    p.nTileChunksPrd = p.nPostChunksPrd = 0;
    if (!tileListPrd.empty())
    {
        ht.tslotsPrd = tslots;
        for (size_t e = 0; e < tslots.size(); ++e)
            ht.tslotsPrd[e].cs = swPrd.cs[e];
        ht.chunkTilePrd = swPrd.chunkTile;
        ht.tileSlotTrPrd = swPrd.slotTr;
        ht.postChunkTilePrd = poPrd.chunkTile;
        p.nTileChunksPrd = (int)ht.chunkTilePrd.size() - 1;
        p.nPostChunksPrd = (int)ht.postChunkTilePrd.size() - 1;
    }
    return check_launch_lds(c, p);
}

// ---- the flat per-transition, per-atom and per-ray tables; full own grids and trapezoid weights of the lines ----------------
void plan_transition_tables(const lwhip_context& c, const TablePlan& p, HostTables& ht)
{
    const int NR2 = 2 * c.Nrays;
    std::vector<DevTrans>& dt = ht.dtrans;
    std::vector<int32_t>&li = ht.transLi, &lj = ht.transLj, &rayAll = ht.rayAll, &rayUp = ht.rayUp, &aNl = ht.atomNlevel, &aDet = ht.atomDetailed;
    dt.resize(p.Ntrans);
    li.resize(p.Ntrans);
    lj.resize(p.Ntrans);
    for (int tr = 0; tr < p.Ntrans; ++tr)
    {
        const HostTrans& h = ht.trans[tr];
        DevTrans& d = dt[tr];
        d.type = h.t.type;
        d.atom = h.atom;
        d.gi = ht.levelOff[h.atom] + h.t.i;
        d.gj = ht.levelOff[h.atom] + h.t.j;
        d.Nblue = h.NblueLoc;
        d.Nred = h.NredLoc;
        d.prd = (h.t.type == LWHIP_LINE && h.t.prd) ? 1 : 0;
        d.op = c.atoms[h.atom].detailed ? 0 : 1;
        d.row = h.row;
        d._pad = 0;
        d.parOff = h.parOff;
        d.phiOff = h.phiOff;
        d.rhoOff = h.rhoOff;
        li[tr] = h.t.i;
        lj[tr] = h.t.j;
    }
    rayAll.resize(NR2);
    rayUp.resize(c.Nrays);
    for (int r = 0; r < NR2; ++r)
        rayAll[r] = r;
    for (int m = 0; m < c.Nrays; ++m)
        rayUp[m] = 2 * m + 1;
    aNl.resize(c.Natom);
    aDet.resize(c.Natom);
    for (int ia = 0; ia < c.Natom; ++ia)
    {
        aNl[ia] = c.atoms[ia].Nlevel;
        aDet[ia] = c.atoms[ia].detailed ? 1 : 0;
    }
    ht.atomTrOffD.assign(ht.atomTrOff.begin(), ht.atomTrOff.end());
    // full own grids and trapezoid weights of the lines (device Voigt profiles)
    std::vector<double>&lw = ht.lineWave, &lq = ht.lineWlam;
    for (auto& h : ht.trans)
    {
        h.waveOff = -1;
        if (h.t.type != LWHIP_LINE)
            continue;
        h.waveOff = (int64_t)lw.size();
        const int len = h.t.Nred - h.t.Nblue;
        for (int lt = 0; lt < len; ++lt)
        {
            lw.push_back(h.t.wavelength[lt]);
            lq.push_back(trans_wlambda(h.t, lt));
        }
    }
    if (lw.empty())
    {
        lw.push_back(0.0);
        lq.push_back(0.0);
    }
    // (never an empty upload)
    if (ht.slotTrD.empty())
        ht.slotTrD.push_back(0);
}

// the continua of every wavelength in transition order, ready-to-use offsets and level-column slots
void plan_cont_records(const lwhip_context& c, const TablePlan& p, HostTables& ht)
{
    const int Ns = c.Ns;
    const std::vector<DevLaHeader>& hdr = ht.laHdr;
    const std::vector<DevSlot>& slots = ht.slots;
    const std::vector<int32_t>& slotTr = ht.slotTrD;
    const std::vector<int>& laneCsPure = ht.laneCsPure;
    std::vector<DevContRec>& cr = ht.contRec;
    cr.assign(std::max<size_t>(slots.size(), 1), DevContRec{});
    for (int la = 0; la < c.Nla; ++la)
    {
        const DevLaHeader& h = hdr[la];
        const int base = h.off + h.nLine;
        for (int q = 0; q < h.nMixed + h.nPure; ++q)
        {
            const int ord = slots[base + q]._pad;
            const DevSlot& sl = slots[base + ord];
            DevContRec r{};
            r.nI = (uint32_t)((size_t)sl.gi * Ns * sizeof(double));
            r.nJ = (uint32_t)((size_t)sl.gj * Ns * sizeof(double));
            r.rat = (uint32_t)((size_t)sl.row * Ns * sizeof(double));
            r.pOff = (uint32_t)((size_t)(h.nLine + ord) * sizeof(DevSlot) + offsetof(DevSlot, p));
            r.sEta = (uint16_t)sl.atom;
            r.sChiI = (uint16_t)(c.Natom + sl.gi);
            r.sChiJ = (uint16_t)(c.Natom + sl.gj);
            r.sUi = (uint16_t)(c.Natom + p.NlevTot + sl.gi);
            r.sUj = (uint16_t)(c.Natom + p.NlevTot + sl.gj);
            r.flags = (uint8_t)((sl.flags & 1) | (ord >= h.nMixed ? 2 : 0));
            r.ms = (int8_t)sl.ms;
            r.tr = (int16_t)slotTr[base + ord];
            r.cs = (int16_t)((p.laneSweep && ord >= h.nMixed) ? laneCsPure[base + ord] : 0);
            cr[base + q] = r;
        }
    }
}

// Lane sweep: every tile's finish program (post_program), and whether its words are in the wide encoding
int plan_post_programs(const lwhip_context& c, const TableKnobs& k, const TablePlan& p, HostTables& ht)
{
    const std::vector<DevLaHeader>& hdr = ht.laHdr;
    const std::vector<DevTile>& tiles = ht.tiles;
    std::vector<DevPostProg>& pp = ht.postProg;
    std::vector<char>& ppWide = ht.ppWide;
    pp.assign(std::max<size_t>(tiles.size(), 1), DevPostProg{});
    ppWide.assign(std::max<size_t>(tiles.size(), 1), 0);
    for (size_t t = 0; t < tiles.size(); ++t)
    {
        bool wide = false;
        if (!post_program(c, p, ht, tiles[t].la0, pp[t], &wide))
            return fail(LWHIP_ERR_UNSUPPORTED, "lane sweep: post program");
        ppWide[t] = wide ? 1 : 0;
    }
    if (k.verbose)
    {
        // which program words occur (the finish serves the common ones with fixed registers)
        std::map<std::pair<unsigned, unsigned>, int> hist;
        for (size_t t = 0; t < tiles.size(); ++t)
        {
            const DevLaHeader& h = hdr[tiles[t].la0];
            for (int q = 0; q < h.nMixed + h.nPure; ++q)
                hist[{ pp[t].code[q], pp[t].ops[q] }]++;
        }
        for (const auto& kv : hist)
            std::fprintf(stderr, "  finish program word code %#x ops %#x: %d continua\n", kv.first.first, kv.first.second, kv.second);
    }
    return LWHIP_OK;
}

// Fixed-order mode (LWHIP_OPT_DETERMINISTIC): every task's turn at each of its accumulator slots -- the value the slot's
// turn counter holds when the task may add (lwhip_lanesweep.hip, ls_turn_wait).  Per workgroup: its rounds in order;
// inside a round first the line / mixed-continuum adds of every task (they precede the barriers of a split tile, the
// pure continua's follow them: a wait never points across a barrier the other way), then the pure continua's; the
// tasks of a round in order of expected cost, so that nobody waits for a wavefront that is still marching.  A line /
// mixed slot counts one per wavefront of the tile's group (each adds the integrals of its own rays to every point), a
// pure continuum one per task (every point is finished by exactly one wavefront).  The turn rides in bits 8 .. 23 of
// the slot's flags (lines, mixed continua) and in bits 16 .. 31 of DevLaneFin::feed (pure continua).
bool assign_turns(const TableKnobs& k, const TablePlan& p, HostTables& ht, std::vector<DevTileSlot>& ts, const std::vector<int32_t>& chTile,
                  const std::vector<int32_t>* list, const std::vector<int32_t>* split, int launchSplit, bool pure)
{
    std::vector<uint32_t>& turnPure = ht.turnPure;
    const std::vector<DevLaHeader>& hdr = ht.laHdr;
    const std::vector<DevTile>& tiles = ht.tiles;
    const std::vector<DevContRec>& cr = ht.contRec;
    const int nch = (int)chTile.size() - 1;
    std::vector<int> cnt(std::max(p.maxCTTile, 1));
    // (measurement only: bit 0 -- the line / mixed slots' turns are 0, nobody waits there; bit 1 -- the pure continua's;
    // bit 2 -- tasks in wavefront order instead of by expected cost.  With a bit of 0 / 1 set the sums' order is the timing's)
    const int noWaitBits = k.detNoWait;
    for (int ch = 0; ch < nch; ++ch)
    {
        std::fill(cnt.begin(), cnt.end(), 0);
        const int S = std::max(1, split ? (*split)[ch] : launchSplit);
        const int nGroups = std::max(1, p.tileWaves / S);
        const int n = chTile[ch + 1] - chTile[ch];
        for (int r0 = 0; r0 < n; r0 += nGroups)
        {
            std::vector<int> tasks;
            for (int i = r0; i < std::min(n, r0 + nGroups); ++i)
                tasks.push_back(list ? (*list)[chTile[ch] + i] : chTile[ch] + i);
            if (!(noWaitBits & 4))
                std::stable_sort(tasks.begin(), tasks.end(), [&](int x, int y) { return task_cost(tiles[x]) < task_cost(tiles[y]); });
            // (a tile that walks its rays more than once -- a blend, a generic tile -- adds after every run: it takes a
            // SECOND turn for the adds of its later runs, behind the first turns of the whole round, so that it does not
            // hold a slot while it marches again -- 28 blends of 3 429 tiles doubled the launch's time when they did)
            for (int pass = 0; pass < 2; ++pass)
                for (int t : tasks)
                {
                    const int nl = tiles[t].nLine;
                    const bool fastKind = fast_kind(nl, tiles[t].nMixed);
                    if (pass == 1 && !(fastKind && nl == 2)) // (only the compiled blend kind walks its rays twice)
                        continue;
                    for (int e = 0; e < tiles[t].nLine + tiles[t].nMixed; ++e)
                    {
                        DevTileSlot& u = ts[tiles[t].slotOff + e];
                        if (u.cs < 0 || u.cs >= (int)cnt.size() || cnt[u.cs] + S > 0x7ff)
                            return false;
                        const int turn = (noWaitBits & 1) ? 0 : cnt[u.cs];
                        if (pass == 0)
                            u.flags = (u.flags & 0xff) | (turn << 8);
                        else
                            u.flags |= turn << 20;
                        cnt[u.cs] += S;
                    }
                }
            for (int t : tasks)
            {
                const DevLaHeader& h = hdr[tiles[t].la0];
                if (!pure || h.nPure == 0)
                    continue;
                for (int q = 0; q < std::min(h.nMixed + h.nPure, (int)LWHIP_POST_MAXC); ++q)
                {
                    const DevContRec& r = cr[h.off + h.nLine + q];
                    if (!(r.flags & 2))
                        continue;
                    if (r.cs < 0 || r.cs >= (int)cnt.size() || cnt[r.cs] + 1 > 0xffff)
                        return false;
                    turnPure[(size_t)t * LWHIP_POST_MAXC + q] = (noWaitBits & 2) ? 0u : (uint32_t)cnt[r.cs];
                    cnt[r.cs] += 1;
                }
            }
        }
    }
    return true;
}

int plan_fixed_order_turns(const TableKnobs& k, const TablePlan& p, HostTables& ht)
{
    ht.turnPure.assign(std::max<size_t>(ht.tiles.size() * LWHIP_POST_MAXC, 1), 0u);
    if (!p.laneSweep || !p.deterministic)
        return LWHIP_OK;
    bool okT = assign_turns(k, p, ht, ht.tslots, ht.chunkTile, nullptr, ht.chunkSplit.empty() ? nullptr : &ht.chunkSplit, p.laneSplit, true);
    if (okT && !ht.tileListPrd.empty())
        okT = assign_turns(k, p, ht, ht.tslotsPrd, ht.chunkTilePrd, &ht.tileListPrd, nullptr, p.laneSplitPrd, false);
    if (!okT)
        return fail(LWHIP_ERR_UNSUPPORTED, "fixed-order mode: more adds to one accumulator slot of a workgroup than a turn counter counts");
    return LWHIP_OK;
}

// Lane sweep, more workgroups than the chip holds at once (2 per CU): the heavy ones go first, the light ones fill the tail
// (measured: 8 192 wavelengths 0.188 -> 0.179 ms, 10 240: 0.203 -> 0.200; lightest first: 0.196 / 0.207).
// The chunks stay what they are (neighbouring wavelengths: few accumulator slots); only the order in which the
// workgroups take them changes.  Where the tail was cut (cut_tail_chunks) the order is already there.
void plan_chunk_order(const lwhip_context& c, int numCU, TablePlan& p, HostTables& ht)
{
    const std::vector<DevTile>& tiles = ht.tiles;
    const std::vector<int32_t>& chunkTile = ht.chunkTile;
    p.chunkOrderOn = p.chunkSplitOn = !ht.chunkOrder.empty();
    const int nch = (int)chunkTile.size() - 1;
    if (!p.laneSweep || c.batchHint > 1 || nch <= 2 * numCU || p.chunkOrderOn)
        return;
    std::vector<double> cost(nch, 0.0);
    for (int ch = 0; ch < nch; ++ch)
        for (int i = chunkTile[ch]; i < chunkTile[ch + 1]; ++i)
            cost[ch] += task_cost(tiles[i]);
    std::vector<int32_t>& order = ht.chunkOrder;
    order.resize(nch);
    for (int ch = 0; ch < nch; ++ch)
        order[ch] = ch;
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return cost[x] > cost[y]; });
    p.chunkOrderOn = true;
}

// ---- the flat records of the lane sweep's tasks (lwhip_internal.h: DevLaneWg, DevLaneTile, DevLaneRay, DevLaneFin) --------
std::vector<DevLaneWg> lane_wg_records(const std::vector<int32_t>& chTile, const std::vector<int32_t>* order, const std::vector<int32_t>* split,
                                       int launchSplit)
{
    const int nch = (int)chTile.size() - 1;
    std::vector<DevLaneWg> w(std::max(nch, 1));
    for (int b = 0; b < nch; ++b)
    {
        const int ch = order ? (*order)[b] : b;
        const int S = split ? (*split)[ch] : launchSplit;
        w[b] = DevLaneWg{ ch, S > 1 ? S : 1, chTile[ch], chTile[ch + 1] };
    }
    return w;
}

// the rows of a tile's slot `us` that continuum `cs` feeds (zero_mask's matching, per continuum)
uint8_t feed_byte(const DevSlot& cs, const DevTileSlot& us, bool isThisMixed)
{
    uint32_t b = 0;
    if ((cs.flags & 1) && (us.flags & 1))
    {
        b |= cs.atom == us.atom ? 1u : 0u;
        b |= cs.gi == us.gi ? 2u : 0u;
        b |= cs.gj == us.gi ? 4u : 0u;
        b |= cs.gi == us.gj ? 8u : 0u;
        b |= cs.gj == us.gj ? 16u : 0u;
        b |= cs.gj == us.gi ? 32u : 0u;
        b |= cs.gj == us.gj ? 64u : 0u;
    }
    if (isThisMixed)
        b |= 128u;
    return (uint8_t)b;
}

// which tiles run the generic kind (no compiled kind for their line / mixed-continuum counts), and for those the
// feed bytes of every (continuum, slot) pair -- DevLaneFin::feed holds two slots' worth -- and their moment scratch
std::vector<int32_t> plan_generic_tiles(TablePlan& p, HostTables& ht)
{
    const std::vector<DevLaHeader>& hdr = ht.laHdr;
    const std::vector<DevSlot>& slots = ht.slots;
    const std::vector<DevTile>& tiles = ht.tiles;
    const std::vector<DevTileSlot>& tslots = ht.tslots;
    std::vector<uint8_t>& feedG = ht.laneFeedG;
    std::vector<int32_t> genOf(std::max<size_t>(tiles.size(), 1), -1);
    p.nGenTiles = 0;
    for (size_t t = 0; t < tiles.size(); ++t)
    {
        const DevTile& td = tiles[t];
        if (fast_kind(td.nLine, td.nMixed))
            continue;
        genOf[t] = p.nGenTiles++;
        const DevLaHeader& h0 = hdr[td.la0];
        const size_t base = feedG.size();
        feedG.resize(base + (size_t)LWHIP_POST_MAXC * LWHIP_GEN_MAXS, 0);
        const int nC = std::min(h0.nMixed + h0.nPure, (int)LWHIP_POST_MAXC);
        for (int q = 0; q < nC; ++q)
        {
            const int ord = slots[h0.off + h0.nLine + q]._pad;
            const DevSlot& cs = slots[h0.off + h0.nLine + ord];
            for (int e = 0; e < std::min(td.nLine + td.nMixed, (int)LWHIP_GEN_MAXS); ++e)
                feedG[base + (size_t)q * LWHIP_GEN_MAXS + e] = feed_byte(cs, tslots[td.slotOff + e], e >= td.nLine && ord == e - td.nLine);
        }
    }
    // the moment scratch of the generic tiles' wavefronts: every workgroup of the largest launch, W wavefronts each
    p.momA = 0;
    for (size_t t = 0; t < tiles.size(); ++t)
        if (genOf[t] >= 0)
        {
            const int nl = tiles[t].nLine;
            p.momA = std::max(p.momA, 4 * std::max(nl - 1, 0) + nl * (nl - 1) / 2 + 4 * nl);
        }
    if (p.momA > 0)
        ht.momScratchCount = std::max<size_t>(ht.chunkTile.size(), ht.chunkTilePrd.size()) * p.tileWaves * (size_t)p.momA * p.laneD * 64;
    if (feedG.empty())
        feedG.push_back(0);
    return genOf;
}

std::vector<DevLaneTile> lane_tile_records(const TableKnobs& k, const HostTables& ht, const std::vector<int32_t>& genOf, const std::vector<DevTileSlot>& ts)
{
    const std::vector<DevLaHeader>& hdr = ht.laHdr;
    const std::vector<DevTile>& tiles = ht.tiles;
    const std::vector<DevContRec>& cr = ht.contRec;
    const std::vector<DevPostProg>& pp = ht.postProg;
    const std::vector<char>& ppWide = ht.ppWide;
    std::vector<DevLaneTile> v(std::max<size_t>(tiles.size(), 1), DevLaneTile{});
    for (size_t t = 0; t < tiles.size(); ++t)
    {
        const DevLaHeader& h = hdr[tiles[t].la0];
        v[t].td = tiles[t];
        v[t].nCont = h.nPure > 0 ? h.nMixed + h.nPure : 0;
        v[t].nContAll = std::min(h.nMixed + h.nPure, (int)LWHIP_POST_MAXC);
        {
            // the finish's named-register form serves the tiles whose continua all carry the common words
            bool fast = !ppWide[t];
            const int nC = h.nMixed + h.nPure;
            for (int q = 0; q < nC && q < LWHIP_POST_MAXC; ++q)
            {
                const DevContRec& r = cr[h.off + h.nLine + q];
                const unsigned code = (r.flags & 1) ? pp[t].code[q] : 0x9999u, ops = pp[t].ops[q];
                if (code != 0x9999u && code != 0x1239u && code != 0x4569u)
                    fast = false;
                if ((r.flags & 2) && (r.flags & 1) && ops != 0x03291u && ops != 0x06594u && ops != 0x0AB9Cu)
                    fast = false;
            }
            v[t].finFast = ppWide[t] ? 2 : (fast && k.finFast != 0) ? 1 : 0; // (2: the wide encoding, general form)
        }
        for (int e = 0; e < std::min(2, tiles[t].nLine + tiles[t].nMixed); ++e)
            v[t].slot[e] = ts[tiles[t].slotOff + e];
        v[t].gen = genOf[t];
    }
    return v;
}

// per (tile, wavelength) and per (tile, continuum): what a task's rays and its finish read
void plan_lane_rays_fin(const lwhip_context& c, const TablePlan& p, HostTables& ht)
{
    const int L = p.tileL;
    const std::vector<DevLaHeader>& hdr = ht.laHdr;
    const std::vector<DevSlot>& slots = ht.slots;
    const std::vector<DevTile>& tiles = ht.tiles;
    const std::vector<DevTileSlot>& tslots = ht.tslots;
    const std::vector<DevContRec>& cr = ht.contRec;
    const std::vector<DevPostProg>& pp = ht.postProg;
    std::vector<DevLaneRay>& rays = ht.laneRays;
    std::vector<DevLaneFin>& fin = ht.laneFin;
    std::vector<double>& finPar = ht.laneFinPar;
    rays.assign(std::max<size_t>(tiles.size() * L, 1), DevLaneRay{});
    fin.assign(std::max<size_t>(tiles.size() * LWHIP_POST_MAXC, 1), DevLaneFin{});
    finPar.assign(std::max<size_t>(tiles.size() * LWHIP_POST_MAXC * L * 3, 1), 0.0);
    for (size_t t = 0; t < tiles.size(); ++t)
    {
        const DevTile& td = tiles[t];
        const DevLaHeader& h0 = hdr[td.la0];
        const int nSl = std::min(2, td.nLine + td.nMixed);
        for (int r = 0; r < L; ++r)
        {
            const int la = td.la0 + std::min(r, td.nl - 1);
            DevLaneRay& lr = rays[t * L + r];
            lr.wav = c.prob.wavelength[c.laStart + la];
            for (int e = 0; e < nSl; ++e)
                for (int q = 0; q < 4; ++q)
                    lr.p[e][q] = slots[hdr[la].off + tslots[td.slotOff + e].e].p[q];
        }
        const int nC = h0.nMixed + h0.nPure;
        for (int q = 0; q < nC && q < LWHIP_POST_MAXC; ++q)
        {
            const DevContRec& r = cr[h0.off + h0.nLine + q];
            uint32_t w[8];
            std::memcpy(w, &r, sizeof(w));
            // the rows of the tile's slots this continuum feeds (zero_mask's matching, per continuum)
            uint32_t feed = 0;
            const int ord = slots[h0.off + h0.nLine + q]._pad; // transition-order position q -> slot ordinal
            const DevSlot& cs = slots[h0.off + h0.nLine + ord];
            for (int e = 0; e < nSl; ++e)
                feed |= (uint32_t)feed_byte(cs, tslots[td.slotOff + e], e >= td.nLine && ord == e - td.nLine) << (8 * e);
            feed |= (ht.turnPure[t * LWHIP_POST_MAXC + q] & 0xffffu) << 16; // (fixed-order mode: the task's turn at this continuum's slot)
            fin[t * LWHIP_POST_MAXC + q] = DevLaneFin{ w[0], w[1], w[2], w[6], w[7], pp[t].code[q], pp[t].ops[q], feed };
            for (int rr = 0; rr < L; ++rr)
            {
                const int la = td.la0 + std::min(rr, td.nl - 1);
                const char* lsB = (const char*)&slots[hdr[la].off];
                for (int k = 0; k < 3; ++k)
                {
                    double v;
                    std::memcpy(&v, lsB + r.pOff + 8 * k, sizeof(double));
                    finPar[((t * LWHIP_POST_MAXC + q) * L + rr) * 3 + k] = v;
                }
            }
        }
    }
}

void plan_lane_records(const lwhip_context& c, const TableKnobs& k, TablePlan& p, HostTables& ht)
{
    ht.laneWg = lane_wg_records(ht.chunkTile, p.chunkOrderOn ? &ht.chunkOrder : nullptr, p.chunkSplitOn ? &ht.chunkSplit : nullptr, p.laneSplit);
    const std::vector<int32_t> genOf = plan_generic_tiles(p, ht);
    ht.laneTiles = lane_tile_records(k, ht, genOf, ht.tslots);
    if (p.nTilesPrd > 0)
    {
        ht.laneTilesPrd = lane_tile_records(k, ht, genOf, ht.tslotsPrd);
        ht.laneWgPrd = lane_wg_records(ht.chunkTilePrd, nullptr, nullptr, p.laneSplitPrd);
    }
    plan_lane_rays_fin(c, p, ht);
}
}

// The device-free half of build_tables: every decision and every byte of the structure tables, from the context's host fields
// (context_init_host), the knobs and the device's compute-unit count.  Calls no HIP function.
int plan_tables(const lwhip_context& c, const TableKnobs& k, int numCU, TablePlan& p, HostTables& ht)
{
    Ticker tick{ k.createTiming };
    p = TablePlan{};
    p.deterministic = c.deterministic;
    ht = HostTables{};
    plan_atom_offsets(c, p, ht);
    int st = plan_hybrid_prd(c, p, ht);
    if (st != LWHIP_OK)
        return st;
    plan_transition_list(c, p, ht);
    tick("transition list, hybrid PRD");
    plan_transition_params(p, ht);
    tick("per-transition parameters");
    st = plan_wavelength_activity(c, p, ht);
    if (st != LWHIP_OK)
        return st;
    tick("wavelength activity, programs");
    p.tiled = !c.is2d;
    if (p.tiled)
    {
        st = choose_sweep(c, k, p, ht);
        if (st == LWHIP_OK)
            st = plan_tiles(c, k, numCU, p, ht);
        if (st == LWHIP_OK)
            st = plan_chunks(c, k, numCU, p, ht);
        if (st != LWHIP_OK)
            return st;
    }
    tick("tiles, chunks, work distribution");
    plan_transition_tables(c, p, ht);
    if (p.tiled)
    {
        plan_cont_records(c, p, ht);
        if (p.laneSweep)
            st = plan_post_programs(c, k, p, ht);
        if (st == LWHIP_OK)
            st = plan_fixed_order_turns(k, p, ht);
        if (st != LWHIP_OK)
            return st;
        plan_chunk_order(c, numCU, p, ht);
        if (p.laneSweep)
            plan_lane_records(c, k, p, ht);
        // (never an empty upload)
        for (std::vector<int32_t>* v : { &ht.tileRemap, &ht.chunkTile, &ht.chunkTilePrd, &ht.tileListPrd, &ht.tileSlotTr, &ht.tileSlotTrPrd, &ht.postChunkTile,
                                        &ht.postChunkTilePrd, &ht.postSlotTr, &ht.postCs })
            if (v->empty())
                v->resize(1);
        if (ht.tiles.empty())
            ht.tiles.resize(1);
        if (ht.tslots.empty())
            ht.tslots.resize(1);
        if (ht.tslotsPrd.empty())
            ht.tslotsPrd.resize(1);
        if (ht.tcopies.empty())
            ht.tcopies.resize(1);
    }
    tick("device tables, lane records");
    return LWHIP_OK;
}

namespace
{
// a structure table: this context's copy, or -- for a context made with lwhip_create_like -- its owner's where that holds
// exactly these bytes (DevBuf::upload_or_borrow).  An empty vector is a table this context does not have.
template <class T> hipError_t put(lwhip_context* c, DevBuf<T> TableBufs::*buf, const std::vector<T>& v)
{
    const TableBufs* from = c->tablesFrom;
    return (c->*buf).upload_or_borrow(c->mem, v, from ? &(from->*buf) : nullptr);
}
}

// The device half: the plan into the context, the tables onto the device -- every upload and the few allocations in one fixed
// order on the context's stream, so that a borrower's arena and its gathered upload always see the same sequence.
int upload_tables(lwhip_context* c, const TablePlan& p, const HostTables& ht)
{
    static_cast<TablePlan&>(*c) = p;
    c->trans = ht.trans;
    c->levelOff = ht.levelOff;
    c->atomTrOff = ht.atomTrOff;
    c->gammaOff = ht.gammaOff;
    c->hLa2prdHost = ht.hLa2prdHost;
    c->hLa2hHost = ht.hLa2hHost;
    c->hRhoOffHost = ht.hRhoOffHost;
    c->hdrHost = ht.laHdr;
    c->contLaHost.assign(ht.contLa.begin(), ht.contLa.begin() + p.nContLa);
    // hybrid PRD: every context's own (the coefficients follow the atmosphere)
    HIP_TRY(c->hRho.upload(c->mem, ht.hRho));
    HIP_TRY(c->hLa2h.upload(c->mem, ht.hLa2h));
    HIP_TRY(c->hJOff.upload(c->mem, ht.hJOff));
    HIP_TRY(c->hJCoef.upload(c->mem, ht.hJCoef));
    HIP_TRY(c->JRest.alloc_zero(c->mem, ht.JRestCount));
    // fixed-order mode
    HIP_TRY(put(c, &TableBufs::detOff, ht.detOff));
    HIP_TRY(put(c, &TableBufs::detEnt, ht.detEnt));
    HIP_TRY(put(c, &TableBufs::detOffPrd, ht.detOffPrd));
    HIP_TRY(put(c, &TableBufs::detEntPrd, ht.detEntPrd));
    HIP_TRY(c->detSlab.alloc(c->mem, ht.detSlabCount));
    HIP_TRY(c->detPart.alloc(c->mem, ht.detPartCount));
    HIP_TRY(put(c, &TableBufs::lineWave, ht.lineWave));
    HIP_TRY(put(c, &TableBufs::lineWlam, ht.lineWlam));
    HIP_TRY(put(c, &TableBufs::par, ht.par));
    HIP_TRY(put(c, &TableBufs::dtrans, ht.dtrans));
    HIP_TRY(put(c, &TableBufs::laHdr, ht.laHdr));
    HIP_TRY(put(c, &TableBufs::slots, ht.slots));
    HIP_TRY(put(c, &TableBufs::slotTrD, ht.slotTrD));
    HIP_TRY(put(c, &TableBufs::progs, ht.progs));
    HIP_TRY(put(c, &TableBufs::progRows, ht.progRows));
    HIP_TRY(put(c, &TableBufs::progEnts, ht.progEnts));
    HIP_TRY(put(c, &TableBufs::contLa, ht.contLa));
    HIP_TRY(put(c, &TableBufs::rayAll, ht.rayAll));
    HIP_TRY(put(c, &TableBufs::rayUp, ht.rayUp));
    // the sweeps' tiles and chunks
    HIP_TRY(put(c, &TableBufs::contRec, ht.contRec));
    HIP_TRY(put(c, &TableBufs::postProg, ht.postProg));
    HIP_TRY(put(c, &TableBufs::tiles, ht.tiles));
    HIP_TRY(put(c, &TableBufs::tslots, ht.tslots));
    HIP_TRY(put(c, &TableBufs::tslotsPrd, ht.tslotsPrd));
    HIP_TRY(put(c, &TableBufs::tcopies, ht.tcopies));
    HIP_TRY(put(c, &TableBufs::tileRemap, ht.tileRemap));
    HIP_TRY(put(c, &TableBufs::chunkTile, ht.chunkTile));
    HIP_TRY(put(c, &TableBufs::chunkOrder, ht.chunkOrder));
    HIP_TRY(put(c, &TableBufs::chunkSplit, ht.chunkSplit));
    // the lane sweep's records
    HIP_TRY(put(c, &TableBufs::laneWg, ht.laneWg));
    HIP_TRY(c->momScratch.alloc(c->mem, ht.momScratchCount)); // (written before it is read: first ray / per point)
    HIP_TRY(put(c, &TableBufs::laneFeedG, ht.laneFeedG));
    HIP_TRY(put(c, &TableBufs::laneTiles, ht.laneTiles));
    HIP_TRY(put(c, &TableBufs::laneTilesPrd, ht.laneTilesPrd));
    HIP_TRY(put(c, &TableBufs::laneWgPrd, ht.laneWgPrd));
    HIP_TRY(put(c, &TableBufs::laneRays, ht.laneRays));
    HIP_TRY(put(c, &TableBufs::laneFin, ht.laneFin));
    HIP_TRY(put(c, &TableBufs::laneFinPar, ht.laneFinPar));
    HIP_TRY(put(c, &TableBufs::chunkTilePrd, ht.chunkTilePrd));
    HIP_TRY(put(c, &TableBufs::tileListPrd, ht.tileListPrd));
    HIP_TRY(put(c, &TableBufs::tileSlotTr, ht.tileSlotTr));
    HIP_TRY(put(c, &TableBufs::tileSlotTrPrd, ht.tileSlotTrPrd));
    HIP_TRY(put(c, &TableBufs::postChunkTile, ht.postChunkTile));
    HIP_TRY(put(c, &TableBufs::postChunkTilePrd, ht.postChunkTilePrd));
    HIP_TRY(put(c, &TableBufs::postSlotTr, ht.postSlotTr));
    HIP_TRY(put(c, &TableBufs::postCs, ht.postCs));
    HIP_TRY(put(c, &TableBufs::transLi, ht.transLi));
    HIP_TRY(put(c, &TableBufs::transLj, ht.transLj));
    HIP_TRY(put(c, &TableBufs::atomNlevel, ht.atomNlevel));
    HIP_TRY(put(c, &TableBufs::atomDetailed, ht.atomDetailed));
    HIP_TRY(put(c, &TableBufs::atomTrOffD, ht.atomTrOffD));
    HIP_TRY(c->atomGammaOff.upload(c->mem, c->gammaOff));
    return LWHIP_OK;
}

// lwhip_create's tables: read the knobs, ask the device for its compute units, plan, upload
int build_tables(lwhip_context* c)
{
    const TableKnobs knobs = read_table_knobs();
    int numCU = 256;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, c->device) == hipSuccess && prop.multiProcessorCount > 0)
        numCU = prop.multiProcessorCount;
    TablePlan plan;
    HostTables tables;
    int st = plan_tables(*c, knobs, numCU, plan, tables);
    if (st != LWHIP_OK)
        return st;
    Ticker tick{ knobs.createTiming };
    st = upload_tables(c, plan, tables);
    tick("upload");
    return st;
}

uint64_t plan_signature(const TablePlan& p)
{
    SigFold f;
#define X(type, name, init) f.mix((uint64_t)(int64_t)p.name);
    LWHIP_TABLE_PLAN(X)
#undef X
    return f.h;
}
}

int lwhip_tables_signature(lwhip_context* c, uint64_t out[2])
{
    if (!c || !out)
        return fail(LWHIP_ERR_INVALID, "tables_signature: null argument");
    SigFold f;
#define X(type, name) f.mix((uint64_t)c->name.n), f.mix(c->name.sig);
    LWHIP_TABLE_BUFS(X)
#undef X
    out[0] = f.h;
    out[1] = plan_signature(*c);
    return LWHIP_OK;
}
