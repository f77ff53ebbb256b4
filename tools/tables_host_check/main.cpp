// tables_host_check -- plan_tables on a machine without a device, for the sanitizers: a small synthetic problem built here,
// context_init_host, then the device-free half of lwhip_create's tables (lwhip_tables.hip) for a handful of sizes, solvers and
// options.  Prints the plan's signature word of every case; exits 0 when every case ends as expected.  run.sh builds it, and
// the host unit it calls, with -fsanitize=address,undefined and runs it.  Never run on a GPU machine: it has nothing to do there.
#include "../../lightweaver_amd/csrc/lwhip_host.h"

#include <cinttypes>

namespace
{
// Two atoms on a grid of 40 wavelengths.  The first has three levels, two lines whose ranges overlap and two continua: one
// shares a level with a line active at its wavelengths (a mixed continuum), one lies where no line is (pure).  The second has
// two levels, a line across both of the first atom's (three lines at one wavelength: the generic kind) and a continuum over
// the whole grid.  nineLines: instead, one atom of ten levels whose nine lines all overlap.
struct Synthetic
{
    int Ns, Nrays = 3, Nlambda = 40;
    std::vector<double> wave, pool, muz, wmu;
    std::vector<lwhip_transition> tr0, tr1;
    std::vector<lwhip_atom> atoms;
    lwhip_problem prob{};

    lwhip_transition transition(int type, int i, int j, int Nblue, int Nred)
    {
        lwhip_transition t{};
        t.type = type;
        t.i = i;
        t.j = j;
        t.Nblue = Nblue;
        t.Nred = Nred;
        t.Aji = 1.0e7;
        t.Bji = 2.0e9;
        t.Bij = 3.0e9;
        t.lambda0 = wave[(Nblue + Nred) / 2];
        t.dopplerWidth = type == LWHIP_LINE ? 2.99792458e8 / t.lambda0 : 1.0;
        t.wavelength = wave.data() + Nblue;
        t.alpha = type == LWHIP_CONTINUUM ? pool.data() : nullptr;
        t.phi = t.wphi = t.Rij = t.Rji = pool.data();
        return t;
    }
    lwhip_atom atom(int Nlevel, std::vector<lwhip_transition>& tr)
    {
        lwhip_atom a{};
        a.Nlevel = Nlevel;
        a.Ntrans = (int)tr.size();
        a.n = a.Gamma = pool.data();
        a.nStar = a.nTotal = a.vBroad = pool.data();
        a.trans = tr.data();
        return a;
    }
    Synthetic(int Ns_, int solver, bool nineLines) : Ns(Ns_)
    {
        for (int la = 0; la < Nlambda; ++la)
            wave.push_back(100.0 + la);
        // (every array the plan does not read points here: it is as long as the longest of them, 10 x 10 x Ns)
        pool.assign((size_t)std::max(Nlambda * Nrays * 2, 100) * Ns, 1.0e-3);
        muz = { 0.11, 0.5, 0.89 };
        wmu = { 0.28, 0.44, 0.28 };
        if (nineLines)
        {
            for (int i = 0; i < 9; ++i)
                tr0.push_back(transition(LWHIP_LINE, i, 9, 10 + i, 30));
            atoms = { atom(10, tr0) };
        }
        else
        {
            tr0 = { transition(LWHIP_LINE, 0, 1, 5, 20), transition(LWHIP_LINE, 1, 2, 12, 30), transition(LWHIP_CONTINUUM, 0, 2, 0, 10),
                    transition(LWHIP_CONTINUUM, 1, 2, 32, 40) };
            tr1 = { transition(LWHIP_LINE, 0, 1, 15, 25), transition(LWHIP_CONTINUUM, 0, 1, 0, 40) };
            atoms = { atom(3, tr0), atom(2, tr1) };
        }
        prob.abiVersion = LWHIP_ABI_VERSION;
        prob.Nspace = Ns;
        prob.Nrays = Nrays;
        prob.Nlambda = Nlambda;
        prob.Natom = (int)atoms.size();
        prob.formalSolver = solver;
        prob.height = prob.temperature = prob.vlosMu = prob.bgChi = prob.bgEta = prob.bgSca = pool.data();
        prob.J = prob.I = pool.data();
        prob.muz = muz.data();
        prob.wmu = wmu.data();
        prob.wavelength = wave.data();
        prob.zLowerBc.type = LWHIP_BC_THERMALISED;
        prob.zUpperBc.type = LWHIP_BC_ZERO;
        prob.atoms = atoms.data();
    }
};

// one case: the status plan_tables must end with; prints the case and the plan's word
bool run(const char* name, Synthetic&& s, const lwhip_options* opts, int want)
{
    std::string why;
    int st = validate(&s.prob, why);
    lwhip_context c;
    if (st == LWHIP_OK)
        st = context_init_host(&c, &s.prob, opts);
    TablePlan plan;
    HostTables tables;
    if (st == LWHIP_OK)
        st = plan_tables(c, read_table_knobs(), 256, plan, tables);
    if (st == LWHIP_OK)
        std::printf("%-28s Ns %3d  %s  tiles %3d  chunks %3d  plan %016" PRIx64 "\n", name, s.Ns, plan.laneSweep ? "lanes" : "march", plan.nTiles,
                    plan.nTileChunks, plan_signature(plan));
    else
        std::printf("%-28s Ns %3d  refused (%d): %s%s\n", name, s.Ns, st, why.c_str(), lwhip_last_error());
    return st == want;
}
}

int main()
{
    bool ok = true;
    const char* solverName[3] = { "linear", "besser", "bezier3" };
    for (int Ns : { 13, 82, 300 })
        for (int solver : { LWHIP_FS_LINEAR_1D, LWHIP_FS_BESSER_1D, LWHIP_FS_BEZIER3_1D })
            ok &= run(solverName[solver], Synthetic(Ns, solver, false), nullptr, LWHIP_OK);
    lwhip_options o{};
    o.flags = LWHIP_OPT_DETERMINISTIC;
    ok &= run("deterministic", Synthetic(82, LWHIP_FS_BEZIER3_1D, false), &o, LWHIP_OK);
    o = lwhip_options{};
    o.flags = 4;
    ok &= run("batchHint 4", Synthetic(82, LWHIP_FS_BEZIER3_1D, false), &o, LWHIP_OK);
    for (int rank = 0; rank < 2; ++rank)
    {
        o = lwhip_options{};
        o.worldSize = 2;
        o.worldRank = rank;
        o.laStart = rank * 20;
        o.laEnd = o.laStart + 20;
        ok &= run(rank ? "shard 1 of 2" : "shard 0 of 2", Synthetic(82, LWHIP_FS_BEZIER3_1D, false), &o, LWHIP_OK);
    }
    ok &= run("nine overlapping lines", Synthetic(82, LWHIP_FS_BEZIER3_1D, true), nullptr, LWHIP_ERR_UNSUPPORTED);
    std::printf(ok ? "tables_host_check: every case ended as expected\n" : "tables_host_check: FAILED\n");
    return ok ? 0 : 1;
}
