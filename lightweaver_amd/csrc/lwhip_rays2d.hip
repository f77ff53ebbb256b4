// lwhip_rays2d.hip -- emergent intensity along observer rays of a 2D context: what LwContext.compute_rays(mus, upOnly=True)
// (Source/LwMiddleLayer.pyx:3898-4002) computes on a 2D atmosphere, from the state that is resident on the device.
// lwhip_compute_rays_2d.
//
// The reference copies the problem, sets the new rays, builds their intersection table, makes a second context, recomputes
// and stores phi for the new rays and runs formal_sol(upOnly).  Here the table of the requested directions is built on the
// host (lwhip_build_intersections_impl), uploaded next to the context's own (geom2d_upload) and kept until another view is
// asked for; rays2d_gather_kernel forms chi and S of every (wavelength, direction, point) with phi = H(a, v) / (sqrt(pi) vBroad),
// v = ((lambda - lambda0) c / lambda0 + mux vx + muz vz) / vBroad, evaluated where it gathers; the solve is the 2D formal solver
// of the iteration (launch_fs2d, up-going rays only) in the context's batch scratch, and iout2d_kernel moves the top plane to
// the staging buffer of the call.  No phi pool, no second context; I, J, Gamma, the rates, phi / wphi, the context's own
// tables, depth data and z-plane outputs are not touched.
#include "lwhip_host.h"
#include "lwhip_device.h"
// H(a, v) under the same contraction setting as the stored profiles' unit: the same argument gives the same bits
#include "lwhip_voigt_dev.h"

// As in lwhip_rays.hip: no fused multiply-adds from here on, so that the operations match the reference's one for one.
#pragma clang fp contract(off)

#include <algorithm>
#include <atomic>
#include <cstring>
#include <memory>
#include <mutex>
#include <vector>

extern "C" int lwhip_build_intersections_impl(const lwhip_grid2d* grid, lwhip_intersection* uw, lwhip_intersection* dw,
                                              int32_t* longCharIdx, int32_t* substepOff, int32_t capLongChar,
                                              lwhip_intersection* substeps, int64_t capSubsteps, int32_t* nLongChar,
                                              int64_t* nSubsteps);

namespace lwhip
{
namespace
{
enum { R2G_THREADS = 256 };

struct Rays2dArgs
{
    int32_t Ns, nDir, la0, nLa; // nDir: the directions of this launch; la0: first row of the context's grid
    const double* temperature;
    const double* wavelength;
    const double* bgChi;
    const double* bgEta;
    const double* bgSca;
    const double* J;
    const double* n;
    const double* ratio;
    const double* par;
    const double* rho;
    const double* vBroad;
    const double* aDamp;
    const double* lineWave;
    const RayTrans* tr;
    const int32_t* laOff; // [Nla + 1] the transitions active at each of the context's rows, reference order
    const int32_t* laTr;
    const double* vz;     // [Ns] staged
    const double* vx;
    const double* mux;    // [nDir] staged
    const double* muz;
    double2* cs;          // [nLa, nDir, Ns] (chi, S) pairs: the layout fs2d reads
};

// The job of cont_kernel + gather2d_kernel for observer directions: one thread per (wavelength of the batch, point),
// consecutive lanes on consecutive points.  What no direction changes is fetched once per point -- the background, sca J,
// exp(-hc / k lambda T), and per transition the populations, rho, vBroad, aDamp / the nStar ratio -- and the directions are the
// inner loop: per direction only the Voigt evaluation of a line, or two additions of a continuum.  Every direction's chi and
// eta are added up in the reference's order (background, then the transitions in atom / kr order: intensity_core's gather,
// SimdFullIterationTemplates.hpp:59-179) in the thread's own column of LDS, [2 nDir][256] doubles: 4 KB for one direction,
// 64 KB for sixteen (two workgroups per CU, which is what the Faddeeva code's registers allow anyway).
__global__ void __launch_bounds__(R2G_THREADS) rays2d_gather_kernel(const Rays2dArgs a)
{
    dbg_poison_lds();
    extern __shared__ double acc[];
    const int k = blockIdx.x * R2G_THREADS + threadIdx.x;
    if (k >= a.Ns)
        return; // (no barrier below: the columns are thread-private)
    const int Ns = a.Ns, nDir = a.nDir;
    const int b = blockIdx.y;
    const int la = a.la0 + b;
    const double sqrtPi = 1.772453850905516027298167483341145182798;
    double* col = acc + threadIdx.x;
    const size_t lk = (size_t)la * Ns + k;
    const double chi0 = a.bgChi[lk], eta0 = a.bgEta[lk];
    const double sca = a.bgSca[lk] * a.J[lk];
    const double vz = a.vz[k], vx = a.vx[k];
    const double hc_kl = HC_K / CTAB(double, a.wavelength)[la];
    const double boltz = exp(-hc_kl / a.temperature[k]);
    for (int m = 0; m < nDir; ++m)
    {
        col[(size_t)(2 * m) * R2G_THREADS] = chi0;
        col[(size_t)(2 * m + 1) * R2G_THREADS] = eta0;
    }
    const int q0 = CTAB(int32_t, a.laOff)[la], q1 = CTAB(int32_t, a.laOff)[la + 1];
    for (int q = q0; q < q1; ++q)
    {
        const RayTrans t = ld_c(CTAB(RayTrans, a.tr) + CTAB(int32_t, a.laTr)[q]);
        const int l0 = la - t.Nblue;
        const CONST_AS double* p = CTAB(double, a.par) + t.parOff + 4 * (size_t)l0;
        const double ni = a.n[(size_t)t.gi * Ns + k], nj = a.n[(size_t)t.gj * Ns + k];
        if (t.type == LWHIP_LINE)
        {
            // Transition::uv (LwTransition.hpp:98-127) with gij of Atom::setup_wavelength (LwAtom.hpp:99-123); phi of
            // compute_phi_la (FormalScalar.cpp:28-51) for each direction
            const double vb = a.vBroad[(size_t)t.atom * Ns + k];
            const double ad = a.aDamp[(size_t)t.row * Ns + k];
            const double vBase = (CTAB(double, a.lineWave)[t.waveOff + t.ltStart + l0] - t.lambda0) * CLight / t.lambda0;
            const double p0 = p[0], p3 = p[3];
            double gij = p[2];
            if (t.prd)
                gij *= a.rho[t.rhoOff + (size_t)l0 * Ns + k];
            for (int m = 0; m < nDir; ++m)
            {
                const double vlos = CTAB(double, a.mux)[m] * vx + CTAB(double, a.muz)[m] * vz;
                const double vk = (vBase + vlos) / vb;
                const double phi = d_voigt_H(ad, vk) / (sqrtPi * vb);
                const double Vij = p0 * phi;
                const double Vji = gij * Vij;
                const double Uji = p3 * Vji;
                col[(size_t)(2 * m) * R2G_THREADS] += ni * Vij - nj * Vji;
                col[(size_t)(2 * m + 1) * R2G_THREADS] += nj * Uji;
            }
        }
        else
        {
            const double gij = a.ratio[(size_t)t.row * Ns + k] * boltz;
            const double Vij = p[0];
            const double Vji = gij * Vij;
            const double Uji = p[2] * Vji;
            const double dChi = ni * Vij - nj * Vji, dEta = nj * Uji;
            for (int m = 0; m < nDir; ++m)
            {
                col[(size_t)(2 * m) * R2G_THREADS] += dChi;
                col[(size_t)(2 * m + 1) * R2G_THREADS] += dEta;
            }
        }
    }
    for (int m = 0; m < nDir; ++m)
    {
        const double chi = col[(size_t)(2 * m) * R2G_THREADS], eta = col[(size_t)(2 * m + 1) * R2G_THREADS];
        a.cs[((size_t)b * nDir + m) * Ns + k] = make_double2(chi, (eta + sca) / chi);
    }
}

hipError_t launch_rays2d_gather(const Rays2dArgs& a, hipStream_t stream)
{
    const size_t lds = (size_t)2 * a.nDir * R2G_THREADS * sizeof(double);
    if (lds > 48 * 1024)
    {
        const hipError_t err = hipFuncSetAttribute((const void*)rays2d_gather_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (err != hipSuccess)
            return err;
    }
    LWHIP_LAUNCH(rays2d_gather_kernel, dim3((a.Ns + R2G_THREADS - 1) / R2G_THREADS, a.nLa), dim3(R2G_THREADS), lds, stream, a);
    return hipGetLastError();
}

// this unit's copy of the Voigt table
hipError_t rays2d_init_table(int device)
{
    static std::atomic<bool> done[64];
    if (device >= 0 && device < 64 && done[device].load())
        return hipSuccess;
    const hipError_t e = voigt_fill_table();
    if (e == hipSuccess && device >= 0 && device < 64)
        done[device].store(true);
    return e;
}

// the intersection table of a set of directions on the host
struct HostGeom
{
    std::vector<double> mux, muz;
    std::vector<lwhip_intersection> uw, dw, sub;
    std::vector<int32_t> longIdx, subOff;
    lwhip_grid2d g{};
};

int build_host_geom(const lwhip_grid2d& ctxGrid, const double* mux, const double* muz, int n, HostGeom& h, const std::string& what)
{
    h.mux.assign(mux, mux + n);
    h.muz.assign(muz, muz + n);
    h.g = ctxGrid;
    h.g.Nrays = n;
    h.g.mux = h.mux.data();
    h.g.muz = h.muz.data();
    h.g.uw = h.g.dw = h.g.substeps = nullptr;
    h.g.longCharIdx = h.g.substepOff = nullptr;
    int32_t nl = 0;
    int64_t ns = 0;
    int st = lwhip_build_intersections_impl(&h.g, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0, &nl, &ns);
    if (st != LWHIP_OK)
        return fail(LWHIP_ERR_UNSUPPORTED, what + ": a long characteristic of the requested directions does not reach a z plane");
    const size_t nSt = (size_t)n * 2 * ctxGrid.Nx * ctxGrid.Nz;
    h.uw.assign(nSt, lwhip_intersection{});
    h.dw.assign(nSt, lwhip_intersection{});
    h.longIdx.assign(nSt, -1);
    h.subOff.assign((size_t)nl + 1, 0);
    h.sub.assign((size_t)std::max<int64_t>(ns, 1), lwhip_intersection{});
    st = lwhip_build_intersections_impl(&h.g, h.uw.data(), h.dw.data(), h.longIdx.data(), h.subOff.data(), nl, h.sub.data(), ns, &nl,
                                        &ns);
    if (st != LWHIP_OK)
        return fail(LWHIP_ERR_UNSUPPORTED, what + ": a long characteristic of the requested directions does not reach a z plane");
    h.g.NlongChar = nl;
    h.g.uw = h.uw.data();
    h.g.dw = h.dw.data();
    h.g.longCharIdx = h.longIdx.data();
    h.g.substepOff = h.subOff.data();
    h.g.substeps = h.sub.data();
    if (!fs2d_long_chars_ok(&h.g))
        return fail(LWHIP_ERR_UNSUPPORTED, what + ": a long characteristic of the requested directions does not end on a z plane");
    return LWHIP_OK;
}
} // namespace

// One chunk of a view's directions on the device: its geometry tables, its ray list (the up-going rays 2 m + 1) and the rows of
// the staged lower-boundary data its rays read.  A view is one chunk unless the context's batch scratch holds fewer solves than
// the view has directions (LWHIP_BATCH2D=1 with few quadrature rays); a chunk is a grid of its own, so that the solver's
// long-characteristic pass, which numbers the up-going rays of a table from zero, needs no change.
struct Rays2dChunk
{
    Geom2dDev dev;
    DevBuf<int32_t> rayList, lowIdx;
    int m0 = 0, n = 0, NlongChar = 0;
};

// What a 2D context keeps for its observer calls: the geometry of the last view (one slot, keyed by the bits of the directions)
// and the staging of a call.
struct Rays2dState
{
    std::mutex lock;
    std::vector<uint64_t> key;
    std::vector<std::unique_ptr<Rays2dChunk>> chunks;
    DevBuf<double> lc;                 // [wavelengths of a batch][NlongChar of the chunk][3]: the observer's own
    DevBuf<unsigned char> in;          // [vz | vx | mux | muz | lowerBc]
    DevBuf<double> out;                // [nla, Nmu, Nx]
    PinnedBlock inPinned, outPinned;
};

void rays2d_release(Rays2dState* s)
{
    if (s)
    {
        s->inPinned.release();
        s->outPinned.release();
    }
    delete s;
}

namespace
{
std::mutex g_rays2dCreate;

Rays2dState* rays2d_state(Rays2dState*& slot)
{
    std::lock_guard<std::mutex> g(g_rays2dCreate);
    if (!slot)
        slot = new Rays2dState();
    return slot;
}

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

uint64_t bits_of(double v)
{
    uint64_t u;
    std::memcpy(&u, &v, sizeof(u));
    return u;
}

int rays2d_run(lwhip_context* c, const lwhip_rays2d* r, const std::string& what)
{
    // ---- every refusal, before anything is queued ----------------------------------------------------------------------------
    if (!c->is2d)
        return fail(LWHIP_ERR_UNSUPPORTED, what + ": a 1D context (lwhip_compute_rays serves those)");
    const lwhip_grid2d& g = *c->prob.grid2d;
    if (!g.periodic)
        return fail(LWHIP_ERR_UNSUPPORTED, what + ": fixed (CALLABLE) x boundaries have no data for new directions");
    if (r->Nmu < 1 || !r->muz || !r->mux || !r->vz || !r->vx || !r->I)
        return fail(LWHIP_ERR_INVALID, what + ": Nmu >= 1, muz, mux, vz, vx and I are required");
    if (r->Nmu > LWHIP_RAYS_MAX_MU)
        return fail(LWHIP_ERR_UNSUPPORTED, what + ": Nmu above LWHIP_RAYS_MAX_MU (" + std::to_string(LWHIP_RAYS_MAX_MU)
                                               + " directions per call)");
    for (int m = 0; m < r->Nmu; ++m)
    {
        if (!(r->muz[m] > 0.0 && r->muz[m] <= 1.0))
            return fail(LWHIP_ERR_INVALID, what + ": muz of direction " + std::to_string(m) + " is outside (0, 1]");
        if (!(r->muz[m] * r->muz[m] + r->mux[m] * r->mux[m] <= 1.0 + 1e-12))
            return fail(LWHIP_ERR_INVALID, what + ": direction " + std::to_string(m) + " has muz^2 + mux^2 > 1");
    }
    const int la0 = (r->laStart == 0 && r->laEnd == 0) ? c->laStart : r->laStart;
    const int la1 = (r->laEnd == 0) ? c->laEnd : r->laEnd;
    if (la0 < c->laStart || la1 > c->laEnd || la1 <= la0)
        return fail(LWHIP_ERR_INVALID, what + ": wavelength range [" + std::to_string(la0) + ", " + std::to_string(la1)
                                           + ") is not inside the context's rows [" + std::to_string(c->laStart) + ", "
                                           + std::to_string(c->laEnd) + ")");
    const bool lowCallable = c->prob.zLowerBc.type == LWHIP_BC_CALLABLE;
    if (lowCallable && !r->lowerBc)
        return fail(LWHIP_ERR_INVALID, what + ": a CALLABLE lower boundary has no data for new directions (pass lowerBc [Nla, Nmu, Nx])");
    for (const HostTrans& h : c->trans)
        if (h.t.type == LWHIP_LINE && !h.t.aDamp)
            return fail(LWHIP_ERR_INVALID, what + ": needs aDamp for every line (the profiles are evaluated in the kernel)");
    const int Ns = c->Ns, Nx = c->Nx, Nmu = r->Nmu, nla = la1 - la0;
    // the batch scratch holds batch2d x 2 Nrays solves of the context's own iteration
    const int capacity = c->batch2d * 2 * c->Nrays;
    const int chunkN = std::min(Nmu, capacity);
    const int nLaBatch = std::max(1, capacity / chunkN);
    HIP_TRY(hipSetDevice(c->device));
    Rays2dState& st = *rays2d_state(c->rays2d);
    std::lock_guard<std::mutex> guard(st.lock);
    // ---- the geometry of the view: cached, or built on the host (still nothing queued: a table may be refused) ---------------
    std::vector<uint64_t> key;
    key.push_back((uint64_t)Nmu);
    key.push_back((uint64_t)chunkN);
    for (int m = 0; m < Nmu; ++m)
        key.push_back(bits_of(r->muz[m]));
    for (int m = 0; m < Nmu; ++m)
        key.push_back(bits_of(r->mux[m]));
    const bool cached = !st.chunks.empty() && st.key == key;
    std::vector<HostGeom> host;
    if (!cached)
    {
        host.resize((Nmu + chunkN - 1) / chunkN);
        for (size_t q = 0; q < host.size(); ++q)
        {
            const int m0 = (int)q * chunkN, n = std::min(chunkN, Nmu - m0);
            const int sg = build_host_geom(g, r->mux + m0, r->muz + m0, n, host[q], what);
            if (sg != LWHIP_OK)
                return sg;
        }
    }
    HIP_TRY(rays2d_init_table(c->device));
    lwhip_context* owner = c->tablesFrom ? c->tablesFrom : c;
    RaysState* tabs = nullptr;
    const int stp = rays_tables(owner, tabs);
    if (stp != LWHIP_OK)
        return stp;
    if (!cached)
    {
        HIP_TRY(hipStreamSynchronize(c->stream)); // (the previous view's tables may still be read)
        st.chunks.clear();
        st.key.clear();
        size_t maxLong = 0;
        for (size_t q = 0; q < host.size(); ++q)
        {
            std::unique_ptr<Rays2dChunk> ch(new Rays2dChunk());
            ch->m0 = (int)q * chunkN;
            ch->n = host[q].g.Nrays;
            ch->NlongChar = host[q].g.NlongChar;
            const int su = geom2d_upload(c->mem, host[q].g, ch->dev);
            if (su != LWHIP_OK)
                return su;
            std::vector<int32_t> rays(ch->n), idx((size_t)2 * ch->n, -1);
            for (int m = 0; m < ch->n; ++m)
            {
                rays[m] = 2 * m + 1;
                idx[2 * (size_t)m + 1] = ch->m0 + m; // idxs[m, toObs]: the direction's row of the staged lowerBc
            }
            HIP_TRY(ch->rayList.upload(c->mem, rays));
            HIP_TRY(ch->lowIdx.upload(c->mem, idx));
            maxLong = std::max(maxLong, (size_t)ch->NlongChar);
            st.chunks.push_back(std::move(ch));
        }
        const size_t lcNeed = (size_t)nLaBatch * maxLong * 3;
        if (st.lc.n < lcNeed)
            HIP_TRY(st.lc.alloc(c->mem, lcNeed));
        HIP_TRY(hipStreamSynchronize(c->stream)); // (the host tables go when this function returns)
        st.key = key;
    }
    // ---- the staged request: [vz | vx | mux | muz | lowerBc], one copy up -----------------------------------------------------
    const size_t offVz = 0, offVx = align256((size_t)Ns * sizeof(double)), offMux = 2 * offVx;
    const size_t offMuz = offMux + align256((size_t)Nmu * sizeof(double)), offBc = offMuz + align256((size_t)Nmu * sizeof(double));
    const size_t nOut = (size_t)nla * Nmu * Nx;
    const size_t inBytes = offBc + (lowCallable ? align256(nOut * sizeof(double)) : 0);
    if (st.in.n < inBytes || st.out.n < nOut)
    {
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (st.in.n < inBytes)
            HIP_TRY(st.in.alloc(c->mem, inBytes, false));
        if (st.out.n < nOut)
            HIP_TRY(st.out.alloc(c->mem, nOut, false));
    }
    HIP_TRY(st.inPinned.reserve(c->device, inBytes, c->stream));
    HIP_TRY(st.outPinned.reserve(c->device, nOut * sizeof(double), c->stream));
    unsigned char* hin = st.inPinned.as<unsigned char>();
    std::memcpy(hin + offVz, r->vz, (size_t)Ns * sizeof(double));
    std::memcpy(hin + offVx, r->vx, (size_t)Ns * sizeof(double));
    std::memcpy(hin + offMux, r->mux, (size_t)Nmu * sizeof(double));
    std::memcpy(hin + offMuz, r->muz, (size_t)Nmu * sizeof(double));
    if (lowCallable)
        std::memcpy(hin + offBc, r->lowerBc, nOut * sizeof(double));
    HIP_TRY(c->mem.h2d(st.in.p, hin, inBytes));
    // ---- the launches: per chunk of directions, per batch of wavelengths: gather -> fs2d (up-going rays) -> top plane out ------
    Rays2dArgs ga{};
    ga.Ns = Ns;
    ga.temperature = c->temperature.p;
    ga.wavelength = c->wavelength.p;
    ga.bgChi = c->bgChi.p;
    ga.bgEta = c->bgEta.p;
    ga.bgSca = c->bgSca.p;
    ga.J = c->J.p;
    ga.n = c->n.p;
    ga.ratio = c->ratio.p;
    ga.par = c->par.p;
    ga.rho = c->rho.p;
    ga.vBroad = c->vBroad.p;
    ga.aDamp = c->aDamp.p;
    ga.lineWave = c->lineWave.p;
    ga.tr = tabs->tr.p;
    ga.laOff = tabs->laOff.p;
    ga.laTr = tabs->laTr.p;
    ga.vz = (const double*)(st.in.p + offVz);
    ga.vx = (const double*)(st.in.p + offVx);
    ga.cs = (double2*)c->b2cs.p;
    Fs2dArgs f{};
    f.Nx = g.Nx;
    f.rNx = 1.0f / (float)g.Nx;
    f.Nz = g.Nz;
    f.zLowerBc = g.zLowerBc;
    f.zUpperBc = g.zUpperBc == LWHIP_BC_CALLABLE ? LWHIP_BC_ZERO : g.zUpperBc; // (an up-going ray never reads it)
    f.periodic = 1;
    f.zNmuLow = Nmu;
    f.zbcLow = lowCallable ? (const double*)(st.in.p + offBc) : nullptr;
    f.temperature = c->temperature.p;
    f.lcUpOnly = 1;
    f.cs = (const double2*)c->b2cs.p;
    f.I = c->b2I.p;
    f.PsiStar = c->b2Psi.p;
    f.coef = c->b2coef.p;
    f.cidx = c->b2idx.p;
    Batch2dArgs oa{}; // what iout2d_kernel reads: the top plane of every solve to out[la, m0 + m, x]
    oa.Ns = Ns;
    oa.Nx = Nx;
    oa.Nrays = Nmu;
    oa.I = c->b2I.p;
    const int loc0 = la0 - c->laStart;
    for (const auto& chp : st.chunks)
    {
        const Rays2dChunk& ch = *chp;
        ga.nDir = ch.n;
        ga.mux = (const double*)(st.in.p + offMux) + ch.m0;
        ga.muz = (const double*)(st.in.p + offMuz) + ch.m0;
        f.Nrays = ch.n;
        f.nRayCycle = ch.n;
        f.mux = ch.dev.mux.p;
        f.zIdxLow = ch.lowIdx.p;
        f.uw = ch.dev.uw.p;
        f.dw = ch.dev.dw.p;
        f.uwS = ch.dev.uwS.p;
        f.dwS = ch.dev.dwS.p;
        f.uwA = ch.dev.uwA.p;
        f.dwA = ch.dev.dwA.p;
        f.nRec = (size_t)2 * ch.n * Ns;
        f.longCharIdx = ch.dev.longIdx.p;
        f.substepOff = ch.dev.subOff.p;
        f.substeps = ch.dev.sub.p;
        f.NlongChar = ch.NlongChar;
        f.lcOwner = ch.dev.lcOwner.p;
        f.lcBuf = ch.NlongChar > 0 ? st.lc.p : nullptr;
        f.rays = ch.rayList.p;
        oa.nRaysActive = ch.n;
        oa.rayList = ch.rayList.p;
        oa.Iout = st.out.p + (size_t)ch.m0 * Nx;
        for (int b0 = 0; b0 < nla; b0 += nLaBatch)
        {
            const int nLa = std::min(nLaBatch, nla - b0);
            ga.la0 = loc0 + b0;
            ga.nLa = nLa;
            HIP_TRY(launch_rays2d_gather(ga, c->stream));
            f.wavs = c->wavelength.p + loc0 + b0;
            f.la0 = b0; // (row of the staged boundary data)
            f.nSolve = nLa * ch.n;
            HIP_TRY(launch_fs2d(f, nLa * ch.n, c->stream));
            oa.la0 = b0;
            oa.nLa = nLa;
            HIP_TRY(launch_iout2d(oa, c->stream));
        }
    }
    // ---- one copy back, one wait ---------------------------------------------------------------------------------------------
    double* hout = st.outPinned.as<double>();
    HIP_TRY(hipMemcpyAsync(hout, st.out.p, nOut * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    std::memcpy(r->I, hout, nOut * sizeof(double));
    return LWHIP_OK;
}
} // namespace
} // namespace lwhip

extern "C"
{
int lwhip_compute_rays_2d(lwhip_context* c, const lwhip_rays2d* rays)
{
    if (!c)
        return fail(LWHIP_ERR_INVALID, "lwhip_compute_rays_2d: null context");
    if (!rays)
        return fail(LWHIP_ERR_INVALID, "lwhip_compute_rays_2d: null request");
    if (lwhip_device_count() <= 0)
        return fail(LWHIP_ERR_DEVICE, "lwhip_compute_rays_2d: no gfx950 device");
    return rays2d_run(c, rays, "lwhip_compute_rays_2d");
}
}
