// lwhip_rays.hip -- emergent intensity along observer rays (1D plane-parallel): what LwContext.compute_rays(mus, upOnly=True)
// (Source/LwMiddleLayer.pyx:3898-4002) computes, from the state that is resident on the device.  lwhip_compute_rays for one
// context, lwhip_batch_compute_rays for every column of a 1.5D batch.
//
// The reference copies the problem, replaces its rays, makes a second context, recomputes and stores phi for the new rays
// and runs formal_sol.  Here nothing is created: the directions are not quadrature nodes, so the stored phi does not
// apply, and instead of storing another one the kernel evaluates phi = H(a, v) / (sqrt(pi) vBroad) where it gathers,
// v = ((lambda - lambda0) c / lambda0 + mu v_z) / vBroad (the to-observer sign of voigt_phi_kernel).  No phi pool, no rows in
// HBM, no second context; the context's own phi, wphi, I, J, Gamma and rates are not touched.
//
// rays_kernel: one launch for the whole call.  A workgroup of 256 threads owns R consecutive rays (lambda, mu) of one
// column, the column outermost in the grid.  Its R x Ns depth points are spread over the threads -- depth across lanes: the
// Voigt evaluations, the expensive part, are independent per depth point, and n, aDamp, vBroad and the background rows are
// read along k -- in five passes through LDS separated by barriers:
//   1  chi and S of every point (intensity_core's gather, SimdFullIterationTemplates.hpp:59-179, with the in-kernel phi);
//   2  the Steffen derivative of chi at every point (linear at the two ends);
//   3  the optical depth of every interval (Bezier3 control points), the upwind intensity of the lower boundary;
//   4  the derivative of S in optical depth at every point;
//   5  the five terms of every point's step: I_k = I_uw edt + alpha S_uw + beta S_k + gamma C_uw + delta C_0;
// then one lane per ray adds them up the atmosphere in the reference's order (piecewise_bezier3_1d_impl,
// FormalScalar.cpp:209-325: five dependent operations per depth point) and stores I(k = 0).  Every quantity is formed by
// the operations of the serial algorithm, only not in its order in time.  R is chosen by the host so that R x Ns fills
// whole passes of 256 threads within 40 KB of LDS (eight arrays of R x Ns doubles): 6 rays at 82 depth points.
//
// lwhip_compute_rays_grid / lwhip_batch_compute_rays_grid: the same on a wavelength grid of the caller's choice.  The kernel's
// row sources are pointers of the column's record; for a new grid they point at the request's rows (staged background, par and
// transition records; J and rho interpolated on the device by rays_grid_rows_kernel) instead of the context's.
//
// lwhip_compute_rays_hprd and its three kin: the same four calls for contexts with hybrid-PRD tables, which the plain ones refuse.
// The reference's second context runs configure_hprd_coeffs on the new rays; rays_kernel<true> forms that coefficient where it
// gathers (d_hprd_rho_coeff, lwhip_device.h) and interpolates the line's rest-frame rho with it.  Same driver, same staging.
#include "lwhip_host.h"
#include "lwhip_device.h"
// H(a, v) under the same contraction setting as the stored profiles' unit: the same argument gives the same bits
#include "lwhip_voigt_dev.h"

// As in lwhip_stokes_fs.hip: no fused multiply-adds from here on, so that the operations match the reference's one for one.
#pragma clang fp contract(off)

#include <algorithm>
#include <atomic>
#include <cstring>
#include <mutex>
#include <vector>

namespace lwhip
{
namespace
{
enum { RAYS_THREADS = 256, RAYS_ARRAYS = 8, RAYS_MAX_NS = 1024, RAYS_LDS_TARGET = 40 << 10 };

// one column: the context's resident state, the request's staged inputs and its outputs
struct RayCol
{
    const double* height;
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
    const double* vlosMu;
    const double* muzCtx;
    const double* vBroad;
    const double* aDamp;
    const double* lineWave;
    const RayTrans* tr;
    const int32_t* laOff; // [Nla + 1] the transitions active at each of the context's rows, reference order
    const int32_t* laTr;
    const double* vz;      // [Ns] staged, or null: vlosMu[0] / muz[0] of the resident atmosphere
    const double* lowerBc; // [nla, Nmu] staged (CALLABLE lower boundary)
    double* I;             // [nla, Nmu]
    double* depthChi;      // [nla, Nmu, Ns] each, or null
    double* depthEta;
    double* depthI;
    int32_t lowerType, _pad;
    double mu[LWHIP_RAYS_MAX_MU];
};

struct RaysArgs
{
    const RayCol* cols;
    int32_t Ns, Nmu, la0, nla; // la0: first row of the context's grid
    int32_t R, blocksPerCol;
};

// HYBRID: the context carries hybrid-PRD tables (lwhip_compute_rays_hprd and its kin).  rho of a line of the hybrid list is then
// not the row's but what Transition::uv (LwTransition.hpp:116-127) interpolates from the line's rest-frame rho, with the
// coefficient configure_hprd_coeffs (Prd.cpp:899-939) forms for this direction and depth -- formed here, where it is used,
// like phi.  The line's grid is read from global memory: a few hundred doubles that every lane of the launch shares.  The
// false instance reads nothing of this.
template <bool HYBRID> __global__ void __launch_bounds__(RAYS_THREADS) rays_kernel(const RaysArgs g)
{
    dbg_poison_lds();
    extern __shared__ double lds[];
    const int Ns = g.Ns, Nmu = g.Nmu;
    const RayCol* a = g.cols + blockIdx.x / g.blocksPerCol;
    const int ray0 = (blockIdx.x % g.blocksPerCol) * g.R;
    const int nRay = min(g.R, g.nla * Nmu - ray0);
    const int nPt = nRay * Ns;
    const size_t W = (size_t)g.R * Ns;
    double* sChi = lds;         // chi; from pass 5 on: edt of the step into k, then I(k)
    double* sS = lds + W;       // S
    double* sD = lds + 2 * W;   // d chi / ds; from pass 5 on: the step's first term
    double* sTau = lds + 3 * W; // [k] optical depth of the interval k + 1 -> k; [Ns - 1]: of the last step's linear rule
    double* sDS = lds + 4 * W;  // [k] dS / dtau at k (k >= 1); [0]: the upwind intensity at the lower boundary
    double* sT2 = lds + 5 * W;
    double* sT3 = lds + 6 * W;
    double* sT4 = lds + 7 * W;
    const double* h = a->height;

    // ---- 1: chi and S ---------------------------------------------------------------------------------------------------
    {
        const double sqrtPi = 1.772453850905516027298167483341145182798;
        const double* temperature = a->temperature;
        const double* nPool = a->n;
        const double* par = a->par;
        const double* vBroad = a->vBroad;
        const double* aDamp = a->aDamp;
        const double* lineWave = a->lineWave;
        const RayTrans* tr = a->tr;
        const int32_t* laOff = a->laOff;
        const int32_t* laTr = a->laTr;
        const double* vzIn = a->vz;
        for (int idx = threadIdx.x; idx < nPt; idx += RAYS_THREADS)
        {
            const int r = idx / Ns, k = idx - r * Ns;
            const int ray = ray0 + r;
            const int l = ray / Nmu, m = ray - l * Nmu;
            const int la = g.la0 + l;
            const double vz = vzIn ? vzIn[k] : a->vlosMu[k] / a->muzCtx[0];
            const double vlos = a->mu[m] * vz;
            const double T = temperature[k];
            const size_t lk = (size_t)la * Ns + k;
            double chi = a->bgChi[lk], eta = a->bgEta[lk];
            for (int q = laOff[la]; q < laOff[la + 1]; ++q)
            {
                const RayTrans t = tr[laTr[q]];
                const int l0 = la - t.Nblue;
                const double* p = par + t.parOff + 4 * (size_t)l0;
                double Vij, Vji, Uji;
                if (t.type == LWHIP_LINE)
                {
                    // Transition::uv (LwTransition.hpp:98-127) with gij of Atom::setup_wavelength (LwAtom.hpp:99-123); phi of
                    // compute_phi_la (FormalScalar.cpp:28-51) for this direction
                    const double vb = vBroad[(size_t)t.atom * Ns + k];
                    const double vBase = (lineWave[t.waveOff + t.ltStart + l0] - t.lambda0) * CLight / t.lambda0;
                    const double vk = (vBase + vlos) / vb;
                    const double phi = d_voigt_H(aDamp[(size_t)t.row * Ns + k], vk) / (sqrtPi * vb);
                    Vij = p[0] * phi;
                    double gij = p[2];
                    if (HYBRID && t.hybrid)
                    {
                        // (gij stays Bji / Bij, LwAtom.hpp:118-123; rho multiplies Vji, LwTransition.hpp:118-126)
                        // lambdaRest of the line's own-grid point for this ray (toObs = 1), in the reference's order
                        const double* w = lineWave + t.waveOff;
                        const double lambdaRest = w[t.ltStart + l0] * (1.0 + vlos * 1.0 / CLight);
                        int i0, i1;
                        double frac;
                        d_hprd_rho_coeff(w, t.nlt, lambdaRest, i0, i1, frac);
                        const double* rho0 = a->rho + t.rho0Off + k;
                        const double rho = (1.0 - frac) * rho0[(size_t)i0 * Ns] + frac * rho0[(size_t)i1 * Ns];
                        Vji = gij * Vij;
                        Vji *= rho;
                    }
                    else
                    {
                        if (t.prd)
                            gij *= a->rho[t.rhoOff + (size_t)l0 * Ns + k];
                        Vji = gij * Vij;
                    }
                    Uji = p[3] * Vji;
                }
                else
                {
                    const double hc_kl = HC_K / a->wavelength[la];
                    const double gij = a->ratio[(size_t)t.row * Ns + k] * exp(-hc_kl / T);
                    Vij = p[0];
                    Vji = gij * Vij;
                    Uji = p[2] * Vji;
                }
                const double ni = nPool[(size_t)t.gi * Ns + k], nj = nPool[(size_t)t.gj * Ns + k];
                chi += ni * Vij - nj * Vji;
                eta += nj * Uji;
            }
            sChi[idx] = chi;
            sS[idx] = (eta + a->bgSca[lk] * a->J[lk]) / chi;
            if (a->depthChi)
            {
                // (rays are consecutive in the output: [nla, Nmu, Ns])
                a->depthChi[(size_t)ray0 * Ns + idx] = chi;
                a->depthEta[(size_t)ray0 * Ns + idx] = eta;
            }
        }
    }
    __syncthreads();
    // The ray goes up: from k = Ns - 1 (upwind end) to k = 0; the upwind neighbour of k is k + 1.
    // ---- 2: d chi / ds (cent_deriv inside, the one-sided difference at the two ends) -------------------------------------
    for (int idx = threadIdx.x; idx < nPt; idx += RAYS_THREADS)
    {
        const int r = idx / Ns, k = idx - r * Ns;
        const double zmu = 1.0 / a->mu[(ray0 + r) % Nmu];
        const double* c = sChi + r * Ns;
        double D;
        if (k == Ns - 1)
            D = (c[Ns - 2] - c[Ns - 1]) / (fabs(h[Ns - 2] - h[Ns - 1]) * zmu);
        else if (k == 0)
            D = (c[0] - c[1]) / (fabs(h[0] - h[1]) * zmu);
        else
            D = d_cent_deriv(fabs(h[k] - h[k + 1]) * zmu, fabs(h[k - 1] - h[k]) * zmu, c[k + 1], c[k], c[k - 1]);
        sD[idx] = D;
    }
    __syncthreads();
    // ---- 3: optical depths; the upwind intensity ---------------------------------------------------------------------------
    for (int idx = threadIdx.x; idx < nPt; idx += RAYS_THREADS)
    {
        const int r = idx / Ns, k = idx - r * Ns;
        const int ray = ray0 + r;
        const int l = ray / Nmu, m = ray - l * Nmu;
        const double zmu = 1.0 / a->mu[m];
        const double* c = sChi + r * Ns;
        const double* D = sD + r * Ns;
        if (k < Ns - 1)
        {
            const double ds = fabs(h[k] - h[k + 1]) * zmu;
            const double Cuw = c[k + 1] + (ds / 3.0) * D[k + 1];
            const double C0 = c[k] - (ds / 3.0) * D[k];
            sTau[idx] = ds * (c[k] + c[k + 1] + Cuw + C0) * 0.25;
        }
        else
        {
            // the last step (into k = 0) is linear; the boundary (FormalScalar.cpp:551-597)
            sTau[idx] = 0.5 * zmu * (c[0] + c[1]) * fabs(h[0] - h[1]);
            double Iupw = 0.0;
            if (a->lowerType == LWHIP_BC_THERMALISED)
            {
                const double dtau_uw = 0.5 * zmu * (c[Ns - 1] + c[Ns - 2]) * fabs(h[Ns - 1] - h[Ns - 2]);
                const double wav = a->wavelength[g.la0 + l];
                const double B0 = d_planck(a->temperature[Ns - 2], wav), B1 = d_planck(a->temperature[Ns - 1], wav);
                Iupw = B1 - (B0 - B1) / dtau_uw;
            }
            else if (a->lowerType == LWHIP_BC_CALLABLE)
                Iupw = a->lowerBc[ray];
            sDS[r * Ns] = Iupw;
        }
    }
    __syncthreads();
    // ---- 4: dS / dtau ------------------------------------------------------------------------------------------------------
    for (int idx = threadIdx.x; idx < nPt; idx += RAYS_THREADS)
    {
        const int r = idx / Ns, k = idx - r * Ns;
        const double* S = sS + r * Ns;
        const double* tau = sTau + r * Ns;
        if (k == Ns - 1)
            sDS[idx] = (S[Ns - 2] - S[Ns - 1]) / tau[Ns - 2];
        else if (k > 0)
            sDS[idx] = d_cent_deriv(tau[k], tau[k - 1], S[k + 1], S[k], S[k - 1]);
    }
    __syncthreads();
    // ---- 5: the terms of every step (nothing below reads chi or its derivative: their arrays take the first two) ------------
    for (int idx = threadIdx.x; idx < nPt; idx += RAYS_THREADS)
    {
        const int r = idx / Ns, k = idx - r * Ns;
        const double* S = sS + r * Ns;
        const double* tau = sTau + r * Ns;
        const double* DS = sDS + r * Ns;
        if (k == Ns - 1)
            continue;
        double E, t1, t2, t3 = 0.0, t4 = 0.0;
        if (k > 0)
        {
            const double dt = tau[k];
            double alpha, beta, gamma, delta, edt;
            d_bezier3_coeffs(dt, alpha, beta, gamma, delta, edt);
            const double Cuw = S[k + 1] + (dt / 3.0) * DS[k + 1];
            const double C0 = S[k] - (dt / 3.0) * DS[k];
            E = edt;
            t1 = alpha * S[k + 1];
            t2 = beta * S[k];
            t3 = gamma * Cuw;
            t4 = delta * C0;
        }
        else
        {
            const double dt = tau[Ns - 1];
            const double dS_uw = (S[0] - S[1]) / dt;
            double w0, w1;
            d_w2(dt, w0, w1);
            E = 1.0 - w0;
            t1 = w0 * S[0];
            t2 = -(w1 * dS_uw);
        }
        sChi[idx] = E;
        sD[idx] = t1;
        sT2[idx] = t2;
        sT3[idx] = t3;
        sT4[idx] = t4;
    }
    __syncthreads();
    // ---- the recurrence: one lane per ray ------------------------------------------------------------------------------------
    if ((int)threadIdx.x < nRay)
    {
        const int o = threadIdx.x * Ns;
        double I = sDS[o];
        sChi[o + Ns - 1] = I;
        for (int k = Ns - 2; k >= 0; --k)
        {
            I = I * sChi[o + k] + sD[o + k] + sT2[o + k] + sT3[o + k] + sT4[o + k];
            sChi[o + k] = I;
        }
        a->I[ray0 + threadIdx.x] = I;
    }
    if (a->depthI)
    {
        __syncthreads();
        for (int idx = threadIdx.x; idx < nPt; idx += RAYS_THREADS)
            a->depthI[(size_t)ray0 * Ns + idx] = sChi[idx];
    }
}

// rays per workgroup: the R whose R x Ns points waste the fewest lanes of the passes, the largest such R, within the LDS target
int rays_per_group(int Ns)
{
    int best = 1;
    double bestUse = 0.0;
    for (int R = 1; R <= 64 && (size_t)R * Ns * RAYS_ARRAYS * sizeof(double) <= (size_t)RAYS_LDS_TARGET; ++R)
    {
        const int pts = R * Ns;
        const double use = (double)pts / (double)(((pts + RAYS_THREADS - 1) / RAYS_THREADS) * RAYS_THREADS);
        if (use >= bestUse)
        {
            bestUse = use;
            best = R;
        }
    }
    return best;
}
} // namespace

void rays_release(RaysState* s)
{
    if (s)
    {
        s->inPinned.release();
        s->outPinned.release();
    }
    delete s;
}

// Every refusal of a request, before anything is queued.  la0 / la1: the rows of the global grid.  (Shared with the full-Stokes
// observer rays, lwhip_stokes_fs.hip: anySolver.)
int rays_check(lwhip_context* c, const lwhip_rays* r, const std::string& what, bool anySolver, int& la0, int& la1, bool hybrid)
{
    if (!c)
        return fail(LWHIP_ERR_INVALID, what + ": null context");
    if (!r)
        return fail(LWHIP_ERR_INVALID, what + ": null request");
    if (c->is2d)
        return fail(LWHIP_ERR_UNSUPPORTED, what + ": observer rays are 1D plane-parallel only");
    if (c->hprd && !hybrid)
        return fail(LWHIP_ERR_UNSUPPORTED, what + ": not with hybrid PRD tables (rho there is tied to the quadrature rays; the "
                                               "_hprd form of this call interpolates it for the new ones)");
    if (!c->hprd && hybrid)
        return fail(LWHIP_ERR_INVALID, what + ": the context has no hybrid PRD tables (lwhip_options.hprd); its observer rays are "
                                           "those of the call without _hprd");
    if (!anySolver && c->prob.formalSolver != LWHIP_FS_BEZIER3_1D)
        return fail(LWHIP_ERR_UNSUPPORTED, what + ": piecewise_bezier3_1d contexts only");
    if (c->Ns < 3)
        return fail(LWHIP_ERR_INVALID, what + ": needs at least 3 depth points");
    if (c->Ns > RAYS_MAX_NS) // (lwhip_create admits no deeper 1D column: a guard for the LDS rows, should that change)
        return fail(LWHIP_ERR_UNSUPPORTED, what + ": more than " + std::to_string((int)RAYS_MAX_NS) + " depth points");
    if (r->Nmu < 1 || !r->muz || !r->I)
        return fail(LWHIP_ERR_INVALID, what + ": Nmu >= 1, muz and I are required");
    if (r->Nmu > LWHIP_RAYS_MAX_MU)
        return fail(LWHIP_ERR_UNSUPPORTED, what + ": Nmu above LWHIP_RAYS_MAX_MU (" + std::to_string(LWHIP_RAYS_MAX_MU)
                                               + " directions per call)");
    for (int m = 0; m < r->Nmu; ++m)
        if (!(r->muz[m] > 0.0 && r->muz[m] <= 1.0))
            return fail(LWHIP_ERR_INVALID, what + ": direction cosine " + std::to_string(m) + " is outside (0, 1]");
    la0 = (r->laStart == 0 && r->laEnd == 0) ? c->laStart : r->laStart;
    la1 = (r->laEnd == 0) ? c->laEnd : r->laEnd;
    if (la0 < c->laStart || la1 > c->laEnd || la1 <= la0)
        return fail(LWHIP_ERR_INVALID, what + ": wavelength range [" + std::to_string(la0) + ", " + std::to_string(la1)
                                           + ") is not inside the context's rows [" + std::to_string(c->laStart) + ", "
                                           + std::to_string(c->laEnd) + ")");
    if (c->prob.zLowerBc.type == LWHIP_BC_CALLABLE && !r->lowerBc)
        return fail(LWHIP_ERR_INVALID, what + ": a CALLABLE lower boundary has no data for new directions (pass lowerBc [Nla, Nmu])");
    const int nDepth = (r->depthChi ? 1 : 0) + (r->depthEta ? 1 : 0) + (r->depthI ? 1 : 0);
    if (nDepth != 0 && nDepth != 3)
        return fail(LWHIP_ERR_INVALID, what + ": depthChi, depthEta and depthI go together");
    if (!r->vz && !c->prob.vlosMu)
        return fail(LWHIP_ERR_INVALID, what + ": needs vz, or vlosMu in the descriptor");
    for (const HostTrans& h : c->trans)
        if (h.t.type == LWHIP_LINE && !h.t.aDamp)
            return fail(LWHIP_ERR_INVALID, what + ": needs aDamp for every line (the profiles are evaluated in the kernel)");
    return LWHIP_OK;
}

namespace
{
std::mutex g_raysCreate;

RaysState* rays_state(RaysState*& slot)
{
    std::lock_guard<std::mutex> g(g_raysCreate);
    if (!slot)
        slot = new RaysState();
    return slot;
}

hipError_t rays_init_table(int device)
{
    static std::atomic<bool> done[64];
    if (device >= 0 && device < 64 && done[device].load())
        return hipSuccess;
    const hipError_t e = voigt_fill_table();
    if (e == hipSuccess && device >= 0 && device < 64)
        done[device].store(true);
    return e;
}

// transition `tr` is in the context's hybrid line list (what configure_hprd_coeffs covered: plan_hybrid_prd); a PRD line outside
// it keeps rho by row, as Transition::uv does where hPrdCoeffs is empty
bool rays_hybrid_line(const lwhip_context* c, size_t tr)
{
    return c->hprd && tr < c->hRhoOffHost.size() && c->hRhoOffHost[tr] >= 0;
}
} // namespace

// the gather tables of `o` (a table owner), made on first use
int rays_tables(lwhip_context* o, RaysState*& out)
{
    RaysState* s = rays_state(o->rays);
    out = s;
    std::lock_guard<std::mutex> g(s->lock);
    if (s->built)
        return LWHIP_OK;
    const int Ns = o->Ns;
    std::vector<RayTrans> trs(std::max<size_t>(o->trans.size(), 1));
    const std::vector<LineEval> ev = line_eval_records(o->trans);
    for (size_t i = 0; i < o->trans.size(); ++i)
    {
        const HostTrans& h = o->trans[i];
        RayTrans& t = trs[i];
        t = RayTrans{};
        t.type = h.t.type;
        t.gi = o->levelOff[h.atom] + h.t.i;
        t.gj = o->levelOff[h.atom] + h.t.j;
        t.Nblue = h.NblueLoc;
        t.prd = (h.t.type == LWHIP_LINE && h.t.prd && h.rhoOff >= 0) ? 1 : 0;
        t.row = ev[i].row;
        t.atom = ev[i].atom;
        t.ltStart = ev[i].ltStart;
        t.parOff = h.parOff;
        t.rhoOff = h.rhoOff >= 0 ? h.rhoOff + (int64_t)(h.ltStart - h.rhoLt0) * Ns : 0;
        t.waveOff = ev[i].waveOff;
        t.lambda0 = ev[i].lambda0;
        if (t.prd && rays_hybrid_line(o, i))
        {
            // (rho of a hybrid line is resident for its whole grid, rhoLt0 = 0: plan_transition_list)
            t.hybrid = 1;
            t.nlt = h.t.Nred - h.t.Nblue;
            t.rho0Off = h.rhoOff;
        }
    }
    std::vector<int32_t> laOff, laTr;
    active_trans_lists(o->trans, o->Nla, true, laOff, laTr);
    HIP_TRY(hipSetDevice(o->device));
    // (outside any arena and any gathered upload: the tables outlive lwhip_create)
    HIP_TRY(s->tr.upload(o->mem, trs));
    HIP_TRY(s->laOff.upload(o->mem, laOff));
    HIP_TRY(s->laTr.upload(o->mem, laTr));
    HIP_TRY(hipStreamSynchronize(o->stream)); // (borrowers may run on other streams)
    s->built = true;
    return LWHIP_OK;
}

namespace
{
size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// what a column's outputs take in the `out` buffer: I [nla, Nmu], then chi, eta, I(k) [nla, Nmu, Ns] each
size_t rays_out_bytes(size_t nRayCol, int Ns, bool depth) { return (nRayCol + (depth ? 3 * nRayCol * Ns : 0)) * sizeof(double); }

// The end of a call: the staged block (st.inPinned, whose first bytes are the columns' RayCol records) goes up in one copy,
// one launch of rays_kernel over rows [la0, la0 + nla) of what the records point at, one copy back, one wait, and every
// column's outputs into its request's arrays.  `pre`: queued between the copy and the launch (the rows a new grid needs).
template <typename Pre>
int rays_launch_fetch(lwhip_context* c0, RaysState& st, const std::vector<const lwhip_rays*>& reqs, int Ns, int Nmu, int la0,
                      int nla, size_t inBytes, const std::string& what, bool hybrid, Pre pre)
{
    const int n = (int)reqs.size();
    const bool depth = reqs[0]->depthI != nullptr;
    const size_t nRayCol = (size_t)nla * Nmu;
    const size_t perColOut = rays_out_bytes(nRayCol, Ns, depth);
    const size_t outBytes = (size_t)n * perColOut;
    unsigned char* hin = st.inPinned.as<unsigned char>();
    HIP_TRY(c0->mem.h2d(st.in.p, hin, inBytes));
    const int stp = pre();
    if (stp != LWHIP_OK)
        return stp;
    // ---- one launch ------------------------------------------------------------------------------------------------------------
    RaysArgs g{};
    g.cols = (const RayCol*)st.in.p;
    g.Ns = Ns;
    g.Nmu = Nmu;
    g.la0 = la0;
    g.nla = nla;
    g.R = rays_per_group(Ns);
    g.blocksPerCol = (int)((nRayCol + g.R - 1) / g.R);
    const size_t ldsBytes = (size_t)RAYS_ARRAYS * g.R * Ns * sizeof(double);
    const size_t nBlk = (size_t)n * g.blocksPerCol;
    if (nBlk > 0x7fffffffu)
        return fail(LWHIP_ERR_UNSUPPORTED, what + ": too many rays for one launch");
    if (hybrid)
        LWHIP_LAUNCH(rays_kernel<true>, dim3((unsigned)nBlk), dim3(RAYS_THREADS), ldsBytes, c0->stream, g);
    else
        LWHIP_LAUNCH(rays_kernel<false>, dim3((unsigned)nBlk), dim3(RAYS_THREADS), ldsBytes, c0->stream, g);
    HIP_TRY(hipGetLastError());
    // ---- one copy back, one wait -------------------------------------------------------------------------------------------------
    unsigned char* hout = st.outPinned.as<unsigned char>();
    HIP_TRY(hipMemcpyAsync(hout, st.out.p, outBytes, hipMemcpyDeviceToHost, c0->stream));
    HIP_TRY(hipStreamSynchronize(c0->stream));
    for (int i = 0; i < n; ++i)
    {
        const double* o = (const double*)(hout + (size_t)i * perColOut);
        std::memcpy(reqs[i]->I, o, nRayCol * sizeof(double));
        if (depth)
        {
            std::memcpy(reqs[i]->depthChi, o + nRayCol, nRayCol * Ns * sizeof(double));
            std::memcpy(reqs[i]->depthEta, o + nRayCol + nRayCol * Ns, nRayCol * Ns * sizeof(double));
            std::memcpy(reqs[i]->depthI, o + nRayCol + 2 * nRayCol * Ns, nRayCol * Ns * sizeof(double));
        }
    }
    return LWHIP_OK;
}

// the context's resident state as a column's record reads it; the rows of a wavelength grid are filled in by the caller
RayCol rays_col_base(const lwhip_context* c, const lwhip_rays& r)
{
    RayCol a{};
    a.height = c->height.p;
    a.temperature = c->temperature.p;
    a.n = c->n.p;
    a.ratio = c->ratio.p;
    a.vlosMu = c->vlosMu.p;
    a.muzCtx = c->muz.p;
    a.vBroad = c->vBroad.p;
    a.aDamp = c->aDamp.p;
    a.lowerType = c->prob.zLowerBc.type;
    for (int m = 0; m < r.Nmu; ++m)
        a.mu[m] = r.muz[m];
    return a;
}

// ---- a new wavelength grid -----------------------------------------------------------------------------------------------------
// The active set of the grid w [Nwave] (lightweaver/atomic_set.py:209-257): the rows [Nb, Nr) of the old grid it spans, both
// searches from the left; a transition is active iff its old rows [Nblue, Nred) meet them.  The one place the rule lives.
void grid_active(const lwhip_context* c, const double* w, int Nwave, std::vector<int32_t>& active)
{
    const double* old = c->prob.wavelength;
    const int N = c->prob.Nlambda;
    const int Nb = (int)(std::lower_bound(old, old + N, w[0]) - old);
    const int Nr = std::min((int)(std::lower_bound(old, old + N, w[Nwave - 1]) - old) + 1, N);
    active.assign(c->trans.size(), 0);
    for (size_t t = 0; t < c->trans.size(); ++t)
        active[t] = std::max(Nb, c->trans[t].t.Nblue) < std::min(Nr, c->trans[t].t.Nred) ? 1 : 0;
}

// what a new grid adds to the refusals of rays_check; the active set comes back
int grid_check(lwhip_context* c, const lwhip_rays_grid* q, const std::string& what, std::vector<int32_t>& active)
{
    if (c->worldSize > 1 || c->laStart != 0 || c->laEnd != c->prob.Nlambda)
        return fail(LWHIP_ERR_UNSUPPORTED, what + ": not on a wavelength shard (J of the other rows is not resident)");
    if (q->Nwave < 2)
        return fail(LWHIP_ERR_INVALID, what + ": Nwave >= 2 is required");
    if (!q->wavelength)
        return fail(LWHIP_ERR_INVALID, what + ": wavelength is required");
    for (int l = 0; l < q->Nwave; ++l)
    {
        if (!std::isfinite(q->wavelength[l]))
            return fail(LWHIP_ERR_INVALID, what + ": wavelength " + std::to_string(l) + " is not finite");
        if (l > 0 && !(q->wavelength[l] > q->wavelength[l - 1]))
            return fail(LWHIP_ERR_INVALID, what + ": the wavelengths are not strictly increasing (at " + std::to_string(l) + ")");
    }
    if (!q->bgChi || !q->bgEta || !q->bgSca)
        return fail(LWHIP_ERR_INVALID, what + ": bgChi, bgEta and bgSca [Nwave, Nspace] are required (missing: "
                                           + (!q->bgChi ? "bgChi" : !q->bgEta ? "bgEta" : "bgSca") + ")");
    grid_active(c, q->wavelength, q->Nwave, active);
    for (size_t t = 0; t < c->trans.size(); ++t)
        if (active[t] && c->trans[t].t.type != LWHIP_LINE && (!q->contAlpha || !q->contAlpha[t]))
            return fail(LWHIP_ERR_INVALID, what + ": contAlpha of transition " + std::to_string(t)
                                               + " is NULL (an active continuum needs its cross-section [Nwave])");
    return LWHIP_OK;
}

// One row-interpolation of the prep kernel: f [nOld, Ns] given at x [nOld] -> out [Nwave, Ns] at the new wavelengths.
struct InterpJob
{
    const double* x;
    const double* f;
    double* out;
    int32_t nOld, _pad;
};
struct InterpArgs
{
    const InterpJob* jobs;
    const double* xNew;
    int32_t nJobs, Nwave, Ns, _pad;
};

// numpy.interp at one point: the bracket x[j] <= xv < x[j + 1], slope (xv - x[j]) + f[j]; the end values held outside the
// grid; a node gives its value exactly.  f is strided by Ns (one depth point's column of a [rows, Ns] array).
__device__ double d_interp_row(const double* x, const double* f, int n, int Ns, double xv)
{
    if (xv > x[n - 1])
        return f[(size_t)(n - 1) * Ns];
    if (xv < x[0])
        return f[0];
    int lo = 0, hi = n - 1; // x[lo] <= xv throughout
    while (hi - lo > 1)
    {
        const int mid = (lo + hi) >> 1;
        if (x[mid] <= xv)
            lo = mid;
        else
            hi = mid;
    }
    if (x[hi] <= xv) // (the last node itself)
        lo = hi;
    if (lo == n - 1 || x[lo] == xv)
        return f[(size_t)lo * Ns];
    const double f0 = f[(size_t)lo * Ns], f1 = f[(size_t)(lo + 1) * Ns];
    const double slope = (f1 - f0) / (x[lo + 1] - x[lo]);
    return slope * (xv - x[lo]) + f0;
}

// J and rho of the PRD lines on the new grid, from the resident arrays: a thread per (new wavelength, depth point), depth
// fastest (the reads of a row and the stores are contiguous in k); the jobs along y.
__global__ void __launch_bounds__(RAYS_THREADS) rays_grid_rows_kernel(const InterpArgs g)
{
    const int nPt = g.Nwave * g.Ns;
    for (int j = blockIdx.y; j < g.nJobs; j += gridDim.y)
    {
        const InterpJob job = g.jobs[j];
        for (int idx = blockIdx.x * RAYS_THREADS + threadIdx.x; idx < nPt; idx += gridDim.x * RAYS_THREADS)
        {
            const int l = idx / g.Ns, k = idx - l * g.Ns;
            job.out[idx] = d_interp_row(job.x, job.f + k, job.nOld, g.Ns, g.xNew[l]);
        }
    }
}

// a staged block's layout, piece by piece
struct Stage
{
    size_t bytes = 0;
    size_t take(size_t b)
    {
        const size_t at = bytes;
        bytes += align256(b);
        return at;
    }
};

// The call: cols[i] with request reqs[i], everything on cols[0]'s stream, staged through `st`.  grids: empty, or the new-grid
// requests reqs[i] is embedded in -- then the rows the kernel reads are the request's, not the context's.  hybrid: every column
// carries hybrid-PRD tables, and rho of the lines of its hybrid list is interpolated for the new rays (rays_kernel<true>).
int rays_run(lwhip_context* const* cols, int n, const std::vector<const lwhip_rays*>& reqs,
             const std::vector<const lwhip_rays_grid*>& grids, RaysState*& slot, const std::string& what, bool hybrid)
{
    const bool grid = !grids.empty();
    int la0 = 0, la1 = 0;
    std::vector<int32_t> active; // (new grid) of column 0, which every column shares
    for (int i = 0; i < n; ++i)
    {
        auto named = [&](int code) {
            return n > 1 ? fail(code, std::string(lwhip_last_error()) + " (column " + std::to_string(i) + ")") : code;
        };
        if (grid && (reqs[i]->laStart != 0 || reqs[i]->laEnd != 0))
            return fail(LWHIP_ERR_INVALID, what + ": laStart and laEnd must be 0 with a wavelength grid (they select rows of the "
                                               "context's own)" + (n > 1 ? " (column " + std::to_string(i) + ")" : ""));
        int a0 = 0, a1 = 0;
        const int chk = rays_check(cols[i], reqs[i], what, false, a0, a1, hybrid);
        if (chk != LWHIP_OK)
            return named(chk);
        if (i == 0)
        {
            la0 = a0;
            la1 = a1;
        }
        const lwhip_context* c = cols[i];
        if (c->Ns != cols[0]->Ns || c->device != cols[0]->device || reqs[i]->Nmu != reqs[0]->Nmu || a0 != la0 || a1 != la1
            || (reqs[i]->depthI != nullptr) != (reqs[0]->depthI != nullptr))
            return fail(LWHIP_ERR_INVALID, what + ": column " + std::to_string(i)
                                               + " differs from column 0 (depth points, Nmu, wavelength range and depth outputs "
                                                 "are the same for every column)");
        if (grid)
        {
            std::vector<int32_t> act;
            const int gchk = grid_check(cols[i], grids[i], what, act);
            if (gchk != LWHIP_OK)
                return named(gchk);
            if (i == 0)
                active = act;
            else if (grids[i]->Nwave != grids[0]->Nwave
                     || std::memcmp(grids[i]->wavelength, grids[0]->wavelength, (size_t)grids[0]->Nwave * sizeof(double)) != 0
                     || act != active)
                return fail(LWHIP_ERR_INVALID, what + ": column " + std::to_string(i)
                                                   + " differs from column 0 (Nwave, the wavelengths and the active transitions "
                                                     "are the same for every column)");
        }
    }
    lwhip_context* c0 = cols[0];
    const int Ns = c0->Ns, Nmu = reqs[0]->Nmu, nla = grid ? grids[0]->Nwave : la1 - la0;
    const bool depth = reqs[0]->depthI != nullptr;
    HIP_TRY(hipSetDevice(c0->device));
    HIP_TRY(rays_init_table(c0->device));
    std::vector<RaysState*> tabs(n, nullptr);
    for (int i = 0; i < n && !grid; ++i)
    {
        lwhip_context* o = cols[i]->tablesFrom ? cols[i]->tablesFrom : cols[i];
        // (the tables are the owner's: its hybrid list is this column's, as its rho layout is -- both follow the structure)
        for (size_t t = 0; hybrid && t < cols[i]->trans.size(); ++t)
            if (rays_hybrid_line(o, t) != rays_hybrid_line(cols[i], t))
                return fail(LWHIP_ERR_INVALID, what + ": the hybrid PRD line list differs from that of the context whose tables "
                                                   "this one shares" + (n > 1 ? " (column " + std::to_string(i) + ")" : ""));
        const int stp = rays_tables(o, tabs[i]);
        if (stp != LWHIP_OK)
            return stp;
    }
    RaysState& st = *rays_state(slot);
    // ---- the staged request: [RayCol x n | vz | lowerBc], one copy up ------------------------------------------------------
    // a new grid adds [wavelength | row lists] once and per column [RayTrans | par | bgChi | bgEta | bgSca], then the jobs of
    // the prep kernel; the rows that kernel fills (J', rho' of each active PRD line) follow the outputs in st.out
    const size_t nRayCol = (size_t)nla * Nmu;
    const size_t rowBytes = (size_t)nla * Ns * sizeof(double);
    Stage in, rows;
    in.take((size_t)n * sizeof(RayCol));
    std::vector<int> act; // the active transitions, context order
    for (size_t t = 0; t < active.size(); ++t)
        if (active[t])
            act.push_back((int)t);
    const size_t nA = act.size();
    std::vector<int> prdLines; // positions in `act` of the lines that carry rho
    if (grid)
        for (size_t a = 0; a < nA; ++a)
        {
            const HostTrans& h = c0->trans[act[a]];
            if (h.t.type == LWHIP_LINE && h.t.prd && h.rhoOff >= 0)
                prdLines.push_back((int)a);
        }
    const size_t jobsPerCol = 1 + prdLines.size();
    size_t waveOff = 0, laOffOff = 0, laTrOff = 0, jobsOff = 0;
    if (grid)
    {
        waveOff = in.take((size_t)nla * sizeof(double));
        laOffOff = in.take((size_t)(nla + 1) * sizeof(int32_t));
        laTrOff = in.take(std::max<size_t>((size_t)nla * nA, 1) * sizeof(int32_t));
        jobsOff = in.take((size_t)n * jobsPerCol * sizeof(InterpJob));
    }
    std::vector<size_t> vzOff(n, 0), bcOff(n, 0), trOff(n, 0), parOff(n, 0), bgOff(n, 0), rowsOff(n, 0);
    for (int i = 0; i < n; ++i)
    {
        if (reqs[i]->vz)
            vzOff[i] = in.take((size_t)Ns * sizeof(double));
        if (cols[i]->prob.zLowerBc.type == LWHIP_BC_CALLABLE)
            bcOff[i] = in.take(nRayCol * sizeof(double));
        if (grid)
        {
            trOff[i] = in.take(std::max<size_t>(nA, 1) * sizeof(RayTrans));
            parOff[i] = in.take(std::max<size_t>(nA * 4 * nla, 1) * sizeof(double));
            bgOff[i] = in.take(3 * rowBytes);
            rowsOff[i] = rows.take(jobsPerCol * rowBytes);
        }
    }
    const size_t inBytes = in.bytes;
    const size_t perColOut = rays_out_bytes(nRayCol, Ns, depth);
    const size_t outBytes = (size_t)n * perColOut;
    // (the rows a new grid needs are device-only: they follow the outputs in the `out` buffer and are not copied back)
    const size_t rowsBase = align256(outBytes);
    if (st.in.n < inBytes || st.out.n < rowsBase + rows.bytes)
    {
        HIP_TRY(hipStreamSynchronize(c0->stream));
        if (st.in.n < inBytes)
            HIP_TRY(st.in.alloc(c0->mem, inBytes, false));
        if (st.out.n < rowsBase + rows.bytes)
            HIP_TRY(st.out.alloc(c0->mem, rowsBase + rows.bytes, false));
    }
    HIP_TRY(st.inPinned.reserve(c0->device, inBytes, c0->stream));
    HIP_TRY(st.outPinned.reserve(c0->device, outBytes, c0->stream));
    unsigned char* hin = st.inPinned.as<unsigned char>();
    RayCol* hc = (RayCol*)hin;
    if (grid)
    {
        // every active transition on every row, reference order
        std::memcpy(hin + waveOff, grids[0]->wavelength, (size_t)nla * sizeof(double));
        int32_t* lo = (int32_t*)(hin + laOffOff);
        int32_t* lt = (int32_t*)(hin + laTrOff);
        for (int l = 0; l <= nla; ++l)
            lo[l] = (int32_t)((size_t)l * nA);
        for (size_t e = 0; e < (size_t)nla * nA; ++e)
            lt[e] = (int32_t)(e % nA);
    }
    for (int i = 0; i < n; ++i)
    {
        lwhip_context* c = cols[i];
        const lwhip_rays& r = *reqs[i];
        RayCol a = rays_col_base(c, r);
        if (!grid)
        {
            a.wavelength = c->wavelength.p;
            a.bgChi = c->bgChi.p;
            a.bgEta = c->bgEta.p;
            a.bgSca = c->bgSca.p;
            a.J = c->J.p;
            a.par = c->par.p;
            a.rho = c->rho.p;
            a.lineWave = c->lineWave.p;
            a.tr = tabs[i]->tr.p;
            a.laOff = tabs[i]->laOff.p;
            a.laTr = tabs[i]->laTr.p;
        }
        else
        {
            const lwhip_rays_grid& q = *grids[i];
            const double* wl = q.wavelength;
            double* rowsDev = (double*)(st.out.p + rowsBase + rowsOff[i]); // J', then rho' of each PRD line
            const size_t rowLen = (size_t)nla * Ns;
            a.wavelength = a.lineWave = (const double*)(st.in.p + waveOff);
            std::memcpy(hin + bgOff[i], q.bgChi, rowBytes);
            std::memcpy(hin + bgOff[i] + rowBytes, q.bgEta, rowBytes);
            std::memcpy(hin + bgOff[i] + 2 * rowBytes, q.bgSca, rowBytes);
            a.bgChi = (const double*)(st.in.p + bgOff[i]);
            a.bgEta = a.bgChi + rowLen;
            a.bgSca = a.bgEta + rowLen;
            a.J = rowsDev;
            a.rho = rowsDev;
            a.par = (const double*)(st.in.p + parOff[i]);
            a.tr = (const RayTrans*)(st.in.p + trOff[i]);
            a.laOff = (const int32_t*)(st.in.p + laOffOff);
            a.laTr = (const int32_t*)(st.in.p + laTrOff);
            InterpJob* jobs = (InterpJob*)(hin + jobsOff) + (size_t)i * jobsPerCol;
            jobs[0] = InterpJob{ c->wavelength.p, c->J.p, rowsDev, c->Nla, 0 };
            RayTrans* trs = (RayTrans*)(hin + trOff[i]);
            double* par = (double*)(hin + parOff[i]);
            const std::vector<LineEval> ev = line_eval_records(c->trans);
            size_t nPrd = 0;
            for (size_t k = 0; k < nA; ++k)
            {
                const HostTrans& h = c->trans[act[k]];
                RayTrans t{};
                t.type = h.t.type;
                t.gi = c->levelOff[h.atom] + h.t.i;
                t.gj = c->levelOff[h.atom] + h.t.j;
                t.Nblue = 0;
                t.prd = (h.t.type == LWHIP_LINE && h.t.prd && h.rhoOff >= 0) ? 1 : 0;
                t.row = ev[act[k]].row;
                t.atom = ev[act[k]].atom;
                t.ltStart = 0;
                t.parOff = (int64_t)(k * 4 * nla);
                t.waveOff = 0;
                t.lambda0 = h.t.lambda0;
                if (t.prd)
                {
                    if (++nPrd > prdLines.size())
                        break;
                    t.rhoOff = (int64_t)(nPrd * rowLen);
                    if (hybrid && rays_hybrid_line(c, (size_t)act[k]))
                    {
                        // the line's own grid is the request's, and rho' [Nwave, Ns] is its rho (what the reference's second
                        // context holds after subset_configuration)
                        t.hybrid = 1;
                        t.nlt = nla;
                        t.rho0Off = t.rhoOff;
                    }
                    jobs[nPrd] = InterpJob{ c->lineWave.p + h.waveOff + h.rhoLt0, c->rho.p + h.rhoOff, rowsDev + nPrd * rowLen,
                                            h.rhoRows, 0 };
                }
                trs[k] = t;
                // the per-(transition, wavelength) scalars of build_tables (lwhip_tables.hip) on the new grid; the quadrature
                // weight [1] has no meaning here and is not read
                double* p = par + k * 4 * (size_t)nla;
                for (int l = 0; l < nla; ++l, p += 4)
                {
                    if (h.t.type == LWHIP_LINE)
                    {
                        const double hnu_4pi = HC_4PI * (h.t.lambda0 / wl[l]);
                        p[0] = hnu_4pi * h.t.Bij;
                        p[1] = 0.0;
                        p[2] = h.t.Bji / h.t.Bij;
                        p[3] = h.t.Aji / h.t.Bji;
                    }
                    else
                    {
                        p[0] = q.contAlpha[act[k]][l];
                        p[1] = 0.0;
                        p[2] = TWO_HC_NM3 / (wl[l] * wl[l] * wl[l]);
                        p[3] = 0.0;
                    }
                }
            }
            if (nPrd != prdLines.size()) // (before anything is queued)
                return fail(LWHIP_ERR_INVALID, what + ": column " + std::to_string(i) + " differs from column 0 (its PRD lines)");
        }
        if (r.vz)
        {
            std::memcpy(hin + vzOff[i], r.vz, (size_t)Ns * sizeof(double));
            a.vz = (const double*)(st.in.p + vzOff[i]);
        }
        if (a.lowerType == LWHIP_BC_CALLABLE)
        {
            std::memcpy(hin + bcOff[i], r.lowerBc, nRayCol * sizeof(double));
            a.lowerBc = (const double*)(st.in.p + bcOff[i]);
        }
        double* o = (double*)(st.out.p + (size_t)i * perColOut);
        a.I = o;
        if (depth)
        {
            a.depthChi = o + nRayCol;
            a.depthEta = o + nRayCol + nRayCol * Ns;
            a.depthI = o + nRayCol + 2 * nRayCol * Ns;
        }
        hc[i] = a;
    }
    if (!grid)
        return rays_launch_fetch(c0, st, reqs, Ns, Nmu, la0 - c0->laStart, nla, inBytes, what, hybrid, [] { return LWHIP_OK; });
    // the rows of the new grid first, on the same stream
    InterpArgs ia{};
    ia.jobs = (const InterpJob*)(st.in.p + jobsOff);
    ia.xNew = (const double*)(st.in.p + waveOff);
    ia.nJobs = (int32_t)((size_t)n * jobsPerCol);
    ia.Nwave = nla;
    ia.Ns = Ns;
    if ((size_t)nla * Ns > 0x7fffffffu || (size_t)n * jobsPerCol > 0x7fffffffu)
        return fail(LWHIP_ERR_UNSUPPORTED, what + ": too many rows for one launch");
    const unsigned bx = (unsigned)std::min<size_t>(((size_t)nla * Ns + RAYS_THREADS - 1) / RAYS_THREADS, 4096);
    const unsigned by = (unsigned)std::min<size_t>((size_t)n * jobsPerCol, 65535);
    hipStream_t stream = c0->stream;
    return rays_launch_fetch(c0, st, reqs, Ns, Nmu, 0, nla, inBytes, what, hybrid, [&]() -> int {
        LWHIP_LAUNCH(rays_grid_rows_kernel, dim3(bx, by), dim3(RAYS_THREADS), 0, stream, ia);
        HIP_TRY(hipGetLastError());
        return LWHIP_OK;
    });
}

int rays_run_reqs(lwhip_context* const* cols, int n, const lwhip_rays* reqs, RaysState*& slot, const char* whatC, bool hybrid)
{
    const std::string what(whatC);
    if (lwhip_device_count() <= 0)
        return fail(LWHIP_ERR_DEVICE, what + ": no gfx950 device");
    if (n <= 0 || !cols || !reqs)
        return fail(LWHIP_ERR_INVALID, what + ": null " + (n > 1 ? "batch" : "context") + " or request");
    std::vector<const lwhip_rays*> ptrs(n);
    for (int i = 0; i < n; ++i)
        ptrs[i] = reqs + i;
    return rays_run(cols, n, ptrs, {}, slot, what, hybrid);
}

int rays_run_reqs(lwhip_context* const* cols, int n, const lwhip_rays_grid* reqs, RaysState*& slot, const char* whatC, bool hybrid)
{
    const std::string what(whatC);
    if (lwhip_device_count() <= 0)
        return fail(LWHIP_ERR_DEVICE, what + ": no gfx950 device");
    if (n <= 0 || !cols || !reqs)
        return fail(LWHIP_ERR_INVALID, what + ": null " + (n > 1 ? "batch" : "context") + " or request");
    std::vector<const lwhip_rays*> ptrs(n);
    std::vector<const lwhip_rays_grid*> grids(n);
    for (int i = 0; i < n; ++i)
    {
        grids[i] = reqs + i;
        ptrs[i] = &reqs[i].rays;
    }
    return rays_run(cols, n, ptrs, grids, slot, what, hybrid);
}

// The entry points: one context or the columns of a batch, the stored grid (lwhip_rays) or a new one (lwhip_rays_grid), plain or
// for hybrid-PRD contexts.
template <typename Req> int rays_ctx(lwhip_context* c, const Req* rays, bool hybrid, const char* what)
{
    if (lwhip_device_count() <= 0)
        return fail(LWHIP_ERR_DEVICE, std::string(what) + ": no gfx950 device");
    if (!c)
        return fail(LWHIP_ERR_INVALID, std::string(what) + ": null context");
    lwhip_context* cols[1] = { c };
    return rays_run_reqs(cols, 1, rays, c->rays, what, hybrid);
}

template <typename Req> int rays_batch(lwhip_batch* b, const Req* perColumn, bool hybrid, const char* what)
{
    if (lwhip_device_count() <= 0)
        return fail(LWHIP_ERR_DEVICE, std::string(what) + ": no gfx950 device");
    if (!b || b->ctxs.empty())
        return fail(LWHIP_ERR_INVALID, std::string(what) + ": null batch");
    return rays_run_reqs(b->ctxs.data(), (int)b->ctxs.size(), perColumn, b->rays, what, hybrid);
}
} // namespace
} // namespace lwhip

extern "C"
{
int lwhip_compute_rays(lwhip_context* c, const lwhip_rays* rays) { return rays_ctx(c, rays, false, "lwhip_compute_rays"); }

int lwhip_batch_compute_rays(lwhip_batch* b, const lwhip_rays* perColumn)
{
    return rays_batch(b, perColumn, false, "lwhip_batch_compute_rays");
}

int lwhip_compute_rays_hprd(lwhip_context* c, const lwhip_rays* rays) { return rays_ctx(c, rays, true, "lwhip_compute_rays_hprd"); }

int lwhip_batch_compute_rays_hprd(lwhip_batch* b, const lwhip_rays* perColumn)
{
    return rays_batch(b, perColumn, true, "lwhip_batch_compute_rays_hprd");
}

int lwhip_rays_grid_active(lwhip_context* c, const double* wavelength, int Nwave, int32_t* active)
{
    if (!c || !wavelength || !active || Nwave < 1)
        return fail(LWHIP_ERR_INVALID, "lwhip_rays_grid_active: a context, wavelength [Nwave >= 1] and active are required");
    std::vector<int32_t> act;
    grid_active(c, wavelength, Nwave, act);
    std::copy(act.begin(), act.end(), active);
    return LWHIP_OK;
}

int lwhip_compute_rays_grid(lwhip_context* c, const lwhip_rays_grid* rays)
{
    return rays_ctx(c, rays, false, "lwhip_compute_rays_grid");
}

int lwhip_batch_compute_rays_grid(lwhip_batch* b, const lwhip_rays_grid* perColumn)
{
    return rays_batch(b, perColumn, false, "lwhip_batch_compute_rays_grid");
}

int lwhip_compute_rays_grid_hprd(lwhip_context* c, const lwhip_rays_grid* rays)
{
    return rays_ctx(c, rays, true, "lwhip_compute_rays_grid_hprd");
}

int lwhip_batch_compute_rays_grid_hprd(lwhip_batch* b, const lwhip_rays_grid* perColumn)
{
    return rays_batch(b, perColumn, true, "lwhip_batch_compute_rays_grid_hprd");
}
}
