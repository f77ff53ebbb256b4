// lwhip_stokes_fs.hip -- the full-Stokes formal solution for Zeeman-polarised lines (1D plane-parallel): formal_sol_full_stokes
// (Source/FormalStokes.cpp:166-723) of one context (lwhip_full_stokes_fs) or of every column of a 1.5D batch
// (lwhip_batch_full_stokes_fs), and the emergent Stokes vector along observer rays (lwhip_compute_stokes_rays,
// lwhip_batch_compute_stokes_rays).  One driver, stokes_fs_run, serves them all: a context on its own is a batch of one column,
// and an observer call is a column whose argument block carries the request's directions and outputs.
//
// A chunk of (columns x wavelength range) runs as up to three launches on the first column's stream, each over ALL columns
// of the chunk, the column outermost in the work index:
//   stokes_gather_kernel  one workgroup per block of 64 rays: chi[7] and eta[4] of every depth point summed over the
//                         transitions active at lambda (stokes_fs_core :496-602), stored as the rays' rows chi[0..6], S[0..3];
//                         stokes_observer_gather_kernel is the same sum for the directions of an observer request, whose
//                         profiles it forms in place (see "Observer rays" below);
//   stokes_march_kernel   one lane per ray, one wavefront per block of 64 rays: the DELO-Bezier3 march of
//                         piecewise_stokes_bezier3_1d_impl (:166-340) down the ray with a 4 x 4 Crout LU per depth point
//                         (lwhip_lu.h), or the scalar piecewise_bezier3_1d (FormalScalar.cpp:209-325) where the wavelength
//                         is not polarised;
//   stokes_j_kernel       (updateJ) one thread per (column, lambda): J, J20 and dJ, the rays added in the reference's order.
// The march is serial in depth, so a ray is one lane and needs no exchange between lanes.  K is carried as its six
// independent entries (stokes_K :119-142) and expanded where a step uses it; no scratch memory ("Full Stokes").
// Layout.  A column's rays of the chunk (its nla x Nr x nDir rays: lambda outermost, then mu, then direction) are cut into
// blocks of 64, the last one padded, so that every wavefront belongs to one column and reads its argument block with scalar
// loads.  A block's rows are [ST_ROWS][Ns][64]: at each depth point the 64 lanes read 64 consecutive doubles.  The I / Q
// profiles of updateJ are [2][Ns][64] per block.
// Scratch.  The rows of a chunk belong to the caller's slot (the context's, or the batch's) and are capped by the caller:
// they do not grow with the number of columns.  A chunk takes as many whole columns as fit, or one column's wavelength
// range when a single column does not fit.  The results are the same bits for any chunking (tested).
//
// Observer rays.  What LwContext.compute_rays(mus, stokes=True) (Source/LwMiddleLayer.pyx:3898-4002) computes: the result of
// formal_sol_full_stokes(updateJ = 0, upOnly = 1) on a second context with the same state, rays muz = mus, vlosMu = mu (x) v_z,
// wmu = 0, the field projected onto the new directions and the profiles of those directions.  Here no context is made and no
// profile stored: the observer gather evaluates, per (ray, depth point, active line), phi = H(a, v) / (sqrt(pi) vBroad) of a
// line that is not polarised (as rays_kernel does) or the Zeeman sum and projections of compute_polarised_profiles
// (FormalStokes.cpp:43-110; d_polarised_profile) of a polarised one, and writes the row blocks the march reads.  The march is
// stokes_march_kernel as it stands: it reaches everything through StokesArgs, and an observer column's StokesArgs has the
// request's directions as muz, the identity as lowerIdx, the staged request data as lowerBc and the request's device output as
// I / Quv.  As in the reference: no scattering term (J dagger = 0 without updateJ), exact zeros for Q, U, V where no polarised
// line is active, and whatever 1D solver the context was built with.
#include "lwhip_host.h"
#include "lwhip_device.h"
// H(a, v), H + iF and the Zeeman sum under the contraction setting of the stored profiles' unit (d_voigt_H: the compiler's
// default; the other two carry their own `fp contract(off)`): the same arguments give the same bits
#include "lwhip_voigt_dev.h"

// As in lwhip_pops.hip: no fused multiply-adds, so that the operations match the reference's one for one.
#pragma clang fp contract(off)

#include "lwhip_lu.h"

#include <algorithm>
#include <atomic>
#include <cstring>
#include <vector>

namespace lwhip
{
namespace
{
enum { ST_ROWS = 11 }; // per ray: chi[0..6], S[0..3]
enum { SB_LANES = 64 };

// one column: its context's resident state and where its results go
struct StokesArgs
{
    int32_t Ns, Nr, Nla, updateJ;
    int32_t hasJ20, _pad;
    int32_t lowerType, upperType, lowerNmu, upperNmu;
    const double* height;
    const double* temperature;
    const double* muz;
    const double* wmu;
    const double* wavelength;
    const double* bgChi;
    const double* bgEta;
    const double* bgSca;
    double* J;
    double* J20;
    const double* n;
    const double* ratio;
    const double* par;
    const double* phi;
    const double* rho;
    const double* pol;
    const double* lowerBc;
    const double* upperBc;
    const int32_t* lowerIdx;
    const int32_t* upperIdx;
    const int32_t* laOff;
    const int32_t* laTr;
    const int32_t* laPol;
    const StokesTrans* tr;
    double* I;       // [Nla, Nr]
    double* Quv;     // [3, Nla, Nr]
    double* dJ;      // [Nla]
    int32_t* singular; // set when a depth point's 4 x 4 system is singular (solve_lin_eq throws there, LuSolve.cpp:22-23)
};

// One ray's rows within its block: index i is 64 doubles (one per lane of the wavefront's rays) after i - 1, so row m at
// depth k is row[m * Ns + k]
template <typename T> struct LaneRow
{
    T* p;
    DEVINL T& operator[](int i) const { return p[(size_t)i * SB_LANES]; }
    DEVINL LaneRow operator+(int i) const { return LaneRow{ p + (size_t)i * SB_LANES }; }
    DEVINL explicit operator bool() const { return p != nullptr; }
};
using RowIn = LaneRow<const double>;
using RowOut = LaneRow<double>;

DEVINL bool polarised_la(const StokesArgs& a, int la) { return a.laPol[la] != 0 || a.hasJ20; }

// one column of an observer call: what forming the profiles of its directions takes (the rest is in its StokesArgs)
struct ObsCol
{
    const LineEval* ev;      // per transition, indexed as StokesArgs::tr
    const int32_t* polComp;  // per polarised line: offset of its Zeeman components in the three arrays below, their number
    const int32_t* alpha;
    const double* shift;
    const double* strength;
    const double* vBroad;
    const double* aDamp;
    const double* lineWave;
    const double* B;
    const double* vz;        // [Ns] staged, or null: vlosMu[0] / muz[0] of the resident atmosphere
    const double* vlosMu;
    const double* muzCtx;
    const double* cosGamma;  // [Nmu, Ns] staged: the field projected onto the request's directions
    const double* cos2chi;
    const double* sin2chi;
};

// Where the gather takes the profiles of a line at a point from.  at(...) gives the point's phi(a, t) and, of a polarised
// line, pol(a, t)[q]: phiQ, phiU, phiV, psiQ, psiU, psiV.
// The context's own rays: the stored phi and phiQ..psiV.
struct StoredProfiles
{
    struct Point
    {
        size_t pk = 0;
        DEVINL double phi(const StokesArgs& a, const StokesTrans& t) const { return a.phi[t.phiOff + pk]; }
        struct Pol
        {
            const double* P;
            size_t s;
            DEVINL double operator[](int q) const { return P[q * s]; }
        };
        DEVINL Pol pol(const StokesArgs& a, const StokesTrans& t) const { return Pol{ a.pol + t.polOff + pk, (size_t)t.polStride }; }
    };
    DEVINL Point at(const StokesArgs& a, const StokesTrans&, int, int lt, int mu, int d, int k) const
    {
        return Point{ (((size_t)lt * a.Nr + mu) * 2 + d) * a.Ns + k };
    }
};
// The directions of an observer request (up-going: s = +1): formed here, never stored.  phi of a line that is not polarised
// as voigt_phi_kernel / rays_kernel form it, the seven profiles of a polarised one as polarised_profile_kernel does.
struct ObserverProfiles
{
    const ObsCol o;
    struct Point
    {
        double ph = 0.0, p[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
        DEVINL double phi(const StokesArgs&, const StokesTrans&) const { return ph; }
        DEVINL const double* pol(const StokesArgs&, const StokesTrans&) const { return p; }
    };
    DEVINL Point at(const StokesArgs& a, const StokesTrans& t, int tr, int lt, int mu, int, int k) const
    {
        const double sqrtPi = 1.772453850905516027298167483341145182798;
        const int Ns = a.Ns;
        const LineEval e = o.ev[tr];
        const double vb = o.vBroad[(size_t)e.atom * Ns + k];
        const double ad = o.aDamp[(size_t)e.row * Ns + k];
        const double vBase = (o.lineWave[e.waveOff + lt] - e.lambda0) * CLight / e.lambda0;
        const double vz = o.vz ? o.vz[k] : o.vlosMu[k] / o.muzCtx[0];
        const double vk = (vBase + a.muz[mu] * vz) / vb;
        Point pt;
        if (t.pol < 0)
        {
            pt.ph = d_voigt_H(ad, vk) / (sqrtPi * vb);
            return pt;
        }
        const double larmor = 1.60217733E-19 / (4.0 * Pi * 9.1093897E-31) * (e.lambda0 * NM_TO_M); // QElectron, MElectron
        const double vB = larmor * o.B[k] / vb;
        const double sv = 1.0 / (sqrtPi * vb);
        const int c0 = o.polComp[2 * t.pol], nComp = o.polComp[2 * t.pol + 1];
        const size_t mk = (size_t)mu * Ns + k;
        d_polarised_profile(ad, vk, vB, nComp, o.alpha + c0, o.shift + c0, o.strength + c0, o.cosGamma, o.cos2chi, o.sin2chi, mk, sv,
                            1.0, &pt.ph, pt.p, 1, 0);
        return pt;
    }
};

// chi[7] and eta[4] of (la, mu, d) at depth k summed over the transitions active at la (stokes_fs_core :496-602), stored as
// the ray's rows chi[0..6], S[0..3]: row[m * Ns] is row m at this depth.  prof: where the lines' profiles come from.
template <typename Prof> DEVINL void stokes_gather_point(const StokesArgs& a, const Prof& prof, int la, int mu, int d, int k, RowOut row)
{
    const int Ns = a.Ns;
    const double inv2root2 = 1.0 / (2.0 * sqrt(2.0));
    const bool polF = polarised_la(a, la);
    double chi[7] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
    double eta[4] = { 0.0, 0.0, 0.0, 0.0 };
    for (int q = a.laOff[la]; q < a.laOff[la + 1]; ++q)
    {
        const int tr = a.laTr[q];
        const StokesTrans t = a.tr[tr];
        const int lt = la - t.Nblue;
        const double* p = a.par + t.parOff + 4 * (size_t)lt;
        double Vij, Vji, Uji;
        typename Prof::Point pt;
        if (t.type == LWHIP_LINE)
        {
            // Transition::uv (LwTransition.hpp:98-127) with gij of Atom::setup_wavelength (LwAtom.hpp:99-123)
            pt = prof.at(a, t, tr, lt, mu, d, k);
            Vij = p[0] * pt.phi(a, t);
            double g = p[2];
            if (t.prd)
                g *= a.rho[t.rhoOff + (size_t)lt * Ns + k];
            Vji = g * Vij;
            Uji = p[3] * Vji;
        }
        else
        {
            const double hc_kl = HC_K / a.wavelength[la];
            const double g = a.ratio[(size_t)t.row * Ns + k] * exp(-hc_kl / a.temperature[k]);
            Vij = p[0];
            Vji = g * Vij;
            Uji = p[2] * Vji;
        }
        const double ni = a.n[(size_t)t.gi * Ns + k], nj = a.n[(size_t)t.gj * Ns + k];
        const double c = ni * Vij - nj * Vji;
        const double e = nj * Uji;
        chi[0] += c;
        eta[0] += e;
        if (t.pol >= 0)
        {
            // :515-531.  chiNoProfile = chi / phi is kept as a division, as the reference writes it.
            const auto P = pt.pol(a, t);
            const double ph = pt.phi(a, t);
            const double cnp = c / ph;
            chi[1] += cnp * P[0];
            chi[2] += cnp * P[1];
            chi[3] += cnp * P[2];
            chi[4] += cnp * P[3];
            chi[5] += cnp * P[4];
            chi[6] += cnp * P[5];
            const double enp = e / ph;
            eta[1] += enp * P[0];
            eta[2] += enp * P[1];
            eta[3] += enp * P[2];
        }
    }
    const size_t lk = (size_t)la * Ns + k;
    const double sca = a.bgSca[lk];
    if (a.hasJ20)
    {
        // :575-583; J20 dagger is what J20 held when J is updated, zero otherwise (J20Dag is only filled then)
        const double mu2 = a.muz[mu] * a.muz[mu];
        const double wJ20_I = inv2root2 * (3.0 * mu2 - 1.0);
        const double wJ20_Q = inv2root2 * 3.0 * (mu2 - 1.0);
        const double j20 = a.updateJ ? a.J20[lk] : 0.0;
        eta[0] += wJ20_I * sca * j20;
        eta[1] += wJ20_Q * sca * j20;
    }
    // :585-602; JDag = J(la) when J is updated, zero otherwise (as in the reference: JDag is only filled then)
    const double jdag = a.updateJ ? a.J[lk] : 0.0;
    chi[0] += a.bgChi[lk];
    row[0] = chi[0];
    row[7 * Ns] = (eta[0] + a.bgEta[lk] + sca * jdag) / chi[0];
    if (polF)
    {
        for (int m = 1; m < 7; ++m)
            row[m * Ns] = chi[m];
        for (int m = 1; m < 4; ++m)
            row[(7 + m) * Ns] = eta[m] / chi[0];
    }
}

// Iupw of the ray's first point (:365-410 / FormalScalar.cpp:551-597): Stokes I only
DEVINL double upwind_intensity(const StokesArgs& a, RowIn chi0, int la, int mu, int d, double zmu)
{
    const int Ns = a.Ns;
    const int dk = d ? -1 : 1;
    const int kStart = d ? Ns - 1 : 0;
    const double dtau_uw = 0.5 * zmu * (chi0[kStart] + chi0[kStart + dk]) * fabs(a.height[kStart] - a.height[kStart + dk]);
    const double wav = a.wavelength[la];
    if (d)
    {
        if (a.lowerType == LWHIP_BC_THERMALISED)
        {
            const double B0 = d_planck(a.temperature[Ns - 2], wav), B1 = d_planck(a.temperature[Ns - 1], wav);
            return B1 - (B0 - B1) / dtau_uw;
        }
        if (a.lowerType == LWHIP_BC_CALLABLE)
        {
            const int m = a.lowerIdx[mu * 2 + d];
            return m >= 0 ? a.lowerBc[(size_t)la * a.lowerNmu + m] : 0.0;
        }
    }
    else
    {
        if (a.upperType == LWHIP_BC_THERMALISED)
        {
            const double B0 = d_planck(a.temperature[0], wav), B1 = d_planck(a.temperature[1], wav);
            return B0 - (B1 - B0) / dtau_uw;
        }
        if (a.upperType == LWHIP_BC_CALLABLE)
        {
            const int m = a.upperIdx[mu * 2 + d];
            return m >= 0 ? a.upperBc[(size_t)la * a.upperNmu + m] : 0.0;
        }
    }
    return 0.0;
}

// K of stokes_K (:119-142) as its six independent entries u = (K01, K02, K03, K12, K13, K23); K is symmetric in its first
// row and column and antisymmetric in the 3 x 3 block below them (K10 = u0, K21 = -u3, K31 = -u4, K32 = -u5)
DEVINL void stokes_k6(RowIn row, int Ns, int k, double (&u)[6])
{
    const double chiI = row[k];
    u[0] = row[1 * Ns + k] / chiI;
    u[1] = row[2 * Ns + k] / chiI;
    u[2] = row[3 * Ns + k] / chiI;
    u[3] = row[6 * Ns + k] / chiI;
    u[4] = -(row[5 * Ns + k] / chiI);
    u[5] = row[4 * Ns + k] / chiI;
}
DEVINL void expand_k(const double (&u)[6], double (&K)[4][4])
{
    K[0][0] = 0.0; K[0][1] = u[0];  K[0][2] = u[1];  K[0][3] = u[2];
    K[1][0] = u[0]; K[1][1] = 0.0;  K[1][2] = u[3];  K[1][3] = u[4];
    K[2][0] = u[1]; K[2][1] = -u[3]; K[2][2] = 0.0;  K[2][3] = u[5];
    K[3][0] = u[2]; K[3][1] = -u[4]; K[3][2] = -u[5]; K[3][3] = 0.0;
}
// prod(a, b, c) of :144-152: c(j, i) = sum_k a(k, i) b(j, k), from zero in k order
DEVINL void prod44(const double (&A)[4][4], double (&C)[4][4])
{
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i)
        {
            double s = 0.0;
#pragma unroll
            for (int q = 0; q < 4; ++q)
                s += A[q][i] * A[j][q];
            C[j][i] = s;
        }
}

// piecewise_bezier3_1d_impl (FormalScalar.cpp:209-325) without the operator; I0 at every depth into `out` if given
DEVINL double scalar_bezier3(const StokesArgs& a, RowIn chi, RowIn S, double zmu, int d, double Iupw, RowOut out)
{
    const int Ns = a.Ns;
    const double* h = a.height;
    int dk = -1, k_start = Ns - 1, k_end = 0;
    if (!d)
    {
        dk = 1;
        k_start = 0;
        k_end = Ns - 1;
    }
    double I_upw = Iupw;
    if (out)
        out[k_start] = I_upw;
    int k = k_start + dk;
    double ds_uw = fabs(h[k] - h[k - dk]) * zmu;
    double ds_dw = fabs(h[k + dk] - h[k]) * zmu;
    double dx_uw = (chi[k] - chi[k - dk]) / ds_uw;
    double dx_c = d_cent_deriv(ds_uw, ds_dw, chi[k - dk], chi[k], chi[k + dk]);
    double Cuw = chi[k - dk] + (ds_uw / 3.0) * dx_uw;
    double C0 = chi[k] - (ds_uw / 3.0) * dx_c;
    double dtau_uw = ds_uw * (chi[k] + chi[k - dk] + Cuw + C0) * 0.25;
    double dS_uw = (S[k] - S[k - dk]) / dtau_uw;
    double ds_dw2 = 0.0, dtau_dw = 0.0;
    for (; k != k_end - dk; k += dk)
    {
        ds_dw2 = fabs(h[k + 2 * dk] - h[k + dk]) * zmu;
        const double dx_dw = d_cent_deriv(ds_dw, ds_dw2, chi[k], chi[k + dk], chi[k + 2 * dk]);
        Cuw = chi[k] + (ds_dw / 3.0) * dx_c;
        C0 = chi[k + dk] - (ds_dw / 3.0) * dx_dw;
        dtau_dw = ds_dw * (chi[k] + chi[k + dk] + Cuw + C0) * 0.25;
        double alpha, beta, gamma, delta, edt;
        d_bezier3_coeffs(dtau_uw, alpha, beta, gamma, delta, edt);
        const double dS_c = d_cent_deriv(dtau_uw, dtau_dw, S[k - dk], S[k], S[k + dk]);
        Cuw = S[k - dk] + (dtau_uw / 3.0) * dS_uw;
        C0 = S[k] - (dtau_uw / 3.0) * dS_c;
        const double Ik = I_upw * edt + alpha * S[k - dk] + beta * S[k] + gamma * Cuw + delta * C0;
        if (out)
            out[k] = Ik;
        I_upw = Ik;
        ds_uw = ds_dw;
        ds_dw = ds_dw2;
        dx_uw = dx_c;
        dx_c = dx_dw;
        dtau_uw = dtau_dw;
        dS_uw = dS_c;
    }
    k = k_end - dk;
    ds_dw = fabs(h[k + dk] - h[k]) * zmu;
    const double dx_dw = (chi[k + dk] - chi[k]) / ds_dw;
    Cuw = chi[k] + (ds_dw / 3.0) * dx_c;
    C0 = chi[k + dk] - (ds_dw / 3.0) * dx_dw;
    dtau_dw = ds_dw * (chi[k] + chi[k + dk] + Cuw + C0) * 0.25;
    {
        double alpha, beta, gamma, delta, edt;
        d_bezier3_coeffs(dtau_uw, alpha, beta, gamma, delta, edt);
        const double dS_c = d_cent_deriv(dtau_uw, dtau_dw, S[k - dk], S[k], S[k + dk]);
        Cuw = S[k - dk] + dtau_uw / 3.0 * dS_uw;
        C0 = S[k] - dtau_uw / 3.0 * dS_c;
        const double Ik = I_upw * edt + alpha * S[k - dk] + beta * S[k] + gamma * Cuw + delta * C0;
        if (out)
            out[k] = Ik;
        I_upw = Ik;
    }
    k = k_end;
    dtau_uw = 0.5 * zmu * (chi[k] + chi[k - dk]) * fabs(h[k] - h[k - dk]);
    dS_uw = (S[k] - S[k - dk]) / dtau_uw;
    double w0, w1;
    d_w2(dtau_uw, w0, w1);
    const double Ik = (1.0 - w0) * I_upw + w0 * S[k] - w1 * dS_uw;
    if (out)
        out[k] = Ik;
    return Ik;
}

// piecewise_stokes_bezier3_1d_impl (:166-340); I(0..3) of the last point (k_end) returned, I and Q at every depth into
// out0 / out1 if given
DEVINL void stokes_bezier3(const StokesArgs& a, RowIn row, double zmu, int d, double Iupw, RowOut out0, RowOut out1,
                           double (&Iend)[4])
{
    const int Ns = a.Ns;
    const double* h = a.height;
    const RowIn chi = row;
    const RowIn Srow = row + 7 * Ns;
    int dk = -1, k_start = Ns - 1, k_end = 0;
    if (!d)
    {
        dk = 1;
        k_start = 0;
        k_end = Ns - 1;
    }
    double I[4] = { Iupw, 0.0, 0.0, 0.0 };
    if (out0)
    {
        out0[k_start] = I[0];
        out1[k_start] = I[1];
    }
    int k = k_start + dk;
    double ds_uw = fabs(h[k] - h[k - dk]) * zmu;
    double ds_dw = fabs(h[k + dk] - h[k]) * zmu;
    double dx_uw = (chi[k] - chi[k - dk]) / ds_uw;
    double dx_c = d_cent_deriv(ds_uw, ds_dw, chi[k - dk], chi[k], chi[k + dk]);
    double c1 = chi[k] - (ds_uw / 3.0) * dx_c;
    double c2 = chi[k - dk] + (ds_uw / 3.0) * dx_uw;
    double dtau_uw = ds_uw * (chi[k] + chi[k - dk] + c1 + c2) * 0.25;

    double Ku[6], K0[6], Kd[6], dKu[6], dK0[6];
    double Su[4], S0[4], Sd[4], dSu[4], dS0[4];
    stokes_k6(row, Ns, k_start, Ku);
    stokes_k6(row, Ns, k, K0);
#pragma unroll
    for (int m = 0; m < 4; ++m)
    {
        Su[m] = Srow[m * Ns + k_start];
        S0[m] = Srow[m * Ns + k];
        Sd[m] = 0.0;
        dS0[m] = 0.0;
    }
#pragma unroll
    for (int m = 0; m < 4; ++m)
        dSu[m] = (S0[m] - Su[m]) / dtau_uw;
#pragma unroll
    for (int m = 0; m < 6; ++m)
    {
        dKu[m] = (K0[m] - Ku[m]) / dtau_uw;
        Kd[m] = 0.0;
        dK0[m] = 0.0;
    }
    double ds_dw2 = 0.0, dtau_dw = 0.0, dx_dw = 0.0;
    for (; k != k_end + dk; k += dk)
    {
        if (k == k_end)
        {
            // linear on the end: no downwind point
#pragma unroll
            for (int m = 0; m < 4; ++m)
                dS0[m] = (S0[m] - Su[m]) / dtau_uw;
#pragma unroll
            for (int m = 0; m < 6; ++m)
                dK0[m] = (K0[m] - Ku[m]) / dtau_uw;
        }
        else
        {
            if (k_end - k == dk)
                dx_dw = (chi[k + dk] - chi[k]) / ds_dw;
            else
            {
                ds_dw2 = fabs(h[k + 2 * dk] - h[k + dk]) * zmu;
                dx_dw = d_cent_deriv(ds_dw, ds_dw2, chi[k], chi[k + dk], chi[k + 2 * dk]);
            }
            c1 = chi[k] + (ds_dw / 3.0) * dx_c;
            c2 = chi[k + dk] - (ds_dw / 3.0) * dx_dw;
            dtau_dw = ds_dw * (chi[k] + chi[k + dk] + c1 + c2) * 0.25;
            stokes_k6(row, Ns, k + dk, Kd);
#pragma unroll
            for (int m = 0; m < 4; ++m)
                Sd[m] = Srow[m * Ns + k + dk];
            // (the lower entries of dK are the negated upper ones: cent_deriv is odd in its three values, up to the sign of
            // a zero)
#pragma unroll
            for (int m = 0; m < 6; ++m)
                dK0[m] = d_cent_deriv(dtau_uw, dtau_dw, Ku[m], K0[m], Kd[m]);
#pragma unroll
            for (int m = 0; m < 4; ++m)
                dS0[m] = d_cent_deriv(dtau_uw, dtau_dw, Su[m], S0[m], Sd[m]);
        }
        double mKu[4][4], mK0[4][4], mdKu[4][4], mdK0[4][4], Ku2[4][4], K02[4][4];
        expand_k(Ku, mKu);
        expand_k(K0, mK0);
        expand_k(dKu, mdKu);
        expand_k(dK0, mdK0);
        // (the diagonal of dK is (0 - 0) / dtau = 0 in the reference too)
        prod44(mKu, Ku2);
        prod44(mK0, K02);
        double alpha, beta, gamma, delta, edt;
        d_bezier3_coeffs(dtau_uw, alpha, beta, gamma, delta, edt);
        double Md[4][4], V0[4];
        const double t3 = dtau_uw / 3.0;
#pragma unroll
        for (int j = 0; j < 4; ++j)
        {
            double v = 0.0;
#pragma unroll
            for (int i = 0; i < 4; ++i)
            {
                const double id = (i == j) ? 1.0 : 0.0;
                const double dd = t3 * (Ku2[j][i] + mKu[j][i] - mdKu[j][i]) - mKu[j][i];
                const double e = t3 * (K02[j][i] + mK0[j][i] - mdK0[j][i]) + mK0[j][i];
                Md[j][i] = id + beta * mK0[j][i] + delta * e;
                const double Ma = edt * id - alpha * mKu[j][i] + gamma * dd;
                const double Mb = alpha * id + gamma * (id - t3 * mKu[j][i]);
                const double Mc = beta * id + delta * (id + t3 * mK0[j][i]);
                v += Ma * I[i] + Mb * Su[i] + Mc * S0[i];
            }
            V0[j] = v + t3 * (gamma * dSu[j] - delta * dS0[j]);
        }
        if (!d_solve_lin_eq_reg<4>(Md, V0))
            *a.singular = 1;
#pragma unroll
        for (int m = 0; m < 4; ++m)
            I[m] = V0[m];
        if (out0)
        {
            out0[k] = I[0];
            out1[k] = I[1];
        }
#pragma unroll
        for (int m = 0; m < 4; ++m)
        {
            Su[m] = S0[m];
            S0[m] = Sd[m];
            dSu[m] = dS0[m];
        }
#pragma unroll
        for (int m = 0; m < 6; ++m)
        {
            Ku[m] = K0[m];
            K0[m] = Kd[m];
            dKu[m] = dK0[m];
        }
        dtau_uw = dtau_dw;
        ds_uw = ds_dw;
        ds_dw = ds_dw2;
        dx_uw = dx_c;
        dx_c = dx_dw;
    }
    (void)dx_uw;
#pragma unroll
    for (int m = 0; m < 4; ++m)
        Iend[m] = I[m];
}

// One ray (la, mu, d) of a context whose rows are `row`: its march, I and Q at every depth into out0 / out1 (updateJ), and
// the emergent Stokes vector into a.I / a.Quv
DEVINL void stokes_march_ray(const StokesArgs& a, RowIn row, RowOut out0, RowOut out1, int la, int mu, int d, int nDir)
{
    const int Ns = a.Ns;
    const double zmu = 1.0 / a.muz[mu];
    const double Iupw = upwind_intensity(a, row, la, mu, d, zmu);
    double I[4] = { 0.0, 0.0, 0.0, 0.0 };
    if (polarised_la(a, la))
    {
        double Iend[4];
        stokes_bezier3(a, row, zmu, d, Iupw, out0, out1, Iend);
        // I(., 0): the end of an up-going ray; the down-going rays start at k = 0
        if (d)
            for (int m = 0; m < 4; ++m)
                I[m] = Iend[m];
        else
            I[0] = Iupw;
    }
    else
    {
        // the scalar solver fills Stokes I only; Q, U, V stay exact zeros here (see lwhip_full_stokes_fs)
        const double Iend = scalar_bezier3(a, row, row + 7 * Ns, zmu, d, Iupw, out0);
        if (out1)
            for (int k = 0; k < Ns; ++k)
                out1[k] = 0.0;
        I[0] = d ? Iend : Iupw;
    }
    // the up-going ray of an angle is written last (also with both directions), so it is what I and Quv keep
    if (d == 1 || nDir == 1)
    {
        const size_t Nla = (size_t)a.Nla;
        const size_t o = (size_t)la * a.Nr + mu;
        a.I[o] = I[0];
        a.Quv[0 * Nla * a.Nr + o] = I[1];
        a.Quv[1 * Nla * a.Nr + o] = I[2];
        a.Quv[2 * Nla * a.Nr + o] = I[3];
    }
}

// J(k) = sum_{mu, dir} 0.5 wmu I(0, k), J20(k) = sum wmu (wJ20_I I(0, k) + wJ20_Q I(1, k)) (:635-649) and
// dJ = max_k |1 - JDag / J| (:652-659) of one wavelength; isc(mu, dd, q, k): I (q = 0) or Q (q = 1) of ray (mu, dd) at k
template <typename F> DEVINL void stokes_j_lambda(const StokesArgs& a, int la, int nDir, F isc)
{
    const int Ns = a.Ns;
    const double inv2root2 = 1.0 / (2.0 * sqrt(2.0));
    double dJMax = 0.0;
    for (int k = 0; k < Ns; ++k)
    {
        double acc = 0.0, acc20 = 0.0;
        for (int mu = 0; mu < a.Nr; ++mu)
        {
            const double wmu = a.wmu[mu];
            const double mu2 = a.muz[mu] * a.muz[mu];
            const double wJ20_I = inv2root2 * (3.0 * mu2 - 1.0);
            const double wJ20_Q = inv2root2 * 3.0 * (mu2 - 1.0);
            for (int dd = 0; dd < nDir; ++dd)
            {
                acc += 0.5 * wmu * isc(mu, dd, 0, k);
                if (a.hasJ20)
                    acc20 += (wJ20_I * wmu) * isc(mu, dd, 0, k) + (wJ20_Q * wmu) * isc(mu, dd, 1, k);
            }
        }
        const size_t lk = (size_t)la * Ns + k;
        const double jdag = a.J[lk];
        a.J[lk] = acc;
        if (a.hasJ20)
            a.J20[lk] = acc20;
        const double dJ = fabs(1.0 - jdag / acc);
        dJMax = (dJ < dJMax) ? dJMax : dJ; // std::max(dJ, dJMax)
    }
    a.dJ[la] = dJMax;
}

// one chunk: columns [col0, col0 + ncol) x wavelengths [la0, la0 + nla)
struct StokesChunk
{
    const StokesArgs* cols; // [n] the columns' argument blocks
    int32_t col0, ncol, la0, nla;
    int32_t nDir, dir0, blocksPerCol, Ns;
    int32_t Nr, updateJ;
    double* scratch; // [ncol * blocksPerCol][ST_ROWS][Ns][64]
    double* Isc;     // [ncol * blocksPerCol][2][Ns][64]: I and Q at every depth (updateJ)
};

// (la, mu, d) of ray r of a column in the chunk
DEVINL void chunk_ray(const StokesChunk& b, int r, int& la, int& mu, int& d)
{
    d = b.dir0 + r % b.nDir;
    mu = (r / b.nDir) % b.Nr;
    la = b.la0 + r / (b.nDir * b.Nr);
}

// one workgroup of 256 threads per block of 64 rays: 64 lanes x 4 depth points at a time
__global__ void __launch_bounds__(256) stokes_gather_kernel(const StokesChunk b)
{
    const int blk = blockIdx.x;
    const int lane = threadIdx.x % SB_LANES;
    const StokesArgs a = b.cols[b.col0 + blk / b.blocksPerCol];
    const int r = (blk % b.blocksPerCol) * SB_LANES + lane;
    if (r >= b.nla * b.Nr * b.nDir)
        return;
    int la, mu, d;
    chunk_ray(b, r, la, mu, d);
    const int Ns = b.Ns;
    double* base = b.scratch + (size_t)blk * ST_ROWS * Ns * SB_LANES + lane;
    for (int k = threadIdx.x / SB_LANES; k < Ns; k += blockDim.x / SB_LANES)
        stokes_gather_point(a, StoredProfiles{}, la, mu, d, k, RowOut{ base + (size_t)k * SB_LANES });
}
// The observer gather: the same rows, in the same layout, for the rays (lambda, m) of an observer request, the profiles formed
// in place; obs: [n] the columns' observer blocks, indexed as b.cols.  Lanes are rays as above, so neighbouring lanes sit at
// different wavelengths and diverge inside the Faddeeva algorithm ("Full-Stokes observer rays").
__global__ void __launch_bounds__(256) stokes_observer_gather_kernel(const StokesChunk b, const ObsCol* __restrict__ obs)
{
    const int blk = blockIdx.x;
    const int lane = threadIdx.x % SB_LANES;
    const int col = b.col0 + blk / b.blocksPerCol;
    const StokesArgs a = b.cols[col];
    const int r = (blk % b.blocksPerCol) * SB_LANES + lane;
    if (r >= b.nla * b.Nr * b.nDir)
        return;
    int la, mu, d;
    chunk_ray(b, r, la, mu, d);
    const int Ns = b.Ns;
    const ObserverProfiles prof{ obs[col] };
    double* base = b.scratch + (size_t)blk * ST_ROWS * Ns * SB_LANES + lane;
    for (int k = threadIdx.x / SB_LANES; k < Ns; k += blockDim.x / SB_LANES)
        stokes_gather_point(a, prof, la, mu, d, k, RowOut{ base + (size_t)k * SB_LANES });
}

// one wavefront per block of 64 rays, a lane per ray.  One wavefront per SIMD: held to two (256 registers) the march spills
// 37 VGPRs to scratch memory ("Full Stokes")
__global__ void __launch_bounds__(64) stokes_march_kernel(const StokesChunk b)
{
    const int blk = blockIdx.x;
    const int lane = threadIdx.x;
    const StokesArgs a = b.cols[b.col0 + blk / b.blocksPerCol];
    const int r = (blk % b.blocksPerCol) * SB_LANES + lane;
    if (r >= b.nla * b.Nr * b.nDir)
        return;
    int la, mu, d;
    chunk_ray(b, r, la, mu, d);
    const int Ns = b.Ns;
    const RowIn row{ b.scratch + (size_t)blk * ST_ROWS * Ns * SB_LANES + lane };
    const RowOut out0{ b.updateJ ? b.Isc + (size_t)blk * 2 * Ns * SB_LANES + lane : nullptr };
    const RowOut out1{ b.updateJ ? out0.p + (size_t)Ns * SB_LANES : nullptr };
    stokes_march_ray(a, row, out0, out1, la, mu, d, b.nDir);
}

// J, J20 and dJ: one thread per wavelength of the chunk, blockIdx.y = the column in the chunk
__global__ void stokes_j_kernel(const StokesChunk b)
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

// what a context, or a batch, keeps for its full-Stokes formal solutions
struct StokesBatch
{
    DevBuf<StokesArgs> args; // the columns' argument blocks, as argsHost
    std::vector<StokesArgs> argsHost;
    DevBuf<double> scratch, Isc; // one chunk's rows and I / Q profiles
    DevBuf<double> tail;         // [n][Nla] dJ of every column, then n int32 singular flags
    PinnedBlock tailPinned;
    // observer rays: the staged request [args | observer blocks | per column: muz, projections, v_z, lowerBc, lowerIdx] and
    // its results [per column: I, Quv | flags]
    DevBuf<unsigned char> obsIn, obsOut;
    PinnedBlock obsInPinned, obsOutPinned;
};

void stokes_batch_release(StokesBatch* s)
{
    if (s)
    {
        s->tailPinned.release();
        s->obsInPinned.release();
        s->obsOutPinned.release();
    }
    delete s;
}

namespace
{
StokesArgs stokes_args(lwhip_context* c, int updateJ, double* dJ, int32_t* singular)
{
    const StokesState& s = c->stokes;
    StokesArgs a{};
    a.Ns = c->Ns;
    a.Nr = c->Nrays;
    a.Nla = c->Nla;
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
    a.I = c->I.p;
    a.Quv = s.Quv.p;
    a.dJ = dJ;
    a.singular = singular;
    return a;
}

// formal_sol_full_stokes_impl's serial loop: dJMax = max_idx(dJ, dJMax, maxIdx, la) (FormalStokes.cpp:708-714)
void stokes_max_idx(const double* dJ, int Nla, lwhip_iter_result& r)
{
    double dJMax = 0.0;
    int maxIdx = 0;
    for (int la = 0; la < Nla; ++la)
    {
        if (dJ[la] < dJMax)
            maxIdx = la;
        else
            dJMax = dJ[la];
    }
    r.dJMax = dJMax;
    r.dJMaxIdx = maxIdx;
}

// One call of the driver: n columns whose argument blocks are on the device, the wavelengths [la0, la1) of their grid, Nr rays
// per wavelength.  obs: the columns' observer blocks (the observer gather forms the profiles), or null (the stored profiles).
struct StokesCall
{
    const StokesArgs* args; // device [n]
    const ObsCol* obs;      // device [n], or null
    int32_t* flags;         // device [n]: set where a 4 x 4 system is singular; cleared here
    int n, Ns, Nr, la0, la1, updateJ, upOnly;
};

// The driver of every full-Stokes formal solution: everything queued on c0's stream, the rows in `sb` and at most capBytes of
// them.  Nothing is waited for unless the scratch has to grow; the caller copies its results back.
int stokes_fs_run(lwhip_context* c0, StokesBatch& sb, const StokesCall& call, size_t capBytes)
{
    const int n = call.n, Ns = call.Ns, Nr = call.Nr, updateJ = call.updateJ;
    const int Nla = call.la1 - call.la0;
    const int nDir = call.upOnly ? 1 : 2;
    // chunks of (columns x wavelength range) whose rows stay within the cap.  Two debug knobs (LWHIP_DEBUG) make small chunks
    // for the tests: LWHIP_STOKES_BATCH_RAYS caps the rays of a chunk instead, LWHIP_STOKES_CHUNK_LA caps its wavelengths
    const size_t rowsPerRay = (size_t)ST_ROWS + (updateJ ? 2 : 0);
    size_t maxBlocks = std::max<size_t>(1, capBytes / (rowsPerRay * Ns * sizeof(double) * SB_LANES));
    const int dbgRays = dbg_env_int("LWHIP_STOKES_BATCH_RAYS", 0);
    if (dbgRays > 0)
        maxBlocks = std::max<size_t>(1, (size_t)dbgRays / SB_LANES);
    const size_t raysPerLa = (size_t)Nr * nDir;
    int nlaChunk = (int)std::min<size_t>((size_t)Nla, std::max<size_t>(1, maxBlocks * SB_LANES / raysPerLa));
    const int dbgLa = dbg_env_int("LWHIP_STOKES_CHUNK_LA", 0);
    if (dbgLa > 0)
        nlaChunk = std::min(nlaChunk, dbgLa);
    const size_t blocksPerColMax = (nlaChunk * raysPerLa + SB_LANES - 1) / SB_LANES;
    // (65 535: the columns of a chunk are the second grid dimension of stokes_j_kernel)
    const int colsChunk = (int)std::max<size_t>(1, std::min<size_t>({ (size_t)n, maxBlocks / blocksPerColMax, 65535 }));
    const size_t blocksMax = (size_t)colsChunk * blocksPerColMax;
    if (sb.scratch.n < blocksMax * ST_ROWS * Ns * SB_LANES || (updateJ && sb.Isc.n < blocksMax * 2 * Ns * SB_LANES))
    {
        HIP_TRY(hipStreamSynchronize(c0->stream));
        if (sb.scratch.n < blocksMax * ST_ROWS * Ns * SB_LANES)
            HIP_TRY(sb.scratch.alloc(c0->mem, blocksMax * ST_ROWS * Ns * SB_LANES, false));
        if (updateJ && sb.Isc.n < blocksMax * 2 * Ns * SB_LANES)
            HIP_TRY(sb.Isc.alloc(c0->mem, blocksMax * 2 * Ns * SB_LANES, false));
    }
    HIP_TRY(hipMemsetAsync(call.flags, 0, (size_t)n * sizeof(int32_t), c0->stream));
    StokesChunk ch{};
    ch.cols = call.args;
    ch.nDir = nDir;
    ch.dir0 = call.upOnly ? 1 : 0;
    ch.Ns = Ns;
    ch.Nr = Nr;
    ch.updateJ = updateJ ? 1 : 0;
    ch.scratch = sb.scratch.p;
    ch.Isc = sb.Isc.p;
    for (int col0 = 0; col0 < n; col0 += colsChunk)
        for (int la0 = call.la0; la0 < call.la1; la0 += nlaChunk)
        {
            ch.col0 = col0;
            ch.ncol = std::min(colsChunk, n - col0);
            ch.la0 = la0;
            ch.nla = std::min(nlaChunk, call.la1 - la0);
            ch.blocksPerCol = (int)((ch.nla * raysPerLa + SB_LANES - 1) / SB_LANES);
            const unsigned nBlk = (unsigned)ch.ncol * ch.blocksPerCol;
            if (call.obs)
                LWHIP_LAUNCH(stokes_observer_gather_kernel, dim3(nBlk), dim3(256), 0, c0->stream, ch, call.obs);
            else
                LWHIP_LAUNCH(stokes_gather_kernel, dim3(nBlk), dim3(256), 0, c0->stream, ch);
            LWHIP_LAUNCH(stokes_march_kernel, dim3(nBlk), dim3(SB_LANES), 0, c0->stream, ch);
            if (updateJ)
                LWHIP_LAUNCH(stokes_j_kernel, dim3((ch.nla + 63) / 64, ch.ncol), dim3(64), 0, c0->stream, ch);
            HIP_TRY(hipGetLastError());
        }
    return LWHIP_OK;
}

// solve_lin_eq throws on a singular system (LuSolve.cpp:22-23): the first column whose flag is set
int stokes_singular(const int32_t* sing, int n, const std::string& what)
{
    for (int i = 0; i < n; ++i)
        if (sing[i])
            return fail(LWHIP_ERR_SINGULAR, what + ": Singular Matrix in the 4 x 4 DELO-Bezier3 step"
                                                + (n > 1 ? " of column " + std::to_string(i) : std::string()));
    return LWHIP_OK;
}

// formal_sol_full_stokes of the n columns `cols` (of batch `b`, or one context on its own: b null) on their own rays.  The
// columns have passed check_stokes_ctx / check_stokes_batch.
int stokes_fs_solve(lwhip_context* const* cols, int n, lwhip_batch* b, int updateJ, int upOnly, lwhip_iter_result* results,
                    StokesBatch*& slot, size_t capBytes, const char* whatC)
{
    const std::string what(whatC);
    auto column = [&](const char* pre, int i) { return n > 1 ? pre + std::to_string(i) : std::string(); };
    for (int i = 0; i < n; ++i)
        if (updateJ && cols[i]->JhostReg)
            return fail(LWHIP_ERR_UNSUPPORTED, what + ": updateJ with a mapped host J" + column(" in column ", i)
                                                   + " (lwhip_map_host_J(ctx, 0) first)");
    lwhip_context* c0 = cols[0];
    if (c0->Ns < 3)
        return fail(LWHIP_ERR_INVALID, what + ": needs at least 3 depth points");
    HIP_TRY(hipSetDevice(c0->device));
    {
        const int stp = b ? batch_ensure_profiles(b) : ensure_profiles(c0);
        if (stp != LWHIP_OK)
            return stp;
    }
    if (!slot)
        slot = new StokesBatch();
    StokesBatch& sb = *slot;
    const int Nla = c0->Nla;
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
        args[i] = stokes_args(cols[i], updateJ, sb.tail.p + (size_t)i * Nla, flags + i);
    if (sb.argsHost.size() != args.size() || std::memcmp(sb.argsHost.data(), args.data(), args.size() * sizeof(StokesArgs)) != 0)
    {
        HIP_TRY(hipStreamSynchronize(c0->stream)); // (nothing queued may still read the blocks about to be replaced)
        sb.argsHost = args;
        if (sb.args.n < (size_t)n)
            HIP_TRY(sb.args.alloc(c0->mem, (size_t)n, false));
        HIP_TRY(hipMemcpyAsync(sb.args.p, sb.argsHost.data(), (size_t)n * sizeof(StokesArgs), hipMemcpyHostToDevice, c0->stream));
    }
    StokesCall call{};
    call.args = sb.args.p;
    call.flags = flags;
    call.n = n;
    call.Ns = c0->Ns;
    call.Nr = c0->Nrays;
    call.la0 = 0;
    call.la1 = Nla;
    call.updateJ = updateJ ? 1 : 0;
    call.upOnly = upOnly ? 1 : 0;
    {
        const int stp = stokes_fs_run(c0, sb, call, capBytes);
        if (stp != LWHIP_OK)
            return stp;
    }
    if (updateJ)
        for (int i = 0; i < n; ++i)
            cols[i]->fpJValid = false;
    // one copy back: the dJ rows (updateJ) and the flags, then one wait
    const size_t off = updateJ ? 0 : (size_t)n * Nla;
    HIP_TRY(hipMemcpyAsync(sb.tailPinned.as<double>() + off, sb.tail.p + off, (tailN - off) * sizeof(double), hipMemcpyDeviceToHost,
                           c0->stream));
    HIP_TRY(hipStreamSynchronize(c0->stream));
    const double* dJ = sb.tailPinned.as<double>();
    for (int i = 0; i < n && results; ++i)
    {
        results[i].updatedJ = updateJ ? 1 : 0;
        results[i].dJMax = 0.0;
        results[i].dJMaxIdx = 0;
        if (updateJ)
            stokes_max_idx(dJ + (size_t)i * Nla, Nla, results[i]);
    }
    return stokes_singular((const int32_t*)(dJ + (size_t)n * Nla), n, what);
}

hipError_t stokes_init_voigt_table(int device)
{
    // (this unit's copy of the table of lwhip_voigt_dev.h, as rays_init_table)
    static std::atomic<bool> done[64];
    if (device >= 0 && device < 64 && done[device].load())
        return hipSuccess;
    const hipError_t e = voigt_fill_table();
    if (e == hipSuccess && device >= 0 && device < 64)
        done[device].store(true);
    return e;
}

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// Observer rays: cols[i] (which have passed check_stokes_ctx / check_stokes_batch) with request reqs[i].  Every other refusal
// comes first; then the request is staged as rays_run stages its own -- one pinned block [args | observer blocks | per column:
// muz, projections, v_z, lowerBc, lowerIdx], one copy up -- the driver runs with the observer gather, and I, Quv and the
// singular flags come back in one copy, after one wait.  The argument blocks that stokes_fs_solve keeps are not touched.
int stokes_rays_solve(lwhip_context* const* cols, int n, const lwhip_stokes_rays* reqs, StokesBatch*& slot, size_t capBytes,
                      const char* whatC)
{
    const std::string what(whatC);
    if (!reqs)
        return fail(LWHIP_ERR_INVALID, what + ": null request");
    int la0 = 0, la1 = 0;
    for (int i = 0; i < n; ++i)
    {
        const std::string col = n > 1 ? " (column " + std::to_string(i) + ")" : std::string();
        int a0 = 0, a1 = 0;
        const int chk = rays_check(cols[i], &reqs[i].rays, what, true, a0, a1);
        if (chk != LWHIP_OK)
            return n > 1 ? fail(chk, std::string(lwhip_last_error()) + col) : chk;
        const lwhip_stokes_rays& q = reqs[i];
        if (!q.cosGamma || !q.cos2chi || !q.sin2chi)
            return fail(LWHIP_ERR_INVALID, what + ": cosGamma, cos2chi and sin2chi [Nmu, Nspace] of the new directions are required" + col);
        if (!q.Quv)
            return fail(LWHIP_ERR_INVALID, what + ": Quv [3, Nla, Nmu] is required" + col);
        if (q.rays.depthChi || q.rays.depthEta || q.rays.depthI)
            return fail(LWHIP_ERR_INVALID, what + ": no depth output of the Stokes vector (depthChi, depthEta and depthI must be NULL)" + col);
        if (!cols[i]->lineWave.p)
            return fail(LWHIP_ERR_INVALID, what + ": the context has no line grids on the device" + col);
        if (i == 0)
        {
            la0 = a0;
            la1 = a1;
        }
        if (cols[i]->Ns != cols[0]->Ns || cols[i]->device != cols[0]->device || q.rays.Nmu != reqs[0].rays.Nmu || a0 != la0 || a1 != la1)
            return fail(LWHIP_ERR_INVALID, what + ": column " + std::to_string(i)
                                               + " differs from column 0 (depth points, Nmu and wavelength range are the same for "
                                                 "every column)");
    }
    lwhip_context* c0 = cols[0];
    const int Ns = c0->Ns, Nmu = reqs[0].rays.Nmu, nla = la1 - la0;
    HIP_TRY(hipSetDevice(c0->device));
    HIP_TRY(stokes_init_voigt_table(c0->device));
    if (!slot)
        slot = new StokesBatch();
    StokesBatch& sb = *slot;
    // ---- the staged request ------------------------------------------------------------------------------------------------
    const size_t nRayCol = (size_t)nla * Nmu;
    const size_t argsBytes = align256((size_t)n * sizeof(StokesArgs)), obsBytes = align256((size_t)n * sizeof(ObsCol));
    const size_t muBytes = align256((size_t)Nmu * sizeof(double)), projBytes = align256((size_t)3 * Nmu * Ns * sizeof(double));
    const size_t vzBytes = align256((size_t)Ns * sizeof(double)), bcBytes = align256(nRayCol * sizeof(double));
    const size_t idxBytes = align256((size_t)2 * Nmu * sizeof(int32_t));
    std::vector<size_t> colOff(n);
    size_t inBytes = argsBytes + obsBytes;
    for (int i = 0; i < n; ++i)
    {
        colOff[i] = inBytes;
        inBytes += muBytes + projBytes + (reqs[i].rays.vz ? vzBytes : 0);
        if (cols[i]->prob.zLowerBc.type == LWHIP_BC_CALLABLE)
            inBytes += bcBytes + idxBytes;
    }
    // out: per column I [nla, Nmu] and Quv [3, nla, Nmu], then the n flags
    const size_t perColOut = 4 * nRayCol * sizeof(double);
    const size_t outBytes = (size_t)n * perColOut + (size_t)n * sizeof(int32_t);
    if (sb.obsIn.n < inBytes || sb.obsOut.n < outBytes)
    {
        HIP_TRY(hipStreamSynchronize(c0->stream));
        if (sb.obsIn.n < inBytes)
            HIP_TRY(sb.obsIn.alloc(c0->mem, inBytes, false));
        if (sb.obsOut.n < outBytes)
            HIP_TRY(sb.obsOut.alloc(c0->mem, outBytes, false));
    }
    HIP_TRY(sb.obsInPinned.reserve(c0->device, inBytes, c0->stream));
    HIP_TRY(sb.obsOutPinned.reserve(c0->device, outBytes, c0->stream));
    unsigned char* hin = sb.obsInPinned.as<unsigned char>();
    unsigned char* din = sb.obsIn.p;
    StokesArgs* ha = (StokesArgs*)hin;
    ObsCol* ho = (ObsCol*)(hin + argsBytes);
    int32_t* flags = (int32_t*)(sb.obsOut.p + (size_t)n * perColOut);
    for (int i = 0; i < n; ++i)
    {
        lwhip_context* c = cols[i];
        const lwhip_stokes_rays& q = reqs[i];
        const StokesState& st = c->stokes;
        size_t off = colOff[i];
        auto stage = [&](const void* src, size_t bytes, size_t padded) {
            std::memcpy(hin + off, src, bytes);
            const unsigned char* dev = din + off;
            off += padded;
            return dev;
        };
        // the column as the march sees it: the context's state, the request's directions, boundary data and outputs.  Rows
        // are addressed by the context's la, so the request's arrays are taken as if they began at row 0
        StokesArgs a = stokes_args(c, 0, nullptr, flags + i);
        const ptrdiff_t rowShift = (ptrdiff_t)la0 * Nmu;
        a.Nr = Nmu;
        a.Nla = nla;
        a.muz = (const double*)stage(q.rays.muz, (size_t)Nmu * sizeof(double), muBytes);
        a.wmu = nullptr;
        ObsCol o{};
        o.cosGamma = (const double*)(din + off);
        o.cos2chi = o.cosGamma + (size_t)Nmu * Ns;
        o.sin2chi = o.cos2chi + (size_t)Nmu * Ns;
        std::memcpy(hin + off, q.cosGamma, (size_t)Nmu * Ns * sizeof(double));
        std::memcpy(hin + off + (size_t)Nmu * Ns * sizeof(double), q.cos2chi, (size_t)Nmu * Ns * sizeof(double));
        std::memcpy(hin + off + (size_t)2 * Nmu * Ns * sizeof(double), q.sin2chi, (size_t)Nmu * Ns * sizeof(double));
        off += projBytes;
        if (q.rays.vz)
            o.vz = (const double*)stage(q.rays.vz, (size_t)Ns * sizeof(double), vzBytes);
        if (a.lowerType == LWHIP_BC_CALLABLE)
        {
            a.lowerBc = (const double*)stage(q.rays.lowerBc, nRayCol * sizeof(double), bcBytes) - rowShift;
            int32_t* idx = (int32_t*)(hin + off);
            for (int m = 0; m < Nmu; ++m)
            {
                idx[2 * m] = -1;
                idx[2 * m + 1] = m;
            }
            a.lowerIdx = (const int32_t*)(din + off);
            off += idxBytes;
            a.lowerNmu = Nmu;
        }
        double* out = (double*)(sb.obsOut.p + (size_t)i * perColOut);
        a.I = out - rowShift;
        a.Quv = out + nRayCol - rowShift;
        ha[i] = a;
        o.ev = st.ev.p;
        o.polComp = st.polComp.p;
        o.alpha = st.alpha.p;
        o.shift = st.comp.p;
        o.strength = st.comp.p + st.nComp;
        o.vBroad = c->vBroad.p;
        o.aDamp = c->aDamp.p;
        o.lineWave = c->lineWave.p;
        o.B = st.B.p;
        o.vlosMu = c->vlosMu.p;
        o.muzCtx = c->muz.p;
        ho[i] = o;
    }
    HIP_TRY(c0->mem.h2d(din, hin, inBytes));
    StokesCall call{};
    call.args = (const StokesArgs*)din;
    call.obs = (const ObsCol*)(din + argsBytes);
    call.flags = flags;
    call.n = n;
    call.Ns = Ns;
    call.Nr = Nmu;
    call.la0 = la0;
    call.la1 = la1;
    call.updateJ = 0;
    call.upOnly = 1;
    {
        const int stp = stokes_fs_run(c0, sb, call, capBytes);
        if (stp != LWHIP_OK)
            return stp;
    }
    // ---- one copy back, one wait ---------------------------------------------------------------------------------------------
    unsigned char* hout = sb.obsOutPinned.as<unsigned char>();
    HIP_TRY(hipMemcpyAsync(hout, sb.obsOut.p, outBytes, hipMemcpyDeviceToHost, c0->stream));
    HIP_TRY(hipStreamSynchronize(c0->stream));
    for (int i = 0; i < n; ++i)
    {
        const double* o = (const double*)(hout + (size_t)i * perColOut);
        std::memcpy(reqs[i].rays.I, o, nRayCol * sizeof(double));
        std::memcpy(reqs[i].Quv, o + nRayCol, 3 * nRayCol * sizeof(double));
    }
    return stokes_singular((const int32_t*)(hout + (size_t)n * perColOut), n, what);
}
} // namespace
} // namespace lwhip

extern "C"
{
int lwhip_full_stokes_fs(lwhip_context* c, int updateJ, int upOnly, lwhip_iter_result* res)
{
    const char* what = "lwhip_full_stokes_fs";
    const int chk = check_stokes_ctx(c, what, true);
    if (chk != LWHIP_OK)
        return chk;
    lwhip_context* cols[1] = { c };
    return stokes_fs_solve(cols, 1, nullptr, updateJ, upOnly, res, c->stokesFs, (size_t)256 << 20, what);
}

int lwhip_batch_full_stokes_fs(lwhip_batch* b, int updateJ, int upOnly, lwhip_iter_result* results)
{
    const char* what = "lwhip_batch_full_stokes_fs";
    const int chk = check_stokes_batch(b, what);
    if (chk != LWHIP_OK)
        return chk;
    return stokes_fs_solve(b->ctxs.data(), (int)b->ctxs.size(), b, updateJ, upOnly, results, b->stokes, (size_t)1 << 30, what);
}

int lwhip_compute_stokes_rays(lwhip_context* c, const lwhip_stokes_rays* rays)
{
    const char* what = "lwhip_compute_stokes_rays";
    const int chk = check_stokes_ctx(c, what, true);
    if (chk != LWHIP_OK)
        return chk;
    lwhip_context* cols[1] = { c };
    return stokes_rays_solve(cols, 1, rays, c->stokesFs, (size_t)256 << 20, what);
}

int lwhip_batch_compute_stokes_rays(lwhip_batch* b, const lwhip_stokes_rays* perColumn)
{
    const char* what = "lwhip_batch_compute_stokes_rays";
    const int chk = check_stokes_batch(b, what);
    if (chk != LWHIP_OK)
        return chk;
    return stokes_rays_solve(b->ctxs.data(), (int)b->ctxs.size(), perColumn, b->stokes, (size_t)1 << 30, what);
}
}
