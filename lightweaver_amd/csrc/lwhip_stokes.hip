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
// memory ("Full Stokes").
#include "lwhip_host.h"
#include "lwhip_device.h"

// As in lwhip_pops.hip: no fused multiply-adds, so that the operations match the reference's one for one.
#pragma clang fp contract(off)

#include "lwhip_lu.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace lwhip
{
namespace
{
enum { ST_ROWS = 11 }; // per ray: chi[0..6], S[0..3]

struct StokesArgs
{
    int32_t Ns, Nr, la0, nla;
    int32_t Nla, nDir, dir0, updateJ;
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
    double* scratch; // [nla * Nr * nDir][ST_ROWS][Ns]
    double* Isc;     // [nla * Nr * nDir][2][Ns]: I and Q at every depth (updateJ)
    double* I;       // [Nla, Nr]
    double* Quv;     // [3, Nla, Nr]
    double* dJ;      // [Nla]
    int32_t* singular; // set when a depth point's 4 x 4 system is singular (solve_lin_eq throws there, LuSolve.cpp:22-23)
};

DEVINL bool polarised_la(const StokesArgs& a, int la) { return a.laPol[la] != 0 || a.hasJ20; }

__global__ void stokes_gather_kernel(const StokesArgs a)
{
    const size_t nRay = (size_t)a.nla * a.Nr * a.nDir;
    const size_t total = nRay * a.Ns;
    const double inv2root2 = 1.0 / (2.0 * sqrt(2.0));
    for (size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x)
    {
        const int Ns = a.Ns;
        const int k = (int)(idx % Ns);
        const size_t ray = idx / Ns;
        const int d = a.dir0 + (int)(ray % a.nDir);
        const int mu = (int)((ray / a.nDir) % a.Nr);
        const int la = a.la0 + (int)(ray / ((size_t)a.nDir * a.Nr));
        const bool polF = polarised_la(a, la);
        double chi[7] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
        double eta[4] = { 0.0, 0.0, 0.0, 0.0 };
        for (int q = a.laOff[la]; q < a.laOff[la + 1]; ++q)
        {
            const StokesTrans t = a.tr[a.laTr[q]];
            const int lt = la - t.Nblue;
            const double* p = a.par + t.parOff + 4 * (size_t)lt;
            double Vij, Vji, Uji;
            size_t pk = 0;
            if (t.type == LWHIP_LINE)
            {
                // Transition::uv (LwTransition.hpp:98-127) with gij of Atom::setup_wavelength (LwAtom.hpp:99-123)
                pk = (((size_t)lt * a.Nr + mu) * 2 + d) * Ns + k;
                Vij = p[0] * a.phi[t.phiOff + pk];
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
                const double* P = a.pol + t.polOff + pk;
                const size_t s = (size_t)t.polStride;
                const double ph = a.phi[t.phiOff + pk];
                const double cnp = c / ph;
                chi[1] += cnp * P[0];
                chi[2] += cnp * P[s];
                chi[3] += cnp * P[2 * s];
                chi[4] += cnp * P[3 * s];
                chi[5] += cnp * P[4 * s];
                chi[6] += cnp * P[5 * s];
                const double enp = e / ph;
                eta[1] += enp * P[0];
                eta[2] += enp * P[s];
                eta[3] += enp * P[2 * s];
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
        double* row = a.scratch + ray * ST_ROWS * Ns + k;
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
}

// Iupw of the ray's first point (:365-410 / FormalScalar.cpp:551-597): Stokes I only
DEVINL double upwind_intensity(const StokesArgs& a, const double* chi0, int la, int mu, int d, double zmu)
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
DEVINL void stokes_k6(const double* row, int Ns, int k, double (&u)[6])
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
DEVINL double scalar_bezier3(const StokesArgs& a, const double* chi, const double* S, double zmu, int d, double Iupw,
                             double* out)
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
DEVINL void stokes_bezier3(const StokesArgs& a, const double* row, double zmu, int d, double Iupw, double* out0,
                           double* out1, double (&Iend)[4])
{
    const int Ns = a.Ns;
    const double* h = a.height;
    const double* chi = row;
    const double* Srow = row + 7 * Ns;
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
    const double zmu = 1.0 / a.muz[mu];
    const double Iupw = upwind_intensity(a, row, la, mu, d, zmu);
    double* out0 = a.updateJ ? a.Isc + ray * 2 * Ns : nullptr;
    double* out1 = a.updateJ ? out0 + Ns : nullptr;
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
    if (d == 1 || a.nDir == 1)
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
// dJ = max_k |1 - JDag / J| (:652-659), one thread per wavelength
__global__ void stokes_j_kernel(const StokesArgs a)
{
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= a.nla)
        return;
    const int la = a.la0 + l;
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
            for (int dd = 0; dd < a.nDir; ++dd)
            {
                const double* o = a.Isc + (((size_t)l * a.Nr + mu) * a.nDir + dd) * 2 * Ns;
                acc += 0.5 * wmu * o[k];
                if (a.hasJ20)
                    acc20 += (wJ20_I * wmu) * o[k] + (wJ20_Q * wmu) * o[Ns + k];
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
} // namespace

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
    // wavelength chunks: the rows of a chunk's rays stay within 256 MB
    const size_t perLa = (size_t)Nr * nDir * (ST_ROWS + (updateJ ? 2 : 0)) * Ns * sizeof(double);
    const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)Nla, ((size_t)256 << 20) / perLa));
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
