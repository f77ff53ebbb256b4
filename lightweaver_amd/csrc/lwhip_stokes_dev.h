// lwhip_stokes_dev.h -- the device side of the full-Stokes formal solution that the single-context kernels (lwhip_stokes.hip)
// and the column-batch kernels (lwhip_stokes_batch.hip) share: the per-column argument block, the gather of one depth point,
// the upwind intensity, the DELO-Bezier3 and scalar Bezier3 marches of one ray, and the J / J20 / dJ sums of one wavelength.
//
// The marches are templated on how a ray's rows are read and its I / Q profile is written: a plain pointer (the
// single-context layout, row m at depth k is row[m * Ns + k]) or a LaneRow (the batch's layout, the same element 64
// doubles further per index, so that the 64 rays of a wavefront sit side by side).  Only the addressing differs; every
// operation, and its order, is the same in both, so a column of a batch gets the bits of its own context.
//
// Both units include this after `#pragma clang fp contract(off)` (repeated here): no fused multiply-adds, so that the
// operations match the reference's one for one.
#pragma once
#pragma clang fp contract(off)

#include "lwhip_host.h"
#include "lwhip_device.h"
#include "lwhip_lu.h"

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
    double* scratch; // [nla * Nr * nDir][ST_ROWS][Ns] (single context)
    double* Isc;     // [nla * Nr * nDir][2][Ns]: I and Q at every depth (updateJ; single context)
    double* I;       // [Nla, Nr]
    double* Quv;     // [3, Nla, Nr]
    double* dJ;      // [Nla]
    int32_t* singular; // set when a depth point's 4 x 4 system is singular (solve_lin_eq throws there, LuSolve.cpp:22-23)
};

// One element of a ray's rows in the batch layout: index i is 64 doubles (one per lane of the wavefront's rays) after i - 1
template <typename T> struct LaneRow
{
    T* p;
    DEVINL T& operator[](int i) const { return p[(size_t)i * 64]; }
    DEVINL LaneRow operator+(int i) const { return LaneRow{ p + (size_t)i * 64 }; }
    DEVINL explicit operator bool() const { return p != nullptr; }
};

DEVINL bool polarised_la(const StokesArgs& a, int la) { return a.laPol[la] != 0 || a.hasJ20; }

// chi[7] and eta[4] of (la, mu, d) at depth k summed over the transitions active at la (stokes_fs_core :496-602), stored as
// the ray's rows chi[0..6], S[0..3]: row[m * Ns] is row m at this depth
template <typename W> DEVINL void stokes_gather_point(const StokesArgs& a, int la, int mu, int d, int k, W row)
{
    const int Ns = a.Ns;
    const double inv2root2 = 1.0 / (2.0 * sqrt(2.0));
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
template <typename R> DEVINL double upwind_intensity(const StokesArgs& a, R chi0, int la, int mu, int d, double zmu)
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
template <typename R> DEVINL void stokes_k6(R row, int Ns, int k, double (&u)[6])
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
template <typename R, typename O>
DEVINL double scalar_bezier3(const StokesArgs& a, R chi, R S, double zmu, int d, double Iupw, O out)
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
template <typename R, typename O>
DEVINL void stokes_bezier3(const StokesArgs& a, R row, double zmu, int d, double Iupw, O out0, O out1, double (&Iend)[4])
{
    const int Ns = a.Ns;
    const double* h = a.height;
    const R chi = row;
    const R Srow = row + 7 * Ns;
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
template <typename R, typename O>
DEVINL void stokes_march_ray(const StokesArgs& a, R row, O out0, O out1, int la, int mu, int d, int nDir)
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
} // namespace
} // namespace lwhip
