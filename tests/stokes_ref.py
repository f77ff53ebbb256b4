"""numpy restatement of formal_sol_full_stokes (Source/FormalStokes.cpp:166-723) for the tests: the chi[7] / eta[4]
gather of stokes_fs_core, the DELO-Bezier3 march of piecewise_stokes_bezier3_1d_impl (vectorised over rays) and the
scalar piecewise_bezier3_1d where a wavelength is not polarised.  Pinned to the reference by tests/test_stokes_ref.py
(falc_stokes_small.npz and every case of falc_stokes_matrix.npz); the GPU tests use it where the fixture cannot reach (the timed grid).  The profiles (phi and
phiQ..psiV of the problem's lines) are inputs.  Q, U, V are zero at unpolarised wavelengths, as on the device."""
import numpy as np

from lightweaver_amd import _abi as abi

HC_K = 6.6260755E-34 * 2.99792458E+08 / (1.380658E-23 * 1.0E-09)
TWO_HC = 2.0 * 6.6260755E-34 * 2.99792458E+08 / (1.0E-09) ** 3
HC_4PI = 0.25 * 6.6260755E-34 * 2.99792458E+08 / np.pi
INV2ROOT2 = 1.0 / (2.0 * np.sqrt(2.0))


def _planck(T, lam):
    x = HC_K / lam / T
    with np.errstate(over='ignore'):
        return np.where(x <= 150.0, (TWO_HC / lam ** 3) / (np.exp(np.minimum(x, 150.0)) - 1.0), 0.0)


def _cent_deriv(dsuw, dsdw, yuw, y0, ydw):
    S0 = (ydw - y0) / dsdw
    Suw = (y0 - yuw) / dsuw
    P0 = np.abs((Suw * dsdw + S0 * dsuw) / (dsdw + dsuw))
    return (np.copysign(1.0, S0) + np.copysign(1.0, Suw)) * np.minimum(np.abs(Suw), np.minimum(np.abs(S0), 0.5 * P0))


def _bezier3_coeffs(dt):
    dt2, dt3 = dt * dt, dt * dt * dt
    with np.errstate(over='ignore', invalid='ignore'):
        edt = np.exp(-dt)
        a = np.where(dt < 5e-2, 0.25 * dt - 0.2 * dt2 + dt3 / 12.0,
                     np.where(dt > 30.0, 6.0 / dt3, (6.0 - edt * (6.0 + 6.0 * dt + 3 * dt2 + dt3)) / dt3))
        b = np.where(dt < 5e-2, 0.25 * dt - 0.05 * dt2 + dt3 / 120.0,
                     np.where(dt > 30.0, (-6.0 + 6.0 * dt - 3.0 * dt2 + dt3) / dt3,
                              (6.0 * edt - 6.0 + 6.0 * dt - 3.0 * dt2 + dt3) / dt3))
        g = np.where(dt < 5e-2, 0.25 * dt - 0.15 * dt2 + 0.05 * dt3,
                     np.where(dt > 30.0, 3.0 * (2.0 * dt - 6.0) / dt3,
                              3.0 * (2.0 * dt - 6.0 + edt * (6.0 + 4.0 * dt + dt2)) / dt3))
        d = np.where(dt < 5e-2, 0.25 * dt - 0.1 * dt2 + 0.025 * dt3,
                     np.where(dt > 30.0, 3.0 * (6.0 - 4.0 * dt + dt2) / dt3,
                              3.0 * (6.0 - 4.0 * dt + dt2 - 2.0 * edt * (3.0 + dt)) / dt3))
        e = np.where(dt < 5e-2, 1.0 - dt + 0.5 * dt2 - dt3 / 6.0, np.where(dt > 30.0, 0.0, edt))
    return a, b, g, d, e


def _w2(dt):
    with np.errstate(over='ignore'):
        e = np.exp(-dt)
    w0 = np.where(dt < 5e-4, dt * (1.0 - 0.5 * dt), np.where(dt > 50.0, 1.0, 1.0 - e))
    w1 = np.where(dt < 5e-4, dt * dt * (0.5 - dt / 3.0), np.where(dt > 50.0, 1.0, (1.0 - e) - dt * e))
    return w0, w1


def _stokes_K(chi):
    """stokes_K (:119-142) for chi [R, 7, Ns] -> K [R, Ns, 4, 4]"""
    R, _, Ns = chi.shape
    K = np.zeros((R, Ns, 4, 4))
    ci = chi[:, 0]
    K[..., 0, 1] = K[..., 1, 0] = chi[:, 1] / ci
    K[..., 0, 2] = K[..., 2, 0] = chi[:, 2] / ci
    K[..., 0, 3] = K[..., 3, 0] = chi[:, 3] / ci
    K[..., 1, 2] = chi[:, 6] / ci
    K[..., 2, 1] = -chi[:, 6] / ci
    K[..., 1, 3] = -chi[:, 5] / ci
    K[..., 3, 1] = chi[:, 5] / ci
    K[..., 2, 3] = chi[:, 4] / ci
    K[..., 3, 2] = -chi[:, 4] / ci
    return K


def gather(prob, la, mu, d, updateJ, J20=None):
    """chi [7, Ns], S [4, Ns] and the polarised flag of ray (la, mu, d) (stokes_fs_core :496-602)."""
    Ns = prob.Nspace
    chi = np.zeros((7, Ns))
    eta = np.zeros((4, Ns))
    pol = {(L.atom, L.trans): L for L in prob.stokes.lines}
    polF = J20 is not None
    for ia, a in enumerate(prob.atoms):
        for kr, t in enumerate(a.trans):
            if not (t.Nblue <= la < t.Nred):
                continue
            lt = la - t.Nblue
            if t.type == abi.LINE:
                ph = t.phi[lt, mu, d]
                Vij = (HC_4PI * (t.lambda0 / t.wavelength[lt]) * t.Bij) * ph
                g = t.Bji / t.Bij
                if t.rhoPrd is not None:
                    g = g * t.rhoPrd[lt]
                Vji = g * Vij
                Uji = (t.Aji / t.Bji) * Vji
            else:
                g = a.nStar[t.i] / a.nStar[t.j] * np.exp(-(HC_K / t.wavelength[lt]) / prob.temperature)
                Vij = t.alpha[lt]
                Vji = g * Vij
                Uji = (TWO_HC / t.wavelength[lt] ** 3) * Vji
            c = a.n[t.i] * Vij - a.n[t.j] * Vji
            e = a.n[t.j] * Uji
            chi[0] += c
            eta[0] += e
            L = pol.get((ia, kr))
            if L is not None:
                polF = True
                cnp, enp = c / ph, e / ph
                for m, name in enumerate(('phiQ', 'phiU', 'phiV', 'psiQ', 'psiU', 'psiV')):
                    chi[1 + m] += cnp * getattr(L, name)[lt, mu, d]
                for m, name in enumerate(('phiQ', 'phiU', 'phiV')):
                    eta[1 + m] += enp * getattr(L, name)[lt, mu, d]
    sca = prob.bgSca[la]
    if J20 is not None:
        mu2 = prob.muz[mu] ** 2
        j20 = J20[la] if updateJ else 0.0
        eta[0] += INV2ROOT2 * (3.0 * mu2 - 1.0) * sca * j20
        eta[1] += INV2ROOT2 * 3.0 * (mu2 - 1.0) * sca * j20
    jdag = prob.J[la] if updateJ else 0.0
    chi[0] += prob.bgChi[la]
    S = np.zeros((4, Ns))
    S[0] = (eta[0] + prob.bgEta[la] + sca * jdag) / chi[0]
    S[1:] = eta[1:] / chi[0]
    return chi, S, polF


def _iupw(prob, chi0, la, mu, d, zmu):
    """the boundary intensity (:365-410), for rays of one direction: chi0 [R, Ns]"""
    Ns, h, T = prob.Nspace, prob.height, prob.temperature
    k0, k1 = (Ns - 1, Ns - 2) if d else (0, 1)
    dtau = 0.5 * zmu * (chi0[:, k0] + chi0[:, k1]) * abs(h[k0] - h[k1])
    bc = prob.zLowerBc if d else prob.zUpperBc
    wav = prob.wavelength[la]
    if bc.type == abi.BC_THERMALISED:
        Bk0, Bk1 = _planck(T[k0], wav), _planck(T[k1], wav)
        return Bk0 - (Bk1 - Bk0) / dtau
    if bc.type == abi.BC_CALLABLE:
        m = bc.idxs[mu, d]
        return np.where(m >= 0, bc.bcData[la, np.maximum(m, 0)], 0.0)
    return np.zeros(chi0.shape[0])


def march(prob, chi, S, zmu, d, Iupw, polarised):
    """I [R, 4, Ns] of rays of one direction d: the Stokes march where `polarised`, else the scalar Bezier3."""
    R, _, Ns = chi.shape
    h = prob.height
    I = np.zeros((R, 4, Ns))
    dk, ks, ke = (-1, Ns - 1, 0) if d else (1, 0, Ns - 1)
    c0 = chi[:, 0]
    I[:, 0, ks] = Iupw
    # ---- scalar piecewise_bezier3_1d (FormalScalar.cpp:209-325) on all rays; the polarised ones are redone below
    S0 = S[:, 0]
    k = ks + dk
    ds_uw = abs(h[k] - h[k - dk]) * zmu
    ds_dw = abs(h[k + dk] - h[k]) * zmu
    dx_uw = (c0[:, k] - c0[:, k - dk]) / ds_uw
    dx_c = _cent_deriv(ds_uw, ds_dw, c0[:, k - dk], c0[:, k], c0[:, k + dk])
    Cuw = c0[:, k - dk] + (ds_uw / 3.0) * dx_uw
    C0 = c0[:, k] - (ds_uw / 3.0) * dx_c
    dtau_uw = ds_uw * (c0[:, k] + c0[:, k - dk] + Cuw + C0) * 0.25
    dS_uw = (S0[:, k] - S0[:, k - dk]) / dtau_uw
    I_upw = Iupw.copy()
    while k != ke - dk:
        ds_dw2 = abs(h[k + 2 * dk] - h[k + dk]) * zmu
        dx_dw = _cent_deriv(ds_dw, ds_dw2, c0[:, k], c0[:, k + dk], c0[:, k + 2 * dk])
        Cuw = c0[:, k] + (ds_dw / 3.0) * dx_c
        C0 = c0[:, k + dk] - (ds_dw / 3.0) * dx_dw
        dtau_dw = ds_dw * (c0[:, k] + c0[:, k + dk] + Cuw + C0) * 0.25
        al, be, ga, de, ed = _bezier3_coeffs(dtau_uw)
        dS_c = _cent_deriv(dtau_uw, dtau_dw, S0[:, k - dk], S0[:, k], S0[:, k + dk])
        Cuw = S0[:, k - dk] + (dtau_uw / 3.0) * dS_uw
        C0 = S0[:, k] - (dtau_uw / 3.0) * dS_c
        I[:, 0, k] = I_upw * ed + al * S0[:, k - dk] + be * S0[:, k] + ga * Cuw + de * C0
        I_upw = I[:, 0, k]
        ds_uw, ds_dw, dx_uw, dx_c, dtau_uw, dS_uw = ds_dw, ds_dw2, dx_c, dx_dw, dtau_dw, dS_c
        k += dk
    k = ke - dk
    ds_dw = abs(h[k + dk] - h[k]) * zmu
    dx_dw = (c0[:, k + dk] - c0[:, k]) / ds_dw
    Cuw = c0[:, k] + (ds_dw / 3.0) * dx_c
    C0 = c0[:, k + dk] - (ds_dw / 3.0) * dx_dw
    dtau_dw = ds_dw * (c0[:, k] + c0[:, k + dk] + Cuw + C0) * 0.25
    al, be, ga, de, ed = _bezier3_coeffs(dtau_uw)
    dS_c = _cent_deriv(dtau_uw, dtau_dw, S0[:, k - dk], S0[:, k], S0[:, k + dk])
    Cuw = S0[:, k - dk] + dtau_uw / 3.0 * dS_uw
    C0 = S0[:, k] - dtau_uw / 3.0 * dS_c
    I[:, 0, k] = I_upw * ed + al * S0[:, k - dk] + be * S0[:, k] + ga * Cuw + de * C0
    I_upw = I[:, 0, k]
    k = ke
    dtau_uw = 0.5 * zmu * (c0[:, k] + c0[:, k - dk]) * abs(h[k] - h[k - dk])
    dS_uw = (S0[:, k] - S0[:, k - dk]) / dtau_uw
    w0, w1 = _w2(dtau_uw)
    I[:, 0, k] = (1.0 - w0) * I_upw + w0 * S0[:, k] - w1 * dS_uw
    p = np.flatnonzero(polarised)
    if p.size:
        I[p] = _stokes_march(prob, chi[p], S[p], zmu[p], d, Iupw[p])
    return I


def _stokes_march(prob, chi, S, zmu, d, Iupw):
    """piecewise_stokes_bezier3_1d_impl (:166-340)"""
    R, _, Ns = chi.shape
    h = prob.height
    K = _stokes_K(chi)                      # [R, Ns, 4, 4]
    I = np.zeros((R, 4, Ns))
    dk, ks, ke = (-1, Ns - 1, 0) if d else (1, 0, Ns - 1)
    c0 = chi[:, 0]
    I[:, 0, ks] = Iupw
    k = ks + dk
    ds_uw = abs(h[k] - h[k - dk]) * zmu
    ds_dw = abs(h[k + dk] - h[k]) * zmu
    dx_uw = (c0[:, k] - c0[:, k - dk]) / ds_uw
    dx_c = _cent_deriv(ds_uw, ds_dw, c0[:, k - dk], c0[:, k], c0[:, k + dk])
    c1 = c0[:, k] - (ds_uw / 3.0) * dx_c
    c2 = c0[:, k - dk] + (ds_uw / 3.0) * dx_uw
    dtau_uw = ds_uw * (c0[:, k] + c0[:, k - dk] + c1 + c2) * 0.25
    Ku, K0 = K[:, ks], K[:, k]
    Su, S0 = S[:, :, ks], S[:, :, k]
    dSu = (S0 - Su) / dtau_uw[:, None]
    dKu = (K0 - Ku) / dtau_uw[:, None, None]
    ds_dw2 = np.zeros(R)
    dtau_dw = np.zeros(R)
    Kd, Sd = np.zeros_like(K0), np.zeros_like(S0)
    eye = np.eye(4)[None]
    while k != ke + dk:
        if k == ke:
            dS0 = (S0 - Su) / dtau_uw[:, None]
            dK0 = (K0 - Ku) / dtau_uw[:, None, None]
        else:
            if ke - k == dk:
                dx_dw = (c0[:, k + dk] - c0[:, k]) / ds_dw
            else:
                ds_dw2 = abs(h[k + 2 * dk] - h[k + dk]) * zmu
                dx_dw = _cent_deriv(ds_dw, ds_dw2, c0[:, k], c0[:, k + dk], c0[:, k + 2 * dk])
            c1 = c0[:, k] + (ds_dw / 3.0) * dx_c
            c2 = c0[:, k + dk] - (ds_dw / 3.0) * dx_dw
            dtau_dw = ds_dw * (c0[:, k] + c0[:, k + dk] + c1 + c2) * 0.25
            Kd, Sd = K[:, k + dk], S[:, :, k + dk]
            dK0 = _cent_deriv(dtau_uw[:, None, None], dtau_dw[:, None, None], Ku, K0, Kd)
            dS0 = _cent_deriv(dtau_uw[:, None], dtau_dw[:, None], Su, S0, Sd)
        Ku2, K02 = Ku @ Ku, K0 @ K0
        al, be, ga, de, ed = (x[:, None, None] for x in _bezier3_coeffs(dtau_uw))
        t3 = (dtau_uw / 3.0)[:, None, None]
        dd = t3 * (Ku2 + Ku - dKu) - Ku
        e = t3 * (K02 + K0 - dK0) + K0
        Md = eye + be * K0 + de * e
        Ma = ed * eye - al * Ku + ga * dd
        Mb = al * eye + ga * (eye - t3 * Ku)
        Mc = be * eye + de * (eye + t3 * K0)
        V0 = (np.einsum('rij,rj->ri', Ma, I[:, :, k - dk]) + np.einsum('rij,rj->ri', Mb, Su)
              + np.einsum('rij,rj->ri', Mc, S0))
        V0 += t3[:, :, 0] * (ga[:, :, 0] * dSu - de[:, :, 0] * dS0)
        x = np.linalg.solve(Md, V0[..., None])[..., 0]
        x += np.linalg.solve(Md, (V0 - np.einsum('rij,rj->ri', Md, x))[..., None])[..., 0]
        I[:, :, k] = x
        Su, S0, dSu = S0, Sd, dS0
        Ku, K0, dKu = K0, Kd, dK0
        dtau_uw, ds_uw, ds_dw, dx_uw, dx_c = dtau_dw, ds_dw, ds_dw2, dx_c, dx_dw
        k += dk
    return I


def full_stokes(prob, updateJ=False, upOnly=True, J20=None, las=None):
    """I [Nla, Nrays], Quv [3, Nla, Nrays] at the wavelengths `las` (default all); with updateJ also J [Nla, Ns], J20,
    dJ [Nla] (rows of the wavelengths computed)."""
    las = np.arange(prob.Nlambda) if las is None else np.asarray(las)
    Nr, Ns = prob.Nrays, prob.Nspace
    I = np.zeros((len(las), Nr))
    Quv = np.zeros((3, len(las), Nr))
    J = np.zeros((len(las), Ns))
    J20o = np.zeros((len(las), Ns))
    dJ = np.zeros(len(las))
    dirs = (1,) if upOnly else (0, 1)
    for i, la in enumerate(las):
        acc = np.zeros(Ns)
        acc20 = np.zeros(Ns)
        rays = {}
        for d in dirs:
            g = [gather(prob, la, mu, d, updateJ, J20) for mu in range(Nr)]
            chi = np.stack([x[0] for x in g])
            S = np.stack([x[1] for x in g])
            pol = np.array([x[2] for x in g])
            zmu = 1.0 / prob.muz
            Iu = _iupw(prob, chi[:, 0], la, np.arange(Nr), d, zmu)
            rays[d] = (march(prob, chi, S, zmu, d, Iu, pol), pol)
        for mu in range(Nr):
            wmu = prob.wmu[mu]
            mu2 = prob.muz[mu] ** 2
            for d in dirs:
                Ir = rays[d][0][mu]
                acc += 0.5 * wmu * Ir[0]
                acc20 += (INV2ROOT2 * (3.0 * mu2 - 1.0) * wmu) * Ir[0] + (INV2ROOT2 * 3.0 * (mu2 - 1.0) * wmu) * Ir[1]
        Iup, pol = rays[1]
        I[i] = Iup[:, 0, 0]
        Quv[:, i] = np.where(pol[None], Iup[:, 1:, 0].T, 0.0)
        if updateJ:
            J[i] = acc
            J20o[i] = acc20
            dJ[i] = np.abs(1.0 - prob.J[la] / acc).max()
    return I, Quv, J, J20o, dJ


def ref_profiles(prob, L):
    """Transition::compute_polarised_profiles (Source/FormalStokes.cpp:9-117) in numpy with scipy's w(z)."""
    from scipy.special import wofz
    a = prob.atoms[L.atom]
    t = a.trans[L.trans]
    st = prob.stokes
    larmor = 1.60217733E-19 / (4.0 * np.pi * 9.1093897E-31) * (t.lambda0 * 1e-9)
    vB = larmor * st.B / a.vBroad
    sv = 1.0 / (np.sqrt(np.pi) * a.vBroad)
    vBase = (t.wavelength - t.lambda0) * 2.99792458E+08 / t.lambda0
    out = {k: np.zeros(t.phi.shape) for k in ('phi', 'phiQ', 'phiU', 'phiV', 'psiQ', 'psiU', 'psiV')}
    for d, s in ((0, -1.0), (1, 1.0)):
        v = (vBase[:, None, None] + s * prob.vlosMu[None]) / a.vBroad      # [l, mu, k]
        ph = {al: 0.0 for al in (-1, 0, 1)}
        ps = {al: 0.0 for al in (-1, 0, 1)}
        for al, sh, strn in zip(L.alpha, L.shift, L.strength):
            w = wofz(v - sh * vB + 1j * t.aDamp)
            ph[int(al)] = ph[int(al)] + strn * w.real
            ps[int(al)] = ps[int(al)] + strn * w.imag
        cg, c2, s2 = st.cosGamma[None], st.cos2chi[None], st.sin2chi[None]
        sin2g = 1.0 - cg ** 2
        phs, pss = ph[1] + ph[-1], ps[1] + ps[-1]
        phd, psd = 0.5 * ph[0] - 0.25 * phs, 0.5 * ps[0] - 0.25 * pss
        out['phi'][:, :, d] = (phd * sin2g + 0.5 * phs) * sv
        out['phiQ'][:, :, d] = s * phd * sin2g * c2 * sv
        out['phiU'][:, :, d] = phd * sin2g * s2 * sv
        out['phiV'][:, :, d] = s * 0.5 * (ph[1] - ph[-1]) * cg * sv
        out['psiQ'][:, :, d] = s * psd * sin2g * c2 * sv
        out['psiU'][:, :, d] = psd * sin2g * s2 * sv
        out['psiV'][:, :, d] = s * 0.5 * (ps[1] - ps[-1]) * cg * sv
    wl = t.wlambda()[:, None, None, None] * 0.5 * prob.wmu[None, :, None, None]
    out['wphi'] = 1.0 / (wl * out['phi']).sum(axis=(0, 1, 2))
    return out


def set_polarised_profiles(prob):
    """phi, wphi and phiQ..psiV of every polarised line of prob from ref_profiles."""
    for L in prob.stokes.lines:
        t = prob.atoms[L.atom].trans[L.trans]
        ref = ref_profiles(prob, L)
        t.phi[...] = ref['phi']
        t.wphi[...] = ref['wphi']
        for name in ('phiQ', 'phiU', 'phiV', 'psiQ', 'psiU', 'psiV'):
            getattr(L, name)[...] = ref[name]
