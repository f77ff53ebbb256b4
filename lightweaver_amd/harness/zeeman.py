"""Zeeman components of a line (restated from the reference's lightweaver/zeeman.py:31-157): the three-component
splitting of an effective Lande factor, or the anomalous splitting of LS coupling, and the term symbols of the Ca II
model of harness/models.py (CaII_6) so that H, K and the infrared triplet can be polarised."""
from fractions import Fraction
from typing import Optional, Tuple

import numpy as np

from ..model import StokesLine

# (J, L, S) of the CaII_6 levels: 4s 2S1/2, 3d 2D3/2, 3d 2D5/2, 4p 2P1/2, 4p 2P3/2 (level 5 is Ca III)
CAII_TERMS = [(Fraction(1, 2), 0, Fraction(1, 2)), (Fraction(3, 2), 2, Fraction(1, 2)), (Fraction(5, 2), 2, Fraction(1, 2)),
              (Fraction(1, 2), 1, Fraction(1, 2)), (Fraction(3, 2), 1, Fraction(1, 2)), None]


def fraction_range(start: Fraction, stop: Fraction, step: Fraction = Fraction(1, 1)):
    while start < stop:
        yield start
        start += step


def zeeman_strength(Ju: Fraction, Mu: Fraction, Jl: Fraction, Ml: Fraction) -> float:
    """Strength of one component (del Toro Iniesta p. 137, x2; normalised by the caller)."""
    alpha = int(Ml - Mu)
    dJ = int(Ju - Jl)
    if dJ == 0:
        s = {0: 2.0 * Mu**2, -1: (Ju + Mu) * (Ju - Mu + 1.0), 1: (Ju - Mu) * (Ju + Mu + 1.0)}[alpha]
    elif dJ == 1:
        s = {0: 2.0 * ((Jl + 1)**2 - Ml**2), -1: (Jl + Ml + 1) * (Jl + Ml + 2.0),
             1: (Jl - Ml + 1.0) * (Jl - Ml + 2.0)}[alpha]
    elif dJ == -1:
        s = {0: 2.0 * ((Ju + 1)**2 - Mu**2), -1: (Ju - Mu + 1) * (Ju - Mu + 2.0),
             1: (Ju + Mu + 1.0) * (Ju + Mu + 2.0)}[alpha]
    else:
        raise ValueError('Invalid dJ: %d' % dJ)
    return float(s)


def lande_factor(J: Fraction, L: int, S: Fraction) -> float:
    if J == 0.0:
        return 0.0
    return float(1.5 + (S * (S + 1.0) - L * (L + 1)) / (2.0 * J * (J + 1.0)))


def components(lower: Optional[Tuple], upper: Optional[Tuple], gLandeEff: Optional[float] = None):
    """(alpha int32, strength, shift) of a line between levels with terms `lower` / `upper` = (J, L, S), or of its
    effective Lande factor when given; None when neither applies (compute_zeeman_components)."""
    if gLandeEff is not None:
        alpha = np.array([-1, 0, 1], dtype=np.int32)
        return alpha, np.ones(3), alpha * gLandeEff
    if lower is None or upper is None:
        return None
    (Jl, Ll, Sl), (Ju, Lu, Su) = lower, upper
    if Jl > Ll + Sl or Ju > Lu + Su:
        return None
    gLl = lande_factor(Jl, Ll, Sl)
    gLu = lande_factor(Ju, Lu, Su)
    alpha, strength, shift = [], [], []
    norm = np.zeros(3)
    for ml in fraction_range(-Jl, Jl + 1):
        for mu in fraction_range(-Ju, Ju + 1):
            if abs(ml - mu) <= 1.0:
                alpha.append(int(ml - mu))
                shift.append(gLl * ml - gLu * mu)
                strength.append(zeeman_strength(Ju, mu, Jl, ml))
                norm[alpha[-1] + 1] += strength[-1]
    alpha = np.array(alpha, dtype=np.int32)
    strength = np.array(strength) / norm[alpha + 1]
    return alpha, strength, np.array(shift, dtype=np.float64)


def polarise_lines(prob, atomIdx: int, terms=CAII_TERMS, lines=None):
    """StokesLine entries for the lines of prob.atoms[atomIdx] (all of them, or the transition indices `lines`) from the
    atom's term symbols."""
    out = []
    a = prob.atoms[atomIdx]
    for kr, t in enumerate(a.trans):
        if t.type != 0 or (lines is not None and kr not in lines):
            continue
        comp = components(terms[t.i], terms[t.j])
        if comp is None:
            continue
        alpha, strength, shift = comp
        out.append(StokesLine(atomIdx, kr, alpha, shift, strength))
    return out


def falc_h_ca_stokes(Nrays=3, lineScale=0.2, B=None, gammaB=None, chiB=None, discCentre=True, atmos=None, **kw):
    """FAL-C, H + Ca II (models.falc_h_ca) with a magnetic field and the Ca II lines H, K and the infrared triplet
    polarised: the B-field option of the problem builder.  B [T], gammaB, chiB default to depth-varying profiles;
    discCentre replaces the last ray's muz by exactly 1 (the branch of update_projections that tests the symmetries)."""
    from . import models
    atmos = atmos if atmos is not None else models.falc82()
    prob = models.build_problem(atmos, [models.H_6(lineScale), models.CaII_6(lineScale)], Nrays=Nrays,
                                computeProfiles=False, **kw)
    if discCentre:
        prob.muz[-1] = 1.0
    prob.vlosMu[...] = prob.muz[:, None] * atmos.vlos[None, :]
    models.compute_profiles_host(prob)
    z = np.linspace(0.0, 1.0, prob.Nspace)
    B = 0.1 * (0.5 + z) if B is None else B
    gammaB = 0.3 + 0.9 * z if gammaB is None else gammaB
    chiB = 0.2 + 1.1 * z if chiB is None else chiB
    mux = np.sqrt(1.0 - prob.muz ** 2)
    from ..model import StokesData
    prob.set_stokes(StokesData(B=B, gammaB=gammaB, chiB=chiB, mux=mux, muy=np.zeros(Nrays),
                               lines=polarise_lines(prob, 1)))
    prob.stokes.vz = np.ascontiguousarray(atmos.vlos, dtype=np.float64)
    return prob


def stokes_columns(ncol, Nrays=5, lineScale=3.1, seed0=1234, Nspace=None):
    """`ncol` columns of a 1.5D batch for polarised synthesis: seeded perturbed FAL-C (models.perturbed, seeds seed0,
    seed0 + 1, ...), H + Ca II with the Ca II lines polarised, each column with its own smooth seeded B, gammaB and chiB.
    The profiles are left to the device (computeProfiles=False).  Nspace: FAL-C resampled to that many depth points
    before it is perturbed (default: its own 82)."""
    from . import models
    from ..model import StokesData
    base = models.falc82()
    if Nspace is not None:
        base = models.resample(base, Nspace)
    ker = np.ones(9) / 9.0
    probs = []
    for c in range(ncol):
        seed = seed0 + c
        atmos = models.perturbed(base, seed=seed)
        prob = models.build_problem(atmos, [models.H_6(lineScale), models.CaII_6(lineScale)], Nrays=Nrays,
                                    computeProfiles=False)
        rng = np.random.default_rng([seed, 7])
        Ns = prob.Nspace
        z = np.linspace(0.0, 1.0, Ns)
        sm = lambda a: np.convolve(np.pad(a, 4, mode='edge'), ker, mode='valid')  # noqa: E731
        B = rng.uniform(0.02, 0.2) * (0.5 + z) * (1.0 + 0.2 * sm(rng.standard_normal(Ns)))
        gammaB = rng.uniform(0.1, 1.4) + rng.uniform(-0.6, 0.6) * z + 0.1 * sm(rng.standard_normal(Ns))
        chiB = rng.uniform(0.0, 2.0 * np.pi) + rng.uniform(-1.0, 1.0) * z + 0.1 * sm(rng.standard_normal(Ns))
        prob.set_stokes(StokesData(B=B, gammaB=gammaB, chiB=chiB, mux=np.sqrt(1.0 - prob.muz ** 2),
                                   muy=np.zeros(Nrays), lines=polarise_lines(prob, 1)))
        prob.stokes.vz = np.ascontiguousarray(atmos.vlos, dtype=np.float64)
        probs.append(prob)
    return probs
