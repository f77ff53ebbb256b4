"""The full-Stokes parity matrix: the problems that tests/golden/make_stokes_golden.py runs through the reference
(falc_stokes_matrix.npz) and that tests/test_stokes_ref.py and tests/test_stokes.py rebuild.  Everything is deterministic.

Base problem: FAL-C (resampled to Ns points unless Ns = 82) with a seeded velocity field (models.perturbed, seed 5,
dv = 6 km/s), H_6 + CaII_6 at lineScale 0.2 (Nlambda = 208), vlosMu = muz (x) vlos, the field of
harness.zeeman.falc_h_ca_stokes, the Ca II lines polarised.  With `disc` the last ray's muz is exactly 1."""
import os

import numpy as np

from lightweaver_amd import _abi as abi
from lightweaver_amd.harness import models, zeeman
from lightweaver_amd.model import Boundary, StokesData

# name -> (Ns, Nrays, disc, what differs)
CASES = {
    'moving82': (82, 3, True, {}),
    'n3': (3, 3, True, {}),
    'n4': (4, 1, True, {}),
    'n5': (5, 2, False, {}),
    'n130': (130, 4, False, {}),
    'bc_lower_callable': (37, 3, True, dict(bc='lower')),
    'bc_upper_callable': (37, 3, True, dict(bc='upper')),
    'prd': (37, 3, True, dict(prd=True)),
    'strongB': (37, 3, True, dict(Bscale=3.0)),
    'B0': (37, 3, True, dict(Bscale=0.0)),
    'gamma_edges': (37, 3, True, dict(gammaEdges=True)),
    'fastv': (37, 3, True, dict(dv=3.0e4)),
    'nr1': (24, 1, True, {}),
    'nr7': (24, 7, False, {}),
    'j20': (37, 3, True, dict(j20=True)),
}

# variant -> (updateJ, upOnly)
VARIANTS = {'up': (False, True), 'j': (True, False), 'all': (False, False), 'jup': (True, True)}
FOUR_VARIANT_CASES = ('moving82', 'bc_lower_callable')
PROFILE_CASES = ('moving82', 'fastv')
PROFILE_NAMES = ('phiQ', 'phiU', 'phiV', 'psiQ', 'psiU', 'psiV')
DEPTH_STRIDE = 8
MATRIX_ROW = 100   # the wavelength row of bcData / J20 that the fixture keeps for the rebuild check


def variants(name):
    return ('up', 'j', 'all', 'jup') if name in FOUR_VARIANT_CASES else ('up', 'j')


def case_variants():
    return [(c, v) for c in CASES for v in variants(c)]


def j_depths(Ns):
    """The depths at which the fixture holds J and J20: all of a short column, else every DEPTH_STRIDE-th and the last."""
    if Ns <= DEPTH_STRIDE:
        return np.arange(Ns)
    return np.unique(np.concatenate([np.arange(0, Ns, DEPTH_STRIDE), [Ns - 1]]))


def build(name):
    """The Problem of case `name`, with the harness's own Zeeman components; for `j20` prob.stokes.J20 holds J20 dagger
    (pass a copy of it to single_stokes_fs / full_stokes as the J20 argument)."""
    Ns, Nrays, disc, o = CASES[name]
    base = models.falc82()
    atmos = base if Ns == base.Nspace else models.resample(base, Ns)
    atmos = models.perturbed(atmos, seed=5, dv=o.get('dv', 6.0e3))
    prob = models.build_problem(atmos, [models.H_6(0.2), models.CaII_6(0.2, prd=o.get('prd', False))], Nrays=Nrays,
                                computeProfiles=False)
    if disc:
        prob.muz[-1] = 1.0
    prob.vlosMu[...] = prob.muz[:, None] * atmos.vlos[None, :]
    models.compute_profiles_host(prob)
    z = np.linspace(0.0, 1.0, Ns)
    B = 0.1 * (0.5 + z) * o.get('Bscale', 1.0)
    gammaB = 0.3 + 0.9 * z
    if o.get('gammaEdges'):
        gammaB = np.where(z < 0.3, 0.0, np.where(z < 0.6, np.pi / 2, np.pi))
    chiB = 0.2 + 1.1 * z
    prob.set_stokes(StokesData(B=B, gammaB=gammaB, chiB=chiB, mux=np.sqrt(1.0 - prob.muz ** 2), muy=np.zeros(Nrays),
                               lines=zeeman.polarise_lines(prob, 1)))
    prob.stokes.vz = np.ascontiguousarray(atmos.vlos, dtype=np.float64)
    if o.get('bc') == 'lower':
        rng = np.random.default_rng(7)
        idxs = np.full((Nrays, 2), -1, dtype=np.int32)
        idxs[:, 1] = np.arange(Nrays)[::-1]
        bc = (1.0 + 0.3 * rng.random((prob.Nlambda, Nrays))) * prob.J[:, -1, None]
        prob.zLowerBc = Boundary(abi.BC_CALLABLE, idxs=idxs, bcData=bc)
        prob.zUpperBc = Boundary(abi.BC_THERMALISED)
    elif o.get('bc') == 'upper':
        rng = np.random.default_rng(7)
        idxs = np.full((Nrays, 2), -1, dtype=np.int32)
        idxs[:, 0] = np.arange(Nrays)
        bc = 0.2 * rng.random((prob.Nlambda, Nrays)) * prob.J[:, 0, None]
        prob.zUpperBc = Boundary(abi.BC_CALLABLE, idxs=idxs, bcData=bc)
        prob.zLowerBc = Boundary(abi.BC_ZERO)
    if o.get('prd'):
        for t in prob.atoms[1].trans:
            if t.rhoPrd is not None:
                t.rhoPrd = 1.0 + 0.3 * np.sin(np.arange(t.Nlambda))[:, None] * np.cos(3.0 * z)[None]
    if o.get('j20'):
        rng = np.random.default_rng(11)
        prob.stokes.J20 = 0.05 * prob.J * (rng.random(prob.J.shape) - 0.5)
    return prob


def polarised_mask(prob, j20=False):
    m = np.zeros(prob.Nlambda, dtype=bool)
    if j20:
        m[:] = True
    for L in prob.stokes.lines:
        t = prob.atoms[L.atom].trans[L.trans]
        m[t.Nblue:t.Nred] = True
    return m


def load_fixture():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'falc_stokes_matrix.npz'))


def fixture_problem(d, name):
    """build(name) with the reference's Zeeman components, checked against the inputs the fixture recorded."""
    prob = build(name)
    assert np.array_equal(prob.muz, d[f'in/{name}/muz']) and np.array_equal(prob.vlosMu, d[f'in/{name}/vlosMu']), name
    for bc in (prob.zLowerBc, prob.zUpperBc):
        if bc.type == abi.BC_CALLABLE:
            assert np.array_equal(bc.bcData[MATRIX_ROW], d[f'in/{name}/bcData']), name
    if prob.stokes.J20 is not None:
        assert np.array_equal(prob.stokes.J20[MATRIX_ROW], d[f'in/{name}/J20']), name
    for i, L in enumerate(prob.stokes.lines):
        L.alpha, L.strength, L.shift = d[f'in/alpha{i}'], d[f'in/strength{i}'], d[f'in/shift{i}']
    return prob


def sampled_wavelengths(prob, seed=5):
    """48 polarised + 16 unpolarised wavelengths, seeded, with the first and last wavelength of every polarised line."""
    pol = polarised_mask(prob)
    rng = np.random.default_rng(seed)
    ends = [w for L in prob.stokes.lines for t in [prob.atoms[L.atom].trans[L.trans]] for w in (t.Nblue, t.Nred - 1)]
    rest = np.setdiff1d(np.flatnonzero(pol), ends)
    return np.sort(np.concatenate([ends, rng.choice(rest, 48 - len(ends), replace=False),
                                   rng.choice(np.flatnonzero(~pol), 16, replace=False)]).astype(np.int64))


def errors_against(d, case, variant, I, Quv, J=None, dJMax=None, J20=None, las=None, pol=None):
    """The largest relative differences of a result from the fixture's: I, Quv / I at the polarised wavelengths `pol`, and
    with updateJ J, dJMax and J20 (against each wavelength's largest |J20|).  `las`: the wavelengths I, Quv, J, J20 hold."""
    key = f'out/{case}/{variant}'
    las = np.arange(d[f'{key}/I'].shape[0]) if las is None else las
    Iref = d[f'{key}/I'][las]
    err = {'I': np.max(np.abs(I / Iref - 1.0)),
           'Quv': np.max((np.abs(Quv - d[f'{key}/Quv'][:, las]) / Iref[None])[:, pol[las]])}
    if J is not None:
        kd = j_depths(J.shape[1])
        err['J'] = np.max(np.abs(J[:, kd] / d[f'{key}/J'][las] - 1.0))
        if dJMax is not None:
            err['dJMax'] = abs(dJMax / float(d[f'{key}/dJMax']) - 1.0)
        if J20 is not None:
            ref = d[f'{key}/J20'][las]
            err['J20'] = np.max(np.abs(J20[:, kd] - ref) / np.abs(ref).max(axis=1, keepdims=True))
    return {k: float(v) for k, v in err.items()}


def profile_errors(d, case, i, got):
    """phi, wphi and phiQ..psiV of polarised line i (`got`: name -> array at every DEPTH_STRIDE-th depth) against the
    fixture's, on the scales of test_parity_with_reference: phi for the absorption profiles, phi + |psiQ| + |psiU| + |psiV|
    for the dispersion profiles (psi falls off as 1 / v against phi's a / v^2)."""
    phi = d[f'prof/{case}/phi{i}']
    pscale = phi + sum(np.abs(d[f'prof/{case}/{n}{i}']) for n in ('psiQ', 'psiU', 'psiV'))
    err = {'phi': np.max(np.abs(got['phi'] - phi) / phi), 'wphi': np.max(np.abs(got['wphi'] / d[f'prof/{case}/wphi{i}'] - 1.0))}
    for name in PROFILE_NAMES:
        sc = phi if name.startswith('phi') else pscale
        err[name] = np.max(np.abs(got[name] - d[f'prof/{case}/{name}{i}']) / sc)
    return {k: float(v) for k, v in err.items()}
