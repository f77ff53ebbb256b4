"""CPU checks of the full-Stokes helpers against the reference (falc_stokes_small.npz, make_stokes_golden.py): the Zeeman
components and projections exactly, and the numpy march of tests/stokes_ref.py to 1e-10."""
import numpy as np

from lightweaver_amd.model import update_projections
from lightweaver_amd.harness import zeeman
from tests import stokes_ref
from tests.test_stokes import fixture_problem, load_stokes_fixture, _polarised_mask


def test_components_and_projections_match_reference():
    d = load_stokes_fixture()
    prob = zeeman.falc_h_ca_stokes()
    for i, L in enumerate(prob.stokes.lines):
        assert np.array_equal(L.alpha, d[f'in/alpha{i}'])
        assert np.array_equal(L.strength, d[f'in/strength{i}'])
        assert np.array_equal(L.shift, d[f'in/shift{i}'])
    cg, c2, s2 = update_projections(d['in/muz'], d['in/mux'], d['in/muy'], d['in/gammaB'], d['in/chiB'])
    # (exact on the disc-centre ray; elsewhere one element of the 246 differs by one unit in the last place)
    for got, key in ((cg, 'cosGamma'), (c2, 'cos2chi'), (s2, 'sin2chi')):
        assert np.array_equal(got[d['in/muz'] == 1.0], d[f'in/{key}'][d['in/muz'] == 1.0])
        assert np.max(np.abs(got - d[f'in/{key}'])) <= 2.3e-16


def test_numpy_march_matches_reference():
    d = load_stokes_fixture()
    for variant, kw in (('up', dict(updateJ=False, upOnly=True)), ('j', dict(updateJ=True, upOnly=False)),
                        ('j20', dict(updateJ=True, upOnly=False, J20=d['in/J20']))):
        prob = fixture_problem(d)
        stokes_ref.set_polarised_profiles(prob)
        I, Quv, J, J20, dJ = stokes_ref.full_stokes(prob, **kw)
        pol = _polarised_mask(prob) if variant != 'j20' else np.ones(prob.Nlambda, bool)
        Iref = d[f'out/{variant}/I']
        assert np.max(np.abs(I / Iref - 1.0)) <= 1e-10, variant
        assert np.max(np.abs(Quv - d[f'out/{variant}/Quv'])[:, pol] / Iref[pol][None]) <= 1e-10, variant
        if kw['updateJ']:
            assert np.max(np.abs(J / d[f'out/{variant}/J'] - 1.0)) <= 1e-10
            assert abs(dJ.max() / float(d[f'out/{variant}/dJMax']) - 1.0) <= 1e-10
        if variant == 'j20':
            ref = d['out/j20/J20']
            assert np.max(np.abs(J20 - ref) / np.abs(ref).max(axis=1, keepdims=True)) <= 1e-10
