"""CPU checks of the full-Stokes helpers against the reference (falc_stokes_small.npz, make_stokes_golden.py): the Zeeman
components and projections exactly, and the numpy march of tests/stokes_ref.py to 1e-10; then the numpy march and the
numpy profiles on every case of the parity matrix (falc_stokes_matrix.npz, tests/stokes_cases.py) to 1e-9 and 1e-12."""
import numpy as np
import pytest

from lightweaver_amd.model import update_projections
from lightweaver_amd.harness import zeeman
from tests import stokes_cases as sc
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


# ---- the parity matrix -------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def matrix():
    return sc.load_fixture()


_built = {}


def _case_with_numpy_profiles(d, case):
    if case not in _built:
        prob = sc.fixture_problem(d, case)
        stokes_ref.set_polarised_profiles(prob)
        _built[case] = prob
    return _built[case].copy()


def test_cases_cover_the_matrix(matrix):
    assert len(sc.case_variants()) == 34
    keys = {k for k in matrix.files if k.startswith('out/') and k.endswith('/I')}
    assert keys == {f'out/{c}/{v}/I' for c, v in sc.case_variants()}
    for case, (Ns, Nrays, disc, _) in sc.CASES.items():
        prob = sc.fixture_problem(matrix, case)    # (the stored inputs are reproduced exactly: asserted there)
        assert (prob.Nspace, prob.Nrays, prob.Nlambda) == (Ns, Nrays, 208), case
        assert (prob.muz[-1] == 1.0) == disc, case
        assert np.abs(prob.vlosMu).max() > 1.0e3, case


@pytest.mark.parametrize('case,variant', sc.case_variants())
def test_numpy_march_matches_reference_matrix(matrix, case, variant):
    """Worst figures measured: I 2.1e-10 (n5, j), Quv / I 6.4e-12 (strongB), J 3.2e-10 (bc_lower_callable)."""
    updateJ, upOnly = sc.VARIANTS[variant]
    prob = _case_with_numpy_profiles(matrix, case)
    J20 = None if prob.stokes.J20 is None else prob.stokes.J20.copy()
    # (n130: the march over all 208 wavelengths of 130 depth points takes 14 s: a seeded sample with every line's ends)
    las = sc.sampled_wavelengths(prob) if case == 'n130' else None
    I, Quv, J, J20o, dJ = stokes_ref.full_stokes(prob, updateJ=updateJ, upOnly=upOnly, J20=J20, las=las)
    pol = sc.polarised_mask(prob, j20=J20 is not None)
    err = sc.errors_against(matrix, case, variant, I, Quv, J=J if updateJ else None,
                            dJMax=dJ.max() if updateJ and las is None else None,
                            J20=J20o if updateJ and J20 is not None else None, las=las, pol=pol)
    print(case, variant, err)
    assert set(err) >= ({'I', 'Quv', 'J'} if updateJ else {'I', 'Quv'})
    assert all(v <= 1e-9 for v in err.values()), err
    assert np.abs(Quv[:, pol[las] if las is not None else pol]).max() > 0.0 or case == 'B0'


@pytest.mark.parametrize('case', sc.PROFILE_CASES)
def test_numpy_profiles_match_reference_with_velocities(matrix, case):
    """stokes_ref.ref_profiles against the core's on a moving atmosphere (< 1e-16 measured)."""
    prob = sc.fixture_problem(matrix, case)
    ks = slice(None, None, sc.DEPTH_STRIDE)
    for i, L in enumerate(prob.stokes.lines):
        ref = stokes_ref.ref_profiles(prob, L)
        err = sc.profile_errors(matrix, case, i, {k: v[..., ks] if k != 'wphi' else v for k, v in ref.items()})
        print(case, i, err)
        assert all(v <= 1e-12 for v in err.values()), err
        # the two directions differ: otherwise the sign of the velocity term is invisible
        assert not np.array_equal(ref['phi'][:, :, 0], ref['phi'][:, :, 1])
