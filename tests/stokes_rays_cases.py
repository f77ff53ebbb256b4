"""Full-Stokes observer rays: the directions, the cases and the observer problems that
tests/golden/make_stokes_rays_golden.py runs through the reference (falc_stokes_rays.npz) and that
tests/test_stokes_rays.py rebuilds.  The base problems are those of tests/stokes_cases.py; everything is deterministic."""
import os

import numpy as np

from lightweaver_amd import _abi as abi
from lightweaver_amd.model import observer_problem

from tests import stokes_cases as sc

MUS = np.array([1.0, 0.6, 0.2])          # none of them a quadrature node of any case (asserted by the tests)
FIXTURE_CASES = ('moving82', 'n3', 'n5', 'bc_lower_callable', 'prd', 'gamma_edges')
# the extra entry: moving82 seen at mu = 0.6 with the azimuth turned by 90 degrees
AZ_KEY, AZ_CASE, AZ_MUS, AZ_MUX, AZ_MUY = 'moving82_az', 'moving82', np.array([0.6]), np.array([0.0]), np.array([0.8])


def entries():
    """(key in the fixture, case of stokes_cases, mus, mux, muy)"""
    return [(c, c, MUS, None, None) for c in FIXTURE_CASES] + [(AZ_KEY, AZ_CASE, AZ_MUS, AZ_MUX, AZ_MUY)]


def lower_bc(prob, Nmu):
    """The intensity entering at the bottom along Nmu new directions [Nlambda, Nmu] of a CALLABLE lower boundary (seeded),
    None for any other boundary."""
    if prob.zLowerBc.type != abi.BC_CALLABLE:
        return None
    rng = np.random.default_rng(13)
    return (1.0 + 0.3 * rng.random((prob.Nlambda, Nmu))) * prob.J[:, -1, None]


def observer(prob, mus=MUS, mux=None, muy=None, vz=None):
    """observer_problem(stokes=True) of a stokes_cases problem: v_z is the atmosphere's own (prob.stokes.vz)."""
    mus = np.atleast_1d(mus)
    return observer_problem(prob, mus, vz=prob.stokes.vz if vz is None else vz, lowerBc=lower_bc(prob, mus.shape[0]),
                            stokes=True, mux=mux, muy=muy)


def load_fixture():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'falc_stokes_rays.npz'))


def errors(I, Quv, Iref, Quvref, pol):
    """The largest relative differences of (I [Nla, Nmu], Quv [3, Nla, Nmu]) from a reference: I, and Quv / I at the
    polarised wavelengths `pol` (the scales of stokes_cases.errors_against)."""
    return {'I': float(np.max(np.abs(I / Iref - 1.0))),
            'Quv': float(np.max((np.abs(Quv - Quvref) / Iref[None])[:, pol]))}
