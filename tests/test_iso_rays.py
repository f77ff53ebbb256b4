"""Angle-independent line profiles (a static atmosphere: no line-of-sight velocity, so the Voigt argument does not know the
ray): the lane sweep forms chi, S and the stencils of a one-line tile ONCE per wavefront and every ray of it scales / mirrors
them (TileDyn::phiIso; `LWHIP_ISO_RAYS=0` forms them once per angle as before, `LWHIP_PAIR_RAYS=0` is the general path).
The host finds the property where it finds the direction symmetry -- when the profiles are uploaded (the arrays are
compared) or generated (all velocities zero) -- and must drop it by itself.  Everything at the size of the pair test
(tests/test_timed_sizes.py): ~1 024 wavelengths, 3 mu, one iteration against the C oracle at the one-call bound 1e-9."""
import functools
import os

import numpy as np
import pytest

from helpers import rel_err
from lightweaver_amd import _abi as abi
from lightweaver_amd.harness import models
from oracle.bindings import OracleContext

pytestmark = pytest.mark.gpu
THREADS = min(os.cpu_count() or 1, 64)


def assert_iteration_matches(p, q, tolGamma=1e-9, tol=1e-9):
    worst = {'J': rel_err(p.J, q.J), 'I': rel_err(p.I, q.I)}
    for ia, (a, b) in enumerate(zip(p.atoms, q.atoms)):
        if not a.detailed:
            worst[f'Gamma{ia}'] = rel_err(a.Gamma, b.Gamma)
        worst[f'R{ia}'] = max(max(rel_err(ta.Rij, tb.Rij), rel_err(ta.Rji, tb.Rji)) for ta, tb in zip(a.trans, b.trans))
    assert all(v <= (tolGamma if k.startswith('Gamma') else tol) for k, v in worst.items()), worst
    return worst


def assert_same_bits(p, r, rates=True):
    assert np.array_equal(p.J, r.J) and np.array_equal(p.I, r.I)
    if rates:
        for a, b in zip(p.atoms, r.atoms):
            assert np.array_equal(a.Gamma, b.Gamma)
            for ta, tb in zip(a.trans, b.trans):
                assert np.array_equal(ta.Rij, tb.Rij) and np.array_equal(ta.Rji, tb.Rji)


def copy_profiles(dst, src):
    for a, b in zip(dst.atoms, src.atoms):
        for ta, tb in zip(a.trans, b.trans):
            if ta.type == abi.LINE:
                ta.phi[...] = tb.phi
                ta.wphi[...] = tb.wphi


@functools.lru_cache(maxsize=None)
def _base(Nrays=3, device=False, moving=False):
    """The problems are built once and only ever copied."""
    kw = dict(atmos=models.perturbed(models.falc82(), seed=5)) if moving else {}
    return models.throughput_grid(NlambdaTarget=1024, Nrays=Nrays, computeProfiles=not device, **kw)


def oracle_of(q):
    """One oracle iteration on q's own inputs (profiles included), in place."""
    oc = OracleContext(q)
    q.gamma_prefill()
    oc.formal_sol_gamma_matrices(Nthreads=THREADS)
    return q


def run(monkeypatch, prob, iso='1', pair='1', split='1', device=False, deterministic=False):
    """One iteration of a copy of `prob` under the given knobs (read once per context, when it is created)."""
    from lightweaver_amd.context import Context
    monkeypatch.setenv('LWHIP_LANE_SPLIT', split)
    monkeypatch.setenv('LWHIP_ISO_RAYS', iso)
    monkeypatch.setenv('LWHIP_PAIR_RAYS', pair)
    p = prob.copy()
    with Context(p, deterministic=deterministic) as ctx:
        assert ctx.sweep_kind() == 'lanes'
        if device:
            ctx.compute_profiles()       # (and brings them to the host: the oracle iterates on the same arrays)
        ctx.formal_sol_gamma_matrices()
    return p


@pytest.mark.parametrize('device', [True, False], ids=['device_profiles', 'host_profiles'])
def test_static_whole_rays_vs_oracle(gpu, monkeypatch, device):
    """Whole rays per wavefront, profiles generated on the device and uploaded from the host: with and without the
    wavefront-wide reuse against the oracle, the two bit-identical (the same operations on the same values: J and I in the
    default mode; Gamma and the rates, which the default mode sums with atomics in whatever order the workgroups arrive,
    in the fixed-order mode, where a run is reproducible to the bit -- tests/test_hip_parity.py), and the general path
    different in J's last bits only."""
    prob = _base(device=device)
    on, off = run(monkeypatch, prob, iso='1', device=device), run(monkeypatch, prob, iso='0', device=device)
    gen = run(monkeypatch, prob, pair='0', device=device)
    q = prob.copy()
    copy_profiles(q, on)
    oracle_of(q)
    print('iso on', assert_iteration_matches(on, q), 'iso off', assert_iteration_matches(off, q))
    assert_same_bits(on, off, rates=False)
    dOn, dOff = (run(monkeypatch, prob, iso=i, device=device, deterministic=True) for i in ('1', '0'))
    assert_same_bits(dOn, dOff)
    assert_iteration_matches(dOn, q)
    dJ = float(np.max(np.abs(on.J - gen.J) / gen.J))
    print('J: reuse against the general path', dJ)
    assert not np.array_equal(on.J, gen.J) and dJ < 1e-10


def test_library_finds_the_one_angle_that_differs(gpu, monkeypatch):
    """Host profiles of a static atmosphere in which one line's profile of ONE angle (both directions: the direction
    symmetry holds) is off by 1e-3 at one wavelength.  The library must find that out by itself from the uploaded arrays:
    used nevertheless, the first angle's stencils and profile would leave that line's rates four orders of magnitude
    beyond the bound."""
    prob = _base().copy()
    t = prob.atoms[1].trans[0]      # Ca II (H or K): narrow enough that its core wavelengths carry this line alone
    assert t.type == abi.LINE
    la = t.phi.shape[0] // 2
    t.phi[la, 1, :, :] *= 1.0 + 1e-3
    assert np.array_equal(t.phi[la, 1, 0], t.phi[la, 1, 1]) and not np.array_equal(t.phi[la, 1, 0], t.phi[la, 0, 0])
    q = oracle_of(prob.copy())
    on, off = run(monkeypatch, prob, iso='1'), run(monkeypatch, prob, iso='0')
    print(assert_iteration_matches(on, q))
    assert_iteration_matches(off, q)
    assert_same_bits(on, off, rates=False)
    dOn, dOff = (run(monkeypatch, prob, iso=i, deterministic=True) for i in ('1', '0'))
    assert_same_bits(dOn, dOff)
    # (the case has teeth: the oracle on the unscaled profiles is 3e-5 away in that line's rates)
    r = oracle_of(_base().copy())
    assert rel_err(r.atoms[1].trans[0].Rij, q.atoms[1].trans[0].Rij) > 1e-6


def test_moving_atmosphere_is_one_code_path(gpu, monkeypatch):
    """With a velocity field the profiles differ from ray to ray: the three settings are the same code path."""
    prob = _base(moving=True)
    assert np.abs(prob.vlosMu).max() > 0.0
    on, off, gen = run(monkeypatch, prob, iso='1'), run(monkeypatch, prob, iso='0'), run(monkeypatch, prob, pair='0')
    assert_same_bits(on, off, rates=False)
    assert_same_bits(on, gen, rates=False)
    assert_iteration_matches(on, oracle_of(prob.copy()))


def test_flag_drops_when_a_velocity_is_uploaded(gpu, monkeypatch):
    """A static context generates its profiles on the device and iterates; then a velocity field arrives through the
    ordinary upload.  The next iteration regenerates the profiles and must take the general path: against the oracle on
    the same inputs (the device's new profiles, J of the first iteration) with that velocity."""
    from lightweaver_amd.context import Context
    monkeypatch.setenv('LWHIP_LANE_SPLIT', '1')
    p = _base(device=True).copy()
    assert not p.vlosMu.any()
    with Context(p) as ctx:
        ctx.compute_profiles()
        ctx.formal_sol_gamma_matrices()
        q0 = p.copy()
        assert_iteration_matches(p, oracle_of(_with_inputs_of(_base(device=True).copy(), p)))
        p.vlosMu[...] = p.muz[:, None] * models.perturbed(models.falc82(), seed=5).vlos[None, :]
        ctx.upload(abi.ATMOS)
        ctx.formal_sol_gamma_matrices()
        ctx.download(abi.PROFILES)
    q = q0                                # the state the second iteration started from ...
    q.vlosMu[...] = p.vlosMu              # ... with the velocity and the profiles the device made of it
    copy_profiles(q, p)
    t = p.atoms[0].trans[0]
    assert not np.array_equal(t.phi[:, 0, 0], t.phi[:, 0, 1])
    print(assert_iteration_matches(p, oracle_of(q)))


def _with_inputs_of(q, p):
    copy_profiles(q, p)
    return q


@pytest.mark.parametrize('Nrays,split', [(3, '2'), (3, '4'), (5, '2')])
def test_static_split_rays_vs_oracle(gpu, monkeypatch, Nrays, split):
    """A tile's rays split over 2 / 4 wavefronts: every wavefront forms the stencils once, of its first angle, whichever
    rays it holds (3 mu: shares of 3 rays -- the second one starts on the up ray of an angle -- and of 1, 2, 1, 2 rays;
    5 mu: two shares of 5).  Against the oracle, and against the general path the split took before."""
    prob = _base(Nrays=Nrays)
    on, off = run(monkeypatch, prob, iso='1', split=split), run(monkeypatch, prob, iso='0', split=split)
    q = oracle_of(prob.copy())
    print(assert_iteration_matches(on, q))
    assert_iteration_matches(off, q)
    dJ = float(np.max(np.abs(on.J - off.J) / off.J))
    print('J: reuse against the general path', dJ)
    assert dJ < 1e-10


@pytest.mark.parametrize('movingColumn', [None, 2], ids=['all_static', 'one_moving'])
def test_fused_column_batch(gpu, movingColumn):
    """Four columns in one set of launches: the wavefront-wide reuse only if EVERY column's profiles are angle-independent
    -- one moving column and the launch falls back; every column against its own oracle run (on the device's profiles)."""
    from lightweaver_amd.batch import ColumnBatch
    base = models.falc82()
    mk = lambda i: models.throughput_grid(NlambdaTarget=1024, Nrays=3, computeProfiles=False,   # noqa: E731
                                          atmos=models.perturbed(base, seed=100 + i, dv=2e3 if i == movingColumn else 0.0))
    probs = [mk(i) for i in range(4)]
    assert [bool(p.vlosMu.any()) for p in probs] == [i == movingColumn for i in range(4)]
    with ColumnBatch(probs) as batch:
        assert batch._batch is not None
        batch.formal_sol_gamma_matrices()
        for c in batch.contexts:
            c.download(abi.ALL_OUTPUTS | abi.PROFILES)
    for i, p in enumerate(probs):
        q = mk(i)
        copy_profiles(q, p)
        assert_iteration_matches(p, oracle_of(q))
