"""Full Stokes (Zeeman-polarised lines, 1D): the lwhip_stokes ABI, the polarised profiles and the DELO-Bezier3 march.

CPU: the struct layout against the header, the refusals without a device, the projections and the Zeeman components.
GPU: the profiles against a numpy restatement of Transition::compute_polarised_profiles built on scipy's Faddeeva
function, and exact properties of the transfer problem that need no oracle: the scalar solver at unpolarised
wavelengths, the symmetries of field reversal and azimuth rotation on the disc-centre ray, no side effects, and a clean
run at the timed size.  Then the device against the reference: the static fixture (falc_stokes_small.npz) and the parity
matrix of tests/stokes_cases.py (falc_stokes_matrix.npz: velocities, 3 to 130 depth points, every boundary branch, a PRD
line's rho, field edge cases, all four (updateJ, upOnly) variants), and the wavelength chunking, which must be invisible."""
import ctypes as C
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from lightweaver_amd import _abi as abi
from lightweaver_amd.harness import models
from lightweaver_amd.harness import zeeman
from lightweaver_amd.model import StokesData, update_projections

from tests import stokes_cases as sc
from tests import stokes_ref

STRUCTS = [abi.lwhip_stokes_line, abi.lwhip_stokes]


def test_stokes_struct_layout_matches_header(tmp_path):
    import os
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include')
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "lwhip.h"', 'int main(void) {']
    for st in STRUCTS:
        name = st.__name__
        lines.append(f'printf("{name} %zu\\n", sizeof({name}));')
        for fname, _ in st._fields_:
            lines.append(f'printf("{name}.{fname} %zu\\n", offsetof({name}, {fname}));')
    lines.append(f'printf("LWHIP_STOKES %d\\n", (int)LWHIP_STOKES);')
    lines.append('return 0; }')
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'layout'
    subprocess.run(['gcc', '-std=c11', f'-I{inc}', '-o', str(exe), str(src)], check=True)
    got = dict(line.rsplit(' ', 1) for line in subprocess.run([str(exe)], capture_output=True, text=True,
                                                                 check=True).stdout.split('\n') if line)
    for st in STRUCTS:
        name = st.__name__
        assert int(got[name]) == C.sizeof(st), name
        for fname, _ in st._fields_:
            assert int(got[f'{name}.{fname}']) == getattr(st, fname).offset, f'{name}.{fname}'
    assert int(got['LWHIP_STOKES']) == abi.STOKES
    assert abi.STOKES & (abi.ALL_INPUTS | abi.ALL_OUTPUTS) == 0


def test_stokes_entry_points_refuse_without_device(hip_lib):
    if hip_lib.lwhip_device_count() > 0:
        pytest.skip('a device is present: the refusal is the no-device path')
    st = abi.lwhip_stokes()
    assert hip_lib.lwhip_set_stokes(None, C.byref(st)) == abi.ERR_DEVICE
    assert hip_lib.lwhip_compute_polarised_profiles(None) == abi.ERR_DEVICE
    assert hip_lib.lwhip_full_stokes_fs(None, 1, 1, None) == abi.ERR_DEVICE
    assert b'device' in hip_lib.lwhip_last_error()


def test_projections():
    rng = np.random.default_rng(3)
    gamma, chi = rng.uniform(0, np.pi, 7), rng.uniform(0, 2 * np.pi, 7)
    muz = np.array([1.0, 0.6])
    mux = np.array([0.0, 0.8])
    muy = np.zeros(2)
    cg, c2, s2 = update_projections(muz, mux, muy, gamma, chi)
    # disc centre: the exact branch of Atmosphere::update_projections
    assert np.array_equal(cg[0], np.cos(gamma))
    assert np.array_equal(c2[0], np.cos(2 * chi))
    assert np.array_equal(s2[0], np.sin(2 * chi))
    # an inclined ray: cos(gamma') is the field's component along the ray, and (cos 2chi', sin 2chi') a unit vector
    b = np.stack([np.sin(gamma) * np.cos(chi), np.sin(gamma) * np.sin(chi), np.cos(gamma)])
    assert np.allclose(cg[1], 0.8 * b[0] + 0.6 * b[2], rtol=0, atol=1e-15)
    assert np.allclose(c2[1] ** 2 + s2[1] ** 2, 1.0, rtol=0, atol=1e-12)


def test_zeeman_components_ls_coupling():
    T = zeeman.CAII_TERMS
    # Ca II H (4s 2S1/2 - 4p 2P1/2): g = 2 and 2/3, four components, each alpha's strengths summing to 1
    alpha, strength, shift = zeeman.components(T[0], T[3])
    assert sorted(alpha.tolist()) == [-1, 0, 0, 1]
    for al in (-1, 0, 1):
        assert np.isclose(strength[alpha == al].sum(), 1.0, rtol=0, atol=1e-15)
    assert np.allclose(sorted(np.abs(shift)), [2.0 / 3.0, 2.0 / 3.0, 4.0 / 3.0, 4.0 / 3.0])
    assert zeeman.lande_factor(Fraction(3, 2), 1, Fraction(1, 2)) == pytest.approx(4.0 / 3.0)
    # effective Lande factor: three components
    a3, s3, sh3 = zeeman.components(None, None, gLandeEff=1.1)
    assert a3.tolist() == [-1, 0, 1] and np.allclose(sh3, [-1.1, 0.0, 1.1]) and np.all(s3 == 1.0)


# ---- GPU -------------------------------------------------------------------------------------------------------------

def _stokes_problem(lineScale=0.3, Nrays=3, B=0.1, gamma=None, chi=None, disc_centre=True, **kw):
    """FAL-C, H + Ca II with the Ca II lines (H, K, IR triplet) polarised; the last ray is mu = 1 exactly."""
    prob = models.falc_h_ca(Nrays=Nrays, lineScale=lineScale, **kw)
    Ns = prob.Nspace
    if disc_centre:
        prob.muz[-1] = 1.0
    mux = np.sqrt(1.0 - prob.muz ** 2)
    z = np.linspace(0.0, 1.0, Ns)
    Bk = B * (0.5 + z) if np.ndim(B) == 0 else B
    g = 0.3 + 0.9 * z if gamma is None else gamma
    c = 0.2 + 1.1 * z if chi is None else chi
    prob.set_stokes(StokesData(B=Bk, gammaB=g, chiB=c, mux=mux, muy=np.zeros(Nrays),
                               lines=zeeman.polarise_lines(prob, 1)))
    return prob


@pytest.mark.gpu
def test_polarised_profiles_match_faddeeva(gpu):
    from lightweaver_amd.context import Context
    prob = _stokes_problem()
    with Context(prob) as ctx:
        ctx.compute_polarised_profiles()
    assert len(prob.stokes.lines) == 5
    for L in prob.stokes.lines:
        t = prob.atoms[L.atom].trans[L.trans]
        ref = stokes_ref.ref_profiles(prob, L)
        scale = np.abs(ref['phi'])
        assert np.max(np.abs(t.phi - ref['phi']) / scale) <= 1e-12
        # (the dispersion profiles fall off as 1 / v against phi's a / v^2: in the far wings they are measured against
        # their own size as well, since two independent evaluations of w(z) differ there by rounding of F)
        pscale = scale + np.abs(ref['psiQ']) + np.abs(ref['psiU']) + np.abs(ref['psiV'])
        for name in ('phiQ', 'phiU', 'phiV', 'psiQ', 'psiU', 'psiV'):
            got = getattr(L, name)
            assert np.max(np.abs(got - ref[name]) / (scale if name.startswith('phi') else pscale)) <= 1e-12, name
            assert np.abs(got).max() > 0.0, name
        assert np.max(np.abs(t.wphi / ref['wphi'] - 1.0)) <= 1e-12


def _run(prob, **kw):
    from lightweaver_amd.context import Context
    with Context(prob) as ctx:
        ctx.compute_polarised_profiles()
        res = ctx.single_stokes_fs(**kw)
    return res


@pytest.mark.gpu
def test_unpolarised_wavelengths_use_the_scalar_solver(gpu):
    from lightweaver_amd.context import Context
    prob = _stokes_problem()
    prob.J[...] = 0.0   # (without updateJ the Stokes path takes J dagger = 0, as the reference does)
    ref = prob.copy()
    with Context(ref) as ctx:
        ctx.formal_sol(upOnly=True)
    _run(prob, upOnly=True)
    pol = _polarised_mask(prob)
    assert (~pol).sum() > 0 and pol.sum() > 0
    # (the sweep's own Bezier3 restatement rounds differently from this unfused one: 8e-12 measured)
    assert np.max(np.abs(prob.I[~pol] / ref.I[~pol] - 1.0)) <= 1e-10
    assert np.all(prob.Quv[:, ~pol] == 0.0)
    assert np.all(np.isfinite(prob.Quv)) and np.abs(prob.Quv[:, pol]).max() > 0.0


def _polarised_mask(prob):
    m = np.zeros(prob.Nlambda, dtype=bool)
    for L in prob.stokes.lines:
        t = prob.atoms[L.atom].trans[L.trans]
        m[t.Nblue:t.Nred] = True
    return m


@pytest.mark.gpu
def test_field_reversal_symmetry(gpu):
    Ns = models.falc82().Nspace
    z = np.linspace(0.0, 1.0, Ns)
    gamma = 0.3 + 0.9 * z
    a = _stokes_problem(gamma=gamma, chi=np.zeros(Ns))
    b = _stokes_problem(gamma=np.pi - gamma, chi=np.zeros(Ns))
    _run(a, upOnly=True)
    _run(b, upOnly=True)
    pol = _polarised_mask(a)
    I = a.I[pol, -1]
    assert np.max(np.abs(b.I[pol, -1] - I) / I) <= 1e-12
    assert np.max(np.abs(b.Quv[0, pol, -1] - a.Quv[0, pol, -1]) / I) <= 1e-12
    for n in (1, 2):
        assert np.max(np.abs(b.Quv[n, pol, -1] + a.Quv[n, pol, -1]) / I) <= 1e-12
    assert np.abs(a.Quv[2, pol, -1]).max() > 1e-6 * I.max()


@pytest.mark.gpu
def test_azimuth_rotation(gpu):
    Ns = models.falc82().Nspace
    z = np.linspace(0.0, 1.0, Ns)
    chi = 0.2 + 1.1 * z
    a = _stokes_problem(chi=chi)
    b = _stokes_problem(chi=chi + np.pi / 4)
    _run(a, upOnly=True)
    _run(b, upOnly=True)
    pol = _polarised_mask(a)
    I = a.I[pol, -1]
    Q, U, V = a.Quv[:, pol, -1]
    assert np.max(np.abs(b.I[pol, -1] - I) / I) <= 1e-12
    assert np.max(np.abs(b.Quv[0, pol, -1] + U) / I) <= 1e-12
    assert np.max(np.abs(b.Quv[1, pol, -1] - Q) / I) <= 1e-12
    assert np.max(np.abs(b.Quv[2, pol, -1] - V) / I) <= 1e-12
    assert np.abs(Q).max() > 1e-6 * I.max() and np.abs(U).max() > 1e-6 * I.max()


@pytest.mark.gpu
def test_no_side_effects_and_update_j(gpu):
    from lightweaver_amd.context import Context
    prob = _stokes_problem()
    with Context(prob) as ctx:
        ctx.compute_polarised_profiles()
        ctx.download(abi.ALL_OUTPUTS)
        before = prob.outputs()
        ctx.single_stokes_fs(updateJ=False, upOnly=False)
        ctx.download(abi.ALL_OUTPUTS)
        after = prob.outputs()
        for k in before:
            if k != 'I':
                assert np.array_equal(before[k], after[k]), k
        J0 = prob.J.copy()
        res = ctx.single_stokes_fs(updateJ=True, upOnly=False)
    assert res.updatedJ and np.all(np.isfinite(prob.J)) and np.all(prob.J > 0.0)
    dJ = np.abs(1.0 - J0 / prob.J).max(axis=1)
    assert res.dJMax == pytest.approx(dJ.max(), rel=1e-12)
    # the serial loop's index: the last wavelength whose dJ is below the running maximum
    m, idx = 0.0, 0
    for la, v in enumerate(dJ):
        if v < m:
            idx = la
        else:
            m = v
    assert res.dJMaxIdx == idx


@pytest.mark.gpu
def test_timed_size_is_finite(gpu):
    prob = models.throughput_grid()
    Ns = prob.Nspace
    z = np.linspace(0.0, 1.0, Ns)
    prob.set_stokes(StokesData(B=0.1 * (0.5 + z), gammaB=0.3 + 0.9 * z, chiB=0.2 + 1.1 * z,
                               mux=np.sqrt(1.0 - prob.muz ** 2), muy=np.zeros(prob.Nrays),
                               lines=zeeman.polarise_lines(prob, 1)))
    _run(prob, upOnly=True)
    assert np.all(np.isfinite(prob.I)) and np.all(np.isfinite(prob.Quv))
    pol = _polarised_mask(prob)
    assert np.abs(prob.Quv[:, pol]).max() > 0.0 and np.all(prob.Quv[:, ~pol] == 0.0)


# ---- against the reference (falc_stokes_small.npz, tests/golden/make_stokes_golden.py) ---------------------------------

def fixture_problem(d):
    """harness.zeeman.falc_h_ca_stokes with the reference's components, checked against the fixture's inputs."""
    prob = zeeman.falc_h_ca_stokes()
    assert np.array_equal(prob.wavelength, d['in/wavelength']) and np.array_equal(prob.bgChi[:, ::8], d['in/bgChi'])
    assert np.array_equal(prob.J[:, ::8], d['in/J'])
    for i, L in enumerate(prob.stokes.lines):
        L.alpha, L.strength, L.shift = d[f'in/alpha{i}'], d[f'in/strength{i}'], d[f'in/shift{i}']
    return prob


def load_stokes_fixture():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'falc_stokes_small.npz'))


def check_against(prob, d, variant, J20out=None, res=None):
    pol = _polarised_mask(prob)
    I = d[f'out/{variant}/I']
    assert np.max(np.abs(prob.I / I - 1.0)) <= 1e-9, variant
    dq = np.abs(prob.Quv - d[f'out/{variant}/Quv'])[:, pol] / I[pol][None]
    assert dq.max() <= 1e-9, variant
    if variant != 'j20':
        assert np.all(prob.Quv[:, ~pol] == 0.0)
    if res is not None:
        assert np.max(np.abs(prob.J / d[f'out/{variant}/J'] - 1.0)) <= 1e-9
        assert abs(res.dJMax / float(d[f'out/{variant}/dJMax']) - 1.0) <= 1e-9
        assert res.dJMaxIdx == int(d[f'out/{variant}/dJMaxIdx'])
    if J20out is not None:
        ref = d['out/j20/J20']
        assert np.max(np.abs(J20out - ref) / np.abs(ref).max(axis=1, keepdims=True)) <= 1e-9


@pytest.mark.gpu
def test_parity_with_reference(gpu):
    from lightweaver_amd.context import Context
    d = load_stokes_fixture()
    prob = fixture_problem(d)
    with Context(prob) as ctx:
        ctx.compute_polarised_profiles()
        for i, L in enumerate(prob.stokes.lines):
            t = prob.atoms[L.atom].trans[L.trans]
            phi = d[f'prof/phi{i}']
            assert np.max(np.abs(t.phi[..., ::8] - phi) / phi) <= 1e-12
            assert np.max(np.abs(t.wphi / d[f'prof/wphi{i}'] - 1.0)) <= 1e-12
            # (psi falls off as 1 / v against phi's a / v^2: in the far wings psi is up to 1e4 phi and its rounding is
            # measured against its own size as well -- 3e-12 phi at most, 1e-16 of psi)
            pscale = phi + sum(np.abs(d[f'prof/{n}{i}']) for n in ('psiQ', 'psiU', 'psiV'))
            for name in ('phiQ', 'phiU', 'phiV', 'psiQ', 'psiU', 'psiV'):
                sc = phi if name.startswith('phi') else pscale
                assert np.max(np.abs(getattr(L, name)[..., ::8] - d[f'prof/{name}{i}']) / sc) <= 1e-12, name
        ctx.single_stokes_fs(updateJ=False, upOnly=True)
        check_against(prob, d, 'up')
        # unpolarised wavelengths: the scalar Bezier3 against the reference's own (4e-11 measured: the device's exp and
        # the host's differ in the last bit, and the optically thick march carries that; formal_sol's own sweep is 3e-11
        # from the reference on the same kind of problem)
        pol = _polarised_mask(prob)
        assert np.max(np.abs(prob.I[~pol] / d['out/up/I'][~pol] - 1.0)) <= 1e-10
        res = ctx.single_stokes_fs(updateJ=True, upOnly=False)
        check_against(prob, d, 'j', res=res)
    prob = fixture_problem(d)
    J20 = d['in/J20'].copy()
    with Context(prob) as ctx:
        ctx.compute_polarised_profiles()
        res = ctx.single_stokes_fs(updateJ=True, upOnly=False, J20=J20)
        check_against(prob, d, 'j20', J20out=prob.stokes.J20, res=res)
        # J20 is an argument of the call: without it the next call is an ordinary one
        ctx.single_stokes_fs(updateJ=False, upOnly=True)
    pol = _polarised_mask(prob)
    assert np.all(prob.Quv[:, ~pol] == 0.0)


@pytest.mark.gpu
def test_stale_device_profiles_do_not_replace_polarised_phi(gpu):
    from lightweaver_amd.context import Context
    d = load_stokes_fixture()
    prob = fixture_problem(d)
    with Context(prob) as ctx:
        ctx.compute_profiles(deviceResident=True)
        ctx.upload(abi.ATMOS)          # the device-made profiles are stale now
        ctx.compute_polarised_profiles()
        ctx.single_stokes_fs(updateJ=False, upOnly=True)
        ctx.download(abi.PROFILES)
    check_against(prob, d, 'up')
    for i, L in enumerate(prob.stokes.lines):
        t = prob.atoms[L.atom].trans[L.trans]
        assert np.max(np.abs(t.phi[..., ::8] / d[f'prof/phi{i}'] - 1.0)) <= 1e-12


@pytest.mark.gpu
def test_timed_size_against_numpy_march(gpu):
    from lightweaver_amd.context import Context
    prob = models.throughput_grid()
    Ns = prob.Nspace
    z = np.linspace(0.0, 1.0, Ns)
    prob.set_stokes(StokesData(B=0.1 * (0.5 + z), gammaB=0.3 + 0.9 * z, chiB=0.2 + 1.1 * z,
                               mux=np.sqrt(1.0 - prob.muz ** 2), muy=np.zeros(prob.Nrays),
                               lines=zeeman.polarise_lines(prob, 1)))
    J0 = prob.J.copy()
    with Context(prob) as ctx:
        ctx.compute_polarised_profiles()
        ctx.single_stokes_fs(upOnly=True)
        pol = _polarised_mask(prob)
        rng = np.random.default_rng(5)
        las = np.sort(np.concatenate([rng.choice(np.flatnonzero(pol), 48, replace=False),
                                      rng.choice(np.flatnonzero(~pol), 16, replace=False)]))
        I, Quv, *_ = stokes_ref.full_stokes(prob, updateJ=False, upOnly=True, las=las)
        assert np.max(np.abs(prob.I[las] / I - 1.0)) <= 1e-9
        assert np.max(np.abs(prob.Quv[:, las] - Quv) / I[None]) <= 1e-9
        # both directions with J updated: several 256 MB wavelength chunks, each with its own rows of I and Q at every
        # depth for stokes_j_kernel.  A context's chunk is the whole blocks of 64 rays whose 11 + 2 rows of Ns doubles fit
        # into 256 MB, and the whole wavelengths (Nrays x 2 rays each) that these blocks hold
        blocks = (256 << 20) // (13 * Ns * 8 * 64)
        chunk = blocks * 64 // (prob.Nrays * 2)
        assert prob.Nlambda > 2 * chunk
        res = ctx.single_stokes_fs(updateJ=True, upOnly=False)
    las = np.unique(np.concatenate([las, [0, prob.Nlambda - 1]]))
    # (the wavelengths sampled lie in more than one chunk, the last one included)
    assert len(set(las // chunk)) >= 3 and (prob.Nlambda - 1) // chunk in set(las // chunk)
    ref = prob.copy()
    ref.J[...] = J0     # (J dagger of the restatement is the J the call read, not the one it wrote)
    I, Quv, J, _, dJ = stokes_ref.full_stokes(ref, updateJ=True, upOnly=False, las=las)
    print('timed size, updateJ: I', np.max(np.abs(prob.I[las] / I - 1.0)), 'Quv',
          np.max(np.abs(prob.Quv[:, las] - Quv) / I[None]), 'J', np.max(np.abs(prob.J[las] / J - 1.0)))
    assert np.max(np.abs(prob.I[las] / I - 1.0)) <= 1e-9
    assert np.max(np.abs(prob.Quv[:, las] - Quv) / I[None]) <= 1e-9
    assert np.max(np.abs(prob.J[las] / J - 1.0)) <= 1e-9
    assert np.all(np.isfinite(prob.J)) and res.dJMax >= dJ.max() * (1.0 - 1e-9)


# ---- the parity matrix (falc_stokes_matrix.npz, tests/stokes_cases.py) --------------------------------------------------

@pytest.fixture(scope='module')
def matrix():
    return sc.load_fixture()


@pytest.mark.gpu
@pytest.mark.parametrize('case,variant', sc.case_variants())
def test_matrix_against_reference(gpu, matrix, case, variant):
    """The device against the real core on every case and variant of the matrix, to the project's device-vs-reference
    tolerance of 1e-9 (the numpy restatement meets the same bound on the CPU, tests/test_stokes_ref.py)."""
    from lightweaver_amd.context import Context
    updateJ, upOnly = sc.VARIANTS[variant]
    prob = sc.fixture_problem(matrix, case)
    J20 = prob.stokes.J20          # (an argument of the call, as in test_parity_with_reference)
    prob.stokes.J20 = None
    with Context(prob) as ctx:
        ctx.compute_polarised_profiles()
        res = ctx.single_stokes_fs(updateJ=updateJ, upOnly=upOnly, J20=J20)
    pol = sc.polarised_mask(prob, j20=J20 is not None)
    err = sc.errors_against(matrix, case, variant, prob.I, prob.Quv, J=prob.J if updateJ else None,
                            dJMax=res.dJMax if updateJ else None,
                            J20=prob.stokes.J20 if updateJ and J20 is not None else None, pol=pol)
    print('matrix', case, variant, err)
    assert set(err) >= ({'I', 'Quv', 'J', 'dJMax'} if updateJ else {'I', 'Quv'})
    assert all(v <= 1e-9 for v in err.values()), err
    if updateJ:
        assert res.dJMaxIdx == int(matrix[f'out/{case}/{variant}/dJMaxIdx'])
    assert np.all(prob.Quv[:, ~pol] == 0.0)
    if case != 'B0':
        assert np.abs(prob.Quv[:, pol]).max() > 0.0


@pytest.mark.gpu
@pytest.mark.parametrize('case', sc.PROFILE_CASES)
def test_moving_profiles_against_faddeeva(gpu, matrix, case):
    """The device's polarised profiles on a moving atmosphere, both directions: against the numpy restatement built on
    scipy's Faddeeva function at every depth, and against the core's own (every 8th depth)."""
    from lightweaver_amd.context import Context
    prob = sc.fixture_problem(matrix, case)
    with Context(prob) as ctx:
        ctx.compute_polarised_profiles()
    ks = slice(None, None, sc.DEPTH_STRIDE)
    for i, L in enumerate(prob.stokes.lines):
        t = prob.atoms[L.atom].trans[L.trans]
        # the two directions differ: otherwise the sign of the velocity term is invisible
        assert not np.array_equal(t.phi[:, :, 0], t.phi[:, :, 1])
        assert np.max(np.abs(t.phi[:, :, 0] / t.phi[:, :, 1] - 1.0)) > 1e-2
        ref = stokes_ref.ref_profiles(prob, L)
        scale = np.abs(ref['phi'])
        pscale = scale + np.abs(ref['psiQ']) + np.abs(ref['psiU']) + np.abs(ref['psiV'])
        assert np.max(np.abs(t.phi - ref['phi']) / scale) <= 1e-12
        for name in sc.PROFILE_NAMES:
            got = getattr(L, name)
            for d in (0, 1):
                e = np.max(np.abs(got[:, :, d] - ref[name][:, :, d]) / (scale if name.startswith('phi') else pscale)[:, :, d])
                assert e <= 1e-12, (name, d, e)
            assert np.abs(got).max() > 0.0, name
        assert np.max(np.abs(t.wphi / ref['wphi'] - 1.0)) <= 1e-12
        got = {name: getattr(L, name)[..., ks] for name in sc.PROFILE_NAMES}
        got['phi'], got['wphi'] = t.phi[..., ks], t.wphi
        err = sc.profile_errors(matrix, case, i, got)
        print('profiles', case, i, err)
        assert all(v <= 1e-12 for v in err.values()), err


CHUNK_VARIANTS = [(False, True), (False, False), (True, False), (True, True)]


@pytest.mark.gpu
def test_wavelength_chunks_are_invisible(gpu, matrix, monkeypatch):
    """LWHIP_STOKES_CHUNK_LA (a debug knob) caps the wavelengths of a chunk of lwhip_full_stokes_fs: every output is the
    same bits for 1, 7 (no divisor of 208) and 64 wavelengths per chunk as for the whole grid in one.  So it is with
    LWHIP_STOKES_BATCH_RAYS, the column batch's knob, which caps the rays of a chunk: one block of 64 rays, and five."""
    from lightweaver_amd.context import Context
    prob = sc.fixture_problem(matrix, 'moving82')
    rng = np.random.default_rng(11)
    J0 = prob.J.copy()
    J20dag = 0.05 * J0 * (rng.random(J0.shape) - 0.5)
    assert prob.Nlambda == 208
    knobs = ('LWHIP_STOKES_CHUNK_LA', 'LWHIP_STOKES_BATCH_RAYS')
    for k in knobs:
        monkeypatch.delenv(k, raising=False)
    with Context(prob) as ctx:
        ctx.compute_polarised_profiles()
        for updateJ, upOnly in CHUNK_VARIANTS:
            base = None
            for chunk in (None, (0, 1), (0, 7), (0, 64), (1, 64), (1, 5 * 64)):
                for k in knobs:
                    monkeypatch.delenv(k, raising=False)
                if chunk is not None:
                    monkeypatch.setenv(knobs[chunk[0]], str(chunk[1]))
                prob.J[...] = J0
                res = ctx.single_stokes_fs(updateJ=updateJ, upOnly=upOnly, J20=J20dag.copy())
                got = dict(I=prob.I.copy(), Quv=prob.Quv.copy(), J=prob.J.copy(), J20=prob.stokes.J20.copy(),
                           dJMax=np.array(res.dJMax), dJMaxIdx=np.array(res.dJMaxIdx))
                if base is None:
                    base = got
                    assert np.abs(got['Quv']).max() > 0.0 and (not updateJ or not np.array_equal(got['J'], J0))
                    continue
                for k in base:
                    assert np.array_equal(got[k], base[k]), (updateJ, upOnly, chunk, k)
    for k in knobs:
        monkeypatch.delenv(k, raising=False)


def test_stokes_needs_three_depth_points(hip_lib):
    """A 2-point column is refused with ERR_INVALID.  Every context needs Nspace >= 3, so the refusal comes from
    lwhip_create: lwhip_full_stokes_fs, which repeats the check, is never reached with such a column and there is no
    device I or Quv that it could have touched; the 3-point column next to it runs (test_matrix_against_reference[n3-*])."""
    from lightweaver_amd.context import Context, LwHipError
    atmos = models.resample(models.falc82(), 2)
    prob = models.build_problem(atmos, [models.H_6(0.2), models.CaII_6(0.2)], Nrays=3)
    prob.set_stokes(StokesData(B=np.full(2, 0.1), gammaB=np.full(2, 0.3), chiB=np.full(2, 0.2),
                               mux=np.sqrt(1.0 - prob.muz ** 2), muy=np.zeros(3), lines=zeeman.polarise_lines(prob, 1)))
    I0, Q0 = prob.I.copy(), prob.Quv.copy()
    with pytest.raises(LwHipError, match=r'\(%d\).*Nspace >= 3' % abi.ERR_INVALID):
        with Context(prob) as ctx:
            ctx.compute_polarised_profiles()
            ctx.single_stokes_fs(upOnly=True)
    assert np.array_equal(prob.I, I0) and np.array_equal(prob.Quv, Q0)
