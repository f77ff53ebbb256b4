"""Observer rays of hybrid-PRD contexts and column batches: lwhip_compute_rays_hprd, lwhip_batch_compute_rays_hprd,
lwhip_compute_rays_grid_hprd, lwhip_batch_compute_rays_grid_hprd; Context.compute_rays_hprd, ColumnBatch.compute_rays_hprd.

The state under test has a non-trivial rho: three hybrid iterations with three PRD sub-iterations each on the oracle
(tests/test_hprd.py::run_hprd), handed to Context(p, hprd=True) -- both sides start from the same numbers.  The oracle's
route for the new rays is the reference's: observer_problem -> compute_profiles -> build_hprd (configure_hprd_coeffs on the new
vlosMu) -> set_hprd -> formal_sol(upOnly=True).  The bound is TOL_ONE_CALL everywhere: the interpolation adds no rounding of
its own (its coefficients are the table's bits).

CPU: symbols, the refusal without a device, the oracle route against the real core (where oracle/_ref is built), and the
discrimination guard -- the oracle's hybrid spectrum differs from its plain-row one by far more than the tolerance, so a
kernel that ignored the interpolation could not pass; the GPU cases take it as a precondition.
GPU: the stored grid (depth counts x velocity amplitudes, Nmu = 1 and 16, a caller vz), the quadrature angles against the
context's own formal solution, the depth output, ranges and shards, new grids, detailed atoms, column batches, that the context
is left alone, the refusals.  Every oracle result is computed once and only read."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from lightweaver_amd import _abi as abi
from lightweaver_amd.harness import models
from lightweaver_amd.model import observer_problem
from oracle import bindings
from oracle.bindings import OracleContext
from tests.helpers import TOL_ONE_CALL, rel_err
from tests.test_hprd import hprd_problem, run_hprd
from tests.test_hprd_build import detailed_problem, snapshot

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'lwhip.h')
NEW_SYMBOLS = ('lwhip_compute_rays_hprd', 'lwhip_batch_compute_rays_hprd', 'lwhip_compute_rays_grid_hprd',
               'lwhip_batch_compute_rays_grid_hprd')
MUS = [1.0, 0.6, 0.2]
WINDOWS = {
    'caK': np.linspace(392.9, 393.85, 37),
    'two': np.array([393.3, 393.4]),            # Nwave = nlt = 2: the smallest grid the bisection sees
    'HandK': np.linspace(392.0, 398.0, 41),     # H and K both hybrid at every row
    'beyond': np.linspace(385.0, 405.0, 45),    # past both lines' own grids: rho' is held at its end values
}
# the floors of the discrimination guard (hybrid against plain-row spectrum on the oracle, maximum relative difference in I)
GUARD_FLOOR = {'stored': 1e-2, 'caK': 1e-2, 'two': 1e-4}


def atom_models():
    return [models.H_6(0.3), models.CaII_6(0.3, prd=True)]   # (what hprd_problem builds)


def atmosphere(Ns):
    """The column of hprd_problem without its velocities (the background does not depend on them)."""
    return models.falc82() if Ns == 82 else models.resample(models.falc82(), Ns)


@functools.lru_cache(maxsize=None)
def _state(Ns, vamp, seed):
    p, _, _ = run_hprd(OracleContext, hprd_problem(vamp=vamp, seed=seed, Nspace=None if Ns == 82 else Ns), nIter=3, prdIter=3)
    assert p.Nspace == Ns and p.Nlambda == 298
    lines = [t for a in p.atoms for t in a.trans if t.rhoPrd is not None]
    assert len(lines) == 2 and max(np.abs(t.rhoPrd - 1.0).max() for t in lines) > 1e-2   # a non-trivial rho
    return p


def state(Ns=24, vamp=8.0e3, seed=7):
    """A fresh copy of the iterated problem (built once)."""
    return _state(Ns, vamp, seed).copy()


@functools.lru_cache(maxsize=None)
def grid_inputs(Ns, name):
    chi, eta, sca, alpha = models.observer_grid_inputs(atmosphere(Ns), atom_models(), WINDOWS[name])
    return (chi, eta, sca), alpha


def grid_kw(Ns, name):
    bg, alpha = grid_inputs(Ns, name)
    return dict(wavelengths=WINDOWS[name], background=bg, contAlpha=alpha)


def oracle_rays(ctxFactory, p, mus, hybrid=True, includeDetailed=False, depth=False, **kw):
    """The reference's route for new rays (and, with wavelengths in kw, a new grid): the observer problem, its profiles, the
    hybrid tables of ITS vlosMu, its up-only formal solution.  hybrid=False: the same route with rho by row.  depth: chi, eta and
    I of the to-observer direction as well (filled in formal_sol_gamma_matrices only; they do not depend on the weights)."""
    mus = np.atleast_1d(np.asarray(mus, dtype=np.float64))
    q = observer_problem(p, mus, **(dict(kw, wmu=np.ones(mus.size)) if depth else kw))
    if depth:
        q.storeDepthData = True
        q.depthChi, q.depthEta, q.depthI = (np.zeros((q.Nlambda, mus.size, 2, q.Nspace)) for _ in range(3))
    with ctxFactory(q) as oc:
        oc.compute_profiles()
        t = None
        if hybrid and hasattr(oc, 'configure_hprd'):
            t = oc.configure_hprd(includeDetailed)
        elif hybrid:
            t = oc.build_hprd(includeDetailed)
            oc.set_hprd(t)
        if depth:
            q.gamma_prefill()
            oc.formal_sol_gamma_matrices()
        else:
            oc.formal_sol(upOnly=True)
        if t is not None:
            if hasattr(oc, 'set_hprd'):
                oc.set_hprd(None)
            t.close()
    if depth:
        return q.I.copy(), q.depthChi[:, :, 1, :].copy(), q.depthEta[:, :, 1, :].copy(), q.depthI[:, :, 1, :].copy()
    return q.I.copy()


@functools.lru_cache(maxsize=None)
def _want(Ns, vamp, window, flipVz=False, hybrid=True, mus=tuple(MUS), seed=7):
    p = state(Ns, vamp, seed)
    kw = {} if window == 'stored' else grid_kw(Ns, window)
    if flipVz:
        kw['vz'] = -(p.vlosMu[0] / p.muz[0])
    out = oracle_rays(OracleContext, p, list(mus), hybrid=hybrid, **kw)
    out.setflags(write=False)
    return out


def want(Ns, vamp, window='stored', **kw):
    return _want(Ns, float(vamp), window, **kw)


def guard(Ns, vamp, window):
    """The discrimination guard: how far the oracle's hybrid spectrum is from its plain-row one."""
    return rel_err(want(Ns, vamp, window), want(Ns, vamp, window, hybrid=False))


def require_guard(Ns, vamp, window):
    if vamp and window in GUARD_FLOOR:
        assert guard(Ns, vamp, window) > GUARD_FLOOR[window], (Ns, vamp, window)


# ---- CPU -------------------------------------------------------------------------------------------------------------------

def test_hprd_rays_symbols_declared_bound_and_exported(hip_lib):
    txt = open(HEADER).read()
    names = [s[0] for s in abi.SYMBOLS]
    for name in NEW_SYMBOLS:
        assert re.search(rf'\bint {name}\s*\(', txt), name
        assert name in names, name
        fn = getattr(hip_lib, name)
        req = abi.lwhip_rays_grid if '_grid' in name else abi.lwhip_rays
        assert fn.restype is C.c_int and fn.argtypes[1] is C.POINTER(req), name
    m = re.search(r'#define LWHIP_ABI_VERSION (\d+)', txt)
    assert m and int(m.group(1)) == 4 == abi.ABI_VERSION


def test_hprd_rays_refuse_without_device(hip_lib):
    if hip_lib.lwhip_device_count() > 0:
        pytest.skip('a device is present: the refusal is the no-device path')
    r, q = abi.lwhip_rays(), abi.lwhip_rays_grid()
    for name in NEW_SYMBOLS:
        assert getattr(hip_lib, name)(None, C.byref(q if '_grid' in name else r)) == abi.ERR_DEVICE, name
        assert b'device' in hip_lib.lwhip_last_error(), name


@pytest.mark.skipif(not bindings.ref_available(), reason='oracle/_ref not built')
@pytest.mark.parametrize('window', ['stored', 'caK'])
def test_oracle_hybrid_route_against_the_real_core(window):
    """The specification: the oracle's route equals the same route on the reference's own Context (configure_hprd_coeffs and
    Transition::uv themselves) within TOL_ONE_CALL.  Measured at Ns = 24 on the stored grid: 1.7e-11, not bit-equal."""
    p = state(24, 8.0e3)
    kw = {} if window == 'stored' else grid_kw(24, window)
    ref = oracle_rays(bindings.RefContext, p, MUS, **kw)
    err = rel_err(want(24, 8.0e3, window), ref)
    print(f'oracle hybrid route vs the real core, {window}: {err:.3e}')
    assert np.all(np.isfinite(ref)) and err <= TOL_ONE_CALL


@pytest.mark.parametrize('Ns', [24, 82])
@pytest.mark.parametrize('vamp', [8.0e3, 40.0e3])
def test_hybrid_spectrum_differs_from_plain_rows(Ns, vamp):
    """Measured (range over the four cases): stored grid 0.57 - 2.6, caK 0.19 - 1.2, two-point grid 1e-3 - 2e-3."""
    for window, floor in GUARD_FLOOR.items():
        d = guard(Ns, vamp, window)
        print(f'Ns = {Ns}, vamp = {vamp:g}, {window}: hybrid vs plain rows {d:.3e}')
        assert d > floor, (window, d)


# ---- GPU -------------------------------------------------------------------------------------------------------------------

def hybrid_context(p, **kw):
    from lightweaver_amd.context import Context
    ctx = Context(p, hprd=True, **kw)
    assert ctx.hprd_tables is not None
    return ctx


@pytest.mark.gpu
@pytest.mark.parametrize('Ns', [24, 82])
@pytest.mark.parametrize('vamp', [0.0, 8.0e3, 40.0e3])
def test_stored_grid_against_oracle(gpu, Ns, vamp):
    """vamp = 0: every comparison of the rule is a tie.  A caller vz = -v_z flips which clamped end the line-grid edges hit."""
    require_guard(Ns, vamp, 'stored')
    p = state(Ns, vamp)
    with hybrid_context(p) as ctx:
        got = ctx.compute_rays_hprd(MUS)
        err = rel_err(got, want(Ns, vamp))
        print(f'Ns = {Ns}, vamp = {vamp:g}: compute_rays_hprd vs oracle {err:.3e}')
        assert got.shape == (p.Nlambda, 3) and err <= TOL_ONE_CALL
        one = ctx.compute_rays_hprd(0.6)
        assert one.shape == (p.Nlambda,) and np.array_equal(one, got[:, 1])   # Nmu = 1
        vz = p.vlosMu[0] / p.muz[0]
        assert np.array_equal(ctx.compute_rays_hprd(MUS, vz=vz), got)         # (the default v_z)
        back = ctx.compute_rays_hprd(MUS, vz=-vz)
        errBack = rel_err(back, want(Ns, vamp, flipVz=True))
        print(f'   vz = -v_z: {errBack:.3e}')
        assert errBack <= TOL_ONE_CALL and (vamp == 0.0 or not np.array_equal(back, got))


@pytest.mark.gpu
def test_sixteen_directions(gpu):
    mus = tuple(np.linspace(0.05, 1.0, abi.RAYS_MAX_MU))
    p = state(24, 40.0e3)
    with hybrid_context(p) as ctx:
        got = ctx.compute_rays_hprd(list(mus))
    err = rel_err(got, want(24, 40.0e3, mus=mus))
    print(f'Nmu = 16: {err:.3e}')
    assert got.shape == (p.Nlambda, 16) and err <= TOL_ONE_CALL


@pytest.mark.gpu
@pytest.mark.parametrize('vamp', [8.0e3, 40.0e3])
def test_quadrature_angles_equal_formal_sol(gpu, vamp):
    p = state(24, vamp)
    with hybrid_context(p) as ctx:
        ctx.compute_profiles(deviceResident=True)   # (the same phi function on both sides)
        ctx.formal_sol(upOnly=True, deviceResident=True)
        ctx.download(abi.I)
        got = ctx.compute_rays_hprd(p.muz)
    err = rel_err(got, p.I)
    print(f'vamp = {vamp:g}: compute_rays_hprd(mus=muz) vs formal_sol(upOnly): {err:.3e}')
    assert err <= TOL_ONE_CALL


@pytest.mark.gpu
@pytest.mark.parametrize('Ns', [24, 82])
def test_depth_output(gpu, Ns):
    p = state(Ns, 8.0e3)
    I, chi, eta, Id = oracle_rays(OracleContext, p, MUS, depth=True)
    assert rel_err(I, want(Ns, 8.0e3)) <= TOL_ONE_CALL
    with hybrid_context(p) as ctx:
        res = ctx.compute_rays_hprd(MUS, depthData=True)
        plain = ctx.compute_rays_hprd(MUS)
    errs = {'chi': rel_err(res.chi, chi), 'eta': rel_err(res.eta, eta), 'I': rel_err(res.Idepth, Id)}
    print(f'Ns = {Ns}: depth output vs oracle: {errs}')
    assert all(e <= TOL_ONE_CALL for e in errs.values()), errs
    assert np.array_equal(res.Idepth[..., 0], res.I) and np.array_equal(res.I, plain)


def caK_cut(p):
    """Ca II K and a row in its core (393.37 nm)."""
    k = min((t for a in p.atoms for t in a.trans if t.rhoPrd is not None), key=lambda t: t.lambda0)   # K lies blueward of H
    assert abs(k.lambda0 - 393.37) < 0.2 and k.wavelength[0] < 393.3 < 393.5 < k.wavelength[-1]
    cut = int(np.searchsorted(p.wavelength, k.lambda0))
    assert k.Nblue + 11 < cut < k.Nred - 11
    return k, cut


@pytest.mark.gpu
def test_wavelength_range_and_shards(gpu):
    from lightweaver_amd.context import LwHipError
    require_guard(24, 40.0e3, 'stored')
    p = state(24, 40.0e3)
    k, cut = caK_cut(p)
    lo, hi = cut - 11, k.Nred + 3       # from inside K to past its red end
    assert k.Nblue < lo < cut < k.Nred < hi <= p.Nlambda
    with hybrid_context(p) as ctx:
        full = ctx.compute_rays_hprd(MUS, depthData=True)
        assert rel_err(full.I, want(24, 40.0e3)) <= TOL_ONE_CALL
        part = ctx.compute_rays_hprd(MUS, laStart=lo, laEnd=hi, depthData=True)
        assert part.I.shape == (hi - lo, 3)
        assert np.array_equal(part.I, full.I[lo:hi]) and np.array_equal(part.Idepth, full.Idepth[lo:hi])
        assert np.array_equal(part.chi, full.chi[lo:hi]) and np.array_equal(part.eta, full.eta[lo:hi])
    # the two shards in one process, the cut inside K: a ray's rho is interpolated across it, from the whole grid's resident rho
    Nla = p.Nlambda
    with hybrid_context(p.copy(), laStart=0, laEnd=cut, worldSize=2, worldRank=0) as A, \
            hybrid_context(p.copy(), laStart=cut, laEnd=Nla, worldSize=2, worldRank=1) as B:
        for sh, s, e in ((A, 0, cut), (B, cut, Nla)):
            own = sh.compute_rays_hprd(MUS)
            assert own.shape == (e - s, 3) and np.array_equal(own, full.I[s:e]), (s, e)
            inner = sh.compute_rays_hprd(MUS, laStart=s + 5, laEnd=e - 7)
            assert np.array_equal(inner, full.I[s + 5:e - 7])
            with pytest.raises(LwHipError, match='wavelength range'):
                sh.compute_rays_hprd(MUS, laStart=max(s - 1, 0), laEnd=min(e + 1, Nla))
            with pytest.raises(LwHipError, match='shard'):
                sh.compute_rays_hprd(MUS, **grid_kw(24, 'caK'))


@pytest.mark.gpu
@pytest.mark.parametrize('window', list(WINDOWS))
@pytest.mark.parametrize('Ns,vamp', [(24, 8.0e3), (82, 40.0e3)])
def test_new_grid_against_oracle(gpu, window, Ns, vamp):
    require_guard(Ns, vamp, window)
    ref = want(Ns, vamp, window)
    assert np.all(np.isfinite(ref)) and np.all(ref > 0.0)    # (the oracle's own result, before it is relied on)
    p = state(Ns, vamp)
    with hybrid_context(p) as ctx:
        got = ctx.compute_rays_hprd(MUS, **grid_kw(Ns, window))
    err = rel_err(got, ref)
    print(f'{window}, Ns = {Ns}, vamp = {vamp:g}: grid vs oracle {err:.3e}; hybrid vs plain rows '
          f'{rel_err(ref, want(Ns, vamp, window, hybrid=False)):.3e}')
    assert got.shape == (WINDOWS[window].size, 3) and err <= TOL_ONE_CALL


@pytest.mark.gpu
def test_new_grid_depth_output(gpu):
    p = state(24, 8.0e3)
    I, chi, eta, Id = oracle_rays(OracleContext, p, MUS, depth=True, **grid_kw(24, 'caK'))
    with hybrid_context(p) as ctx:
        res = ctx.compute_rays_hprd(MUS, depthData=True, **grid_kw(24, 'caK'))
    errs = {'Iout': rel_err(res.I, want(24, 8.0e3, 'caK')), 'chi': rel_err(res.chi, chi), 'eta': rel_err(res.eta, eta),
            'I': rel_err(res.Idepth, Id)}
    print(f'caK depth output vs oracle: {errs}')
    assert all(e <= TOL_ONE_CALL for e in errs.values()), errs


@functools.lru_cache(maxsize=None)
def detailed_state():
    """detailed_problem with rho of every PRD line set by a seeded generator."""
    p = detailed_problem()
    rng = np.random.default_rng(23)
    for a in p.atoms:
        for t in a.trans:
            if t.rhoPrd is not None:
                t.rhoPrd[...] = 1.0 + 0.3 * rng.random(t.rhoPrd.shape)
    return p


@pytest.mark.gpu
@pytest.mark.parametrize('prdDetailed', [0, 1])
def test_detailed_atoms_follow_the_hybrid_line_list(gpu, prdDetailed):
    """The hybrid list is what configure_hprd_coeffs covered: 1 line without the detailed atoms' lines, 3 with them; a PRD line
    outside it keeps rho by row.  The oracle's two spectra differ by 0.24."""
    from lightweaver_amd.context import Context, LwHipError
    p = detailed_state().copy()
    refs = [oracle_rays(OracleContext, p, MUS, includeDetailed=bool(d)) for d in (0, 1)]
    assert rel_err(refs[0], refs[1]) > 1e-2
    try:
        ctx = Context(p, hprd=True, prdDetailed=bool(prdDetailed))
    except LwHipError as e:
        pytest.skip(f'lwhip_create does not admit this problem as a hybrid context: {e}')
    with ctx:
        assert int(ctx.hprd_tables.ptr.contents.Nlines) == (3 if prdDetailed else 1)
        got = ctx.compute_rays_hprd(MUS)
    err = rel_err(got, refs[prdDetailed])
    print(f'prdDetailed = {prdDetailed}: vs oracle {err:.3e}; vs the other line list {rel_err(got, refs[1 - prdDetailed]):.3e}')
    assert err <= TOL_ONE_CALL


COLUMNS = ((8.0e3, 7), (40.0e3, 8), (20.0e3, 9))   # (velocity amplitude, seed) of each column


def column_states():
    return [state(24, v, s) for v, s in COLUMNS]


@pytest.mark.gpu
def test_column_batch_equals_lone_contexts_and_oracle(gpu):
    from lightweaver_amd.batch import ColumnBatch
    probs = column_states()
    assert not np.array_equal(probs[0].vlosMu, probs[1].vlosMu)
    kw = grid_kw(24, 'caK')
    bkw = dict(wavelengths=kw['wavelengths'], background=[kw['background']] * 3, contAlpha=[kw['contAlpha']] * 3)
    lone, loneGrid = [], []
    for p in probs:
        with hybrid_context(p.copy()) as ctx:
            lone.append(ctx.compute_rays_hprd(MUS, depthData=True))
            loneGrid.append(ctx.compute_rays_hprd(MUS, **kw))
    with ColumnBatch([p.copy() for p in probs], hprd=True) as b:
        assert b._batch is not None
        got = b.compute_rays_hprd(MUS)
        dep = b.compute_rays_hprd(MUS, depthData=True)
        grid = b.compute_rays_hprd(MUS, **bkw)
        # a column retired beforehand is still served, from the state it stopped in
        b.set_active([0, 2])
        retired = b.compute_rays_hprd(MUS)
        retiredGrid = b.compute_rays_hprd(MUS, **bkw)
        b.set_active(None)
    with ColumnBatch([p.copy() for p in probs], hprd=True, fused=False) as u:
        assert u._batch is None
        unfused = u.compute_rays_hprd(MUS)
    assert got.shape == (3, probs[0].Nlambda, 3) and grid.shape == (3, 37, 3)
    for i, (v, s) in enumerate(COLUMNS):
        assert np.array_equal(got[i], lone[i].I) and np.array_equal(unfused[i], lone[i].I), i
        assert np.array_equal(dep.I[i], lone[i].I) and np.array_equal(dep.Idepth[i], lone[i].Idepth), i
        assert np.array_equal(dep.chi[i], lone[i].chi) and np.array_equal(dep.eta[i], lone[i].eta), i
        assert np.array_equal(grid[i], loneGrid[i]), i
        assert np.array_equal(retired[i], got[i]) and np.array_equal(retiredGrid[i], grid[i]), i
        errs = rel_err(got[i], want(24, v, seed=s)), rel_err(grid[i], want(24, v, 'caK', seed=s))
        print(f'batch column {i} vs oracle: stored {errs[0]:.3e}, caK {errs[1]:.3e}')
        assert max(errs) <= TOL_ONE_CALL
    assert not np.array_equal(got[0], got[1])


def downloads(ctx, p):
    ctx.download(abi.J | abi.I | abi.RHOPRD | abi.POPS)
    lines = [t for a in p.atoms for t in a.trans if t.rhoPrd is not None]
    return [p.J.copy(), p.I.copy(), ctx.hprd_tables.JRest.copy()] + [a.n.copy() for a in p.atoms] + [t.rhoPrd.copy() for t in lines]


@pytest.mark.gpu
def test_the_context_is_left_alone(gpu):
    """Nothing of the context changes: the downloads and the tables are the same bits before and after a stored-grid and a grid
    call, and a following formal solution gives what it gives on a context that never made the calls -- I, a per-ray quantity,
    to the bit; J, JRest, Gamma and the rates within 1e-11, the run-to-run bound of the sums the sweep accumulates with
    atomics (tests/test_compute_rays.py::test_rays_leave_the_context_alone)."""
    from test_hip_parity import compare_problems

    def run(withRays):
        p = state(24, 8.0e3)
        with hybrid_context(p) as ctx:
            p.gamma_prefill()
            ctx.formal_sol_gamma_matrices()   # (JRest and I are not what they were made with)
            if withRays:
                before, tabs = downloads(ctx, p), snapshot(ctx.hprd_tables)
                ctx.compute_rays_hprd(MUS, depthData=True)
                ctx.compute_rays_hprd(1.0, laStart=100, laEnd=160)
                ctx.compute_rays_hprd(MUS, depthData=True, **grid_kw(24, 'caK'))
                after, tabsAfter = downloads(ctx, p), snapshot(ctx.hprd_tables)
                assert all(np.array_equal(x, y) for x, y in zip(before, after))
                for name, x in vars(tabs).items():
                    y = getattr(tabsAfter, name)
                    if name == 'rho':
                        assert all(np.array_equal(u, v) for a, b in zip(x, y) for u, v in zip(a, b))
                    else:
                        assert np.array_equal(x, y), name
            p.gamma_prefill()
            ctx.formal_sol_gamma_matrices()
            ctx.download(abi.J)
            JRest = ctx.hprd_tables.JRest.copy()
        return p, JRest

    (a, Ja), (b, Jb) = run(False), run(True)
    assert np.abs(Ja).max() > 0.0
    assert np.array_equal(a.I, b.I)
    assert rel_err(b.J, a.J) <= 1e-11 and rel_err(Jb, Ja) <= 1e-11
    compare_problems(b, a, tol=1e-11, what=('Gamma', 'R'))


def raw_call(ctx, name, req, out, fill=-7.0):
    """The raw ABI call with a sentinel in every output: (status, message, outputs untouched)."""
    arrs = [a for a in (out.I, out.chi, out.eta, out.Idepth) if a is not None]
    for a in arrs:
        a[...] = fill
    st = getattr(ctx.lib, name)(ctx._h, C.byref(req))
    return st, ctx.lib.lwhip_last_error(), all(bool(np.all(a == fill)) for a in arrs)


def both_calls(ctx, Ns, mus=MUS, depthData=False, **kw):
    """(name, request, outputs) of the stored-grid and the grid call."""
    r, out, keep = ctx._rays_request(mus, kw.get('laStart', 0), kw.get('laEnd', 0), None, None, depthData)
    g = grid_kw(Ns, 'caK')
    q, outG, keepG = ctx._rays_grid_request(mus, g['wavelengths'], g['background'], g['contAlpha'], None, None, depthData)
    return [('lwhip_compute_rays_hprd', r, out, keep), ('lwhip_compute_rays_grid_hprd', q, outG, keepG)]


@pytest.mark.gpu
def test_refusals_launch_nothing(gpu):
    from lightweaver_amd.batch import ColumnBatch
    from lightweaver_amd.context import Context
    from test_fs2d import load_2d_problem
    p = state(24, 8.0e3)
    with hybrid_context(p) as ctx:
        for name, req, out, keep in both_calls(ctx, 24, depthData=True):
            st, msg, clean = raw_call(ctx, name, req, out)
            assert st == abi.OK and not clean, name
        # Nmu above the cap
        for name, req, out, keep in both_calls(ctx, 24, mus=np.linspace(0.1, 1.0, abi.RAYS_MAX_MU + 1)):
            st, msg, clean = raw_call(ctx, name, req, out)
            assert st == abi.ERR_UNSUPPORTED and b'LWHIP_RAYS_MAX_MU' in msg and clean, name
        # what the plain call refuses beside: a direction cosine, a range, one depth array, null arguments
        name, req, out, keep = both_calls(ctx, 24)[0]
        bad = np.array([0.5, 1.25, 1.0])
        req.muz = bad.ctypes.data_as(abi.f64p)
        st, msg, clean = raw_call(ctx, name, req, out)
        assert st == abi.ERR_INVALID and b'(0, 1]' in msg and clean
        name, req, out, keep = both_calls(ctx, 24, laStart=10, laEnd=p.Nlambda + 1)[0]
        st, msg, clean = raw_call(ctx, name, req, out)
        assert st == abi.ERR_INVALID and b'wavelength range' in msg and clean
        for name, req, out, keep in both_calls(ctx, 24, depthData=True):
            (req.rays if '_grid' in name else req).depthEta = None
            st, msg, clean = raw_call(ctx, name, req, out)
            assert st == abi.ERR_INVALID and b'go together' in msg and clean, name
            assert getattr(ctx.lib, name)(ctx._h, None) == abi.ERR_INVALID
            assert getattr(ctx.lib, name)(None, C.byref(req)) == abi.ERR_INVALID
        # the plain calls keep refusing this context
        for name, req, out, keep in both_calls(ctx, 24):
            st, msg, clean = raw_call(ctx, name.replace('_hprd', ''), req, out)
            assert st == abi.ERR_UNSUPPORTED and b'hybrid PRD' in msg and clean, name
    # a context without hybrid tables: plain PRD
    with Context(state(24, 8.0e3)) as ctx:
        for name, req, out, keep in both_calls(ctx, 24, depthData=True):
            st, msg, clean = raw_call(ctx, name, req, out)
            assert st == abi.ERR_INVALID and b'no hybrid PRD tables' in msg and clean, name
    # hybrid contexts with the other formal solvers exist; their observer rays are refused as the plain call refuses them
    ph = hprd_problem(formalSolver=abi.FS_LINEAR_1D, Nspace=24)
    with hybrid_context(ph) as ctx:
        for name, req, out, keep in both_calls(ctx, 24):
            st, msg, clean = raw_call(ctx, name, req, out)
            assert st == abi.ERR_UNSUPPORTED and b'piecewise_bezier3_1d' in msg and clean, name
    # 2D
    p2 = load_2d_problem()
    p2 = p2[0] if isinstance(p2, tuple) else p2
    with Context(p2) as ctx:
        r, out, keep = ctx._rays_request(MUS, 0, 0, None, None, False)
        st, msg, clean = raw_call(ctx, 'lwhip_compute_rays_hprd', r, out)
        assert st == abi.ERR_UNSUPPORTED and b'1D plane-parallel' in msg and clean
    # a wavelength shard, grid call
    _, cut = caK_cut(p)
    with hybrid_context(state(24, 8.0e3), laStart=0, laEnd=cut, worldSize=2, worldRank=0) as ctx:
        name, req, out, keep = both_calls(ctx, 24)[1]
        st, msg, clean = raw_call(ctx, name, req, out)
        assert st == abi.ERR_UNSUPPORTED and b'shard' in msg and clean
    # batches: a column that differs is named; a batch without hybrid tables
    probs = column_states()
    g = grid_kw(24, 'caK')
    with ColumnBatch(probs, hprd=True) as b:
        lib = b.contexts[0].lib
        reqs = [c._rays_request(MUS, 0, 0, None, None, False) for c in b.contexts]
        greqs = [c._rays_grid_request(MUS, g['wavelengths'], g['background'], g['contAlpha'], None, None, False) for c in b.contexts]
        for _, o, _ in reqs + greqs:
            o.I[...] = -7.0
        arr = (abi.lwhip_rays * 3)(*[r for r, _, _ in reqs])
        garr = (abi.lwhip_rays_grid * 3)(*[q for q, _, _ in greqs])
        arr[1].Nmu = 2
        assert lib.lwhip_batch_compute_rays_hprd(b._batch, arr) == abi.ERR_INVALID and b'column 1' in lib.lwhip_last_error()
        arr[1].Nmu = abi.RAYS_MAX_MU + 1
        assert lib.lwhip_batch_compute_rays_hprd(b._batch, arr) == abi.ERR_UNSUPPORTED and b'column 1' in lib.lwhip_last_error()
        arr[1].Nmu = 3
        arr[2].laStart, arr[2].laEnd = 5, 50
        assert lib.lwhip_batch_compute_rays_hprd(b._batch, arr) == abi.ERR_INVALID and b'column 2' in lib.lwhip_last_error()
        garr[2].Nwave = 36
        assert lib.lwhip_batch_compute_rays_grid_hprd(b._batch, garr) == abi.ERR_INVALID and b'column 2' in lib.lwhip_last_error()
        garr[2].Nwave = 37
        garr[1].rays.Nmu = 2
        assert lib.lwhip_batch_compute_rays_grid_hprd(b._batch, garr) == abi.ERR_INVALID and b'column 1' in lib.lwhip_last_error()
        assert lib.lwhip_batch_compute_rays_hprd(b._batch, None) == abi.ERR_INVALID
        assert lib.lwhip_batch_compute_rays_hprd(None, arr) == abi.ERR_INVALID
        assert lib.lwhip_batch_compute_rays_grid_hprd(None, garr) == abi.ERR_INVALID
        assert all(np.all(o.I == -7.0) for _, o, _ in reqs + greqs)
    with ColumnBatch(column_states()) as b:
        lib = b.contexts[0].lib
        reqs = [c._rays_request(MUS, 0, 0, None, None, False) for c in b.contexts]
        for _, o, _ in reqs:
            o.I[...] = -7.0
        arr = (abi.lwhip_rays * 3)(*[r for r, _, _ in reqs])
        assert lib.lwhip_batch_compute_rays_hprd(b._batch, arr) == abi.ERR_INVALID
        msg = lib.lwhip_last_error()
        assert b'no hybrid PRD tables' in msg and b'column 0' in msg
        assert all(np.all(o.I == -7.0) for _, o, _ in reqs)
