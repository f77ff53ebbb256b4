"""Observer rays on a caller-chosen wavelength grid: lwhip_compute_rays_grid / lwhip_batch_compute_rays_grid /
lwhip_rays_grid_active, Context.compute_rays(wavelengths=...), ColumnBatch.compute_rays(wavelengths=...),
Context.rays_grid_active, model.observer_problem(wavelengths=...) and harness.models.observer_grid_inputs.

CPU: the symbols and the struct layout, the refusal without a device, observer_problem(wavelengths=...) (the active sets of
seven windows, shapes, J and rho equal to numpy.interp with the end values held, alpha zero beyond an edge, state equal and not
shared), the oracle route against the real core where oracle/_ref is built.
GPU: every window against OracleContext(observer_problem(..., wavelengths=...)) -> compute_profiles -> formal_sol(upOnly) within
TOL_ONE_CALL, the depth output, another depth count, consistency with compute_rays(laStart, laEnd) on rows of the context's own
grid, a CALLABLE lower boundary, column batches (bit-equal to the single context), that the context is left alone and that the
staging buffers are reused and regrown, the refusals."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from helpers import TOL_ONE_CALL, load_fixture, rel_err, variant_problem
from lightweaver_amd import _abi as abi
from lightweaver_amd.harness import models
from lightweaver_amd.model import grid_active_transitions, observer_problem
from oracle import bindings
from oracle.bindings import OracleContext

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'lwhip.h')
NEW_SYMBOLS = ('lwhip_compute_rays_grid', 'lwhip_batch_compute_rays_grid', 'lwhip_rays_grid_active')
MUS = [1.0, 0.37]
H, CA = 0, 1


def atom_models():
    return [models.H_6(0.2), models.CaII_6(0.2, prd=True)]


def randomise(p, seed=11):
    """A state that is not the LTE start: n, J and every rhoPrd changed by a seeded generator (before any context exists)."""
    rng = np.random.default_rng(seed)
    for a in p.atoms:
        a.n *= np.exp(0.3 * rng.standard_normal(a.n.shape))
    p.J *= np.exp(0.2 * rng.standard_normal(p.J.shape))
    for a in p.atoms:
        for t in a.trans:
            if t.rhoPrd is not None:
                t.rhoPrd[...] = 1.0 + 0.3 * rng.random(t.rhoPrd.shape)
    return p


@functools.lru_cache(maxsize=None)
def _base(Ns, seed):
    atmos = models.falc82() if Ns == 82 else models.resample(models.falc82(), Ns)
    atmos = models.perturbed(atmos, seed)
    return atmos, randomise(models.build_problem(atmos, atom_models(), Nrays=3))


def base_problem(Ns=82, seed=3):
    """(atmosphere, a fresh copy of the base problem): 208 wavelengths, 82 depths, non-zero velocities at the defaults."""
    atmos, p = _base(Ns, seed)
    return atmos, p.copy()


def windows(p):
    lam = p.wavelength
    return {
        'caK': np.linspace(392.9, 393.85, 37),
        'halpha': np.linspace(655.9, 656.7, 23),
        'lyman_edge': np.linspace(90.5, 92.5, 11),
        'lyman': np.linspace(93.0, 122.5, 31),
        'last': np.linspace(lam[-1] - 0.5, lam[-1] + 0.5, 9),
        'first': np.linspace(lam[0] - 1.0, lam[0] + 1.0, 7),
        'two': np.array([393.3, 393.4]),
    }


_CA_CONT = {(CA, 'cont', i, 5) for i in range(5)}
ACTIVE = {
    'caK': {(H, 'cont', 2, 5), (H, 'cont', 3, 5), (CA, 'line', 0, 4)},
    'halpha': {(H, 'line', 1, 2), (H, 'cont', 2, 5), (H, 'cont', 3, 5), (H, 'cont', 4, 5)},
    'lyman_edge': {(H, 'line', 0, 4), (H, 'cont', 0, 5), (H, 'cont', 1, 5)} | _CA_CONT,
    'lyman': {(H, 'line', 0, j) for j in (1, 2, 3, 4)} | {(H, 'cont', 1, 5)} | _CA_CONT,
    'last': {(H, 'line', 3, 4)},
    'first': {(H, 'cont', 0, 5)},
    'two': {(H, 'cont', 2, 5), (H, 'cont', 3, 5), (CA, 'line', 0, 4)},
}
WINDOW_NAMES = list(ACTIVE)


def named(p, keys):
    """{(atomIdx, transIdx)} as {(atom, 'line' / 'cont', i, j)}."""
    out = set()
    for ia, kr in keys:
        t = p.atoms[ia].trans[kr]
        out.add((ia, 'line' if t.type == abi.LINE else 'cont', t.i, t.j))
    return out


def grid_inputs(atmos, w):
    chi, eta, sca, alpha = models.observer_grid_inputs(atmos, atom_models(), w)
    return (chi, eta, sca), alpha


def oracle_rays_grid(p, mus, w, bg, alpha, depth=False, **kw):
    """The reference's route on a new grid: the observer problem, its profiles, its up-only formal solution.  depth: the
    to-observer DepthData as well (the oracle fills it in formal_sol_gamma_matrices only; chi, eta and I of a ray do not depend
    on the weights, so any positive wmu serves)."""
    if not depth:
        q = observer_problem(p, mus, wavelengths=w, background=bg, contAlpha=alpha, **kw)
        with OracleContext(q) as oc:
            oc.compute_profiles()
            oc.formal_sol(upOnly=True)
        return q.I.copy()
    q = observer_problem(p, mus, wmu=np.ones(len(mus)), wavelengths=w, background=bg, contAlpha=alpha, **kw)
    q.storeDepthData = True
    q.depthChi, q.depthEta, q.depthI = (np.zeros((q.Nlambda, len(mus), 2, q.Nspace)) for _ in range(3))
    with OracleContext(q) as oc:
        oc.compute_profiles()
        q.gamma_prefill()
        oc.formal_sol_gamma_matrices()
    return q.I.copy(), q.depthChi[:, :, 1, :].copy(), q.depthEta[:, :, 1, :].copy(), q.depthI[:, :, 1, :].copy()


# ---- CPU -------------------------------------------------------------------------------------------------------------------

def test_grid_symbols_declared_bound_and_exported(hip_lib):
    txt = open(HEADER).read()
    names = [s[0] for s in abi.SYMBOLS]
    for name in NEW_SYMBOLS:
        assert re.search(rf'\bint {name}\s*\(', txt), name
        assert name in names, name
        fn = getattr(hip_lib, name)
        assert fn.restype is C.c_int, name
    assert hip_lib.lwhip_compute_rays_grid.argtypes[1] is C.POINTER(abi.lwhip_rays_grid)
    assert hip_lib.lwhip_batch_compute_rays_grid.argtypes[1] is C.POINTER(abi.lwhip_rays_grid)
    m = re.search(r'#define LWHIP_ABI_VERSION (\d+)', txt)
    assert m and int(m.group(1)) == abi.ABI_VERSION == 4   # (additive: the version stays)


def test_rays_grid_struct_layout_matches_header(tmp_path):
    st = abi.lwhip_rays_grid
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', 'int main(void){',
             f'printf("size %zu\\n", sizeof({st.__name__}));']
    for fname, _ in st._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof({st.__name__}, {fname}));')
    lines.append('return 0;}')
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'layout'
    subprocess.run(['gcc', '-std=c11', '-o', str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    got = dict(l.split() for l in out.strip().splitlines())
    assert int(got['size']) == C.sizeof(st)
    for fname, _ in st._fields_:
        assert int(got[fname]) == getattr(st, fname).offset, fname
    assert st.rays.offset == 0 and st.rays.size == C.sizeof(abi.lwhip_rays)


def test_rays_grid_refuse_without_device(hip_lib):
    if hip_lib.lwhip_device_count() > 0:
        pytest.skip('a device is present: the refusal is the no-device path')
    q = abi.lwhip_rays_grid()
    assert hip_lib.lwhip_compute_rays_grid(None, C.byref(q)) == abi.ERR_DEVICE
    assert b'device' in hip_lib.lwhip_last_error()
    assert hip_lib.lwhip_batch_compute_rays_grid(None, C.byref(q)) == abi.ERR_DEVICE
    assert b'device' in hip_lib.lwhip_last_error()


def test_base_problem_is_the_stated_one():
    _, p = base_problem()
    assert p.Nlambda == 208 and p.Nspace == 82 and np.abs(p.vlosMu).max() > 0.0
    rho = [t.rhoPrd for a in p.atoms for t in a.trans if t.rhoPrd is not None]
    assert len(rho) == 2 and all(np.abs(r - 1.0).max() > 0.2 for r in rho)


@pytest.mark.parametrize('name', WINDOW_NAMES)
def test_observer_problem_grid_active_sets_and_shapes(name):
    atmos, p = base_problem()
    w = windows(p)[name]
    bg, alpha = grid_inputs(atmos, w)
    act = grid_active_transitions(p, w)
    assert named(p, [k for k, v in act.items() if v]) == ACTIVE[name]
    q = observer_problem(p, MUS, wavelengths=w, background=bg, contAlpha=alpha)
    Nw, Ns = w.shape[0], p.Nspace
    assert q.Nlambda == Nw and np.array_equal(q.wavelength, w) and q.Nrays == 2
    assert q.J.shape == (Nw, Ns) and q.I.shape == (Nw, 2)
    for a, b in zip((q.bgChi, q.bgEta, q.bgSca), bg):
        assert np.array_equal(a, b) and not np.shares_memory(a, b)
    kept = set()
    for ia, a in enumerate(q.atoms):
        for t in a.trans:
            kept.add((ia, 'line' if t.type == abi.LINE else 'cont', t.i, t.j))
            assert (t.Nblue, t.Nred) == (0, Nw) and np.array_equal(t.wavelength, w)
            if t.type == abi.LINE:
                assert t.phi.shape == (Nw, 2, 2, Ns) and not np.any(t.phi)
            else:
                assert t.alpha.shape == (Nw,)
    assert kept == ACTIVE[name]
    q.descriptor()
    # J: numpy.interp per depth, the end values held outside the old grid
    for k in (0, 17, Ns - 1):
        assert np.array_equal(q.J[:, k], np.interp(w, p.wavelength, p.J[:, k]))
    if name == 'last':
        beyond = w > p.wavelength[-1]
        assert beyond.any() and np.array_equal(q.J[beyond], np.broadcast_to(p.J[-1], (beyond.sum(), Ns)))
    if name == 'first':
        before = w < p.wavelength[0]
        assert before.any() and np.array_equal(q.J[before], np.broadcast_to(p.J[0], (before.sum(), Ns)))
    # the state is equal and not shared
    for x, y in zip(p.atoms, q.atoms):
        assert np.array_equal(x.n, y.n) and not np.shares_memory(x.n, y.n)
    assert np.array_equal(p.height, q.height) and not np.shares_memory(p.height, q.height)


def test_observer_problem_grid_rho_and_alpha():
    atmos, p = base_problem()
    w = windows(p)['caK']
    bg, alpha = grid_inputs(atmos, w)
    q = observer_problem(p, MUS, wavelengths=w, background=bg, contAlpha=alpha)
    old = p.atoms[CA].trans[1]
    (line,) = [t for t in q.atoms[CA].trans if t.type == abi.LINE]
    assert (line.i, line.j) == (0, 4) and line.rhoPrd.shape == (w.shape[0], p.Nspace)
    for k in (0, 40, p.Nspace - 1):
        assert np.array_equal(line.rhoPrd[:, k], np.interp(w, old.wavelength, old.rhoPrd[:, k]))
    assert np.abs(line.rhoPrd - 1.0).max() > 0.1
    # rho held beyond the line's own grid
    wide = np.linspace(old.wavelength[0] - 0.2, old.wavelength[-1] + 0.2, 12)
    bgw, alw = grid_inputs(atmos, wide)
    qw = observer_problem(p, MUS, wavelengths=wide, background=bgw, contAlpha=alw)
    (lw,) = [t for t in qw.atoms[CA].trans if t.type == abi.LINE and (t.i, t.j) == (0, 4)]
    assert np.array_equal(lw.rhoPrd[0], old.rhoPrd[0]) and np.array_equal(lw.rhoPrd[-1], old.rhoPrd[-1])
    # alpha: alpha0 (lambda / edge)^3 up to the edge, 0 beyond it -- the window straddles the Lyman edge
    we = windows(p)['lyman_edge']
    _, ale = grid_inputs(atmos, we)
    hm = atom_models()[H]
    kr = len(hm.lines)    # H cont 0-5
    edge = hm.lambda0(0, 5)
    a = ale[(H, kr)]
    assert np.any(we > edge) and np.any(we <= edge)
    assert np.all(a[we > edge] == 0.0) and np.array_equal(a[we <= edge], hm.continua[0].alpha0 * (we[we <= edge] / edge)**3)
    # on the continuum's own grid the rule is build_problem's
    t = p.atoms[H].trans[kr]
    assert np.array_equal(models.observer_grid_inputs(atmos, atom_models(), t.wavelength)[3][(H, kr)], t.alpha)
    # refusals of the host route
    for bad in (w[::-1], w[:1], np.r_[w[:3], w[2:]]):
        with pytest.raises(ValueError):
            observer_problem(p, MUS, wavelengths=bad, background=bg, contAlpha=alpha)
    with pytest.raises(ValueError):
        observer_problem(p, MUS, wavelengths=w, contAlpha=alpha)
    with pytest.raises(ValueError):
        observer_problem(p, MUS, wavelengths=w, background=bg, contAlpha={})


@pytest.mark.skipif(not bindings.ref_available(), reason='oracle/_ref/liblwref.so not built (no reference sources)')
@pytest.mark.parametrize('name', ['caK', 'lyman'])
def test_oracle_grid_route_against_the_real_core(name):
    from oracle.bindings import RefContext
    atmos, p = base_problem()
    w = windows(p)[name]
    bg, alpha = grid_inputs(atmos, w)
    want = oracle_rays_grid(p, MUS, w, bg, alpha)
    q = observer_problem(p, MUS, wavelengths=w, background=bg, contAlpha=alpha)
    with RefContext(q) as rc:
        rc.compute_profiles()
        rc.formal_sol(upOnly=True)
    err = rel_err(want, q.I)
    print(f'{name}: oracle vs real core on the new grid: {err:.3e}')
    assert np.all(np.isfinite(q.I)) and np.all(q.I > 0.0) and err <= TOL_ONE_CALL


# ---- GPU -------------------------------------------------------------------------------------------------------------------

def ctx_names(ctx, mask):
    return named(ctx.prob, [k for k, v in zip(ctx._trans_index(), mask) if v])


@pytest.mark.gpu
@pytest.mark.parametrize('name', WINDOW_NAMES)
def test_grid_rays_every_window_against_oracle(gpu, name):
    from lightweaver_amd.context import Context
    atmos, p = base_problem()
    w = windows(p)[name]
    bg, alpha = grid_inputs(atmos, w)
    want = oracle_rays_grid(p, MUS, w, bg, alpha)
    with Context(p) as ctx:
        assert ctx_names(ctx, ctx.rays_grid_active(w)) == ACTIVE[name]
        got = ctx.compute_rays(MUS, wavelengths=w, background=bg, contAlpha=alpha)
        one = ctx.compute_rays(0.37, wavelengths=w, background=bg, contAlpha=alpha)
    err = rel_err(got, want)
    print(f'{name}: compute_rays(wavelengths) vs oracle: {err:.3e}')
    assert got.shape == (w.shape[0], 2) and np.all(np.isfinite(want)) and np.all(want > 0.0)
    assert err <= TOL_ONE_CALL
    assert one.shape == (w.shape[0],) and np.array_equal(one, got[:, 1])


@pytest.mark.gpu
def test_grid_rays_depth_output(gpu):
    from lightweaver_amd.context import Context
    atmos, p = base_problem()
    w = windows(p)['caK']
    bg, alpha = grid_inputs(atmos, w)
    I, chi, eta, Id = oracle_rays_grid(p, MUS, w, bg, alpha, depth=True)
    with Context(p) as ctx:
        res = ctx.compute_rays(MUS, wavelengths=w, background=bg, contAlpha=alpha, depthData=True)
        plain = ctx.compute_rays(MUS, wavelengths=w, background=bg, contAlpha=alpha)
    errs = {'chi': rel_err(res.chi, chi), 'eta': rel_err(res.eta, eta), 'I': rel_err(res.Idepth, Id)}
    print(f'depth output on the new grid vs oracle: {errs}')
    assert res.chi.shape == (37, 2, p.Nspace)
    assert all(e <= TOL_ONE_CALL for e in errs.values()), errs
    assert np.array_equal(res.Idepth[..., 0], res.I) and np.array_equal(res.I, plain)


@pytest.mark.gpu
def test_grid_rays_31_depths(gpu):
    from lightweaver_amd.context import Context
    atmos, p = base_problem(Ns=31, seed=5)
    assert p.Nspace == 31
    w = windows(p)['caK']
    bg, alpha = grid_inputs(atmos, w)
    want = oracle_rays_grid(p, MUS, w, bg, alpha)
    with Context(p) as ctx:
        got = ctx.compute_rays(MUS, wavelengths=w, background=bg, contAlpha=alpha)
    err = rel_err(got, want)
    print(f'31 depths: compute_rays(wavelengths) vs oracle: {err:.3e}')
    assert err <= TOL_ONE_CALL


def constant_rows(p):
    """Rows [a, b) of the Ca K line's core on which the set of active transitions does not change, the longest such run."""
    k = p.atoms[CA].trans[1]
    sets = []
    for la in range(p.Nlambda):
        sets.append(frozenset((ia, kr) for ia, a in enumerate(p.atoms) for kr, t in enumerate(a.trans) if t.Nblue <= la < t.Nred))
    best = (0, 0)
    a = k.Nblue
    for la in range(k.Nblue + 1, k.Nred + 1):
        if la == k.Nred or sets[la] != sets[a]:
            if la - a > best[1] - best[0]:
                best = (a, la)
            a = la
    return best[0], best[1], sets[best[0]]


@pytest.mark.gpu
def test_grid_rays_consistent_with_own_rows(gpu):
    from lightweaver_amd.context import Context
    _, p = base_problem()
    a, b, rowSet = constant_rows(p)
    assert b - a >= 8
    w = p.wavelength[a:b].copy()
    act = grid_active_transitions(p, w)
    assert {k for k, v in act.items() if v} == set(rowSet)
    assert named(p, rowSet) == ACTIVE['caK']
    bg = (p.bgChi[a:b].copy(), p.bgEta[a:b].copy(), p.bgSca[a:b].copy())
    alpha = {}
    for ia, kr in rowSet:
        t = p.atoms[ia].trans[kr]
        if t.type == abi.CONTINUUM:
            alpha[(ia, kr)] = t.alpha[a - t.Nblue:b - t.Nblue].copy()
    with Context(p) as ctx:
        own = ctx.compute_rays(MUS, laStart=a, laEnd=b, depthData=True)
        new = ctx.compute_rays(MUS, wavelengths=w, background=bg, contAlpha=alpha, depthData=True)
    errs = {k: rel_err(getattr(new, k), getattr(own, k)) for k in ('I', 'chi', 'eta', 'Idepth')}
    print(f'rows [{a}, {b}): new-grid call vs laStart/laEnd call: {errs}; bit-equal I: {np.array_equal(new.I, own.I)}')
    assert all(e <= TOL_ONE_CALL for e in errs.values()), errs


@pytest.mark.gpu
def test_grid_rays_callable_lower_boundary(gpu):
    from lightweaver_amd.context import Context, LwHipError
    base, d = load_fixture('falc_h_ca_small')
    pb = variant_problem(base, d, 'bc')
    lam = pb.wavelength
    mid = pb.Nlambda // 2
    w = np.linspace(lam[mid], lam[mid + 6], 13)
    bg = tuple(np.stack([np.interp(w, lam, f[:, k]) for k in range(pb.Nspace)], axis=1) for f in (pb.bgChi, pb.bgEta, pb.bgSca))
    act = grid_active_transitions(pb, w)
    alpha = {}
    for (ia, kr), on in act.items():
        t = pb.atoms[ia].trans[kr]
        if on and t.type == abi.CONTINUUM:
            alpha[(ia, kr)] = np.interp(w, t.wavelength, t.alpha)
    bc = np.linspace(1.0e-9, 3.0e-9, w.shape[0] * 2).reshape(w.shape[0], 2)
    want = oracle_rays_grid(pb, MUS, w, bg, alpha, lowerBc=bc)
    with Context(pb) as ctx:
        res = ctx.compute_rays(MUS, wavelengths=w, background=bg, contAlpha=alpha, lowerBc=bc, depthData=True)
        got = res.I
        other = ctx.compute_rays(MUS, wavelengths=w, background=bg, contAlpha=alpha, lowerBc=2.0 * bc, depthData=True)
        with pytest.raises(LwHipError, match='CALLABLE'):
            ctx.compute_rays(MUS, wavelengths=w, background=bg, contAlpha=alpha)
    err = rel_err(got, want)
    print(f'CALLABLE lower boundary on the new grid vs oracle: {err:.3e}')
    assert err <= TOL_ONE_CALL
    # (the atmosphere is opaque here: the boundary shows at the bottom of each ray, not at the top)
    assert np.array_equal(res.Idepth[:, :, -1], bc) and np.array_equal(other.Idepth[:, :, -1], 2.0 * bc)
    assert not np.array_equal(res.Idepth, other.Idepth)


@pytest.mark.gpu
def test_grid_rays_batch_equals_single_context_and_oracle(gpu):
    from lightweaver_amd.batch import ColumnBatch
    from lightweaver_amd.context import Context
    cols = [base_problem(seed=s) for s in (1, 2, 3)]
    w = windows(cols[0][1])['caK']
    ins = [grid_inputs(atmos, w) for atmos, _ in cols]
    bgs, alphas = [i[0] for i in ins], [i[1] for i in ins]
    singles = []
    for (_, p), bg, al in zip(cols, bgs, alphas):
        with Context(p.copy()) as ctx:
            singles.append(ctx.compute_rays(MUS, wavelengths=w, background=bg, contAlpha=al, depthData=True))
    with ColumnBatch([p.copy() for _, p in cols]) as b:
        assert b._batch is not None
        got = b.compute_rays(MUS, wavelengths=w, background=bgs, contAlpha=alphas, depthData=True)
        plain = b.compute_rays(MUS, wavelengths=w, background=bgs, contAlpha=alphas)
    assert got.I.shape == (3, 37, 2) and not np.array_equal(got.I[0], got.I[1])
    for i, s in enumerate(singles):
        assert np.array_equal(got.I[i], s.I) and np.array_equal(plain[i], s.I), i
        assert np.array_equal(got.chi[i], s.chi) and np.array_equal(got.eta[i], s.eta), i
        assert np.array_equal(got.Idepth[i], s.Idepth), i
        err = rel_err(got.I[i], oracle_rays_grid(cols[i][1], MUS, w, bgs[i], alphas[i]))
        print(f'batch column {i} on the new grid vs oracle: {err:.3e}')
        assert err <= TOL_ONE_CALL


@pytest.mark.gpu
def test_grid_rays_leave_the_context_alone(gpu):
    from lightweaver_amd.context import Context
    atmos, base = base_problem()
    wins = windows(base)
    w37, w9 = wins['caK'], wins['last']
    (bg37, al37), (bg9, al9) = grid_inputs(atmos, w37), grid_inputs(atmos, w9)
    state = abi.J | abi.RHOPRD | abi.I | abi.POPS

    def snapshot(p):
        out = [p.J.copy(), p.I.copy()]
        for a in p.atoms:
            out.append(a.n.copy())
            out += [t.rhoPrd.copy() for t in a.trans if t.rhoPrd is not None]
        return out

    def run(withGrid):
        p = base.copy()
        with Context(p, deterministic=True) as ctx:
            ctx.formal_sol(upOnly=True, deviceResident=True)
            extra = None
            if withGrid:
                ctx.download(state)
                before = snapshot(p)
                own0 = ctx.compute_rays(MUS)
                first = ctx.compute_rays(MUS, wavelengths=w37, background=bg37, contAlpha=al37, depthData=True)
                small = ctx.compute_rays(MUS, wavelengths=w9, background=bg9, contAlpha=al9)
                again = ctx.compute_rays(MUS, wavelengths=w37, background=bg37, contAlpha=al37, depthData=True)
                own1 = ctx.compute_rays(MUS)
                ctx.download(state)
                extra = (before, snapshot(p), own0, own1, first, small, again)
            p.gamma_prefill()
            ctx.formal_sol_gamma_matrices()
        return p, extra

    fresh, _ = run(False)
    used, (before, after, own0, own1, first, small, again) = run(True)
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    assert np.array_equal(own0, own1)
    assert small.shape == (9, 2)
    for k in ('I', 'chi', 'eta', 'Idepth'):
        assert np.array_equal(getattr(first, k), getattr(again, k)), k
    assert np.array_equal(fresh.J, used.J) and np.array_equal(fresh.I, used.I)
    for x, y in zip(fresh.atoms, used.atoms):
        assert np.array_equal(x.Gamma, y.Gamma)
        for t, u in zip(x.trans, y.trans):
            assert np.array_equal(t.Rij, u.Rij) and np.array_equal(t.Rji, u.Rji)


def raw_call(ctx, w, bg, alpha, mus=MUS, fill=-7.0, drop=(), **kw):
    """The raw ABI call with a sentinel in the output: (status, message, output untouched).  drop: pointer fields of the
    lwhip_rays_grid block set to NULL; kw: integer fields of the embedded lwhip_rays / the block overwritten."""
    q, out, keep = ctx._rays_grid_request(mus, w, bg, alpha, None, kw.pop('lowerBc', None), False)
    for k in drop:
        setattr(q, k, None)
    for k, v in kw.items():
        setattr(q.rays if k in ('laStart', 'laEnd', 'Nmu') else q, k, v)
    out.I[...] = fill
    st = ctx.lib.lwhip_compute_rays_grid(ctx._h, C.byref(q))
    return st, ctx.lib.lwhip_last_error(), bool(np.all(out.I == fill))


@pytest.mark.gpu
def test_grid_rays_refusals_launch_nothing(gpu):
    from lightweaver_amd.batch import ColumnBatch
    from lightweaver_amd.context import Context
    atmos, p = base_problem()
    w = windows(p)['caK']
    bg, alpha = grid_inputs(atmos, w)
    with Context(p.copy()) as ctx:
        st, msg, clean = raw_call(ctx, w, bg, alpha)
        assert st == abi.OK and not clean
        for bad, word in ((w[::-1].copy(), b'increasing'), (np.r_[w[:5], w[4:]], b'increasing'),
                          (np.r_[w[:5], np.nan, w[6:]], b'finite')):
            st, msg, clean = raw_call(ctx, bad, tuple(np.ones((bad.shape[0], p.Nspace)) for _ in range(3)),
                                      {k: np.ones(bad.shape[0]) for k in alpha})
            assert st == abi.ERR_INVALID and word in msg and clean, (bad, msg)
        st, msg, clean = raw_call(ctx, w[:1], tuple(b[:1] for b in bg), {k: v[:1] for k, v in alpha.items()})
        assert st == abi.ERR_INVALID and b'Nwave' in msg and clean
        st, msg, clean = raw_call(ctx, w, bg, alpha, drop=('bgSca',))
        assert st == abi.ERR_INVALID and b'bgSca' in msg and clean
        st, msg, clean = raw_call(ctx, w, (bg[0], bg[1], None), alpha)
        assert st == abi.ERR_INVALID and b'bgSca' in msg and clean
        # a NULL cross-section: refused for an active continuum, accepted for an inactive one
        active = [k for k, v in zip(ctx._trans_index(), ctx.rays_grid_active(w)) if v]
        cont = [k for k in active if p.atoms[k[0]].trans[k[1]].type == abi.CONTINUUM]
        st, msg, clean = raw_call(ctx, w, bg, {k: v for k, v in alpha.items() if k != cont[0]})
        assert st == abi.ERR_INVALID and b'contAlpha' in msg and clean
        st, msg, clean = raw_call(ctx, w, bg, {k: alpha[k] for k in cont})
        assert st == abi.OK and not clean
        st, msg, clean = raw_call(ctx, w, bg, alpha, laStart=3, laEnd=3 + w.shape[0])
        assert st == abi.ERR_INVALID and b'laStart' in msg and clean
        st, msg, clean = raw_call(ctx, w, bg, alpha, laStart=3)
        assert st == abi.ERR_INVALID and b'laStart' in msg and clean
        assert ctx.lib.lwhip_compute_rays_grid(ctx._h, None) == abi.ERR_INVALID
        with pytest.raises(ValueError, match='stokes'):
            ctx.compute_rays(MUS, wavelengths=w, background=bg, contAlpha=alpha, stokes=True)
        with pytest.raises(ValueError):
            ctx.compute_rays(MUS, wavelengths=w, background=bg, contAlpha=alpha, laStart=2, laEnd=9)
        with pytest.raises(ValueError):
            ctx.compute_rays(MUS, wavelengths=w, contAlpha=alpha)
    # the other formal solvers
    for solver, nm in ((abi.FS_LINEAR_1D, 'linear'), (abi.FS_BESSER_1D, 'besser')):
        q = p.copy()
        q.formalSolver = solver
        with Context(q) as ctx:
            st, msg, clean = raw_call(ctx, w, bg, alpha)
            assert st == abi.ERR_UNSUPPORTED and b'piecewise_bezier3_1d' in msg and clean, nm
    # a wavelength shard
    cut = p.Nlambda // 2
    with Context(p.copy(), laStart=0, laEnd=cut, worldSize=2, worldRank=0) as sh:
        st, msg, clean = raw_call(sh, w, bg, alpha)
        assert st == abi.ERR_UNSUPPORTED and b'shard' in msg and clean
    # a batch: a column with another Nwave; a null request list
    cols = [base_problem(seed=s) for s in (1, 2, 3)]
    with ColumnBatch([q for _, q in cols]) as b:
        lib = b.contexts[0].lib
        ws = [w, w[:20].copy(), w]
        reqs = []
        for (at, _), c, wi in zip(cols, b.contexts, ws):
            bgi, ali = grid_inputs(at, wi)
            reqs.append(c._rays_grid_request(MUS, wi, bgi, ali, None, None, False))
        for _, o, _ in reqs:
            o.I[...] = -7.0
        arr = (abi.lwhip_rays_grid * 3)(*[r for r, _, _ in reqs])
        assert lib.lwhip_batch_compute_rays_grid(b._batch, arr) == abi.ERR_INVALID and b'column 1' in lib.lwhip_last_error()
        assert lib.lwhip_batch_compute_rays_grid(b._batch, None) == abi.ERR_INVALID
        assert lib.lwhip_batch_compute_rays_grid(None, arr) == abi.ERR_INVALID
        assert all(np.all(o.I == -7.0) for _, o, _ in reqs)


@pytest.mark.gpu
def test_grid_rays_refuse_2d_and_hybrid_prd(gpu):
    from lightweaver_amd.context import Context
    from test_fs2d import load_2d_problem
    from test_hprd import hprd_problem
    w = np.linspace(392.9, 393.85, 7)

    def ones(prob):
        return tuple(np.ones((w.shape[0], prob.Nspace)) for _ in range(3))

    def all_alpha(prob):
        return {(ia, kr): np.ones(w.shape[0]) for ia, a in enumerate(prob.atoms) for kr, t in enumerate(a.trans)
                if t.type == abi.CONTINUUM}

    p2 = load_2d_problem()
    p2 = p2[0] if isinstance(p2, tuple) else p2
    with Context(p2) as ctx:
        st, msg, clean = raw_call(ctx, w, ones(p2), all_alpha(p2), mus=[1.0])
        assert st == abi.ERR_UNSUPPORTED and b'1D plane-parallel' in msg and clean
    ph = hprd_problem()
    with OracleContext(ph.copy()) as oc:
        tables = oc.build_hprd()
        with Context(ph, hprd=tables) as ctx:
            st, msg, clean = raw_call(ctx, w, ones(ph), all_alpha(ph), mus=[1.0])
            assert st == abi.ERR_UNSUPPORTED and b'hybrid PRD' in msg and clean
