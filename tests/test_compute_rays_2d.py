"""Emergent spectra at arbitrary viewing angles from 2D contexts: lwhip_compute_rays_2d / Context.compute_rays_2d against
the route the reference takes (LwContext.compute_rays, Source/LwMiddleLayer.pyx:3898-4002): model.observer_problem_2d (new
rays, their intersection table, vlosMu = mux vx + muz vz, zero phi) -> compute_profiles -> formal_sol(upOnly=True), through the
oracle, and against tests/golden/rays2d_small.npz, which the real core recorded by that route
(tests/golden/make_rays2d_golden.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from helpers import GOLDEN, TOL_ONE_CALL, load_fixture, rel_err
from lightweaver_amd import _abi as abi
from lightweaver_amd.model import Boundary, observer_problem_2d
from oracle.bindings import OracleContext

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'lwhip.h')
# (muz, mux): the vertical ray, two inclined views with either sign of mux, a grazing one (long characteristics), and an
# inclined direction in the y-z plane (mux = 0, muz < 1)
MUZ = np.array([1.0, 0.6, 0.6, 0.25, 0.9])
MUX = np.array([0.0, 0.8, -0.5, 0.9, 0.0])
INCLINED = [1, 2, 3]
SENTINEL = -7.0


def load_rays2d_golden():
    with np.load(os.path.join(GOLDEN, 'rays2d_small.npz')) as z:
        return {k: z[k] for k in z.files}


def seeded_flow(Ns, seed=77, vzRms=3.0e3, vxRms=4.0e3):
    rng = np.random.default_rng(seed)
    return vzRms * rng.standard_normal(Ns), vxRms * rng.standard_normal(Ns)


def oracle_rays_2d(p, muz, mux, vz, vx, **kw):
    """The reference's route: the observer problem, its profiles, its up-only formal solution."""
    q = observer_problem_2d(p, muz, mux, vz, vx, **kw)
    with OracleContext(q) as oc:
        oc.compute_profiles()
        oc.formal_sol(upOnly=True)
    return q.I.copy()


_cache = {}


def golden_oracle():
    """The oracle's I of the fixture's five directions on falc2d_small, computed once."""
    if 'gold' not in _cache:
        p, _ = load_fixture('falc2d_small')
        g = load_rays2d_golden()
        I = oracle_rays_2d(p, g['muz'], g['mux'], g['vz'], g['vx'])
        I.setflags(write=False)
        _cache['gold'] = (p, g, I)
    return _cache['gold']


# ---- CPU -------------------------------------------------------------------------------------------------------------------

def test_rays2d_symbol_declared_bound_and_exported(hip_lib):
    txt = open(HEADER).read()
    assert re.search(r'\bint lwhip_compute_rays_2d\s*\(', txt)
    assert 'lwhip_compute_rays_2d' in [s[0] for s in abi.SYMBOLS]
    fn = hip_lib.lwhip_compute_rays_2d
    assert fn.restype is C.c_int and fn.argtypes[1] is C.POINTER(abi.lwhip_rays2d)


def test_rays2d_struct_layout_matches_header(tmp_path):
    st = abi.lwhip_rays2d
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


def test_rays2d_null_arguments_and_no_device(hip_lib):
    r = abi.lwhip_rays2d()
    assert hip_lib.lwhip_compute_rays_2d(None, C.byref(r)) == abi.ERR_INVALID
    assert b'null context' in hip_lib.lwhip_last_error()
    if hip_lib.lwhip_device_count() > 0:
        return   # (the rest is the no-device path; with a device test_rays2d_refusals_launch_nothing covers the refusals)
    # a complete request on a handle that is never dereferenced: the device check comes before anything reads it
    muz, mux, vz, vx = np.array([1.0]), np.array([0.0]), np.zeros(4), np.zeros(4)
    I = np.full((3, 1, 2), SENTINEL)
    r.Nmu = 1
    r.muz, r.mux = muz.ctypes.data_as(abi.f64p), mux.ctypes.data_as(abi.f64p)
    r.vz, r.vx, r.I = vz.ctypes.data_as(abi.f64p), vx.ctypes.data_as(abi.f64p), I.ctypes.data_as(abi.f64p)
    fake = C.cast(C.create_string_buffer(64), C.c_void_p)
    assert hip_lib.lwhip_compute_rays_2d(fake, C.byref(r)) == abi.ERR_DEVICE
    assert b'device' in hip_lib.lwhip_last_error()
    assert np.all(I == SENTINEL)
    assert hip_lib.lwhip_compute_rays_2d(fake, None) == abi.ERR_INVALID


def test_observer_problem_2d_properties():
    p, _ = load_fixture('falc2d_small')
    Ns, Nx = p.Nspace, p.grid2d.Nx
    vz, vx = seeded_flow(Ns)
    q = observer_problem_2d(p, MUZ, MUX, vz, vx)
    assert q.Nrays == 5 and np.array_equal(q.muz, MUZ) and np.all(q.wmu == 0.0)
    assert np.array_equal(q.vlosMu, MUX[:, None] * vx[None, :] + MUZ[:, None] * vz[None, :])
    assert q.I.shape == (p.Nlambda, 5, Nx)
    g = q.grid2d
    assert g is not p.grid2d and g.Nrays == 5 and np.array_equal(g.mux, MUX) and np.array_equal(g.muz, MUZ)
    assert g.uw.shape == (5, 2, g.Nz, Nx) and g.substepOff.size - 1 > 0       # (the grazing ray has long characteristics)
    assert np.array_equal(g.x, p.grid2d.x) and np.array_equal(g.temperature, p.grid2d.temperature)
    for name in ('J', 'bgChi', 'bgEta', 'bgSca', 'temperature', 'wavelength'):
        a, b = getattr(p, name), getattr(q, name)
        assert np.array_equal(a, b) and not np.shares_memory(a, b), name
    for a, b in zip(p.atoms, q.atoms):
        assert np.array_equal(a.n, b.n) and not np.shares_memory(a.n, b.n)
        for t, u in zip(a.trans, b.trans):
            if t.type == abi.LINE:
                assert u.phi.shape == (t.Nlambda, 5, 2, Ns) and not np.any(u.phi)
    q.descriptor()
    # defaults: mux = sqrt(1 - muz^2), no horizontal flow
    q1 = observer_problem_2d(p, 0.6, vz=vz)
    assert q1.grid2d.mux[0] == np.sqrt(1.0 - 0.36) and np.array_equal(q1.vlosMu, 0.6 * vz[None, :])
    with pytest.raises(ValueError):
        observer_problem_2d(p, 0.6)                        # vz is required
    with pytest.raises(ValueError):
        observer_problem_2d(p, 0.0, 0.5, vz, vx)
    with pytest.raises(ValueError):
        observer_problem_2d(p, 0.8, 0.7, vz, vx)            # muz^2 + mux^2 > 1
    from lightweaver_amd.model import observer_problem
    with pytest.raises(ValueError):
        observer_problem(p, 1.0)                            # (the 1D call keeps its refusal)
    p1, _ = load_fixture('falc_h_vel')
    with pytest.raises(ValueError):
        observer_problem_2d(p1, 1.0, 0.0, np.zeros(p1.Nspace))


def test_oracle_route_reproduces_recorded_rays2d():
    """The oracle on observer_problem_2d against what the real core recorded: 1e-12 (5.5e-14 measured on this problem's
    twin; the two Voigt functions differ in the last digits, so not bit-equal)."""
    p, g, I = golden_oracle()
    assert g['I'].shape == (p.Nlambda, 5, p.grid2d.Nx) == (90, 5, 10)
    assert np.array_equal(g['muz'], MUZ) and np.array_equal(g['mux'], MUX)
    assert np.all(np.isfinite(g['I'])) and np.all(g['I'] > 0.0)
    err = rel_err(I, g['I'])
    print('oracle route vs recorded rays2d I:', err)
    assert err <= 1e-12


def test_observer_problem_2d_at_quadrature_is_formal_sol():
    """At the problem's own directions, with the problem's own v_z and no horizontal flow, the observer problem is the
    problem itself: its up-only formal solution is that of the fixture."""
    p, g, _ = golden_oracle()
    own = p.copy()
    with OracleContext(own) as oc:
        oc.formal_sol(upOnly=True)
    vz = p.vlosMu[0] / p.muz[0]
    err = rel_err(oracle_rays_2d(p, p.muz, p.grid2d.mux, vz, None), own.I)
    print('observer_problem_2d at the quadrature directions vs formal_sol:', err)
    assert err <= 1e-12


def test_seeded_flow_matters():
    """A kernel that drops vx, or loses the sign of mux, cannot pass against the recorded I: either changes every inclined
    ray by more than 1e-3 (0.07 - 0.70 measured), and vx leaves the two mux = 0 rays bit-equal."""
    p, g, I = golden_oracle()

    def change(a, b):
        return float(np.max(np.abs(a - b) / np.abs(b)))
    noVx = oracle_rays_2d(p, g['muz'], g['mux'], g['vz'], np.zeros_like(g['vx']))
    flipped = oracle_rays_2d(p, g['muz'], -g['mux'], g['vz'], g['vx'])
    noFlow = oracle_rays_2d(p, g['muz'], g['mux'], np.zeros_like(g['vz']), np.zeros_like(g['vx']))
    for m in INCLINED:
        dv, df = change(noVx[:, m], g['I'][:, m]), change(flipped[:, m], g['I'][:, m])
        print('direction', m, 'vx zeroed:', dv, 'mux flipped:', df)
        assert dv > 1e-3 and df > 1e-3, (m, dv, df)
    for m in (0, 4):
        assert np.array_equal(noVx[:, m], I[:, m]), m
    assert change(noFlow, g['I']) > 1e-3


# ---- GPU -------------------------------------------------------------------------------------------------------------------

def check(got, want, what):
    err = rel_err(got, want)
    print(f'{what}: {err:.3e}')
    assert err <= TOL_ONE_CALL, (what, err)


@pytest.mark.gpu
def test_rays2d_five_directions_against_oracle_and_fixture(gpu):
    from lightweaver_amd.context import Context
    p, g, Iorc = golden_oracle()
    with Context(p.copy()) as ctx:
        I = ctx.compute_rays_2d(g['muz'], g['mux'], g['vz'], g['vx'])
        vert = ctx.compute_rays_2d(1.0, 0.0, g['vz'], g['vx'])
        dflt = ctx.compute_rays_2d(1.0, vz=g['vz'])               # mux = sqrt(1 - 1) = 0, vx = 0: the same ray
    assert I.shape == (90, 5, 10)
    check(I, Iorc, 'five directions vs oracle')
    check(I, g['I'], 'five directions vs recorded')
    for m in range(5):
        check(I[:, m], Iorc[:, m], f'direction {m} vs oracle')
    assert vert.shape == (90, 10) and np.array_equal(vert, I[:, 0]) and np.array_equal(dflt, vert)


@pytest.mark.gpu
def test_rays2d_at_quadrature_directions_equal_formal_sol(gpu):
    from lightweaver_amd.context import Context
    p, _ = load_fixture('falc2d_small')
    vz = p.vlosMu[0] / p.muz[0]
    with Context(p) as ctx:
        ctx.formal_sol(upOnly=True)
        ctx.download(abi.I)
        I = ctx.compute_rays_2d(p.muz, p.grid2d.mux, vz, None)
    check(I, p.I, 'quadrature directions vs formal_sol(upOnly)')


def problem_14():
    """14 x 24: Nspace = 336 is one full 256-thread block of the gather plus a remainder."""
    from lightweaver_amd.harness import models
    base = models.resample(models.falc82(), 24)
    cols = [models.perturbed(base, seed=150 + j) for j in range(14)]
    return models.build_problem_2d(cols, np.linspace(0.0, 13.0e5, 14), [models.H_6(0.12)])


def prd_problem_after_redistribution():
    """test_fs2d.prd_problem_2d after one iteration and one redistribution on the device: rho differs from 1."""
    from lightweaver_amd.context import Context
    from test_fs2d import prd_problem_2d
    p = prd_problem_2d()
    with Context(p) as ctx:
        ctx.formal_sol_gamma_matrices()
        ctx.stat_equil()
        ctx.prd_redistribute(2, 1e-2)
    rho = [t.rhoPrd for a in p.atoms for t in a.trans if t.rhoPrd is not None]
    assert rho and max(float(np.abs(r - 1.0).max()) for r in rho) > 1e-3
    return p


def blended_problem():
    from lightweaver_amd.harness import models
    from test_fs2d import blended_atoms
    base = models.resample(models.falc82(), 24)
    cols = [models.perturbed(base, seed=300 + j) for j in range(6)]
    return models.build_problem_2d(cols, np.linspace(0.0, 5 * 40e3, 6), blended_atoms(2))


@pytest.mark.gpu
@pytest.mark.parametrize('case', ['14x24', 'prd', 'blended'])
def test_rays2d_other_problems_against_oracle(gpu, case):
    from lightweaver_amd.context import Context
    p = {'14x24': problem_14, 'prd': prd_problem_after_redistribution, 'blended': blended_problem}[case]()
    vz, vx = seeded_flow(p.Nspace, seed=5)
    muz, mux = MUZ[[0, 1, 2]], MUX[[0, 1, 2]]
    want = oracle_rays_2d(p, muz, mux, vz, vx)
    with Context(p) as ctx:
        got = ctx.compute_rays_2d(muz, mux, vz, vx)
    assert np.all(np.isfinite(got)) and np.all(got > 0.0)
    check(got, want, case)


def callable_lower_problem(seed=9):
    """test_fs2d.callable_z_problem (zUpperBc CALLABLE) with a CALLABLE lower boundary too: a fraction of the Planck function
    of the bottom row, per column and ray."""
    from lightweaver_amd.harness import physics as ph
    from test_fs2d import callable_z_problem
    p = callable_z_problem()
    g = p.grid2d
    rng = np.random.default_rng(seed)
    idxs = np.arange(2 * g.Nrays, dtype=np.int32).reshape(g.Nrays, 2)
    B = np.stack([ph.planck_nu(g.temperature[-1], lam) for lam in p.wavelength])          # [Nlambda, Nx]
    p.zLowerBc = Boundary(abi.BC_CALLABLE, idxs=idxs, bcData=B[:, None, :] * rng.uniform(0.7, 1.0, (1, 2 * g.Nrays, 1)))
    g.zLowerBc = abi.BC_CALLABLE
    return p


def seeded_lower_bc(p, Nmu, seed=21):
    from lightweaver_amd.harness import physics as ph
    rng = np.random.default_rng(seed)
    B = np.stack([ph.planck_nu(p.grid2d.temperature[-1], lam) for lam in p.wavelength])
    return np.ascontiguousarray(B[:, None, :] * rng.uniform(0.5, 1.0, (p.Nlambda, Nmu, p.grid2d.Nx)))


@pytest.mark.gpu
def test_rays2d_callable_z_boundaries(gpu):
    """callable_z_problem as it is (the CALLABLE boundary is the upper one, which an up-going ray never reads: no lowerBc
    needed), and with a CALLABLE lower boundary fed by a seeded lowerBc [Nla, Nmu, Nx]."""
    from lightweaver_amd.context import Context
    from test_fs2d import callable_z_problem
    muz, mux = MUZ[[0, 1, 2]], MUX[[0, 1, 2]]
    p = callable_z_problem()
    vz, vx = seeded_flow(p.Nspace, seed=6)
    with Context(p.copy()) as ctx:
        got = ctx.compute_rays_2d(muz, mux, vz, vx)
    check(got, oracle_rays_2d(p, muz, mux, vz, vx), 'CALLABLE upper boundary')
    pl = callable_lower_problem()
    bc = seeded_lower_bc(pl, 3)
    want = oracle_rays_2d(pl, muz, mux, vz, vx, lowerBc=bc)
    with Context(pl.copy()) as ctx:
        got = ctx.compute_rays_2d(muz, mux, vz, vx, lowerBc=bc)
        sub = ctx.compute_rays_2d(muz, mux, vz, vx, laStart=20, laEnd=50, lowerBc=bc[20:50])
        other = ctx.compute_rays_2d(muz, mux, vz, vx, lowerBc=2.0 * bc)
    check(got, want, 'CALLABLE lower boundary')
    assert np.array_equal(sub, got[20:50])
    assert rel_err(other, got) > 1e-3          # (the data enters)


@pytest.mark.gpu
def test_rays2d_ranges_shards_batches_chunks_and_cache(gpu, monkeypatch):
    from lightweaver_amd.context import Context, LwHipError
    p, g, _ = golden_oracle()
    Nla = p.Nlambda
    args = (g['muz'], g['mux'], g['vz'], g['vx'])
    mu16 = np.linspace(0.2, 1.0, 16)
    mx16 = np.sqrt(1.0 - mu16 ** 2) * np.where(np.arange(16) % 2, -0.9, 0.8)
    with Context(p.copy()) as ctx:
        full = ctx.compute_rays_2d(*args)
        lo, hi = 17, 64
        assert np.array_equal(ctx.compute_rays_2d(*args, laStart=lo, laEnd=hi), full[lo:hi])
        assert np.array_equal(ctx.compute_rays_2d(*args, laStart=0, laEnd=lo), full[:lo])
        # A, then B, then A again: the one-slot geometry cache is replaced correctly
        B = ctx.compute_rays_2d(g['muz'][::-1].copy(), g['mux'][::-1].copy(), g['vz'], g['vx'])
        assert np.array_equal(B[:, ::-1], full)
        assert np.array_equal(ctx.compute_rays_2d(*args), full)
        assert np.array_equal(ctx.compute_rays_2d(*args), full)     # (the cached view)
        full16 = ctx.compute_rays_2d(mu16, mx16, g['vz'], g['vx'])
    cut = Nla // 2 + 3
    for s, e in ((0, cut), (cut, Nla)):
        with Context(p.copy(), laStart=s, laEnd=e, worldSize=2, worldRank=0 if s == 0 else 1) as sh:
            own = sh.compute_rays_2d(*args)
            assert own.shape == (e - s, 5, 10) and np.array_equal(own, full[s:e])
            assert np.array_equal(sh.compute_rays_2d(*args, laStart=s + 5, laEnd=e - 7), full[s + 5:e - 7])
            with pytest.raises(LwHipError, match='wavelength range'):
                sh.compute_rays_2d(*args, laStart=max(s - 1, 0), laEnd=min(e + 1, Nla))
    monkeypatch.setenv('LWHIP_BATCH2D', '1')      # 8 solves of scratch: several batches, and 16 directions go in two chunks
    with Context(p.copy()) as ctx:
        assert np.array_equal(ctx.compute_rays_2d(*args), full)
        chunked = ctx.compute_rays_2d(mu16, mx16, g['vz'], g['vx'])
        assert np.array_equal(chunked, full16)
        for m in range(16):
            one = ctx.compute_rays_2d(float(mu16[m]), float(mx16[m]), g['vz'], g['vx'])
            assert np.array_equal(one, chunked[:, m]), m


@pytest.mark.gpu
def test_rays2d_leave_the_context_alone(gpu):
    from lightweaver_amd.context import Context
    from helpers import collect
    base, g, _ = golden_oracle()

    def run(withRays):
        p = base.copy()
        with Context(p) as ctx:
            ctx.formal_sol_gamma_matrices()
            ctx.download(abi.ALL_OUTPUTS | abi.PROFILES)
            before = {k: v.copy() for k, v in collect(p).items()}
            phi = [(t.phi.copy(), t.wphi.copy()) for a in p.atoms for t in a.trans if t.type == abi.LINE]
            if withRays:
                ctx.compute_rays_2d(g['muz'], g['mux'], g['vz'], g['vx'])
                ctx.compute_rays_2d(1.0, 0.0, g['vz'], g['vx'], laStart=3, laEnd=40)
                for a in p.atoms:          # (what the call leaves on the device is what comes back)
                    a.Gamma[...] = 0.0
                p.J[...] = 0.0
                p.I[...] = 0.0
                ctx.download(abi.ALL_OUTPUTS | abi.PROFILES)
                after = collect(p)
                for k, v in before.items():
                    assert np.array_equal(v, after[k]), k
                lines = [t for a in p.atoms for t in a.trans if t.type == abi.LINE]
                for (f0, w0), t in zip(phi, lines):
                    assert np.array_equal(f0, t.phi) and np.array_equal(w0, t.wphi)
            p.gamma_prefill()
            ctx.formal_sol_gamma_matrices()
        return p

    a, b = run(False), run(True)
    assert np.array_equal(a.J, b.J) and np.array_equal(a.I, b.I)
    for x, y in zip(a.atoms, b.atoms):
        assert np.array_equal(x.Gamma, y.Gamma)
        for t, u in zip(x.trans, y.trans):
            assert np.array_equal(t.Rij, u.Rij) and np.array_equal(t.Rji, u.Rji)


@pytest.mark.gpu
def test_rays2d_refusals_launch_nothing(gpu):
    from lightweaver_amd.context import Context
    from test_fs2d import fixed_x_problem
    p, g, _ = golden_oracle()

    def call(ctx, muz, mux, vz, vx, drop=None, **kw):
        """The raw ABI call with a sentinel in the output: (status, message, output untouched).  drop: a field of the request
        that is set to NULL."""
        r, I, keep = ctx._rays2d_request(muz, mux, vz, vx, kw.pop('laStart', 0), kw.pop('laEnd', 0), kw.pop('lowerBc', None))
        for k, v in kw.items():
            setattr(r, k, v)
        if drop is not None:
            setattr(r, drop, None)
        I[...] = SENTINEL
        st = ctx.lib.lwhip_compute_rays_2d(ctx._h, C.byref(r))
        return st, ctx.lib.lwhip_last_error(), bool(np.all(I == SENTINEL))

    with Context(p.copy()) as ctx:
        lib = ctx.lib
        st, msg, clean = call(ctx, g['muz'], g['mux'], g['vz'], g['vx'])
        assert st == abi.OK and not clean
        many = np.linspace(0.1, 1.0, abi.RAYS_MAX_MU + 1)
        st, msg, clean = call(ctx, many, np.zeros(many.size), g['vz'], g['vx'])
        assert st == abi.ERR_UNSUPPORTED and b'LWHIP_RAYS_MAX_MU' in msg and clean
        # muz = 0 and muz^2 + mux^2 > 1: through the ABI (the Python layer refuses the first before the call)
        for bad in ((0.0, 0.3), (0.8, 0.7), (1.25, 0.0)):
            zm, xm = np.array([1.0, bad[0]]), np.array([0.0, bad[1]])
            r, I, keep = ctx._rays2d_request([1.0, 0.5], [0.0, 0.1], g['vz'], g['vx'], 0, 0, None)
            r.muz, r.mux = zm.ctypes.data_as(abi.f64p), xm.ctypes.data_as(abi.f64p)
            I[...] = SENTINEL
            assert lib.lwhip_compute_rays_2d(ctx._h, C.byref(r)) == abi.ERR_INVALID, bad
            assert np.all(I == SENTINEL), bad
        # a missing vx (and each of the other required arrays)
        for name in ('vx', 'vz', 'mux', 'muz', 'I'):
            st, msg, clean = call(ctx, g['muz'], g['mux'], g['vz'], g['vx'], drop=name)
            assert st == abi.ERR_INVALID and b'required' in msg and clean, name
        for la0, la1 in ((10, p.Nlambda + 1), (40, 40), (50, 20), (-3, 10)):
            st, msg, clean = call(ctx, g['muz'], g['mux'], g['vz'], g['vx'], laStart=la0, laEnd=la1)
            assert st == abi.ERR_INVALID and b'wavelength range' in msg and clean, (la0, la1)
        assert lib.lwhip_compute_rays_2d(ctx._h, None) == abi.ERR_INVALID
        assert lib.lwhip_compute_rays_2d(None, None) == abi.ERR_INVALID
    # a range outside a shard
    with Context(p.copy(), laStart=30, laEnd=p.Nlambda, worldSize=2, worldRank=1) as sh:
        st, msg, clean = call(sh, g['muz'], g['mux'], g['vz'], g['vx'], laStart=29, laEnd=50)
        assert st == abi.ERR_INVALID and b'wavelength range' in msg and clean
    # a 1D context
    p1, _ = load_fixture('falc_h_vel')
    with Context(p1) as ctx:
        st, msg, clean = call(ctx, [1.0], [0.0], np.zeros(p1.Nspace), np.zeros(p1.Nspace))
        assert st == abi.ERR_UNSUPPORTED and b'1D context' in msg and clean
    # fixed x boundaries
    pf = fixed_x_problem()
    with Context(pf) as ctx:
        st, msg, clean = call(ctx, [1.0], [0.0], np.zeros(pf.Nspace), np.zeros(pf.Nspace))
        assert st == abi.ERR_UNSUPPORTED and b'x boundaries' in msg and clean
    # a CALLABLE lower boundary without data; callable_z_problem itself (CALLABLE upper boundary only) needs none
    pl = callable_lower_problem()
    with Context(pl) as ctx:
        st, msg, clean = call(ctx, [1.0], [0.0], np.zeros(pl.Nspace), np.zeros(pl.Nspace))
        assert st == abi.ERR_INVALID and b'CALLABLE' in msg and clean
