"""Emergent spectra along observer rays: lwhip_compute_rays / lwhip_batch_compute_rays, Context.compute_rays,
ColumnBatch.compute_rays and model.observer_problem.

CPU: the symbols and the struct layout, the refusal without a device, observer_problem (the host-side route of the reference,
which is also what feeds the oracle below) pinned against the golden up-only formal solution.
GPU: the device call against OracleContext(observer_problem(...)) -> compute_profiles -> formal_sol(upOnly) at directions that
are not quadrature nodes, against the context's own formal solution at one that is, the depth output, that the context is left
alone, wavelength ranges and shards, column batches (bit-equal to the single context), the refusals."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from helpers import FIXTURES, TOL_ONE_CALL, load_fixture, rel_err, variant_problem
from lightweaver_amd import _abi as abi
from lightweaver_amd.harness import models
from lightweaver_amd.model import observer_problem
from oracle.bindings import OracleContext

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'lwhip.h')
NEW_SYMBOLS = ('lwhip_compute_rays', 'lwhip_batch_compute_rays')
MUS = [1.0, 0.6, 0.2]


# ---- CPU -------------------------------------------------------------------------------------------------------------------

def test_rays_symbols_declared_bound_and_exported(hip_lib):
    txt = open(HEADER).read()
    names = [s[0] for s in abi.SYMBOLS]
    for name in NEW_SYMBOLS:
        assert re.search(rf'\bint {name}\s*\(', txt), name
        assert name in names, name
        fn = getattr(hip_lib, name)
        assert fn.restype is C.c_int and fn.argtypes[1] is C.POINTER(abi.lwhip_rays), name
    m = re.search(r'#define LWHIP_RAYS_MAX_MU (\d+)', txt)
    assert m and int(m.group(1)) == abi.RAYS_MAX_MU


def test_rays_struct_layout_matches_header(tmp_path):
    st = abi.lwhip_rays
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


def test_rays_refuse_without_device(hip_lib):
    if hip_lib.lwhip_device_count() > 0:
        pytest.skip('a device is present: the refusal is the no-device path')
    r = abi.lwhip_rays()
    assert hip_lib.lwhip_compute_rays(None, C.byref(r)) == abi.ERR_DEVICE
    assert b'device' in hip_lib.lwhip_last_error()
    assert hip_lib.lwhip_batch_compute_rays(None, C.byref(r)) == abi.ERR_DEVICE
    assert b'device' in hip_lib.lwhip_last_error()


def test_observer_problem_properties():
    p, _ = load_fixture('falc_h_vel')
    mus = np.array(MUS)
    vz = p.vlosMu[0] / p.muz[0]
    q = observer_problem(p, mus)
    assert q.Nrays == 3 and np.array_equal(q.muz, mus) and np.all(q.wmu == 0.0)
    assert np.array_equal(q.vlosMu, mus[:, None] * vz[None, :]) and np.abs(q.vlosMu).max() > 0.0
    assert q.I.shape == (p.Nlambda, 3)
    # the state is equal and not shared
    for name in ('J', 'bgChi', 'bgEta', 'bgSca', 'height', 'temperature', 'wavelength'):
        a, b = getattr(p, name), getattr(q, name)
        assert np.array_equal(a, b) and not np.shares_memory(a, b), name
    for a, b in zip(p.atoms, q.atoms):
        assert a is not b and np.array_equal(a.n, b.n) and not np.shares_memory(a.n, b.n)
        assert np.array_equal(a.vBroad, b.vBroad) and not np.shares_memory(a.vBroad, b.vBroad)
        for t, u in zip(a.trans, b.trans):
            assert t is not u
            if t.type == abi.LINE:
                assert u.phi.shape == (t.Nlambda, 3, 2, p.Nspace) and not np.any(u.phi)
                assert np.array_equal(t.aDamp, u.aDamp) and not np.shares_memory(t.aDamp, u.aDamp)
    q.descriptor()   # (Problem's own consistency checks pass for the new ray count)
    # explicit v_z and weights
    q2 = observer_problem(p, 0.5, vz=-vz, wmu=[1.0])
    assert np.array_equal(q2.vlosMu, -0.5 * vz[None, :]) and q2.wmu[0] == 1.0
    for bad in (0.0, 1.5, -0.2, [0.5, np.nan]):
        with pytest.raises(ValueError):
            observer_problem(p, bad)
    # a CALLABLE lower boundary has no data for a new direction
    base, d = load_fixture('falc_h_ca_small')
    pb = variant_problem(base, d, 'bc')
    with pytest.raises(ValueError):
        observer_problem(pb, mus)
    bc = np.full((pb.Nlambda, 3), 2.5e-9)
    qb = observer_problem(pb, mus, lowerBc=bc)
    assert qb.zLowerBc.type == abi.BC_CALLABLE and np.array_equal(qb.zLowerBc.bcData, bc)
    assert list(qb.zLowerBc.idxs[:, 1]) == [0, 1, 2]


def oracle_rays(p, mus, **kw):
    """The reference's route: the observer problem, its profiles, its up-only formal solution."""
    q = observer_problem(p, mus, **kw)
    with OracleContext(q) as oc:
        oc.compute_profiles()
        oc.formal_sol(upOnly=True)
    return q.I.copy()


def test_observer_problem_route_reproduces_golden_fs_up():
    """At the problem's own quadrature angles the observer problem is the problem itself (up to the rounding of
    mu * (vlosMu[0] / muz[0]) against vlosMu[mu]): its oracle solution is the golden one of the real core."""
    p, d = load_fixture('falc_h_vel')
    assert np.abs(p.vlosMu).max() > 0.0
    err = rel_err(oracle_rays(p, p.muz), d['out/fs_up/I'])
    print('observer_problem route vs golden fs_up/I:', err)
    assert err <= TOL_ONE_CALL


# ---- GPU -------------------------------------------------------------------------------------------------------------------

def _prd_problem():
    """falc_h_ca_prd after one prd_redistribute on the device: rho differs from 1; rho, J and n downloaded."""
    from lightweaver_amd.context import Context
    from test_prd import golden_prd_problem
    p, _ = golden_prd_problem()
    with Context(p) as ctx:
        p.gamma_prefill()
        ctx.formal_sol_gamma_matrices()
        ctx.prd_redistribute(maxIter=1)
        ctx.download(abi.RHOPRD | abi.J | abi.POPS)
    rho = [t.rhoPrd for a in p.atoms for t in a.trans if t.type == abi.LINE and t.rhoPrd is not None]
    assert rho and max(np.abs(r - 1.0).max() for r in rho) > 1e-3
    return p


def _problem(case):
    if case == 'prd':
        return _prd_problem()
    if case == 'prd_detailed':
        base, d = load_fixture('falc_h_ca_small')
        return variant_problem(base, d, 'prd_detailed')
    return load_fixture(case)[0]


@pytest.mark.gpu
@pytest.mark.parametrize('case', ['falc_h_ca_small', 'falc_h_vel', 'prd', 'prd_detailed'])
def test_rays_against_oracle_off_quadrature(gpu, case):
    from lightweaver_amd.context import Context
    p = _problem(case)
    assert not any(np.any(np.isclose(p.muz, m)) for m in MUS[1:])
    want = oracle_rays(p, MUS)
    with Context(p) as ctx:
        got = ctx.compute_rays(MUS)
        err = rel_err(got, want)
        print(f'{case}: compute_rays vs oracle, mu = {MUS}: {err:.3e}')
        assert got.shape == (p.Nlambda, 3) and err <= TOL_ONE_CALL
        one = ctx.compute_rays(0.6)
        assert one.shape == (p.Nlambda,) and np.array_equal(one, got[:, 1])
        if case == 'falc_h_vel':
            # the Doppler term: its sign and its scaling with mu show far above the tolerance
            vz = p.vlosMu[0] / p.muz[0]
            still = ctx.compute_rays(MUS, vz=np.zeros_like(vz))
            back = ctx.compute_rays(MUS, vz=-vz)
            dStill, dBack = np.max(np.abs(got / still - 1.0)), np.max(np.abs(got / back - 1.0))
            print(f'falc_h_vel: change of I against vz = 0: {dStill:.3e}, against -vz: {dBack:.3e}')
            assert dStill >= 1e-3 and dBack >= 1e-3
            assert rel_err(back, oracle_rays(p, MUS, vz=-vz)) <= TOL_ONE_CALL
            assert np.array_equal(ctx.compute_rays(MUS, vz=vz), got)   # (the default v_z is vlosMu[0] / muz[0])


@pytest.mark.gpu
@pytest.mark.parametrize('name', FIXTURES)
def test_rays_at_quadrature_angles_equal_formal_sol(gpu, name):
    from lightweaver_amd.context import Context
    p, _ = load_fixture(name)
    with Context(p) as ctx:
        ctx.compute_profiles(deviceResident=True)   # (the same phi function on both sides)
        ctx.formal_sol(upOnly=True, deviceResident=True)
        ctx.download(abi.I)
        got = ctx.compute_rays(p.muz)
    err = rel_err(got, p.I)
    print(f'{name}: compute_rays(mus=muz) vs formal_sol(upOnly): {err:.3e}')
    assert err <= TOL_ONE_CALL


@pytest.mark.gpu
@pytest.mark.parametrize('name', FIXTURES)
def test_rays_depth_output(gpu, name):
    """The oracle fills depth data in formal_sol_gamma_matrices only: chi, eta and I of a to-observer ray do not depend on the
    weights, so any positive wmu serves (Gamma of that call is meaningless and ignored)."""
    from lightweaver_amd.context import Context
    p, _ = load_fixture(name)
    q = observer_problem(p, MUS, wmu=np.ones(3))
    if not q.storeDepthData:
        q.storeDepthData = True
        q.depthChi, q.depthEta, q.depthI = (np.zeros((q.Nlambda, 3, 2, q.Nspace)) for _ in range(3))
    with OracleContext(q) as oc:
        oc.compute_profiles()
        q.gamma_prefill()
        oc.formal_sol_gamma_matrices()
    with Context(p) as ctx:
        res = ctx.compute_rays(MUS, depthData=True)
        plain = ctx.compute_rays(MUS)
    errs = {k: rel_err(a, b[:, :, 1, :]) for k, a, b in (('chi', res.chi, q.depthChi), ('eta', res.eta, q.depthEta),
                                                         ('I', res.Idepth, q.depthI))}
    print(f'{name}: depth output vs oracle: {errs}')
    assert all(e <= TOL_ONE_CALL for e in errs.values()), errs
    assert np.array_equal(res.Idepth[..., 0], res.I) and np.array_equal(res.I, plain)


@pytest.mark.gpu
def test_rays_leave_the_context_alone(gpu):
    from lightweaver_amd.context import Context
    from test_hip_parity import compare_problems
    base, _ = load_fixture('falc_h_vel')

    def run(withRays):
        p = base.copy()
        with Context(p) as ctx:
            ctx.compute_profiles(deviceResident=True)
            if withRays:
                ctx.compute_rays(MUS, depthData=True)
                ctx.compute_rays(1.0, laStart=3, laEnd=40)
            p.gamma_prefill()
            ctx.formal_sol_gamma_matrices()
            ctx.download(abi.PROFILES)
        return p

    a, b = run(False), run(True)
    assert np.array_equal(a.J, b.J) and np.array_equal(a.I, b.I)
    compare_problems(b, a, tol=1e-11, what=('Gamma', 'R'))   # (the run-to-run bound of the atomically summed Gamma)
    for x, y in zip(a.atoms, b.atoms):
        for t, u in zip(x.trans, y.trans):
            if t.type == abi.LINE:
                assert np.array_equal(t.phi, u.phi) and np.array_equal(t.wphi, u.wphi)


@pytest.mark.gpu
def test_rays_wavelength_range_and_shard(gpu):
    from lightweaver_amd.context import Context, LwHipError
    p, _ = load_fixture('falc_h_vel')
    Nla = p.Nlambda
    lo, hi = Nla // 3, Nla // 3 + 57
    with Context(p) as ctx:
        full = ctx.compute_rays(MUS, depthData=True)
        part = ctx.compute_rays(MUS, laStart=lo, laEnd=hi, depthData=True)
        assert part.I.shape == (hi - lo, 3)
        assert np.array_equal(part.I, full.I[lo:hi]) and np.array_equal(part.Idepth, full.Idepth[lo:hi])
        assert np.array_equal(part.chi, full.chi[lo:hi]) and np.array_equal(part.eta, full.eta[lo:hi])
        assert np.array_equal(ctx.compute_rays(MUS, laStart=0, laEnd=lo), full.I[:lo])
    cut = Nla // 2 + 3
    for s, e in ((0, cut), (cut, Nla)):
        with Context(p.copy(), laStart=s, laEnd=e, worldSize=2, worldRank=0 if s == 0 else 1) as sh:
            own = sh.compute_rays(MUS)
            assert own.shape == (e - s, 3) and np.array_equal(own, full.I[s:e])
            inner = sh.compute_rays(MUS, laStart=s + 5, laEnd=e - 7)
            assert np.array_equal(inner, full.I[s + 5:e - 7])
            with pytest.raises(LwHipError):
                sh.compute_rays(MUS, laStart=max(s - 1, 0), laEnd=min(e + 1, Nla))   # (one row outside the shard)


def _columns(n, seed0=700):
    return [models.build_problem(models.perturbed(models.falc82(), seed=seed0 + i, dv=2.0e3),
                                 [models.H_6(0.3), models.CaII_6(0.3)], Nrays=3) for i in range(n)]


@pytest.mark.gpu
def test_rays_batch_equals_single_context_and_oracle(gpu):
    from lightweaver_amd.batch import ColumnBatch
    from lightweaver_amd.context import Context
    probs = _columns(8)
    assert all(np.abs(p.vlosMu).max() > 0.0 for p in probs)
    singles = []
    for p in probs:
        with Context(p.copy()) as ctx:
            singles.append(ctx.compute_rays(MUS, depthData=True))
    with ColumnBatch([p.copy() for p in probs]) as b:
        assert b._batch is not None
        got = b.compute_rays(MUS)
        dep = b.compute_rays(MUS, depthData=True)
        sub = b.compute_rays(MUS, laStart=10, laEnd=75)
        vz2 = [2.0 * (p.vlosMu[0] / p.muz[0]) for p in probs]
        fast = b.compute_rays(MUS, vz=vz2)
    with ColumnBatch([p.copy() for p in probs], fused=False) as u:
        assert u._batch is None
        unfused = u.compute_rays(MUS)
    assert got.shape == (8, probs[0].Nlambda, 3)
    for i, s in enumerate(singles):
        assert np.array_equal(got[i], s.I), i
        assert np.array_equal(unfused[i], s.I), i
        assert np.array_equal(dep.I[i], s.I) and np.array_equal(dep.Idepth[i], s.Idepth), i
        assert np.array_equal(dep.chi[i], s.chi) and np.array_equal(dep.eta[i], s.eta), i
        assert np.array_equal(sub[i], s.I[10:75]), i
    assert not np.array_equal(got[0], got[1]) and not np.array_equal(fast, got)
    for i in (0, 5):
        err = rel_err(got[i], oracle_rays(probs[i], MUS))
        print(f'batch column {i} vs oracle: {err:.3e}')
        assert err <= TOL_ONE_CALL
    assert rel_err(fast[3], oracle_rays(probs[3], MUS, vz=vz2[3])) <= TOL_ONE_CALL


@pytest.mark.gpu
def test_rays_large_batch_c4_size(gpu):
    from lightweaver_amd.batch import ColumnBatch
    from lightweaver_amd.context import Context
    base = models.falc82()
    probs = [models.falc_h_ca(Nrays=5, lineScale=3.1, atmos=models.perturbed(base, seed=1234 + c), computeProfiles=False)
             for c in range(512)]
    assert 2800 <= probs[0].Nlambda <= 3200
    with ColumnBatch(probs) as b:
        assert b._batch is not None
        got = b.compute_rays(1.0)
    assert got.shape == (512, probs[0].Nlambda, 1) and np.all(np.isfinite(got)) and np.all(got > 0.0)
    assert not np.array_equal(got[0], got[511])
    for i in (0, 137, 511):
        with Context(probs[i].copy()) as ctx:
            assert np.array_equal(ctx.compute_rays(1.0, squeeze=False), got[i]), i


@pytest.mark.gpu
def test_rays_refusals_launch_nothing(gpu):
    from lightweaver_amd.batch import ColumnBatch
    from lightweaver_amd.context import Context
    p, d = load_fixture('falc_h_ca_small')

    def call(ctx, mus, fill=-7.0, **kw):
        """The raw ABI call with a sentinel in the output: (status, message, output untouched)."""
        r, out, keep = ctx._rays_request(mus, kw.pop('laStart', 0), kw.pop('laEnd', 0), kw.pop('vz', None),
                                         kw.pop('lowerBc', None), kw.pop('depthData', False))
        for k, v in kw.items():
            setattr(r, k, v)
        out.I[...] = fill
        st = ctx.lib.lwhip_compute_rays(ctx._h, C.byref(r))
        return st, ctx.lib.lwhip_last_error(), bool(np.all(out.I == fill))

    with Context(p) as ctx:
        lib = ctx.lib
        st, msg, clean = call(ctx, MUS)
        assert st == abi.OK and not clean
        # direction cosines outside (0, 1]: through the ABI (the Python layer refuses them before the call)
        bad = np.array([0.5, 1.25])
        r, out, keep = ctx._rays_request([0.5, 1.0], 0, 0, None, None, False)
        r.muz = bad.ctypes.data_as(abi.f64p)
        out.I[...] = -7.0
        assert lib.lwhip_compute_rays(ctx._h, C.byref(r)) == abi.ERR_INVALID and b'(0, 1]' in lib.lwhip_last_error()
        assert np.all(out.I == -7.0)
        zero = np.array([0.0, 1.0])
        r.muz = zero.ctypes.data_as(abi.f64p)
        assert lib.lwhip_compute_rays(ctx._h, C.byref(r)) == abi.ERR_INVALID and np.all(out.I == -7.0)
        # Nmu over the cap
        many = np.linspace(0.1, 1.0, abi.RAYS_MAX_MU + 1)
        st, msg, clean = call(ctx, many)
        assert st == abi.ERR_UNSUPPORTED and b'LWHIP_RAYS_MAX_MU' in msg and clean
        assert call(ctx, np.linspace(0.1, 1.0, abi.RAYS_MAX_MU))[0] == abi.OK
        # a range outside the context's rows
        for la0, la1 in ((10, p.Nlambda + 1), (40, 40), (50, 20), (-3, 10)):
            st, msg, clean = call(ctx, MUS[:1], Nmu=1, laStart=la0, laEnd=la1)
            assert st == abi.ERR_INVALID and b'wavelength range' in msg, (la0, la1)
        # one of the three depth arrays
        r, out, keep = ctx._rays_request(MUS, 0, 0, None, None, True)
        r.depthEta = None
        assert lib.lwhip_compute_rays(ctx._h, C.byref(r)) == abi.ERR_INVALID and b'go together' in lib.lwhip_last_error()
        assert lib.lwhip_compute_rays(ctx._h, None) == abi.ERR_INVALID
        assert lib.lwhip_compute_rays(None, C.byref(r)) == abi.ERR_INVALID
    # a CALLABLE lower boundary without data; with data it is used
    pb = variant_problem(p, d, 'bc')
    with Context(pb) as ctx:
        st, msg, clean = call(ctx, MUS)
        assert st == abi.ERR_INVALID and b'CALLABLE' in msg and clean
        bc = np.full((pb.Nlambda, 3), 1.0e-9) * np.array([1.0, 2.0, 3.0])
        got = ctx.compute_rays(MUS, lowerBc=bc)
        assert rel_err(got, oracle_rays(pb, MUS, lowerBc=bc)) <= TOL_ONE_CALL
        assert not np.array_equal(got, ctx.compute_rays(MUS, lowerBc=2.0 * bc))
    # the other formal solvers are refused
    for variant in ('linear', 'besser'):
        with Context(variant_problem(p, d, variant)) as ctx:
            st, msg, clean = call(ctx, MUS)
            assert st == abi.ERR_UNSUPPORTED and b'piecewise_bezier3_1d' in msg and clean, variant
    # a batch: a column that differs, a null request list
    probs = _columns(3)
    with ColumnBatch(probs) as b:
        lib = b.contexts[0].lib
        reqs = [c._rays_request(MUS, 0, 0, None, None, False) for c in b.contexts]
        for _, o, _ in reqs:
            o.I[...] = -7.0
        reqs[1][0].Nmu = 2
        arr = (abi.lwhip_rays * 3)(*[r for r, _, _ in reqs])
        assert lib.lwhip_batch_compute_rays(b._batch, arr) == abi.ERR_INVALID and b'column 1' in lib.lwhip_last_error()
        arr[1].Nmu = abi.RAYS_MAX_MU + 1
        assert lib.lwhip_batch_compute_rays(b._batch, arr) == abi.ERR_UNSUPPORTED and b'column 1' in lib.lwhip_last_error()
        assert lib.lwhip_batch_compute_rays(b._batch, None) == abi.ERR_INVALID
        assert lib.lwhip_batch_compute_rays(None, arr) == abi.ERR_INVALID
        assert all(np.all(o.I == -7.0) for _, o, _ in reqs)


@pytest.mark.gpu
def test_rays_refuse_2d_and_hybrid_prd(gpu):
    from lightweaver_amd.context import Context, LwHipError
    from test_fs2d import load_2d_problem
    from test_hprd import hprd_problem
    p2 = load_2d_problem()
    p2 = p2[0] if isinstance(p2, tuple) else p2
    with Context(p2) as ctx:
        with pytest.raises(LwHipError, match='1D plane-parallel'):
            ctx.compute_rays(1.0)
    ph = hprd_problem()
    with OracleContext(ph.copy()) as oc:
        tables = oc.build_hprd()
        with Context(ph, hprd=tables) as ctx:
            with pytest.raises(LwHipError, match='hybrid PRD'):
                ctx.compute_rays(1.0)


@pytest.mark.gpu
@pytest.mark.parametrize('Ns', [24, 300, 1000])
def test_rays_other_depth_counts(gpu, Ns):
    """Rays per workgroup and the LDS rows follow the depth count (one ray per workgroup from 641 points on;
    lwhip_create admits at most 1 024 in 1D, which is also what a ray's eight LDS rows hold)."""
    from lightweaver_amd.context import Context
    p = models.build_problem(models.perturbed(models.resample(models.falc82(), Ns), seed=3), [models.H_6(0.12)], Nrays=3)
    want = oracle_rays(p, MUS)
    with Context(p) as ctx:
        err = rel_err(ctx.compute_rays(MUS), want)
    print(f'Ns = {Ns}: compute_rays vs oracle {err:.3e}')
    assert err <= TOL_ONE_CALL

