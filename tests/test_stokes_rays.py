"""Full Stokes along observer rays: lwhip_compute_stokes_rays / lwhip_batch_compute_stokes_rays,
Context.compute_rays(stokes=True), ColumnBatch.compute_rays(stokes=True) and model.observer_problem(stokes=True).

The bound is the project's bound for Stokes results against the reference (tests/stokes_cases.errors_against): 1e-9 on I
(relative) and on |dQuv| / I at the polarised wavelengths.

CPU: the symbols and the struct layout, the refusal without a device, observer_problem(stokes=True), and the numpy route
(observer_problem -> stokes_ref.set_polarised_profiles -> stokes_ref.full_stokes) against the reference's results in
falc_stokes_rays.npz (tests/golden/make_stokes_rays_golden.py).
GPU: the device call against that fixture; against a second Context on the observer problem (compute_polarised_profiles +
single_stokes_fs(upOnly), the device path held to the reference over the whole matrix) for every case of the matrix; at the
context's own angles; that the context is left alone, sub-ranges and chunk knobs; column batches; the physics; the refusals."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from lightweaver_amd import _abi as abi
from lightweaver_amd.harness import models, zeeman
from lightweaver_amd.model import observer_problem, update_projections

from tests import stokes_cases as sc
from tests import stokes_rays_cases as src
from tests import stokes_ref

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'lwhip.h')
NEW_SYMBOLS = ('lwhip_compute_stokes_rays', 'lwhip_batch_compute_stokes_rays')
TOL = 1e-9
MUS = src.MUS
# test 2 wants directions that are no quadrature node of any case (MUS holds mu = 1, the disc-centre ray of most cases)
MUS_OFF = np.array([0.97, 0.6, 0.2])
MATRIX_CASES = [c for c in sc.CASES if c != 'j20']
SMALL = dict(Nrays=3, lineScale=0.2)


@pytest.fixture(scope='module')
def matrix():
    return sc.load_fixture()


@pytest.fixture(scope='module')
def golden():
    return src.load_fixture()


# ---- CPU -------------------------------------------------------------------------------------------------------------------

def test_stokes_rays_symbols_declared_bound_and_exported(hip_lib):
    txt = open(HEADER).read()
    names = [s[0] for s in abi.SYMBOLS]
    for name in NEW_SYMBOLS:
        assert re.search(rf'\bint {name}\s*\(', txt), name
        assert name in names, name
        fn = getattr(hip_lib, name)
        assert fn.restype is C.c_int and fn.argtypes[1] is C.POINTER(abi.lwhip_stokes_rays), name
    assert re.search(r'#define LWHIP_ABI_VERSION 4\b', txt)   # (additive: the ABI version stays)


def test_stokes_rays_struct_layout_matches_header(tmp_path):
    st = abi.lwhip_stokes_rays
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', 'int main(void){',
             f'printf("size %zu\\n", sizeof({st.__name__}));']
    for fname, _ in st._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof({st.__name__}, {fname}));')
    lines.append('return 0;}')
    srcf = tmp_path / 'layout.c'
    srcf.write_text('\n'.join(lines))
    exe = tmp_path / 'layout'
    subprocess.run(['gcc', '-std=c11', '-o', str(exe), str(srcf)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    got = dict(l.split() for l in out.strip().splitlines())
    assert int(got['size']) == C.sizeof(st)
    for fname, _ in st._fields_:
        assert int(got[fname]) == getattr(st, fname).offset, fname
    assert st.rays.offset == 0 and C.sizeof(abi.lwhip_rays) == st.cosGamma.offset


def test_stokes_rays_refuse_without_device(hip_lib):
    if hip_lib.lwhip_device_count() > 0:
        pytest.skip('a device is present: the refusal is the no-device path')
    r = abi.lwhip_stokes_rays()
    assert hip_lib.lwhip_compute_stokes_rays(None, C.byref(r)) == abi.ERR_DEVICE
    assert b'device' in hip_lib.lwhip_last_error()
    assert hip_lib.lwhip_batch_compute_stokes_rays(None, C.byref(r)) == abi.ERR_DEVICE
    assert b'device' in hip_lib.lwhip_last_error()


def test_observer_problem_stokes_properties(matrix, golden):
    p = sc.fixture_problem(matrix, 'moving82')
    q = src.observer(p)
    st, so = p.stokes, q.stokes
    assert q.Nrays == 3 and np.array_equal(q.muz, MUS) and np.all(q.wmu == 0.0)
    assert np.array_equal(q.vlosMu, MUS[:, None] * st.vz[None, :]) and q.Quv.shape == (3, p.Nlambda, 3)
    # the reference's 1D convention for the azimuth
    assert np.array_equal(so.mux, np.sqrt(1.0 - MUS ** 2)) and np.array_equal(so.muy, np.zeros(3))
    for name in ('B', 'gammaB', 'chiB'):
        a, b = getattr(st, name), getattr(so, name)
        assert np.array_equal(a, b) and not np.shares_memory(a, b), name
    assert len(so.lines) == len(st.lines) > 0
    for L, M in zip(st.lines, so.lines):
        assert (L.atom, L.trans) == (M.atom, M.trans)
        for name in ('alpha', 'shift', 'strength'):
            a, b = getattr(L, name), getattr(M, name)
            assert np.array_equal(a, b) and not np.shares_memory(a, b), name
        t = q.atoms[M.atom].trans[M.trans]
        for name in M.PROFILES:
            a = getattr(M, name)
            assert a.shape == (t.Nlambda, 3, 2, p.Nspace) and not np.any(a), name
    # the projections: the fixture's (Atmosphere::update_projections of the core) within the bound of
    # test_components_and_projections_match_reference, exact at mu = 1
    for key, case, mus, mux, muy in src.entries():
        o = src.observer(sc.fixture_problem(matrix, case), mus, mux, muy).stokes
        for name in ('cosGamma', 'cos2chi', 'sin2chi'):
            ref = golden[f'in/{key}/{name}']
            assert np.max(np.abs(getattr(o, name) - ref)) <= 2.3e-16, (key, name)
            for m in np.flatnonzero(mus == 1.0):
                assert np.array_equal(getattr(o, name)[m], ref[m]), (key, name)
    # an explicit azimuth; the default (stokes=False) carries no Stokes data, as before
    az = src.observer(p, src.AZ_MUS, src.AZ_MUX, src.AZ_MUY).stokes
    assert np.array_equal(az.mux, [0.0]) and np.array_equal(az.muy, [0.8])
    plain = observer_problem(p, MUS)
    assert plain.stokes is None and plain.Quv is None
    with pytest.raises(ValueError):
        observer_problem(observer_problem(p, MUS), MUS, stokes=True)


def numpy_route(prob, mus, mux=None, muy=None, las=None, vz=None):
    """The host route: observer_problem(stokes=True), the profiles of the new directions, the numpy restatement of the core."""
    obs = src.observer(prob, mus, mux, muy, vz=vz)
    models.compute_profiles_host(obs)
    with np.errstate(divide='ignore'):
        stokes_ref.set_polarised_profiles(obs)   # (wmu = 0: wphi is infinite, and never read)
    I, Quv, _, _, _ = stokes_ref.full_stokes(obs, updateJ=False, upOnly=True, las=las)
    return I, Quv


@pytest.mark.parametrize('key,case,mus,mux,muy', src.entries(), ids=[e[0] for e in src.entries()])
def test_numpy_route_against_reference(matrix, golden, key, case, mus, mux, muy):
    prob = sc.fixture_problem(matrix, case)
    if prob.zLowerBc.type == abi.BC_CALLABLE:
        assert np.array_equal(src.lower_bc(prob, len(mus))[sc.MATRIX_ROW], golden[f'in/{key}/lowerBc'])
    las = sc.sampled_wavelengths(prob) if prob.Nspace > 40 else None
    with np.errstate(divide='ignore'):
        I, Quv = numpy_route(prob, mus, mux, muy, las=las)
    sel = slice(None) if las is None else las
    err = src.errors(I, Quv, golden[f'out/{key}/I'][sel], golden[f'out/{key}/Quv'][:, sel], sc.polarised_mask(prob)[sel])
    print(key, err)
    assert err['I'] <= TOL and err['Quv'] <= TOL, (key, err)


# ---- GPU -------------------------------------------------------------------------------------------------------------------

def device_rays(prob, mus=MUS, mux=None, muy=None, **kw):
    from lightweaver_amd.context import Context
    with Context(prob) as ctx:
        return ctx.compute_rays(mus, vz=kw.pop('vz', prob.stokes.vz), lowerBc=kw.pop('lowerBc', src.lower_bc(prob, len(mus))),
                                stokes=True, mux=mux, muy=muy, **kw)


def second_context(prob, mus=MUS, mux=None, muy=None, vz=None):
    """The parent's route on the device: a second Context on the observer problem, its profiles, single_stokes_fs(upOnly)."""
    from lightweaver_amd.context import Context
    obs = src.observer(prob, mus, mux, muy, vz=vz)
    with Context(obs) as c2:
        c2.compute_profiles()
        c2.compute_polarised_profiles()
        c2.single_stokes_fs(updateJ=False, upOnly=True)
    return obs.I.copy(), obs.Quv.copy()


@pytest.mark.gpu
@pytest.mark.parametrize('key,case,mus,mux,muy', src.entries(), ids=[e[0] for e in src.entries()])
def test_device_against_reference(gpu, matrix, golden, key, case, mus, mux, muy):
    prob = sc.fixture_problem(matrix, case)
    got = device_rays(prob, mus, mux, muy)
    assert got.shape == (4, prob.Nlambda, len(mus))
    pol = sc.polarised_mask(prob)
    assert not np.any(got[1:, ~pol]) and np.any(got[1:, pol])   # exact zeros where no polarised line is active
    err = src.errors(got[0], got[1:], golden[f'out/{key}/I'], golden[f'out/{key}/Quv'], pol)
    print(key, err)
    assert err['I'] <= TOL and err['Quv'] <= TOL, (key, err)


@pytest.mark.gpu
@pytest.mark.parametrize('case', MATRIX_CASES)
def test_device_against_second_context(gpu, matrix, case):
    prob = sc.fixture_problem(matrix, case)
    assert not np.any(np.isin(MUS_OFF, prob.muz)), 'the directions must not be quadrature nodes'
    got = device_rays(prob, MUS_OFF)
    Iref, Quvref = second_context(prob, MUS_OFF)
    pol = sc.polarised_mask(prob)
    err = src.errors(got[0], got[1:], Iref, Quvref, pol)
    print(f'{case}: Ns {prob.Nspace}, context rays {prob.Nrays}, {prob.Nlambda * 3} observer rays: {err}')
    assert not np.any(got[1:, ~pol])
    assert err['I'] <= TOL and err['Quv'] <= TOL, (case, err)


@pytest.mark.gpu
def test_at_the_contexts_own_angles(gpu, matrix):
    from lightweaver_amd.context import Context
    prob = sc.fixture_problem(matrix, 'moving82')
    st = prob.stokes
    with Context(prob) as ctx:
        got = ctx.compute_rays(prob.muz, vz=st.vz, stokes=True, mux=st.mux, muy=st.muy)
        ctx.compute_profiles()   # (phi of the lines that are not polarised from the device's H(a, v), as the observer gather forms it)
        ctx.compute_polarised_profiles()
        ctx.single_stokes_fs(updateJ=False, upOnly=True)
    err = src.errors(got[0], got[1:], prob.I, prob.Quv, sc.polarised_mask(prob))
    print('own angles:', err, 'bit-equal' if np.array_equal(got[0], prob.I) and np.array_equal(got[1:], prob.Quv) else 'not bit-equal')
    assert err['I'] <= TOL and err['Quv'] <= TOL, err


@pytest.mark.gpu
def test_context_is_left_alone_and_chunks_are_invisible(gpu, matrix, monkeypatch):
    from lightweaver_amd.context import Context
    knobs = ('LWHIP_STOKES_CHUNK_LA', 'LWHIP_STOKES_BATCH_RAYS')
    for k in knobs:
        monkeypatch.delenv(k, raising=False)

    def run(withRays):
        p = sc.fixture_problem(matrix, 'moving82')
        with Context(p) as ctx:
            ctx.compute_polarised_profiles()
            ctx.single_stokes_fs(updateJ=True, upOnly=False)
            rays = None
            if withRays:
                full = ctx.compute_rays(MUS, vz=p.stokes.vz, stokes=True)
                part = ctx.compute_rays(MUS, laStart=31, laEnd=118, vz=p.stokes.vz, stokes=True)
                rays = (full, part)
            ctx.download(abi.I | abi.STOKES | abi.PROFILES | abi.J)
            state = dict(I=p.I.copy(), Quv=p.Quv.copy(), J=p.J.copy())
            for i, L in enumerate(p.stokes.lines):
                t = p.atoms[L.atom].trans[L.trans]
                state[f'phi{i}'], state[f'wphi{i}'] = t.phi.copy(), t.wphi.copy()
                for name in L.PROFILES:
                    state[f'{name}{i}'] = getattr(L, name).copy()
            ctx.single_stokes_fs(updateJ=False, upOnly=True)
            state['I2'], state['Quv2'] = p.I.copy(), p.Quv.copy()
        return state, rays

    a, _ = run(False)
    b, (full, part) = run(True)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert part.shape == (4, 118 - 31, 3) and np.array_equal(part, full[:, 31:118])
    # the chunk knobs (LWHIP_DEBUG is set by the suite) do not change a bit
    p = sc.fixture_problem(matrix, 'moving82')
    with Context(p) as ctx:
        for knob, value in (('LWHIP_STOKES_BATCH_RAYS', '64'), ('LWHIP_STOKES_CHUNK_LA', '7')):
            monkeypatch.setenv(knob, value)
            assert np.array_equal(ctx.compute_rays(MUS, vz=p.stokes.vz, stokes=True), full), knob
            assert np.array_equal(ctx.compute_rays(MUS, laStart=31, laEnd=118, vz=p.stokes.vz, stokes=True), part), knob
            monkeypatch.delenv(knob)
        # squeeze: a scalar direction drops the Nmu axis
        one = ctx.compute_rays(0.6, vz=p.stokes.vz, stokes=True)
        assert one.shape == (4, p.Nlambda) and np.array_equal(one, full[:, :, 1])
        with pytest.raises(ValueError):
            ctx.compute_rays(MUS, stokes=True, depthData=True)


@pytest.mark.gpu
def test_batch_equals_single_contexts(gpu):
    from lightweaver_amd.batch import ColumnBatch
    from lightweaver_amd.context import Context
    probs = zeeman.stokes_columns(8, **SMALL)
    vz = [p.stokes.vz for p in probs]
    singles = []
    for p in zeeman.stokes_columns(8, **SMALL):
        with Context(p) as ctx:
            singles.append(ctx.compute_rays(MUS, vz=p.stokes.vz, stokes=True))
    with ColumnBatch(probs) as b:
        assert b._batch is not None
        got = b.compute_rays(MUS, vz=vz, stokes=True)
        sub = b.compute_rays(MUS, laStart=10, laEnd=75, vz=vz, stokes=True)
    with ColumnBatch(zeeman.stokes_columns(8, **SMALL), fused=False) as u:
        assert u._batch is None
        unfused = u.compute_rays(MUS, vz=vz, stokes=True)
    assert got.shape == (8, 4, probs[0].Nlambda, 3)
    for i, s in enumerate(singles):
        assert np.array_equal(got[i], s) and np.array_equal(unfused[i], s) and np.array_equal(sub[i], s[:, 10:75]), i
    assert not np.array_equal(got[0], got[1])
    # two columns against the route through a second context
    for i in (0, 5):
        p = zeeman.stokes_columns(i + 1, **SMALL)[i]
        Iref, Quvref = second_context(p, MUS)
        err = src.errors(got[i, 0], got[i, 1:], Iref, Quvref, sc.polarised_mask(p))
        print(f'batch column {i} vs second context: {err}')
        assert err['I'] <= TOL and err['Quv'] <= TOL, (i, err)


@pytest.mark.gpu
def test_large_batch_c4_size(gpu):
    """64 columns at the C4 size (2 908 wavelengths x 82 depths), mu = 1, in one call: 1.4 GB of rows, so the call is cut into
    chunks of columns under the batch's 1 GiB cap.  (With 512 columns the test passed as well but took 7.7 s, most of it
    building the problems on the host; 64 keep it to about a second.)"""
    from lightweaver_amd.batch import ColumnBatch
    from lightweaver_amd.context import Context
    NCOL = 64
    probs = zeeman.stokes_columns(NCOL)
    assert 2800 <= probs[0].Nlambda <= 3200
    with ColumnBatch(probs) as b:
        assert b._batch is not None
        got = b.compute_rays(1.0, stokes=True)
    assert got.shape == (NCOL, 4, probs[0].Nlambda, 1) and np.all(np.isfinite(got)) and np.all(got[:, 0] > 0.0)
    assert not np.array_equal(got[0], got[NCOL - 1])
    for i in (0, 37, NCOL - 1):
        with Context(probs[i].copy()) as ctx:
            assert np.array_equal(ctx.compute_rays(1.0, squeeze=False, stokes=True), got[i]), i


@pytest.mark.gpu
def test_the_physics_shows(gpu, matrix):
    """CPU figures of the numpy route: max |V| / I >= 0.17 at each direction of moving82; turning the azimuth at mu = 0.6
    changes Quv by 3.0e-2 of I and I by 4.6e-3.  Each asserted at >= 1e-3, six orders above the tolerance."""
    prob = sc.fixture_problem(matrix, 'moving82')
    pol = sc.polarised_mask(prob)
    got = device_rays(prob, MUS)
    vOverI = np.max(np.abs(got[3]) / got[0], axis=0)
    print('max |V| / I per direction:', vOverI)
    assert np.all(vOverI >= 1e-3)
    a = device_rays(prob, [0.6], [0.8], [0.0])
    b = device_rays(prob, [0.6], [0.0], [0.8])
    assert np.array_equal(a, got[:, :, 1:2])   # (the default azimuth is mux = sqrt(1 - mu^2), muy = 0)
    dQuv = np.max((np.abs(a[1:] - b[1:]) / a[0][None])[:, pol])
    dI = np.max(np.abs(a[0] / b[0] - 1.0))
    print(f'azimuth turned by 90 degrees at mu = 0.6: dQuv / I {dQuv:.3e}, dI / I {dI:.3e}')
    assert dQuv >= 1e-3 and dI >= 1e-3
    c = device_rays(prob, MUS, vz=-prob.stokes.vz)
    dv = np.max(np.abs(c[0] / got[0] - 1.0))
    print(f'vz -> -vz: dI / I {dv:.3e}')
    assert dv >= 1e-3


@pytest.mark.gpu
def test_refusals_launch_nothing(gpu, matrix):
    from lightweaver_amd.batch import ColumnBatch
    from lightweaver_amd.context import Context
    from helpers import load_fixture
    FILL = -7.0

    def request(ctx, mus=MUS, laStart=0, laEnd=0, lowerBc=None, **kw):
        q, out, keep = ctx._stokes_rays_request(mus, laStart, laEnd, None, lowerBc, None, None)
        for k, v in kw.items():
            setattr(q.rays if hasattr(abi.lwhip_rays, k) else q, k, v)
        out[...] = FILL
        return q, out, keep

    def call(ctx, *a, **kw):
        q, out, keep = request(ctx, *a, **kw)
        st = ctx.lib.lwhip_compute_stokes_rays(ctx._h, C.byref(q))
        return st, ctx.lib.lwhip_last_error(), bool(np.all(out == FILL))

    p = sc.fixture_problem(matrix, 'n5')
    with Context(p) as ctx:
        lib = ctx.lib
        st, msg, clean = call(ctx)
        assert st == abi.OK and not clean
        # a null projection array, a null Quv, a depth array present
        for name in ('cosGamma', 'cos2chi', 'sin2chi'):
            st, msg, clean = call(ctx, **{name: None})
            assert st == abi.ERR_INVALID and b'cosGamma, cos2chi and sin2chi' in msg and clean, name
        st, msg, clean = call(ctx, Quv=None)
        assert st == abi.ERR_INVALID and b'Quv' in msg and clean
        depth = np.zeros((p.Nlambda, 3, p.Nspace))
        q, out, keep = request(ctx)
        for name in ('depthChi', 'depthEta', 'depthI'):
            setattr(q.rays, name, depth.ctypes.data_as(abi.f64p))
        assert lib.lwhip_compute_stokes_rays(ctx._h, C.byref(q)) == abi.ERR_INVALID and b'depth' in lib.lwhip_last_error()
        assert np.all(out == FILL) and not np.any(depth)
        # direction cosines outside (0, 1] (through the ABI: the Python layer refuses them before the call)
        for bad in (np.array([0.5, 1.25, 1.0]), np.array([0.0, 0.5, 1.0])):
            st, msg, clean = call(ctx, muz=bad.ctypes.data_as(abi.f64p))
            assert st == abi.ERR_INVALID and b'(0, 1]' in msg and clean
        # Nmu over the cap
        st, msg, clean = call(ctx, np.linspace(0.1, 1.0, abi.RAYS_MAX_MU + 1))
        assert st == abi.ERR_UNSUPPORTED and b'LWHIP_RAYS_MAX_MU' in msg and clean
        # a range outside the rows
        for la0, la1 in ((10, p.Nlambda + 1), (40, 40), (50, 20), (-3, 10)):
            st, msg, clean = call(ctx, MUS[:1], laStart=la0, laEnd=la1)
            assert st == abi.ERR_INVALID and b'wavelength range' in msg and clean, (la0, la1)
        assert lib.lwhip_compute_stokes_rays(ctx._h, None) == abi.ERR_INVALID
        assert lib.lwhip_compute_stokes_rays(None, C.byref(q)) == abi.ERR_INVALID
    # no Stokes data
    plain, _ = load_fixture('falc_h_ca_small')
    with Context(plain) as ctx:
        q = abi.lwhip_stokes_rays()
        assert ctx.lib.lwhip_compute_stokes_rays(ctx._h, C.byref(q)) == abi.ERR_INVALID
        assert b'no Stokes data' in ctx.lib.lwhip_last_error()
    # a CALLABLE lower boundary without data
    pb = sc.fixture_problem(matrix, 'bc_lower_callable')
    with Context(pb) as ctx:
        st, msg, clean = call(ctx)
        assert st == abi.ERR_INVALID and b'CALLABLE' in msg and clean
    # a piecewise_linear_1d context is accepted (the Stokes path ignores the context's solver) and gives the same numbers
    pl = sc.fixture_problem(matrix, 'n5')
    pl.formalSolver = abi.FS_LINEAR_1D
    got = device_rays(pl, MUS_OFF)
    Iref, Quvref = second_context(sc.fixture_problem(matrix, 'n5'), MUS_OFF)
    err = src.errors(got[0], got[1:], Iref, Quvref, sc.polarised_mask(pl))
    assert err['I'] <= TOL and err['Quv'] <= TOL, err
    # a batch: a column that differs, a null request list, a column without Stokes data
    with ColumnBatch(zeeman.stokes_columns(3, **SMALL)) as b:
        lib = b.contexts[0].lib
        reqs = [request(c) for c in b.contexts]
        reqs[1][0].rays.Nmu = 2
        arr = (abi.lwhip_stokes_rays * 3)(*[q for q, _, _ in reqs])
        assert lib.lwhip_batch_compute_stokes_rays(b._batch, arr) == abi.ERR_INVALID and b'column 1' in lib.lwhip_last_error()
        arr[1].rays.Nmu = 3
        arr[2].rays.laEnd = 50
        assert lib.lwhip_batch_compute_stokes_rays(b._batch, arr) == abi.ERR_INVALID and b'column 2' in lib.lwhip_last_error()
        arr[2].rays.laEnd = reqs[2][0].rays.laEnd
        arr[2].sin2chi = None
        assert lib.lwhip_batch_compute_stokes_rays(b._batch, arr) == abi.ERR_INVALID and b'column 2' in lib.lwhip_last_error()
        assert lib.lwhip_batch_compute_stokes_rays(b._batch, None) == abi.ERR_INVALID
        assert lib.lwhip_batch_compute_stokes_rays(None, arr) == abi.ERR_INVALID
        assert all(np.all(o == FILL) for _, o, _ in reqs)
