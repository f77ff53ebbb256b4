"""Full Stokes for 1.5D column batches: lwhip_batch_compute_polarised_profiles, lwhip_batch_full_stokes_fs and
ColumnBatch.compute_polarised_profiles / single_stokes_fs.

CPU: the two symbols are exported and bound, both refuse without a device, harness.zeeman.stokes_columns is seeded.
GPU: each column of a fused batch against the same column on its own Context (the device functions are shared, so the
results are the same bits), against the numpy restatement of the march, the batched profiles, chunking, column order,
the refusals, and a 512-column batch of the C4 size."""
import ctypes as C
import os

import numpy as np
import pytest

from lightweaver_amd import _abi as abi
from lightweaver_amd.harness import zeeman
from lightweaver_amd.model import StokesData

from tests import stokes_ref

NEW_SYMBOLS = ('lwhip_batch_compute_polarised_profiles', 'lwhip_batch_full_stokes_fs')


def test_batch_stokes_symbols_exported_and_bound(hip_lib):
    names = [s[0] for s in abi.SYMBOLS]
    for name in NEW_SYMBOLS:
        assert name in names, name
        fn = getattr(hip_lib, name)
        assert fn.restype is C.c_int and fn.argtypes[0] is C.c_void_p, name
    assert list(hip_lib.lwhip_batch_full_stokes_fs.argtypes[1:]) == [C.c_int, C.c_int, C.POINTER(abi.lwhip_iter_result)]


def test_batch_stokes_refuses_without_device(hip_lib):
    if hip_lib.lwhip_device_count() > 0:
        pytest.skip('a device is present: the refusal is the no-device path')
    assert hip_lib.lwhip_batch_compute_polarised_profiles(None) == abi.ERR_DEVICE
    assert b'device' in hip_lib.lwhip_last_error()
    res = (abi.lwhip_iter_result * 2)()
    assert hip_lib.lwhip_batch_full_stokes_fs(None, 1, 1, res) == abi.ERR_DEVICE
    assert b'device' in hip_lib.lwhip_last_error()


def test_stokes_columns_are_seeded():
    a = zeeman.stokes_columns(3, Nrays=3, lineScale=0.2)
    b = zeeman.stokes_columns(3, Nrays=3, lineScale=0.2)
    for p, q in zip(a, b):
        for name in ('B', 'gammaB', 'chiB', 'cosGamma', 'cos2chi', 'sin2chi'):
            assert np.array_equal(getattr(p.stokes, name), getattr(q.stokes, name)), name
        assert np.array_equal(p.temperature, q.temperature)
        assert [(L.atom, L.trans, len(L.alpha)) for L in p.stokes.lines] == [(L.atom, L.trans, len(L.alpha))
                                                                              for L in q.stokes.lines]
    assert len(a[0].stokes.lines) == 5
    # every column its own field and atmosphere, the same wavelength grid and polarised lines
    for i in range(3):
        for j in range(i + 1, 3):
            assert not np.allclose(a[i].stokes.B, a[j].stokes.B)
            assert not np.allclose(a[i].stokes.chiB, a[j].stokes.chiB)
            assert not np.array_equal(a[i].temperature, a[j].temperature)
            assert np.array_equal(a[i].wavelength, a[j].wavelength)
    c = zeeman.stokes_columns(1, Nrays=3, lineScale=0.2, seed0=99)
    assert not np.array_equal(c[0].stokes.B, a[0].stokes.B)
    assert np.all(a[0].stokes.B > 0.0)


# ---- GPU -------------------------------------------------------------------------------------------------------------

SMALL = dict(Nrays=3, lineScale=0.3)


def _polarised_mask(prob):
    m = np.zeros(prob.Nlambda, dtype=bool)
    for L in prob.stokes.lines:
        t = prob.atoms[L.atom].trans[L.trans]
        m[t.Nblue:t.Nred] = True
    return m


def _with_j20(probs):
    for p in probs:
        rng = np.random.default_rng(int(p.temperature[0]) % 1000)
        p.stokes.J20 = (0.05 * rng.standard_normal((p.Nlambda, p.Nspace))) * p.J
    return probs


def _single(p, variants):
    """Each variant (updateJ, upOnly) on the column's own Context; I, Quv, J, J20 and the update after each."""
    from lightweaver_amd.context import Context
    out = []
    with Context(p) as ctx:
        ctx.compute_profiles(deviceResident=True)
        # (downloaded: the calls below upload the host's Stokes data, profiles included, as Context.single_stokes_fs does)
        ctx.compute_polarised_profiles(deviceResident=False)
        for updateJ, upOnly in variants:
            r = ctx.single_stokes_fs(updateJ=updateJ, upOnly=upOnly, J20=p.stokes.J20)
            out.append(_snap(p, r))
    return out


def _snap(p, r):
    return dict(I=p.I.copy(), Quv=p.Quv.copy(), J=p.J.copy(), J20=None if p.stokes.J20 is None else p.stokes.J20.copy(),
                dJMax=r.dJMax, dJMaxIdx=r.dJMaxIdx)


def _batched(probs, variants, **kw):
    from lightweaver_amd.batch import ColumnBatch
    out = []
    with ColumnBatch(probs, **kw) as b:
        assert b._batch is not None
        b.compute_polarised_profiles(deviceResident=False)
        for updateJ, upOnly in variants:
            ups = b.single_stokes_fs(updateJ=updateJ, upOnly=upOnly)
            assert len(ups) == len(probs)
            out.append([_snap(p, r) for p, r in zip(probs, ups)])
    return out


def _assert_same(a, b, what):
    for k in ('I', 'Quv', 'J', 'J20'):
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, (what, k)
            continue
        assert np.array_equal(a[k], b[k]), (what, k, float(np.max(np.abs(a[k] - b[k]))))
    assert a['dJMax'] == b['dJMax'] and a['dJMaxIdx'] == b['dJMaxIdx'], what


VARIANTS = [(False, True), (False, False), (True, False), (True, True)]


@pytest.mark.gpu
def test_batch_matches_single_context(gpu):
    probs = zeeman.stokes_columns(8, **SMALL)
    singles = [_single(p, VARIANTS) for p in [q.copy() for q in probs]]
    got = _batched(probs, VARIANTS)
    for v, (updateJ, upOnly) in enumerate(VARIANTS):
        for i in range(len(probs)):
            _assert_same(got[v][i], singles[i][v], (updateJ, upOnly, i))
    # the columns differ, and the polarised wavelengths carry Q, U, V
    pol = _polarised_mask(probs[0])
    assert not np.array_equal(got[0][0]['Quv'], got[0][1]['Quv'])
    assert np.abs(got[0][0]['Quv'][:, pol]).max() > 0.0 and np.all(got[0][0]['Quv'][:, ~pol] == 0.0)
    assert got[2][0]['dJMax'] > 0.0


@pytest.mark.gpu
@pytest.mark.parametrize('Ns', (3, 24, 130))
def test_batch_other_depth_counts(gpu, Ns):
    """The batch kernels at other depth counts than FAL-C's 82: the first step, the last-but-one step and the last point of
    the marches fall onto each other at 3 points.  The single context is held to the reference at these depths by
    tests/test_stokes.py::test_matrix_against_reference."""
    probs = zeeman.stokes_columns(3, Nspace=Ns, **SMALL)
    assert all(p.Nspace == Ns for p in probs)
    singles = [_single(p, VARIANTS) for p in [q.copy() for q in probs]]
    got = _batched(probs, VARIANTS)
    for v, (updateJ, upOnly) in enumerate(VARIANTS):
        for i in range(len(probs)):
            _assert_same(got[v][i], singles[i][v], (Ns, updateJ, upOnly, i))
    pol = _polarised_mask(probs[0])
    assert np.abs(got[0][0]['Quv'][:, pol]).max() > 0.0 and got[2][0]['dJMax'] > 0.0


@pytest.mark.gpu
def test_batch_with_j20_matches_single_context(gpu):
    probs = _with_j20(zeeman.stokes_columns(8, **SMALL))
    probs[3].stokes.J20 = None   # (a column without J20 in the same batch: an ordinary call for it)
    variants = [(True, False), (False, True)]
    singles = [_single(p, variants) for p in [q.copy() for q in probs]]
    got = _batched(probs, variants)
    for v in range(len(variants)):
        for i in range(len(probs)):
            _assert_same(got[v][i], singles[i][v], (variants[v], i))
    assert got[0][0]['J20'] is not None and np.abs(got[0][0]['J20']).max() > 0.0


@pytest.mark.gpu
def test_batch_against_numpy_march(gpu):
    from lightweaver_amd.batch import ColumnBatch
    probs = zeeman.stokes_columns(4, **SMALL)
    with ColumnBatch(probs) as b:
        b.compute_polarised_profiles(deviceResident=False)   # (the host needs the profiles for the restatement)
        b.single_stokes_fs(updateJ=False, upOnly=True)
    pol = _polarised_mask(probs[0])
    rng = np.random.default_rng(11)
    for p in (probs[0], probs[3]):
        las = np.sort(np.concatenate([rng.choice(np.flatnonzero(pol), 24, replace=False),
                                      rng.choice(np.flatnonzero(~pol), 8, replace=False)]))
        I, Quv, *_ = stokes_ref.full_stokes(p, updateJ=False, upOnly=True, las=las)
        assert np.max(np.abs(p.I[las] / I - 1.0)) <= 1e-9
        assert np.max(np.abs(p.Quv[:, las] - Quv) / I[None]) <= 1e-9


PROFILE_NAMES = ('phiQ', 'phiU', 'phiV', 'psiQ', 'psiU', 'psiV')


@pytest.mark.gpu
def test_batched_polarised_profiles(gpu):
    from lightweaver_amd.batch import ColumnBatch
    from lightweaver_amd.context import Context
    probs = zeeman.stokes_columns(5, **SMALL)
    ref = [p.copy() for p in probs]
    for p in ref:
        with Context(p) as ctx:
            ctx.compute_profiles(deviceResident=True)
            ctx.compute_polarised_profiles(deviceResident=False)
    with ColumnBatch(probs) as b:
        b.compute_polarised_profiles(deviceResident=False)
        for p, q in zip(probs, ref):
            for L, M in zip(p.stokes.lines, q.stokes.lines):
                t, u = p.atoms[L.atom].trans[L.trans], q.atoms[M.atom].trans[M.trans]
                assert np.array_equal(t.phi, u.phi) and np.array_equal(t.wphi, u.wphi)
                for name in PROFILE_NAMES:
                    assert np.array_equal(getattr(L, name), getattr(M, name)), name
                assert np.abs(L.phiV).max() > 0.0
        # a column's atmosphere uploaded again: its plain profiles are made again BEFORE the polarised ones
        L = probs[2].stokes.lines[0]
        t = probs[2].atoms[L.atom].trans[L.trans]
        polPhi = t.phi.copy()
        b.contexts[2].upload(abi.ATMOS)
        b.compute_polarised_profiles(deviceResident=True)
        b.single_stokes_fs(upOnly=True)
        t.phi[...] = 0.0
        b.contexts[2].download(abi.PROFILES)
        assert np.array_equal(t.phi, polPhi)


@pytest.mark.gpu
def test_batch_chunks_order_and_single_column(gpu):
    variants = [(False, True), (True, False)]
    probs = zeeman.stokes_columns(6, **SMALL)
    base = _batched([p.copy() for p in probs], variants)
    Nla, Nr = probs[0].Nlambda, probs[0].Nrays
    # chunks of two whole columns, then chunks of part of one column's wavelengths
    for rays in (2 * 2 * Nla * Nr + 64, 5 * 64):
        os.environ['LWHIP_STOKES_BATCH_RAYS'] = str(rays)
        try:
            got = _batched([p.copy() for p in probs], variants)
        finally:
            del os.environ['LWHIP_STOKES_BATCH_RAYS']
        for v in range(len(variants)):
            for i in range(len(probs)):
                _assert_same(got[v][i], base[v][i], ('chunked', rays, v, i))
    perm = [4, 0, 5, 2, 1, 3]
    got = _batched([probs[j].copy() for j in perm], variants)
    for v in range(len(variants)):
        for i, j in enumerate(perm):
            _assert_same(got[v][i], base[v][j], ('permuted', v, i))
    one = _batched([probs[1].copy()], variants)
    single = _single(probs[1].copy(), variants)
    for v in range(len(variants)):
        _assert_same(one[v][0], single[v], ('one column', v))


@pytest.mark.gpu
def test_member_context_alone_between_batched_calls(gpu):
    """A column of a batch called alone through its own Context between two batched calls: the context's own scratch next
    to the batch's.  All three results of that column are the same bits."""
    from lightweaver_amd.batch import ColumnBatch
    probs = zeeman.stokes_columns(3, **SMALL)
    J0 = [p.J.copy() for p in probs]
    with ColumnBatch(probs) as b:
        assert b._batch is not None
        b.compute_polarised_profiles(deviceResident=False)
        for updateJ, upOnly in VARIANTS:
            got = []
            for alone in (False, True, False):
                for p, j in zip(probs, J0):   # (every call uploads and reads the same J)
                    p.J[...] = j
                if alone:
                    r = b.contexts[1].single_stokes_fs(updateJ=updateJ, upOnly=upOnly)
                else:
                    r = b.single_stokes_fs(updateJ=updateJ, upOnly=upOnly)[1]
                got.append(_snap(probs[1], r))
            _assert_same(got[1], got[0], ('alone', updateJ, upOnly))
            _assert_same(got[2], got[0], ('batched again', updateJ, upOnly))
            assert np.abs(got[0]['Quv']).max() > 0.0 and (not updateJ or got[0]['dJMax'] > 0.0)


@pytest.mark.gpu
def test_batch_refusals_launch_nothing(gpu):
    from lightweaver_amd.batch import ColumnBatch
    from lightweaver_amd.context import LwHipError
    probs = zeeman.stokes_columns(3, **SMALL)
    with ColumnBatch(probs) as b:
        lib = b.contexts[0].lib
        b.compute_polarised_profiles(deviceResident=False)
        b.single_stokes_fs(upOnly=True)
        before = [(p.I.copy(), p.Quv.copy()) for p in probs]
        assert all(np.abs(Q).max() > 0.0 for _, Q in before)
        # J changed on the device: a launch with updateJ would change I, Quv and J
        J2 = [2.0 * p.J for p in probs]
        for c, j in zip(b.contexts, J2):
            c.prob.J[...] = j
            c.upload(abi.J)

        def unchanged(cols):
            for i in cols:
                p, c = probs[i], b.contexts[i]
                p.I[...] = np.nan
                p.Quv[...] = np.nan
                p.J[...] = np.nan
                c.download(abi.I | abi.J | abi.STOKES)
                assert np.array_equal(p.I, before[i][0]) and np.array_equal(p.Quv, before[i][1]), i
                assert np.array_equal(p.J, J2[i]), i

        # a column without Stokes data
        assert lib.lwhip_set_stokes(b.contexts[1]._h, None) == abi.OK
        b.contexts[1]._stokes_key = None
        res = (abi.lwhip_iter_result * 3)()
        assert lib.lwhip_batch_full_stokes_fs(b._batch, 1, 0, res) == abi.ERR_INVALID
        assert b'column 1' in lib.lwhip_last_error() and b'Stokes data' in lib.lwhip_last_error()
        assert lib.lwhip_batch_compute_polarised_profiles(b._batch) == abi.ERR_INVALID
        unchanged([0, 2])
        # a column with another polarised-line list
        p1 = probs[1]
        p1.set_stokes(StokesData(B=p1.stokes.B, gammaB=p1.stokes.gammaB, chiB=p1.stokes.chiB, mux=p1.stokes.mux,
                                 muy=p1.stokes.muy, lines=zeeman.polarise_lines(p1, 1, lines=[0, 1])))
        b.contexts[1]._stokes_attach()
        assert lib.lwhip_batch_full_stokes_fs(b._batch, 1, 0, res) == abi.ERR_INVALID
        assert b'column 1' in lib.lwhip_last_error() and b'polarised lines' in lib.lwhip_last_error()
        assert lib.lwhip_batch_compute_polarised_profiles(b._batch) == abi.ERR_INVALID
        with pytest.raises(LwHipError):
            b.single_stokes_fs(updateJ=True, upOnly=False, deviceResident=True)
        unchanged([0, 2])


@pytest.mark.gpu
def test_large_batch_c4_size(gpu):
    from lightweaver_amd.batch import ColumnBatch
    probs = zeeman.stokes_columns(512, Nrays=5, lineScale=3.1)
    pol = _polarised_mask(probs[0])
    assert 2800 <= probs[0].Nlambda <= 3200 and pol.sum() > 0 and (~pol).sum() > 0
    with ColumnBatch(probs) as b:
        b.compute_polarised_profiles()
        assert b.single_stokes_fs(upOnly=True, deviceResident=True, sync_host=False) is None
        nz = 0
        for c, p in zip(b.contexts, probs):
            c.download(abi.I | abi.STOKES)
            assert np.all(np.isfinite(p.I)) and np.all(np.isfinite(p.Quv)) and np.all(p.I > 0.0)
            assert np.all(p.Quv[:, ~pol] == 0.0)
            nz += int(np.abs(p.Quv[:, pol]).max() > 0.0)
        assert nz == len(probs)
    assert not np.array_equal(probs[0].Quv, probs[511].Quv)
