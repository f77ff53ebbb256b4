"""PRD sub-iterations of a column batch (lwhip_batch_redistribute_prd, ColumnBatch.prd_redistribute, iterate_to_convergence(prd=True)):
every active column gets what a lone Context's redistribute_prd gives it -- its own number of sub-iterations, its own state at
its own stop -- against the CPU oracle column by column and against lone Contexts on the same inputs.

Columns: models.falc_h_ca(Nrays=3, lineScale=0.3, prd=True, atmos=...), the base problem of test_lanesweep_matrix (298
wavelengths, Ca II H & K in PRD).  Bounds are the project's own: 1e-7 on state against the oracle for a fused batch
(test_fused_batch), 1e-10 between two layouts of one problem with a PRD sub-iteration in between
(test_lane_sweep_ray_split_vs_oracle; here: batch against lone Context), dRho rtol 1e-5 / atol 1e-12 and dJPrdMax rtol 1e-7
(test_prd.py), TOL_CONVERGED after iteration.  Every oracle result is computed once and only read."""
import ctypes as C
import functools

import numpy as np
import pytest

from helpers import TOL_CONVERGED, rel_err
from lightweaver_amd import _abi as abi
from lightweaver_amd.batch import ColumnBatch
from lightweaver_amd.harness import models
from lightweaver_amd.iterate import iterate_ctx_se
from oracle.bindings import OracleContext
from test_batch_converge import OracleBatch
from test_hip_parity import compare_problems
from test_iterate import OracleLoopContext

STATE = abi.J | abi.I | abi.RATES | abi.RHOPRD | abi.POPS
FILL, IFILL = -7.0, -7

# ---- the stop tests: three columns whose sub-iteration maxima differ, tolerances between them -------------------------------
STOP_SEEDS = (5, 6, 7)
STOP_TOLS = {0.25: (2, 3, 3), 0.15: (3, 4, 3), 0.07: (4, 5, 4), 0.03: (6, 6, 5)}
MAXIT = 7
# ---- the loop tests (seeds 101, 104, 105 come within 1 % of a tolerance and are left out) -----------------------------------
LOOP_SEEDS = (100, 102, 103, 107, 106)
JTOL, PTOL, NSCATTER, NMAX = 1e-1, 6e-2, 3, 60
KW = dict(Nscatter=NSCATTER, NmaxIter=NMAX, JTol=JTOL, popsTol=PTOL, prd=True)


def prd_column(atmos):
    return models.falc_h_ca(Nrays=3, lineScale=0.3, prd=True, atmos=atmos)


@functools.lru_cache(maxsize=None)
def hot_column(seed):
    """FAL-C at 82 depths, temperatures perturbed by 30 %.  Built once, only ever copied."""
    return prd_column(models.perturbed(models.falc82(), seed, dT=0.3))


def prd_lines(p):
    return [t for a in p.atoms for t in a.trans if t.rhoPrd is not None]


def frozen(u):
    """An oracle PRD update as read-only arrays."""
    out = dict(NprdSubIter=int(u['NprdSubIter']))
    for k in ('dRho', 'dRhoMaxIdx', 'dJPrdMax', 'dJPrdMaxIdx'):
        out[k] = np.array(u[k])
        out[k].setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle_stop(seed, tol):
    """One formal solution, then redistribute_prd(MAXIT, tol) on the oracle: (problem at the stop, update)."""
    q = hot_column(seed).copy()
    with OracleContext(q) as oc:
        q.gamma_prefill()
        oc.formal_sol_gamma_matrices()
        u = frozen(oc.redistribute_prd(MAXIT, tol))
    return q, u


def maxima(seed):
    q, u = oracle_stop(seed, 0.0)
    assert u['NprdSubIter'] == MAXIT
    return np.max(np.asarray(u['dRho']).reshape(MAXIT, -1), axis=1)


def assert_state(tag, got, want, tol, what=('J', 'I', 'R')):
    """J, I, the rates and rho of the PRD lines of `got` against `want`; prints the worst relative error of each."""
    worst = compare_problems(got, want, tol=tol, what=what)
    la, lb = prd_lines(got), prd_lines(want)
    assert len(la) == len(lb) == 2
    worst['rhoPrd'] = max(rel_err(a.rhoPrd, b.rhoPrd) for a, b in zip(la, lb))
    print(tag, {k: float(f'{v:.3g}') for k, v in worst.items()})
    assert worst['rhoPrd'] <= tol, (tag, worst)


def assert_update(tag, up, ref):
    """A column's IterationUpdate against the oracle's update: counts and indices equal, values to test_prd.py's bounds."""
    n = ref['NprdSubIter']
    print(tag, 'NprdSubIter', up.NprdSubIter, n, 'dRho', np.asarray(up.dRho).tolist(), 'dJPrdMax', np.asarray(up.dJPrdMax).tolist())
    assert up.NprdSubIter == n, tag
    assert up.dRho.shape == (n, 2) and up.dRhoMaxIdx.shape == (n, 2) and up.dJPrdMax.shape == (n,), tag
    assert np.allclose(up.dRho, np.asarray(ref['dRho']).reshape(-1, 2)[:n], rtol=1e-5, atol=1e-12), tag
    assert np.array_equal(up.dRhoMaxIdx, np.asarray(ref['dRhoMaxIdx']).reshape(-1, 2)[:n]), tag
    assert np.allclose(up.dJPrdMax, np.asarray(ref['dJPrdMax'])[:n], rtol=1e-7, atol=1e-12), tag
    assert up.dJMax == up.dJPrdMax[n - 1] and up.dJMaxIdx == up.dJPrdMaxIdx[n - 1], tag


# ---- 0. CPU: the result block of the new entry point as the header lays it out ---------------------------------------------------
def test_result_struct_layout_matches_header(tmp_path, monkeypatch):
    import test_abi
    monkeypatch.setattr(test_abi, 'STRUCTS', [abi.lwhip_batch_prd_result])
    test_abi.test_struct_layout_matches_header(tmp_path)
    assert C.sizeof(abi.lwhip_batch_prd_result) == 48


# ---- 1. CPU: the oracle precondition of the stop tests ------------------------------------------------------------------------
def test_oracle_stops_spread_and_are_not_fragile():
    for s in STOP_SEEDS:
        m = maxima(s)
        print('seed', s, 'maxima', m.tolist())
        assert np.all(m[1:] < m[:-1]), (s, m)
        for tol in STOP_TOLS:
            assert not np.any((m > 0.99 * tol) & (m < 1.01 * tol)), (s, tol, m)
    for tol, want in STOP_TOLS.items():
        stops = tuple(oracle_stop(s, tol)[1]['NprdSubIter'] for s in STOP_SEEDS)
        # (the first sub-iteration below the tolerance, from the maxima of the unstopped run)
        assert stops == tuple(int(np.argmax(maxima(s) < tol)) + 1 for s in STOP_SEEDS), (tol, stops)
        assert stops == want, (tol, stops)
        assert len(set(stops)) >= 2, (tol, stops)


# ---- 2. CPU: iterate_to_convergence(prd=True) on oracle columns ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_loop(seed):
    """iterate_ctx_se(prd=True) on the oracle for one column, every iteration's numbers kept: the stop iteration, the trace of
    (dJMax, max dPops, the PRD pass's dJMax) and the state at the stop.  Computed once and never modified."""
    q = hot_column(seed).copy()
    oc = OracleLoopContext(q)
    trace, stop = [], None
    for it in range(NMAX):
        Ju = oc.formal_sol_gamma_matrices()
        if it < NSCATTER:
            continue
        Pu = oc.stat_equil()
        Ru = oc.prd_redistribute(maxIter=3, tol=1e-2)
        trace.append((it, Ju.dJMax, max(Pu.dPops), Ru.dJMax))
        if max(Ju.dJMax, Ru.dJMax) < JTOL and max(Pu.dPops) < PTOL:
            stop = it
            break
    assert stop is not None, seed
    return dict(stop=stop, trace=trace, q=q)


def test_iterate_to_convergence_prd_on_oracle_columns():
    want = [oracle_loop(s)['stop'] for s in LOOP_SEEDS]
    print('oracle stop iterations', dict(zip(LOOP_SEEDS, want)))
    assert len(set(want)) >= 3
    # no iteration at which one number is within 1 % of its tolerance while the others are below 1.01 x theirs: the device's
    # 1e-6-level differences then cannot move a stop iteration (test_oracle_traces_spread_and_are_not_fragile)
    for s in LOOP_SEEDS:
        for it, dJ, dP, dJPrd in oracle_loop(s)['trace']:
            nums = ((dJ, JTOL), (dP, PTOL), (dJPrd, JTOL))
            near = any(0.99 * t < x < 1.01 * t for x, t in nums) and all(x < 1.01 * t for x, t in nums)
            assert not near, (s, it, dJ, dP, dJPrd)
    # the traces are iterate_ctx_se's own
    assert iterate_ctx_se(OracleLoopContext(hot_column(LOOP_SEEDS[1]).copy()), **KW) == want[1]
    probs = [hot_column(s).copy() for s in LOOP_SEEDS]
    batch = OracleBatch(probs)
    seen = []
    res = batch.iterate_to_convergence(callback=lambda it, J, P, act, R: seen.append((it, list(act), R)), **KW)
    assert res.iterations == want and res.converged == [True] * len(LOOP_SEEDS)
    assert batch.active == list(range(len(LOOP_SEEDS)))
    for s, p, fin in zip(LOOP_SEEDS, probs, res.final):
        q = oracle_loop(s)['q']
        assert len(fin) == 3 and fin[2].NprdSubIter >= 1 and fin[2].dJMax == oracle_loop(s)['trace'][-1][3]
        # a retired column stays at its own stop iteration's state (the oracle is deterministic: the same bits)
        assert np.array_equal(p.J, q.J) and all(np.array_equal(a.n, b.n) for a, b in zip(p.atoms, q.atoms))
        assert all(np.array_equal(a.rhoPrd, b.rhoPrd) for a, b in zip(prd_lines(p), prd_lines(q)))
    assert seen[-1][:2] == (max(want), [])
    for it, act, R in seen:
        assert act == [i for i, w in enumerate(want) if w > it]
        assert R is None if it < NSCATTER else len(R) == len(LOOP_SEEDS)
    # without prd the callback keeps its four arguments
    four = []
    OracleBatch([hot_column(LOOP_SEEDS[1]).copy()]).iterate_to_convergence(Nscatter=1, NmaxIter=2, callback=lambda *a: four.append(len(a)))
    assert four == [4, 4]


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
def raw_prd(batch, maxIter, tol, expect=abi.OK):
    """lwhip_batch_redistribute_prd called directly, every array pre-filled with a sentinel."""
    lib, n = batch.contexts[0].lib, len(batch.contexts)
    nSub = np.full(n, IFILL, dtype=np.int32)
    dRho, dIdx = np.full((n, max(maxIter, 1), 2), FILL), np.full((n, max(maxIter, 1), 2), IFILL, dtype=np.int32)
    dJ, dJIdx = np.full((n, max(maxIter, 1)), FILL), np.full((n, max(maxIter, 1)), IFILL, dtype=np.int32)
    res = abi.lwhip_batch_prd_result(IFILL, 0, nSub.ctypes.data_as(abi.i32p), dRho.ctypes.data_as(abi.f64p), dIdx.ctypes.data_as(abi.i32p),
                                     dJ.ctypes.data_as(abi.f64p), dJIdx.ctypes.data_as(abi.i32p))
    st = lib.lwhip_batch_redistribute_prd(batch._batch, maxIter, tol, C.byref(res))
    assert st == expect, (st, lib.lwhip_last_error())
    return dict(Nprd=res.Nprd, nSub=nSub, dRho=dRho, dRhoMaxIdx=dIdx, dJPrdMax=dJ, dJPrdMaxIdx=dJIdx)


def lone_contexts(probs):
    from lightweaver_amd.context import Context
    return [Context(p) for p in probs]


def resampled(Ns):
    return models.falc82() if Ns == 82 else models.resample(models.falc82(), Ns)


@functools.lru_cache(maxsize=None)
def geometry_case(Ns):
    """Three columns at Ns depths -- static, perturbed(seed = 3), perturbed(seed = 4) -- and two oracle iterations of each, a
    formal solution and redistribute_prd(2, 0.0): per column the problems and updates after the first and the second."""
    A = resampled(Ns)
    probs = [prd_column(A), prd_column(models.perturbed(A, seed=3)), prd_column(models.perturbed(A, seed=4))]
    refs = []
    for prob in probs:
        q = prob.copy()
        stages = []
        with OracleContext(q) as oc:
            for it in range(2):
                q.gamma_prefill()
                oc.formal_sol_gamma_matrices()
                u = frozen(oc.redistribute_prd(2, 0.0))
                stages.append((q.copy(), u))
        refs.append(stages)
    return probs, refs


@pytest.mark.gpu
@pytest.mark.parametrize('Ns', [13, 82, 253])
def test_one_call_every_geometry_class(gpu, monkeypatch, Ns):
    """16 rays per wavefront, 3 rays per wavefront, two-wavefront workgroups: one formal solution and prd_redistribute(2, 0.0),
    twice (the second call's sub-iterations all run the cached scatter kernel), every column against its own oracle run and
    against a lone Context given the same calls."""
    monkeypatch.setenv('LWHIP_SWEEP', 'lanes')
    built, refs = geometry_case(Ns)
    probs, twins = [p.copy() for p in built], [p.copy() for p in built]
    lones = lone_contexts(twins)
    try:
        with ColumnBatch(probs, fused=True, device_profiles=False) as batch:
            assert batch._batch is not None and all(c.sweep_kind() == 'lanes' for c in batch.contexts)
            for it in range(2):
                batch.formal_sol_gamma_matrices(sync_host=False)
                ups = batch.prd_redistribute(2, 0.0)
                batch.download(STATE)
                for i, (p, up) in enumerate(zip(probs, ups)):
                    tag = 'Ns %d call %d column %d' % (Ns, it, i)
                    q, u = refs[i][it]
                    assert_update(tag, up, u)
                    assert_state(tag + ' vs oracle', p, q, 1e-7)
                    lones[i].formal_sol_gamma_matrices(deviceResident=True)
                    lu = lones[i].prd_redistribute(2, 0.0, deviceResident=True)
                    lones[i].download(STATE)
                    assert lu.NprdSubIter == 2 and np.array_equal(lu.dRhoMaxIdx, up.dRhoMaxIdx), tag
                    assert_state(tag + ' vs lone', p, twins[i], 1e-10)
    finally:
        for c in lones:
            c.close()


@pytest.mark.gpu
@pytest.mark.parametrize('tol', sorted(STOP_TOLS, reverse=True))
def test_each_column_stops_by_its_own_changes(gpu, tol):
    """MAXIT = 7 sub-iterations asked for, two queued groups: each column runs the oracle's count for it and sits at the state
    of ITS stop -- a sub-iteration more would move rho by the next maximum of the table (>= 1.7 %), far above the bounds."""
    probs = [hot_column(s).copy() for s in STOP_SEEDS]
    twins = [hot_column(s).copy() for s in STOP_SEEDS]
    lones = lone_contexts(twins)
    try:
        with ColumnBatch(probs, device_profiles=False) as batch:
            assert batch._batch is not None
            batch.formal_sol_gamma_matrices(sync_host=False)
            ups = batch.prd_redistribute(MAXIT, tol)
            batch.download(STATE)
        for i, s in enumerate(STOP_SEEDS):
            tag = 'tol %g seed %d' % (tol, s)
            q, u = oracle_stop(s, tol)
            assert ups[i].NprdSubIter == STOP_TOLS[tol][i], tag
            assert_update(tag, ups[i], u)
            assert_state(tag + ' vs oracle', probs[i], q, 1e-7)
            lones[i].formal_sol_gamma_matrices(deviceResident=True)
            lu = lones[i].prd_redistribute(MAXIT, tol, deviceResident=True)
            lones[i].download(STATE)
            assert lu.NprdSubIter == ups[i].NprdSubIter, tag
            assert_state(tag + ' vs lone', probs[i], twins[i], 1e-10)
    finally:
        for c in lones:
            c.close()


@pytest.mark.gpu
def test_raw_call_leaves_slots_beyond_the_stop(gpu):
    tol = 0.07     # (stops 4, 5, 4: the last launch of a queued group and the first of the next)
    probs = [hot_column(s).copy() for s in STOP_SEEDS]
    with ColumnBatch(probs, device_profiles=False) as batch:
        batch.formal_sol_gamma_matrices(sync_host=False)
        r = raw_prd(batch, MAXIT, tol)
    assert r['Nprd'] == 2 and tuple(r['nSub']) == STOP_TOLS[tol]
    for i, s in enumerate(STOP_SEEDS):
        n, u = r['nSub'][i], oracle_stop(s, tol)[1]
        assert np.allclose(r['dRho'][i, :n], np.asarray(u['dRho']).reshape(-1, 2)[:n], rtol=1e-5, atol=1e-12)
        assert np.array_equal(r['dRhoMaxIdx'][i, :n], np.asarray(u['dRhoMaxIdx']).reshape(-1, 2)[:n])
        assert np.allclose(r['dJPrdMax'][i, :n], np.asarray(u['dJPrdMax'])[:n], rtol=1e-7, atol=1e-12)
        assert np.all(r['dRho'][i, n:] == FILL) and np.all(r['dRhoMaxIdx'][i, n:] == IFILL), s
        assert np.all(r['dJPrdMax'][i, n:] == FILL) and np.all(r['dJPrdMaxIdx'][i, n:] == IFILL), s


def snapshot(p):
    return dict(J=p.J.copy(), I=p.I.copy(), n=[a.n.copy() for a in p.atoms], rho=[t.rhoPrd.copy() for t in prd_lines(p)],
                Rij=[np.stack([t.Rij for t in a.trans]) for a in p.atoms], Rji=[np.stack([t.Rji for t in a.trans]) for a in p.atoms])


def same_bits(a, b):
    for k in a:
        xs, ys = (a[k], b[k]) if isinstance(a[k], list) else ([a[k]], [b[k]])
        if not all(np.array_equal(x, y) for x, y in zip(xs, ys)):
            return False
    return True


@pytest.mark.gpu
def test_inactive_column_is_untouched(gpu):
    """set_active([0, 2]): column 1 keeps its bits and its rows of the pre-filled result; columns 0 and 2 get what they get with
    everybody active (a twin batch); the convergence records keep the formal solution's dJMax."""
    tol = 0.15
    pa, pb = [hot_column(s).copy() for s in STOP_SEEDS], [hot_column(s).copy() for s in STOP_SEEDS]
    with ColumnBatch(pa, device_profiles=False) as A, ColumnBatch(pb, device_profiles=False) as B:
        for batch in (A, B):
            for it in range(NSCATTER):
                batch.formal_sol_gamma_matrices(sync_host=False)
            fs = batch.formal_sol_gamma_matrices()
            batch.stat_equil(report=True)
        B.set_active([0, 2])
        B.download(STATE)
        before = snapshot(pb[1])
        ra, rb = raw_prd(A, MAXIT, tol), raw_prd(B, MAXIT, tol)
        ups = B.prd_redistribute(1, 0.0)
        assert [u is None for u in ups] == [False, True, False]
        rb2 = raw_prd(B, MAXIT, tol)      # (a second call on the subset: column 1 still untouched)
        rec = np.zeros((3, 2 + 2 * 2))
        assert B.contexts[0].lib.lwhip_batch_conv_records(B._batch, rec.ctypes.data_as(abi.f64p), None) == abi.OK
        assert [rec[i, 0] for i in range(3)] == [u.dJMax for u in fs] and all(u.dJMax > 0.0 for u in fs)
        B.download(STATE)
        assert same_bits(before, snapshot(pb[1]))
        # ... and on the device: the next reported solve builds its records from the batch's tail again
        B.set_active(None)
        Js, _ = B._stat_equil_report()
        assert [u.dJMax for u in Js] == [u.dJMax for u in fs]
        assert rb['nSub'][1] == IFILL and np.all(rb['dRho'][1] == FILL) and np.all(rb['dJPrdMaxIdx'][1] == IFILL)
        assert rb2['nSub'][1] == IFILL and rb2['nSub'][0] >= 1
    # columns 0 and 2 of B report what they report in A, to test_prd.py's bounds for these numbers: the twin batches' populations
    # differ in the last bits after four iterations and a solve (Gamma is summed by atomics), which max |d rho / rho| amplifies
    # where rho passes close to zero.  (The state itself, to 1e-10: test_active_subset_state_matches_all_active.)
    for i in (0, 2):
        n = ra['nSub'][i]
        assert n == rb['nSub'][i] and n >= 1
        assert np.array_equal(ra['dRhoMaxIdx'][i, :n], rb['dRhoMaxIdx'][i, :n])
        assert np.allclose(ra['dRho'][i, :n], rb['dRho'][i, :n], rtol=1e-5, atol=1e-12)
        assert np.allclose(ra['dJPrdMax'][i, :n], rb['dJPrdMax'][i, :n], rtol=1e-7, atol=1e-12)


@pytest.mark.gpu
def test_active_subset_state_matches_all_active(gpu):
    tol = 0.15
    pa, pb = [hot_column(s).copy() for s in STOP_SEEDS], [hot_column(s).copy() for s in STOP_SEEDS]
    with ColumnBatch(pa, device_profiles=False) as A, ColumnBatch(pb, device_profiles=False) as B:
        for batch in (A, B):
            batch.formal_sol_gamma_matrices(sync_host=False)
        B.set_active([0, 2])
        ua, ub = A.prd_redistribute(MAXIT, tol), B.prd_redistribute(MAXIT, tol)
        A.download(STATE)
        B.download(STATE)
    assert ub[1] is None
    for i in (0, 2):
        assert ua[i].NprdSubIter == ub[i].NprdSubIter == STOP_TOLS[tol][i]
        assert_state('subset column %d' % i, pb[i], pa[i], 1e-10)
    assert rel_err(prd_lines(pb[1])[0].rhoPrd, prd_lines(pa[1])[0].rhoPrd) > 1e-3      # (column 1 of B never ran)


@pytest.mark.gpu
def test_refusals_and_empties(gpu):
    from lightweaver_amd.context import Context
    # a missing C, a pending split iteration: LWHIP_ERR_INVALID before anything is queued
    probs = [hot_column(s).copy() for s in STOP_SEEDS]
    probs[1].atoms[1].C = None
    with ColumnBatch(probs, device_profiles=False) as batch:
        lib = batch.contexts[0].lib
        r = raw_prd(batch, 2, 0.0, expect=abi.ERR_INVALID)
        assert b'collisional rates' in lib.lwhip_last_error() and np.all(r['nSub'] == IFILL) and np.all(r['dRho'] == FILL)
        assert lib.lwhip_batch_redistribute_prd(batch._batch, 2, 0.0, None) == abi.ERR_INVALID
        assert lib.lwhip_batch_redistribute_prd(None, 2, 0.0, None) == abi.ERR_INVALID
        batch.set_active([0, 2])
        batch.contexts[2].fs_partial()
        r = raw_prd(batch, 2, 0.0, expect=abi.ERR_INVALID)
        assert b'pending' in lib.lwhip_last_error() and np.all(r['nSub'] == IFILL)
        batch.contexts[2].fs_finalise()
        batch.formal_sol_gamma_matrices(sync_host=False)
        r = raw_prd(batch, 2, 0.0)         # (the column without C is inactive: the call runs)
        assert list(r['nSub']) == [2, IFILL, 2]
        # maxIter = 0: nothing runs
        r = raw_prd(batch, 0, 0.0)
        assert list(r['nSub']) == [0, IFILL, 0] and r['Nprd'] == 2 and np.all(r['dRho'] == FILL)
        ups = batch.prd_redistribute(0, 0.0)
        assert ups[1] is None and ups[0].NprdSubIter == 0 and ups[0].dRho.shape == (0, 2) and ups[0].dJMax == 0.0
    # no PRD line
    plain = [models.falc_h_ca(Nrays=3, lineScale=0.3, atmos=models.perturbed(models.falc82(), s)) for s in (1, 2)]
    with ColumnBatch(plain, device_profiles=False) as batch:
        batch.formal_sol_gamma_matrices(sync_host=False)
        ups = batch.prd_redistribute(3, 1e-2)
        assert [u.NprdSubIter for u in ups] == [0, 0] and not ups[0].updatedRho
    # hybrid-PRD columns: LWHIP_ERR_UNSUPPORTED
    prob = hot_column(STOP_SEEDS[0])
    with OracleContext(prob.copy()) as oc:
        tables = oc.build_hprd()
        try:
            ctxs = [Context(prob.copy(), hprd=tables) for _ in range(2)]
            try:
                lib = ctxs[0].lib
                arr = (C.c_void_p * 2)(*[c._h for c in ctxs])
                h = C.c_void_p()
                assert lib.lwhip_batch_create(arr, 2, C.byref(h)) == abi.OK
                nSub = np.full(2, IFILL, dtype=np.int32)
                res = abi.lwhip_batch_prd_result(0, 0, nSub.ctypes.data_as(abi.i32p), None, None, None, None)
                assert lib.lwhip_batch_redistribute_prd(h, 2, 0.0, C.byref(res)) == abi.ERR_UNSUPPORTED
                assert np.all(nSub == IFILL)
                lib.lwhip_batch_destroy(h)
            finally:
                for c in reversed(ctxs):
                    c.close()
        finally:
            tables.close()


@pytest.mark.gpu
def test_unfused_batch_gives_the_columns_results(gpu):
    tol = 0.15
    probs = [hot_column(s).copy() for s in STOP_SEEDS]
    with ColumnBatch(probs, device_profiles=False, fused=False) as batch:
        assert batch._batch is None
        batch.formal_sol_gamma_matrices(sync_host=False)
        batch.set_active([0, 2])
        ups = batch.prd_redistribute(MAXIT, tol)
        batch.download(STATE)
    assert ups[1] is None
    for i in (0, 2):
        q, u = oracle_stop(STOP_SEEDS[i], tol)
        assert_update('unfused column %d' % i, ups[i], u)
        assert_state('unfused column %d' % i, probs[i], q, 1e-7)


@pytest.mark.gpu
def test_march_batch_runs_the_columns_one_by_one(gpu, monkeypatch):
    monkeypatch.setenv('LWHIP_SWEEP', 'march')
    built, refs = geometry_case(13)
    probs = [p.copy() for p in built]
    with ColumnBatch(probs, fused=True, device_profiles=False) as batch:
        assert batch._batch is not None and all(c.sweep_kind() != 'lanes' for c in batch.contexts)
        batch.formal_sol_gamma_matrices(sync_host=False)
        ups = batch.prd_redistribute(2, 0.0)
        batch.download(STATE)
    for i, (p, up) in enumerate(zip(probs, ups)):
        q, u = refs[i][0]
        assert_update('march column %d' % i, up, u)
        assert_state('march column %d' % i, p, q, 1e-7)


@pytest.mark.gpu
def test_iterate_to_convergence_prd_matches_oracle_per_column(gpu):
    probs = [hot_column(s).copy() for s in LOOP_SEEDS]
    with ColumnBatch(probs) as batch:
        assert batch._batch is not None
        res = batch.iterate_to_convergence(retire=True, **KW)
        assert batch.active == list(range(len(LOOP_SEEDS)))
        batch.download(abi.ALL_OUTPUTS | abi.POPS | abi.RHOPRD)
    want = [oracle_loop(s)['stop'] for s in LOOP_SEEDS]
    print('iterations', res.iterations, 'oracle', want)
    assert res.iterations == want and res.converged == [True] * len(LOOP_SEEDS)
    for s, p, fin in zip(LOOP_SEEDS, probs, res.final):
        q = oracle_loop(s)['q']
        assert len(fin) == 3 and fin[2].NprdSubIter >= 1
        errs = dict(J=rel_err(p.J, q.J), n=max(rel_err(a.n, b.n) for a, b in zip(p.atoms, q.atoms)),
                    rho=max(rel_err(a.rhoPrd, b.rhoPrd) for a, b in zip(prd_lines(p), prd_lines(q))))
        print('seed', s, errs)
        # every column sits at the state of its OWN stop iteration: a retired column is frozen there
        assert errs['J'] <= TOL_CONVERGED and errs['n'] <= TOL_CONVERGED and errs['rho'] <= 1e-6, (s, errs)
