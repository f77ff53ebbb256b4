"""Column batches iterated to convergence: the per-column population change (lwhip_batch_stat_equil_report), the active set
(lwhip_batch_set_active) and ColumnBatch.iterate_to_convergence, against the loop of iterate_ctx_se driven on the CPU oracle
column by column.

Columns: the batch tests' perturbed FAL-C columns (82 depths: two solve blocks per atom, so the cross-block combine of the
change records is exercised), H(6) + Ca II(6), 3 rays.  Tolerances are the project's own for exactly these comparisons
(test_iterate_ctx_se_device_resident_matches_oracle_loop): dJMax rel 1e-6, dPops rtol 1e-5, states TOL_CONVERGED."""
import ctypes as C
import functools

import numpy as np
import pytest

from helpers import TOL_CONVERGED, rel_err
from lightweaver_amd import _abi as abi
from lightweaver_amd.batch import ColumnBatch
from lightweaver_amd.harness import models
from lightweaver_amd.iterate import iterate_ctx_se
from test_iterate import OracleLoopContext

# Oracle stop iterations 28, 20, 20, 24, 26.  Left out as fragile (test_oracle_traces_spread_and_are_not_fragile): seed 101,
# whose final dJMax is 0.09996 against JTol = 0.1, and seed 104, whose final max dPops is 0.05952 against popsTol = 0.06 --
# within 1 %; 107 stands in for it.
SEEDS = [100, 102, 103, 107, 105]
JTOL, PTOL, NSCATTER, NMAX = 1e-1, 6e-2, 3, 60
KW = dict(Nscatter=NSCATTER, NmaxIter=NMAX, JTol=JTOL, popsTol=PTOL)


def column(seed, dv=2.0e3):
    return models.build_problem(models.perturbed(models.falc82(), seed, dT=0.3, dv=dv), [models.H_6(0.3), models.CaII_6(0.3)], Nrays=3)


@functools.lru_cache(maxsize=None)
def oracle_trace(seed):
    """The loop of iterate_ctx_se on the oracle for one column, every iteration's numbers kept: stop iteration, per iteration
    (dJMax, dPops or None, dPopsMaxIdx or None), and J and n at the stop.  Computed once and never modified."""
    q = column(seed)
    oc = OracleLoopContext(q)
    trace, stop = [], None
    for it in range(NMAX):
        Ju = oc.formal_sol_gamma_matrices()
        if it < NSCATTER:
            trace.append((Ju.dJMax, None, None))
            continue
        Pu = oc.stat_equil()
        trace.append((Ju.dJMax, list(Pu.dPops), list(Pu.dPopsMaxIdx)))
        if Ju.dJMax < JTOL and max(Pu.dPops) < PTOL:
            stop = it
            break
    assert stop is not None
    out = dict(stop=stop, trace=trace, J=q.J.copy(), n=[a.n.copy() for a in q.atoms])
    out['J'].setflags(write=False)
    return out


class OracleBatch(ColumnBatch):
    """A ColumnBatch that is not fused and whose columns compute on the CPU oracle: no device."""

    def __init__(self, problems):
        self.problems = list(problems)
        self.contexts = [OracleLoopContext(p) for p in self.problems]
        self._batch = None
        self._active = None

    def formal_sol_gamma_matrices(self, lambdaIterate=False, sync_host=True):
        ups = [None] * len(self.contexts)
        for i in self.active:
            ups[i] = self.contexts[i].formal_sol_gamma_matrices()
        return ups if sync_host else None


# ---- 1. CPU: the oracle precondition and the loop's logic -----------------------------------------------------------------
def test_oracle_traces_spread_and_are_not_fragile():
    stops = {s: oracle_trace(s)['stop'] for s in SEEDS}
    print('oracle stop iterations', stops)
    assert len(set(stops.values())) >= 3, stops
    # the traces agree with iterate_ctx_se itself
    assert iterate_ctx_se(OracleLoopContext(column(SEEDS[1])), **KW) == stops[SEEDS[1]]
    # at no iteration is one number within 1 % of its tolerance while the other is below 1.01 x its own: the device's
    # 1e-6-level differences then cannot move a stop iteration
    for s in SEEDS:
        for it, (dJ, dP, _) in enumerate(oracle_trace(s)['trace']):
            if dP is None:
                continue
            p = max(dP)
            nearJ = 0.99 * JTOL < dJ < 1.01 * JTOL and p < 1.01 * PTOL
            nearP = 0.99 * PTOL < p < 1.01 * PTOL and dJ < 1.01 * JTOL
            assert not (nearJ or nearP), (s, it, dJ, p)


def test_iterate_to_convergence_on_oracle_columns():
    probs = [column(s) for s in SEEDS]
    batch = OracleBatch(probs)
    seen = []
    res = batch.iterate_to_convergence(callback=lambda it, J, P, act: seen.append((it, list(act))), **KW)
    want = [oracle_trace(s)['stop'] for s in SEEDS]
    assert res.iterations == want
    assert res.converged == [True] * len(SEEDS)
    assert batch.active == list(range(len(SEEDS)))
    for s, p, fin in zip(SEEDS, probs, res.final):
        tr = oracle_trace(s)
        # a retired column stays at its own stop iteration's state (the oracle is deterministic: the same bits)
        assert np.array_equal(p.J, tr['J']) and all(np.array_equal(a.n, n) for a, n in zip(p.atoms, tr['n']))
        assert fin[0].dJMax == tr['trace'][tr['stop']][0] and fin[1].dPops == tr['trace'][tr['stop']][1]
    # the active set shrinks exactly at the stop iterations and ends empty
    assert seen[-1] == (max(want), [])
    for it, act in seen:
        assert act == [i for i, w in enumerate(want) if w > it]


def test_iterate_to_convergence_nmaxiter_and_no_retire():
    seeds = [100, 102, 103]
    want = [oracle_trace(s)['stop'] for s in seeds]
    nmax = min(want) + 2
    assert min(want) < nmax - 1 < max(want)
    batch = OracleBatch([column(s) for s in seeds])
    seen = []
    res = batch.iterate_to_convergence(Nscatter=NSCATTER, NmaxIter=nmax, JTol=JTOL, popsTol=PTOL, retire=False,
                                       callback=lambda it, J, P, act: seen.append(list(act)))
    assert res.converged == [w < nmax for w in want]
    assert res.iterations == [w if w < nmax else nmax - 1 for w in want]
    assert [f == [] for f in res.final] == [w >= nmax for w in want]
    assert all(a == [0, 1, 2] for a in seen) and len(seen) == nmax     # (retire=False: recorded only, everybody keeps iterating)
    assert batch.active == [0, 1, 2]
    # the full set is restored when an exception passes through
    def boom(it, J, P, act):
        if it == NSCATTER + 1:
            raise RuntimeError('stop here')
    batch.set_active([1])
    with pytest.raises(RuntimeError, match='stop here'):
        batch.iterate_to_convergence(Nscatter=NSCATTER, NmaxIter=8, JTol=10.0, popsTol=1e-30, callback=boom)
    assert batch.active == [0, 1, 2]
    with pytest.raises(ValueError):
        batch.set_active([2, 1])
    with pytest.raises(ValueError):
        batch.set_active([0, 3])


# ---- GPU ------------------------------------------------------------------------------------------------------------------
def snapshot(p):
    return dict(J=p.J.copy(), I=p.I.copy(), n=[a.n.copy() for a in p.atoms], Gamma=[a.Gamma.copy() for a in p.atoms],
                Rij=[np.stack([t.Rij for t in a.trans]) for a in p.atoms], Rji=[np.stack([t.Rji for t in a.trans]) for a in p.atoms])


def same_bits(a, b, keys=('J', 'I', 'n', 'Gamma', 'Rij', 'Rji')):
    for k in keys:
        xs, ys = (a[k], b[k]) if isinstance(a[k], list) else ([a[k]], [b[k]])
        if not all(np.array_equal(x, y) for x, y in zip(xs, ys)):
            return False
    return True


@pytest.mark.gpu
def test_reported_solve_matches_oracle_and_lone_context(gpu):
    """stat_equil(report=True) after 4 iterations (nscatter = 3).  The solve itself is unchanged: from the same Gamma and
    the same n, the reported and the unreported launch leave the same bits in n.  (Both run on ONE batch, n put back in
    between: the Gamma of twin batches differ in the last bits, summed by atomics as they are, and so would n.)"""
    from lightweaver_amd.context import Context
    seeds = SEEDS[:3]
    probs = [column(s) for s in seeds]
    with ColumnBatch(probs) as batch:
        assert batch._batch is not None
        for it in range(NSCATTER + 1):
            batch.formal_sol_gamma_matrices(sync_host=False)
        n0 = [[a.n.copy() for a in p.atoms] for p in probs]
        ups = batch.stat_equil(report=True)
        batch.download(abi.POPS)
        n1 = [[a.n.copy() for a in p.atoms] for p in probs]
        for p, c, n in zip(probs, batch.contexts, n0):
            for a, x in zip(p.atoms, n):
                a.n[...] = x
            c.upload(abi.POPS)
        batch.stat_equil()
        batch.download(abi.POPS)
        for p, n, old in zip(probs, n1, n0):
            assert all(np.array_equal(a.n, x) for a, x in zip(p.atoms, n))
            assert not any(np.array_equal(a.n, x) for a, x in zip(p.atoms, old))
    # ... and a twin batch that never asks for a report lands on the same n up to what its own Gamma's rounding does to one
    # solve: 1e-8, the bound smoke() holds n to after one stat_equil
    twins = [column(s) for s in seeds]
    with ColumnBatch(twins) as twin:
        twin.iterate(NSCATTER + 1, nscatter=NSCATTER)
        twin.download(abi.POPS)
    for p, n in zip(twins, n1):
        errs = [rel_err(a.n, x) for a, x in zip(p.atoms, n)]
        print('twin batch, unreported solve: n rel', errs)
        assert max(errs) <= 1e-8
    for s, u in zip(seeds, ups):
        dJ, dP, idx = oracle_trace(s)['trace'][NSCATTER]
        print('seed', s, 'dPops', u.dPops, 'oracle', dP, 'idx', u.dPopsMaxIdx, idx)
        assert u.updatedPops and np.allclose(u.dPops, dP, rtol=1e-5)
        assert list(u.dPopsMaxIdx) == list(idx)
        with Context(column(s)) as ctx:
            ctx.compute_profiles(deviceResident=True)      # (as the batch's columns: profiles made on the device)
            for it in range(NSCATTER + 1):
                ctx.formal_sol_gamma_matrices(deviceResident=True)
            lone = ctx.stat_equil(deviceResident=True)
        assert list(u.dPopsMaxIdx) == list(lone.dPopsMaxIdx)
        assert np.allclose(u.dPops, lone.dPops, rtol=1e-9, atol=0.0)


@pytest.mark.gpu
@pytest.mark.parametrize('fused', [True, False])
def test_iterate_to_convergence_matches_oracle_per_column(gpu, fused):
    probs = [column(s) for s in SEEDS]
    with ColumnBatch(probs, fused=fused) as batch:
        assert (batch._batch is not None) == fused
        res = batch.iterate_to_convergence(**KW)
        assert batch.active == list(range(len(SEEDS)))
        batch.download()
    want = [oracle_trace(s)['stop'] for s in SEEDS]
    print('iterations', res.iterations, 'oracle', want)
    assert res.iterations == want and res.converged == [True] * len(SEEDS)
    for s, p, fin in zip(SEEDS, probs, res.final):
        tr = oracle_trace(s)
        dJ, dP, idx = tr['trace'][tr['stop']]
        print('seed', s, 'dJMax', fin[0].dJMax, dJ, 'dPops', fin[1].dPops, dP, 'J', rel_err(p.J, tr['J']),
              'n', [rel_err(a.n, n) for a, n in zip(p.atoms, tr['n'])])
        assert fin[0].dJMax == pytest.approx(dJ, rel=1e-6)
        assert np.allclose(fin[1].dPops, dP, rtol=1e-5)
        # every column sits at the state of its OWN stop iteration
        assert rel_err(p.J, tr['J']) <= TOL_CONVERGED
        for a, n in zip(p.atoms, tr['n']):
            assert rel_err(a.n, n) <= TOL_CONVERGED


@pytest.mark.gpu
def test_retired_columns_are_untouched(gpu):
    probs = [column(s) for s in SEEDS]
    with ColumnBatch(probs) as batch:
        batch.iterate(2, nscatter=0)
        batch.download()
        first = [snapshot(p) for p in probs]
        batch.set_active([0, 2, 4])
        assert batch.active == [0, 2, 4]
        ups = batch.formal_sol_gamma_matrices()
        assert [u is None for u in ups] == [False, True, False, True, False]
        batch.stat_equil()
        batch.formal_sol_gamma_matrices(sync_host=False)
        pu = batch.stat_equil(report=True)
        assert [u is None for u in pu] == [False, True, False, True, False]
        batch.download()
        second = [snapshot(p) for p in probs]
        batch.set_active(None)
        assert batch.active == [0, 1, 2, 3, 4]
    for i in (1, 3):
        assert same_bits(first[i], second[i]), i
    for i in (0, 2, 4):
        for k in ('J', 'I', 'n', 'Gamma'):
            assert not same_bits(first[i], second[i], keys=(k,)), (i, k)


def raw_fs(batch, fill=-7.0):
    """lwhip_batch_formal_sol_gamma_matrices called directly, the caller's results pre-filled."""
    lib = batch.contexts[0].lib
    res = (abi.lwhip_iter_result * len(batch.contexts))()
    for r in res:
        r.dJMax, r.dJMaxIdx = fill, -7
    assert lib.lwhip_batch_formal_sol_gamma_matrices(batch._batch, 0, batch.contexts[0].crsw, res) == abi.OK
    return [(r.dJMax, r.dJMaxIdx) for r in res]


@pytest.mark.gpu
@pytest.mark.parametrize('moving', ['all', 'one'])
def test_result_of_a_column_does_not_depend_on_the_active_set(gpu, moving):
    """One formal_sol_gamma_matrices with only {1, 3} active and one with everybody, on twin batches: J and I of columns 1
    and 3 to the last bit, Gamma to the run-to-run bound of its atomics (test_column_batch_gathered_upload_equals_separate_copies:
    1e-11).  moving='one': column 0 moves and the rest are static, so whether the launch may pair rays / share stencils
    (phiSym / phiIso) has to be decided over ALL columns -- decided over the active ones, columns 1 and 3 would run another
    code path here than in the full batch."""
    from test_hip_parity import compare_problems
    dvs = [2.0e3] * 5 if moving == 'all' else [2.0e3, 0.0, 0.0, 0.0, 0.0]
    make = lambda: [column(s, dv=dv) for s, dv in zip(SEEDS, dvs)]    # noqa: E731
    pa, pb = make(), make()
    with ColumnBatch(pa) as A, ColumnBatch(pb) as B:
        A.set_active([1, 3])
        ra = raw_fs(A)
        rb = raw_fs(B)
        A.download()
        B.download()
    assert ra[0] == ra[2] == ra[4] == (-7.0, -7)          # (entries of inactive columns: as the caller filled them)
    for i in (1, 3):
        assert ra[i] == rb[i] and ra[i][0] > 0.0
        assert np.array_equal(pa[i].J, pb[i].J) and np.array_equal(pa[i].I, pb[i].I)
        compare_problems(pa[i], pb[i], tol=1e-11, what=('Gamma',))
    for i in (0, 2, 4):
        assert not np.array_equal(pa[i].J, pb[i].J)       # (never iterated in A)


@pytest.mark.gpu
def test_edges_one_column_twins_and_rays_after_retiring(gpu):
    s = SEEDS[1]
    want = oracle_trace(s)['stop']
    seen = []
    with ColumnBatch([column(s)]) as one:
        res = one.iterate_to_convergence(callback=lambda it, J, P, act: seen.append(list(act)), **KW)
        assert res.iterations == [want] and res.converged == [True]
        assert seen[-1] == [] and all(a == [0] for a in seen[:-1]) and len(seen) == want + 1
        assert one.active == [0]
    seen = []
    with ColumnBatch([column(s), column(SEEDS[0]), column(s)]) as three:
        res = three.iterate_to_convergence(callback=lambda it, J, P, act: seen.append(list(act)), **KW)
        assert res.iterations == [want, oracle_trace(SEEDS[0])['stop'], want]
        assert seen[want - 1] == [0, 1, 2] and seen[want] == [1]          # the twins leave in the same iteration
        three.set_active([1])
        three.set_active(None)
        assert three.active == [0, 1, 2]
        I = three.compute_rays(mus=[1.0, 0.5])
        assert I.shape[0] == 3 and I.shape[2] == 2 and np.all(np.isfinite(I)) and np.all(I[:, :, 0] > 0.0)
        # (the twins' Gamma are summed by atomics: their spectra agree to rounding, not to the bit)
        assert np.allclose(I[0], I[2], rtol=1e-8, atol=0.0) and not np.allclose(I[0], I[1], rtol=1e-3, atol=0.0)


@pytest.mark.gpu
def test_set_active_refusals_leave_the_set(gpu):
    with ColumnBatch([column(s) for s in SEEDS[:4]]) as batch:
        lib, h = batch.contexts[0].lib, batch._batch

        def active():
            cols = (C.c_int32 * 4)()
            n = C.c_int(-1)
            assert lib.lwhip_batch_active(h, cols, C.byref(n)) == abi.OK
            return list(cols[:n.value])

        def set_active(cols, n=None):
            arr = (C.c_int32 * max(len(cols), 1))(*cols)
            return lib.lwhip_batch_set_active(h, arr, len(cols) if n is None else n)

        assert active() == [0, 1, 2, 3]
        assert set_active([1, 3]) == abi.OK and active() == [1, 3]
        for bad, n in (([1, 4], None), ([-1, 2], None), ([2, 2], None), ([3, 1], None), ([1, 3], -1)):
            assert set_active(bad, n) == abi.ERR_INVALID, (bad, n)
            assert active() == [1, 3]
        ra = raw_fs(batch)                                  # the next iteration still runs, on the set that was kept
        assert ra[0] == ra[2] == (-7.0, -7) and ra[1][0] > 0.0 and ra[3][0] > 0.0
        assert lib.lwhip_batch_set_active(h, None, 0) == abi.OK and active() == [0, 1, 2, 3]
        assert all(r[0] > 0.0 for r in raw_fs(batch))


# ---- the active set as one list per kind: grown, shrunk and restored with iterations in between ---------------------------------
def raw_report(batch, fill=-7.0):
    """lwhip_batch_stat_equil_report called directly, the caller's arrays pre-filled: (dPops, indices), one row per column."""
    lib = batch.contexts[0].lib
    n, nAt = len(batch.contexts), sum(1 for a in batch.problems[0].atoms if not a.detailed)
    dP, dI = np.full((n, nAt), fill), np.full((n, nAt), -7, dtype=np.int32)
    assert lib.lwhip_batch_stat_equil_report(batch._batch, dP.ctypes.data_as(abi.f64p), dI.ctypes.data_as(abi.i32p)) == abi.OK
    return dP, dI


def lone_column(seed):
    """A lone Context on a twin of the column, its profiles made on the device as the batch's are."""
    from lightweaver_amd.context import Context
    p = column(seed)
    ctx = Context(p)
    ctx.compute_profiles(deviceResident=True)
    return p, ctx


def close_to_lone(tag, got, want, idxGot, idxWant):
    """Batch column against lone context, the bounds of test_reported_solve_matches_oracle_and_lone_context: the same index,
    the value to rtol 1e-9."""
    print(tag, 'batch', got, idxGot, 'lone', want, idxWant)
    assert list(np.atleast_1d(idxGot)) == list(np.atleast_1d(idxWant)), tag
    assert np.allclose(got, want, rtol=1e-9, atol=0.0), tag


@pytest.mark.gpu
def test_an_active_set_walk_matches_fresh_batches(gpu):
    """all -> [1, 3] -> [0, 1, 3, 4] -> all -> [2] -> all, one raw iteration and one reported solve at every stop: the lists
    are refreshed to a smaller set, to a larger one and to the full one with work in between.  Every column is held to a lone
    Context driven through the same calls; an inactive column keeps its bits and its entries of the pre-filled results."""
    walk = [None, [1, 3], [0, 1, 3, 4], None, [2], None]
    probs = [column(s) for s in SEEDS]
    lones = [lone_column(s) for s in SEEDS]
    try:
        with ColumnBatch(probs) as batch:
            assert batch._batch is not None
            for stop, cols in enumerate(walk):
                batch.download()
                before = [snapshot(p) for p in probs]
                batch.set_active(cols)
                act = list(range(len(SEEDS))) if cols is None else cols
                assert batch.active == act
                rJ = raw_fs(batch)
                dP, dI = raw_report(batch)
                batch.download()
                for i, (p, (q, ctx)) in enumerate(zip(probs, lones)):
                    if i not in act:
                        assert same_bits(before[i], snapshot(p)), (stop, i)
                        assert rJ[i] == (-7.0, -7) and np.all(dP[i] == -7.0) and np.all(dI[i] == -7), (stop, i)
                        continue
                    Ju = ctx.formal_sol_gamma_matrices(deviceResident=True)
                    Pu = ctx.stat_equil(deviceResident=True)
                    ctx.download(abi.ALL_OUTPUTS | abi.POPS)
                    tag = 'stop %d column %d' % (stop, i)
                    close_to_lone(tag + ' dJMax', rJ[i][0], Ju.dJMax, rJ[i][1], Ju.dJMaxIdx)
                    close_to_lone(tag + ' dPops', dP[i], Pu.dPops, dI[i], Pu.dPopsMaxIdx)
                    errs = rel_err(p.J, q.J), rel_err(p.I, q.I)
                    print(tag, 'J, I rel', errs)
                    assert max(errs) <= 1e-9, tag
                    assert not same_bits(before[i], snapshot(p), keys=('J',)), tag
    finally:
        for _, ctx in lones:
            ctx.close()


@pytest.mark.gpu
def test_apply_blocks_follow_crsw_on_a_subset(gpu):
    """The device copy of the apply blocks (aValid / aCrsw) across a change of crsw and a change of set: [1, 3] active, one raw
    iteration with crsw and one with half of it, then all columns with that half again -- the same crsw, but another set's
    blocks.  Gamma of every column that ran against a fresh twin batch given the same calls, to the bound of its atomics
    (test_result_of_a_column_does_not_depend_on_the_active_set: 1e-11)."""
    from test_hip_parity import compare_problems
    pa, pb = [column(s) for s in SEEDS], [column(s) for s in SEEDS]

    def fs(batch, crsw):
        lib = batch.contexts[0].lib
        assert lib.lwhip_batch_formal_sol_gamma_matrices(batch._batch, 0, crsw, None) == abi.OK
        batch.download()

    def lone_fs(pc, cw):
        pc[1].crsw = cw
        pc[1].formal_sol_gamma_matrices(deviceResident=True)
        pc[1].download(abi.ALL_OUTPUTS)
        return pc[0]

    lones = {i: lone_column(SEEDS[i]) for i in (0, 1)}
    try:
        with ColumnBatch(pa) as A, ColumnBatch(pb) as B:
            crsw = A.contexts[0].crsw
            for cols, cw in (([1, 3], crsw), ([1, 3], 0.5 * crsw), (None, 0.5 * crsw)):
                for batch in (A, B):
                    batch.set_active(cols)
                    fs(batch, cw)
                ran = list(range(len(SEEDS))) if cols is None else cols
                for i in ran:
                    worst = compare_problems(pa[i], pb[i], tol=1e-11, what=('Gamma',))
                    print('set', cols, 'crsw', cw, 'column', i, worst)
                # ... and crsw did arrive (twins would agree on a stale block too): lone Contexts given the same crsw, to the
                # walk's bound for a batch column against a lone context -- a block of the other crsw is off by half of C
                for i in lones:
                    if i in ran:
                        worst = compare_problems(pa[i], lone_fs(lones[i], cw), tol=1e-9, what=('Gamma',))
                        print('column', i, 'against its lone context', worst)
    finally:
        for _, ctx in lones.values():
            ctx.close()


@functools.lru_cache(maxsize=None)
def lone_first_report(seed, ng):
    """A lone Context's reported solve after NSCATTER + 1 iterations (ng: configured just before it), computed once: dPops,
    indices, ngAccelerated."""
    p, ctx = lone_column(seed)
    with ctx:
        for it in range(NSCATTER + 1):
            ctx.formal_sol_gamma_matrices(deviceResident=True)
        if ng is not None:
            ctx.configure_ng(*ng)
        up = ctx.stat_equil(deviceResident=True)
    return tuple(up.dPops), tuple(up.dPopsMaxIdx), bool(up.ngAccelerated)


ORDERS = [(first, ng) for first in ('all', 'subset') for ng in (None, (2, 3, 5))]


@functools.lru_cache(maxsize=None)
def first_report_order(first, ng):
    """One order of first reports on a fresh batch, computed once: all columns or [0, 2] active; with ng the first report is
    made with Ng configured, which is switched off again before the next.  Every report starts from the same populations
    (put back in between) and the Gamma of NSCATTER + 1 iterations.  Returns the active set, {column: (dPops, indices,
    ngAccelerated)} of the Ng-on report (None without ng), of the Ng-off report of that set and of a last one of all columns,
    and the Ng call counts after the Ng-on report."""
    from ng_cases import put
    ncol = len(SEEDS)
    act = list(range(ncol)) if first == 'all' else [0, 2]
    probs = [column(s) for s in SEEDS]

    def report(batch, n0, active):
        for i in active:
            put(batch.contexts[i], probs[i], n0[i])
        ups = batch.stat_equil(report=True)
        assert [u is not None for u in ups] == [i in active for i in range(ncol)]
        return {i: (list(ups[i].dPops), list(ups[i].dPopsMaxIdx), bool(ups[i].ngAccelerated)) for i in active}

    with ColumnBatch(probs) as batch:
        assert batch._batch is not None
        for it in range(NSCATTER + 1):
            batch.formal_sol_gamma_matrices(sync_host=False)
        batch.download(abi.POPS)
        n0 = [[a.n.copy() for a in p.atoms] for p in probs]
        batch.set_active(act)
        on = counts = None
        if ng is not None:
            batch.configure_ng(*ng)
            on = report(batch, n0, act)
            counts = batch.ng_state()['counts']
            batch.configure_ng(0, 0, 0)
        off = report(batch, n0, act)
        batch.set_active(None)
        full = report(batch, n0, list(range(ncol)))
    return dict(act=act, on=on, counts=counts, off=off, full=full)


@pytest.mark.gpu
@pytest.mark.parametrize('first,ng', ORDERS)
def test_first_report_in_any_order(gpu, first, ng):
    """The change records are made with the batch, so the first report finds the same state whatever came before it
    (first_report_order: the four orders the lazily made records used to distinguish).  The Ng-off reports agree between this
    order and each of the other three, and with a lone Context, within the bounds of the walk above.  With Ng on the report
    agrees with a lone Context that was given configure_ng at the same point -- one recording step, not extrapolated -- within
    those bounds too (the bound of test_ng_on_changes_nothing_but_ng).  Not bit for bit, as test_batch_ng.py's Twins compare
    an Ng step from uploaded populations: here the solve in front of the step reads a Gamma that the fused batch sums by
    atomics, which no lone context reproduces to the last bit."""
    got = first_report_order(first, ng)
    act = got['act']
    if ng is not None:
        assert got['counts'] == [2 if i in act else 1 for i in range(len(SEEDS))]
        for i in act:
            dP, dI, acc = lone_first_report(SEEDS[i], ng)
            close_to_lone('Ng on, column %d' % i, got['on'][i][0], dP, got['on'][i][1], dI)
            assert got['on'][i][2] == acc and not acc
    for i, s in enumerate(SEEDS):
        dP, dI, _ = lone_first_report(s, None)
        close_to_lone('all columns at the end, column %d' % i, got['full'][i][0], dP, got['full'][i][1], dI)
        assert not got['full'][i][2]
        if i in act:
            close_to_lone('Ng off, column %d' % i, got['off'][i][0], dP, got['off'][i][1], dI)
            assert not got['off'][i][2]
    for other in ORDERS:
        if other == (first, ng):
            continue
        theirs = first_report_order(*other)['off']
        for i in sorted(set(got['off']) & set(theirs)):
            close_to_lone('column %d against the order %s' % (i, other), got['off'][i][0], theirs[i][0], got['off'][i][1], theirs[i][1])
