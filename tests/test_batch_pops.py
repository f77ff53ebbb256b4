"""Time-dependent and charge-conserving population updates of column batches: ColumnBatch.time_dep_update /
nr_post_update (lwhip_batch_time_dep_update, lwhip_batch_nr_post_update; time_dep_kernel<true>, nr_post_kernel<true>).

Columns: pops_cases.build(levels, seed) with seeds 11, 12, 13 -- 70 depth points, more than one block at every block size
and a multiple of none.  Per case every column is held
  1. to its own oracle run within TOL = 1e-9, and to the longdouble reference by the second condition of
     test_pops_levels.accept (at most four times the oracle's error plus 64 eps);
  2. to a lone Context given the same Gamma, C, n and inputs: the same bits;
  3. in what it reports: dPops / dPopsMaxIdx are, exactly, the value and first-maximum index numpy forms from the populations
     downloaded before and after the call by the rule of Context._rel_diff_pops -- the same fp64 subtraction, division and
     absolute value on the same bits, so there is no tolerance --, and lwhip_batch_conv_records carries the same numbers.
The end-to-end test drives a time step's sub-iterations (formal solution, then time_dep_update against the populations of the
step's start) with retirement, against the same loop on the oracle; the CPU test of that loop holds the oracle's own stops
apart from popsTol by more than 1 %, so that a last-bit difference cannot move one.

Measured on an MI355X (hip against oracle / against longdouble as a multiple of the oracle's error): see CHANGELOG.md."""
import ctypes as C
import functools

import numpy as np
import pytest

import pops_cases as pc
from helpers import TOL_CONVERGED, rel_err
from lightweaver_amd import _abi as abi
from lightweaver_amd import batch as lb
from oracle.bindings import OracleContext
from test_pops_levels import TOL, accept, frozen

SEEDS = (11, 12, 13)
NS = pc.NSPACE
FILL = -7.25            # what the tests put into outputs that must not be written
IFILL = -77

TD_CASES = [pytest.param(tuple(l), dt, id='-'.join(map(str, l)) + f'-dt{dt}')
            for l in (pc.MIXED, [6, 6]) for dt in (1e-3, 0.1, 10.0)] + [pytest.param(tuple(pc.MIXED), (1e-3, 0.1, 10.0), id='mixed-dt-per-column')]
NR_CASES = [pytest.param(tuple(l), td, fdc, id='-'.join(map(str, l)) + ('-td' if td else '') + ('-dC' if fdc else ''))
            for l in ([3, 2, 5], [6, 6], [20, 19]) for td in (False, True) for fdc in (False, True)] \
    + [pytest.param((32, 31), True, True, id='32-31-td-dC')]


# ---- the rule of Context._rel_diff_pops, and helpers --------------------------------------------------------------------
def expected_change(new, old):
    """(max |(new - old) / new| over new != 0, flattened index of its first occurrence); (0.0, 0) if nothing changed."""
    new, old = np.asarray(new).reshape(-1), np.asarray(old).reshape(-1)
    ch = np.zeros_like(new)
    nz = new != 0.0
    ch[nz] = np.abs((new[nz] - old[nz]) / new[nz])
    i = int(np.argmax(ch))
    return float(ch[i]), i


def pops(p):
    return [a.n.copy() for a in p.atoms]


def dts_of(dt):
    return list(dt) if isinstance(dt, tuple) else [dt] * len(SEEDS)


def td_problem(levels, seed):
    return pc.build(list(levels), seed=seed)


def nr_problem(levels, seed):
    """(problem, stages, bg, ne, dC, nPrev): nr_inputs moves nTotal, so it belongs to the problem."""
    p = pc.build(list(levels), seed=seed, span=4.0)
    return (p,) + tuple(pc.nr_inputs(p))


@functools.lru_cache(maxsize=None)
def td_refs(levels, seed, dt):
    """(oracle, longdouble) populations of one column after time_dep_update of every atom."""
    p = td_problem(levels, seed)
    old = pc.old_pops(p)
    ref = [pc.ref_time_dep(a.Gamma, o, dt) for a, o in zip(p.atoms, old)]
    with OracleContext(p) as oc:
        for ia, o in enumerate(old):
            assert oc.time_dep_update(ia, o, dt) == 0
    return frozen(pops(p)), frozen(ref)


@functools.lru_cache(maxsize=None)
def nr_refs(levels, seed, timeDep, fdC):
    p, stages, bg, ne, dC, nPrev = nr_problem(levels, seed)
    atoms = list(range(len(levels)))
    kw = dict(dC=dC if fdC else None, nPrev=nPrev if timeDep else None, dt=pc.NR_DT, crsw=1.0)
    n, neNew = pc.ref_nr(p, atoms, stages, bg, ne, **kw)
    with OracleContext(p) as oc:
        assert oc.nr_post_update(atoms, stages, bg, ne, **kw) == 0
    return frozen(pops(p) + [ne]), frozen(list(n) + [neNew])


def open_batch(probs, mask=abi.GAMMA | abi.POPS, **kw):
    batch = lb.ColumnBatch(probs, device_profiles=False, **kw)
    if kw.get('fused', True):
        assert batch._batch is not None, 'the columns did not fuse: the batched kernels would not run'
    for c in batch.contexts:
        c.upload(mask)
    return batch


def conv_records(batch, fill=FILL):
    nSolved = sum(1 for a in batch.problems[0].atoms if not a.detailed)
    rec = np.full((len(batch), 2 + 2 * nSolved), fill)
    stride = C.c_int(0)
    lib = batch.contexts[0].lib
    assert lib.lwhip_batch_conv_records(batch._batch, rec.ctypes.data_as(abi.f64p), C.byref(stride)) == abi.OK
    assert stride.value == rec.shape[1]
    return rec


def check_reports(ups, rec, before, after, cols, atoms=None):
    """Condition 3 of the module docstring for the columns `cols`; atoms: the listed atoms (default all)."""
    for i in cols:
        listed = range(len(before[i])) if atoms is None else atoms
        assert ups[i].updatedPops and len(ups[i].dPops) == len(listed)
        for q, ia in enumerate(listed):
            v, idx = expected_change(after[i][ia], before[i][ia])
            assert (ups[i].dPops[q], ups[i].dPopsMaxIdx[q]) == (v, idx), (i, ia)
            if rec is not None:
                assert (rec[i, 2 + 2 * ia], rec[i, 3 + 2 * ia]) == (v, float(idx)), (i, ia)


def lone_time_dep(p, prev, dt):
    from lightweaver_amd.context import Context
    with Context(p) as ctx:
        ctx.time_dep_update(dt, prev)
    return pops(p)


def lone_nr(p, stages, bg, ne, **kw):
    from lightweaver_amd.context import Context
    with Context(p) as ctx:
        ctx.nr_post_update(stages, bg, ne, **kw)
    return pops(p)


def assert_same_bits(xs, ys, what=''):
    assert len(xs) == len(ys)
    for q, (x, y) in enumerate(zip(xs, ys)):
        assert np.array_equal(x, y), (what, q, float(np.max(np.abs(np.asarray(x) - np.asarray(y)))))


# ---- CPU ------------------------------------------------------------------------------------------------------------------
def test_abi_declares_both_entry_points_as_the_header_does():
    import os
    import re
    txt = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'lwhip.h')).read()
    sym = {name: (res, args) for name, res, args in abi.SYMBOLS}
    m = re.search(r'int lwhip_batch_time_dep_update\(lwhip_batch\* batch, const double\* const\* nOld, const double\* dt,\s*'
                  r'double\* dPops, int32_t\* dPopsMaxIdx\);', txt)
    assert m, 'lwhip_batch_time_dep_update is not declared with the signature of the issue'
    assert sym['lwhip_batch_time_dep_update'] == (C.c_int, [C.c_void_p, C.POINTER(abi.f64p), abi.f64p, abi.f64p, abi.i32p])
    m = re.search(r'int lwhip_batch_nr_post_update\(lwhip_batch\* batch, const lwhip_nr_args\* perColumn,\s*'
                  r'double\* dPops, int32_t\* dPopsMaxIdx\);', txt)
    assert m, 'lwhip_batch_nr_post_update is not declared with the signature of the issue'
    assert sym['lwhip_batch_nr_post_update'] == (C.c_int, [C.c_void_p, C.POINTER(abi.lwhip_nr_args), abi.f64p, abi.i32p])
    assert re.search(r'#define LWHIP_ABI_VERSION 4\b', txt) and abi.ABI_VERSION == 4


def test_pack_time_dep_lays_the_atoms_blocks_back_to_back():
    probs = [td_problem(pc.MIXED, s) for s in SEEDS]
    prev = [pc.old_pops(p) for p in probs]
    prev[1] = None                                  # (an inactive column needs none)
    ptrs, keep = lb.pack_time_dep(probs, [0, 2], prev)
    assert len(ptrs) == 3 and not ptrs[1] and keep[1] is None
    rows = sum(pc.MIXED)
    for i in (0, 2):
        got = np.ctypeslib.as_array(ptrs[i], (rows * NS,))
        off = 0
        for a, o in zip(probs[i].atoms, prev[i]):
            assert np.array_equal(got[off * NS:(off + a.Nlevel) * NS].reshape(a.Nlevel, NS), o)
            off += a.Nlevel
        assert off == rows
    with pytest.raises(ValueError):
        lb.pack_time_dep(probs, [0, 1], prev)       # an active column without populations
    with pytest.raises(ValueError):
        lb.pack_time_dep(probs, [0], [[o.T for o in prev[0]], None, None])


def test_pack_nr_args_is_one_block_per_active_column():
    cols = [nr_problem((3, 2, 5), s) for s in SEEDS]
    stages = cols[0][1]
    bg, ne, dC, nPrev = ([c[k] for c in cols] for k in (2, 3, 4, 5))
    arr, keep = lb.pack_nr_args(3, [0, 2], [0, 1, 2], stages, bg, ne, dC=dC, nPrev=None, dt=0.25, crsw=[1.0, 0.5, 0.75])
    assert len(arr) == 3 and keep[1] is None
    assert arr[1].Natoms == 0 and not arr[1].atoms and not arr[1].ne         # inactive: zeroed
    for i in (0, 2):
        a = arr[i]
        assert a.Natoms == 3 and [a.atoms[q] for q in range(3)] == [0, 1, 2]
        assert C.addressof(a.ne.contents) == ne[i].ctypes.data              # ne is updated in place: the caller's array
        assert np.array_equal(np.ctypeslib.as_array(a.backgroundNe, (NS,)), bg[i])
        assert not a.nPrev and a.dt == 0.25 and a.crsw == [1.0, 0.5, 0.75][i]
        for q, N in enumerate((3, 2, 5)):
            assert np.array_equal(np.ctypeslib.as_array(a.stages[q], (N,)), stages[q])
            assert np.array_equal(np.ctypeslib.as_array(a.dC[q], (N, N, NS)), dC[i][q])


# the time step of the end-to-end tests: sub-iterations until the column's own max dPops < popsTol
E2E_SEEDS = (100, 102, 107)
E2E_DT, E2E_PTOL, E2E_NSUB = 1e-3, 0.15, 14


@functools.lru_cache(maxsize=None)
def e2e_oracle(seed):
    """The sub-iterations of one time step on the oracle: per sub-iteration formal_sol_gamma_matrices, then time_dep_update
    of every solved atom against the populations of the step's start.  {stop, trace of max dPops, n at the stop}."""
    from test_batch_converge import column
    from test_iterate import OracleLoopContext
    q = column(seed)
    oc = OracleLoopContext(q)
    act = [ia for ia, a in enumerate(q.atoms) if not a.detailed]
    prev = [q.atoms[ia].n.copy() for ia in act]
    trace, stop = [], None
    for it in range(E2E_NSUB):
        oc.formal_sol_gamma_matrices()
        before = [q.atoms[ia].n.copy() for ia in act]
        for k, ia in enumerate(act):
            assert oc.oc.time_dep_update(ia, prev[k], E2E_DT) == 0
        trace.append(max(expected_change(q.atoms[ia].n, b)[0] for ia, b in zip(act, before)))
        if trace[-1] < E2E_PTOL:
            stop = it
            break
    assert stop is not None
    return dict(stop=stop, trace=trace, n=frozen(pops(q)))


def test_oracle_time_steps_stop_apart_and_are_not_fragile():
    stops = [e2e_oracle(s)['stop'] for s in E2E_SEEDS]
    print('oracle stop sub-iterations', stops)
    assert len(set(stops)) == len(stops), stops
    for s in E2E_SEEDS:
        for it, d in enumerate(e2e_oracle(s)['trace']):
            assert not 0.99 * E2E_PTOL < d < 1.01 * E2E_PTOL, (s, it, d)


# ---- GPU: time_dep_update -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('levels,dt', TD_CASES)
def test_hip_batch_time_dep(gpu, levels, dt):
    probs = [td_problem(levels, s) for s in SEEDS]
    prev = [pc.old_pops(p) for p in probs]
    before = [pops(p) for p in probs]
    with open_batch(probs) as batch:
        ups = batch.time_dep_update(dt if isinstance(dt, tuple) else dt, prev)
        rec = conv_records(batch)
        batch.download(abi.POPS)
    after = [pops(p) for p in probs]
    check_reports(ups, rec, before, after, range(3))
    for i, s in enumerate(SEEDS):
        ora, ref = td_refs(levels, s, dts_of(dt)[i])
        accept(f'batch time_dep {list(levels)} dt={dts_of(dt)[i]} seed={s}', after[i], ora, ref)
        assert_same_bits(after[i], lone_time_dep(td_problem(levels, s), prev[i], dts_of(dt)[i]), f'lone context, column {i}')


@pytest.mark.gpu
def test_hip_batch_time_dep_tie_across_blocks_and_zeros(gpu):
    """Column 0: per atom the depth with the largest change is moved to depth 5 and copied to depth 61 (Gamma, n, nOld): two
    blocks, at every block size, report the same value and the first index must win.  Column 1: Gamma = 0 and nOld = n, so
    the update changes nothing and reports (0.0, 0).  Column 2 is an ordinary one."""
    levels, dt = tuple(pc.MIXED), 0.1
    probs = [td_problem(levels, s) for s in SEEDS]
    prev = [pc.old_pops(p) for p in probs]
    want = []
    for a, o, new in zip(probs[0].atoms, prev[0], td_refs(levels, SEEDS[0], dt)[0]):
        v, idx = expected_change(new, a.n)
        lvl, k = divmod(idx, NS)
        for arr in (a.Gamma, a.n, o):
            arr[..., [5, k]] = arr[..., [k, 5]]
            arr[..., 61] = arr[..., 5]
        want.append(lvl * NS + 5)
    for a in probs[1].atoms:
        a.Gamma[...] = 0.0
    prev[1] = pops(probs[1])
    before = [pops(p) for p in probs]
    with open_batch(probs) as batch:
        ups = batch.time_dep_update(dt, prev)
        rec = conv_records(batch)
        batch.download(abi.POPS)
    after = [pops(p) for p in probs]
    check_reports(ups, rec, before, after, range(3))
    assert list(ups[0].dPopsMaxIdx) == want
    for ia, a in enumerate(probs[0].atoms):
        assert np.array_equal(a.n[:, 5], a.n[:, 61])
        assert expected_change(a.n[:, 61], before[0][ia][:, 61])[0] == ups[0].dPops[ia]      # the tie is there
    assert ups[1].dPops == [0.0] * 4 and ups[1].dPopsMaxIdx == [0] * 4
    assert_same_bits(after[1], before[1])


@pytest.mark.gpu
def test_hip_batch_time_dep_active_set(gpu):
    """Columns {0, 2} active: column 1 keeps its n, its dPops row and record row; 0 and 2 land on the bits of the all-active
    call from the same start; returning to all columns works."""
    levels, dt = tuple(pc.MIXED), 0.1
    probs = [td_problem(levels, s) for s in SEEDS]
    prev = [pc.old_pops(p) for p in probs]
    start = [pops(p) for p in probs]
    with open_batch(probs) as batch:
        lib = batch.contexts[0].lib
        upsAll = batch.time_dep_update(dt, prev)
        batch.download(abi.POPS)
        allActive = [pops(p) for p in probs]
        for p, c, n0 in zip(probs, batch.contexts, start):
            for a, x in zip(p.atoms, n0):
                a.n[...] = x
            c.upload(abi.POPS)
        batch.set_active([0, 2])
        ptrs, keep = lb.pack_time_dep(probs, [0, 2], [prev[0], None, prev[2]])
        dP, dI = np.full((3, 4), FILL), np.full((3, 4), IFILL, dtype=np.int32)
        dts = np.full(3, dt)
        assert lib.lwhip_batch_time_dep_update(batch._batch, ptrs, dts.ctypes.data_as(abi.f64p), dP.ctypes.data_as(abi.f64p),
                                               dI.ctypes.data_as(abi.i32p)) == abi.OK
        rec = conv_records(batch)
        batch.download(abi.POPS)
        part = [pops(p) for p in probs]
        assert_same_bits(part[1], start[1], 'the retired column')
        assert np.all(dP[1] == FILL) and np.all(dI[1] == IFILL) and np.all(rec[1] == FILL)
        for i in (0, 2):
            assert_same_bits(part[i], allActive[i], f'column {i}')
            assert list(dP[i]) == upsAll[i].dPops and list(dI[i]) == upsAll[i].dPopsMaxIdx
        ups = batch.time_dep_update(dt, [prev[0], None, prev[2]])
        assert ups[1] is None and ups[0] is not None and ups[2] is not None
        batch.set_active(None)
        ups = batch.time_dep_update(dt, prev)
        batch.download(abi.POPS)
        assert all(u is not None for u in ups)
        assert not np.array_equal(probs[1].atoms[0].n, start[1][0])
        ora, ref = td_refs(levels, SEEDS[1], dt)
        accept('batch time_dep, column 1 after returning to all columns', pops(probs[1]), ora, ref)


def zero_row(p, dt, atom, k=7):
    """One all-zero row of (1 - dt Gamma) at depth k of `atom`: the diagonal entry 1 / dt (1 - g dt is then exactly 0 for the
    dt = 0.5 used here), the others 0."""
    G = p.atoms[atom].Gamma
    G[1, :, k] = 0.0
    G[1, 1, k] = 1.0 / dt
    assert 1.0 - G[1, 1, k] * dt == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize('atom', [0, 1], ids=['registers', 'lds'])
def test_hip_batch_time_dep_singular_column(gpu, atom):
    """Column 1 has a zero row at depth 7 of one atom (3 levels: the register path; 9: LDS).  The call raises
    ExplodingMatrixError; that point keeps its n, and every other point of every column holds the lone context's bits."""
    from lightweaver_amd.context import Context, ExplodingMatrixError
    levels, dt = (3, 9), 0.5
    probs = [td_problem(levels, s) for s in SEEDS]
    prev = [pc.old_pops(p) for p in probs]
    zero_row(probs[1], dt, atom)
    before = [pops(p) for p in probs]
    with open_batch(probs) as batch:
        lib = batch.contexts[0].lib
        ptrs, keep = lb.pack_time_dep(probs, [0, 1, 2], prev)
        dP, dI = np.full((3, 2), FILL), np.full((3, 2), IFILL, dtype=np.int32)
        dts = np.full(3, dt)
        st = lib.lwhip_batch_time_dep_update(batch._batch, ptrs, dts.ctypes.data_as(abi.f64p), dP.ctypes.data_as(abi.f64p),
                                             dI.ctypes.data_as(abi.i32p))
        assert st == abi.ERR_SINGULAR and np.all(dP == FILL) and np.all(dI == IFILL)
        batch.download(abi.POPS)
        after = [pops(p) for p in probs]
        # ... and the status is consumed: the same call on the Python level raises, then a sound batch runs
        for p, c, n0 in zip(probs, batch.contexts, before):
            for a, x in zip(p.atoms, n0):
                a.n[...] = x
            c.upload(abi.POPS)
        with pytest.raises(ExplodingMatrixError):
            batch.time_dep_update(dt, prev)
    for i, s in enumerate(SEEDS):
        q = td_problem(levels, s)
        if i == 1:
            zero_row(q, dt, atom)
        with Context(q) as ctx:         # (atom by atom: the lone call stops at the atom that is singular)
            ctx.upload(abi.GAMMA | abi.POPS)
            for ia in range(len(levels)):
                if i == 1 and ia == atom:
                    with pytest.raises(ExplodingMatrixError):
                        ctx.time_dep_update(dt, prev[i], deviceResident=True, atom=ia)
                else:
                    ctx.time_dep_update(dt, prev[i], deviceResident=True, atom=ia)
            ctx.download(abi.POPS)
        assert_same_bits(after[i], pops(q), f'column {i}')
    assert np.array_equal(after[1][atom][:, 7], before[1][atom][:, 7])
    assert not np.array_equal(after[1][atom][:, 8], before[1][atom][:, 8])


@pytest.mark.gpu
def test_hip_batch_time_dep_leaves_ng_alone(gpu):
    levels, dt = (6, 6), 0.1
    probs = [td_problem(levels, s) for s in SEEDS]
    prev = [pc.old_pops(p) for p in probs]
    with open_batch(probs) as batch:
        batch.configure_ng(2, 3, 5)
        st0 = batch.ng_state()
        batch.time_dep_update(dt, prev)
        assert batch.ng_state() == st0 and st0['counts'] == [1, 1, 1]
        batch.download(abi.POPS)
    withNg = [pops(p) for p in probs]
    probs = [td_problem(levels, s) for s in SEEDS]
    with open_batch(probs) as batch:
        batch.time_dep_update(dt, prev)
        batch.download(abi.POPS)
    for i, p in enumerate(probs):
        assert_same_bits(withNg[i], pops(p), f'column {i}')


# ---- GPU: nr_post_update --------------------------------------------------------------------------------------------------
def run_batch_nr(cols, timeDep, fdC, active=None, **kw):
    """One batched step on the columns `cols` (nr_problem tuples): (ups, records, before, after, ne after)."""
    probs = [c[0] for c in cols]
    stages = cols[0][1]
    bg, ne, dC, nPrev = ([c[k] for c in cols] for k in (2, 3, 4, 5))
    before = [pops(p) for p in probs]
    with open_batch(probs, abi.GAMMA | abi.POPS | abi.COLLISIONS, **kw) as batch:
        if active is not None:
            batch.set_active(active)
        ups = batch.nr_post_update(stages, bg, ne, dC=dC if fdC else None, nPrev=nPrev if timeDep else None, dt=pc.NR_DT)
        rec = conv_records(batch) if batch._batch is not None else None
        batch.download(abi.POPS)
    return ups, rec, before, [pops(p) for p in probs], ne


@pytest.mark.gpu
@pytest.mark.parametrize('levels,timeDep,fdC', NR_CASES)
def test_hip_batch_nr(gpu, levels, timeDep, fdC):
    cols = [nr_problem(levels, s) for s in SEEDS]
    ups, rec, before, after, ne = run_batch_nr(cols, timeDep, fdC)
    check_reports(ups, rec, before, after, range(3))
    for i, s in enumerate(SEEDS):
        ora, ref = nr_refs(levels, s, timeDep, fdC)
        accept(f'batch nr {list(levels)} timeDep={timeDep} fdC={fdC} seed={s}', after[i] + [ne[i]], list(ora), list(ref))
        p, stages, bg, ne1, dC, nPrev = nr_problem(levels, s)
        lone = lone_nr(p, stages, bg, ne1, dC=dC if fdC else None, nPrev=nPrev if timeDep else None, dt=pc.NR_DT)
        assert_same_bits(after[i] + [ne[i]], lone + [ne1], f'lone context, column {i}')


@pytest.mark.gpu
def test_hip_batch_nr_active_set_and_listed_atoms(gpu):
    """Columns {0, 2} active, atoms [0, 2] of [3, 2, 5] listed: column 1's n and ne are untouched, atom 1 of every column is
    untouched and has no report, and 0 and 2 land on the bits of a lone context given the same list."""
    levels = (3, 2, 5)
    cols = [nr_problem(levels, s) for s in SEEDS]
    probs = [c[0] for c in cols]
    stages = [cols[0][1][0], cols[0][1][2]]
    bg = [c[2] for c in cols]
    ne = [c[3] for c in cols]
    ne[1] = np.full(NS, FILL)
    nPrev = [[c[5][0], c[5][2]] for c in cols]
    before = [pops(p) for p in probs]
    with open_batch(probs, abi.GAMMA | abi.POPS | abi.COLLISIONS) as batch:
        batch.set_active([0, 2])
        ups = batch.nr_post_update(stages, bg, ne, nPrev=nPrev, dt=pc.NR_DT, atoms=[0, 2])
        rec = conv_records(batch)
        batch.download(abi.POPS)
    after = [pops(p) for p in probs]
    assert ups[1] is None and np.all(ne[1] == FILL) and np.all(rec[1] == FILL)
    assert_same_bits(after[1], before[1], 'the retired column')
    check_reports(ups, rec, before, after, (0, 2), atoms=[0, 2])
    for i in (0, 2):
        assert np.array_equal(after[i][1], before[i][1]) and (rec[i, 4], rec[i, 5]) == (0.0, 0.0)
        p, _, bg1, ne1, _, _ = nr_problem(levels, SEEDS[i])
        lone = lone_nr(p, stages, bg1, ne1, nPrev=nPrev[i], dt=pc.NR_DT, atoms=[0, 2])
        assert_same_bits(after[i] + [ne[i]], lone + [ne1], f'lone context, column {i}')


@pytest.mark.gpu
def test_hip_batch_nr_singular_column(gpu):
    """The time-dependent Jacobian dt Gamma - 1 of column 1 gets a zero row at depth 7 (off-diagonals 0, the diagonal of
    Gamma 1 / dt, no continuum from that level and no dC): ExplodingMatrixError; the point keeps n and ne, everything else
    -- ne of every column included -- holds the lone context's bits."""
    from lightweaver_amd.context import Context, ExplodingMatrixError
    levels, dt = (3, 2, 5), 0.5

    def make(s, bad):
        p, stages, bg, ne, dC, nPrev = nr_problem(levels, s)
        if bad:
            G = p.atoms[0].Gamma          # level 1 of 3: odd, so no continuum starts there; not the atom's last equation
            G[1, :, 7] = 0.0
            G[1, 1, 7] = 1.0 / dt
            assert -G[1, 1, 7] * (-1.0 * dt) - 1.0 == 0.0
        return p, stages, bg, ne, dC, nPrev
    cols = [make(s, i == 1) for i, s in enumerate(SEEDS)]
    probs = [c[0] for c in cols]
    ne0 = [c[3].copy() for c in cols]
    before = [pops(p) for p in probs]
    with open_batch(probs, abi.GAMMA | abi.POPS | abi.COLLISIONS) as batch:
        with pytest.raises(ExplodingMatrixError):
            batch.nr_post_update(cols[0][1], [c[2] for c in cols], [c[3] for c in cols], nPrev=[c[5] for c in cols], dt=dt)
        batch.download(abi.POPS)
    after = [pops(p) for p in probs]
    for i, s in enumerate(SEEDS):
        p, stages, bg, ne1, dC, nPrev = make(s, i == 1)
        with Context(p) as ctx:
            if i == 1:
                with pytest.raises(ExplodingMatrixError):
                    ctx.nr_post_update(stages, bg, ne1, nPrev=nPrev, dt=dt)
                ctx.download(abi.POPS)
            else:
                ctx.nr_post_update(stages, bg, ne1, nPrev=nPrev, dt=dt)
        assert_same_bits(after[i] + [cols[i][3]], pops(p) + [ne1], f'column {i}')
    assert cols[1][3][7] == ne0[1][7] and all(np.array_equal(a[:, 7], b[:, 7]) for a, b in zip(after[1], before[1]))
    assert cols[1][3][8] != ne0[1][8]


# ---- GPU: refusals, before anything is queued -----------------------------------------------------------------------------
@pytest.mark.gpu
def test_hip_batch_pops_refusals(gpu):
    levels = (3, 2, 5)
    cols = [nr_problem(levels, s) for s in SEEDS]
    probs = [c[0] for c in cols]
    probs[1].atoms[1].C = None                      # (column 1, atom 1: no collisional rates)
    prev = [pc.old_pops(p) for p in probs]
    stages = cols[0][1]
    bg, ne, dC, nPrev = ([c[k] for c in cols] for k in (2, 3, 4, 5))
    neFill = [np.full(NS, FILL) for _ in cols]
    start = [pops(p) for p in probs]
    with open_batch(probs, abi.GAMMA | abi.POPS | abi.COLLISIONS) as batch:
        lib, h = batch.contexts[0].lib, batch._batch
        dP, dI = np.full((3, 3), FILL), np.full((3, 3), IFILL, dtype=np.int32)
        out = (dP.ctypes.data_as(abi.f64p), dI.ctypes.data_as(abi.i32p))
        dts = np.full(3, 0.1)
        dtp = dts.ctypes.data_as(abi.f64p)
        ptrs, keep = lb.pack_time_dep(probs, [0, 1, 2], prev)
        err = lambda: lib.lwhip_last_error().decode()       # noqa: E731

        def td(*a):
            return lib.lwhip_batch_time_dep_update(*a, *out)

        def nr(arr, hh=h):
            return lib.lwhip_batch_nr_post_update(hh, arr, *out)

        def args(active=(0, 1, 2), atoms=(0, 2), st=None, **kw):
            """perColumn over the fill ne arrays: nothing a refused call could write into is the test's data."""
            st = [stages[q] for q in atoms] if st is None else st
            pick = lambda lst, i: None if lst is None else [lst[i][q] for q in atoms]     # noqa: E731
            k = dict(dC=None, nPrev=None)
            k.update(kw)
            arr = (abi.lwhip_nr_args * 3)()
            held = []
            for i in active:
                a1, k1 = abi.make_nr_args(list(atoms), st, bg[i], neFill[i], dC=pick(k['dC'], i), nPrev=pick(k['nPrev'], i), dt=0.1)
                arr[i] = a1
                held.append((a1, k1))
            return arr, held

        # time_dep_update
        assert td(None, ptrs, dtp) == abi.ERR_INVALID
        assert td(h, None, dtp) == abi.ERR_INVALID and td(h, ptrs, None) == abi.ERR_INVALID
        gap, _ = lb.pack_time_dep(probs, [0, 2], [prev[0], None, prev[2]])
        assert td(h, gap, dtp) == abi.ERR_INVALID and 'column 1' in err()
        # nr_post_update
        good, g0 = args()
        assert nr(good, None) == abi.ERR_INVALID and nr(None) == abi.ERR_INVALID
        for field in ('stages', 'ne', 'backgroundNe', 'atoms'):
            arr, held = args()
            setattr(abi.raw_view(arr[2]), field, None)
            assert nr(arr) == abi.ERR_INVALID and 'column 2' in err(), field
        arr, held = args(atoms=(0, 3), st=[stages[0], stages[0]])
        assert nr(arr) == abi.ERR_INVALID                                   # out of range
        arr, held = args(atoms=(0, 1))
        assert nr(arr) == abi.ERR_INVALID and 'column 1' in err() and 'collisional' in err()      # no C
        arr, held = args()
        abi.raw_view(arr[1]).Natoms = 1
        assert nr(arr) == abi.ERR_INVALID and 'column 1' in err()
        arr, held = args()
        other, h2 = args(atoms=(2, 0), st=[stages[2], stages[0]])
        arr[2] = other[2]
        assert nr(arr) == abi.ERR_INVALID and 'column 2' in err()           # another atom list
        arr, held = args()
        withdc, h3 = args(dC=dC)
        arr[1] = withdc[1]
        assert nr(arr) == abi.ERR_INVALID and 'column 1' in err()           # dC in one column only
        arr, held = args(nPrev=nPrev)
        arr[2] = good[2]
        assert nr(arr) == abi.ERR_INVALID and 'column 2' in err()           # nPrev missing in one column
        # nothing was written, nothing ran
        assert np.all(dP == FILL) and np.all(dI == IFILL) and all(np.all(x == FILL) for x in neFill)
        batch.download(abi.POPS)
        for p, n0 in zip(probs, start):
            assert_same_bits(pops(p), n0)
        # ... and the batch still works: the columns that have C, with atoms (0, 2)
        arr, held = args()
        for i in range(3):
            neFill[i][...] = ne[i]
        assert nr(arr) == abi.OK and not np.any(dP[:, [0, 2]] == FILL) and np.all(dP[:, 1] == FILL)


@pytest.mark.gpu
def test_hip_batch_nr_refuses_a_detailed_atom_and_65_equations(gpu):
    from lightweaver_amd.context import LwHipError
    cols = [nr_problem((3, 2, 5), s) for s in SEEDS]
    for c in cols:
        c[0].atoms[2].detailed = True
    ne = [np.full(NS, FILL) for _ in cols]
    with open_batch([c[0] for c in cols], abi.GAMMA | abi.POPS | abi.COLLISIONS) as batch:
        with pytest.raises(LwHipError, match='not an active atom'):
            batch.nr_post_update(cols[0][1], [c[2] for c in cols], ne, atoms=[0, 1, 2])
    assert all(np.all(x == FILL) for x in ne)
    cols = [(pc.build([32, 32], 3, seed=s, span=4.0),) for s in SEEDS]
    cols = [c + tuple(pc.nr_inputs(c[0])) for c in cols]
    ne = [np.full(3, FILL) for _ in cols]
    with open_batch([c[0] for c in cols], abi.GAMMA | abi.POPS | abi.COLLISIONS) as batch:
        with pytest.raises(LwHipError, match=r'failed \(%d\).*63 coupled levels' % abi.ERR_UNSUPPORTED):
            batch.nr_post_update(cols[0][1], [c[2] for c in cols], ne)
    assert all(np.all(x == FILL) for x in ne)


# ---- GPU: the per-column route of a batch that is not fused ---------------------------------------------------------------
@pytest.mark.gpu
def test_hip_unfused_batch_gives_the_same_numbers_and_reports(gpu):
    levels, dt = tuple(pc.MIXED), 0.1
    probs = [td_problem(levels, s) for s in SEEDS]
    prev = [pc.old_pops(p) for p in probs]
    before = [pops(p) for p in probs]
    with open_batch(probs, fused=False) as batch:
        assert batch._batch is None
        batch.set_active([0, 2])
        ups = batch.time_dep_update(dt, prev)
        after = [pops(p) for p in probs]
    assert ups[1] is None
    assert_same_bits(after[1], before[1])
    check_reports(ups, None, before, after, (0, 2))
    for i in (0, 2):
        assert max(rel_err(x, o) for x, o in zip(after[i], td_refs(levels, SEEDS[i], dt)[0])) <= TOL
    nl = (3, 2, 5)
    cols = [nr_problem(nl, s) for s in SEEDS]
    ups, _, before, after, ne = run_batch_nr(cols, True, True, fused=False)
    check_reports(ups, None, before, after, range(3))
    for i, s in enumerate(SEEDS):
        ora = nr_refs(nl, s, True, True)[0]
        assert max(rel_err(x, o) for x, o in zip(after[i] + [ne[i]], ora)) <= TOL


# ---- GPU: a time step's sub-iterations with retirement, against the oracle loop -------------------------------------------
@pytest.mark.gpu
def test_hip_batch_time_step_with_retirement_matches_oracle_loops(gpu):
    from test_batch_converge import column
    probs = [column(s) for s in E2E_SEEDS]
    want = [e2e_oracle(s)['stop'] for s in E2E_SEEDS]
    prev = [[a.n.copy() for a in p.atoms if not a.detailed] for p in probs]
    stops, kept = [None] * 3, [None] * 3
    with lb.ColumnBatch(probs) as batch:
        assert batch._batch is not None
        pending = [0, 1, 2]
        for it in range(E2E_NSUB):
            batch.formal_sol_gamma_matrices(sync_host=False)
            ups = batch.time_dep_update(E2E_DT, [prev[i] if i in pending else None for i in range(3)])
            assert [u is not None for u in ups] == [i in pending for i in range(3)]
            done = [i for i in pending if max(ups[i].dPops) < E2E_PTOL]
            print('sub-iteration', it, [None if u is None else max(u.dPops) for u in ups], [e2e_oracle(s)['trace'][it:it + 1] for s in E2E_SEEDS])
            for i in done:
                stops[i] = it
                batch.contexts[i].download(abi.POPS)
                kept[i] = pops(probs[i])
            pending = [i for i in pending if i not in done]
            if not pending:
                break
            if done:
                batch.set_active(pending)
        batch.set_active(None)
        batch.download(abi.POPS)
    assert stops == want
    for i, s in enumerate(E2E_SEEDS):
        assert_same_bits(pops(probs[i]), kept[i], f'retired column {i}')
        errs = [rel_err(a.n, x) for a, x in zip(probs[i].atoms, e2e_oracle(s)['n'])]
        print('seed', s, 'stop', stops[i], 'n rel', errs)
        assert max(errs) <= TOL_CONVERGED
