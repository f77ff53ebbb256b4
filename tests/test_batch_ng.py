"""Ng acceleration for column batches (lwhip_batch_ng_configure / _accelerate / _state; ColumnBatch.configure_ng, ng_accelerate,
ng_state, iterate_to_convergence(ng=...)): every column of a batch behaves as a lone Context with configure_ng does -- both run
ng_kernel, a lone context as a batch of one column.

Columns: the batch tests' perturbed FAL-C columns with dT = 0.1 (with the dT = 0.3 of test_batch_converge.py the oracle's own Ng
loop ends in "Singular Matrix" for three seeds), H(6) + Ca II(6), 3 rays, NgOptions(2, 3, 5).  On the CPU oracle these stop at
iterations 26, 26, 23, 32, 29 (plain MALI: 40, 38, 29, 37, 34) and accelerate at 6, 9, 12, ...; a relative 1e-9 perturbation of
the starting populations moves no stop and the final dJMax / dPops by at most 5.5e-7 / 7.5e-7 relative, so the device's
1e-10-level differences stay well inside the project's bounds for this comparison (dJMax rel 1e-6, dPops rtol 1e-5, states
TOL_CONVERGED).  The Ng step itself is held, for the lone context and for the batch, to the bits recorded from lone contexts
before the two routes shared a kernel (tests/golden/ng_step_bits.json, tools/record_ng_bits.py); the comparison of batch and lone
context bit for bit now guards the column addressing, the history stride and the compacted list."""
import ctypes as C
import functools

import numpy as np
import pytest

import ng_cases
from helpers import TOL_CONVERGED, rel_err
from lightweaver_amd import _abi as abi
from lightweaver_amd.batch import ColumnBatch
from lightweaver_amd.context import ExplodingMatrixError
from lightweaver_amd.iterate import iterate_ctx_se
from oracle import bindings
from test_batch_converge import OracleBatch, same_bits, snapshot
from ng_cases import SEEDS, Synthetic, column, get, lone_ng, put
from test_iterate import OracleLoopContext

NG = (2, 3, 5)
JTOL, PTOL, NSCATTER, NMAX = 5e-2, 3e-2, 3, 60
KW = dict(Nscatter=NSCATTER, NmaxIter=NMAX, JTol=JTOL, popsTol=PTOL)


@functools.lru_cache(maxsize=None)
def oracle_trace(seed):
    """iterate_ctx_se's loop on the oracle with Ng, every iteration's numbers kept: per iteration (dJMax, dPops, dPopsMaxIdx,
    ngAccelerated), the stop iteration, J and n at the stop.  Computed once and never modified."""
    q = column(seed)
    oc = OracleLoopContext(q, ng=NG)
    trace, stop = [], None
    for it in range(NMAX):
        Ju = oc.formal_sol_gamma_matrices()
        if it < NSCATTER:
            trace.append((Ju.dJMax, None, None, False))
            continue
        Pu = oc.stat_equil()
        trace.append((Ju.dJMax, list(Pu.dPops), list(Pu.dPopsMaxIdx), bool(Pu.ngAccelerated)))
        if Ju.dJMax < JTOL and max(Pu.dPops) < PTOL:
            stop = it
            break
    assert stop is not None
    out = dict(stop=stop, trace=trace, J=q.J.copy(), n=[a.n.copy() for a in q.atoms],
               accelerated=[it for it, t in enumerate(trace) if t[3]])
    out['J'].setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def plain_converged_by(seed, last):
    """Whether plain MALI on the oracle converges at an iteration <= last (its stop is above `last` iff it does not)."""
    oc = OracleLoopContext(column(seed))
    for it in range(last + 1):
        Ju = oc.formal_sol_gamma_matrices()
        if it < NSCATTER:
            continue
        Pu = oc.stat_equil()
        if Ju.dJMax < JTOL and max(Pu.dPops) < PTOL:
            return True
    return False


class NgOracleContext(OracleLoopContext):
    """... with Context.configure_ng / ng_state: the oracle's Ng keeps its count to itself, so the calls are counted here."""

    def configure_ng(self, Norder=0, Nperiod=0, Ndelay=0):
        self.ng = [bindings.NgHandle('oracle', Norder, Nperiod, Ndelay, sol=a.n) for a in self.prob.atoms if not a.detailed]
        self._state = dict(options=(Norder, Nperiod, max(Ndelay, Nperiod + 2)), count=1, lastAccelerated=False)

    def stat_equil(self, deviceResident=False):
        up = super().stat_equil(deviceResident)
        self._state['count'] += 1
        self._state['lastAccelerated'] = bool(up.ngAccelerated)
        return up

    def ng_state(self):
        return dict(self._state)


class NgOracleBatch(OracleBatch):
    """OracleBatch whose columns take configure_ng: what ColumnBatch.configure_ng calls on an unfused batch."""

    def __init__(self, problems):
        super().__init__(problems)
        self.contexts = [NgOracleContext(p) for p in self.problems]


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_oracle_ng_traces_preconditions():
    stops = {s: oracle_trace(s)['stop'] for s in SEEDS}
    print('oracle stop iterations with Ng', stops)
    assert len(set(stops.values())) >= 3, stops
    for s in SEEDS:
        tr = oracle_trace(s)
        # plain MALI has not converged by the iteration Ng stops at: every stop is below the column's plain stop
        assert not plain_converged_by(s, tr['stop']), s
        assert tr['accelerated'] == list(range(6, tr['stop'] + 1, 3)), (s, tr['accelerated'])
        for it, (dJ, dP, _, _) in enumerate(tr['trace']):
            if dP is None:
                continue
            p = max(dP)
            nearJ = 0.99 * JTOL < dJ < 1.01 * JTOL and p < 1.01 * PTOL
            nearP = 0.99 * PTOL < p < 1.01 * PTOL and dJ < 1.01 * JTOL
            assert not (nearJ or nearP), (s, it, dJ, p)
    assert iterate_ctx_se(OracleLoopContext(column(SEEDS[2]), ng=NG), **KW) == stops[SEEDS[2]]


def test_iterate_to_convergence_with_ng_on_oracle_columns():
    probs = [column(s) for s in SEEDS]
    batch = NgOracleBatch(probs)
    acc = [[] for _ in SEEDS]

    def cb(it, J, P, act):
        for i, u in enumerate(P or []):
            if u is not None and u.ngAccelerated:
                acc[i].append(it)

    res = batch.iterate_to_convergence(ng=NG, callback=cb, **KW)
    want = [oracle_trace(s)['stop'] for s in SEEDS]
    assert res.iterations == want and res.converged == [True] * len(SEEDS)
    assert batch.ng_state()['options'] == NG
    assert batch.ng_state()['counts'] == [w - 1 for w in want]     # (configure: 1; one call per iteration 3 .. stop)
    for i, (s, p, fin) in enumerate(zip(SEEDS, probs, res.final)):
        tr = oracle_trace(s)
        assert np.array_equal(p.J, tr['J']) and all(np.array_equal(a.n, n) for a, n in zip(p.atoms, tr['n']))
        assert fin[0].dJMax == tr['trace'][tr['stop']][0] and fin[1].dPops == tr['trace'][tr['stop']][1]
        assert acc[i] == tr['accelerated'], (s, acc[i])


# ---- GPU ----------------------------------------------------------------------------------------------------------------
class Twins:
    """A fused batch of 3 columns and one lone Context per column, fed the same vectors."""

    def __init__(self, Nspace, problem='HCa', fused=True):
        from lightweaver_amd.context import Context
        seeds = SEEDS[:3]
        self.probs = [column(s, Nspace, problem) for s in seeds]
        self.lprobs = [column(s, Nspace, problem) for s in seeds]
        self.batch = ColumnBatch(self.probs, fused=fused)
        assert (self.batch._batch is not None) == fused
        self.lones = [Context(p) for p in self.lprobs]
        self.nAtoms = len(self.probs[0].atoms)
        self.gold, self.stepNo = None, 0

    def close(self):
        for c in self.lones:
            c.close()
        self.batch.close()

    def seed(self, syn, opts, gold=None):
        """gold: the recorded sequence (ng_cases.golden) that the steps from here on are held to, step 1 first."""
        self.gold, self.stepNo = gold, 0
        if gold is not None:
            ng_cases.check_inputs(gold, syn)
        for i in range(3):
            put(self.batch.contexts[i], self.probs[i], syn.x0[i])
            put(self.lones[i], self.lprobs[i], syn.x0[i])
            self.lones[i].configure_ng(*opts)
        self.batch.configure_ng(*opts)
        return [[x.copy() for x in syn.x0[i]] for i in range(3)]

    def step(self, syn, xs, cols=(0, 1, 2), oracle=None, worst=None):
        """Advance the sequences of `cols`, upload, one Ng step on batch and lone contexts; everything equal bit for bit, and
        (seeded with a recorded sequence) both equal to the recorded bits of this step.  Returns the new vectors (the batch's n)."""
        self.stepNo += 1
        for i in cols:
            xs[i] = syn.advance(i, xs[i])
            put(self.batch.contexts[i], self.probs[i], xs[i])
            put(self.lones[i], self.lprobs[i], xs[i])
        ups = self.batch.ng_accelerate()
        assert [u is not None for u in ups] == [i in cols for i in range(3)]
        for i in cols:
            st, acc, dP, dI = lone_ng(self.lones[i], self.nAtoms)
            assert st == abi.OK
            nb, nl = get(self.batch.contexts[i], self.probs[i]), get(self.lones[i], self.lprobs[i])
            assert all(np.array_equal(a, b) for a, b in zip(nb, nl)), i
            assert ups[i].ngAccelerated == acc and ups[i].dPops == dP and ups[i].dPopsMaxIdx == dI, (i, ups[i], acc, dP, dI)
            if self.gold is not None:
                ng_cases.check_step(self.gold, i, self.stepNo, 'lone', nl, acc, dP, dI)
                ng_cases.check_step(self.gold, i, self.stepNo, 'batch', nb, ups[i].ngAccelerated, ups[i].dPops, ups[i].dPopsMaxIdx)
            if oracle is not None:
                for q, g in enumerate(oracle[i]):
                    xo = np.ascontiguousarray(xs[i][q]).copy()
                    assert g.accelerate(xo) == acc, (i, q)
                    assert g.max_change()[1] == dI[q], (i, q)
                    worst[0] = max(worst[0], rel_err(nb[q], xo))
                    worst[1] = max(worst[1], rel_err(nl[q], xo))
            xs[i] = nb
        return xs


@pytest.mark.gpu
@pytest.mark.parametrize('Nspace', [13, 32, 82])
def test_ng_step_matches_the_lone_context_bit_for_bit(gpu, Nspace):
    """L = 6 Nspace = 78, 192, 492: a partial last chunk of 64, none, the usual size.  Norder 1 extrapolates on every call
    from the second on; Norder 6 has 42 weighted sums (more than 32 lanes, fewer than 64).
    (6, 4, 2) extrapolates first at count 6 = Ndelay, below Norder + 2 = 8: Ng::accelerate then asks storage_index for counts
    -1 and -2, which in the reference (Ng.hpp:47-50, `cnt % (Norder + 2)` of a negative int) and in the oracle's restatement
    index BEFORE the history -- an out-of-bounds read (the oracle answered "singular" from it when this was tried; nothing
    defines that).  The device wraps such a count onto slots that still hold the zeros of configure, so the comparison with
    the recorded bits and with the lone context stands for that set; the oracle is compared wherever it is defined
    (Ndelay >= Norder + 2), and (6, 4, 8) is added so that a 42-sum system meets it too.
    Lone context and batch column run the same ng_kernel: their equality guards the column addressing, the history stride and
    the compacted list, and the arithmetic is held -- both of them -- to tests/golden/ng_step_bits.json, recorded from lone
    contexts when they still had a kernel of their own (one thread forming every sum)."""
    tw = Twins(Nspace)
    try:
        for opts in ng_cases.OPTIONS:
            syn = ng_cases.sequence_inputs(tw.probs, opts)
            xs = tw.seed(syn, opts, gold=ng_cases.golden('HCa', Nspace, opts))
            eff = (opts[0], opts[1], max(opts[2], opts[1] + 2))
            assert tw.batch.ng_state()['options'] == eff
            oracle = None
            if eff[2] >= opts[0] + 2:
                oracle = [[bindings.NgHandle('oracle', *opts, sol=x) for x in syn.x0[i]] for i in range(3)]
            worst, nacc = [0.0, 0.0], 0
            for stepNo in range(1, 13):
                xs = tw.step(syn, xs, oracle=oracle, worst=worst)
                st = tw.batch.ng_state()
                want = stepNo + 1 >= eff[2] and (stepNo + 1 - eff[2]) % eff[1] == 0
                assert st['counts'] == [stepNo + 1] * 3 and st['lastAccelerated'] == [want] * 3
                nacc += want
            assert nacc >= 2
            print('Nspace', Nspace, 'Ng', opts, 'accelerated steps', nacc, 'max rel diff of n against the oracle: batch %.3e lone %.3e'
                  % tuple(worst))
    finally:
        tw.close()


@pytest.mark.gpu
def test_each_column_keeps_its_own_ng_schedule(gpu):
    tw = Twins(32)
    try:
        syn = Synthetic(tw.probs)
        xs = tw.seed(syn, NG)
        for stepNo in range(1, 4):
            xs = tw.step(syn, xs)
        tw.batch.set_active([0, 2])
        n1 = get(tw.batch.contexts[1], tw.probs[1])
        for stepNo in range(4, 7):
            xs = tw.step(syn, xs, cols=(0, 2))
            assert tw.batch.ng_state()['counts'] == [stepNo + 1, 4, stepNo + 1]
            assert all(np.array_equal(a, b) for a, b in zip(get(tw.batch.contexts[1], tw.probs[1]), n1))
        tw.batch.set_active(None)
        seen = []
        for stepNo in range(7, 13):     # column 1 goes on bit-equal to its lone context, which skipped the same calls
            xs = tw.step(syn, xs)
            seen.append(tw.batch.ng_state()['lastAccelerated'])
        st = tw.batch.ng_state()
        assert st['counts'] == [13, 10, 13]
        # counts 8 .. 13 and, for column 1, 5 .. 10: (2, 3, 5) extrapolates at 5, 8, 11, ... -- column 1 from other slots of a
        # history that is three calls shorter (which the bit-equality with its lone context has checked)
        assert [s[0] for s in seen] == [True, False, False, True, False, False] == [s[2] for s in seen]
        assert [s[1] for s in seen] == [True, False, False, True, False, False]
    finally:
        tw.close()


@pytest.mark.gpu
def test_one_solved_atom_matches_the_recorded_bits(gpu):
    """H alone: each column has ONE workgroup, the first to take the column's ticket and the last -- it must still write the
    count back (and only after its own read).  Lone contexts and a fused batch of 3 against the recorded steps."""
    opts = (2, 3, 5)
    tw = Twins(13, problem='H')
    try:
        assert tw.nAtoms == 1
        syn = ng_cases.sequence_inputs(tw.probs, opts)
        xs = tw.seed(syn, opts, gold=ng_cases.golden('H', 13, opts))
        for stepNo in range(1, ng_cases.NSTEPS + 1):
            xs = tw.step(syn, xs)
            assert tw.batch.ng_state()['counts'] == [stepNo + 1] * 3
            assert [c.ng_state()['count'] for c in tw.lones] == [stepNo + 1] * 3
    finally:
        tw.close()


@pytest.mark.gpu
def test_a_repeated_configure_seeds_again(gpu):
    """(2, 3, 5), three steps, then (1, 1, 0) on the SAME context -- a smaller history, allocated anew -- fed the (1, 1, 0)
    sequence from its x0: the recorded (1, 1, 0) steps, one by one.  Nothing of the first configuration's history or count
    may survive."""
    from lightweaver_amd.context import Context
    prob = column(SEEDS[0], 13)
    with Context(prob) as ctx:
        first = ng_cases.sequence_inputs([prob], (2, 3, 5))
        put(ctx, prob, first.x0[0])
        ctx.configure_ng(2, 3, 5)
        xs = first.x0[0]
        for _ in range(3):
            xs = first.advance(0, xs)
            put(ctx, prob, xs)
            assert lone_ng(ctx, 2)[0] == abi.OK
            xs = get(ctx, prob)
        assert ctx.ng_state() == dict(options=(2, 3, 5), count=4, lastAccelerated=False)
        opts = (1, 1, 0)
        syn, gold = ng_cases.sequence_inputs([prob], opts), ng_cases.golden('HCa', 13, opts)
        ng_cases.check_inputs(gold[:1], syn)
        put(ctx, prob, syn.x0[0])
        ctx.configure_ng(*opts)
        assert ctx.ng_state() == dict(options=(1, 1, 3), count=1, lastAccelerated=False)
        xs = syn.x0[0]
        for stepNo in range(1, ng_cases.NSTEPS + 1):
            put(ctx, prob, syn.advance(0, xs))
            st, acc, dP, dI = lone_ng(ctx, 2)
            assert st == abi.OK
            xs = get(ctx, prob)
            ng_cases.check_step(gold, 0, stepNo, 'reconfigured lone', xs, acc, dP, dI)


@pytest.mark.gpu
def test_ng_state_is_the_devices_word_for_lone_contexts_and_unfused_batches(gpu):
    from lightweaver_amd.context import Context
    prob = column(SEEDS[0], 13)
    syn = Synthetic([prob])
    with Context(prob) as ctx:
        assert ctx.ng_state() == dict(options=None, count=0, lastAccelerated=False)
        put(ctx, prob, syn.x0[0])
        ctx.configure_ng(*NG)
        assert ctx.ng_state() == dict(options=NG, count=1, lastAccelerated=False)
        xs = syn.x0[0]
        for k in range(1, 9):
            put(ctx, prob, syn.advance(0, xs))
            st, acc, _, _ = lone_ng(ctx, 2)
            assert st == abi.OK
            xs = get(ctx, prob)
            # (2, 3, 5): counts 5, 8, ... extrapolate
            assert ctx.ng_state() == dict(options=NG, count=k + 1, lastAccelerated=(k + 1) in (5, 8)) and acc == ((k + 1) in (5, 8))
        ctx.configure_ng(0, 0, 0)      # a lone context: order 0, the changes still tracked
        assert ctx.ng_state() == dict(options=(0, 0, 2), count=1, lastAccelerated=False)
    # the scenario of test_each_column_keeps_its_own_ng_schedule on a fused and on an unfused batch: the same state throughout
    probs = [[column(s, 32) for s in SEEDS[:3]] for _ in range(2)]
    syn = Synthetic(probs[0])
    with ColumnBatch(probs[0]) as fused, ColumnBatch(probs[1], fused=False) as unfused:
        assert fused._batch is not None and unfused._batch is None
        assert unfused.ng_state() == fused.ng_state() == dict(options=None, counts=[0] * 3, lastAccelerated=[False] * 3)
        xs = [[x.copy() for x in syn.x0[i]] for i in range(3)]
        for b, pp in zip((fused, unfused), probs):
            for i in range(3):
                put(b.contexts[i], pp[i], xs[i])
            b.configure_ng(*NG)
        assert unfused.ng_state() == fused.ng_state() == dict(options=NG, counts=[1] * 3, lastAccelerated=[False] * 3)
        for stepNo in range(1, 13):
            cols = (0, 2) if 4 <= stepNo <= 6 else (0, 1, 2)
            for b in (fused, unfused):
                b.set_active(list(cols) if len(cols) < 3 else None)
            for i in cols:
                xs[i] = syn.advance(i, xs[i])
            for b, pp in zip((fused, unfused), probs):
                for i in cols:
                    put(b.contexts[i], pp[i], xs[i])
            uf, uu = fused.ng_accelerate(), unfused.ng_accelerate()
            assert uf == uu
            for i in cols:
                xs[i] = get(fused.contexts[i], probs[0][i])
                assert all(np.array_equal(a, b) for a, b in zip(xs[i], get(unfused.contexts[i], probs[1][i])))
            assert unfused.ng_state() == fused.ng_state(), stepNo
        assert unfused.ng_state()['counts'] == [13, 10, 13]


@pytest.mark.gpu
@pytest.mark.parametrize('fused', [True, False])
def test_iterate_to_convergence_with_ng_matches_oracle_per_column(gpu, fused):
    probs = [column(s) for s in SEEDS]
    want = [oracle_trace(s)['stop'] for s in SEEDS]
    acc = [[] for _ in SEEDS]
    retired = {}
    with ColumnBatch(probs, fused=fused) as batch:
        assert (batch._batch is not None) == fused
        before = [list(range(len(SEEDS)))]

        def cb(it, J, P, act):
            for i, u in enumerate(P or []):
                if u is not None and u.ngAccelerated:
                    acc[i].append(it)
            for i in before[0]:
                if i not in act:          # retired in this iteration: its state as of now
                    batch.contexts[i].download(abi.ALL_OUTPUTS | abi.POPS)
                    retired[i] = snapshot(probs[i])
            before[0] = list(act)

        res = batch.iterate_to_convergence(ng=NG, callback=cb, **KW)
        assert batch.active == list(range(len(SEEDS)))
        state = batch.ng_state()
        batch.download()
    print('iterations', res.iterations, 'oracle', want, 'Ng counts', state['counts'])
    assert res.iterations == want and res.converged == [True] * len(SEEDS)
    assert state['options'] == NG and state['counts'] == [w - 1 for w in want]   # frozen at the stop: one call per iteration 3 .. stop
    for i, (s, p, fin) in enumerate(zip(SEEDS, probs, res.final)):
        tr = oracle_trace(s)
        dJ, dP, idx, _ = tr['trace'][tr['stop']]
        print('seed', s, 'dJMax', fin[0].dJMax, dJ, 'dPops', fin[1].dPops, dP, 'J', rel_err(p.J, tr['J']),
              'n', [rel_err(a.n, n) for a, n in zip(p.atoms, tr['n'])])
        assert acc[i] == tr['accelerated'], (s, acc[i])
        assert fin[0].dJMax == pytest.approx(dJ, rel=1e-6)
        assert np.allclose(fin[1].dPops, dP, rtol=1e-5)
        assert list(fin[1].dPopsMaxIdx) == list(idx)
        assert rel_err(p.J, tr['J']) <= TOL_CONVERGED
        for a, n in zip(p.atoms, tr['n']):
            assert rel_err(a.n, n) <= TOL_CONVERGED
        assert not plain_converged_by(s, tr['stop'])          # below the plain-MALI stop
        assert same_bits(retired[i], snapshot(p)), i          # untouched since its retirement


@pytest.mark.gpu
def test_ng_on_changes_nothing_but_ng(gpu):
    seeds = SEEDS[:3]
    probs = [column(s) for s in seeds]

    def put_back(batch, n0):
        for p, c, n in zip(probs, batch.contexts, n0):
            put(c, p, n)

    with ColumnBatch(probs) as batch:
        assert batch._batch is not None
        for it in range(NSCATTER + 1):
            batch.formal_sol_gamma_matrices(sync_host=False)
        n0 = [[a.n.copy() for a in p.atoms] for p in probs]
        assert batch.ng_state() == dict(options=None, counts=[0] * 3, lastAccelerated=[False] * 3)
        off = batch.stat_equil(report=True)
        batch.download(abi.POPS)
        n1 = [[a.n.copy() for a in p.atoms] for p in probs]
        put_back(batch, n0)
        batch.configure_ng(*NG)
        assert batch.ng_state() == dict(options=NG, counts=[1] * 3, lastAccelerated=[False] * 3)
        on = batch.stat_equil(report=True)            # count 2: recorded, not extrapolated
        assert batch.ng_state()['counts'] == [2] * 3
        batch.download(abi.POPS)
        for p, n, old, u, v in zip(probs, n1, n0, on, off):
            assert all(np.array_equal(a.n, x) for a, x in zip(p.atoms, n))
            assert not any(np.array_equal(a.n, x) for a, x in zip(p.atoms, old))
            print('dPops with Ng', u.dPops, 'without', v.dPops)
            assert not u.ngAccelerated and np.allclose(u.dPops, v.dPops, rtol=1e-9, atol=0.0)
            assert list(u.dPopsMaxIdx) == list(v.dPopsMaxIdx)
        batch.configure_ng(0, 0, 0)
        assert batch.ng_state() == dict(options=None, counts=[0] * 3, lastAccelerated=[False] * 3)
        put_back(batch, n0)
        again = batch.stat_equil(report=True)
        batch.download(abi.POPS)
        for p, n, u, v in zip(probs, n1, again, off):
            assert all(np.array_equal(a.n, x) for a, x in zip(p.atoms, n))
            assert u.dPops == v.dPops and list(u.dPopsMaxIdx) == list(v.dPopsMaxIdx) and not u.ngAccelerated


@pytest.mark.gpu
def test_refusals_and_a_singular_column(gpu):
    tw = Twins(13)
    try:
        lib, h = tw.batch.contexts[0].lib, tw.batch._batch
        null = C.c_void_p(None)
        opts = (C.c_int32 * 3)()
        assert lib.lwhip_batch_ng_accelerate(h, None, None, None) == abi.ERR_INVALID     # before configure
        assert lib.lwhip_batch_ng_configure(null, 2, 3, 5) == abi.ERR_INVALID
        assert lib.lwhip_batch_ng_accelerate(null, None, None, None) == abi.ERR_INVALID
        assert lib.lwhip_batch_ng_state(null, opts, None, None) == abi.ERR_INVALID
        syn = Synthetic(tw.probs)
        xs = tw.seed(syn, NG)
        xs = tw.step(syn, xs)
        state = tw.batch.ng_state()
        assert state['options'] == NG and state['counts'] == [2] * 3
        for bad in ((7, 3, 5), (-1, 3, 5), (2, 0, 5)):
            assert lib.lwhip_batch_ng_configure(h, *bad) == abi.ERR_INVALID, bad
            assert tw.batch.ng_state() == state
        xs = tw.step(syn, xs)          # ... and the configuration that was kept still steps
        # column 1 fed the same populations every time with (1, 1, 0): every Delta is 0, the 1 x 1 matrix is 0 -> singular at the
        # first extrapolating call (the second), for the batch and for the lone context alike
        xs = tw.seed(syn, (1, 1, 0))
        xs[1] = [x.copy() for x in syn.x0[1]]
        const = [x.copy() for x in syn.x0[1]]
        for call in (1, 2):
            for i in (0, 2):
                xs[i] = syn.advance(i, xs[i])
            for i in range(3):
                put(tw.batch.contexts[i], tw.probs[i], const if i == 1 else xs[i])
                put(tw.lones[i], tw.lprobs[i], const if i == 1 else xs[i])
            lone = [lone_ng(c, tw.nAtoms) for c in tw.lones]
            if call == 1:
                assert all(u is not None and not u.ngAccelerated for u in tw.batch.ng_accelerate())
                assert [l[0] for l in lone] == [abi.OK] * 3
                continue
            assert [l[0] for l in lone] == [abi.OK, abi.ERR_SINGULAR, abi.OK] and lone[0][1] and lone[2][1]
            with pytest.raises(ExplodingMatrixError):
                tw.batch.ng_accelerate()
            assert tw.batch.ng_state()['counts'] == [3] * 3
            for i in range(3):       # every column's n is what its lone context's is, the singular one's included
                nb, nl = get(tw.batch.contexts[i], tw.probs[i]), get(tw.lones[i], tw.lprobs[i])
                assert all(np.array_equal(a, b) for a, b in zip(nb, nl)), i
    finally:
        tw.close()
