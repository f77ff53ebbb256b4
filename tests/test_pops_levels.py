"""The population solves at every level count, not only six (tests/pops_cases.py builds the problems and holds the
extended-precision reference).

lwhip_pops.hip solves one small dense system per depth point with the reference's Crout LU, in registers for
2 <= N <= 6 (one unrolled instantiation per N) and in LDS otherwise, with a block size that shrinks with N.  The atoms of
every other test have six levels; here statistical equilibrium, the backward-Euler update and the Newton-Raphson step
run at N = 1 .. 7, 11, 13, 32 and at 64 coupled equations, on atoms of different sizes in one launch, as a fused column
batch, over a depth range, and on matrices chosen for the pivoting branches: row exchanges in every row, a column without a
positive candidate (exchange with row 0), a zero pivot replaced by 1e-20, leading zeros of b, pivots decided by the row scaling.

Two conditions per random case, both taken from references and not from the code under test:
  1. the project tolerance: rel_err(hip, oracle) <= 1e-9 (TOL of test_pops.py); the CPU tests here hold the oracle's own
     error against the longdouble solution a decade below that on every case;
  2. the worst component-wise relative error of the HIP result against the longdouble solution is at most four times the
     oracle's plus 64 eps: the kernels claim the oracle's operations one for one, so the expected ratio is 1; the factor
     absorbs a different rounding in one division or one sum, the floor the cases where the oracle happens to be exact.
     A wrong pivot row, a missing swap, a mis-sized LDS stride or an uninitialised workspace element is orders above it.
Each GPU case prints its two errors (pytest -s) before it asserts."""
import functools
import itertools

import numpy as np
import pytest

import pops_cases as pc
from helpers import rel_err
from lightweaver_amd import _abi as abi
from oracle.bindings import OracleContext

TOL = 1e-9              # hip against oracle (test_pops.py)
ORACLE_TOL = 1e-10      # oracle against longdouble: a decade below TOL, so that condition 1 tests the kernel
NS = pc.NSPACE

STAT_EQ_CASES = [(N, NS) for N in pc.STAT_EQ_LEVELS] + [(32, 3)]
TIME_DEP_CASES = list(itertools.product(pc.TIME_DEP_LEVELS, pc.TIME_DEP_DTS))
NR_CASES = [pytest.param(tuple(l), td, fdc, id='-'.join(map(str, l)) + ('-td' if td else '') + ('-dC' if fdc else ''))
            for l in pc.NR_LISTS for td in (False, True) for fdc in (False, True)]
PERM_LEVELS = [1, 2, 3, 4, 5, 6, 7, 13, 32]
DEFICIENT_CASES = ([(N, 'ones') for N in (2, 4, 6, 7)] + [(5, 'proportional')]
                   + [(2, 'zero0'), (2, 'zero1'), (3, 'zero0'), (3, 'zero1'), (4, 'zero2'), (5, 'zero1'), (6, 'zero0'), (6, 'zero2'),
                      (7, 'zero1'), (13, 'zero0'), (13, 'zero2'), (32, 'zero1')])


def frozen(x):
    """x (an array, or a list of arrays: returned as a tuple) made read-only."""
    if isinstance(x, (list, tuple)):
        return tuple(frozen(a) for a in x)
    x.flags.writeable = False
    return x


# ---- one update through a context factory: OracleContext, or the HIP Context behind the same call shapes ----------------
class Hip:
    def __init__(self, p):
        from lightweaver_amd.context import Context
        self.p = p
        self.ctx = Context(p)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ctx.close()

    def set_depth_range(self, s, e):
        self.ctx.set_depth_range(s, e)

    def stat_equil(self, atom=-1):
        self.ctx.stat_equil(atom=atom)
        return 0

    def time_dep_update(self, atom, nOld, dt):
        lst = [nOld if ia == atom else a.n for ia, a in enumerate(self.p.atoms)]
        self.ctx.time_dep_update(dt, lst, atom=atom)
        return 0

    def nr_post_update(self, atoms, stages, bg, ne, dC=None, nPrev=None, dt=0.0, crsw=1.0):
        self.ctx.crsw = crsw
        self.ctx.nr_post_update(stages, bg, ne, dC=dC, nPrev=nPrev, dt=dt, atoms=atoms)
        return 0


Oracle = OracleContext      # (it has no ranged form: a ranged HIP call is compared with its full update)


def run_stat_eq(factory, levels, Ns=NS, seed=1, rng=None):
    p = pc.build(levels, Ns, seed)
    with factory(p) as c:
        if rng:
            c.set_depth_range(*rng)
        assert c.stat_equil() == 0
    return [a.n for a in p.atoms]


def run_time_dep(factory, N, dt, rng=None):
    p = pc.build([N])
    nOld = pc.old_pops(p)[0]
    with factory(p) as c:
        if rng:
            c.set_depth_range(*rng)
        assert c.time_dep_update(0, nOld, dt) == 0
    return p.atoms[0].n


def run_nr(factory, levels, timeDep, fdC, rng=None):
    p = pc.build(levels, span=4.0)
    stages, bg, ne, dC, nPrev = pc.nr_inputs(p)
    with factory(p) as c:
        if rng:
            c.set_depth_range(*rng)
        assert c.nr_post_update(list(range(len(levels))), stages, bg, ne, dC=dC if fdC else None,
                                nPrev=nPrev if timeDep else None, dt=pc.NR_DT, crsw=1.0) == 0
    return [a.n for a in p.atoms], ne


def solve_exact(factory, A, b):
    """x of A x = b at every depth through time_dep_update with dt = 1 and Gamma = I - A."""
    N, Ns = b.shape
    p = pc.build([N], Ns)
    p.atoms[0].Gamma[...] = pc.gamma_for(A)
    with factory(p) as c:
        assert c.time_dep_update(0, b, 1.0) == 0
    return p.atoms[0].n


# ---- references, computed once and shared read-only -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stat_eq_refs(levels, Ns=NS, seed=1):
    """(oracle populations, longdouble populations) per atom."""
    p = pc.build(list(levels), Ns, seed)
    ora = run_stat_eq(Oracle, list(levels), Ns, seed)
    return frozen(ora), frozen([pc.ref_stat_eq(a) for a in p.atoms])


@functools.lru_cache(maxsize=None)
def time_dep_refs(N, dt):
    p = pc.build([N])
    return frozen(run_time_dep(Oracle, N, dt)), frozen(pc.ref_time_dep(p.atoms[0].Gamma, pc.old_pops(p)[0], dt))


@functools.lru_cache(maxsize=None)
def nr_refs(levels, timeDep, fdC):
    p = pc.build(list(levels), span=4.0)
    stages, bg, ne, dC, nPrev = pc.nr_inputs(p)
    n, neNew = pc.ref_nr(p, list(range(len(levels))), stages, bg, ne, dC=dC if fdC else None,
                         nPrev=nPrev if timeDep else None, dt=pc.NR_DT, crsw=1.0)
    ora, neO = run_nr(Oracle, list(levels), timeDep, fdC)
    return (frozen(ora), frozen(neO)), (frozen(n), frozen(neNew))


def as_list(x):
    return list(x) if isinstance(x, (tuple, list)) else [x]


def accept(what, got, ora, ref):
    """The two acceptance conditions of the module docstring for one case (lists of arrays)."""
    got, ora, ref = as_list(got), as_list(ora), as_list(ref)
    eH = max(pc.worst_rel(g, r) for g, r in zip(got, ref))
    eO = max(pc.worst_rel(o, r) for o, r in zip(ora, ref))
    d = max(rel_err(g, o) for g, o in zip(got, ora))
    print(f'\nPOPS_LEVELS {what}: hip-vs-ld {eH:.3e} oracle-vs-ld {eO:.3e} ratio {eH / eO if eO else float(eH != 0):.3f} '
          f'hip-vs-oracle {d:.3e}')
    assert d <= TOL, (what, d)
    assert eH <= 4.0 * eO + 64.0 * pc.EPS, (what, eH, eO)


# ---- CPU: the reference itself, and the oracle against it on every case of the matrix ----------------------------------
def test_longdouble_solver_on_known_systems():
    assert np.finfo(pc.LD).eps < 1e-18, 'longdouble is no wider than double here: the reference would prove nothing'
    rng = np.random.default_rng(0)
    for N in (1, 2, 5, 32, 64):
        A = rng.integers(-9, 10, (N, N)).astype(np.float64) + 20.0 * np.eye(N)
        A[[0, N - 1]] = A[[N - 1, 0]]        # (a pivot search that has to leave the diagonal)
        x = rng.integers(1, 100, N).astype(np.float64)
        assert pc.worst_rel(pc.solve_ld(A, A @ x), x) < 1e-14
    H = 1.0 / (np.arange(6)[:, None] + np.arange(6)[None, :] + 1.0)     # Hilbert, kappa = 1.5e7: double would keep 9 digits
    x = np.arange(1.0, 7.0)
    assert pc.worst_rel(pc.solve_ld(H.astype(pc.LD), H.astype(pc.LD) @ x.astype(pc.LD)), x) < 1e-11


def test_rate_matrices_are_as_specified():
    p = pc.build(pc.MIXED)
    for a in p.atoms:
        N = a.Nlevel
        off = ~np.eye(N, dtype=bool)
        G = a.Gamma
        assert np.all(G[off] >= 0.0) and np.all(G[off][G[off] > 0.0] >= 1e-3) and np.all(G[off] <= 1e3)
        i, j = np.indices((N, N))
        far = np.abs(i - j) > 1
        assert not far.any() or 0.25 < np.mean(G[far] == 0.0) < 0.35
        for l in range(N - 1):
            assert np.all(G[l + 1, l] >= 1e-3) and np.all(G[l, l + 1] >= 1e-3)
        assert np.all(np.abs(G.sum(axis=0)) <= 1e-12 * np.abs(G).sum(axis=0))
        assert np.all(a.n >= 1.0) and np.all(a.n <= 1e8)
        assert [(t.i, t.j) for t in a.trans] == [(i, N - 1) for i in range(0, N - 1, 2)]


@pytest.mark.parametrize('N,Ns', STAT_EQ_CASES)
def test_oracle_stat_eq_matches_longdouble(N, Ns):
    ora, ref = stat_eq_refs((N,), Ns)
    assert pc.worst_rel(ora, ref) <= ORACLE_TOL


@pytest.mark.parametrize('seed', [1, 11, 12, 13])
def test_oracle_stat_eq_mixed_matches_longdouble(seed):
    ora, ref = stat_eq_refs(tuple(pc.MIXED), NS, seed)
    assert max(pc.worst_rel(o, r) for o, r in zip(ora, ref)) <= ORACLE_TOL


@pytest.mark.parametrize('N,dt', TIME_DEP_CASES)
def test_oracle_time_dep_matches_longdouble(N, dt):
    ora, ref = time_dep_refs(N, dt)
    assert pc.worst_rel(ora, ref) <= ORACLE_TOL


@pytest.mark.parametrize('levels,timeDep,fdC', NR_CASES)
def test_oracle_nr_matches_longdouble(levels, timeDep, fdC):
    (ora, neO), (ref, neR) = nr_refs(levels, timeDep, fdC)
    assert max(pc.worst_rel(o, r) for o, r in zip(ora, ref)) <= ORACLE_TOL
    assert pc.worst_rel(neO, neR) <= ORACLE_TOL
    # the step did something
    p = pc.build(list(levels), span=4.0)
    assert max(rel_err(o, a.n) for o, a in zip(ora, p.atoms)) > 1e-6


@pytest.mark.parametrize('N', PERM_LEVELS)
def test_oracle_solves_permutation_matrices_exactly(N):
    A, x, b = pc.permutation_case(N)
    assert np.any(b[0] == 0.0) or N == 1          # leading zeros of b do occur
    np.testing.assert_array_equal(solve_exact(Oracle, A, b), x)


def branch_counts(A, depths=(0, 1, 34, 69)):
    """pops_cases.lu_branches of A at a few depths, summed."""
    tot = {}
    for k in depths:
        for name, v in pc.lu_branches(A[:, :, k]).items():
            tot[name] = tot.get(name, 0) + v
    return tot, len(depths)


def test_oracle_rank_deficient_results_are_the_reference_s():
    """Meaningless but deterministic, derived by hand: all ones at N = 2 with b = [2, 3] has no candidate in column 1,
    exchanges row 1 with row 0 (no zero pivot) and gives [4, -1]; [[0, 1], [0, 2]] x = [2, 3] has no candidate in column
    0, takes the 1e-20 pivot and gives [2 (0.5 / 1e-20), 1.5]."""
    A, b = pc.rank_deficient_case(2, 'ones')
    np.testing.assert_array_equal(solve_exact(Oracle, A, b)[:, 0], [4.0, -1.0])
    A, b = pc.rank_deficient_case(2, 'zero0')
    np.testing.assert_array_equal(solve_exact(Oracle, A, b)[:, 0], [2.0 * (0.5 / 1e-20), 1.5])


@pytest.mark.parametrize('N,kind', DEFICIENT_CASES)
def test_rank_deficient_cases_take_the_branches_they_are_for(N, kind):
    """Counted on a plain restatement of the decomposition: 'ones' and 'proportional' exchange with a row above the
    diagonal and never replace a pivot; the zero-column cases replace exactly one pivot per matrix by 1e-20, and the
    oracle's results show it in their magnitude."""
    A, b = pc.rank_deficient_case(N, kind)
    got, nd = branch_counts(A)
    x = solve_exact(Oracle, A, b)
    if kind.startswith('zero'):
        assert got['replaced'] == nd and got['no_candidate'] >= nd
        assert got['swaps_up'] == (nd if kind != 'zero0' else 0)
        # (a right-hand side whose numerator over that pivot cancels exactly stays small: [[1, 0], [2, 0]] x = [3, 4])
        assert np.mean(np.max(np.abs(np.where(np.isfinite(x), x, np.inf)), axis=0) >= 1e19) > 0.9
    else:
        assert got['replaced'] == 0 and got['swaps_up'] >= nd and got['no_candidate'] >= nd
        assert np.all(np.isfinite(x)) and np.max(np.abs(x)) < 1e3


@pytest.mark.parametrize('N', [3, 6, 7, 13])
def test_scaled_rows_cases_are_decided_by_the_scaling(N):
    """In most columns the scaled candidate picks another row than the largest element, and most exchanges move a scaling
    value that differs from the one it replaces: a vv that stayed in place would decide later pivots differently.  The
    permutation cases, for comparison, are never decided by the scaling."""
    got, nd = branch_counts(pc.scaled_rows_case(N)[0])
    assert got['scaling_decides'] >= nd * (N - 1) // 2 and got['vv_moves'] >= nd * (N - 1) // 2
    assert got['replaced'] == 0
    got, nd = branch_counts(pc.permutation_case(N)[0])
    assert got['scaling_decides'] == 0 and got['swaps'] >= nd * (N - 1) // 2 and got['replaced'] == got['no_candidate'] == 0


def singular_problem(N):
    p = pc.build([N])
    k = 7
    row = (int(np.argmax(p.atoms[0].n[:, k])) + 1) % N      # not the eliminated row, which is overwritten with ones
    p.atoms[0].Gamma[row, :, k] = 0.0
    return p


@pytest.mark.parametrize('N', [3, 9])
def test_oracle_reports_a_zero_row_as_singular(N):
    with Oracle(singular_problem(N)) as oc:
        assert oc.stat_equil() == abi.ERR_SINGULAR


# ---- GPU parity matrix -----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('N,Ns', STAT_EQ_CASES)
def test_hip_stat_eq_levels(gpu, N, Ns):
    ora, ref = stat_eq_refs((N,), Ns)
    accept(f'stat_eq N={N} Ns={Ns}', run_stat_eq(Hip, [N], Ns), ora, ref)


def expected_change(new, old):
    ch = np.abs((new - old) / new).ravel()
    return float(ch.max()), int(np.argmax(ch))


@pytest.mark.gpu
def test_hip_stat_eq_mixed_atoms_all_and_one_by_one(gpu):
    """Atoms of 2, 9, 6 and 32 levels in one launch (the block size and LDS of the largest, the small ones on the register
    path inside those blocks), then each atom on its own through the SAME context: the atom's populations and change
    record are those of the all-atoms call, the other atoms keep their input bit for bit."""
    from lightweaver_amd.context import Context
    ora, ref = stat_eq_refs(tuple(pc.MIXED))
    p = pc.build(pc.MIXED)
    n0 = [a.n.copy() for a in p.atoms]
    with Context(p) as ctx:
        upAll = ctx.stat_equil()
        nAll = [a.n.copy() for a in p.atoms]
        accept('stat_eq mixed', nAll, ora, ref)
        for ia, (o, old) in enumerate(zip(ora, n0)):
            v, idx = expected_change(o, old)
            assert upAll.dPops[ia] == pytest.approx(v, rel=1e-9)
            assert upAll.dPopsMaxIdx[ia] == idx
        for ia in list(range(len(p.atoms))) + [-1]:
            for a, old in zip(p.atoms, n0):
                a.n[...] = old
            up = ctx.stat_equil(atom=ia)
            for ib, a in enumerate(p.atoms):
                solved = ia < 0 or ib == ia
                np.testing.assert_array_equal(a.n, nAll[ib] if solved else n0[ib])
                assert up.dPops[ib] == (upAll.dPops[ib] if solved else 0.0)
                assert up.dPopsMaxIdx[ib] == (upAll.dPopsMaxIdx[ib] if solved else 0)


@pytest.mark.gpu
def test_hip_stat_eq_change_record_tie_across_blocks(gpu):
    """Per atom, the depth with the largest change is moved to depth 5 and copied to depth 61: two blocks, at every block
    size, report the same value, and the index must be the first one."""
    from lightweaver_amd.context import Context
    ora, _ = stat_eq_refs(tuple(pc.MIXED))
    p = pc.build(pc.MIXED)
    Ns = p.Nspace
    want = []
    for a, o in zip(p.atoms, ora):
        v, idx = expected_change(o, a.n)
        lvl, k = divmod(idx, Ns)
        for arr in (a.Gamma, a.n, a.nTotal):
            arr[..., [5, k]] = arr[..., [k, 5]]
            arr[..., 61] = arr[..., 5]
        want.append((v, lvl * Ns + 5))
    q = p.copy()
    with Oracle(q) as oc:
        assert oc.stat_equil() == 0
    for a, b, (v, idx) in zip(q.atoms, p.atoms, want):      # the construction did what it says, on the oracle
        assert expected_change(a.n, b.n) == (pytest.approx(v, rel=1e-12), idx)
        np.testing.assert_array_equal(a.n[:, 5], a.n[:, 61])
    with Context(p) as ctx:
        up = ctx.stat_equil()
    for ia, (v, idx) in enumerate(want):
        assert up.dPops[ia] == pytest.approx(v, rel=1e-9)
        assert up.dPopsMaxIdx[ia] == idx
        np.testing.assert_array_equal(p.atoms[ia].n[:, 5], p.atoms[ia].n[:, 61])
        assert rel_err(p.atoms[ia].n, q.atoms[ia].n) <= TOL


@pytest.mark.gpu
def test_hip_stat_eq_batched_mixed_atoms(gpu):
    """The fused batch launch (stat_eq_kernel<true>, blockIdx.z = column) on three columns of the mixed atoms, each with
    populations and rates of its own, against each column's own oracle run."""
    from lightweaver_amd.batch import ColumnBatch
    seeds = (11, 12, 13)
    probs = [pc.build(pc.MIXED, seed=s) for s in seeds]
    with ColumnBatch(probs, device_profiles=False) as batch:
        assert batch._batch is not None, 'the columns did not fuse: stat_eq_kernel<true> would not run'
        for c in batch.contexts:
            c.upload(abi.GAMMA | abi.POPS)
        batch.stat_equil()
        batch.download(abi.POPS)
    for s, p in zip(seeds, probs):
        ora, ref = stat_eq_refs(tuple(pc.MIXED), NS, s)
        accept(f'stat_eq batched column seed={s}', [a.n for a in p.atoms], ora, ref)


@pytest.mark.gpu
@pytest.mark.parametrize('N,dt', TIME_DEP_CASES)
def test_hip_time_dep_levels(gpu, N, dt):
    ora, ref = time_dep_refs(N, dt)
    accept(f'time_dep N={N} dt={dt}', run_time_dep(Hip, N, dt), ora, ref)


@pytest.mark.gpu
@pytest.mark.parametrize('levels,timeDep,fdC', NR_CASES)
def test_hip_nr_levels(gpu, levels, timeDep, fdC):
    (ora, neO), (ref, neR) = nr_refs(levels, timeDep, fdC)
    n, ne = run_nr(Hip, list(levels), timeDep, fdC)
    accept(f'nr {list(levels)} timeDep={timeDep} fdC={fdC}', n + [ne], list(ora) + [neO], list(ref) + [neR])


@pytest.mark.gpu
@pytest.mark.parametrize('what', ['stat_eq', 'time_dep', 'nr_post'])
def test_hip_depth_range_at_32_levels(gpu, what):
    """The three updates on [17, 49) at 32 levels (NR: 32 + 31 levels, 64 equations, 2 threads per block): the full
    update inside the range, the input bit for bit outside it."""
    if what == 'stat_eq':
        before = [a.n for a in pc.build([32]).atoms]
        got, (ora, ref) = run_stat_eq(Hip, [32], rng=pc.RANGE), stat_eq_refs((32,))
    elif what == 'time_dep':
        before = [a.n for a in pc.build([32]).atoms]
        got, (ora, ref) = [run_time_dep(Hip, 32, 0.1, rng=pc.RANGE)], [[r] for r in time_dep_refs(32, 0.1)]
    else:
        p = pc.build([32, 31], span=4.0)
        before = [a.n for a in p.atoms] + [pc.nr_inputs(p)[2]]
        n, ne = run_nr(Hip, [32, 31], True, True, rng=pc.RANGE)
        (o, neO), (r, neR) = nr_refs((32, 31), True, True)
        got, ora, ref = n + [ne], list(o) + [neO], list(r) + [neR]
    sl = slice(*pc.RANGE)
    outside = np.ones(NS, bool)
    outside[sl] = False
    for g, b in zip(got, before):
        np.testing.assert_array_equal(g[..., outside], b[..., outside])
    accept(f'{what} range {pc.RANGE}', [g[..., sl] for g in got], [o[..., sl] for o in as_list(ora)],
           [r[..., sl] for r in as_list(ref)])


# ---- limits: argument checks, nothing is launched ---------------------------------------------------------------------
@pytest.mark.gpu
def test_hip_rejects_33_levels(gpu):
    from lightweaver_amd.context import Context, LwHipError
    with pytest.raises(LwHipError):
        Context(pc.build([33], 3))


@pytest.mark.gpu
def test_hip_nr_rejects_65_equations(gpu):
    from lightweaver_amd.context import Context, LwHipError
    p = pc.build([32, 32], 3, span=4.0)
    stages, bg, ne, dC, nPrev = pc.nr_inputs(p)
    with Context(p) as ctx:
        with pytest.raises(LwHipError):
            ctx.nr_post_update(stages, bg, ne)


@pytest.mark.gpu
@pytest.mark.parametrize('N', [3, 9])
def test_hip_stat_eq_zero_row_is_singular(gpu, N):
    """One all-zero row of Gamma at one depth, on the register path (3) and the LDS path (9)."""
    from lightweaver_amd.context import Context, ExplodingMatrixError
    with Context(singular_problem(N)) as ctx:
        with pytest.raises(ExplodingMatrixError):
            ctx.stat_equil()


# ---- exact pivoting cases through time_dep_update -----------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('N', PERM_LEVELS)
def test_hip_solves_permutation_matrices_exactly(gpu, N):
    """Every row of every instantiation goes through the swap selects, with another permutation at each depth; all
    operations are exact in fp64, so the result is x itself."""
    A, x, b = pc.permutation_case(N)
    np.testing.assert_array_equal(solve_exact(Hip, A, b), x)


@pytest.mark.gpu
@pytest.mark.parametrize('N,kind', DEFICIENT_CASES)
def test_hip_rank_deficient_matches_oracle_bit_for_bit(gpu, N, kind):
    """'ones', 'proportional': no positive candidate, exchange with row 0.  'zero<c>': the same with a zero in row 0 too,
    so the pivot is replaced by 1e-20 (results of order 1e20), on the register path (N = 2 .. 6) and in LDS (7, 13, 32).
    test_rank_deficient_cases_take_the_branches_they_are_for counts the branches.  The results mean nothing, but the
    kernels state the reference's operations one for one (lwhip_lu.h), so they are the oracle's bits."""
    A, b = pc.rank_deficient_case(N, kind)
    np.testing.assert_array_equal(solve_exact(Hip, A, b), solve_exact(Oracle, A, b))


@pytest.mark.gpu
@pytest.mark.parametrize('N', PERM_LEVELS)
def test_hip_pivot_order_matches_oracle_bit_for_bit(gpu, N):
    """Rows of very different scales and inexact arithmetic: the same pivots in the same order, or the last bits differ
    (pops_cases.scaled_rows_case).  The kernels use IEEE fp64 operations with contraction off, as the oracle does."""
    A, b = pc.scaled_rows_case(N)
    np.testing.assert_array_equal(solve_exact(Hip, A, b), solve_exact(Oracle, A, b))
