"""Columns deeper than 256 points: the ray-column march with a direction's depth points split over S = 4 wavefronts
(raymarch_split_kernel), in the DEFAULT environment -- no LWHIP_SWEEP, no LWHIP_DEPTH_SPLIT -- and what a
context whose sweep is split does elsewhere: formal_sol, the PRD rates pass, shards; and what turns the split off.

Every case asserts which kernel ran (Context.sweep_kind(), Context.depth_split()) and compares with the C oracle at the
project's bounds: 1e-9 element-wise after one call (TOL_ONE_CALL), 1e-12 on J and I between the split and the unsplit march,
1e-6 on iterated J and populations (TOL_CONVERGED).  Depth counts: 257 (the smallest the size rule sends to the march;
segments of 72, 72, 72, 41 points), 333 (88, 88, 88, 69) and the reference benchmark's 500.

The base problem is the one test_march_with_the_depth_points_split_over_wavefronts_vs_oracle uses: a perturbed (moving)
FAL-C resampled to Ns points, H_6(0.3) + CaII_6(0.3), 5 mu.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from helpers import TOL_CONVERGED, TOL_ONE_CALL, rel_err
from lightweaver_amd import _abi as abi
from lightweaver_amd.context import Context, LwHipError
from lightweaver_amd.harness import models
from lightweaver_amd.model import Boundary
from oracle.bindings import OracleContext
from test_hip_parity import compare_problems

pytestmark = pytest.mark.gpu

SOLVERS = [abi.FS_BEZIER3_1D, abi.FS_LINEAR_1D, abi.FS_BESSER_1D]


@pytest.fixture(autouse=True)
def default_environment(monkeypatch):
    """The library chooses the sweep and the split by itself."""
    monkeypatch.delenv('LWHIP_SWEEP', raising=False)
    monkeypatch.delenv('LWHIP_DEPTH_SPLIT', raising=False)


def deep_atmos(Ns, seed=3):
    return models.perturbed(models.resample(models.falc82(), Ns), seed=seed)


def base_problem(Ns, seed=3, **kw):
    return models.build_problem(deep_atmos(Ns, seed), [models.H_6(0.3), models.CaII_6(0.3)], Nrays=5, **kw)


@functools.lru_cache(maxsize=None)
def _base_and_oracle(Ns, solver=abi.FS_BEZIER3_1D):
    """The base problem at Ns points and the oracle's result of one iteration from it: computed once, never written to."""
    prob = base_problem(Ns, formalSolver=solver)
    q = prob.copy()
    q.gamma_prefill()
    dJ, _ = OracleContext(q).formal_sol_gamma_matrices()
    return prob, q, dJ


def march(p, split, **kw):
    """A context of `p` that must run the march with its depth points split over `split` wavefronts."""
    ctx = Context(p, **kw)
    try:
        assert ctx.sweep_kind() == 'march'
        assert ctx.depth_split() == split, (ctx.depth_split(), split)
    except BaseException:
        ctx.close()
        raise
    return ctx


def iterate_once(prob, split, monkeypatch, forced=None, **kw):
    """One formal_sol_gamma_matrices of a copy of `prob` on a context with the expected split (forced: LWHIP_DEPTH_SPLIT)."""
    if forced is not None:
        monkeypatch.setenv('LWHIP_DEPTH_SPLIT', str(forced))
    else:
        monkeypatch.delenv('LWHIP_DEPTH_SPLIT', raising=False)
    p = prob.copy()
    with march(p, split) as ctx:
        p.gamma_prefill()
        up = ctx.formal_sol_gamma_matrices(**kw)
    monkeypatch.delenv('LWHIP_DEPTH_SPLIT', raising=False)
    return p, up


def lines_of_two_atoms(prob):
    """The line-count loop of test_more_than_two_overlapping_lines, per atom: the largest number of lines at one wavelength,
    and the largest number of ATOMS with a line there."""
    lines = np.zeros((len(prob.atoms), prob.Nlambda), dtype=int)
    for ia, a in enumerate(prob.atoms):
        for t in a.trans:
            if t.type == abi.LINE:
                lines[ia, t.Nblue:t.Nred] += 1
    return int(lines.sum(axis=0).max()), int((lines > 0).sum(axis=0).max())


# ---- a. the split never asks for more LDS than a workgroup has ------------------------------------------------------------
def third_atom(Nlevel, lineScale=0.3):
    """A Mg II-like third active atom: 3s, 3p 3/2 + Mg III (3 levels), or 3s, 3p 1/2, 3p 3/2, 4s + Mg III (5 levels).  Its
    lines (279.6, 280.3, 293.7 nm) lie clear of every H and Ca II line; one bound-free continuum from the ground level (edge
    82.5 nm, blueward of the Lyman lines)."""
    n = lambda base: max(int(round(base * lineScale)) | 1, 5)
    line = lambda i, j, f: models.LineModel(i, j, f, 3.0, 30.0, n(41), vdw=2.0e-14)
    if Nlevel == 3:
        E, g, stage = [0.0, 35760.88, 121267.61], [2, 4, 1], [1, 1, 2]
        lines, extra = [line(0, 1, 0.608)], []
    else:
        assert Nlevel == 5
        E, g, stage = [0.0, 35669.31, 35760.88, 69804.95, 121267.61], [2, 2, 4, 2, 1], [1, 1, 1, 1, 2]
        lines, extra = [line(0, 1, 0.303), line(0, 2, 0.608), line(2, 3, 0.14)], [(1, 2, 5.0), (1, 3, 1.0)]
    continua = [models.ContinuumModel(0, Nlevel - 1, 2.4e-23, 50.0, n(20))]
    return models.AtomModel('Mg', 24.305, 10.0 ** (7.58 - 12.0), E, g, stage, lines, continua, extraCE=extra)


def three_atom_problem(Ns, Nlevel):
    prob = models.build_problem(deep_atmos(Ns), [models.H_6(0.3), models.CaII_6(0.3), third_atom(Nlevel)], Nrays=5)
    maxLines, maxAtoms = lines_of_two_atoms(prob)
    assert maxAtoms == 1 and maxLines <= 2   # every tile keeps a compiled kind: the split stays eligible
    return prob


@pytest.mark.parametrize('Ns,Nlevel,forcedTo', [(500, 3, 2), (257, 5, 2)])
def test_split_that_does_not_fit_the_lds_runs_unsplit(monkeypatch, Ns, Nlevel, forcedTo):
    """ADVICE.md's medium finding: the split launch runs its post-pass on 128 S threads, each with its level columns in LDS,
    raymarch_lds_bytes = 8 (maxCT 4 Ns + max(windows + exchange, 16 + (Natom + 2 NlevTot) 128 S)) bytes, and build_tables
    chose S = 4 without asking whether that fits the 163 840 bytes of a workgroup; every iteration of such a context then
    failed at hipFuncSetAttribute.  The contexts here report maxCT = 2 (LWHIP_VERBOSE at create), as H + Ca II alone do at
    this line scale:
      H(6) + Ca II(6) at 500 points:           8 (4 000 + 16 + 26 x 512) = 138 624  fits, S = 4
      + the 3-level atom at 500 (33 columns):  8 (4 000 + 16 + 33 x 512) = 167 296  over;  S = 2: 8 (4 000 + 16 + 33 x 256) = 99 712
      + the 3-level atom at 257:               8 (2 056 + 16 + 33 x 512) = 151 744  fits, S = 4 (three atoms do not end the split)
      + the 5-level atom at 257 (37 columns):  8 (2 056 + 16 + 37 x 512) = 168 128  over;  S = 2: 8 (2 056 + 16 + 37 x 256) = 92 352
    (at 257 points and two slots the split is over from Natom + 2 NlevTot = 36 on; a 4-level third atom, 35, still fits.)
    By default a split that does not fit is dropped (S = 1: two-way is a measured loss); a forced LWHIP_DEPTH_SPLIT=4 is reduced
    to the largest value that fits.  Either way lwhip_create succeeds and one iteration + stat_equil match the oracle."""
    prob = three_atom_problem(Ns, Nlevel)
    q = prob.copy()
    with OracleContext(q) as oc:
        q.gamma_prefill()
        dJ, _ = oc.formal_sol_gamma_matrices()
        assert oc.stat_equil() == 0
    for forced, want in ((None, 1), (4, forcedTo)):
        if forced is not None:
            monkeypatch.setenv('LWHIP_DEPTH_SPLIT', str(forced))
        p = prob.copy()
        with march(p, want) as ctx:
            assert ctx.depth_split() < 4
            up = ctx.formal_sol_gamma_matrices()
            ctx.stat_equil()
        assert up.dJMax == pytest.approx(dJ, rel=TOL_ONE_CALL)
        compare_problems(p, q, tol=TOL_ONE_CALL, what=('J', 'I', 'Gamma', 'R'))
        compare_problems(p, q, tol=1e-7, what=('n',))


def test_split_that_fits_is_kept(monkeypatch):
    """H + Ca II at 500 points (the reference benchmark's shape) keeps S = 4 -- 138 624 bytes here, 154 624 with three slots --,
    a forced S = 2 is honoured there, and a third active atom does not end the split where it fits (257 points: 151 744
    bytes)."""
    prob = base_problem(500)
    with march(prob.copy(), 4):
        pass
    monkeypatch.setenv('LWHIP_DEPTH_SPLIT', '2')
    with march(prob.copy(), 2):
        pass
    monkeypatch.delenv('LWHIP_DEPTH_SPLIT')
    with march(three_atom_problem(257, 3), 4):
        pass


# ---- b. creation and launch agree -----------------------------------------------------------------------------------------
SMALLEST_SCALE = 0.04   # every line and continuum quadrature at its floor of 5 points: a small grid, a fast oracle


def run_and_compare(prob, split):
    q = prob.copy()
    q.gamma_prefill()
    dJ, _ = OracleContext(q).formal_sol_gamma_matrices()
    p = prob.copy()
    with march(p, split) as ctx:
        up = ctx.formal_sol_gamma_matrices()
    assert up.dJMax == pytest.approx(dJ, rel=TOL_ONE_CALL)
    compare_problems(p, q)


def test_h_ca_at_the_deepest_column_the_sweep_admits():
    """H + Ca II never reaches the create-time LDS budget in depth: its tiles need two accumulator slots (maxCT = 2), so the
    unsplit launch is 8 (8 Ns + 16 + 26 x 128) bytes -- 92 288 at the 1 024 points the 1D sweep admits, of 153 600 (the
    edge would lie at 1 982 points; at three slots, 1 321).  What does end there is the split: 8 (8 192 + 16 + 26 x 512) =
    172 160 bytes is more than a workgroup has, and a context that asked for it failed at every launch.  Inside: accepted,
    unsplit, one iteration matches the oracle.  Outside (1 025 points): refused at create, for the depth limit."""
    atoms = [models.H_6(SMALLEST_SCALE), models.CaII_6(SMALLEST_SCALE)]
    run_and_compare(models.build_problem(deep_atmos(1024), atoms, Nrays=5), 1)
    with pytest.raises(LwHipError, match=rf'\({abi.ERR_UNSUPPORTED}\).*Nspace > 1024'):
        Context(models.build_problem(deep_atmos(1025), atoms, Nrays=5))


def test_creation_and_launch_agree_at_the_lds_budget():
    """The depth counts just inside and just outside the create-time LDS budget (150 KB for the unsplit launches, sized by
    raymarch_lds_bytes as the launches size themselves), found by creating contexts: the refusal precedes any launch.  H + Ca II
    has no such edge below 1 024 points (the test above), so the problem is H + three blended Ca II copies (test_fs2d.
    blended_atoms: up to six lines at one wavelength, the generic march, unsplit; Natom + 2 NlevTot = 52), whose workgroups
    need more accumulator slots.  Inside: one iteration succeeds and matches the oracle.  Outside: ERR_UNSUPPORTED with the
    LDS message.  What the check gives: six slots, 8 (24 Ns + 16 + 52 x 128) bytes -- 522 points inside (153 600), 523 outside
    (153 792)."""
    from test_fs2d import blended_atoms
    problem = lambda Ns: models.build_problem(deep_atmos(Ns), blended_atoms(3, SMALLEST_SCALE), Nrays=5)
    refusal = rf'\({abi.ERR_UNSUPPORTED}\).*does not fit the 160 KB LDS budget'

    def accepted(Ns):
        try:
            with march(problem(Ns), 1):
                return True
        except LwHipError as e:
            assert str(e).startswith('lwhip_create failed') and 'does not fit the 160 KB LDS budget' in str(e), str(e)
            return False
    # the check is the launches' own formula, 8 (maxCT 4 Ns + 16 + 52 x 128) <= 153 600: the edge is one of these counts,
    # whichever number of slots the context has -- the largest of them that is accepted, and one point more is refused
    cands = sorted({(19200 - 16 - 52 * 128) // (4 * maxCT) for maxCT in range(2, 17)} & set(range(257, 1025)))
    assert accepted(cands[0]) and not accepted(1024)
    i, j = 0, len(cands)          # cands[i] accepted, cands[j] (or 1 024) refused
    while j - i > 1:
        mid = (i + j) // 2
        i, j = (mid, j) if accepted(cands[mid]) else (i, mid)
    lo, hi = cands[i], cands[i] + 1
    print(f'LDS budget edge: {lo} points inside, {hi} outside')
    run_and_compare(problem(lo), 1)
    with pytest.raises(LwHipError, match=refusal):
        Context(problem(hi))


# ---- c. boundary conditions on a split column -----------------------------------------------------------------------------
def with_boundaries(prob, which):
    p = prob.copy()
    rng = np.random.default_rng(11)
    Nrays = p.Nrays
    idxs = np.full((Nrays, 2), -1, dtype=np.int32)
    if which == 'callable-thermalised':    # (what the golden `bc` variant does at 82 points)
        idxs[:, 1] = np.arange(Nrays)[::-1]
        p.zLowerBc = Boundary(abi.BC_CALLABLE, idxs=idxs, bcData=(1.0 + 0.3 * rng.random((p.Nlambda, Nrays))) * p.J[:, -1, None])
        p.zUpperBc = Boundary(abi.BC_THERMALISED)
    else:
        idxs[:, 0] = np.arange(Nrays)
        p.zLowerBc = Boundary(abi.BC_ZERO)
        p.zUpperBc = Boundary(abi.BC_CALLABLE, idxs=idxs, bcData=0.2 * rng.random((p.Nlambda, Nrays)) * p.J[:, 0, None])
    p.gamma_prefill()
    return p


@pytest.mark.parametrize('which', ['callable-thermalised', 'zero-callable'])
def test_boundary_conditions_on_a_split_column(monkeypatch, which):
    """The intensity entering segment 0 of either direction is the boundary's: a CALLABLE lower boundary under a THERMALISED
    upper one, and a ZERO lower boundary under a CALLABLE upper one, at 333 points; J, I, Gamma and the rates against the
    oracle, and J, I of the split against the unsplit march."""
    prob = with_boundaries(_base_and_oracle(333)[0], which)
    q = prob.copy()
    OracleContext(q).formal_sol_gamma_matrices()
    p4, _ = iterate_once(prob, 4, monkeypatch)
    p1, _ = iterate_once(prob, 1, monkeypatch, forced=1)
    assert not np.array_equal(q.I, _base_and_oracle(333)[1].I)   # the boundaries matter
    compare_problems(p4, q)
    compare_problems(p1, q)
    compare_problems(p4, p1, tol=1e-12, what=('J', 'I'))


# ---- d. per-depth outputs -------------------------------------------------------------------------------------------------
def test_depth_data_of_a_split_column(monkeypatch):
    """storeDepthData: chi, eta and I of both directions at every depth -- each segment stores only the points it owns."""
    prob = base_problem(333, storeDepthData=True)
    q = prob.copy()
    OracleContext(q).formal_sol_gamma_matrices()
    assert q.depthI.shape == (prob.Nlambda, 5, 2, 333) and q.depthI.min() >= 0.0 and q.depthChi.min() > 0.0
    p4, _ = iterate_once(prob, 4, monkeypatch)
    p1, _ = iterate_once(prob, 1, monkeypatch, forced=1)
    for p in (p4, p1):
        for name in ('depthChi', 'depthEta', 'depthI'):
            e = rel_err(getattr(p, name), getattr(q, name))
            assert e <= TOL_ONE_CALL, (name, e)
        compare_problems(p, q)
    compare_problems(p4, p1, tol=1e-12, what=('J', 'I'))
    assert rel_err(p4.depthI, p1.depthI) <= 1e-12


def test_zplane_outputs_of_a_split_column(monkeypatch):
    """ZPlaneDecomposition as test_zplane_decomposition_outputs checks it at 82 points: I of the down rays in plane Nz - 2
    (owned by the last segment of the down direction) and of the up rays in plane 1 (the last segment of the up direction),
    for the iteration and for formal_sol(upOnly=True), which leaves the down plane untouched."""
    prob, qref, _ = _base_and_oracle(333)
    q = prob.copy()
    zr = [np.full((prob.Nlambda, prob.Nrays), -1.0) for _ in range(2)]
    zrUp = [np.full((prob.Nlambda, prob.Nrays), -1.0) for _ in range(2)]
    with OracleContext(q) as oc:
        oc.set_zplane(zr[0], zr[1])
        q.gamma_prefill()
        oc.formal_sol_gamma_matrices()
        oc.set_zplane(zrUp[0], zrUp[1])
        oc.formal_sol(upOnly=True)
    assert zr[0].min() > 0.0 and zr[1].min() > 0.0 and np.all(zrUp[0] == -1.0) and zrUp[1].min() > 0.0
    runs = {}
    for forced, want in ((None, 4), (1, 1)):
        if forced is not None:
            monkeypatch.setenv('LWHIP_DEPTH_SPLIT', str(forced))
        p = prob.copy()
        zh = [np.full((p.Nlambda, p.Nrays), -1.0) for _ in range(2)]
        with march(p, want) as ctx:
            ctx.set_zplane(zh[0], zh[1])
            p.gamma_prefill()
            ctx.formal_sol_gamma_matrices()
            assert rel_err(zh[0], zr[0]) <= TOL_ONE_CALL and rel_err(zh[1], zr[1]) <= TOL_ONE_CALL
            assert rel_err(p.J, qref.J) <= TOL_ONE_CALL
            runs[want] = [z.copy() for z in zh]
            for z in zh:
                z[...] = -1.0
            ctx.formal_sol(upOnly=True)
            assert np.all(zh[0] == -1.0) and rel_err(zh[1], zrUp[1]) <= TOL_ONE_CALL
    for a, b in zip(runs[4], runs[1]):
        assert rel_err(a, b) <= 1e-12


# ---- e. the other entry points on a context whose sweep is split ----------------------------------------------------------
def test_lambda_iterate_on_a_split_column(monkeypatch):
    prob = _base_and_oracle(257)[0]
    q = prob.copy()
    q.gamma_prefill()
    OracleContext(q).formal_sol_gamma_matrices(lambdaIterate=True)
    p, _ = iterate_once(prob, 4, monkeypatch, lambdaIterate=True)
    compare_problems(p, q)
    assert not np.array_equal(q.atoms[0].Gamma, _base_and_oracle(257)[1].atoms[0].Gamma)


@pytest.mark.parametrize('upOnly', [True, False])
def test_formal_sol_on_a_context_whose_sweep_is_split(upOnly):
    """formal_sol of such a context is the unsplit, non-fused march with depthSplit = 4 still in its argument block; J is
    not touched."""
    prob = _base_and_oracle(257)[0]
    q = prob.copy()
    OracleContext(q).formal_sol(upOnly=upOnly)
    p = prob.copy()
    J0 = p.J.copy()
    with march(p, 4) as ctx:
        ctx.formal_sol(upOnly=upOnly)
        ctx.download(abi.J)
    assert q.I.max() > 0.0 and rel_err(p.I, q.I) <= TOL_ONE_CALL
    assert np.array_equal(p.J, J0)


@pytest.mark.parametrize('solver', SOLVERS)
def test_solvers_on_a_split_column(monkeypatch, solver):
    prob, q, dJ = _base_and_oracle(257, solver)
    p, up = iterate_once(prob, 4, monkeypatch)
    assert up.dJMax == pytest.approx(dJ, rel=TOL_ONE_CALL)
    compare_problems(p, q)


# ---- f. PRD on a deep column ----------------------------------------------------------------------------------------------
def prd_problem(Ns):
    return models.falc_h_ca(Nrays=5, lineScale=0.2, prd=True, atmos=deep_atmos(Ns))


def test_prd_on_a_deep_column():
    """One iteration (main sweep split four ways) and two PRD sub-iterations, whose rates pass runs the same context's PRD
    tiles unsplit from a second argument block; against the oracle's redistribute_prd at the bound
    test_lane_sweep_ray_split_vs_oracle holds its PRD runs to."""
    prob = prd_problem(257)
    q = prob.copy()
    q.gamma_prefill()
    with OracleContext(q) as oc:
        oc.formal_sol_gamma_matrices()
        oc.redistribute_prd(2, 0.0)
    p = prob.copy()
    with march(p, 4) as ctx:
        p.gamma_prefill()
        ctx.formal_sol_gamma_matrices()
        up = ctx.redistribute_prd(2, 0.0)
    assert up.NprdSubIter == 2
    compare_problems(p, q)
    for ta, tb in zip(p.atoms[1].trans, q.atoms[1].trans):
        assert (ta.rhoPrd is None) == (tb.rhoPrd is None)
    assert any(t.rhoPrd is not None and not np.all(t.rhoPrd == 1.0) for t in q.atoms[1].trans)


def test_hybrid_prd_on_a_deep_column_is_refused():
    """Hybrid PRD forms its rates ray by ray in the lane sweep, which ends at 256 points: refused at create."""
    prob = prd_problem(257)
    with OracleContext(prob.copy()) as oc:
        tables = oc.build_hprd()
        try:
            with pytest.raises(LwHipError, match='hybrid PRD needs the depth-across-lanes sweep'):
                Context(prob.copy(), hprd=tables)
        finally:
            tables.close()


# ---- g. what turns the split off ------------------------------------------------------------------------------------------
def test_overlapping_lines_take_the_generic_march_unsplit():
    from test_fs2d import blended_atoms
    prob = models.build_problem(deep_atmos(333), blended_atoms(2, 0.3), Nrays=5)
    assert lines_of_two_atoms(prob)[0] == 4
    q = prob.copy()
    q.gamma_prefill()
    dJ, _ = OracleContext(q).formal_sol_gamma_matrices()
    p = prob.copy()
    with march(p, 1) as ctx:
        up = ctx.formal_sol_gamma_matrices()
    assert up.dJMax == pytest.approx(dJ, rel=TOL_ONE_CALL)
    compare_problems(p, q)


def test_fused_batch_of_deep_columns():
    """Three deep columns in one set of launches (the apList kernels, unsplit), each against its own oracle run."""
    from lightweaver_amd.batch import ColumnBatch
    probs = [base_problem(333, seed=s) for s in (1, 2, 3)]
    refs = []
    for prob in probs:
        q = prob.copy()
        q.gamma_prefill()
        refs.append((q, OracleContext(q).formal_sol_gamma_matrices()[0]))
    with ColumnBatch(probs, fused=True, device_profiles=False) as batch:
        assert batch._batch is not None
        for c in batch.contexts:
            assert c.sweep_kind() == 'march' and c.depth_split() == 1
        ups = batch.formal_sol_gamma_matrices()
        batch.download()
    for p, (q, dJ), up in zip(probs, refs, ups):
        assert up.dJMax == pytest.approx(dJ, rel=TOL_ONE_CALL)
        compare_problems(p, q)


def test_deterministic_flag_on_a_deep_column():
    """LWHIP_OPT_DETERMINISTIC orders the lane sweep's sums; the march ignores it -- it sums by atomics, so bit-reproducibility
    is NOT promised at this depth -- and the split is what the rule gives without the flag.  Parity only."""
    prob, q, dJ = _base_and_oracle(333)
    p = prob.copy()
    with march(p, 4, deterministic=True) as ctx:
        p.gamma_prefill()
        up = ctx.formal_sol_gamma_matrices()
    assert up.dJMax == pytest.approx(dJ, rel=TOL_ONE_CALL)
    compare_problems(p, q)


def test_two_wavelength_shards_of_a_split_column():
    """Two contexts owning [0, m) and [m, Nlambda), each with its sweep split, their reduce buffers added on the host as
    test_wavelength_shards_sum_to_whole does: Gamma and the rates equal the whole run's to 1e-9, the J rows bit for bit."""
    prob = _base_and_oracle(333)[0]
    hip = C.cdll.LoadLibrary('libamdhip64.so')
    whole = prob.copy()
    with march(whole, 4) as ctx:
        whole.gamma_prefill()
        upWhole = ctx.formal_sol_gamma_matrices()
    m = prob.Nlambda // 2 + 3
    pa, pb = prob.copy(), prob.copy()
    with march(pa, 4, laStart=0, laEnd=m, worldSize=2, worldRank=0) as A, \
            march(pb, 4, laStart=m, laEnd=prob.Nlambda, worldSize=2, worldRank=1) as B:
        bufs = []
        for c in (A, B):
            c.prob.gamma_prefill()
            c.upload(abi.GAMMA)
            c.fs_partial()
            ptr, n = c.reduce_buffer()
            c.synchronize()
            host = np.zeros(n)
            assert hip.hipMemcpy(host.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_size_t(n * 8), 2) == 0
            bufs.append(host)
        total = bufs[0] + bufs[1]
        for c in (A, B):
            ptr, n = c.reduce_buffer()
            assert hip.hipMemcpy(C.c_void_p(ptr), total.ctypes.data_as(C.c_void_p), C.c_size_t(n * 8), 1) == 0
            up = c.fs_finalise()
            assert up.dJMax == upWhole.dJMax
            c.download(abi.ALL_OUTPUTS)
    for p in (pa, pb):
        compare_problems(p, whole, tol=TOL_ONE_CALL, what=('Gamma', 'R'))
    assert np.array_equal(pa.J[:m], whole.J[:m]) and np.array_equal(pb.J[m:], whole.J[m:])
    compare_problems(whole, _base_and_oracle(333)[1])


# ---- h. convergence -------------------------------------------------------------------------------------------------------
def test_twenty_device_resident_iterations_of_a_split_column():
    """As test_iter20_golden_device_resident: 20 iterations with populations, J and Gamma never leaving HBM, stat_equil from
    the fourth on; against the oracle driven the same way on the host."""
    prob = _base_and_oracle(257)[0]
    q = prob.copy()
    with OracleContext(q) as oc:
        for it in range(20):
            q.gamma_prefill()
            oc.formal_sol_gamma_matrices()
            if it >= 3:
                assert oc.stat_equil() == 0
    p = prob.copy()
    with march(p, 4) as ctx:
        for it in range(20):
            ctx.formal_sol_gamma_matrices(deviceResident=True)
            if it >= 3:
                ctx.stat_equil(deviceResident=True)
        ctx.download(abi.ALL_OUTPUTS | abi.POPS)
    compare_problems(p, q, tol=TOL_CONVERGED, what=('J', 'n'))
