"""The lane sweep's parity matrix: every lane geometry the depth count can give (lane_sweep_supported: D = 4 points per lane,
LR = ceil(Ns / 4) lanes per ray for 13 <= Ns <= 256, R = min(64 / LR, 16) wavelengths per wavefront, ((Ns - 1) % 4) + 1 real
points in a ray's last lane), asserted through Context.sweep_kind() / Context.layout_1d() (lwhip_layout_1d) and compared with
the C oracle, which the CPU tests at the end of this file tie bit for bit to the reference's core at the same depth counts.

    Ns        LR   R   last lane   why
    13         4  16   1           the minimum: sixteen rays per wavefront, c.rRaw up to 15, every tile partly filled
    15         4  16   3           Ns % 4 == 3
    16         4  16   4           full lanes, no idle lane
    17         5  12   1           4 idle lanes; R not a power of two
    31         8   8   3
    82        21   3   2           the size of nearly every other test (Ns % 4 == 2 at R > 1)
    127, 128  32   2   3, 4        the last depth counts at which ls_scan skips its sixth step
    129       33   1   1           the first with the sixth step; 31 idle lanes
    130       33   1   2           (Ns % 4 == 2 at R = 1)
    131       33   1   3
    253       64   1   1           lane 63 holds one point
    255, 256  64   1   3, 4        three points / the whole wavefront

a.  every row x {static, moving} x {Bezier, linear, BESSER} under LWHIP_SWEEP=lanes against the oracle; 12 and 257 points
    report 'march' under the same setting and match too; hybrid PRD at 12 points is refused.
b.  the other instances at the edge set E = {13, 15, 129, 253}, moving unless stated: the ray split (1 / 2 / 4 / default),
    LWHIP_LWAVES = 2 / 8, the general finish, the three boundary pairs (static and moving, E + 16 + 82: one depth count per
    position of the lower boundary point in the last lane; the 1D library refuses no pair of ZERO / THERMALISED / CALLABLE, so
    none is left out; the pair with the THERMALISED upper boundary without the PRD call, see boundary_prd), formal_sol, lambdaIterate, depth data, the fixed-order mode, hybrid PRD, overlapping lines (15, 129),
    wavelength shards (13, 17), the fused batch (13, 253), ten iterations (13, 253).
c.  CPU: the table above from the formula; the oracle against the reference's core.

The base problem: models.falc_h_ca(Nrays=3, lineScale=0.3, prd=True) on FAL-C resampled to Ns points (static: FAL-C has no
velocities) or on models.perturbed(that, seed=3) (moving) -- tiles with no line, one line, a line and a mixed continuum, and
PRD lines.  One "call" is gamma_prefill, formal_sol_gamma_matrices, redistribute_prd(2, 0.0).

Bounds, all the project's own: 1e-9 element-wise after one call (TOL_ONE_CALL) on J, I, Gamma, Rij / Rji and rhoPrd; 1e-6 on
iterated J and populations (TOL_CONVERGED); between two layouts of one problem 1e-12 on J and I, 1e-10 where a PRD
sub-iteration intervenes (test_lane_sweep_ray_split_vs_oracle); the fused batch at test_column_batch_vs_oracle's 1e-7; the
shards at test_wavelength_shards_sum_to_whole's 1e-12 on Gamma; bit equality where a test says so.

Wavefronts per workgroup: every workgroup stages the depth arena (n, wphi, ratio: 37 rows of Ns doubles for H(6) + Ca II(6))
in its LDS next to its accumulator slots (seven transitions at one wavelength, 4 x 4 LR doubles each) and 6.9 KB per
wavefront: with four wavefronts 162 944 bytes at 244 points and 164 264 at 245, of the 163 840 a workgroup has.  Up to 244
points a context keeps the four it is asked for; from 245 on (253: 168 680 bytes) build_tables halves them to two (154 776
at 253), which also ends the ray split, a thing of four-wavefront workgroups.  Before this matrix such a context was created and then failed at every launch
(hipFuncSetAttribute: invalid argument).  workgroup_waves() states the rule for the cases here; layout_1d must report it.

Every oracle result is computed once (functools.lru_cache) and only ever read or copied.
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
from oracle import bindings
from oracle.bindings import OracleContext
from test_hip_parity import compare_problems

SOLVERS = [abi.FS_BEZIER3_1D, abi.FS_LINEAR_1D, abi.FS_BESSER_1D]
SOLVER_IDS = ['bezier', 'linear', 'besser']
# (Ns, LR, R, points in the last lane): the table of the docstring
GEOMETRY = [(13, 4, 16, 1), (15, 4, 16, 3), (16, 4, 16, 4), (17, 5, 12, 1), (31, 8, 8, 3), (82, 21, 3, 2), (127, 32, 2, 3),
            (128, 32, 2, 4), (129, 33, 1, 1), (130, 33, 1, 2), (131, 33, 1, 3), (253, 64, 1, 1), (255, 64, 1, 3), (256, 64, 1, 4)]
DEPTHS = [g[0] for g in GEOMETRY]
EDGES = [13, 15, 129, 253]
MOTION = [False, True]
MOTION_IDS = ['static', 'moving']
KNOBS = ('LWHIP_LANE_SPLIT', 'LWHIP_LWAVES', 'LWHIP_FIN_FAST', 'LWHIP_PAIR_RAYS', 'LWHIP_ISO_RAYS', 'LWHIP_TILE_GENERIC',
         'LWHIP_LANE_GENERIC', 'LWHIP_DEPTH_SPLIT')


def lane_geometry(Ns):
    """(LR, R, points in the last lane) of lane_sweep_supported, or None where it refuses the depth count."""
    D = 4
    LR = (Ns + D - 1) // D
    if LR < 4 or LR > 64:
        return None
    return LR, min(64 // LR, 16), (Ns - 1) % D + 1


def workgroup_waves(Ns, asked=4):
    """Wavefronts per workgroup of a base-problem context (the docstring's LDS count): as asked up to 244 points, at most two
    beyond."""
    return asked if Ns <= 244 else min(asked, 2)


@pytest.fixture(autouse=True)
def lanes_forced(monkeypatch):
    """LWHIP_SWEEP=lanes, every other layout knob at its default."""
    monkeypatch.setenv('LWHIP_SWEEP', 'lanes')
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def column(Ns, moving):
    A = models.resample(models.falc82(), Ns)
    return models.perturbed(A, seed=3) if moving else A


@functools.lru_cache(maxsize=None)
def base_problem(Ns, moving, solver=abi.FS_BEZIER3_1D, storeDepthData=False):
    """Built once, only ever copied."""
    return models.falc_h_ca(Nrays=3, lineScale=0.3, prd=True, atmos=column(Ns, moving), formalSolver=solver,
                            storeDepthData=storeDepthData)


def oracle_call(prob, lambdaIterate=False, prd=True):
    """One call of the oracle on a copy of `prob`: (problem, dJMax, NprdSubIter)."""
    q = prob.copy()
    with OracleContext(q) as oc:
        q.gamma_prefill()
        dJ, _ = oc.formal_sol_gamma_matrices(lambdaIterate=lambdaIterate)
        n = oc.redistribute_prd(2, 0.0)['NprdSubIter'] if prd else 0
    return q, dJ, n


@functools.lru_cache(maxsize=None)
def base_and_oracle(Ns, moving, solver=abi.FS_BEZIER3_1D):
    prob = base_problem(Ns, moving, solver)
    return (prob,) + oracle_call(prob)


def prd_lines(p):
    return [t for a in p.atoms for t in a.trans if t.rhoPrd is not None]


def compare_all(got, want, tol=TOL_ONE_CALL, what=('J', 'I', 'Gamma', 'R'), rho=True):
    """compare_problems + rhoPrd of the PRD lines; prints the worst relative error of every quantity."""
    worst = compare_problems(got, want, tol=tol, what=what)
    if rho:
        la, lb = prd_lines(got), prd_lines(want)
        assert len(la) == len(lb) > 0
        worst['rhoPrd'] = max(rel_err(a.rhoPrd, b.rhoPrd) for a, b in zip(la, lb))
        assert worst['rhoPrd'] <= tol, worst
    print('WORST', {k: float(f'{v:.3g}') for k, v in worst.items()})
    return worst


def lanes(p, **kw):
    """A context of `p` that must run the lane sweep with the geometry its depth count gives."""
    ctx = Context(p, **kw)
    try:
        assert ctx.sweep_kind() == 'lanes'
        lay = ctx.layout_1d()
        LR, R, _ = lane_geometry(p.Nspace)
        assert (lay['sweep'], lay['D'], lay['LR'], lay['R']) == ('lanes', 4, LR, R), lay
        assert lay['nTiles'] >= (ctx.laEnd - ctx.laStart + R - 1) // R and lay['laneSplit'] in (1, 2, 4)
    except BaseException:
        ctx.close()
        raise
    return ctx


def one_call(prob, prd=True, lambdaIterate=False, pairing=None, expect=None, **kw):
    """One call on a copy of `prob` through the lane sweep; `pairing`: what layout_1d must say of ray pairs; `expect`:
    further layout entries."""
    p = prob.copy()
    with lanes(p, **kw) as ctx:
        p.gamma_prefill()
        up = ctx.formal_sol_gamma_matrices(lambdaIterate=lambdaIterate)
        sub = ctx.redistribute_prd(2, 0.0).NprdSubIter if prd else 0
        lay = ctx.layout_1d()
    if pairing is not None:
        assert lay['pairRays'] == pairing, lay
        assert lay['isoRays'] <= lay['pairRays']
    for k, v in (expect or {}).items():
        assert lay[k] == v, (k, lay)
    return p, up, sub, lay


# ---- a. geometry x motion x solver ----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('solver', SOLVERS, ids=SOLVER_IDS)
@pytest.mark.parametrize('moving', MOTION, ids=MOTION_IDS)
@pytest.mark.parametrize('Ns', DEPTHS)
def test_geometry_vs_oracle(gpu, Ns, moving, solver):
    """Every lane geometry, static (the rays of an angle paired) and moving (not paired), under the three solvers: one call
    against the oracle at the one-call bound."""
    prob, q, dJ, nsub = base_and_oracle(Ns, moving, solver)
    p, up, sub, _ = one_call(prob, pairing=not moving, expect={'tileWaves': workgroup_waves(Ns)})
    assert sub == nsub == 2
    compare_all(p, q)
    assert up.dJMax == pytest.approx(dJ, rel=TOL_ONE_CALL)


@pytest.mark.gpu
@pytest.mark.parametrize('Ns', [244, 245])
def test_workgroup_halved_where_four_wavefronts_do_not_fit(gpu, Ns):
    """The two depth counts either side of the LDS edge (LR = 61 with a full last lane, LR = 62 with one point in it): four
    wavefronts and the ray split at 244, two wavefronts with whole rays at 245; one call against the oracle."""
    assert (workgroup_waves(244), workgroup_waves(245)) == (4, 2)
    prob, q, dJ, _ = base_and_oracle(Ns, True)
    p, up, _, lay = one_call(prob, pairing=False, expect={'tileWaves': workgroup_waves(Ns)})
    assert (lay['laneSplit'] > 1) == (Ns == 244), lay
    compare_all(p, q)
    assert up.dJMax == pytest.approx(dJ, rel=TOL_ONE_CALL)


@pytest.mark.gpu
@pytest.mark.parametrize('solver', SOLVERS, ids=SOLVER_IDS)
@pytest.mark.parametrize('moving', MOTION, ids=MOTION_IDS)
@pytest.mark.parametrize('Ns', [12, 257])
def test_outside_the_range_the_march_serves(gpu, Ns, moving, solver):
    """One point below and one above what the lane sweep accepts: LWHIP_SWEEP=lanes or not, the context reports the march
    (no lane geometry), and the call matches the oracle."""
    assert lane_geometry(Ns) is None
    prob, q, dJ, nsub = base_and_oracle(Ns, moving, solver)
    p = prob.copy()
    with Context(p) as ctx:
        assert ctx.sweep_kind() == 'march'
        lay = ctx.layout_1d()
        assert (lay['sweep'], lay['D'], lay['LR'], lay['R'], lay['laneSplit'], lay['laneSplitPrd']) == ('march', 0, 0, 0, 1, 1), lay
        p.gamma_prefill()
        up = ctx.formal_sol_gamma_matrices()
        assert ctx.redistribute_prd(2, 0.0).NprdSubIter == nsub
    compare_all(p, q)
    assert up.dJMax == pytest.approx(dJ, rel=TOL_ONE_CALL)


@pytest.mark.gpu
def test_hybrid_prd_below_the_range_is_refused(gpu):
    prob = base_problem(12, True)
    with OracleContext(prob.copy()) as oc:
        tables = oc.build_hprd()
        try:
            with pytest.raises(LwHipError, match=rf'\({abi.ERR_UNSUPPORTED}\).*hybrid PRD needs the depth-across-lanes sweep'):
                Context(prob.copy(), hprd=tables)
        finally:
            tables.close()


@pytest.mark.gpu
def test_layout_1d_refuses_a_2d_context_and_changes_nothing(gpu):
    """The query is the counterpart of layout_2d: a 2D context is refused with ERR_UNSUPPORTED, a null argument with
    ERR_INVALID; asked twice, and again after a call, a 1D context gives the same geometry."""
    from test_fs2d_matrix import problem as problem_2d
    with Context(problem_2d(37)) as ctx:
        assert ctx.sweep_kind() == '2d'
        with pytest.raises(LwHipError, match=rf'\({abi.ERR_UNSUPPORTED}\).*layout_1d'):
            ctx.layout_1d()
    p = base_problem(13, True).copy()
    with lanes(p) as ctx:
        assert ctx.lib.lwhip_layout_1d(ctx._h, None) == abi.ERR_INVALID
        first = ctx.layout_1d()
        assert ctx.layout_1d() == first
        ctx.formal_sol_gamma_matrices()
        assert ctx.layout_1d() == first


# ---- b. the other instances at the edge set -------------------------------------------------------------------------------
def default_split(nTiles, slotsFull, room):
    """build_tables' rule for one small problem: S wavefronts per tile while they fit `room` of one round of wavefronts."""
    return 4 if 4 * nTiles <= slotsFull * room else 2 if 2 * nTiles <= slotsFull else 1


@pytest.mark.gpu
@pytest.mark.parametrize('Ns', EDGES)
def test_ray_split(gpu, monkeypatch, Ns):
    """A tile's rays over S = 1 / 2 / 4 wavefronts (LWHIP_LANE_SPLIT) and what the library picks by itself: each against the
    oracle; pairwise to 1e-12 on J and I of the iteration and 1e-10 after the PRD call; twice from the same inputs the
    iteration's J and I are the same bits.  At 253 points the workgroups have two wavefronts and the rays stay whole,
    whatever is asked for: the same comparisons, of runs that then share one layout."""
    import torch
    prob, q, dJ, _ = base_and_oracle(Ns, True)
    slots = 2 * 4 * torch.cuda.get_device_properties(0).multi_processor_count
    plain, full = {}, {}
    splits = workgroup_waves(Ns) == 4
    for S in (1, 2, 4, None):
        if S is None:
            monkeypatch.delenv('LWHIP_LANE_SPLIT')
        else:
            monkeypatch.setenv('LWHIP_LANE_SPLIT', str(S))
        want = {'tileWaves': workgroup_waves(Ns)}
        if S is not None or not splits:
            want.update(laneSplit=S if splits else 1, laneSplitPrd=S if splits else 1)
        a, _, _, lay = one_call(prob, prd=False, expect=want)
        b, _, _, _ = one_call(prob, prd=False)
        if S is None and splits:
            # (the PRD rates pass has fewer tiles and more room: never a smaller split)
            assert lay['laneSplit'] == default_split(lay['nTiles'], slots, 0.9), lay
            assert lay['laneSplitPrd'] >= lay['laneSplit'], lay
        assert np.array_equal(a.J, b.J) and np.array_equal(a.I, b.I), S
        plain[S] = a
        full[S], up, _, _ = one_call(prob, expect=want)
        assert up.dJMax == pytest.approx(dJ, rel=TOL_ONE_CALL)
        compare_all(full[S], q)
    keys = list(plain)
    for i, x in enumerate(keys):
        for y in keys[i + 1:]:
            compare_problems(plain[x], plain[y], tol=1e-12, what=('J', 'I'))
            compare_problems(full[x], full[y], tol=1e-10, what=('J', 'I'))


@pytest.mark.gpu
@pytest.mark.parametrize('env,asked', [({'LWHIP_LWAVES': '2'}, 2), ({'LWHIP_LWAVES': '8'}, 8), ({'LWHIP_FIN_FAST': '0'}, 4)],
                         ids=['lwaves2', 'lwaves8', 'fin_general'])
@pytest.mark.parametrize('Ns', EDGES)
def test_workgroup_shapes_and_the_general_finish(gpu, monkeypatch, Ns, env, asked):
    """Two and eight wavefronts (tiles) per workgroup -- at 253 points two either way, see the docstring -- and the finish's
    general (program-decoding) form."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    prob, q, dJ, _ = base_and_oracle(Ns, True)
    p, up, _, _ = one_call(prob, expect={'tileWaves': workgroup_waves(Ns, asked)})
    compare_all(p, q)
    assert up.dJMax == pytest.approx(dJ, rel=TOL_ONE_CALL)


BOUNDARIES = ['zero-thermalised', 'thermalised-callable', 'callable-zero']   # (upper, lower)


def with_boundaries(prob, which):
    p = prob.copy()
    rng = np.random.default_rng(11)
    Nrays = p.Nrays
    idxs = np.full((Nrays, 2), -1, dtype=np.int32)
    if which == 'thermalised-callable':      # (what the golden `bc` variant does at 82 points)
        idxs[:, 1] = np.arange(Nrays)[::-1]
        p.zUpperBc = Boundary(abi.BC_THERMALISED)
        p.zLowerBc = Boundary(abi.BC_CALLABLE, idxs=idxs, bcData=(1.0 + 0.3 * rng.random((p.Nlambda, Nrays))) * p.J[:, -1, None])
    elif which == 'callable-zero':
        idxs[:, 0] = np.arange(Nrays)
        # (a weak illumination from above: fractions of the starting field -- the Planck function -- at its coolest depth.  Of
        # the hot top's Planck function instead, the oracle's own rho turns negative in the sub-iterations: no relative bound)
        p.zUpperBc = Boundary(abi.BC_CALLABLE, idxs=idxs,
                              bcData=(0.05 + 0.2 * rng.random((p.Nlambda, Nrays))) * p.J.min(axis=1)[:, None])
        p.zLowerBc = Boundary(abi.BC_ZERO)
    else:
        assert (p.zUpperBc.type, p.zLowerBc.type) == (abi.BC_ZERO, abi.BC_THERMALISED)
    p.gamma_prefill()
    return p


def boundary_prd(which):
    """A THERMALISED upper boundary extrapolates the Planck function across the optically thin top, and a PRD sub-iteration
    on the J that gives ends, in the oracle itself, at rho of -85, negative opacities and intensities of 1e115: that pair runs
    the iteration alone, as the golden `bc` variant and test_boundary_conditions_on_a_split_column do (J then stays positive).
    The other two make the whole call; their rho stays within 0.1 .. 4 (asserted)."""
    return which != 'thermalised-callable'


@functools.lru_cache(maxsize=None)
def boundary_case(Ns, moving, which):
    prob = with_boundaries(base_problem(Ns, moving), which)
    q, dJ, n = oracle_call(prob, prd=boundary_prd(which))
    assert q.J.min() > 0.0 and all(0.05 < t.rhoPrd.min() and t.rhoPrd.max() < 5.0 for t in prd_lines(q))
    return prob, q, dJ, n


@pytest.mark.gpu
@pytest.mark.parametrize('which', BOUNDARIES)
@pytest.mark.parametrize('moving', MOTION, ids=MOTION_IDS)
@pytest.mark.parametrize('Ns', EDGES + [16, 82])
def test_boundaries(gpu, Ns, moving, which):
    """The intensity entering at the first point of either direction: the lower boundary point sits at position
    (Ns - 1) % 4 of the last lane -- 0 (13, 129, 253), 1 (82), 2 (15), 3 (16)."""
    prob, q, dJ, _ = boundary_case(Ns, moving, which)
    if which != BOUNDARIES[0]:
        assert not np.array_equal(q.I, boundary_case(Ns, moving, BOUNDARIES[0])[1].I)   # the boundaries matter
    p, up, _, _ = one_call(prob, prd=boundary_prd(which), pairing=not moving)
    compare_all(p, q, rho=boundary_prd(which))
    assert up.dJMax == pytest.approx(dJ, rel=TOL_ONE_CALL)


@pytest.mark.gpu
@pytest.mark.parametrize('upOnly', [True, False])
@pytest.mark.parametrize('Ns', EDGES)
def test_formal_sol(gpu, Ns, upOnly):
    prob = base_problem(Ns, True)
    q = prob.copy()
    OracleContext(q).formal_sol(upOnly=upOnly)
    p = prob.copy()
    J0 = p.J.copy()
    with lanes(p) as ctx:
        ctx.formal_sol(upOnly=upOnly)
        ctx.download(abi.J)
    assert q.I.max() > 0.0 and rel_err(p.I, q.I) <= TOL_ONE_CALL
    print('WORST', {'I': rel_err(p.I, q.I)})
    assert np.array_equal(p.J, J0)


@pytest.mark.gpu
@pytest.mark.parametrize('Ns', EDGES)
def test_lambda_iterate(gpu, Ns):
    prob, qfull, _, _ = base_and_oracle(Ns, True)
    q, dJ, _ = oracle_call(prob, lambdaIterate=True, prd=False)
    assert not np.array_equal(q.atoms[0].Gamma, qfull.atoms[0].Gamma)
    p, up, _, _ = one_call(prob, prd=False, lambdaIterate=True)
    compare_all(p, q, rho=False)
    assert up.dJMax == pytest.approx(dJ, rel=TOL_ONE_CALL)


@pytest.mark.gpu
@pytest.mark.parametrize('Ns', EDGES)
def test_depth_data(gpu, Ns):
    """storeDepthData: chi, eta and I of both directions at every depth -- the stores of a partly filled last lane."""
    prob = base_problem(Ns, True, storeDepthData=True)
    q, _, _ = oracle_call(prob, prd=False)
    assert q.depthI.shape == (prob.Nlambda, 3, 2, Ns) and q.depthI.min() >= 0.0 and q.depthChi.min() > 0.0
    p, _, _, _ = one_call(prob, prd=False)
    worst = {name: rel_err(getattr(p, name), getattr(q, name)) for name in ('depthChi', 'depthEta', 'depthI')}
    print('WORST', worst)
    assert all(e <= TOL_ONE_CALL for e in worst.values()), worst
    compare_all(p, q, rho=False)


def assert_same_bits(a, b):
    assert np.array_equal(a.J, b.J) and np.array_equal(a.I, b.I)
    for x, y in zip(a.atoms, b.atoms):
        assert np.array_equal(x.Gamma, y.Gamma)
        for tx, ty in zip(x.trans, y.trans):
            assert np.array_equal(tx.Rij, ty.Rij) and np.array_equal(tx.Rji, ty.Rji)
            if tx.rhoPrd is not None:
                assert np.array_equal(tx.rhoPrd, ty.rhoPrd)


@pytest.mark.gpu
@pytest.mark.parametrize('Ns', EDGES)
def test_fixed_order_mode(gpu, Ns):
    """LWHIP_OPT_DETERMINISTIC: against the oracle, and twice from the same inputs the same bits in J, I, Gamma, the rates
    and rho."""
    prob, q, dJ, _ = base_and_oracle(Ns, True)
    a, up, _, _ = one_call(prob, deterministic=True)
    b, _, _, _ = one_call(prob, deterministic=True)
    compare_all(a, q)
    assert up.dJMax == pytest.approx(dJ, rel=TOL_ONE_CALL)
    assert_same_bits(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize('solver', [abi.FS_BEZIER3_1D, abi.FS_LINEAR_1D], ids=['bezier', 'linear'])
@pytest.mark.parametrize('Ns', EDGES)
def test_hybrid_prd(gpu, Ns, solver):
    """test_hip_hprd_single_call_matches_oracle at the edge depth counts: J, JRest, rho, Gamma and the rates."""
    from test_hprd import assert_same, hprd_problem, run_hprd, run_hprd_hip
    prob = hprd_problem(formalSolver=solver, Nspace=Ns)
    assert prob.Nspace == Ns and np.abs(prob.vlosMu).max() > 1.0e3
    with OracleContext(prob.copy()) as oc:
        tables = oc.build_hprd()
        try:
            with lanes(prob.copy(), hprd=tables):
                pass
        finally:
            tables.close()
    po, uo, Jo = run_hprd(OracleContext, prob, nIter=1, prdIter=2)
    ph, uh, Jh = run_hprd_hip(prob, nIter=1, prdIter=2)
    assert uo[0]['NprdSubIter'] == uh[0].NprdSubIter == 2
    assert np.abs(Jo).max() > 0.0
    print('WORST', {'JRest': rel_err(Jh, Jo)})
    assert rel_err(Jh, Jo) <= TOL_ONE_CALL
    compare_all(ph, po)
    assert_same(po, ph, TOL_ONE_CALL)


@pytest.mark.gpu
@pytest.mark.parametrize('ncopy,maxlines', [(2, 4), (3, 6)])
@pytest.mark.parametrize('Ns', [15, 129])
def test_overlapping_lines(gpu, Ns, ncopy, maxlines):
    """The problems of test_more_than_two_overlapping_lines (blended Ca II copies: up to 4 / 6 lines at one wavelength, the
    tiles of the lane sweep's generic kind next to the compiled ones) on a moving column at 15 and 129 points.  A tile's
    accumulators are [transitions at its wavelengths][4][4 LR] doubles and may have 64 KB: H + three Ca II (17 transitions
    at one wavelength) at 129 points would need 71 808 bytes, so the library takes the march there (lwhip_create used to
    fail); the other three run the lane sweep."""
    from test_fs2d import blended_atoms
    prob = models.build_problem(column(Ns, True), blended_atoms(ncopy, 0.3), Nrays=3)
    lines = np.zeros(prob.Nlambda, dtype=int)
    for a in prob.atoms:
        for t in a.trans:
            if t.type == abi.LINE:
                lines[t.Nblue:t.Nred] += 1
    assert lines.max() == maxlines
    slots = np.zeros(prob.Nlambda, dtype=int)
    for a in prob.atoms:
        for t in a.trans:
            slots[t.Nblue:t.Nred] += 1
    fits = 8 * slots.max() * 4 * 4 * lane_geometry(Ns)[0] <= 64 * 1024
    assert fits == ((Ns, ncopy) != (129, 3)) and (ncopy != 3 or slots.max() == 17)
    q, dJ, _ = oracle_call(prob, prd=False)
    if fits:
        p, up, _, _ = one_call(prob, prd=False, pairing=False)
    else:
        p = prob.copy()
        with Context(p) as ctx:
            assert ctx.sweep_kind() == 'march' and ctx.layout_1d()['LR'] == 0
            up = ctx.formal_sol_gamma_matrices()
    compare_all(p, q, rho=False)
    assert up.dJMax == pytest.approx(dJ, rel=TOL_ONE_CALL)


@pytest.mark.gpu
@pytest.mark.parametrize('Ns', [13, 17])
def test_wavelength_shards(gpu, Ns):
    """Shards [0, k) and [k, Nlambda) for three cuts put one wavelength into different ray slots of its wavefront (R = 16
    and 12): I of formal_sol is the whole grid's bit for bit (ls_scan: a ray's result does not depend on its neighbours in
    the wavefront), and the iteration's sums add up to the whole run's as in test_wavelength_shards_sum_to_whole."""
    prob = base_problem(Ns, True)
    hip = C.cdll.LoadLibrary('libamdhip64.so')
    fs = prob.copy()
    with lanes(fs) as ctx:
        ctx.formal_sol(upOnly=False)
    assert fs.I.min() > 0.0
    whole = prob.copy()
    with lanes(whole) as ctx:
        upWhole = ctx.formal_sol_gamma_matrices()
    Nla = prob.Nlambda
    for k in (Nla // 2, Nla // 2 + 1, Nla // 2 + 5):
        fa, fb = prob.copy(), prob.copy()
        with lanes(fa, laStart=0, laEnd=k, worldSize=2, worldRank=0) as A, \
                lanes(fb, laStart=k, laEnd=Nla, worldSize=2, worldRank=1) as B:
            A.formal_sol(upOnly=False)
            B.formal_sol(upOnly=False)
        assert np.array_equal(fa.I[:k], fs.I[:k]) and np.array_equal(fb.I[k:], fs.I[k:]), k
        pa, pb = prob.copy(), prob.copy()
        with lanes(pa, laStart=0, laEnd=k, worldSize=2, worldRank=0) as A, \
                lanes(pb, laStart=k, laEnd=Nla, worldSize=2, worldRank=1) as B:
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
                assert (up.dJMax, up.dJMaxIdx) == (upWhole.dJMax, upWhole.dJMaxIdx)
                c.download(abi.ALL_OUTPUTS)
        for ia in range(2):
            assert rel_err(pa.atoms[ia].Gamma, whole.atoms[ia].Gamma) <= 1e-12
            assert rel_err(pb.atoms[ia].Gamma, whole.atoms[ia].Gamma) <= 1e-12
        assert np.array_equal(pa.J[:k], whole.J[:k]) and np.array_equal(pb.J[k:], whole.J[k:])
        assert np.array_equal(pa.I[:k], whole.I[:k]) and np.array_equal(pb.I[k:], whole.I[k:])
    q = prob.copy()
    q.gamma_prefill()
    OracleContext(q).formal_sol_gamma_matrices()
    compare_all(whole, q, rho=False)


@functools.lru_cache(maxsize=None)
def batch_columns(Ns, oneMoving):
    """Three columns (temperatures perturbed; without velocities, or the middle one with) and two oracle iterations of each."""
    probs, refs = [], []
    for i in range(3):
        A = models.perturbed(models.resample(models.falc82(), Ns), seed=100 + i, dv=2.0e3 if (oneMoving and i == 1) else 0.0)
        prob = models.falc_h_ca(Nrays=3, lineScale=0.3, prd=True, atmos=A)
        q = prob.copy()
        with OracleContext(q) as oc:
            for it in range(2):
                q.gamma_prefill()
                dJ, _ = oc.formal_sol_gamma_matrices()
        probs.append(prob)
        refs.append((q, dJ))
    return probs, refs


@pytest.mark.gpu
@pytest.mark.parametrize('oneMoving', [False, True], ids=['all_static', 'one_moving'])
@pytest.mark.parametrize('Ns', [13, 253])
def test_fused_batch(gpu, Ns, oneMoving):
    """lanesweep_kernel<..., BATCH = true>: three columns in one set of launches, two iterations, every column against its
    own oracle run.  All static: every column reports ray pairs.  One moving: that column reports none, and the one launch
    that serves all three has to drop them."""
    from lightweaver_amd.batch import ColumnBatch
    built, refs = batch_columns(Ns, oneMoving)
    probs = [p.copy() for p in built]
    LR, R, _ = lane_geometry(Ns)
    with ColumnBatch(probs, fused=True, device_profiles=False) as batch:
        assert batch._batch is not None
        for i, c in enumerate(batch.contexts):
            lay = c.layout_1d()
            assert c.sweep_kind() == 'lanes' and (lay['D'], lay['LR'], lay['R'], lay['laneSplit']) == (4, LR, R, 1), lay
            assert lay['pairRays'] == (not (oneMoving and i == 1)), (i, lay)
        for it in range(2):
            ups = batch.formal_sol_gamma_matrices()
        batch.download()
    for p, (q, dJ), up in zip(probs, refs, ups):
        compare_all(p, q, tol=1e-7, rho=False)
        assert up.dJMax == pytest.approx(dJ, rel=1e-6)


@pytest.mark.gpu
@pytest.mark.parametrize('Ns', [13, 253])
def test_ten_device_resident_iterations(gpu, Ns):
    """As test_iter20_golden_device_resident: populations, J and Gamma never leave HBM, stat_equil from the fourth iteration
    on; against the oracle driven the same way on the host, whose populations must stay positive."""
    prob = base_problem(Ns, True)
    q = prob.copy()
    with OracleContext(q) as oc:
        for it in range(10):
            q.gamma_prefill()
            oc.formal_sol_gamma_matrices()
            if it >= 3:
                assert oc.stat_equil() == 0
                assert all(a.n.min() > 0.0 for a in q.atoms), (it, [float(a.n.min()) for a in q.atoms])
    p = prob.copy()
    with lanes(p) as ctx:
        for it in range(10):
            ctx.formal_sol_gamma_matrices(deviceResident=True)
            if it >= 3:
                ctx.stat_equil(deviceResident=True)
        ctx.download(abi.ALL_OUTPUTS | abi.POPS)
    compare_all(p, q, tol=TOL_CONVERGED, what=('J', 'n'), rho=False)


# ---- c. CPU ---------------------------------------------------------------------------------------------------------------
def test_case_table_follows_from_the_formula():
    for Ns, LR, R, last in GEOMETRY:
        assert lane_geometry(Ns) == (LR, R, last), Ns
    assert lane_geometry(12) is None and lane_geometry(257) is None
    assert lane_geometry(13) == (4, 16, 1) and lane_geometry(256) == (64, 1, 4)     # the ends of the range
    assert set(EDGES) <= set(DEPTHS)
    # the scan's sixth step: skipped up to LR = 32, taken from 33 on -- both sides of the edge are in the table
    assert {32, 33} <= {g[1] for g in GEOMETRY}


def test_case_table_covers_every_remainder():
    many = {Ns % 4 for Ns, LR, R, last in GEOMETRY if R > 1}
    one = {Ns % 4 for Ns, LR, R, last in GEOMETRY if R == 1}
    assert many == one == {0, 1, 2, 3}
    # the boundary cases: every position of the lower boundary point in the last lane
    assert {(Ns - 1) % 4 for Ns in EDGES + [16, 82]} == {0, 1, 2, 3}


def test_fal_c_is_static():
    assert not np.any(models.falc82().vlos) and not np.any(column(13, False).vlos) and np.any(column(13, True).vlos)
    assert 200 <= base_problem(13, False).Nlambda <= 300
    assert len(prd_lines(base_problem(13, False))) == 2


@pytest.mark.skipif(not bindings.ref_available(), reason='oracle/_ref/liblwref.so not built (no reference sources)')
@pytest.mark.parametrize('Ns', DEPTHS + [12, 257])
def test_oracle_equals_the_core_at_these_depth_counts(Ns):
    """What the GPU cases compare with is the reference's own result: one call of the oracle and of the real core from the
    same inputs, bit for bit, static and moving, under the three solvers."""
    from oracle.bindings import RefContext
    for moving in MOTION:
        for solver in SOLVERS:
            prob, q, dJ, nsub = base_and_oracle(Ns, moving, solver)
            r = prob.copy()
            with RefContext(r) as rc:
                r.gamma_prefill()
                rc.formal_sol_gamma_matrices()
                rc.redistribute_prd(2, 0.0)
            assert np.array_equal(q.J, r.J) and np.array_equal(q.I, r.I), (moving, solver)
            for a, b in zip(q.atoms, r.atoms):
                assert np.array_equal(a.Gamma, b.Gamma), (moving, solver)
                for ta, tb in zip(a.trans, b.trans):
                    assert np.array_equal(ta.Rij, tb.Rij) and np.array_equal(ta.Rji, tb.Rji), (moving, solver)
                    if ta.rhoPrd is not None:
                        assert np.array_equal(ta.rhoPrd, tb.rhoPrd), (moving, solver)
