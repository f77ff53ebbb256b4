"""The plain instance of the lane sweep (lanesweep_kernel<BEZIER3, 4, MODE bit 2>): a launch that writes no depth data and no
z-plane rows and has no CALLABLE boundary runs an instance in which those three are compiled out.  Which launches take it is
the host's choice per launch (lane_sweep_plain), reported by Context.sweep_instance() / ColumnBatch.sweep_instance() from the
members the launch reads; `LWHIP_LS_PLAIN=0` (read when a context is created) forces the full instance.  The arithmetic is
the same, so the results are the same bits: J and I in the default mode, Gamma and the rates as well in the fixed-order mode
(the default mode sums those with atomics in whatever order the workgroups arrive).  Problems as tests/test_iso_rays.py:
~1 024 wavelengths, 3 mu, one iteration; the oracle bound is the project's one-call 1e-9."""
import functools

import numpy as np
import pytest

from lightweaver_amd import _abi as abi
from lightweaver_amd.context import Context, LwHipError
from lightweaver_amd.harness import models
from oracle.bindings import OracleContext
from test_iso_rays import assert_iteration_matches, assert_same_bits, oracle_of

pytestmark = pytest.mark.gpu
KNOBS = ('LWHIP_LS_PLAIN', 'LWHIP_LANE_SPLIT', 'LWHIP_ISO_RAYS', 'LWHIP_PAIR_RAYS', 'LWHIP_LWAVES')
PLAIN = {'main': True, 'prdRates': False, 'lanes': True, 'switch': True}       # a context without PRD lines
FULL = {'main': False, 'prdRates': False, 'lanes': True, 'switch': True}


@pytest.fixture(autouse=True)
def lanes_forced(monkeypatch):
    monkeypatch.setenv('LWHIP_SWEEP', 'lanes')
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


@functools.lru_cache(maxsize=None)
def grid(moving=False, Ns=82, realistic=False, **kw):
    """Built once, only ever copied.  82 points: 21 lanes per ray, two points in the last one, three rays per wavefront."""
    A = models.falc82() if Ns == 82 else models.resample(models.falc82(), Ns)
    if moving:
        A = models.perturbed(A, seed=5)
    if realistic:
        assert Ns == 82 and not moving
        return models.throughput_grid(NlambdaTarget=1024, Nrays=3, realistic=True, **kw)
    return models.throughput_grid(NlambdaTarget=1024, Nrays=3, atmos=A, **kw)


@functools.lru_cache(maxsize=None)
def small(moving=False, **kw):
    """The matrix tests' base problem (H + Ca II, ~300 wavelengths; prd=True: Ca II H & K as PRD lines)."""
    A = models.perturbed(models.falc82(), seed=3) if moving else models.falc82()
    return models.falc_h_ca(Nrays=3, lineScale=0.3, atmos=A, **kw)


def instance_of(prob, **kw):
    with Context(prob.copy(), **kw) as ctx:
        return ctx.sweep_instance()


# ---- selection -------------------------------------------------------------------------------------------------------------
def test_default_context_is_plain_and_the_query_changes_nothing(gpu):
    p = grid().copy()
    with Context(p) as ctx:
        assert ctx.sweep_kind() == 'lanes'
        assert ctx.lib.lwhip_sweep_instance(ctx._h, None) == abi.ERR_INVALID
        assert ctx.sweep_instance() == PLAIN
        ctx.formal_sol_gamma_matrices()
        assert ctx.sweep_instance() == PLAIN
    assert instance_of(grid(moving=True)) == PLAIN


def test_2d_context_is_refused(gpu):
    from test_fs2d_matrix import problem as problem_2d
    with Context(problem_2d(37)) as ctx:
        with pytest.raises(LwHipError, match=rf'\({abi.ERR_UNSUPPORTED}\).*sweep_instance'):
            ctx.sweep_instance()


def test_depth_data_is_not_plain(gpu):
    assert instance_of(grid(storeDepthData=True)) == FULL


@pytest.mark.parametrize('which', ['thermalised-callable', 'callable-zero'], ids=['callable_lower', 'callable_upper'])
def test_callable_boundary_is_not_plain(gpu, which):
    from test_lanesweep_matrix import with_boundaries
    p = with_boundaries(small(), which)
    assert abi.BC_CALLABLE in (p.zUpperBc.type, p.zLowerBc.type)
    assert instance_of(p) == FULL


def test_zplane_outputs_are_not_plain_while_they_are_on(gpu):
    p = grid().copy()
    z = np.zeros((p.Nlambda, p.Nrays))
    with Context(p) as ctx:
        assert ctx.sweep_instance() == PLAIN
        ctx.set_zplane(down=z)
        assert ctx.sweep_instance() == FULL
        ctx.set_zplane(up=z)
        assert ctx.sweep_instance() == FULL
        ctx.set_zplane()
        assert ctx.sweep_instance() == PLAIN


def test_hybrid_prd_is_not_plain(gpu):
    from test_hprd import hprd_problem
    p = hprd_problem()
    with OracleContext(p.copy()) as oc:
        tables = oc.build_hprd()
        try:
            assert instance_of(p, hprd=tables) == FULL
        finally:
            tables.close()


@pytest.mark.parametrize('solver', [abi.FS_LINEAR_1D, abi.FS_BESSER_1D], ids=['linear', 'besser'])
def test_other_solvers_are_not_plain(gpu, solver):
    assert instance_of(small(formalSolver=solver)) == FULL
    assert instance_of(small(formalSolver=solver, prd=True)) == FULL


def test_march_is_not_plain(gpu, monkeypatch):
    monkeypatch.setenv('LWHIP_SWEEP', 'march')
    with Context(small().copy()) as ctx:
        assert ctx.sweep_kind() == 'march'
        assert ctx.sweep_instance() == {'main': False, 'prdRates': False, 'lanes': False, 'switch': True}


def test_prd_rates_pass_is_plain_even_with_depth_data(gpu):
    assert instance_of(small(prd=True)) == dict(PLAIN, prdRates=True)
    assert instance_of(small(prd=True, storeDepthData=True)) == dict(FULL, prdRates=True)


def test_switch_forces_the_full_instance(gpu, monkeypatch):
    monkeypatch.setenv('LWHIP_LS_PLAIN', '0')
    assert instance_of(grid()) == dict(FULL, switch=False)
    assert instance_of(small(prd=True)) == dict(FULL, switch=False)


def batch_columns(depthColumn=None):
    base = models.falc82()
    return [models.throughput_grid(NlambdaTarget=1024, Nrays=3, computeProfiles=False, storeDepthData=(i == depthColumn),
                                   atmos=models.perturbed(base, seed=100 + i, dv=0.0)) for i in range(3)]


def test_fused_batch_is_plain_only_if_every_column_is(gpu, monkeypatch):
    from lightweaver_amd.batch import ColumnBatch
    with ColumnBatch(batch_columns()) as batch:
        assert batch._batch is not None
        assert batch.sweep_instance() == PLAIN
    with ColumnBatch(batch_columns(depthColumn=1)) as batch:
        assert batch._batch is not None
        assert [c.sweep_instance()['main'] for c in batch.contexts] == [True, False, True]
        assert batch.sweep_instance() == FULL
    monkeypatch.setenv('LWHIP_LS_PLAIN', '0')
    with ColumnBatch(batch_columns()) as batch:
        assert batch.sweep_instance() == dict(FULL, switch=False)


# ---- the same bits ---------------------------------------------------------------------------------------------------------
def run(monkeypatch, prob, plain, deterministic=False, prd=False, **env):
    """One iteration of a copy of `prob` (and, prd: two PRD sub-iterations) through the plain or -- LWHIP_LS_PLAIN=0 -- the full
    instance; the context must say which."""
    monkeypatch.setenv('LWHIP_LS_PLAIN', '1' if plain else '0')
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    p = prob.copy()
    with Context(p, deterministic=deterministic) as ctx:
        assert ctx.sweep_kind() == 'lanes'
        inst = ctx.sweep_instance()
        assert inst['main'] == plain and inst['switch'] == plain, inst
        if prd:
            assert inst['prdRates'] == plain, inst
            p.gamma_prefill()
        ctx.formal_sol_gamma_matrices()
        if prd:
            assert ctx.redistribute_prd(2, 0.0).NprdSubIter == 2
        lay = ctx.layout_1d()
    return p, lay


def same_bits_both_modes(monkeypatch, prob, **env):
    """Plain against full: J and I in the default mode, Gamma, Rij and Rji as well in the fixed-order mode."""
    a, lay = run(monkeypatch, prob, True, **env)
    b, _ = run(monkeypatch, prob, False, **env)
    assert_same_bits(a, b, rates=False)
    da, _ = run(monkeypatch, prob, True, deterministic=True, **env)
    db, _ = run(monkeypatch, prob, False, deterministic=True, **env)
    assert_same_bits(da, db)
    return a, da, lay


@pytest.mark.parametrize('moving', [False, True], ids=['static_iso', 'moving_general'])
def test_same_bits_and_the_oracle(gpu, monkeypatch, moving):
    """The static grid (one-line tiles take the iso path: stencils once per wavefront) and the moving one (the general ray
    body); the plain results against the C oracle as well."""
    prob = grid(moving=moving)
    a, da, lay = same_bits_both_modes(monkeypatch, prob, LWHIP_LANE_SPLIT='1')
    assert (lay['LR'], lay['R'], lay['laneSplit'], lay['isoRays']) == (21, 3, 1, not moving), lay
    q = oracle_of(prob.copy())
    print(assert_iteration_matches(a, q), assert_iteration_matches(da, q))


@pytest.mark.parametrize('split', ['2', '4'])
def test_same_bits_split_rays(gpu, monkeypatch, split):
    _, _, lay = same_bits_both_modes(monkeypatch, grid(), LWHIP_LANE_SPLIT=split)
    assert lay['laneSplit'] == int(split), lay


def test_same_bits_generic_and_two_line_tiles(gpu, monkeypatch):
    """throughput_grid(realistic=True): the deuterium-like twin gives wavelengths with two lines (blends) and tiles no compiled
    kind covers (the generic kind)."""
    same_bits_both_modes(monkeypatch, grid(realistic=True))


def test_same_bits_one_ray_per_wavefront(gpu, monkeypatch):
    """131 points: 33 lanes per ray, so R = 1, three points in the last lane (82 points, above: R = 3, two points)."""
    for moving in (False, True):
        _, _, lay = same_bits_both_modes(monkeypatch, grid(moving=moving, Ns=131))
        assert (lay['LR'], lay['R']) == (33, 1), lay


def test_same_bits_prd_rates_pass(gpu, monkeypatch):
    """A PRD context: the iteration and two sub-iterations, whose rates pass takes the plain instance too; fixed-order mode,
    every output including rho."""
    from test_lanesweep_matrix import assert_same_bits as same_with_rho
    prob = small(moving=True, prd=True)
    a, _ = run(monkeypatch, prob, True, deterministic=True, prd=True)
    b, _ = run(monkeypatch, prob, False, deterministic=True, prd=True)
    same_with_rho(a, b)


def test_same_bits_fused_batch(gpu, monkeypatch):
    """Three columns in one set of launches (lanesweep_kernel<..., BATCH = true>), plain against full: J and I of every
    column."""
    from lightweaver_amd.batch import ColumnBatch
    out = {}
    for plain in (True, False):
        monkeypatch.setenv('LWHIP_LS_PLAIN', '1' if plain else '0')
        probs = batch_columns()
        with ColumnBatch(probs) as batch:
            assert batch._batch is not None and batch.sweep_instance()['main'] == plain
            batch.formal_sol_gamma_matrices()
            for c in batch.contexts:
                c.download(abi.ALL_OUTPUTS)
        out[plain] = probs
    for a, b in zip(out[True], out[False]):
        assert a.J.max() > 0.0
        assert_same_bits(a, b, rates=False)
