"""The contexts whose structure tables tests/golden/table_signatures.json pins (Context.tables_signature(): one word for the
bytes of every structure-table buffer, one for the plan's scalars), shared by tools/record_table_signatures.py, which records
them, and tests/test_table_signatures.py, which holds every later library to them.  Creation only: nothing is iterated.

A case is (name, environment, make); make() creates its contexts and returns [(label, words or refusal)].  The environment's
knobs are read by the library at lwhip_create, under LWHIP_DEBUG."""
import contextlib
import os

import numpy as np

from lightweaver_amd import _abi as abi
from lightweaver_amd.context import Context, LwHipError
from lightweaver_amd.harness import models

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'table_signatures.json')
SOLVERS = {'linear': abi.FS_LINEAR_1D, 'besser': abi.FS_BESSER_1D, 'bezier3': abi.FS_BEZIER3_1D}
LINE_SCALE = 0.3


def falc(Ns):
    return models.resample(models.falc82(), Ns)


def h_ca(Ns, solver='bezier3', **kw):
    return models.falc_h_ca(Nrays=5, lineScale=LINE_SCALE, formalSolver=SOLVERS[solver], atmos=falc(Ns), **kw)


@contextlib.contextmanager
def environment(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def words(ctx):
    return ['%016x' % w for w in ctx.tables_signature()]


def created(prob, **kw):
    """The words of a context of `prob`, or the library's refusal."""
    try:
        with Context(prob, **kw) as ctx:
            return words(ctx)
    except LwHipError as e:
        return {'refused': str(e)}


def one(problem, **kw):
    return lambda: [('', created(problem(), **kw))]


def shards():
    prob = h_ca(82)
    m = prob.Nlambda // 2
    return [('rank0', created(prob.copy(), laStart=0, laEnd=m, worldSize=2, worldRank=0)),
            ('rank1', created(prob.copy(), laStart=m, laEnd=prob.Nlambda, worldSize=2, worldRank=1))]


def borrowing():
    prob = h_ca(82)
    with Context(prob.copy(), batchHint=4) as owner:
        with Context(prob.copy(), batchHint=4, like=owner) as col:
            assert col._like is owner, 'lwhip_create_like refused a problem of the same structure'
            return [('owner', words(owner)), ('borrower', words(col))]


def hybrid_prd():
    from oracle.bindings import OracleContext
    from test_hprd import hprd_problem
    prob = hprd_problem()
    tables = OracleContext(prob.copy()).build_hprd()
    return [('', created(prob, hprd=tables))]


def two_d():
    # the columns of test_fs2d.small_2d_problem, with the library's own intersection table
    base = falc(24)
    cols = [models.perturbed(base, seed=50 + j) for j in range(10)]
    return [('', created(models.build_problem_2d(cols, np.linspace(0.0, 9.0e5, 10), [models.H_6(0.12)])))]


def blended(ncopy, ls, Ns=82, Nrays=3):
    from test_fs2d import blended_atoms
    return models.build_problem(falc(Ns), blended_atoms(ncopy, ls), Nrays=Nrays)


def three_atoms(Ns):
    return models.build_problem(falc(Ns), [models.H_6(LINE_SCALE), models.D_6(LINE_SCALE), models.CaII_6(LINE_SCALE)], Nrays=5)


CASES = []
# a: every lane geometry (LR = 4 ... 64), both sides of the sixth scan step, the halved workgroup
for _solver in SOLVERS:
    for _Ns in (13, 16, 82, 129, 132, 244, 245, 256):
        CASES.append((f'a:{_solver}:Ns{_Ns}', {}, one(lambda s=_solver, n=_Ns: h_ca(n, s))))
# b: the march, its depth split and the LDS rule that turns it off
for _Ns in (12, 257, 500):
    CASES.append((f'b:Ns{_Ns}', {}, one(lambda n=_Ns: h_ca(n))))
CASES.append(('b:Ns500:split2', {'LWHIP_DEPTH_SPLIT': '2'}, one(lambda: h_ca(500))))
CASES.append(('b:Ns500:H+D+CaII', {}, one(lambda: three_atoms(500))))
# c: chunk split, dispatch order, tail chunks, generic tiles
CASES.append(('c:grid10240', {}, one(lambda: models.throughput_grid(10240))))
CASES.append(('c:grid2048:realistic', {}, one(lambda: models.throughput_grid(2048, realistic=True))))
CASES.append(('d:prd', {}, one(lambda: h_ca(82, prd=True))))
CASES.append(('e:hybrid-prd', {}, hybrid_prd))
CASES.append(('f:deterministic', {}, one(lambda: h_ca(82), deterministic=True)))
CASES.append(('g:shards', {}, shards))
CASES.append(('h:borrowing', {}, borrowing))
for _knob in ('LWHIP_SWEEP=march', 'LWHIP_TILE_GENERIC=1', 'LWHIP_LWAVES=2', 'LWHIP_LANE_GENERIC=0'):
    CASES.append((f'i:{_knob}', dict([_knob.split('=')]), one(lambda: h_ca(82))))
CASES.append(('j:2d', {}, two_d))
# k: refusals, with the code and the message
CASES.append(('k:nine-lines', {}, one(lambda: blended(5, 0.3))))
CASES.append(('k:lds-budget', {}, one(lambda: blended(3, 0.04, Ns=1024, Nrays=5))))


def compute_units():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def run(case):
    name, env, make = case
    with environment(env):
        return make()
