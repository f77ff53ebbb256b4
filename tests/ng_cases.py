"""The synthetic Ng sequences of test_batch_ng.py and their recorded bits (tests/golden/ng_step_bits.json, written by
tools/record_ng_bits.py): what one Ng step leaves in n and reports, per (problem, Nspace, options, column, step)."""
import hashlib
import json
import os

import numpy as np

from lightweaver_amd import _abi as abi
from lightweaver_amd.harness import models

SEEDS = [100, 101, 102, 103, 107]
POPS_SCALE = (1.0e16, 1.0e10)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ng_step_bits.json')
NCOLUMNS, NSTEPS = 3, 12
OPTIONS = ((1, 1, 0), (2, 3, 5), (6, 4, 2), (6, 4, 8))
# (problem, Nspace, options) of every recorded sequence.  'H': one solved atom -- a column's first workgroup is also its last.
SEQUENCES = [('HCa', Ns, o) for Ns in (13, 32, 82) for o in OPTIONS] + [('H', 13, (2, 3, 5))]


def column(seed, Nspace=None, problem='HCa'):
    atmos = models.perturbed(models.falc82(), seed, dT=0.1, dv=2.0e3)
    if Nspace is not None:
        atmos = models.resample(atmos, Nspace)
    return models.build_problem(atmos, [models.H_6(0.3)] + ([models.CaII_6(0.3)] if problem == 'HCa' else []), Nrays=3)


class Synthetic:
    """One slowly converging sequence of positive vectors per (column, atom): the linear map of
    test_oracle_ng_matches_the_reference_struct, its own rng per column, scaled to population size."""

    def __init__(self, probs, seed0=7):
        self.target, self.x0 = [], []
        for i, p in enumerate(probs):
            rng = np.random.default_rng(seed0 + i)
            t = [1.0 + rng.random(a.n.shape) for a in p.atoms]
            self.target.append(t)
            self.x0.append([sc * (tt + 0.4 * rng.uniform(-1.0, 1.0, tt.shape)) for tt, sc in zip(t, POPS_SCALE)])

    def advance(self, i, xs):
        """The iteration being accelerated, applied to column i's current vectors."""
        out = []
        for x, t, sc in zip(xs, self.target[i], POPS_SCALE):
            d = (x / sc - t).ravel()
            out.append(sc * (t + (0.9 * d + 0.05 * np.roll(d, 1)).reshape(t.shape)))
        return out


def sequence_inputs(probs, opts):
    """The Synthetic of the recorded sequence with these options."""
    return Synthetic(probs, seed0=7 + opts[0])


def put(ctx, prob, xs):
    for a, x in zip(prob.atoms, xs):
        a.n[...] = x
    ctx.upload(abi.POPS)


def get(ctx, prob):
    ctx.download(abi.POPS)
    return [a.n.copy() for a in prob.atoms]


def lone_ng(ctx, nAtoms):
    """lwhip_ng_accelerate of a lone context: (status, accelerated, dPops, indices)."""
    acc = np.zeros(nAtoms, dtype=np.int32)
    dP, dI = np.zeros(nAtoms), np.zeros(nAtoms, dtype=np.int32)
    st = ctx.lib.lwhip_ng_accelerate(ctx._h, acc.ctypes.data_as(abi.i32p), dP.ctypes.data_as(abi.f64p), dI.ctypes.data_as(abi.i32p))
    return st, bool(acc.any()), dP.tolist(), dI.tolist()


def digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    return h.hexdigest()


def key(problem, Nspace, opts):
    return '%s/%d/%d,%d,%d' % ((problem, Nspace) + tuple(opts))


def step_record(n, accelerated, dPops, dPopsMaxIdx):
    """One step as the fixture holds it."""
    return dict(n=digest(n), dPops=[float(x).hex() for x in dPops], dPopsMaxIdx=[int(i) for i in dPopsMaxIdx],
                accelerated=bool(accelerated))


_golden = None


def golden(problem, Nspace, opts):
    """The recorded sequence: [column] -> dict(x0=digest, steps=[step_record ...])."""
    global _golden
    if _golden is None:
        with open(GOLDEN) as f:
            _golden = json.load(f)['sequences']
    return _golden[key(problem, Nspace, opts)]


def check_inputs(gold, syn):
    """A different numpy stream is not a kernel failure: said so, loudly, before any step is compared."""
    for i, g in enumerate(gold):
        assert digest(syn.x0[i]) == g['x0'], \
            'column %d: the synthetic INPUTS differ from the recorded ones (numpy random stream?): nothing about the kernel' % i


def check_step(gold, i, stepNo, who, n, accelerated, dPops, dPopsMaxIdx):
    got, want = step_record(n, accelerated, dPops, dPopsMaxIdx), gold[i]['steps'][stepNo - 1]
    assert got == want, (who, 'column', i, 'step', stepNo, got, want)
