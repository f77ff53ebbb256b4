"""Time the observer rays of hybrid-PRD contexts (compute_rays_hprd) at mu = 1.

  (a) hybrid against plain: Context.compute_rays_hprd on a hybrid context at the timed size (FAL-C with a moving column, H + Ca II
      with H & K in PRD, ~10 240 wavelengths, 82 depths) next to Context.compute_rays on a plain-PRD context of the same problem,
      and the same pair for fused batches of C4 columns (tools/batch_hprd_time.py's: perturbed FAL-C, lineScale 3.1, ~3 000
      wavelengths, each column with its own velocities).  The two alternate call by call in one process; the ratio is what the
      in-kernel rho interpolation costs: per hybrid (line, point) one bisection over the line's grid and two rho reads for one.
  (b) the plain call against another build (--parent-root: a checkout of the parent commit with its library built): the same
      plain-PRD compute_rays, one child process per checkout -- this file, importing that checkout's package -- the children
      alternating --rounds times.  rays_kernel<false> is meant to be the parent's kernel.

Every timed call ends in a wait for the stream; shapes are warmed first; medians over --reps.  `spread` is what repeated identical
runs differ by: the same call timed as two interleaved series (A, A') in the same loop, |median A - median A'| / median A, and for
(b) the range of each library's per-round medians.  A ratio inside the spread is no difference.  Prints one JSON line.

    python tools/hprd_rays_time.py [--columns 64] [--reps 21] [--skip-batch] [--parent-root DIR [--rounds 3]]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

# (a child of (b) imports the package of the checkout it is told to time)
ROOT = (sys.argv[sys.argv.index('--child-root') + 1] if '--child-root' in sys.argv
        else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from lightweaver_amd.harness import models  # noqa: E402


def moving(atmos, amp, period=37.0):
    atmos.vlos = atmos.vlos + amp * np.sin(2.0 * np.pi * np.arange(atmos.Nspace) / period)
    return atmos


def set_rho(prob, seed=5):
    """A rho that is not 1 (the time does not depend on it; the comparison of the two results below does)."""
    rng = np.random.default_rng(seed)
    for a in prob.atoms:
        for t in a.trans:
            if t.rhoPrd is not None:
                t.rhoPrd[...] = 1.0 + 0.3 * rng.random(t.rhoPrd.shape)
    return prob


def lone_problem():
    return set_rho(models.throughput_grid(Nrays=3, prd=True, atmos=moving(models.falc82(), 8.0e3), computeProfiles=False))


def column_problems(n):
    base = models.falc82()
    return [set_rho(models.falc_h_ca(Nrays=5, lineScale=3.1, prd=True, computeProfiles=False,
                                     atmos=moving(models.perturbed(base, seed=1234 + c), (c % 9) * 2.5e3)), seed=c)
            for c in range(n)]


def interleaved_ms(fns, sync, reps):
    """Each of `fns` timed once per round, `reps` rounds: {name: [ms]}."""
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            ts[k].append((time.perf_counter() - t0) * 1e3)
    return ts


def summary(ts):
    med = {k: float(np.median(v)) for k, v in ts.items()}
    out = {k + '_ms': {'median': med[k], 'min': float(min(ts[k]))} for k in ts}
    out['spread'] = abs(med['plain'] - med['plain_again']) / med['plain']
    out['hybrid_over_plain'] = med['hybrid'] / med['plain']
    return out


def hybrid_points(prob, Nmu=1):
    """(line, wavelength, depth, ray) points that take the interpolation, and the bisection steps of each."""
    lines = [t for a in prob.atoms for t in a.trans if t.rhoPrd is not None]
    return {'hybrid_points': int(sum(t.Nlambda for t in lines) * prob.Nspace * Nmu),
            'bisection_reads_max': [int(np.ceil(np.log2(t.Nlambda))) + 1 for t in lines]}


def time_lone(reps):
    from lightweaver_amd.context import Context
    prob = lone_problem()
    with Context(prob.copy(), hprd=True) as h, Context(prob.copy()) as p:
        sync = lambda: (h.synchronize(), p.synchronize())   # noqa: E731
        a, b = h.compute_rays_hprd(1.0), p.compute_rays(1.0)    # (tables, staging, warm-up)
        for _ in range(3):
            h.compute_rays_hprd(1.0), p.compute_rays(1.0)
        ts = interleaved_ms({'hybrid': lambda: h.compute_rays_hprd(1.0), 'plain': lambda: p.compute_rays(1.0),
                             'plain_again': lambda: p.compute_rays(1.0)}, sync, reps)
    out = summary(ts)
    out.update(Nlambda=prob.Nlambda, Nspace=prob.Nspace, max_rel_diff_hybrid_vs_plain=float(np.max(np.abs(a / b - 1.0))),
               **hybrid_points(prob))
    return out


def time_batch(n, reps):
    from lightweaver_amd.batch import ColumnBatch
    probs = column_problems(n)
    with ColumnBatch([q.copy() for q in probs], hprd=True) as h, ColumnBatch([q.copy() for q in probs]) as p:
        assert h._batch is not None and p._batch is not None
        sync = lambda: (h.contexts[0].synchronize(), p.contexts[0].synchronize())   # noqa: E731
        a, b = h.compute_rays_hprd(1.0), p.compute_rays(1.0)
        for _ in range(3):
            h.compute_rays_hprd(1.0), p.compute_rays(1.0)
        ts = interleaved_ms({'hybrid': lambda: h.compute_rays_hprd(1.0), 'plain': lambda: p.compute_rays(1.0),
                             'plain_again': lambda: p.compute_rays(1.0)}, sync, reps)
    out = summary(ts)
    out.update(columns=n, Nlambda=probs[0].Nlambda, Nspace=probs[0].Nspace,
               max_rel_diff_hybrid_vs_plain=float(np.max(np.abs(a / b - 1.0))), **hybrid_points(probs[0]))
    return out


def plain_child(reps, columns):
    """One checkout's plain compute_rays on the plain-PRD problems of (a): medians of this process."""
    from lightweaver_amd import context
    from lightweaver_amd.batch import ColumnBatch
    assert os.path.dirname(os.path.abspath(context.__file__)) == os.path.join(os.path.abspath(ROOT), 'lightweaver_amd')
    out = {}
    with context.Context(lone_problem()) as p:
        for _ in range(4):
            p.compute_rays(1.0)
        out['lone_ms'] = float(np.median(interleaved_ms({'plain': lambda: p.compute_rays(1.0)}, p.synchronize, reps)['plain']))
    if columns:
        with ColumnBatch(column_problems(columns)) as b:
            for _ in range(4):
                b.compute_rays(1.0)
            out['batch_ms'] = float(np.median(interleaved_ms({'plain': lambda: b.compute_rays(1.0)},
                                                             b.contexts[0].synchronize, reps)['plain']))
    print(json.dumps(out))


def time_against(parent, rounds, reps, columns):
    res = {'this': [], 'parent': []}
    for _ in range(rounds):
        for who, root in (('this', ROOT), ('parent', parent)):
            cmd = [sys.executable, os.path.abspath(__file__), '--child-root', os.path.abspath(root), '--reps', str(reps)] \
                + (['--columns', str(columns)] if columns else ['--skip-batch'])
            r = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600)
            res[who].append(json.loads(r.stdout.strip().splitlines()[-1]))
    out = {}
    for key in res['this'][0]:
        t, p = [r[key] for r in res['this']], [r[key] for r in res['parent']]
        out[key] = {'this': t, 'parent': p, 'this_over_parent': float(np.median(t) / np.median(p)),
                    'spread_this': (max(t) - min(t)) / float(np.median(t)), 'spread_parent': (max(p) - min(p)) / float(np.median(p))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--columns', type=int, default=64)
    ap.add_argument('--reps', type=int, default=21)
    ap.add_argument('--skip-batch', action='store_true')
    ap.add_argument('--parent-root', default=None)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--child-root', default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    columns = 0 if args.skip_batch else args.columns
    if args.child_root:
        return plain_child(args.reps, columns)
    out = {'lone': time_lone(args.reps)}
    if columns:
        out['batch'] = time_batch(columns, args.reps)
    if args.parent_root:
        out['plain_vs_parent'] = time_against(args.parent_root, args.rounds, args.reps, columns)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
