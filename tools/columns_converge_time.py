"""Time a 1.5D column batch iterated to convergence (the C4 batch of bench.py --mode columns: perturbed FAL-C columns, H + Ca II
at lineScale 3.1, ~3 000 wavelengths, 5 rays, profiles made on the device), from the same start each time:
  (a) ColumnBatch.iterate_to_convergence(retire=True): a converged column leaves the launches at once;
  (b) the same with retire=False: everybody iterates until the slowest column has converged;
  (c) ColumnBatch.iterate(niter = largest stop iteration + 1): the route to the same end without convergence numbers.
The three are alternated --reps times after one warm-up of each; every timed call is bracketed by waits for the batch's stream
(host clock).  Between runs J and the populations are uploaded again from the host arrays, which nothing downloads into.
    python tools/columns_converge_time.py [--columns 512] [--reps 3] [--JTol 5e-2] [--popsTol 2e-2] [--NmaxIter 300]
--ng No,Np,Nd adds the loop with Ng acceleration against plain MALI and the cost of one reported iteration with Ng (extrapolating
/ only recording) against Ng off: ng_measurements."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lightweaver_amd import _abi as abi  # noqa: E402
from lightweaver_amd.batch import ColumnBatch  # noqa: E402
from lightweaver_amd.context import ExplodingMatrixError  # noqa: E402
from lightweaver_amd.harness import models  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--columns', type=int, default=512)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--JTol', type=float, default=5e-2)
    ap.add_argument('--popsTol', type=float, default=2e-2)
    ap.add_argument('--NmaxIter', type=int, default=300)
    ap.add_argument('--Nscatter', type=int, default=3)
    ap.add_argument('--ng', default='', help='No,Np,Nd: also measure the loop with Ng acceleration and the cost of the Ng step')
    ap.add_argument('--ng-iters', type=int, default=14, help='reported iterations timed one by one per route and repetition')
    args = ap.parse_args()
    base = models.falc82()
    probs = [models.falc_h_ca(Nrays=5, lineScale=3.1, atmos=models.perturbed(base, seed=1234 + c), computeProfiles=False)
             for c in range(args.columns)]
    kw = dict(Nscatter=args.Nscatter, NmaxIter=args.NmaxIter, JTol=args.JTol, popsTol=args.popsTol)
    with ColumnBatch(probs) as b:
        assert b._batch is not None
        sync = b.contexts[0].synchronize

        def reset():
            for c in b.contexts:
                c.upload(abi.J | abi.POPS)
            sync()

        def timed(fn):
            reset()
            t0 = time.perf_counter()
            r = fn()
            sync()
            return r, (time.perf_counter() - t0) * 1e3

        res, _ = timed(lambda: b.iterate_to_convergence(retire=True, **kw))
        stops = np.asarray(res.iterations)
        niter = int(stops.max()) + 1
        routes = {'retire': lambda: b.iterate_to_convergence(retire=True, **kw),
                  'no_retire': lambda: b.iterate_to_convergence(retire=False, **kw),
                  'fixed_niter': lambda: b.iterate(niter, nscatter=args.Nscatter)}
        for fn in routes.values():
            timed(fn)
        ms = {k: [] for k in routes}
        same = True
        for _ in range(args.reps):
            for k, fn in routes.items():
                r, t = timed(fn)
                ms[k].append(t)
                if k != 'fixed_niter':
                    same = same and list(r.iterations) == list(res.iterations)
        n = args.columns
        out = {'columns': n, 'Nlambda': probs[0].Nlambda, 'JTol': args.JTol, 'popsTol': args.popsTol, 'Nscatter': args.Nscatter,
               'converged': int(np.sum(res.converged)), 'stop_iteration': {'min': int(stops.min()), 'median': float(np.median(stops)),
                                                                           'max': int(stops.max())},
               'stop_iterations_repeat': same,
               'column_iterations': {'retire': int((stops + 1).sum()), 'no_retire': n * niter, 'fixed_niter': n * niter},
               'ms': {k: {'min': min(v), 'median': float(np.median(v)), 'max': max(v), 'runs': v} for k, v in ms.items()}}
        if args.ng:
            out['ng'] = ng_measurements(b, args, kw, timed, reset, sync, res)
        print(json.dumps(out), flush=True)


def ng_measurements(b, args, kw, timed, reset, sync, plain):
    """--ng No,Np,Nd: (1) the loop to convergence with Ng against plain MALI, alternated --reps times: stop iterations, the
    columns that do not converge within NmaxIter under Ng (counted, not hidden), wall time; (2) the cost of the Ng step: one
    reported iteration (formal_sol_gamma_matrices without a wait + stat_equil(report=True)) timed --ng-iters times from the same
    start with Ng and without, alternated, the Ng iterations split into those that extrapolate and those that only record."""
    ng = tuple(int(x) for x in args.ng.split(','))
    assert len(ng) == 3
    n = args.columns

    def loop(on):
        b.configure_ng(0, 0, 0)
        try:
            return timed(lambda: b.iterate_to_convergence(retire=True, ng=ng if on else None, **kw))
        except ExplodingMatrixError as e:   # (a column's Ng system or solve went singular: the loop has no answer for the batch)
            print(json.dumps({'ng_loop_failed': str(e)}), flush=True)
            raise

    def per_iteration(on):
        reset()
        b.configure_ng(*(ng if on else (0, 0, 0)))
        rows = []
        for it in range(args.Nscatter):     # (as the loop: no solve while it < Nscatter)
            b.formal_sol_gamma_matrices(sync_host=False)
        for it in range(args.ng_iters):
            sync()
            t0 = time.perf_counter()
            b.formal_sol_gamma_matrices(sync_host=False)
            ups = b.stat_equil(report=True)
            rows.append(((time.perf_counter() - t0) * 1e3, any(u.ngAccelerated for u in ups)))
        return rows

    loop(True)
    per_iteration(True)
    ms = {'plain': [], 'ng': []}
    it_ms = {'off': [], 'records': [], 'extrapolates': []}
    last = None
    for _ in range(args.reps):
        for on in (False, True):
            r, t = loop(on)
            ms['ng' if on else 'plain'].append(t)
            if on:
                last = r
            rows = per_iteration(on)[2:]     # (the first two calls of a route still size buffers)
            for t1, acc in rows:
                it_ms['off' if not on else 'extrapolates' if acc else 'records'].append(t1)
    b.configure_ng(0, 0, 0)
    conv = np.asarray(last.converged)
    stops = np.asarray(last.iterations)[conv]
    stat = lambda v: {'min': min(v), 'median': float(np.median(v)), 'max': max(v), 'n': len(v)} if v else None  # noqa: E731
    return {'options': list(ng), 'converged': int(conv.sum()), 'not_converged_within_NmaxIter': int(n - conv.sum()),
            'stop_iteration': {'min': int(stops.min()), 'median': float(np.median(stops)), 'max': int(stops.max())} if stops.size else None,
            'plain_stop_iteration': {'min': int(min(plain.iterations)), 'max': int(max(plain.iterations))},
            'column_iterations': int((np.asarray(last.iterations) + 1).sum()),
            'loop_ms': {k: stat(v) for k, v in ms.items()}, 'reported_iteration_ms': {k: stat(v) for k, v in it_ms.items()}}


if __name__ == '__main__':
    main()
