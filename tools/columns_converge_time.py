"""Time a 1.5D column batch iterated to convergence (the C4 batch of bench.py --mode columns: perturbed FAL-C columns, H + Ca II
at lineScale 3.1, ~3 000 wavelengths, 5 rays, profiles made on the device), from the same start each time:
  (a) ColumnBatch.iterate_to_convergence(retire=True): a converged column leaves the launches at once;
  (b) the same with retire=False: everybody iterates until the slowest column has converged;
  (c) ColumnBatch.iterate(niter = largest stop iteration + 1): the route to the same end without convergence numbers.
The three are alternated --reps times after one warm-up of each; every timed call is bracketed by waits for the batch's stream
(host clock).  Between runs J and the populations are uploaded again from the host arrays, which nothing downloads into.
    python tools/columns_converge_time.py [--columns 512] [--reps 3] [--JTol 5e-2] [--popsTol 2e-2] [--NmaxIter 300]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lightweaver_amd import _abi as abi  # noqa: E402
from lightweaver_amd.batch import ColumnBatch  # noqa: E402
from lightweaver_amd.harness import models  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--columns', type=int, default=512)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--JTol', type=float, default=5e-2)
    ap.add_argument('--popsTol', type=float, default=2e-2)
    ap.add_argument('--NmaxIter', type=int, default=300)
    ap.add_argument('--Nscatter', type=int, default=3)
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
        print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
