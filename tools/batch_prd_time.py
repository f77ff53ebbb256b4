"""Time the PRD sub-iterations of a 1.5D column batch: the C4 batch of bench.py --mode columns (perturbed FAL-C columns, H + Ca II
at lineScale 3.1, ~3 000 wavelengths, 5 rays, profiles made on the device) with Ca II H & K in PRD, after four formal solutions.
  default        ColumnBatch.prd_redistribute(3, 0.0): one set of launches per sub-iteration for the whole batch
  --per-column   each column's own Context.prd_redistribute(3, 0.0, deviceResident=True), one after the other on the batch's
                 contexts: the only route before there was a batched call (this mode runs on such a checkout too)
Every timed call is bracketed by waits for the batch's stream (host clock); two warm-up calls (the first fills the columns' gII
caches), then the median of --reps (5).  With tol = 0 every call runs --sub-iters sub-iterations of every column, whatever the
state the call before it left.  Prints one JSON line: ms per call, microseconds per column and sub-iteration, the runs.
    python tools/batch_prd_time.py [--columns 512] [--sub-iters 3] [--reps 5] [--per-column]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lightweaver_amd.batch import ColumnBatch  # noqa: E402
from lightweaver_amd.harness import models  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--columns', type=int, default=512)
    ap.add_argument('--sub-iters', type=int, default=3)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--per-column', action='store_true')
    args = ap.parse_args()
    n, m = args.columns, args.sub_iters
    base = models.falc82()
    probs = [models.falc_h_ca(Nrays=5, lineScale=3.1, prd=True, atmos=models.perturbed(base, seed=1234 + c), computeProfiles=False)
             for c in range(n)]
    with ColumnBatch(probs) as b:
        assert b._batch is not None and b.contexts[0].Nprd == 2
        sync = b.contexts[0].synchronize
        for _ in range(4):
            b.formal_sol_gamma_matrices(sync_host=False)
        if args.per_column:
            def call():
                return [c.prd_redistribute(m, 0.0, deviceResident=True) for c in b.contexts]
        else:
            def call():
                return b.prd_redistribute(m, 0.0)

        def timed():
            sync()
            t0 = time.perf_counter()
            ups = call()
            sync()
            assert all(u.NprdSubIter == m for u in ups)
            return (time.perf_counter() - t0) * 1e3

        warm = [timed(), timed()]
        runs = [timed() for _ in range(args.reps)]
        med = float(np.median(runs))
        print(json.dumps({'route': 'per_column' if args.per_column else 'batched', 'columns': n, 'sub_iters': m,
                          'Nlambda': probs[0].Nlambda, 'Nspace': probs[0].Nspace, 'sweep': b.contexts[0].sweep_kind(),
                          'ms_per_call': med, 'us_per_column_and_sub_iteration': med * 1e3 / (n * m),
                          'runs_ms': runs, 'spread': (max(runs) - min(runs)) / med, 'warmup_ms': warm}), flush=True)


if __name__ == '__main__':
    main()
