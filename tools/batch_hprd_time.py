"""Time hybrid PRD on a 1.5D column batch whose columns have their own line-of-sight velocities: columns at the C4 size of bench.py
--mode columns (perturbed FAL-C, 82 depths, H + Ca II at lineScale 3.1, ~3 000 wavelengths, 5 rays, profiles made on the device)
with Ca II H & K in hybrid PRD; column c moves with (c mod 9) * 2.5 km/s * sin(2 pi k / 37) on top of its perturbation, so every
column has tables of its own.  (On this stock grid the hybrid wavelength set hardly follows the velocities -- 631 wavelengths and 53
workgroups of the PRD pass for every column, as measured -- so the launches are not ragged here; tests/test_batch_hprd.py runs those.)
  default        ColumnBatch(problems, hprd=True): formal_sol_gamma_matrices and prd_redistribute(3, 0.0) of the fused batch, one
                 set of launches for all columns
  --per-column   each column's own Context(p, hprd=True) and its own calls, one after the other: the only route before hybrid
                 columns could be fused (this mode runs on such a checkout too)
Also timed: the set-up (every column's table build on the device, download, create and re-upload).  Every timed call is bracketed
by waits for the columns' streams (host clock); two warm-up calls of each (the first PRD call fills the gII caches), then the
median of --reps (5).  With tol = 0 every call runs --sub-iters sub-iterations of every column.
Device memory beyond a plain column's state, per column at this size: the gII caches of the two PRD lines, Nspace * 88 * Nlambda(line)
* 10 bytes each (2 x 22.6 MB), and the hybrid tables -- jCoeffs 16 bytes per (hybrid wavelength, ray, direction, depth, entry) plus
the rho coefficients, 29.2 MB measured, reported as `table_MB_per_column`: ~75 MB per column, ~9.5 GB for the default 128 columns.
Prints one JSON line.
    python tools/batch_hprd_time.py [--columns 128] [--sub-iters 3] [--reps 5] [--per-column]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lightweaver_amd.batch import ColumnBatch  # noqa: E402
from lightweaver_amd.context import Context  # noqa: E402
from lightweaver_amd.harness import models  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--columns', type=int, default=128)
    ap.add_argument('--sub-iters', type=int, default=3)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--per-column', action='store_true')
    args = ap.parse_args()
    n, m = args.columns, args.sub_iters
    base = models.falc82()
    probs = []
    for c in range(n):
        atmos = models.perturbed(base, seed=1234 + c)
        atmos.vlos = atmos.vlos + (c % 9) * 2.5e3 * np.sin(2.0 * np.pi * np.arange(atmos.Nspace) / 37.0)
        probs.append(models.falc_h_ca(Nrays=5, lineScale=3.1, prd=True, atmos=atmos, computeProfiles=False))
    t0 = time.perf_counter()
    if args.per_column:
        ctxs = [Context(p, hprd=True) for p in probs]
        for c in ctxs:
            c.compute_profiles(deviceResident=True)
        owner, shape = None, None
    else:
        owner = ColumnBatch(probs, hprd=True)
        assert owner.fused
        ctxs, shape = owner.contexts, owner.sweep_shape()
    for c in ctxs:
        c.synchronize()
    setup = (time.perf_counter() - t0) * 1e3
    try:
        assert ctxs[0].Nprd == 2 and all(c.sweep_kind() == 'lanes' for c in ctxs)
        tables = [c.hprd_tables for c in ctxs]

        def sync():
            for s in ({c for c in ctxs} if args.per_column else {ctxs[0]}):
                s.synchronize()

        if args.per_column:
            def fs():
                for c in ctxs:
                    c.formal_sol_gamma_matrices(deviceResident=True)

            def prd():
                return [c.prd_redistribute(m, 0.0, deviceResident=True) for c in ctxs]
        else:
            def fs():
                owner.formal_sol_gamma_matrices(sync_host=False)

            def prd():
                return owner.prd_redistribute(m, 0.0)

        def timed(call, check=None):
            sync()
            t = time.perf_counter()
            out = call()
            sync()
            ms = (time.perf_counter() - t) * 1e3
            if check:
                check(out)
            return ms

        def all_ran(ups):
            assert all(u.NprdSubIter == m for u in ups)

        for _ in range(2):
            fs()
        warm = [timed(prd, all_ran), timed(prd, all_ran)]
        prdRuns = [timed(prd, all_ran) for _ in range(args.reps)]
        fsRuns = [timed(fs) for _ in range(args.reps)]
        pm, fm = float(np.median(prdRuns)), float(np.median(fsRuns))
        print(json.dumps({'route': 'per_column' if args.per_column else 'fused', 'columns': n, 'sub_iters': m,
                          'Nlambda': probs[0].Nlambda, 'Nspace': probs[0].Nspace,
                          'NhPrd_min_max': [min(t.NhPrd for t in tables), max(t.NhPrd for t in tables)],
                          'table_MB_per_column': float(np.mean([t.nbytes for t in tables])) / 1e6,
                          'sweep_shape_launch': None if shape is None else shape['launch'],
                          'workgroups_prd_min_max': None if shape is None else [min(c[1] for c in shape['columns']),
                                                                                  max(c[1] for c in shape['columns'])],
                          'setup_ms': setup, 'setup_ms_per_column': setup / n,
                          'prd_ms_per_call': pm, 'prd_us_per_column_and_sub_iteration': pm * 1e3 / (n * m),
                          'fs_ms_per_call': fm, 'fs_us_per_column': fm * 1e3 / n,
                          'prd_runs_ms': prdRuns, 'fs_runs_ms': fsRuns, 'prd_warmup_ms': warm}), flush=True)
    finally:
        if owner is not None:
            owner.close()
        else:
            for c in reversed(ctxs):
                c.close()


if __name__ == '__main__':
    main()
