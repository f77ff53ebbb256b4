"""Time the emergent spectrum at mu = 1 two ways, for a fused batch of C4 columns (bench.py --mode columns: perturbed FAL-C,
H + Ca II, ~2 900 wavelengths) and for one context at the timed size (throughput_grid: 10 240 wavelengths):

  new    ColumnBatch.compute_rays / Context.compute_rays from the device-resident state (one launch, one copy back);
  route  what the same numbers cost without it: per column a second Context on model.observer_problem (one ray), its
         uploads, compute_profiles, formal_sol(upOnly=True), the download of I -- set-up included, it is part of that route.

Each call is bracketed by waits for the stream; medians over --reps.  Also printed: the Voigt evaluations of a call (one per
active line, depth point and ray) and the bytes it reads once, for the bounds in DESIGN.md.

    python tools/rays_time.py [--columns 512] [--route-columns 32] [--reps 5] [--skip-grid]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lightweaver_amd import _abi as abi  # noqa: E402
from lightweaver_amd.batch import ColumnBatch  # noqa: E402
from lightweaver_amd.context import Context  # noqa: E402
from lightweaver_amd.harness import models  # noqa: E402
from lightweaver_amd.model import observer_problem  # noqa: E402


def work(prob, Nmu=1):
    """(Voigt evaluations, bytes read once) of one compute_rays call on `prob`."""
    Ns = prob.Nspace
    voigt = sum(t.Nlambda for a in prob.atoms for t in a.trans if t.type == abi.LINE) * Ns * Nmu
    rows = 4 * prob.Nlambda * Ns                                   # bgChi, bgEta, bgSca, J
    rows += sum(a.Nlevel for a in prob.atoms) * Ns                 # n
    rows += sum(1 for a in prob.atoms for t in a.trans) * Ns       # aDamp / ratio
    return voigt, 8 * rows


def median_ms(fn, sync, reps):
    ts = []
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {'min': min(ts), 'median': float(np.median(ts))}


def route(prob):
    """The parent route for one column: second context on the observer problem, profiles, up-only formal solution, I."""
    q = observer_problem(prob, 1.0)
    with Context(q) as ctx:
        ctx.compute_profiles(deviceResident=True)
        ctx.formal_sol(upOnly=True, deviceResident=True)
        ctx.download(abi.I)
    return q.I


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--columns', type=int, default=512)
    ap.add_argument('--route-columns', type=int, default=32, help='columns the per-column route is timed on (scaled to --columns)')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--skip-grid', action='store_true')
    args = ap.parse_args()
    out = {}
    base = models.falc82()
    probs = [models.falc_h_ca(Nrays=5, lineScale=3.1, atmos=models.perturbed(base, seed=1234 + c), computeProfiles=False)
             for c in range(args.columns)]
    voigt, byts = work(probs[0])
    with ColumnBatch(probs) as b:
        sync = b.contexts[0].synchronize
        got = b.compute_rays(1.0)                                   # (tables, staging, warm-up)
        t = median_ms(lambda: b.compute_rays(1.0), sync, args.reps)
        t3 = median_ms(lambda: b.compute_rays([1.0, 0.6, 0.2]), sync, args.reps)
    nr = min(args.route_columns, args.columns)
    route(probs[0])                                                 # (warm-up)
    t0 = time.perf_counter()
    ref = [route(p) for p in probs[:nr]]
    routeMs = (time.perf_counter() - t0) * 1e3
    worst = max(float(np.max(np.abs(got[i] / ref[i] - 1.0))) for i in range(nr))
    out['columns'] = {'columns': args.columns, 'Nlambda': probs[0].Nlambda, 'Nspace': probs[0].Nspace,
                      'compute_rays_mu1_ms': t, 'compute_rays_3mu_ms': t3,
                      'route_ms_per_column': routeMs / nr, 'route_ms_scaled_to_batch': routeMs / nr * args.columns,
                      'route_columns_timed': nr, 'max_rel_diff_new_vs_route': worst,
                      'voigt_evals_per_call': voigt * args.columns, 'bytes_read_once': byts * args.columns}
    if not args.skip_grid:
        prob = models.throughput_grid()
        voigt, byts = work(prob)
        with Context(prob) as ctx:
            got = ctx.compute_rays(1.0)
            t = median_ms(lambda: ctx.compute_rays(1.0), ctx.synchronize, args.reps)
        route(prob)
        tr = median_ms(lambda: route(prob), lambda: None, max(args.reps // 2, 2))
        out['grid'] = {'Nlambda': prob.Nlambda, 'Nspace': prob.Nspace, 'compute_rays_mu1_ms': t, 'route_ms': tr,
                       'max_rel_diff_new_vs_route': float(np.max(np.abs(got / route(prob)[:, 0] - 1.0))),
                       'voigt_evals_per_call': voigt, 'bytes_read_once': byts}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
