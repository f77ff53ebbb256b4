"""Time the emergent Stokes vector at mu = 1 two ways, for a fused batch of polarised C4 columns (harness.zeeman.stokes_columns:
perturbed FAL-C, H + Ca II with the Ca II lines polarised, 2 908 wavelengths x 82 depths) and for one context at the timed
size (throughput_grid: 10 240 wavelengths):

  new    ColumnBatch.compute_rays(stokes=True) / Context.compute_rays(stokes=True) from the device-resident state (the
         observer gather forms the profiles in place; one copy up, one copy back);
  route  what the same numbers cost without it: per column a second Context on model.observer_problem(stokes=True), its
         uploads, compute_profiles, compute_polarised_profiles, single_stokes_fs(upOnly=True), the download -- set-up
         included, it is part of that route.

Each call is bracketed by waits for the stream (host clock); one warm-up, medians over --reps (at least 5).  The two routes are
compared at the sizes timed: the largest difference of I (relative) and of Quv / I.  Kernel times come from a run of its own
under the profiler's kernel trace (tools/README.md).

    python tools/stokes_rays_time.py [--columns 512] [--route-columns 32] [--reps 5] [--skip-grid] [--skip-route]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lightweaver_amd.batch import ColumnBatch  # noqa: E402
from lightweaver_amd.context import Context  # noqa: E402
from lightweaver_amd.harness import models, zeeman  # noqa: E402
from lightweaver_amd.model import StokesData, observer_problem  # noqa: E402


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
    """The parent's route for one column: [4, Nla, 1]."""
    q = observer_problem(prob, 1.0, stokes=True)
    with Context(q) as ctx:
        ctx.compute_profiles(deviceResident=True)
        ctx.compute_polarised_profiles(deviceResident=True)
        ctx.single_stokes_fs(updateJ=False, upOnly=True)
    return np.concatenate([q.I[None], q.Quv])


def diff(got, ref):
    return {'I': float(np.max(np.abs(got[0] / ref[0] - 1.0))), 'Quv_over_I': float(np.max(np.abs(got[1:] - ref[1:]) / ref[0][None]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--columns', type=int, default=512)
    ap.add_argument('--route-columns', type=int, default=32, help='columns the per-column route is timed on (scaled to --columns)')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--skip-grid', action='store_true')
    ap.add_argument('--skip-route', action='store_true')
    args = ap.parse_args()
    reps = max(args.reps, 5)
    out = {}
    probs = zeeman.stokes_columns(args.columns)
    with ColumnBatch(probs) as b:
        sync = b.contexts[0].synchronize
        got = b.compute_rays(1.0, stokes=True)                      # (attaches the Stokes data, staging, warm-up)
        t = median_ms(lambda: b.compute_rays(1.0, stokes=True), sync, reps)
        t3 = median_ms(lambda: b.compute_rays([1.0, 0.6, 0.2], stokes=True), sync, reps)
    out['columns'] = {'columns': args.columns, 'Nlambda': probs[0].Nlambda, 'Nspace': probs[0].Nspace,
                      'compute_rays_stokes_mu1_ms': t, 'compute_rays_stokes_3mu_ms': t3}
    if not args.skip_route:
        nr = min(args.route_columns, args.columns)
        route(probs[0])                                             # (warm-up)
        t0 = time.perf_counter()
        ref = [route(p) for p in probs[:nr]]
        routeMs = (time.perf_counter() - t0) * 1e3
        worst = [diff(got[i], ref[i]) for i in range(nr)]
        out['columns'].update({'route_ms_per_column': routeMs / nr, 'route_ms_scaled_to_batch': routeMs / nr * args.columns,
                               'route_columns_timed': nr, 'ratio_route_over_new': routeMs / nr * args.columns / t['median'],
                               'max_diff_new_vs_route': {k: max(w[k] for w in worst) for k in worst[0]}})
    if not args.skip_grid:
        prob = models.throughput_grid()
        z = np.linspace(0.0, 1.0, prob.Nspace)
        prob.set_stokes(StokesData(B=0.1 * (0.5 + z), gammaB=0.3 + 0.9 * z, chiB=0.2 + 1.1 * z,
                                   mux=np.sqrt(1.0 - prob.muz ** 2), muy=np.zeros(prob.Nrays),
                                   lines=zeeman.polarise_lines(prob, 1)))
        with Context(prob) as ctx:
            got = ctx.compute_rays(1.0, squeeze=False, stokes=True)
            t = median_ms(lambda: ctx.compute_rays(1.0, stokes=True), ctx.synchronize, reps)
        out['grid'] = {'Nlambda': prob.Nlambda, 'Nspace': prob.Nspace, 'compute_rays_stokes_mu1_ms': t}
        if not args.skip_route:
            ref = route(prob)
            tr = median_ms(lambda: route(prob), lambda: None, reps)
            out['grid'].update({'route_ms': tr, 'ratio_route_over_new': tr['median'] / t['median'],
                                'max_diff_new_vs_route': diff(got, ref)})
    print(json.dumps(out))


if __name__ == '__main__':
    main()
