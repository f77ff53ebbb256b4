"""Time the emergent spectrum of a 2D context two ways, on the 256 x 82 problem of bench.py's C5_2d (perturbed FAL-C columns,
H(6), x-periodic):

  new    Context.compute_rays_2d from the device-resident state: the vertical view (1, 0) and a three-direction call, each
         first (its intersection table is built on the host and uploaded) and repeated (the table is cached);
  route  what the same numbers cost without it: a second Context on model.observer_problem_2d, its uploads,
         compute_profiles, formal_sol(upOnly=True), the download of I -- set-up included, it is part of that route.

The clock is the host clock between stream waits; medians over --reps.  Prints one JSON line.

    python tools/rays2d_time.py [--nx 256] [--reps 7]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lightweaver_amd import _abi as abi  # noqa: E402
from lightweaver_amd.context import Context  # noqa: E402
from lightweaver_amd.harness import models  # noqa: E402
from lightweaver_amd.model import observer_problem_2d  # noqa: E402

THREE = (np.array([1.0, 0.6, 0.6]), np.array([0.0, 0.8, -0.5]))


def timed_ms(fn, sync):
    sync()
    t0 = time.perf_counter()
    out = fn()
    sync()
    return (time.perf_counter() - t0) * 1e3, out


def median_ms(fn, sync, reps):
    ts = [timed_ms(fn, sync)[0] for _ in range(reps)]
    return {'min': min(ts), 'median': float(np.median(ts))}


def route(prob, muz, mux, vz, vx):
    """The parent's route: second context on the observer problem, profiles, up-only formal solution, I."""
    q = observer_problem_2d(prob, muz, mux, vz, vx)
    with Context(q) as ctx:
        ctx.compute_profiles(deviceResident=True)
        ctx.formal_sol(upOnly=True, deviceResident=True)
        ctx.download(abi.I)
    return q.I


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nx', type=int, default=256)
    ap.add_argument('--reps', type=int, default=7)
    args = ap.parse_args()
    base = models.falc82()
    cols = [models.perturbed(base, seed=1234 + j) for j in range(args.nx)]
    prob = models.build_problem_2d(cols, np.linspace(0.0, 25.0e3 * (args.nx - 1), args.nx), [models.H_6(0.5)])
    rng = np.random.default_rng(3)
    vz, vx = 3.0e3 * rng.standard_normal(prob.Nspace), 4.0e3 * rng.standard_normal(prob.Nspace)
    one = (np.array([1.0]), np.array([0.0]))
    out = {'Nx': prob.grid2d.Nx, 'Nz': prob.grid2d.Nz, 'Nlambda': prob.Nlambda}
    with Context(prob) as ctx:
        ctx.formal_sol_gamma_matrices(deviceResident=True)              # (a resident state, warm device)
        sync = ctx.synchronize
        first1, got1 = timed_ms(lambda: ctx.compute_rays_2d(*one, vz, vx), sync)
        rep1 = median_ms(lambda: ctx.compute_rays_2d(*one, vz, vx), sync, args.reps)
        first3, got3 = timed_ms(lambda: ctx.compute_rays_2d(*THREE, vz, vx), sync)
        rep3 = median_ms(lambda: ctx.compute_rays_2d(*THREE, vz, vx), sync, args.reps)
        ctx.download(abi.J)                                              # (the route starts from the same J)
    out['new'] = {'vertical_first_ms': first1, 'vertical_repeated_ms': rep1, 'three_first_ms': first3, 'three_repeated_ms': rep3}
    ref1 = route(prob, *one, vz, vx)                                     # (warm-up)
    r1 = median_ms(lambda: route(prob, *one, vz, vx), lambda: None, max(args.reps // 2, 2))
    ref3 = route(prob, *THREE, vz, vx)
    r3 = median_ms(lambda: route(prob, *THREE, vz, vx), lambda: None, max(args.reps // 2, 2))
    out['route'] = {'vertical_ms': r1, 'three_ms': r3}
    out['max_rel_diff_new_vs_route'] = {'vertical': float(np.max(np.abs(got1 / ref1 - 1.0))),
                                         'three': float(np.max(np.abs(got3 / ref3 - 1.0)))}
    out['ratio_route_over_new'] = {'vertical_repeated': r1['median'] / rep1['median'], 'vertical_first': r1['median'] / first1,
                                   'three_repeated': r3['median'] / rep3['median'], 'three_first': r3['median'] / first3}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
