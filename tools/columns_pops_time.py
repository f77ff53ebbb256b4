"""Time the population updates of a 1.5D column batch (the C4 batch of bench.py --mode columns: perturbed FAL-C columns, H + Ca II
at lineScale 3.1, ~3 000 wavelengths, 5 rays, profiles made on the device) as ONE batched call each --
  time_dep      ColumnBatch.time_dep_update(dt, prev)
  nr_static     ColumnBatch.nr_post_update(stages, bg, ne)                     (no dC)
  nr_timedep    ColumnBatch.nr_post_update(stages, bg, ne, dC=, nPrev=, dt=)
-- against the per-column route: the loop over the columns' own Context.time_dep_update / nr_post_update(deviceResident=True),
timed on --lone-columns columns (32) and scaled to the batch.  Every timed call is bracketed by waits for the batch's stream (host
clock); one warm-up, then the median of --reps (5).  Before each call the populations go up again from the host arrays, which
nothing downloads into, so every call starts from the same state.  Also reports what the batched call copies up per call.
    python tools/columns_pops_time.py [--columns 512] [--lone-columns 32] [--reps 5]"""
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
    ap.add_argument('--lone-columns', type=int, default=32)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--dt', type=float, default=1e-3)
    args = ap.parse_args()
    n, nl = args.columns, min(args.lone_columns, args.columns)
    base = models.falc82()
    atmos = [models.perturbed(base, seed=1234 + c) for c in range(n)]
    probs = [models.falc_h_ca(Nrays=5, lineScale=3.1, atmos=a, computeProfiles=False) for a in atmos]
    stages = [np.asarray(m.stage, dtype=np.float64) for m in (models.H_6(3.1), models.CaII_6(3.1))]
    rng = np.random.default_rng(7)
    prev = [[a.n.copy() for a in p.atoms] for p in probs]
    ne0 = [np.ascontiguousarray(a.ne, dtype=np.float64) for a in atmos]
    bg = [ne - sum(s @ a.n for s, a in zip(stages, p.atoms)) for ne, p in zip(ne0, probs)]      # (charge balance at the start)
    dC = [[a.C / ne[None, None, :] * (0.5 + rng.random(a.C.shape)) for a in p.atoms] for ne, p in zip(ne0, probs)]
    Ns = probs[0].Nspace
    rows = sum(a.Nlevel for a in probs[0].atoms)
    sq = sum(a.Nlevel**2 for a in probs[0].atoms)
    nbytes = {'time_dep': n * rows * Ns * 8, 'nr_static': n * (2 * Ns + rows) * 8,
              'nr_timedep': n * (2 * Ns + rows + rows * Ns + sq * Ns) * 8}
    try:
        copies = copy_alone(nbytes, args.reps)
    except RuntimeError as e:       # (torch sees no device: the copy is then not measured, the rest is)
        copies = {'copy_up_alone': 'not measured: %s' % e}
    with ColumnBatch(probs) as b:
        assert b._batch is not None
        sync = b.contexts[0].synchronize
        for _ in range(4):      # (a Gamma that a formal solution made)
            b.formal_sol_gamma_matrices(sync_host=False)
        ne = [x.copy() for x in ne0]

        def reset():
            for c, x, x0 in zip(b.contexts, ne, ne0):
                c.upload(abi.POPS)
                x[...] = x0
            sync()

        def timed(fn):
            reset()
            t0 = time.perf_counter()
            fn()
            sync()
            return (time.perf_counter() - t0) * 1e3

        def lone(update):
            def run():
                for i in range(nl):
                    update(i, b.contexts[i])
            return run

        routes = {
            'time_dep': (lambda: b.time_dep_update(args.dt, prev),
                         lone(lambda i, c: c.time_dep_update(args.dt, prev[i], deviceResident=True))),
            'nr_static': (lambda: b.nr_post_update(stages, bg, ne),
                          lone(lambda i, c: c.nr_post_update(stages, bg[i], ne[i], deviceResident=True))),
            'nr_timedep': (lambda: b.nr_post_update(stages, bg, ne, dC=dC, nPrev=prev, dt=args.dt),
                           lone(lambda i, c: c.nr_post_update(stages, bg[i], ne[i], dC=dC[i], nPrev=prev[i], dt=args.dt,
                                                              deviceResident=True))),
        }
        out = {'columns': n, 'lone_columns': nl, 'reps': args.reps, 'Nspace': Ns, 'upload_bytes_per_call': nbytes}
        for name, (batched, per_column) in routes.items():
            timed(batched)
            timed(per_column)
            tb, tl = [], []
            for _ in range(args.reps):
                tb.append(timed(batched))
                tl.append(timed(per_column))
            mb, ml = float(np.median(tb)), float(np.median(tl)) * n / nl
            out[name] = {'batched_ms': mb, 'per_column_route_ms_scaled': ml, 'ratio': ml / mb, 'batched_runs': tb,
                         'per_column_runs_%d_columns' % nl: tl}
        out['breakdown_ms'] = breakdown(b, args, prev, stages, bg, ne, dC, timed, copies)
        print(json.dumps(out), flush=True)


def copy_alone(nbytes, reps):
    """The price of not keeping the previous time step resident: a copy of as many bytes as a call sends, from page-locked
    memory to the device, on its own (torch; median of reps after one warm-up).  Run before the library opens the device."""
    import torch
    res = {}
    for name in ('time_dep', 'nr_timedep'):
        src = torch.empty(nbytes[name], dtype=torch.uint8).pin_memory()
        dst = torch.empty(nbytes[name], dtype=torch.uint8, device='cuda')
        ts = []
        for _ in range(reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dst.copy_(src, non_blocking=True)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        res[name + '_copy_up_alone'] = float(np.median(ts[1:]))
    return res


def breakdown(b, args, prev, stages, bg, ne, dC, timed, copies):
    """Where a batched call's time goes (medians of --reps): the packing in Python, the library call on packed arguments (staging
    memcpy, copy up, launches, copy back, wait), and what copy_alone measured."""
    from lightweaver_amd import batch as lb
    n, act = len(b.contexts), b.active
    lib, f64p, i32p = b.contexts[0].lib, abi.f64p, abi.i32p
    dP = np.zeros((n, len(b.problems[0].atoms)))
    dI = np.zeros(dP.shape, dtype=np.int32)
    dts = np.full(n, args.dt)
    med = lambda fn: float(np.median([fn() for _ in range(args.reps + 1)][1:]))  # noqa: E731

    def clock(fn):
        t0 = time.perf_counter()
        r = fn()
        return (time.perf_counter() - t0) * 1e3, r

    res = dict(copies)
    res['time_dep_pack'] = med(lambda: clock(lambda: lb.pack_time_dep(b.problems, act, prev))[0])
    ptrs, keep = lb.pack_time_dep(b.problems, act, prev)
    res['time_dep_call'] = med(lambda: timed(lambda: lib.lwhip_batch_time_dep_update(
        b._batch, ptrs, dts.ctypes.data_as(f64p), dP.ctypes.data_as(f64p), dI.ctypes.data_as(i32p))))
    crsw = [c.crsw for c in b.contexts]
    pack = lambda: lb.pack_nr_args(n, act, [0, 1], stages, bg, ne, dC=dC, nPrev=prev, dt=args.dt, crsw=crsw)  # noqa: E731
    res['nr_timedep_pack'] = med(lambda: clock(pack)[0])
    arr, keep2 = pack()
    res['nr_timedep_call'] = med(lambda: timed(lambda: lib.lwhip_batch_nr_post_update(
        b._batch, arr, dP.ctypes.data_as(f64p), dI.ctypes.data_as(i32p))))
    return res


if __name__ == '__main__':
    main()
