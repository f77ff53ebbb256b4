"""Time polarised synthesis over a 1.5D column batch (the C4 size: H + Ca II at lineScale 3.1, ~3 000 wavelengths, 5 rays,
Ca II H, K and the infrared triplet polarised, every column with its own field; harness.zeeman.stokes_columns), up-going
rays, device-resident: the fused ColumnBatch.single_stokes_fs against the loop of Context.single_stokes_fs over the same
columns.  Each timed call is bracketed by waits for the batch's stream; the median of --reps runs after one warm-up.
    python tools/stokes_batch_time.py [--columns 512 64] [--reps 5] [--no-loop]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lightweaver_amd.batch import ColumnBatch  # noqa: E402
from lightweaver_amd.harness import zeeman  # noqa: E402


def timed(fn, sync, reps):
    fn()
    ts = []
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {'min': min(ts), 'median': float(np.median(ts))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--columns', type=int, nargs='+', default=[512, 64])
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--no-loop', action='store_true', help='time the fused call only')
    args = ap.parse_args()
    out = []
    for ncol in args.columns:
        probs = zeeman.stokes_columns(ncol, Nrays=5, lineScale=3.1)
        r = {'columns': ncol, 'Nlambda': probs[0].Nlambda, 'Nspace': probs[0].Nspace, 'Nrays': probs[0].Nrays}
        with ColumnBatch(probs) as b:
            assert b._batch is not None
            sync = b.contexts[0].synchronize
            b.compute_polarised_profiles()
            r['batch_compute_polarised_profiles_ms'] = timed(b.compute_polarised_profiles, sync, args.reps)
            r['batch_single_stokes_fs_ms'] = timed(
                lambda: b.single_stokes_fs(upOnly=True, deviceResident=True, sync_host=False), sync, args.reps)
            if not args.no_loop:
                def loop():
                    for c in b.contexts:
                        c.single_stokes_fs(upOnly=True, deviceResident=True)
                r['loop_single_stokes_fs_ms'] = timed(loop, sync, args.reps)
                r['loop_over_batch'] = r['loop_single_stokes_fs_ms']['median'] / r['batch_single_stokes_fs_ms']['median']
            r['batch_ms_per_column'] = r['batch_single_stokes_fs_ms']['median'] / ncol
        out.append(r)
        print(json.dumps(r), flush=True)


if __name__ == '__main__':
    main()
