"""Time the full-Stokes path at the timed size (throughput_grid: 10 240 wavelengths, 82 depths, 5 rays, Ca II H, K and
the infrared triplet polarised), device-resident; each call is bracketed by waits for the context's stream, so a time is
the call's whole duration on the device plus its launch overhead:  python tools/stokes_time.py [--reps N]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lightweaver_amd.context import Context  # noqa: E402
from lightweaver_amd.harness import models, zeeman  # noqa: E402
from lightweaver_amd.model import StokesData  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    args = ap.parse_args()
    prob = models.throughput_grid()
    z = np.linspace(0.0, 1.0, prob.Nspace)
    prob.set_stokes(StokesData(B=0.1 * (0.5 + z), gammaB=0.3 + 0.9 * z, chiB=0.2 + 1.1 * z,
                               mux=np.sqrt(1.0 - prob.muz ** 2), muy=np.zeros(prob.Nrays),
                               lines=zeeman.polarise_lines(prob, 1)))
    out = {'Nlambda': prob.Nlambda, 'Nspace': prob.Nspace, 'Nrays': prob.Nrays}
    with Context(prob) as ctx:
        ctx.compute_polarised_profiles()            # attaches the Stokes data, uploads it, warms up
        ctx.single_stokes_fs(upOnly=True)
        for name, fn in (('compute_polarised_profiles', lambda: ctx.compute_polarised_profiles(deviceResident=True)),
                         ('single_stokes_fs_upOnly', lambda: ctx.single_stokes_fs(upOnly=True, deviceResident=True))):
            ts = []
            for _ in range(args.reps):
                ctx.synchronize()
                t0 = time.perf_counter()
                fn()
                ctx.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            out[name + '_ms'] = {'min': min(ts), 'median': float(np.median(ts))}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
