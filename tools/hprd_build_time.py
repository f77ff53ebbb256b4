"""Time of the hybrid PRD table build: lwhip_hprd_build on the device against lworacle_hprd_build, the reference's
algorithm (configure_hprd_coeffs, Source/Prd.cpp:697-946) on one host thread, which is how the reference runs it.

    python tools/hprd_build_time.py [--nlambda 10240] [--reps 5] [--json OUT]

Two problems: tests/test_hprd.py's hprd_problem() and the PRD problem at the size bench.py's C3_prd uses
(throughput_grid(--nlambda, Nrays=5, prd=True)) on hprd_problem's velocity field.  Per problem: host clock around each call (the
device call ends in a stream wait), one warm-up, the median of --reps; the table sizes; and one extra device build under
LWHIP_HPRD_TIMING=1, which waits for the stream after every phase and prints where the time goes (kernels / copies).  The two
builders' tables are compared before anything is timed.  Needs a gfx950 device: there is no CPU path to time."""
import argparse
import json
import os
import re
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def moving_atmosphere(vamp=8.0e3, seed=7):
    """falc82 with the velocity field of tests/test_hprd.py::hprd_problem."""
    from lightweaver_amd.harness import models
    atmos = models.falc82()
    rng = np.random.default_rng(seed)
    k = np.arange(atmos.Nspace)
    atmos.vlos = vamp * np.sin(2.0 * np.pi * k / 37.0) + 0.2 * vamp * rng.standard_normal(atmos.Nspace)
    return atmos


def median_ms(fn, reps):
    fn()   # warm-up: code objects, the stream, the allocator
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ts), min(ts), max(ts)


def phases(build):
    """One build with LWHIP_HPRD_TIMING=1: {phase: ms} from what the library prints to stderr."""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode='w+b') as f:
        os.dup2(f.fileno(), 2)
        os.environ['LWHIP_HPRD_TIMING'] = '1'
        try:
            build()
        finally:
            del os.environ['LWHIP_HPRD_TIMING']
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        txt = f.read().decode(errors='replace')
    return {m.group(1).strip(): float(m.group(2)) for m in re.finditer(r'lwhip_hprd_build: (.+?)\s+([0-9.]+) ms', txt)}


def measure(name, prob, reps):
    from lightweaver_amd.hprd import build_hprd
    from oracle.bindings import OracleContext

    with OracleContext(prob.copy()) as oc:
        def host():
            oc.build_hprd().close()
        to = oc.build_hprd()
        td = build_hprd(prob)
        same = (np.array_equal(to.hPrdIdxs, td.hPrdIdxs) and np.array_equal(to.jCoeffOff, td.jCoeffOff)
                and np.array_equal(to.jIdx, td.jIdx) and np.array_equal(to.jFrac, td.jFrac)
                and all(np.array_equal(a, b) for ra, rb in zip(to.rho, td.rho) for a, b in zip(ra, rb)))
        sizes = {'Nlambda': int(prob.Nlambda), 'Nrays': int(prob.Nrays), 'Nspace': int(prob.Nspace),
                 'NprdLambda': td.NprdLambda, 'NhPrd': td.NhPrd, 'Nlines': td.Nlines, 'jCoeffs': int(td.jIdx.size),
                 'bytes_downloaded': td.nbytes}
        to.close()
        td.close()
        if not same:
            raise SystemExit(f'{name}: the device tables differ from the host restatement: nothing timed')
        hostMs = median_ms(host, reps)

    # (both timed calls are the C call plus the numpy views of its result; the problem's descriptor is made once, as the
    # oracle's context made its own)
    from lightweaver_amd import context
    from lightweaver_amd.hprd import build_from_descriptor
    lib, desc = context.load_library(), prob.descriptor()

    def device():
        build_from_descriptor(lib, desc, prob).close()
    devMs = median_ms(device, reps)
    ph = phases(device)
    kernels = sum(v for k, v in ph.items() if k in ('flags', 'count', 'scan', 'rho', 'fill'))
    copies = sum(v for k, v in ph.items() if k in ('upload', 'flags d2h', 'total d2h', 'tables d2h'))
    return {'problem': name, **sizes, 'tables_equal': True,
            'host_ms_median_min_max': hostMs, 'device_ms_median_min_max': devMs,
            'speedup': hostMs[0] / devMs[0], 'phases_ms': ph, 'kernels_ms': kernels, 'copies_ms': copies}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nlambda', type=int, default=10240)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    try:
        import torch   # (torch's HIP runtime first, as everywhere in this project)
        torch.cuda.is_available()
    except Exception:
        pass
    from lightweaver_amd import context
    from lightweaver_amd.harness import models
    if context.load_library().lwhip_device_count() < 1:
        raise SystemExit('no gfx950 device: nothing to time')
    atmos = moving_atmosphere()
    small = models.falc_h_ca(Nrays=3, lineScale=0.3, prd=True, atmos=atmos, computeProfiles=False)
    big = models.throughput_grid(NlambdaTarget=args.nlambda, Nrays=5, prd=True, atmos=moving_atmosphere(), computeProfiles=False)
    out = [measure('hprd_problem', small, args.reps), measure('C3_prd size', big, args.reps)]
    for r in out:
        print(json.dumps(r))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
