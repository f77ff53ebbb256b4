"""Record what the Ng step computes on LONE contexts (lwhip_ng_configure / lwhip_ng_accelerate) for the synthetic sequences of
tests/ng_cases.py, into tests/golden/ng_step_bits.json: per (problem, Nspace, options, column) the sha256 of the inputs x0, and
per step the sha256 of the bytes of all n arrays after the step, dPops as float.hex(), dPopsMaxIdx and the accelerated flag.
tests/test_batch_ng.py holds lone contexts and column batches to these bits.
    python tools/record_ng_bits.py --commit <the commit whose library ran> [--out tests/golden/ng_step_bits.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import ng_cases as ng  # noqa: E402
from lightweaver_amd import _abi as abi  # noqa: E402
from lightweaver_amd.context import Context  # noqa: E402


def record(problem, Nspace, opts, probs, ctxs):
    syn = ng.sequence_inputs(probs, opts)
    nAtoms = len(probs[0].atoms)
    out = []
    for i, (p, c) in enumerate(zip(probs, ctxs)):
        ng.put(c, p, syn.x0[i])
        c.configure_ng(*opts)
        xs, steps = [x.copy() for x in syn.x0[i]], []
        for stepNo in range(1, ng.NSTEPS + 1):
            ng.put(c, p, syn.advance(i, xs))
            st, acc, dP, dI = ng.lone_ng(c, nAtoms)
            assert st == abi.OK, (problem, Nspace, opts, i, stepNo, st)
            xs = ng.get(c, p)
            steps.append(ng.step_record(xs, acc, dP, dI))
        out.append(dict(x0=ng.digest(syn.x0[i]), steps=steps))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--commit', required=True, help='the commit the library in use was built from')
    ap.add_argument('--out', default=ng.GOLDEN)
    args = ap.parse_args()
    seqs, made = {}, {}
    for problem, Nspace, opts in ng.SEQUENCES:
        if (problem, Nspace) not in made:
            probs = [ng.column(s, Nspace, problem) for s in ng.SEEDS[:ng.NCOLUMNS]]
            made[problem, Nspace] = (probs, [Context(p) for p in probs])
        seqs[ng.key(problem, Nspace, opts)] = record(problem, Nspace, opts, *made[problem, Nspace])
    for _, ctxs in made.values():
        for c in ctxs:
            c.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:      # (one line per sequence)
        f.write('{"recorded_at": %s,\n "route": "lone contexts: lwhip_ng_configure / lwhip_ng_accelerate",\n "sequences": {\n'
                % json.dumps(args.commit))
        f.write(',\n'.join('  %s: %s' % (json.dumps(k), json.dumps(v, separators=(',', ':'))) for k, v in seqs.items()))
        f.write('\n }}\n')
    print('recorded', len(seqs), 'sequences at', args.commit, '->', args.out, os.path.getsize(args.out), 'bytes')


if __name__ == '__main__':
    main()
