"""Record Context.tables_signature() of every case of tests/table_cases.py into tests/golden/table_signatures.json: per case
the environment, the device's compute-unit count (the plan depends on it) and, per context, the two words -- or the
library's refusal.  Creation only.  tests/test_table_signatures.py holds the library to these words.  Run it in two
separate processes first (--out elsewhere) and compare: a recording is only worth keeping if it reproduces.
    python tools/record_table_signatures.py --commit <the commit whose library ran> [--out tests/golden/table_signatures.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
os.environ.setdefault('LWHIP_DEBUG', '1')   # (the layout knobs of the cases are read only then)

import table_cases as tc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--commit', required=True, help='the commit the library in use was built from')
    ap.add_argument('--out', default=tc.GOLDEN)
    args = ap.parse_args()
    cu = tc.compute_units()
    cases = {}
    for case in tc.CASES:
        name, env, _ = case
        cases[name] = dict(env=env, computeUnits=cu, contexts=dict(tc.run(case)))
        print(name, cases[name]['contexts'], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:      # (one line per case)
        f.write('{"recorded_at": %s,\n "cases": {\n' % json.dumps(args.commit))
        f.write(',\n'.join('  %s: %s' % (json.dumps(k), json.dumps(v)) for k, v in cases.items()))
        f.write('\n }}\n')
    print('recorded', len(cases), 'cases at', args.commit, 'on', cu, 'compute units ->', args.out)


if __name__ == '__main__':
    main()
