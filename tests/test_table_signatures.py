"""The structure tables and the plan of lwhip_create, bit for bit: Context.tables_signature() of every case of
tests/table_cases.py against tests/golden/table_signatures.json (tools/record_table_signatures.py; `recorded_at` names the
commit whose build_tables wrote it).  Creation only.  The plan depends on the device's compute-unit count: on a device with
another count than the recording's the cases skip."""
import json

import pytest

import table_cases as tc


@pytest.fixture(scope='module')
def golden():
    with open(tc.GOLDEN) as f:
        return json.load(f)['cases']


def test_every_case_is_recorded(golden):
    assert sorted(golden) == sorted(name for name, _, _ in tc.CASES)
    for name, env, _ in tc.CASES:
        assert golden[name]['env'] == env, name


@pytest.mark.gpu
@pytest.mark.parametrize('case', tc.CASES, ids=[c[0] for c in tc.CASES])
def test_tables_match_the_recording(gpu, golden, case):
    want = golden[case[0]]
    cu = tc.compute_units()
    if cu != want['computeUnits']:
        pytest.skip(f'recorded on {want["computeUnits"]} compute units, this device has {cu}')
    got = dict(tc.run(case))
    print(case[0], got)
    assert got == want['contexts']
    if case[0] == 'h:borrowing':
        assert got['borrower'] == got['owner']
