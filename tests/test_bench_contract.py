"""bench.py's output contract (what the round driver parses): ONE JSON line on rank 0 with the headline metric; with --full
also the roofline block of the dominant kernel measured live with HIP events, the CPU baseline and the parity check at the
timed size.  Runs bench.py as a child process on the GPU box (short: 5 timed steps, 2 s of CPU baseline, no aux entry)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_line_contract(gpu):
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--full', '--steps', '5', '--warmup', '2',
                          '--cpu-seconds', '2', '--no-aux'], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for key in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling',
                'vs_baseline', 'dtype', 'data', 'config', 'roofline', 'cpu_baseline', 'parity_checked', 'max_rel_err'):
        assert key in d, key
    assert d['n_gpus'] == 1 and d['steps'] == 5 and d['warmup'] == 2 and d['higher_is_better'] is True
    assert d['dtype'] == 'f64' and d['scaling'] == 'strong' and d['vs_baseline'] is None
    assert 'workload' in d['config'] and abs(d['config']['Nlambda_per_gpu'] - 10240) <= 102
    assert d['config']['sweep'] in ('march', 'lanes')
    assert d['value'] == pytest.approx(1e3 / d['ms_per_step'], rel=1e-9)
    r = d['roofline']
    assert r['bound'] == 'hbm' and r['unit'] == 'GB/s' and r['peak'] == 8000.0 and ('raymarch_kernel' in r['kernel'] or 'lanesweep_kernel' in r['kernel'])
    assert r['launches_timed'] >= 1 and 0.0 < r['kernel_ms'] < d['ms_per_step']
    assert r['achieved'] == pytest.approx(r['algorithmic_bytes_per_launch'] / (r['kernel_ms'] * 1e-3) / 1e9, rel=1e-9)
    assert r['frac'] == pytest.approx(r['achieved'] / r['peak'], rel=1e-12)
    c = d['cpu_baseline']
    assert c['kind'] in ('reference', 'port') and c['cores'] >= 1 and c['value'] > 0 and c['unit'] == 'iters/s'
    assert d['parity_checked'] is True and d['max_rel_err'] <= 1e-8
    # the in-run parity check is the one place where the REFERENCE ITSELF (oracle/_ref: the real core, scalar scheme) runs at the
    # timed size inside the GPU suite (the other timed-size tests compare with the C oracle, which is pinned to it bit for bit
    # on the small fixtures): one call 1e-9 element-wise, populations after stat_equil 1e-8
    par = d['parity']
    if c['kind'] == 'reference':
        assert 'scalar' in par['against']
    for k in ('J', 'I', 'Gamma', 'Rij', 'Rji'):
        assert par['rel_err'][k] <= 1e-9, (k, par['rel_err'][k])
    assert par['rel_err']['n'] <= 1e-8


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_outputs(gpu, tmp_path):
    """A plain run times the headline and nothing else; --dump-outputs writes what the last timed step computed, the same on
    every run with the same arguments (to rounding, where the default mode sums with atomics)."""
    import numpy as np
    from helpers import rel_err
    dumps = []
    for run in range(2):
        d_out = tmp_path / f'run{run}'
        out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '7', '--warmup', '2',
                              '--dump-outputs', str(d_out)], capture_output=True, text=True, timeout=900, cwd=ROOT)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [ln for ln in out.stdout.splitlines() if ln.startswith('{')]
        assert len(lines) == 1
        d = json.loads(lines[0])
        assert d['metric'] == 'formal_sol_gamma_matrices iters/sec' and d['unit'] == 'iters/s' and d['higher_is_better'] is True
        assert d['dtype'] == 'f64' and d['steps'] == 7 and d['warmup'] == 2 and d['n_gpus'] == 1
        assert d['value'] == pytest.approx(1e3 / d['ms_per_step'], rel=1e-9) and d['ms_per_step'] > 0.0
        for key in ('roofline', 'cpu_baseline', 'parity_checked', 'aux'):
            assert key not in d, key
        files = sorted(p.name for p in d_out.iterdir())
        assert {'J.npy', 'I.npy', 'Gamma0.npy', 'Gamma1.npy', 'dJMax.npy'} <= set(files), files
        assert any(f.startswith('Rij') for f in files) and any(f.startswith('Rji') for f in files)
        assert sum((d_out / f).stat().st_size for f in files) <= 64 * 10**6
        arrays = {f: np.load(d_out / f) for f in files}
        assert all(a.dtype == np.float64 and np.isfinite(a).all() for a in arrays.values())
        nla = d['config']['Nlambda_total']
        assert arrays['J.npy'].shape == (nla, 82) and arrays['I.npy'].shape == (nla, 5)
        assert arrays['J.npy'].max() > 0.0 and arrays['dJMax.npy'][0] == d['config']['final_dJMax']
        dumps.append(arrays)
    # J, I and dJMax are bit-identical from run to run; Gamma and the rates are summed with atomics in the default mode (the
    # fixed-order mode is the bit-reproducible one), so they agree to rounding
    for f, a in dumps[0].items():
        if f in ('J.npy', 'I.npy', 'dJMax.npy'):
            assert np.array_equal(a, dumps[1][f]), f
        else:
            assert rel_err(dumps[1][f], a) <= 1e-13, (f, rel_err(dumps[1][f], a))


def test_dump_outputs_samples_past_the_limit(tmp_path):
    """Past the size limit every output keeps a fixed, seeded sample of its elements, in proportion to its size."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    arrays = {'J': np.arange(5000.0).reshape(100, 50), 'n': np.arange(10, dtype=np.float32)}
    bench.dump_outputs(str(tmp_path / 'whole'), arrays)
    assert np.array_equal(np.load(tmp_path / 'whole' / 'J.npy'), arrays['J'])
    assert np.load(tmp_path / 'whole' / 'n.npy').dtype == np.float64
    for run in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / run), arrays, limit=4000)
    J = np.load(tmp_path / 'a' / 'J.npy')
    n = np.load(tmp_path / 'a' / 'n.npy')
    assert J.nbytes + n.nbytes <= 4000 and J.size > 100 * n.size
    assert np.all(np.diff(J) > 0) and np.isin(J, arrays['J']).all()
    assert np.array_equal(J, np.load(tmp_path / 'b' / 'J.npy')) and np.array_equal(n, np.load(tmp_path / 'b' / 'n.npy'))


def test_rank_launch_command_shape():
    """`python bench.py --gpus N` without a launcher starts its ranks itself: the command it spawns."""
    sys.path.insert(0, ROOT)
    import bench
    cmd = bench.rank_launch_command(4, ['--gpus', '4', '--steps', '7'], port=29511)
    assert cmd[1:3] == ['-m', 'torch.distributed.run']
    assert '--nproc-per-node=4' in cmd and '--nnodes=1' in cmd
    assert cmd[cmd.index('--master-addr') + 1] == '127.0.0.1' and cmd[cmd.index('--master-port') + 1] == '29511'
    assert cmd[-5].endswith('bench.py') and cmd[-4:] == ['--gpus', '4', '--steps', '7']


def test_self_launch_spawns_ranks_without_a_gpu():
    """No launcher, no GPU: the parent spawns two ranks (it must not touch the GPU itself), each rank refuses to run
    without a device, and the parent passes the failure on as its own exit code."""
    import torch
    if torch.cuda.is_available():
        pytest.skip('a GPU box: covered by test_bench_self_launch_two_ranks_on_one_gpu')
    env = dict(os.environ)
    env.pop('WORLD_SIZE', None)
    env.pop('RANK', None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--backend', 'gloo', '--share-gpu',
                          '--steps', '1', '--warmup', '0'], capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert out.returncode != 0
    # (the launcher ends the other rank as soon as one has failed: on a loaded machine only the first may get to say so)
    assert out.stderr.count('bench.py needs a GPU') >= 1, out.stderr[-2000:]


@pytest.mark.gpu
def test_bench_self_launch_two_ranks_on_one_gpu(gpu):
    """`python3 bench.py --gpus 2` with no launcher and no WORLD_SIZE: the form the driver's SCALE command may take.  Two
    ranks share the box's one GPU under gloo (functional: the sharded path, one collective per step, rank 0's line)."""
    env = dict(os.environ)
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--backend', 'gloo', '--share-gpu',
                          '--steps', '5', '--warmup', '2', '--no-weak'], capture_output=True, text=True, timeout=900, cwd=ROOT,
                         env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d['n_gpus'] == 2 and d['steps'] == 5 and d['scaling'] == 'strong'
    assert d['value'] == pytest.approx(1e3 / d['ms_per_step'], rel=1e-9)
    assert abs(d['config']['Nlambda_total'] - 10240) <= 102 and d['config']['Nlambda_per_gpu'] < 6000
    assert 'allreduce_us' in d


def test_column_sets_of_the_ranks_partition_the_seeded_set():
    """--mode columns: column c of BASELINE configs[3] is FAL-C perturbed with seed 1234 + c whatever the number of ranks; the
    ranks' round-robin shares are disjoint, cover the set, and a rank's problems are the ones a single rank builds for the
    same column numbers (no rank-dependent input)."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    from lightweaver_amd.harness import models
    whole_idx, whole = bench.column_problems(models, 6, 1, 0, lineScale=0.2)
    assert whole_idx == list(range(6))
    seen = []
    for r in range(3):
        idx, probs = bench.column_problems(models, 6, 3, r, lineScale=0.2)
        assert idx == [r, r + 3]
        for c, p in zip(idx, probs):
            assert np.array_equal(p.temperature, whole[c].temperature) and np.array_equal(p.vlosMu, whole[c].vlosMu)
            assert np.array_equal(p.atoms[1].n, whole[c].atoms[1].n)
        seen += idx
    assert sorted(seen) == list(range(6))
    assert not np.array_equal(whole[0].temperature, whole[1].temperature)


@pytest.mark.gpu
def test_bench_columns_mode_two_ranks_on_one_gpu(gpu):
    """`python3 bench.py --gpus 2 --mode columns` (BASELINE configs[3]'s split, two ranks sharing the box's one GPU under gloo):
    every rank runs ITS columns as a fused batch, no collective in the data path; rank 0's line counts the column-iterations
    of both ranks against the slower rank's clock."""
    env = dict(os.environ)
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--backend', 'gloo', '--share-gpu',
                          '--mode', 'columns', '--columns', '6', '--steps', '4', '--warmup', '1'], capture_output=True, text=True,
                         timeout=900, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d['n_gpus'] == 2 and d['steps'] == 4 and d['scaling'] == 'weak' and d['unit'] == 'column-iters/s'
    assert d['config']['columns_total'] == 12 and d['config']['columns_per_gpu'] == 6 and d['config']['fused'] is True
    assert d['value'] == pytest.approx(12 * 1e3 / d['ms_per_step'], rel=1e-9)
    assert len(d['per_rank_ms_per_step']) == 2 and all(0.0 < x <= d['ms_per_step'] * 1.0001 for x in d['per_rank_ms_per_step'])
    r = d['roofline']
    assert r['bound'] == 'hbm' and r['frac'] == pytest.approx(r['achieved'] / 8000.0, rel=1e-12) and 0.0 < r['frac'] < 1.0
    assert d['config']['final_dJMax_max'] > 0.0   # (the largest relative change of J over the columns: of order 10 after five iterations from LTE)
