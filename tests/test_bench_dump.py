"""bench.py's --dump-outputs: the writer and the argument checks (CPU), and the dump of a real plain run (GPU)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_writes_small_outputs_whole(tmp_path):
    import bench
    h = torch.randn(30, 8)
    ts = torch.arange(12, dtype=torch.float64)
    ids = torch.arange(5, dtype=torch.int32)
    bench.dump_outputs(str(tmp_path), [('h', h), ('ts', ts), ('ids', ids)])
    got = {n: np.load(tmp_path / f'{n}.npy') for n in ('h', 'ts', 'ids')}
    assert got['h'].dtype == np.float32 and np.array_equal(got['h'], h.numpy())
    assert got['ts'].dtype == np.float64 and np.array_equal(got['ts'], ts.numpy())
    assert got['ids'].dtype == np.float32 and np.array_equal(got['ids'], ids.numpy().astype(np.float32))


def test_dump_samples_large_outputs_with_fixed_rows(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, 'DUMP_LIMIT_BYTES', 8192)
    big = torch.randn(1000, 4)
    small = torch.randn(10, 4)
    for run in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / run), [('big', big), ('small', small)])
    a, b = (np.load(tmp_path / run / 'big.npy') for run in ('a', 'b'))
    assert np.array_equal(a, b)  # the same rows in every run
    total = sum(os.path.getsize(tmp_path / 'a' / f) - 128 for f in os.listdir(tmp_path / 'a'))  # less the .npy headers
    assert total <= 8192
    rows = np.sort(np.random.RandomState(0).choice(1000, len(a), replace=False))
    assert len(a) == 4096 // 16 and np.array_equal(a, big.numpy()[rows])
    assert np.array_equal(np.load(tmp_path / 'a' / 'small.npy'), small.numpy())  # within its share: whole


def test_dump_outputs_is_refused_for_multi_gpu_runs(tmp_path):
    for extra in (['--gpus', '2'], ['--force-dist']):
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--dump-outputs', str(tmp_path)] + extra,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and 'single-GPU runs only' in r.stderr


@pytest.mark.gpu
def test_plain_run_dumps_the_streaming_steps_outputs_reproducibly(tmp_path):
    """A short plain C2 run, twice with the same arguments: the headline line, the dumped file set with its shapes and
    dtypes, and the same bytes in both runs (the streaming step is bit-reproducible)."""
    n_nodes, d, B = 8227 + 1000 + 1, 172, 1024
    want = {'h': ((3 * B, d), np.float32), 'left_memory': ((n_nodes, d), np.float32),
            'right_memory': ((n_nodes, d), np.float32), 'left_update_ts': ((n_nodes,), np.float32),
            'right_update_ts': ((n_nodes,), np.float32)}
    for run in ('a', 'b'):
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '4', '--warmup', '2',
                            '--preroll', '10', '--dump-outputs', str(tmp_path / run)],
                           capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-3000:]
        line = json.loads(r.stdout.strip().splitlines()[-1])
        assert line['steps'] == 4 and line['ms_per_step'] > 0 and line['value'] > 0
        assert 'roofline' not in line and 'cpu_baseline' not in line  # a plain run: the headline only
        assert sorted(os.listdir(tmp_path / run)) == sorted(f'{n}.npy' for n in want)
        for name, (shape, dtype) in want.items():
            x = np.load(tmp_path / run / f'{name}.npy')
            assert x.shape == shape and x.dtype == dtype, (name, x.shape, x.dtype)
            assert np.isfinite(x).all() and np.abs(x).max() > 0, name
    for name in want:
        assert (tmp_path / 'a' / f'{name}.npy').read_bytes() == (tmp_path / 'b' / f'{name}.npy').read_bytes(), name
