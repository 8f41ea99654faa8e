"""Trajectory encoding on the device: tg_trajectory_accumulate / tg_trajectory_finish against their host twins (bit for
bit), encode_trajectory against the reference's tables (tests/golden/trajectory_*.npz) over both kinds of loader, the
resident stream against the per-batch loop, the return value and the state left behind, and the example script."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from _util import load, parse_cfg, rel_err
from test_hip_parity import build_hip_model, dev
from test_trajectory_host import (CASES, FIXTURES, RANDOM_B, RANDOM_D, fresh, host_accumulate, host_finish, mode_of,
                                  random_case)

pytestmark = pytest.mark.gpu


def device_tables(n_nodes, d, batches, agg, use_src, use_dst, guard=0):
    """the batches through the device kernel (and finish for 'mean') -> (table, counts, err word) as numpy; with `guard`
    rows of 7.0 allocated on both sides of table and counts, returned too"""
    from www2023tiger_amd._lib import check, lib, ptr
    from www2023tiger_amd.hip_ops import stream_ptr
    tbuf = torch.full((n_nodes + 2 * guard, d), 7.0, dtype=torch.float64, device=dev())
    cbuf = torch.full((n_nodes + 2 * guard,), 7.0, dtype=torch.float64, device=dev())
    table, counts = tbuf[guard:guard + n_nodes], cbuf[guard:guard + n_nodes]
    table.zero_()
    counts.zero_()
    err = torch.zeros(1, dtype=torch.int32, device=dev())
    for h, s, t in batches:
        hd, sd, td = (torch.from_numpy(x).to(dev()) for x in (h, s, t))
        check(lib.tg_trajectory_accumulate(len(s), d, ptr(hd), ptr(sd), ptr(td), None, mode_of(agg), int(use_src),
                                           int(use_dst), n_nodes, ptr(table), ptr(counts), ptr(err), stream_ptr(dev())),
              'tg_trajectory_accumulate')
    if agg == 'mean':
        check(lib.tg_trajectory_finish(n_nodes, d, ptr(table), ptr(counts), stream_ptr(dev())), 'tg_trajectory_finish')
    return table.cpu().numpy(), counts.cpu().numpy(), int(err.item()), tbuf.cpu().numpy(), cbuf.cpu().numpy()


def host_tables(n_nodes, d, batches, agg, use_src, use_dst):
    table, counts, err = fresh(n_nodes, d)
    for h, s, t in batches:
        host_accumulate(h, s, t, mode_of(agg), use_src, use_dst, table, counts, err)
    if agg == 'mean':
        host_finish(table, counts)
    return table, counts, int(err[0])


@pytest.mark.parametrize('d', RANDOM_D)
@pytest.mark.parametrize('B', RANDOM_B)
def test_device_kernel_equals_the_host_twin_bit_for_bit(d, B):
    n_nodes, batches = random_case(d, B, seed=1000 * d + B)
    for agg, use_src, use_dst in CASES + [('last', False, True), ('max', True, False)]:
        want, want_counts, _ = host_tables(n_nodes, d, batches, agg, use_src, use_dst)
        runs = [device_tables(n_nodes, d, batches, agg, use_src, use_dst) for _ in range(2)]
        for table, counts, err, _, _ in runs:
            assert err == 0
            assert np.array_equal(counts, want_counts), (agg, use_src, use_dst)
            assert np.array_equal(table, want), (agg, use_src, use_dst)
        assert np.array_equal(runs[0][0], runs[1][0])


def test_device_kernel_reads_ids_at_the_device_side_offset():
    from www2023tiger_amd._lib import check, lib, ptr
    from www2023tiger_amd.hip_ops import stream_ptr
    d, B = 8, 50
    n_nodes, batches = random_case(d, B, seed=7)
    src = torch.from_numpy(np.concatenate([s for _, s, _ in batches])).to(dev())
    dst = torch.from_numpy(np.concatenate([t for _, _, t in batches])).to(dev())
    table = torch.zeros(n_nodes, d, dtype=torch.float64, device=dev())
    counts = torch.zeros(n_nodes, dtype=torch.float64, device=dev())
    err = torch.zeros(1, dtype=torch.int32, device=dev())
    for b, (h, _, _) in enumerate(batches):
        off = torch.tensor([b * B], dtype=torch.int64, device=dev())
        hd = torch.from_numpy(h).to(dev())
        check(lib.tg_trajectory_accumulate(B, d, ptr(hd), ptr(src), ptr(dst), ptr(off), mode_of('sum'), 1, 1, n_nodes,
                                           ptr(table), ptr(counts), ptr(err), stream_ptr(dev())), 'tg_trajectory_accumulate')
    want, want_counts, _ = host_tables(n_nodes, d, batches, 'sum', True, True)
    assert np.array_equal(table.cpu().numpy(), want) and np.array_equal(counts.cpu().numpy(), want_counts)


def test_out_of_range_ids_on_the_device():
    """the error word is set, nothing is stored for those rows (guard rows on both sides stay as they were), every other
    row is the host twin's; encode_trajectory's ValueError comes from that word"""
    from www2023tiger_amd import _lib
    d, B = 8, 200
    n_nodes, ((h, s, t),) = random_case(d, B, seed=3, n_batches=1)
    s, t = s.copy(), t.copy()
    s[[3, 77]] = [-1, n_nodes]
    t[[0, 150]] = [n_nodes + 5, -(2 ** 40)]
    for agg in ('last', 'max', 'mean'):
        want, want_counts, werr = host_tables(n_nodes, d, [(h, s, t)], agg, True, True)
        table, counts, err, tbuf, cbuf = device_tables(n_nodes, d, [(h, s, t)], agg, True, True, guard=8)
        assert err == werr == _lib.TG_TRAJ_ERR_BAD_ID
        assert np.array_equal(table, want) and np.array_equal(counts, want_counts)
        assert (tbuf[:8] == 7).all() and (tbuf[-8:] == 7).all() and (cbuf[:8] == 7).all() and (cbuf[-8:] == 7).all()
    from www2023tiger_amd.eval_utils import _Trajectory

    traj = _Trajectory(SimpleNamespace(device=dev(), n_nodes=n_nodes, nfeat_dim=d), 'mean', True, True)
    sd, td = torch.from_numpy(s).to(dev()), torch.from_numpy(t).to(dev())
    traj.add(B, torch.from_numpy(h).to(dev()), sd.data_ptr(), td.data_ptr())
    with pytest.raises(ValueError, match='outside'):
        traj.finish(True)


def _loaders(z, cfg, coll):
    from torch.utils.data import DataLoader
    from www2023tiger_amd.data.data_loader import BatchLoader, InteractionData
    E = len(z['src'])
    data = lambda: InteractionData(z['src'], z['dst'], z['ts'], z['eids'], np.zeros(E, dtype=np.int64), seed=0, eval=True)
    return {'DataLoader': lambda: DataLoader(data(), batch_size=cfg['B'], shuffle=False, collate_fn=coll),
            'BatchLoader': lambda: BatchLoader(data(), cfg['B'], coll)}


@pytest.mark.parametrize('loader', ['DataLoader', 'BatchLoader'])
@pytest.mark.parametrize('name', FIXTURES)
def test_encode_trajectory_matches_the_reference(name, loader, monkeypatch):
    """rel_err < 1e-4, the parity bar for embeddings: 'last' / 'max' select entries of h, 'mean' / 'sum' are sums of a few
    of them (divided by their count).  The DataLoader takes the per-batch loop, the BatchLoader the resident stream."""
    from www2023tiger_amd import eval_utils
    z = load(name)
    cfg = parse_cfg(z)
    model, _, coll = build_hip_model(z, cfg, dropout=0.0)
    mk = _loaders(z, cfg, coll)[loader]
    taken = []
    real = eval_utils._eval_resident
    monkeypatch.setattr(eval_utils, '_eval_resident', lambda *a, **k: (taken.append(1), real(*a, **k))[1])
    for agg, use_src, use_dst in CASES:
        got = eval_utils.encode_trajectory(model, mk(), dev(), agg, use_src=use_src, use_dst=use_dst)
        want = z[f'table_{agg}_src{int(use_src)}_dst{int(use_dst)}']
        assert got.shape == want.shape and got.dtype == np.float64
        e = rel_err(got, want)
        print(f'{name} {loader} {agg} src={use_src} dst={use_dst}: rel_err {e:.3e}')
        assert e < 1e-4, (agg, use_src, use_dst, e)
        assert np.array_equal(got.any(1), want.any(1))  # the same nodes were seen; the others stay zero
    assert len(taken) == (len(CASES) if loader == 'BatchLoader' else 0)


@pytest.mark.parametrize('agg', ['last', 'max', 'mean'])
def test_resident_pass_equals_the_per_batch_loop(agg, monkeypatch):
    """With the model's own forms (TG_EVAL_STREAM=0) the resident pass runs the loop's kernels on the loop's inputs: the
    tables are equal bit for bit.  The default streaming form (eager updates, pre-multiplied weights) agrees within 2e-4,
    the bound tests/test_hip_eval.py: test_resident_eval_equals_the_per_batch_loop holds its scores to."""
    from www2023tiger_amd import eval_utils
    z = load('trajectory_static_ll_d16')
    cfg = parse_cfg(z)
    model, _, coll = build_hip_model(z, cfg, dropout=0.0)
    mk = _loaders(z, cfg, coll)['BatchLoader']
    taken = []
    real = eval_utils._eval_resident
    monkeypatch.setattr(eval_utils, '_eval_resident', lambda *a, **k: (taken.append(1), real(*a, **k))[1])
    out = {}
    for form, env in (('loop', dict(TG_EVAL_RESIDENT='0')), ('resident', dict(TG_EVAL_RESIDENT='1', TG_EVAL_STREAM='0')),
                      ('stream', dict(TG_EVAL_RESIDENT='1', TG_EVAL_STREAM='1'))):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        out[form] = eval_utils.encode_trajectory(model, mk(), dev(), agg)
        assert model._pending is None and model._fused is None  # the switches of the streaming form are put back
    assert len(taken) == 2
    assert np.array_equal(out['loop'], out['resident'])
    e = rel_err(out['stream'], out['loop'])
    print(f'{agg}: streaming form against the loop, rel_err {e:.3e}')
    assert e < 2e-4


def test_return_value_and_state_left_behind():
    from www2023tiger_amd.eval_utils import encode_trajectory, eval_edge_prediction
    z = load('trajectory_seq_lr_d8')
    cfg = parse_cfg(z)
    model, _, coll = build_hip_model(z, cfg, dropout=0.0)
    for loader, mk in _loaders(z, cfg, coll).items():
        model.train()
        table = encode_trajectory(model, mk(), dev(), 'mean')
        assert not model.training
        assert isinstance(table, np.ndarray) and table.dtype == np.float64
        assert table.shape == (model.n_nodes, model.nfeat_dim) == (int(z['n_nodes']), cfg['d'])
        state = [t.clone() for t in (model.left_memory.vals, model.right_memory.vals, model.left_memory.update_ts,
                                     model.right_memory.update_ts, model.msg_store.node_msg_vals)]
        t = encode_trajectory(model, mk(), dev(), 'mean', as_tensor=True)  # (starts from model.reset() again)
        assert isinstance(t, torch.Tensor) and t.device.type == 'cuda' and t.dtype == torch.float64
        assert np.array_equal(t.cpu().numpy(), table)
        model.reset()
        eval_edge_prediction(model, mk(), dev(), restart_mode=False)
        for a, b in zip(state, (model.left_memory.vals, model.right_memory.vals, model.left_memory.update_ts,
                                model.right_memory.update_ts, model.msg_store.node_msg_vals)):
            assert torch.equal(a, b), loader


def test_trajectory_example_end_to_end(tmp_path):
    """examples/link_prediction.run writes a checkpoint on toy JODIE files; examples/encode_trajectory.run loads it and
    writes the table: the .npy equals the function's return"""
    from test_input_side import write_files
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, 'examples'))
    import encode_trajectory as et
    import link_prediction as lp
    z0 = load('input_side')
    z = {k: z0[k] for k in ('src', 'dst', 'ts')}
    z['labels'] = np.zeros(len(z['src']), dtype=np.int64)
    write_files(str(tmp_path), 'toy', z, with_feats=False)
    ckpt = str(tmp_path / 'model.pt')
    kw = dict(seed=0, bs=100, dim=8, n_neighbors=4, hist_len=6, restarter_type='static')
    lp.run('toy', str(tmp_path), n_epochs=1, lr=1e-3, restart_prob=0.0, ckpt_path=ckpt, **kw)
    out = str(tmp_path / 'traj.npy')
    table, encoder = et.run('toy', str(tmp_path), ckpt, agg='mean', out_path=out, **kw)
    saved = np.load(out)
    assert saved.dtype == np.float64 and saved.shape == (encoder.n_nodes, encoder.nfeat_dim)
    assert np.array_equal(saved, table)
    seen = np.zeros(encoder.n_nodes, dtype=bool)
    seen[z['src']] = seen[z['dst']] = True
    assert np.isfinite(table).all() and np.array_equal(table.any(1), seen)
    only_dst, _ = et.run('toy', str(tmp_path), ckpt, agg='last', use_src=False, **kw)
    assert not only_dst[np.setdiff1d(z['src'], z['dst'])].any() and only_dst[z['dst']].any(1).all()
