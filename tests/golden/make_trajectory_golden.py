#!/usr/bin/env python3
"""Writes tests/golden/trajectory_<cfg>.npz: the tables of the reference's encode_trajectory (tiger/eval_utils.py)
on two small streams, for tests/test_trajectory_host.py and tests/test_hip_trajectory.py.

    python tests/golden/make_trajectory_golden.py --reference /path/to/www2023tiger

Needs the reference checkout (yzhang1918/www2023tiger @ v1.0.1); the tests read only the .npz.  Each file holds the
stream, features and weight recipe as eval_*.npz do, the per-batch h[:2B] the reference's model produced (float32,
recorded while encode_trajectory ran), and the returned tables for agg in {last, max, mean, sum} with both flags on
and for `mean` with use_src=False and with use_dst=False.

The streams are make_golden.py's bipartite ones with some events turned user -> user (no self-loops), so that nodes
occur as sources and as destinations.  The script checks that within one batch a node is source and destination, that
a node recurs as a source, and that a seen node has a negative embedding entry (so that `max` clips at the zero start).
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

SCENARIOS = {
    'trajectory_seq_lr_d8': dict(d=8, n_u=40, n_i=15, E=900, T=450.0, B=50, K=5, H=8, seed=61, wseed=61, restarter='seq',
                                 msg_src='left', upd_src='right', hit='bin'),
    'trajectory_static_ll_d16': dict(d=16, n_u=60, n_i=25, E=900, T=500.0, B=64, K=10, seed=62, wseed=62,
                                     restarter='static', msg_src='left', upd_src='left', hit='vec'),
}
CASES = [('last', True, True), ('max', True, True), ('mean', True, True), ('sum', True, True), ('mean', False, True),
         ('mean', True, False)]


def case_key(agg, use_src, use_dst):
    return f'table_{agg}_src{int(use_src)}_dst{int(use_dst)}'


def make_stream(G, cfg):
    src, dst, ts, eids = G.make_stream(cfg['seed'], cfg['n_u'], cfg['n_i'], cfg['E'], cfg['T'])
    rs = np.random.RandomState(cfg['seed'] + 7)
    u2u = rs.uniform(size=len(src)) < 0.12
    dst[u2u] = rs.randint(1, cfg['n_u'] + 1, u2u.sum())
    loop = dst == src  # no self-loops: move the destination to the next user
    dst[loop] = dst[loop] % cfg['n_u'] + 1
    assert not (dst == src).any()
    return src, dst, ts, eids


def gen(G, name, cfg):
    import torch
    from torch.utils.data import DataLoader
    from tiger.data.data_loader import GraphCollator, InteractionData
    from tiger.data.graph import Graph
    from tiger.eval_utils import encode_trajectory
    d, B = cfg['d'], cfg['B']
    src, dst, ts, eids = make_stream(G, cfg)
    E = len(src)
    n_nodes = int(max(src.max(), dst.max())) + 1
    rs = np.random.RandomState(cfg['seed'] + 100)
    nfeats = rs.standard_normal((n_nodes, d)).astype(np.float32) * 0.5
    nfeats[0] = 0
    efeats = rs.standard_normal((E + 1, d)).astype(np.float32)
    efeats[0] = 0
    data = InteractionData(src, dst, ts, eids, np.zeros(E, dtype=np.int64), seed=0, eval=True)
    graph = Graph.from_data(data, strategy='recent_edges', seed=0)
    model, pnames, pshapes = G.build_reference_model(cfg, nfeats, efeats, graph, E, dropout=0.0)
    collator = GraphCollator(graph, cfg['K'], 1, restarter=cfg['restarter'], hist_len=cfg.get('H'))
    out = {'versions': G.VERSIONS, 'src': src, 'dst': dst, 'ts': ts, 'eids': eids, 'neg': data.neg_dst,
           'n_nodes': np.int64(n_nodes), 'param_names': np.array(pnames),
           'param_shapes': np.array([','.join(map(str, s)) for s in pshapes]),
           'cfg': np.array([f'{k}={v}' for k, v in sorted(cfg.items())]), 'nfeats': nfeats, 'efeats': efeats}
    mk = lambda: DataLoader(data, batch_size=B, shuffle=False, collate_fn=collator)
    # record the h every call of contrast_learning returns while the reference's own function runs
    seen = []
    inner = model.contrast_learning

    def recording(*a, **k):
        res = inner(*a, **k)
        seen.append(res[1].detach().cpu().numpy().copy())
        return res

    model.contrast_learning = recording
    first = None
    for agg, use_src, use_dst in CASES:
        del seen[:]
        table = encode_trajectory(model, mk(), torch.device('cpu'), agg, use_src=use_src, use_dst=use_dst)
        assert table.dtype == np.float64 and table.shape == (n_nodes, d)
        out[case_key(agg, use_src, use_dst)] = table
        hs = list(seen)  # h is [2B, d]: the sources' rows, then the destinations' (tiger.py:254)
        assert sum(len(h) for h in hs) == 2 * E
        if first is None:
            first = hs
            for b, h in enumerate(hs):
                assert h.dtype == np.float32
                out[f'b{b}_h'] = h
        else:  # every pass starts from model.reset(): the same embeddings every time
            assert len(hs) == len(first) and all(np.array_equal(a, b) for a, b in zip(hs, first))
    out['n_batches'] = np.int64(len(first))
    # what the tests rely on
    both = src_twice = False
    for b in range(len(first)):
        s, t = src[b * B:(b + 1) * B], dst[b * B:(b + 1) * B]
        both |= bool(np.intersect1d(s, t).size)
        src_twice |= len(np.unique(s)) < len(s)
    assert both, 'no node is source and destination within one batch'
    assert src_twice, 'no node recurs as a source within one batch'
    assert (np.concatenate(first) < 0).any(), 'no negative embedding entry: max would not clip'
    assert (out[case_key('max', True, True)] >= 0).all() and (out[case_key('last', True, True)] < 0).any()
    np.savez_compressed(os.path.join(HERE, f'{name}.npz'), **out)
    print(f'{name}.npz', sum(v.nbytes for v in out.values()) // 1024, 'KiB raw', len(first), 'batches')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='root of the reference checkout')
    ap.add_argument('names', nargs='*', help='scenarios to write (default: all)')
    a = ap.parse_args()
    sys.dont_write_bytecode = True
    sys.path.insert(0, a.reference)
    sys.path.insert(0, HERE)
    import make_golden as G  # installs the torch_scatter stand-in and imports the reference's `tiger` package
    import tiger
    ref, got = os.path.realpath(a.reference), os.path.realpath(os.path.dirname(os.path.dirname(tiger.__file__)))
    assert ref == got, f'make_golden.py imported the reference from {got}, not from --reference {ref}'
    for name, cfg in SCENARIOS.items():
        if not a.names or name in a.names:
            gen(G, name, cfg)


if __name__ == '__main__':
    main()
