#!/usr/bin/env python3
"""Per-node trajectory table of a trained TIGER encoder on one MI355X: load a link-prediction checkpoint, stream the
whole dataset through the model from an empty state and fold every event's source / destination embedding into one
float64 row per node (`encode_trajectory`, the reference's tiger/eval_utils.py function of that name), written as a
.npy file for clustering, plotting or a classifier of your own.  The checkpoint is one written by
examples/link_prediction.py with the same encoder settings.

    python examples/encode_trajectory.py --data wikipedia --root /path/with/data --ckpt model.pt --agg mean --out traj.npy

Only `run()` matters; the few flags exist to make the file runnable.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from www2023tiger_amd.data.data_loader import BatchLoader, GraphCollator, load_jodie_data  # noqa: E402
from www2023tiger_amd.data.graph import Graph  # noqa: E402
from www2023tiger_amd.eval_utils import encode_trajectory  # noqa: E402
from www2023tiger_amd.init_utils import init_model  # noqa: E402


def run(data, root, ckpt_path, *, agg='mean', use_src=True, use_dst=True, out_path=None, seed=0, bs=200, dim=None,
        n_neighbors=10, n_heads=2, hit_type='bin', restarter_type='seq', hist_len=40, msg_src='left', upd_src='right',
        strategy='recent_edges', device='cuda:0'):
    """-> (table [n_nodes, nfeat_dim] float64, encoder).  The encoder settings must be those the checkpoint was trained
    with (examples/link_prediction.py defaults here); the table is also saved to `out_path` when given."""
    device = torch.device(device)
    torch.manual_seed(seed)
    np.random.seed(seed)
    nfeats, efeats, full_data, train_data, *_ = load_jodie_data(data, train_seed=seed, root=root)
    max_id = int(max(full_data.src.max(), full_data.dst.max()))  # both graphs over the full id space (init_utils)
    train_graph = Graph.from_data(train_data, strategy=strategy, seed=seed, max_node_id=max_id, device=device)
    full_graph = Graph.from_data(full_data, strategy=strategy, seed=seed, max_node_id=max_id, device=device)
    full_dl = BatchLoader(full_data, bs, GraphCollator(full_graph, n_neighbors, 1, restarter=restarter_type, hist_len=hist_len))
    encoder = init_model(nfeats, efeats, train_graph, full_graph, full_data, device, dim=dim, n_layers=1,
                         n_heads=n_heads, n_neighbors=n_neighbors, hit_type=hit_type, dropout=0.0,
                         restarter_type=restarter_type, hist_len=hist_len, msg_src=msg_src, upd_src=upd_src,
                         msg_tsfm_type='id', mem_update_type='gru')
    encoder.load_state_dict(torch.load(ckpt_path, map_location=device))
    encoder.graph = full_graph
    table = encode_trajectory(encoder, full_dl, device, agg, use_src=use_src, use_dst=use_dst)
    if out_path:
        np.save(out_path, table)
    return table, encoder


if __name__ == '__main__':
    ap = argparse.ArgumentParser(description='Write the per-node trajectory table of a TIGER checkpoint.')
    ap.add_argument('-d', '--data', default='wikipedia')
    ap.add_argument('--root', default='.')
    ap.add_argument('--ckpt', required=True, help='checkpoint written by examples/link_prediction.py')
    ap.add_argument('--agg', default='mean', help="'last', 'max' or 'mean' (anything else sums, as in the reference)")
    ap.add_argument('--no_src', action='store_true', help='leave the source embeddings out')
    ap.add_argument('--no_dst', action='store_true', help='leave the destination embeddings out')
    ap.add_argument('--out', default='trajectory.npy')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--bs', type=int, default=200)
    ap.add_argument('--restarter_type', default='seq', choices=['seq', 'static'])
    a = ap.parse_args()
    table, _ = run(a.data, a.root, a.ckpt, agg=a.agg, use_src=not a.no_src, use_dst=not a.no_dst, out_path=a.out,
                   seed=a.seed, bs=a.bs, restarter_type=a.restarter_type)
    print(f'{a.out}: {table.shape[0]} nodes x {table.shape[1]}, {int((np.abs(table).sum(1) > 0).sum())} seen')
