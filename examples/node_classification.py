#!/usr/bin/env python3
"""Node classification with a trained TIGER encoder on one MI355X: the recipe of the reference's
train_supervised.py (load the link-prediction checkpoint -> embed each batch's source nodes under no_grad ->
train the MLP decoder on the event labels -> validate / early stop -> test AUC), written against this package's
mirror of the reference API.  The checkpoint is one written by examples/link_prediction.py with the same
encoder settings.

    python examples/node_classification.py --data wikipedia --root /path/with/data --ckpt model.pt ...

Only `run()` matters; the few flags exist to make the file runnable.
"""
import argparse
import copy
import os
import sys

import numpy as np
import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from www2023tiger_amd.data.data_loader import BatchLoader, GraphCollator, load_jodie_data_for_node_task  # noqa: E402
from www2023tiger_amd.data.graph import Graph  # noqa: E402
from www2023tiger_amd.eval_utils import eval_node_classification  # noqa: E402
from www2023tiger_amd.init_utils import init_model  # noqa: E402
from www2023tiger_amd.model.basic_modules import MLP  # noqa: E402
from www2023tiger_amd.optim import Adam  # noqa: E402


def train_epoch(encoder, decoder, train_dl, loss_fn, optimizer, device):
    """train_supervised.py:132-155"""
    losses = []
    encoder.reset()
    decoder.train()
    for src, dst, neg, ts, eids, labels, cg in train_dl:
        bs = len(src)
        src, dst, neg, eids = (x.long().to(device) for x in (src, dst, neg, eids))
        ts, labels = ts.float().to(device), labels.float().to(device)
        with torch.no_grad():
            _, h, *_ = encoder.contrast_learning(src, dst, neg, ts, eids, cg)
        optimizer.zero_grad()
        loss = loss_fn(decoder(h[:bs]), labels)  # only the source nodes
        loss.backward()
        optimizer.step()
        losses.append(loss.detach())
    return float(torch.stack(losses).mean()) if losses else float('nan')


def run(data, root, ckpt_path, *, seed=0, n_epochs=10, bs=100, lr=3e-4, dropout=0.1, use_valid=False, patience=5,
        dim=None, n_neighbors=10, n_heads=2, hit_type='bin', restarter_type='seq', hist_len=40, msg_src='left',
        upd_src='right', strategy='recent_edges', device='cuda:0'):
    """-> (dict(epochs=[{epoch, loss, val_auc}], test_auc), encoder, decoder).  The encoder settings must be those the
    checkpoint was trained with (examples/link_prediction.py defaults here)."""
    device = torch.device(device)
    torch.manual_seed(seed)
    np.random.seed(seed)
    nfeats, efeats, full_data, train_data, val_data, test_data = load_jodie_data_for_node_task(
        data, train_seed=seed, root=root, use_validation=use_valid)
    max_id = int(max(full_data.src.max(), full_data.dst.max()))  # both graphs over the full id space (init_utils)
    train_graph = Graph.from_data(train_data, strategy=strategy, seed=seed, max_node_id=max_id, device=device)
    full_graph = Graph.from_data(full_data, strategy=strategy, seed=seed, max_node_id=max_id, device=device)
    coll = lambda g: GraphCollator(g, n_neighbors, 1, restarter=restarter_type, hist_len=hist_len)
    train_dl = BatchLoader(train_data, bs, coll(train_graph))
    val_dl, test_dl = BatchLoader(val_data, bs, coll(full_graph)), BatchLoader(test_data, bs, coll(full_graph))
    encoder = init_model(nfeats, efeats, train_graph, full_graph, full_data, device, dim=dim, n_layers=1,
                         n_heads=n_heads, n_neighbors=n_neighbors, hit_type=hit_type, dropout=dropout,
                         restarter_type=restarter_type, hist_len=hist_len, msg_src=msg_src, upd_src=upd_src,
                         msg_tsfm_type='id', mem_update_type='gru')
    encoder.load_state_dict(torch.load(ckpt_path, map_location=device))
    encoder.eval()
    decoder = MLP(encoder.nfeat_dim, dropout=dropout).to(device)
    loss_fn = nn.BCEWithLogitsLoss()
    optimizer = Adam(decoder.parameters(), lr=lr)
    log, best = [], None
    for epoch in range(n_epochs):
        encoder.graph = train_graph
        loss = train_epoch(encoder, decoder, train_dl, loss_fn, optimizer, device)
        encoder.graph = full_graph
        val_auc = eval_node_classification(encoder, decoder, val_dl, device)
        log.append(dict(epoch=epoch, loss=loss, val_auc=val_auc))
        if use_valid:  # EarlyStopMonitor: stop after `patience` epochs without a better validation AUC
            if best is None or val_auc > best[0]:
                best = (val_auc, epoch, copy.deepcopy(decoder.state_dict()))
            elif epoch - best[1] >= patience:
                break
    if use_valid:
        decoder.load_state_dict(best[2])
        test_auc = eval_node_classification(encoder, decoder, test_dl, device)
    else:  # no validation split: the last epoch's evaluation was on the test events
        test_auc = log[-1]['val_auc'] if log else float('nan')
    return dict(epochs=log, test_auc=test_auc), encoder, decoder


if __name__ == '__main__':
    ap = argparse.ArgumentParser(description='Train the node-classification decoder on a TIGER checkpoint.')
    ap.add_argument('-d', '--data', default='wikipedia')
    ap.add_argument('--root', default='.')
    ap.add_argument('--ckpt', required=True, help='checkpoint written by examples/link_prediction.py')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--n_epochs', type=int, default=10)
    ap.add_argument('--bs', type=int, default=100)
    ap.add_argument('--lr', type=float, default=3e-4)
    ap.add_argument('--dropout', type=float, default=0.1)
    ap.add_argument('--patience', type=int, default=5)
    ap.add_argument('--use_valid', action='store_true')
    ap.add_argument('--restarter_type', default='seq', choices=['seq', 'static'])
    a = ap.parse_args()
    out, _, _ = run(a.data, a.root, a.ckpt, seed=a.seed, n_epochs=a.n_epochs, bs=a.bs, lr=a.lr, dropout=a.dropout,
                    use_valid=a.use_valid, patience=a.patience, restarter_type=a.restarter_type)
    print(out)
