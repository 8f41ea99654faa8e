#!/usr/bin/env python3
"""Self-supervised link prediction with TIGER on one MI355X: the recipe of the reference's
train_self_supervised.py (train with lazy restarts -> validate with memory snapshots -> checkpoint ->
test), written against this package's mirror of the reference API.

    python examples/link_prediction.py --data wikipedia --root /path/with/data/ml_wikipedia.csv ...

--neg_sample hist / ind evaluates the test splits on the historical / inductive negatives of AdversarialEdgeSampler
(Poursafaei et al., NeurIPS 2022) instead of random ones; training and validation keep random negatives.

--rank C (off by default) adds the one-vs-many protocol after testing: every test event's destination is ranked against C
candidate destinations drawn by the sampler --neg_sample selects (rnd: RandEdgeSampler, hist / ind:
AdversarialEdgeSampler), seed RANK_SEED; MRR and Hits@1/3/10 are printed for the transductive and the inductive split.

Only `run()` matters; the few flags exist to make the file runnable.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from www2023tiger_amd.data.adversarial import AdversarialEdgeSampler  # noqa: E402
from www2023tiger_amd.data.data_loader import BatchLoader, InteractionData  # noqa: E402
from www2023tiger_amd.eval_utils import eval_edge_prediction, eval_edge_ranking, warmup  # noqa: E402
from www2023tiger_amd.init_utils import init_data, init_model  # noqa: E402
from www2023tiger_amd.optim import Adam  # noqa: E402  (torch.optim.Adam works too; this one never stalls the loop)


def train_epoch(model, train_dl, optimizer, device, *, restart_prob, mutual_coef, rng):
    """train_self_supervised.py:143-171"""
    model.train()
    model.reset()
    losses, restarting, uptodate = [], False, set()
    for i_batch, (src, dst, neg, ts, eids, _, cg) in enumerate(train_dl):
        src, dst, neg, eids = (x.long().to(device) for x in (src, dst, neg, eids))
        ts = ts.float().to(device)
        optimizer.zero_grad()
        if rng.rand() < restart_prob and i_batch:
            restarting, uptodate = True, set()
            model.msg_store.clear()
        if restarting:  # lazy restart of the nodes this batch touches
            todo = set(cg.np_computation_graph_nodes.tolist()) - uptodate
            nids = torch.tensor(sorted(todo), dtype=torch.long, device=device)
            model.restart(nids, torch.full((len(nids),), ts.min().item(), device=device))
            uptodate |= todo
        c_loss, m_loss = model.contrast_and_mutual_learning(src, dst, neg, ts, eids, cg,
                                                            contrast_only=(restart_prob == 0))
        loss = c_loss + mutual_coef * m_loss
        loss.backward()
        optimizer.step()
        losses.append((loss.item(), c_loss.item(), float(m_loss.detach())))
    return np.array(losses)


def evaluate_pair(model, dl, ind_dl, device, restart_mode, uptodate):
    """Transductive then inductive evaluation from the same memory state (train_self_supervised.py:191-202);
    the memories end at the state after the transductive pass."""
    start = model.save_memory_state()
    ap, auc = eval_edge_prediction(model, dl, device, restart_mode, uptodate_nodes=set(uptodate))
    end = model.save_memory_state()
    model.load_memory_state(start)
    ind_ap, ind_auc = eval_edge_prediction(model, ind_dl, device, restart_mode, uptodate_nodes=set(uptodate))
    model.load_memory_state(end)
    return ap, auc, ind_ap, ind_auc


def adversarial_test_loaders(neg_sample, full_data, full_graph, test_dl, ind_test_dl, seed):
    """The test split's negatives drawn by AdversarialEdgeSampler (chunks of 200 events over the full stream's
    T-CSR); the inductive split, a subset of the test events, keeps the negatives of its events."""
    test, ind = test_dl.dataset, ind_test_dl.dataset
    adv = AdversarialEdgeSampler(full_data.src, full_data.dst, full_data.ts, test.src, test.ts, neg_sample, seed=seed,
                                 graph=full_graph)
    neg = adv.pre_sample_neg_dsts(len(test))
    mk = lambda d, ng: BatchLoader(InteractionData(d.src, d.dst, d.ts, d.eids, d.labels, d.seed, eval=True, neg_dst=ng),
                                   test_dl.batch_size, test_dl.collate_fn)
    return mk(test, neg), mk(ind, neg[np.isin(test.eids, ind.eids)])


RANK_SEED = 2023  # --rank: the seed of the candidate draws (column j is drawn with RANK_SEED + j)


def rank_candidates(neg_sample, n_cand, full_data, full_graph, test):
    """[len(test), n_cand] candidate destinations of the test events: column j is one pre-sampled negative stream of
    the sampler `neg_sample` selects, seeded RANK_SEED + j"""
    cols = []
    for j in range(n_cand):
        if neg_sample == 'rnd':
            cols.append(InteractionData(test.src, test.dst, test.ts, test.eids, test.labels, seed=RANK_SEED + j, eval=True).neg_dst)
        else:
            adv = AdversarialEdgeSampler(full_data.src, full_data.dst, full_data.ts, test.src, test.ts, neg_sample,
                                         seed=RANK_SEED + j, graph=full_graph)
            cols.append(adv.pre_sample_neg_dsts(len(test)))
    return np.stack(cols, 1).astype(np.int64)


def rank_pair(model, dl, ind_dl, device, cand, restart_mode, uptodate):
    """eval_edge_ranking over the transductive then the inductive test split from the same memory state and the same
    up-to-date set (as evaluate_pair); the inductive events keep the candidates of their events.  In restart mode the
    candidates' neighbourhoods are restarted lazily with the batch's own (lazy_restarts): the protocol of the AP / AUC"""
    start = model.save_memory_state()
    out = eval_edge_ranking(model, dl, device, cand, lazy_restarts=restart_mode, uptodate_nodes=set(uptodate))
    end = model.save_memory_state()
    model.load_memory_state(start)
    ind = eval_edge_ranking(model, ind_dl, device, cand[np.isin(dl.dataset.eids, ind_dl.dataset.eids)],
                            lazy_restarts=restart_mode, uptodate_nodes=set(uptodate))
    model.load_memory_state(end)
    return out, ind


def run(data, root, *, seed=0, n_epochs=1, bs=200, lr=1e-4, dim=None, n_neighbors=10, n_heads=2, hit_type='bin',
        restarter_type='seq', hist_len=40, msg_src='left', upd_src='right', restart_prob=0.01, mutual_coef=1.0,
        warmup_steps=0, strategy='recent_edges', dropout=0.1, ckpt_path=None, neg_sample='rnd', rank=0, device='cuda:0'):
    device = torch.device(device)
    torch.manual_seed(seed)
    rng = np.random.RandomState(seed)
    basic, (train_graph, full_graph), dls = init_data(
        data, root, seed, num_workers=0, bs=bs, warmup_steps=warmup_steps, subset=1.0, strategy=strategy, n_layers=1,
        n_neighbors=n_neighbors, restarter_type=restarter_type, hist_len=hist_len, device=device)
    nfeats, efeats, full_data = basic[:3]
    train_dl, _, val_dl, ind_val_dl, test_dl, ind_test_dl, val_warm_dl, test_warm_dl = dls
    if neg_sample != 'rnd':
        test_dl, ind_test_dl = adversarial_test_loaders(neg_sample, full_data, full_graph, test_dl, ind_test_dl, seed)
    model = init_model(nfeats, efeats, train_graph, full_graph, full_data, device, dim=dim, n_layers=1,
                       n_heads=n_heads, n_neighbors=n_neighbors, hit_type=hit_type, dropout=dropout,
                       restarter_type=restarter_type, hist_len=hist_len, msg_src=msg_src, upd_src=upd_src,
                       msg_tsfm_type='id', mem_update_type='gru')
    optimizer = Adam(model.parameters(), lr=lr)
    restart_mode = restart_prob > 0
    log = []
    for epoch in range(n_epochs):
        model.graph = train_graph
        losses = train_epoch(model, train_dl, optimizer, device, restart_prob=restart_prob, mutual_coef=mutual_coef,
                             rng=rng)
        model.eval()
        model.flush_msg()
        model.graph = full_graph
        uptodate = set()
        if restart_mode:
            model.msg_store.clear()
            if warmup_steps:
                uptodate = warmup(model, val_warm_dl, device)
        val = evaluate_pair(model, val_dl, ind_val_dl, device, restart_mode, uptodate)
        model.flush_msg()
        if ckpt_path:
            torch.save(model.state_dict(), ckpt_path)
        log.append(dict(epoch=epoch, loss=float(losses[:, 0].mean()), contrast=float(losses[:, 1].mean()),
                        mutual=float(losses[:, 2].mean()), val_ap=val[0], val_auc=val[1], ind_val_ap=val[2],
                        ind_val_auc=val[3]))
    if ckpt_path:  # the reference reloads its best checkpoint before testing
        model.load_state_dict(torch.load(ckpt_path, map_location=device))
    model.eval()
    model.graph = full_graph
    uptodate = set()
    if restart_mode:
        model.msg_store.clear()
        if warmup_steps:
            uptodate = warmup(model, test_warm_dl, device)
    before_test = model.save_memory_state() if rank > 0 else None
    test = evaluate_pair(model, test_dl, ind_test_dl, device, restart_mode, uptodate)
    out = dict(epochs=log, test_ap=test[0], test_auc=test[1], ind_test_ap=test[2], ind_test_auc=test[3])
    if rank > 0:  # one-vs-many over the same test events, from the state and the up-to-date set the test started from: in
        #             restart mode with lazy restarts that cover the candidates too, so both sets of numbers share a protocol
        after_test = model.save_memory_state()
        model.load_memory_state(before_test)
        cand = rank_candidates(neg_sample, rank, full_data, full_graph, test_dl.dataset)
        r, ind_r = rank_pair(model, test_dl, ind_test_dl, device, cand, restart_mode, uptodate)
        model.load_memory_state(after_test)
        for name, m in (('test', r), ('ind_test', ind_r)):
            out.update({f'{name}_mrr': m['mrr'], **{f'{name}_hits@{k}': v for k, v in m['hits'].items()}})
            print(f"{name}: MRR {m['mrr']:.4f}  " + '  '.join(f'Hits@{k} {v:.4f}' for k, v in m['hits'].items())
                  + f"  ({m['n_events']} events, {rank} {neg_sample} candidates)")
    return out, model


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('-d', '--data', default='wikipedia')
    ap.add_argument('--root', default='.')
    ap.add_argument('--n_epochs', type=int, default=1)
    ap.add_argument('--bs', type=int, default=200)
    ap.add_argument('--lr', type=float, default=1e-4)
    ap.add_argument('--restarter_type', default='seq', choices=['seq', 'static'])
    ap.add_argument('--restart_prob', type=float, default=0.01)
    ap.add_argument('--dropout', type=float, default=0.1)
    ap.add_argument('--neg_sample', default='rnd', choices=['rnd', 'hist', 'ind'])
    ap.add_argument('--rank', type=int, default=0, metavar='C',
                    help='after testing: MRR / Hits@1/3/10 against C candidates per test event (0: off)')
    a = ap.parse_args()
    out, _ = run(a.data, a.root, n_epochs=a.n_epochs, bs=a.bs, lr=a.lr, restarter_type=a.restarter_type,
                 restart_prob=a.restart_prob, dropout=a.dropout, neg_sample=a.neg_sample, rank=a.rank)
    print(out)
