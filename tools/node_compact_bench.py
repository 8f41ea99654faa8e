#!/usr/bin/env python3
"""Node-id compaction measurements (one JSON line; the method of tools/idmap_bench.py).

Per (ids N, share of the ids dropped), at C2's widths (d = d_n = 172, mailbox 4 d), one MI355X, warm-up, every call between
its own pair of device events (median, 10th / 90th percentile):

    plan          hip_ops.node_compact_plan over a graph of E events among the kept ids: remap, old_of, indptr, nbr and the
                  ONE read-back;
    plan_torch    the same work with torch ops on the same tensors: a cumsum over the keep mask for remap (the mask is
                  handed over unpacked), nonzero for old_of, indptr[old_of], remap[nbr], and the same read-back (n_new);
    child         Graph.compacted(plan): host work only, no launch;
    rows          hip_ops.node_rows_compact: the EIGHT tables of both memories and the mailbox in ONE launch, into
                  preallocated stores;
    rows_torch    torch.index_select(table, 0, old_of, out=) per table, into preallocated outputs;
    idmap         IdMap.compact() on a map of N ids with the same free ids: plan without a graph, key_of gathered, the table
                  rebuilt at the smaller capacity;
    compact_keys  (N <= --model_max only) the whole TIGE.compact_keys on a model of N nodes behind such a map, rebuilt for
                  every repetition.

rows also reports effective bytes per second (bytes read + written) against the HBM figure bench.py's roofline uses.  Every
result of the library is compared with the torch composition (torch.equal on the bits).  If the device has too little free
memory for the tables at N the row count of the TABLES is cut and recorded (`table_rows`).

    python tools/node_compact_bench.py [--ids 10000,10000000] [--drop 0.1,0.5,0.9] [--reps 20] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from idmap_bench import keys_of_range, pct, timed  # noqa: E402
from bench import HBM_PEAK_GBS  # noqa: E402
from www2023tiger_amd import hip_ops  # noqa: E402
from www2023tiger_amd.data.graph import Graph  # noqa: E402
from www2023tiger_amd.data.idmap import IdMap  # noqa: E402

D = 172
WIDTHS = (('left_vals', (D,), torch.float32), ('left_ts', (), torch.float32), ('left_active', (), torch.bool),
          ('right_vals', (D,), torch.float32), ('right_ts', (), torch.float32), ('right_active', (), torch.bool),
          ('msg_vals', (4 * D,), torch.float32), ('msg_ts', (), torch.float32))


def row_bytes(shape, dt):
    return int(np.prod(shape, dtype=np.int64)) * torch.empty(0, dtype=dt).element_size()


def summary(xs):
    return round(statistics.median(xs), 2), [round(pct(xs, 0.1), 2), round(pct(xs, 0.9), 2)]


def small_model(n_nodes, ev, dev):
    """a TIGER model with the sequence restarter on n_nodes ids (as the tests build theirs), d = 172"""
    from www2023tiger_amd.model.feature_getter import NumericalFeature
    from www2023tiger_amd.model.restarters import SeqRestarter
    from www2023tiger_amd.model.tiger import TIGER
    g = Graph.from_arrays(*ev, strategy='recent_edges', seed=0, max_node_id=n_nodes - 1, device=dev)
    torch.manual_seed(0)
    fg = NumericalFeature(torch.zeros(n_nodes, D), torch.zeros(len(ev[0]) + 1, D), dim=D, device=dev)
    rst = SeqRestarter(raw_feat_getter=fg, graph=g, hist_len=7, n_head=2, dropout=0.0)
    m = TIGER(raw_feat_getter=fg, graph=g, restarter=rst, n_neighbors=10, hit_type='bin', n_layers=1, n_head=2, dropout=0.0,
              msg_src='left', upd_src='left').to(dev)
    return m.eval()


def measure(N, share, reps, dev, model_max):
    rs = np.random.RandomState(0)
    drop = np.sort(rs.choice(np.arange(1, N), size=int(share * (N - 1)), replace=False))
    keep = np.ones(N, dtype=bool)
    keep[drop] = False
    alive = np.nonzero(keep)[0][1:]
    E = min(2_000_000, 20 * len(alive))
    ev = (alive[rs.randint(0, len(alive), E)], alive[rs.randint(0, len(alive), E)], np.arange(E, dtype=np.float64),
          np.arange(1, E + 1, dtype=np.int64))
    g = Graph.from_arrays(*ev, strategy='recent_edges', seed=0, max_node_id=N - 1, device=dev)
    indptr, _, nbr, _ = g._tensors()
    bits = hip_ops.new_bitmap(N, dev)
    hip_ops.bitmap_mark(torch.from_numpy(drop).to(dev), bits, N)
    keep_d = torch.from_numpy(keep).to(dev)
    # the tables: as many rows as fit twice (source and destination) beside the torch outputs
    per_id = sum(row_bytes(s, dt) for _, s, dt in WIDTHS)
    free = torch.cuda.mem_get_info(dev)[0]
    rows = int(min(N, free * 0.28 // per_id))
    n_out = int(keep[:rows].sum())
    src = [torch.empty((rows,) + s, dtype=dt, device=dev) for _, s, dt in WIDTHS]
    for x in src:
        if x.dtype == torch.bool:
            x.copy_(torch.rand(x.shape, device=dev) < 0.5)
        else:
            x.uniform_()
    dst = [torch.zeros((n_out,) + s, dtype=dt, device=dev) for _, s, dt in WIDTHS]
    out = [torch.empty((n_out,) + s, dtype=dt, device=dev) for _, s, dt in WIDTHS]
    moved = n_out * per_id * 2 + 4 * n_out
    t = {k: [] for k in ('plan', 'plan_torch', 'child', 'rows', 'rows_torch', 'idmap')}

    def plan_torch():
        c = torch.cumsum(keep_d, 0, dtype=torch.int32)
        remap = torch.where(keep_d, c - 1, torch.full_like(c, -1))
        old_of = torch.nonzero(keep_d).reshape(-1).to(torch.int32)
        n_new = int(c[-1])   # the read-back
        ind = torch.cat([indptr[old_of.long()], indptr[-1:]])
        return remap, old_of, n_new, ind, remap[nbr.long()]

    keys = keys_of_range(1, N)
    keys_t, gone_d = torch.from_numpy(keys), torch.from_numpy(keys[drop - 1]).to(dev)
    if N > 1_000_000:
        reps = min(reps, 10)         # (a repetition builds a map of N keys: seconds)
    for rep in range(-2, reps):      # (negative: warm-up, not recorded)
        us = {}
        us['plan'], plan = timed(lambda: hip_ops.node_compact_plan(g, bits, N))
        us['plan_torch'], ref = timed(plan_torch)
        us['child'], child = timed(lambda: g.compacted(plan))
        assert torch.equal(plan.remap, ref[0]) and torch.equal(plan.old_of, ref[1]) and plan.n_new == ref[2]
        assert torch.equal(plan.indptr, ref[3]) and torch.equal(plan.nbr, ref[4]) and child.num_node == plan.n_new
        old_of = plan.old_of[:n_out]
        us['rows'], _ = timed(lambda: hip_ops.node_rows_compact(list(zip(src, dst)), old_of))
        idx = old_of.long()
        us['rows_torch'], _ = timed(lambda: [torch.index_select(s, 0, idx, out=o) for s, o in zip(src, out)])
        if rep <= 0:
            assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(dst, out))
        m = IdMap.from_keys(keys_t, dev)
        m.remove(gone_d)
        cap = m.capacity
        torch.cuda.synchronize()
        us['idmap'], p2 = timed(lambda: m.compact())
        assert m.size == plan.n_new and m.n_free == 0 and torch.equal(p2.old_of, plan.old_of)
        if rep >= 0:
            for k, v in us.items():
                t[k].append(v)
        caps = (cap, m.capacity)
        del m, plan, ref, child, p2
    row = dict(ids=N, share_dropped=share, n_new=int(keep.sum()), events=E, table_rows=rows, table_rows_out=n_out,
               bytes_per_id=per_id, reps=reps, idmap_capacity_before_after=caps, results_checked=True)
    for k, v in t.items():
        row[f'{k}_us'], row[f'{k}_us_p10_p90'] = summary(v)
    row['rows_GBps'] = round(moved / row['rows_us'] / 1e3, 1)
    row['rows_torch_GBps'] = round(moved / row['rows_torch_us'] / 1e3, 1)
    row['rows_share_of_hbm_peak'] = round(row['rows_GBps'] / HBM_PEAK_GBS, 3)
    row['rows_over_torch'] = round(row['rows_us'] / row['rows_torch_us'], 2)
    row['plan_over_torch'] = round(row['plan_us'] / row['plan_torch_us'], 2)
    del src, dst, out
    torch.cuda.empty_cache()
    if N <= model_max:
        whole = []
        for rep in range(-1, min(reps, 5)):
            model = small_model(N, ev, dev)
            m = IdMap.from_keys(keys_t, dev)
            model.erase_keys(m, gone_d)
            torch.cuda.synchronize()
            us, p = timed(lambda: model.compact_keys(m))
            assert model.n_nodes == m.size == int(keep.sum()) and p.n_new == model.n_nodes
            if rep >= 0:
                whole.append(us)
            del model, m
        row['compact_keys_us'], row['compact_keys_us_p10_p90'] = summary(whole)
        row['compact_keys_reps'] = len(whole)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ids', default='10000,10000000')
    ap.add_argument('--drop', default='0.1,0.5,0.9')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--model_max', type=int, default=100000, help='the whole compact_keys is timed on models up to this many nodes')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    dev = torch.device('cuda', 0)
    rows = []
    for N in (int(x) for x in a.ids.split(',') if x):
        for share in (float(x) for x in a.drop.split(',') if x):
            rows.append(measure(N, share, a.reps, dev, a.model_max))
            print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    out = dict(tool='node_compact_bench', device=torch.cuda.get_device_name(0), hbm_peak_GBps=HBM_PEAK_GBS, results=rows)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
