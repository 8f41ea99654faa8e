#!/usr/bin/env python3
"""Id map measurements (one JSON line).

Per (map size, batch, share of new keys): what it costs to turn one batch of external int64 keys into dense ids,

    assign    `IdMap.assign(keys)`: tg_idmap_assign (one launch for n <= 256, four above) and ONE read-back of the two
              result words (new size, error word) - lookup-or-insert, ids in the order of first appearance;
    lookup    `IdMap.lookup(keys)`: one launch, nothing read back (the call is timed to the end of its kernel);
    torch     what a caller has without the kernels: a SORTED key tensor with the ids beside it; per batch `torch.unique(keys,
              return_inverse=True)`, `torch.searchsorted` of the unique keys, ids gathered back through the inverse, and one
              read-back of the number of unknown keys (the caller needs it: it is num_node).  Unknown keys get size + their
              rank among the batch's unknown keys in SORTED order - cheaper than the order of first appearance, and not
              batch-cut invariant.  `torch_merge` adds what keeps that table usable for the next batch: the new keys are
              concatenated and the table is sorted again.

The batches are C2's (2 x 1 024 keys) and C5's (2 x 65 536); the maps hold 10^4 and 10^7 keys; known keys are drawn with
repetition from the map (a stream names its active nodes again and again), new keys are distinct.  Every repetition starts
from the same map: the table is copied back from a pristine one outside the timed region (assign inserts).  `assign`,
`lookup`, `torch` and `torch_merge` alternate for `reps` repetitions after warm-up, each call between its own pair of device
events (median, 10th / 90th percentile).  The ids of `assign` are checked against `lookup` afterwards and, for known keys,
against the torch path.

    python tools/idmap_bench.py [--maps 10000,10000000] [--batches 2048,131072] [--new 0,0.01,0.1,0.5,1] [--reps 50] [--out FILE]

--one_max N says that the library under test (TIGER_HIP_LIB) is a diagnostic build with `make EXTRA=-DTG_IDMAP_ONE_MAX=N`:
batches up to N keys take the one-launch form there.  The value is recorded with the results; that is how the limit of 256
was chosen (`profiles/idmap_one_max_v1.json`: builds with N = 2048, 256 and 0 alternating).
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from www2023tiger_amd.data.idmap import IdMap  # noqa: E402

MULT = np.uint64(0x9E3779B97F4A7C15)   # odd: distinct integers give distinct keys


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(q * len(xs)))]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3, r


def keys_of_range(lo, hi):
    return (np.arange(lo, hi, dtype=np.uint64) * MULT).astype(np.int64)


def batch_keys(map_keys, n, share_new, rep, dev):
    """n keys: a share of new ones (distinct, never seen, different in every repetition), the rest drawn from the map"""
    rs = np.random.RandomState(1000 + rep)
    n_new = int(round(share_new * n))
    fresh = keys_of_range((1 << 40) + rep * n, (1 << 40) + rep * n + n_new)
    keys = np.concatenate([fresh, map_keys[rs.randint(0, len(map_keys), size=n - n_new)]])
    return torch.from_numpy(rs.permutation(keys)).to(dev), n_new


def torch_lookup(sorted_keys, sorted_ids, size, keys):
    u, inv = torch.unique(keys, return_inverse=True)
    pos = torch.searchsorted(sorted_keys, u).clamp(max=sorted_keys.numel() - 1)
    found = sorted_keys[pos] == u
    new_rank = torch.cumsum(~found, 0) - 1
    ids_u = torch.where(found, sorted_ids[pos], (size + new_rank).int())
    n_new = int((~found).sum())   # the read-back
    return ids_u[inv], u[~found], n_new


def torch_merge(sorted_keys, sorted_ids, size, keys):
    ids, new_keys, n_new = torch_lookup(sorted_keys, sorted_ids, size, keys)
    both = torch.cat([sorted_keys, new_keys])
    order = torch.argsort(both)
    new_ids = torch.cat([sorted_ids, torch.arange(size, size + n_new, dtype=torch.int32, device=keys.device)])
    return ids, both[order], new_ids[order]


def measure(n_map, n, shares, reps, dev, one_max=256):
    map_keys = keys_of_range(1, n_map + 1)
    base = IdMap.from_keys(torch.from_numpy(map_keys), dev)
    base._grow(base.size + n)   # room for the largest batch: no growth inside the timed region
    work = IdMap(dev, capacity=base.capacity, reserve=base.key_of.numel())
    sorted_keys, order = torch.sort(base.key_of[1:base.size])
    sorted_ids = (order + 1).int()

    def reset():
        work.slot_key.copy_(base.slot_key)
        work.slot_id.copy_(base.slot_id)
        work.size = base.size
        work.slots_used = base.slots_used   # (the host's count of used slots follows the table it describes)
    work.key_of.copy_(base.key_of)
    rows = []
    for share in shares:
        t = dict(assign=[], lookup=[], torch=[], torch_merge=[])
        for rep in range(-3, reps):   # (negative: warm-up, not recorded)
            keys, n_new = batch_keys(map_keys, n, share, max(rep, 0), dev)
            reset()
            torch.cuda.synchronize()
            us = {}
            us['lookup'], before = timed(lambda: work.lookup(keys))
            us['assign'], ids = timed(lambda: work.assign(keys))
            us['torch'], ref = timed(lambda: torch_lookup(sorted_keys, sorted_ids, base.size, keys))
            us['torch_merge'], _ = timed(lambda: torch_merge(sorted_keys, sorted_ids, base.size, keys))
            assert work.size == base.size + n_new == base.size + ref[2]
            assert torch.equal(work.lookup(keys), ids) and torch.equal(ids[before > 0], before[before > 0])
            assert int((before < 0).sum()) == n_new and torch.equal(ref[0][before > 0], ids[before > 0])
            if rep >= 0:
                for k, v in us.items():
                    t[k].append(v)
        row = dict(map_keys=n_map, capacity=base.capacity, batch_keys=n, share_new=share, new_keys=n_new, reps=reps,
                   launches_assign=1 if n <= one_max else 4, results_checked=True)
        for k, v in t.items():
            row[f'{k}_call_us'] = round(statistics.median(v), 2)
            row[f'{k}_call_us_p10_p90'] = [round(pct(v, 0.1), 2), round(pct(v, 0.9), 2)]
        row['torch_over_assign'] = round(row['torch_call_us'] / row['assign_call_us'], 2)
        row['torch_merge_over_assign'] = round(row['torch_merge_call_us'] / row['assign_call_us'], 2)
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--maps', default='10000,10000000')
    ap.add_argument('--batches', default='2048,131072')
    ap.add_argument('--new', default='0,0.01,0.1,0.5,1')
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--one_max', type=int, default=256, help='TG_IDMAP_ONE_MAX of the library under test (a diagnostic build)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    dev = torch.device('cuda', 0)
    rows = []
    for n_map in (int(x) for x in a.maps.split(',') if x):
        for n in (int(x) for x in a.batches.split(',') if x):
            rows += measure(n_map, n, [float(x) for x in a.new.split(',') if x], a.reps, dev, a.one_max)
    out = dict(tool='idmap_bench', device=torch.cuda.get_device_name(0), one_max=a.one_max, results=rows)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
