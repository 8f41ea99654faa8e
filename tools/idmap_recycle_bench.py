#!/usr/bin/env python3
"""Id map measurements with removal and recycling (one JSON line; the method of tools/idmap_bench.py).

Per (live keys of the map, batch, share of new keys), on a map that holds a pool of free ids LARGER than the batch:

    assign        `IdMap.assign(keys)` on a map of the same live keys with NOTHING free: the entry every map took before
                  there were free ids (tg_idmap_assign; one launch for n <= 256, four above) - what the others are judged
                  against;
    assign_free   `IdMap.assign(keys)` with free ids: tg_idmap_assign_recycle - two launches of the select over the
                  bitmap (a read of size / 8 bytes), then one launch for n <= 256 and four above - and ONE read-back;
    remove        `IdMap.remove(keys)` of the same batch (its known keys leave; the new ones are unknown and ignored):
                  tg_idmap_remove, one launch for n <= 256, two above, ONE read-back, and the sort that orders the
                  released ids.

The map with free ids is built from `live + pool` keys of which `pool` = 1.5 n + 64, spread evenly over the id range, are
removed.  Every repetition starts from the same maps: tables, key_of and bitmap are copied back from pristine ones outside
the timed region.  The calls alternate for `reps` repetitions after warm-up, each between its own pair of device events
(median, 10th / 90th percentile).  Checked per repetition: every new key of assign_free got a recycled id (ids below the
old size, the pool shrinks by the new keys), the known keys kept their ids, and remove released exactly the batch's
distinct known keys.

    python tools/idmap_recycle_bench.py [--maps 10000,10000000] [--batches 256,2048,131072] [--new 0,0.1,1] [--reps 50] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from idmap_bench import batch_keys, keys_of_range, pct, timed  # noqa: E402
from www2023tiger_amd.data.idmap import IdMap  # noqa: E402


class Pristine:
    """a map, a copy of its arrays, and the copy back"""

    def __init__(self, m):
        self.m = m
        self.saved = [t.clone() for t in (m.slot_key, m.slot_id, m.key_of, m.free_bits)]
        self.counts = (m.size, m.n_free, m.slots_used)

    def reset(self):
        m = self.m
        for t, s in zip((m.slot_key, m.slot_id, m.key_of, m.free_bits), self.saved):
            t.copy_(s)
        m.size, m.n_free, m.slots_used = self.counts


def measure(n_live, n, shares, reps, dev):
    pool = n + n // 2 + 64
    # the holed map: pool keys, spread evenly over the ids, are assigned among the live ones and removed again
    total = n_live + pool
    holes = np.unique(np.linspace(1, total, pool).astype(np.int64))
    is_hole = np.zeros(total + 1, dtype=bool)
    is_hole[holes] = True
    held = keys_of_range(1, total - len(holes) + 1)      # the keys both maps hold
    every = np.empty(total, dtype=np.int64)
    every[~is_hole[1:]] = held
    every[is_hole[1:]] = keys_of_range(1 << 50, (1 << 50) + len(holes))
    plain = IdMap.from_keys(torch.from_numpy(held), dev)
    plain._grow(plain.size + n)          # room for the largest batch: no growth inside the timed region
    holed = IdMap.from_keys(torch.from_numpy(every), dev)
    holed._grow(holed.size + 2 * n)
    _, gone = holed.remove(torch.from_numpy(every[holes - 1]).to(dev))
    assert holed.n_free == len(holes) == gone.numel() and holed.n_free > n
    P, H = Pristine(plain), Pristine(holed)
    rows = []
    for share in shares:
        t = dict(assign=[], assign_free=[], remove=[])
        for rep in range(-3, reps):      # (negative: warm-up, not recorded)
            keys, n_new = batch_keys(held, n, share, max(rep, 0), dev)
            P.reset()
            H.reset()
            torch.cuda.synchronize()
            us = {}
            before = holed.lookup(keys)
            us['assign'], _ = timed(lambda: plain.assign(keys))
            us['assign_free'], ids = timed(lambda: holed.assign(keys))
            assert plain.size == P.counts[0] + n_new and holed.size == H.counts[0] and holed.n_free == H.counts[1] - n_new
            assert torch.equal(ids[before > 0], before[before > 0]) and int((before < 0).sum()) == n_new
            assert bool((ids[before < 0] < H.counts[0]).all()) and torch.equal(holed.lookup(keys), ids)
            H.reset()
            us['remove'], (rid, released) = timed(lambda: holed.remove(keys))
            known = torch.unique(before[before > 0])
            assert torch.equal(rid, before) and torch.equal(released.long(), known.long())
            assert holed.n_free == H.counts[1] + known.numel()
            if rep >= 0:
                for k, v in us.items():
                    t[k].append(v)
        row = dict(live_keys=n_live, size=H.counts[0], free_ids=H.counts[1], capacity=holed.capacity,
                   capacity_plain=plain.capacity, bitmap_bytes=(H.counts[0] + 63) // 64 * 8, batch_keys=n, share_new=share,
                   new_keys=n_new, reps=reps, launches_assign=1 if n <= 256 else 4, launches_assign_free=3 if n <= 256 else 6,
                   launches_remove=1 if n <= 256 else 2, results_checked=True)
        for k, v in t.items():
            row[f'{k}_call_us'] = round(statistics.median(v), 2)
            row[f'{k}_call_us_p10_p90'] = [round(pct(v, 0.1), 2), round(pct(v, 0.9), 2)]
        row['assign_free_over_assign'] = round(row['assign_free_call_us'] / row['assign_call_us'], 2)
        row['remove_over_assign'] = round(row['remove_call_us'] / row['assign_call_us'], 2)
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--maps', default='10000,10000000')
    ap.add_argument('--batches', default='256,2048,131072')
    ap.add_argument('--new', default='0,0.1,1')
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    dev = torch.device('cuda', 0)
    rows = []
    for n_live in (int(x) for x in a.maps.split(',') if x):
        for n in (int(x) for x in a.batches.split(',') if x):
            rows += measure(n_live, n, [float(x) for x in a.new.split(',') if x], a.reps, dev)
    out = dict(tool='idmap_recycle_bench', device=torch.cuda.get_device_name(0), results=rows)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
