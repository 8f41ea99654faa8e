#!/usr/bin/env python3
"""Top-k recommendation lists of a trained TIGER model on one MI355X: load a link-prediction checkpoint (its memories are
those the validation pass left, as when examples/link_prediction.py tests), and for every event of the test split list
the k best destinations of its source among ALL destination nodes of the dataset, on the state before the event's batch
(`TIGE.recommend`: the score head over every (source, item) pair, then the device top-k `tg_topk_rows`); the batch then
streams as in evaluation.  Writes ids.npy [n_test, k] / scores.npy [n_test, k] and prints the line of
`eval_recommendation` (hit rate, NDCG and MRR of the true destination in those lists).

    python examples/recommend.py --data wikipedia --root /path/with/data --ckpt model.pt --k 10 [--exclude_seen]

--online replays the test split as a deployed model meets it: the graph is built over the train + validation events
only, and every batch first asks `recommend` at its own (source, time) queries and is then ingested with `TIGE.observe`
(the graph is extended on the device, the batch streams).  The same replay on the full graph with `stream_step` runs
beside it, and the two lines printed - hit rate / NDCG / MRR@k - must be equal exactly (`run_online` asserts it).
--window SECONDS and --keep_last M add sliding-window expiry to that replay: after every `observe` the model calls
`TIGE.forget` (entries older than the batch's last time minus the window, and entries beyond a node's last M, leave the
device graph) and the entries kept and dropped are printed per batch.  With --keep_last at least max(n_neighbors,
hist_len), no window and no --exclude_seen the forgetting replay answers exactly what the replay that never forgets
answers, so the two lines are held to the same equality; a window, a smaller cap or --exclude_seen ("seen inside the
window") answer from less history, and the two lines may differ.
--release_rows lets the edge-feature table shrink with the graph: every forget also releases the rows that no kept entry
names (`TIGE.forget(..., release_edge_rows=True, keep_from=first eid not observed yet)`), the eids of the events still
to come are shifted by the returned `shift`, and the table's rows before and after are printed per batch.  The model
computes what it would have computed, so the equality of the two lines holds under the same conditions.
--grow lets the model itself start small: its tables and its graph cover the node ids of train + validation only, and the
ids the test split brings are admitted batch by batch (`TIGE.observe(..., num_node='auto', nfeats=...)`); the ids admitted
are printed per batch.  Each batch is ranked among the items known at that moment, so there is no offline line beside it.
--erase_nodes FILE and --retract_eids FILE (each a .npy of ids) take nodes and events out of the online replay before it
starts (`TIGE.erase`: a closed account, a de-listed item, a cancelled transaction): their entries leave the device graph,
the erased nodes' memory and mailbox rows are reset, and the entries dropped are printed.  The offline replay beside it
still has them, so the two lines are not held equal; an erased id that the test split brings back starts as a node never
seen.
--save_state PATH saves the served model after the online replay (`TIGE.save_online`: parameters, memories, mailbox, the
feature tables with exactly their rows and the device graph - after a forget, a release of rows or an erase none of that
can be rebuilt from the stream), together with the position in the test split; --save_after N stops the replay after N
batches first.  --load_state PATH starts from such a file instead of train + validation (`TIGE.load_online` into the model
`init_model` builds: the graph is checked by `tg_tcsr_verify` before anything reads it) and replays the rest of the split.
A replay that is saved after N batches and one that loads the file write, between them, the lists of the uninterrupted
replay, exactly.
--journal DIR [--journal_every N] writes INCREMENTAL state files instead (`TIGE.journal().save`): a base before the first
batch, then a file after every N batches that holds only the rows that changed - a delta; a base again whenever something
rewrote everything, as --release_rows does - and index.json with each file's kind and position.  --load_state DIR/BASE.pt
--apply_deltas DIR loads that base, applies the deltas behind it (`TIGE.apply_online_delta`) and replays the rest of the
split: its lists are the journaling replay's from there on, exactly.
--keyed runs the online replay as a service meets its users: every node id of the data set is replaced by an external
64-bit key (a fixed odd-multiplier scramble of the id), the model sits behind a device id map (`IdMap.from_keys` over the ids
it was built on), every batch asks `TIGE.recommend_keys` and is ingested with `TIGE.observe_keys`, and the keys admitted are
printed per batch.  The lists are keys (ids.npy holds int64 keys); without --grow they are the scramble of the offline
replay's, exactly, and `run_online` asserts it.  With --save_state / --load_state the map's state travels in the same file.
--churn FILE (with --keyed) names, per batch, the keys that leave behind it: their nodes are erased and their keys removed
(`TIGE.erase_keys`), the released dense ids go to the keys later batches bring, and released / recycled / n_nodes are
printed per batch - the model stays as large as its peak of live keys.  --compact_at F (with --churn) goes further: when
the share of free ids passes F behind an erase, `TIGE.compact_keys` renumbers the live keys densely and shrinks the map and
every per-node table to them; rows before -> after are printed.
--late FRACTION [--late_by BATCHES] makes part of the feed arrive late: a seeded fraction of every test batch is held back
and handed to `TIGE.observe_late` that many batches later (default 1) - merged into the device graph at the place its
time gives it, never streamed into the memories.  The number of late events merged is printed, there is no offline line
beside it, and at the end the graph is asserted equal to the graph over the whole stream (`run_online`).
--event_keys [--redeliver P] names every event by an external 64-bit key (the scramble of its edge id) and feeds the replay
as an at-least-once bus would: the model tracks event keys (`TIGE.track_events` over the events of train + validation),
the edge table holds the rows of the events seen so far and nothing else, and every batch arrives through
`TIGE.observe_events` together with a seeded fraction P (default 0.25) of itself and of the previous batch a second time.
Kept / dropped are printed per batch; the lists are the plain --online replay's, exactly, and `run_online` asserts it.

--cold answers without replaying anything: the checkpoint's parameters, memories at reset, an empty up-to-date bitmap.
Every batch asks `recommend(..., uptodate=bitmap)`, which first restarts - through the model's restarter - exactly the nodes
its scores will read that the bitmap does not hold yet (`TIGER.restart_involved`), and is then ingested with
`stream_step`; the number of restarted nodes is printed per batch beside the metrics.  What a serving process that has
just loaded a checkpoint and a graph can do before it has seen the stream.

--snapshot embeds the catalogue once per batch, at the batch's earliest event time, instead of once per (query, item) pair
(`TIGE.embed_catalogue`, then `recommend` on the snapshot; `eval_recommendation(..., catalogue_at='batch')`): every item
is scored as of the batch's start - an approximation of the exact per-pair protocol for the queries later in the batch -
and the line printed says which protocol ran.

--online --snapshot --refresh [--max_age S] serves the online replay from ONE catalogue snapshot that is kept current
incrementally: change tracking is switched on (`TIGE.track_changes`), the snapshot is taken once before the replay, every
batch is ranked on it, and after every `observe` `TIGE.refresh_catalogue(snap, t_batch_end, max_age=S)` re-embeds only the
rows that read a node the batch changed (or that are older than S) - `n_dirty / C` is printed per batch.  Items are scored
as of their last refresh, the serving approximation of --snapshot, so no offline replay is made.

--walk C [--fanout 10,10,10] retrieves before it ranks: instead of all destination nodes, every event's candidates are the
C best-connected ends of walks over the graph from its source at its own time (`TIGE.recommend_walk`: `hip_ops.
walk_candidates`, levels 1 and 3 of a three-level walk by default, then `recommend` over those ids; with --exclude_seen the
walk drops what the source has met).  Same outputs; the line printed adds recall@C, the share of events whose true
destination was among the candidates at all (`eval_recommendation(walk=...)`'s coverage: it bounds the hit rate).
--walk C --snapshot does both: the catalogue is embedded once per batch and every event's walk candidates are ranked on
the snapshot's rows (`TIGE.recommend_walk(..., snapshot=snap)`: only the sources are embedded; a candidate that is not a
destination node of the dataset is left out; `eval_recommendation(walk=dict(C=..., catalogue=...))`).  The line printed
adds in_catalogue, the share of generated candidates that the catalogue lists.
--walk C --fill T [--fill_window SECONDS] back-fills: once per batch the T most active destination nodes of the window
before the batch's earliest event time (`hip_ops.trending`; without --fill_window: of everything before it) are appended
to every row the walk leaves short, under the walk's own rules (`hip_ops.fill_candidates`; `TIGE.recommend_walk(...,
fill=dict(T=..., window=..., among=destinations))`), so a source without history gets the popular items instead of an
empty list.  The line printed reads recall@C coverage_walk -> coverage and adds `filled`, the filled share of all
candidates.
--similar S [--metric cos|ip] retrieves in embedding space before it ranks: per batch one snapshot of all destination
nodes at the batch's earliest event time; every event's seed is its source's latest neighbour before the event, its
candidates are the seed's S nearest snapshot rows by cosine or inner product (`TIGE.recommend_similar`: `hip_ops.knn_rows`,
S <= 64), ranked by the score head on the snapshot's rows (`eval_recommendation(similar=dict(S=..., catalogue=...,
metric=...))`).  The line printed adds recall@S and `seeded`, the share of events whose seed has a row.  Embedding
nearness is not what the score head was trained on; what this generator does to hit rate / NDCG is not measured.

Only `run()`, `run_online()` and `run_cold()` matter; the few flags exist to make the file runnable.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from www2023tiger_amd import hip_ops  # noqa: E402
from www2023tiger_amd.data.idmap import INT64_MIN, IdMap  # noqa: E402
from www2023tiger_amd.eval_utils import eval_recommendation  # noqa: E402
from www2023tiger_amd.init_utils import init_data, init_model  # noqa: E402


def run(data, root, ckpt_path, *, k=10, exclude_seen=False, out_dir='.', seed=0, bs=200, dim=None, n_neighbors=10, n_heads=2,
        hit_type='bin', restarter_type='seq', hist_len=40, msg_src='left', upd_src='right', strategy='recent_edges',
        device='cuda:0', snapshot=False, walk=None, fanout=(10, 10, 10), fill=None, fill_window=None, similar=None,
        metric='cos'):
    """-> (ids [n_test, k], scores [n_test, k], the eval_recommendation dict).  The model settings must be those the
    checkpoint was trained with (examples/link_prediction.py defaults here).  snapshot: one catalogue snapshot per batch
    at the batch's earliest event time (catalogue_at='batch') instead of the exact per-pair protocol.  walk=C: per-event
    walk candidates (C per event over `fanout`, the last level and, with three levels, the first one taken) instead of
    the catalogue of all destinations; the dict's coverage is then the generator's recall@C.  walk with snapshot: the
    walk's candidates ranked on the per-batch snapshot of all destinations; the dict gains in_catalogue.  fill=T (with
    walk): rows back-filled from the T most active destinations of the fill_window seconds (None: everything) before the
    batch's earliest event time; the dict gains coverage_walk and filled.  similar=S: per-event candidates are the S
    nearest rows (metric 'cos' | 'ip') of a per-batch snapshot of all destinations to the source's latest neighbour
    (TIGE.recommend_similar); the dict's coverage is the generator's recall@S and it gains seeded and candidates."""
    if fill is not None and walk is None:
        raise ValueError('fill back-fills walk candidates: give walk=C as well')
    if similar is not None and (walk is not None or snapshot or exclude_seen):
        raise ValueError('similar is a candidate generator of its own: it takes neither walk, snapshot nor exclude_seen')
    fanout = tuple(int(f) for f in fanout)
    wk = dict(fanout=fanout, take=tuple(l == len(fanout) - 1 or (l == 0 and len(fanout) == 3) for l in range(len(fanout))))
    device = torch.device(device)
    torch.manual_seed(seed)
    basic, (train_graph, full_graph), dls = init_data(
        data, root, seed, num_workers=0, bs=bs, warmup_steps=0, subset=1.0, strategy=strategy, n_layers=1,
        n_neighbors=n_neighbors, restarter_type=restarter_type, hist_len=hist_len, device=device)
    nfeats, efeats, full_data = basic[:3]
    test_dl = dls[4]
    model = init_model(nfeats, efeats, train_graph, full_graph, full_data, device, dim=dim, n_layers=1, n_heads=n_heads,
                       n_neighbors=n_neighbors, hit_type=hit_type, dropout=0.0, restarter_type=restarter_type,
                       hist_len=hist_len, msg_src=msg_src, upd_src=upd_src, msg_tsfm_type='id', mem_update_type='gru')
    model.load_state_dict(torch.load(ckpt_path, map_location=device))
    model.eval()
    model.graph = full_graph
    catalogue = torch.from_numpy(np.unique(full_data.dst).astype(np.int64)).to(device)
    col_of = hip_ops.catalogue_index(catalogue, model.n_nodes)
    fl = None if fill is None else dict(T=int(fill), window=fill_window, among=catalogue)
    start = model.save_memory_state()
    ids, scores = [], []
    with torch.no_grad():  # the lists themselves: the loop of eval_recommendation, keeping what recommend returns
        for src, dst, neg, ts, eids, _, cg in test_dl:
            src, dst, neg, eids = (x.long().to(device) for x in (src, dst, neg, eids))
            cg.to(device)
            if similar is not None:
                snap = model.embed_catalogue(catalogue, float(cg.ts64.min()), graph=full_graph)
                i, s, _, _ = model.recommend_similar(src, cg.ts64, snap, k, S=int(similar), metric=metric, graph=full_graph)
            elif walk is not None:
                snap = model.embed_catalogue(catalogue, float(cg.ts64.min()), graph=full_graph) if snapshot else None
                i, s, _, _ = model.recommend_walk(src, cg.ts64, k, C=walk, graph=full_graph, exclude_seen=exclude_seen,
                                                  snapshot=snap, fill=fl, **wk)
            else:
                items = model.embed_catalogue(catalogue, float(cg.ts64.min()), graph=full_graph) if snapshot else catalogue
                i, s, _ = model.recommend(src, cg.ts64, items, k, exclude_seen=exclude_seen, graph=full_graph, col_of=col_of)
            ids.append(i.cpu().numpy())
            scores.append(s.cpu().numpy())
            model.contrast_learning(src, dst, neg, ts.float().to(device), eids, cg)
    ids, scores = np.concatenate(ids), np.concatenate(scores)
    np.save(os.path.join(out_dir, 'ids.npy'), ids)
    np.save(os.path.join(out_dir, 'scores.npy'), scores)
    model.load_memory_state(start)  # the same pass once more, folded into the metrics
    if similar is not None:
        out = eval_recommendation(model, test_dl, device, similar=dict(S=int(similar), catalogue=catalogue, metric=metric), k=k)
    elif walk is not None:
        out = eval_recommendation(model, test_dl, device, walk=dict(wk, C=walk, **(dict(catalogue=catalogue) if snapshot else {}),
                                                                    **(dict(fill=fl) if fl is not None else {})),
                                  k=k, exclude_seen=exclude_seen)
    else:
        out = eval_recommendation(model, test_dl, device, catalogue, k=k, exclude_seen=exclude_seen,
                                  catalogue_at='batch' if snapshot else None)
    return ids, scores, out


KEY_MULT = 0x9E3779B97F4A7C15   # odd: id -> id * KEY_MULT (mod 2^64) is a bijection of the 64-bit integers


def scramble(ids) -> np.ndarray:
    """--keyed: the external key of a node id of the data set (int64, wrapping product)"""
    return (np.asarray(ids).astype(np.int64).astype(np.uint64) * np.uint64(KEY_MULT)).astype(np.int64)


def unscramble(keys) -> np.ndarray:
    return (np.asarray(keys).astype(np.int64).astype(np.uint64) * np.uint64(pow(KEY_MULT, -1, 1 << 64))).astype(np.int64)


class _Keyed:
    """--keyed: the model behind an id map.  The map is seeded with the keys of the ids the model was built on (`from_keys`:
    they keep their dense ids); ids admitted later get the next dense id in the order of their first appearance, which is
    not the data set's numbering - so the catalogue, too, is named by keys."""

    def __init__(self, model, catalogue, nfeats, idmap=None):
        self.model, self.nfeats = model, nfeats
        self.idmap = idmap if idmap is not None else IdMap.from_keys(torch.from_numpy(scramble(np.arange(1, model.n_nodes))),
                                                                     model.device)
        self.cat_keys = torch.from_numpy(scramble(catalogue.cpu().numpy())).to(model.device)
        self._n = self._cand = None

    def candidates(self):
        """the keys of the catalogue's items the model knows now, looked up again when ids were admitted"""
        if self._n != self.model.n_nodes:
            ids = self.idmap.lookup(self.cat_keys)
            self._n, self._cand = self.model.n_nodes, self.cat_keys[(ids > 0) & (ids < self.model.n_nodes)].contiguous()
        return self._cand

    def ask(self, src, t, k, exclude_seen):
        """-> keys [B, k], and which sources the model knows: a source nobody has seen yet is asked for as the last id and
        scores as a miss (as in the replay by ids)"""
        qk = torch.from_numpy(scramble(src)).to(self.model.device)
        ids = self.idmap.lookup(qk)
        known = (ids > 0) & (ids < self.model.n_nodes)
        qk = torch.where(known, qk, self.idmap.key_of[self.model.n_nodes - 1])
        keys, _, _ = self.model.recommend_keys(self.idmap, qk, t, None, k, cand_keys=self.candidates(), exclude_seen=exclude_seen)
        return keys, known

    def observe(self, s, d, t, e) -> int:
        """-> ids admitted.  The feature rows of admitted ids are those of the data set's ids their keys stand for"""
        n_old = self.model.n_nodes
        rows = None if self.nfeats is None else (lambda keys: torch.from_numpy(self.nfeats[unscramble(keys.cpu().numpy())]))
        self.model.observe_keys(self.idmap, torch.from_numpy(scramble(s)), torch.from_numpy(scramble(d)), t, e, nfeats=rows)
        return self.model.n_nodes - n_old


def _replay(model, test, catalogue, col_of, k, exclude_seen, bs, ingest, known=None, first=0, stop=None, keyed=None,
            snapshot=None):
    """recommend, then `ingest`, batch by batch over the test split -> (ids [n_test, k], dict of the metrics of
    eval_recommendation: position of the true destination in its list, folded the same way).  known: a callable -> the
    (catalogue, col_of) of the batch, for a model whose node ids grow on the way (run_online(grow=True)).  first / stop: the
    events [first, stop) of the split alone (a replay that was saved, or will be).  keyed (a _Keyed): the lists are asked
    for and returned as keys.  snapshot: a callable -> the catalogue snapshot to rank on instead of embedding the items"""
    dev = model.device
    ids, pos = [], []
    place = torch.arange(k, device=dev)
    stop = len(test.src) if stop is None else min(stop, len(test.src))
    for lo in range(first, stop, bs):
        src, dst, ts, eids = (np.ascontiguousarray(getattr(test, f)[lo:min(lo + bs, stop)]) for f in ('src', 'dst', 'ts', 'eids'))
        q, t, d = torch.from_numpy(src).to(dev), torch.from_numpy(ts.astype(np.float64)).to(dev), torch.from_numpy(dst).to(dev)
        if keyed is not None:
            i, asked = keyed.ask(src, t, k, exclude_seen)
            hit = (i == torch.from_numpy(scramble(dst)).to(dev)[:, None]) & (i != INT64_MIN) & asked[:, None]
        else:
            if known is not None:
                catalogue, col_of = known()
                q = q.clamp(max=model.n_nodes - 1)   # a source nobody has seen yet is asked for as the last id (and scores as a miss)
            i, _, _ = model.recommend(q, t, catalogue if snapshot is None else snapshot(), k, exclude_seen=exclude_seen,
                                      col_of=col_of)
            hit = (i == d[:, None]) & (i != 0)
            if known is not None:
                hit &= torch.from_numpy(src).to(dev)[:, None] < model.n_nodes
        pos.append(torch.where(hit.any(1), torch.where(hit, place, k).amin(1), -1))
        ids.append(i)
        ingest(src, dst, ts.astype(np.float64), eids)
    pos = torch.cat(pos) if pos else torch.zeros(0, dtype=torch.int64, device=dev)
    listed, p = pos >= 0, pos.clamp(min=0).double()
    n = max(1, pos.numel())
    ids = torch.cat(ids).cpu().numpy() if ids else np.zeros((0, k), dtype=np.int64)
    return ids, dict(hit_rate=float(listed.sum()) / n, ndcg=float((listed / torch.log2(p + 2)).sum()) / n,
                                              mrr_at_k=float((listed / (p + 1)).sum()) / n, n_events=pos.numel())


def run_online(data, root, ckpt_path, *, k=10, exclude_seen=False, seed=0, bs=200, dim=None, n_neighbors=10, n_heads=2,
               hit_type='bin', restarter_type='seq', hist_len=40, msg_src='left', upd_src='right', strategy='recent_edges',
               device='cuda:0', window=None, keep_last=None, release_rows=False, verbose=True, offline=True, grow=False,
               erase_nodes=None, retract_eids=None, save_state=None, save_after=None, load_state=None, keyed=False,
               churn=None, compact_at=None, late=None, late_by=1, refresh=False, max_age=None, journal=None, journal_every=1,
               apply_deltas=None, event_keys=False, redeliver=0.25):
    """-> (metrics of the online replay, metrics of the offline replay); they are equal, exactly.  Online: the graph
    covers train + validation only and grows by `observe`.  Offline: the graph over the whole stream, `stream_step`.
    window / keep_last: `forget(before=t_batch_end - window, keep_last=keep_last)` after every `observe`; the online
    metrics then carry 'forgot': (entries kept, entries dropped) per batch.  The two replays are still equal, and that is
    asserted, when what is dropped is never read: no window, keep_last >= max(n_neighbors, hist_len), no exclude_seen.
    release_rows: every forget also releases the edge-table rows that no kept entry names (`forget(...,
    release_edge_rows=True, keep_from=first eid not observed yet)`); the eids of the events still to come are shifted by
    the returned `shift`, and the online metrics carry 'rows': (table rows before, after) per batch.  What the model
    computes does not change, so the equality above holds under the same conditions.
    offline=False: the online replay alone -> (its metrics, None).
    grow: the model itself starts small - its tables and its graph cover the ids of train + validation only (num_node =
    their largest id + 1; the checkpoint's per-node rows beyond it are cut off, they are zeros) - and admits the ids the
    test split brings, batch by batch, through `observe(..., num_node='auto', nfeats=their feature rows)`.  Each batch is
    ranked among the items the model knows at that moment, so the lists differ from the offline replay's (which ranks
    items nobody has seen as well) and no offline replay is made; the metrics carry 'admitted': new ids per batch.  Data
    without a node-feature file get a zero table (the same model: a missing table means zeros).  Needs the sequence
    restarter.
    erase_nodes / retract_eids (int arrays): `erase(nodes=..., eids=...)` once, on the graph over train + validation,
    before the online replay; its metrics then carry 'erased': (entries kept, entries dropped), and the two replays are not
    held equal (the offline one still has the nodes and events).
    save_state (a path): after the online replay - of the first save_after batches, if given - the model is saved with
    `save_online`'s content plus the position: torch.save(dict(state=model.online_state(), next_event=..., shifted=...)).
    load_state (such a file): the online replay starts from it (`load_online`) instead of the graph over train +
    validation, at the file's position.  With either, no offline replay is made and the online metrics carry 'ids': the
    lists of the events replayed - a saved replay's followed by the loading one's are the uninterrupted replay's.
    keyed: the online replay runs behind an id map on scrambled keys (`observe_keys` / `recommend_keys`; module docstring);
    the online metrics carry 'ids' (int64 KEYS) and 'admitted': keys admitted per batch, and the saved file the map's state.
    Without grow the lists are scramble(the offline replay's), and that is asserted under the conditions above.
    churn (a path; keyed only): a text file of lines `batch key` - the keys that LEAVE behind that batch of the split
    (`erase_keys`: their nodes are erased, their keys removed from the map, their dense ids handed out again to the keys
    the next batches bring).  The replay prints, and its metrics carry per batch, 'released' (ids the map released) and
    'recycled' (released ids handed out again), and 'n_nodes' at the end: with accounts that come and go the model stays
    as large as its peak of live keys.  No offline replay is made.
    compact_at (a fraction F; with churn only): behind an erase, when n_free / size of the map passes F, the free ids are
    taken OUT of the id space (`compact_keys`): the live keys are renumbered densely and the map, both memories, the mailbox,
    the node table and the graph shrink to them.  The replay prints rows before -> after and its metrics carry 'compacted':
    (batch, n_nodes before, n_nodes after).  This replay holds keys, never dense ids, between batches and no `uptodate`
    bitmap; a caller that holds either passes them through the returned plan (`plan.translate`, `plan.bitmap`).
    late (a fraction in [0, 1); the plain online replay only): a seeded fraction of every test batch is HELD BACK - never
    the batch's first event - and handed to `observe_late` late_by batches later (what is still held at the end, behind
    the last batch).  A late event is ranked on time but ingested late: it becomes part of the graph - neighbours,
    histories, exclude_seen - from then on and is never streamed into the memories, so the lists differ from the offline
    replay's and none is made.  The replay prints, and its metrics carry, 'late': the number of late events merged; the
    final graph is asserted equal to the graph over the whole stream: indptr and ts exactly, nbr up to the order among
    entries of one node at one time (a late entry stands behind the on-time ones of its time).
    refresh (the plain online replay only): ONE catalogue snapshot, taken before the replay with change tracking on, serves
    every batch and is brought up to date after every `observe` by `refresh_catalogue(snap, t_batch_end, max_age=max_age)`;
    the replay prints `n_dirty / C` per batch and its metrics carry 'refreshed': (n_dirty, n_by_age) per batch.  Items are
    scored as of their last refresh, so the lists differ from the offline replay's and none is made.
    journal (a directory; not with keyed): the replay writes incremental state files there (`model.journal().save`): a base
    before the first batch, then a file after every journal_every batches - a delta that holds only the rows that changed,
    or a base again when something rewrote everything (release_rows does) - as 000000.pt, 000001.pt, ... beside
    index.json: per file its kind and the position in the split.  No offline replay is made; the metrics carry 'ids' and
    'journal': the kinds written.
    apply_deltas (such a directory; with load_state = one of its BASE files): `load_online(base)`, then
    `apply_online_delta` for every delta that follows it in the index, and the replay continues at the last file's
    position - its lists are those of the replay that wrote the files, from there on.
    event_keys (the plain online replay only; data with an edge table): the model tracks event keys (`track_events`), its
    edge table is cut back to the rows of train + validation, and every batch is delivered through `observe_events` with
    a seeded fraction `redeliver` of itself and of the previous batch a second time; the online metrics carry 'ids', 'kept'
    and 'dropped' per batch.  The lists are the plain online replay's, exactly; the two replays are held equal under the
    conditions above."""
    from www2023tiger_amd.data.graph import Graph
    forgetting = window is not None or keep_last is not None
    if journal is not None and keyed:
        raise ValueError('journal: the id map of a keyed replay is not part of the state files')
    if apply_deltas is not None and load_state is None:
        raise ValueError('apply_deltas: name the base file of the directory with load_state')
    if journal is not None or apply_deltas is not None:
        offline = False
    if refresh:
        if keyed or grow or forgetting or late is not None or erase_nodes is not None or retract_eids is not None or save_state \
                or load_state or save_after is not None:
            raise ValueError('refresh: the plain online replay only (no --keyed, --grow, --window / --keep_last, --late, erase, '
                             'save / load)')
        offline = False
    if late is not None:
        if not 0 <= float(late) < 1:
            raise ValueError(f'late = {late} is a fraction of every batch in [0, 1)')
        if int(late_by) < 1:
            raise ValueError(f'late_by = {late_by}: a late event arrives at least one batch later')
        if keyed or grow or forgetting or erase_nodes is not None or retract_eids is not None or save_state or load_state \
                or save_after is not None:
            raise ValueError('late: the plain online replay only (no --keyed, --grow, --window / --keep_last, erase, save / load)')
        offline = False
    if event_keys:
        if keyed or grow or forgetting or late is not None or refresh or erase_nodes is not None or retract_eids is not None \
                or save_state or load_state or save_after is not None or journal is not None:
            raise ValueError('event_keys: the plain online replay only (no --keyed, --grow, --window / --keep_last, --late, '
                             '--refresh, erase, save / load, --journal)')
        if not 0 <= float(redeliver) <= 1:
            raise ValueError(f'redeliver = {redeliver} is a fraction of every batch in [0, 1]')
    if churn is not None and not keyed:
        raise ValueError('churn names the nodes that leave by their keys: it needs --keyed')
    if compact_at is not None and churn is None:
        raise ValueError('compact_at compacts behind the erases of a churn file: it needs --churn')
    if compact_at is not None and not 0 <= float(compact_at) < 1:
        raise ValueError(f'compact_at = {compact_at} is a fraction of the map\'s ids in [0, 1)')
    leaving = {}
    if churn is not None:
        offline = False
        with open(churn) as f:
            for line in f:
                line = line.split('#')[0].split()
                if line:
                    leaving.setdefault(int(line[0]), []).append(int(line[1]))
    device = torch.device(device)
    torch.manual_seed(seed)
    basic, (train_graph, full_graph), dls = init_data(
        data, root, seed, num_workers=0, bs=bs, warmup_steps=0, subset=1.0, strategy=strategy, n_layers=1,
        n_neighbors=n_neighbors, restarter_type=restarter_type, hist_len=hist_len, device=device)
    nfeats, efeats, full_data, test = basic[0], basic[1], basic[2], basic[5]
    n_seen = len(full_data.src) - len(test.src)   # the test split is the tail of the stream
    seen = lambda: Graph.from_arrays(full_data.src[:n_seen], full_data.dst[:n_seen], full_data.ts[:n_seen],
                                     full_data.eids[:n_seen], strategy=full_graph.strategy, seed=seed,
                                     max_node_id=n0 - 1, device=device)
    n0 = full_graph.num_node
    state = torch.load(ckpt_path, map_location=device)
    if grow:
        n0 = int(max(full_data.src[:n_seen].max(), full_data.dst[:n_seen].max())) + 1
        width = dim if dim is not None else (efeats.shape[1] if efeats is not None else None)
        if nfeats is None and width is None:
            raise ValueError('grow: the data have neither a node nor an edge table to take the feature width from: give dim')
        nfeats = np.zeros((full_graph.num_node, width), dtype=np.float32) if nfeats is None else nfeats
        n_full, offline = full_graph.num_node, False
        train_graph = full_graph = seen()   # (the model is built on the ids seen so far)
        # per-node rows of the checkpoint (memories; a model trained on the full id space) beyond the ids seen so far
        per_node = [key for key, v in state.items()
                    if v.dim() and v.shape[0] == n_full and key.split('.')[0].endswith('_memory')]
        for key in per_node:
            if bool(state[key][n0:].any()):   # (e.g. a checkpoint saved after a pass over the test split)
                raise ValueError(f'grow: {key} of the checkpoint holds state for node ids beyond {n0 - 1}, which train + '
                                 'validation never name; cutting its rows off would drop it')
            state[key] = state[key][:n0]
    model = init_model(nfeats[:n0] if grow else nfeats, efeats, train_graph, full_graph, full_data, device, dim=dim, n_layers=1,
                       n_heads=n_heads, n_neighbors=n_neighbors, hit_type=hit_type, dropout=0.0, restarter_type=restarter_type,
                       hist_len=hist_len, msg_src=msg_src, upd_src=upd_src, msg_tsfm_type='id', mem_update_type='gru')
    model.load_state_dict(state)
    model.eval()
    catalogue = torch.from_numpy(np.unique(full_data.dst).astype(np.int64)).to(device)
    col_of = None if grow else hip_ops.catalogue_index(catalogue, model.n_nodes)
    start = model.save_memory_state()
    partial = save_after is not None or load_state is not None
    first, stop = 0, None if save_after is None else int(save_after) * bs
    with torch.no_grad():
        ids_off = None
        if offline and not partial:
            model.graph = full_graph
            ids_off, offline = _replay(model, test, catalogue, col_of, k, exclude_seen, bs,
                                       lambda s, d, t, e: model.stream_step(s, d, d, t, e))
            model.load_memory_state(start)
        # the edge table already holds the rows of the test events; a live system hands them to observe(efeats=...)
        shifted = [0]   # rows released so far: the eids of the events still to come moved down by as much
        if load_state is None:
            model.graph = seen()
        else:   # (checks everything, the graph with tg_tcsr_verify, before anything changes; grows the tables if need be)
            blob = torch.load(load_state, map_location='cpu', weights_only=True)
            if apply_deltas is not None:   # a base of a journal directory and the deltas behind it, in the index's order
                with open(os.path.join(apply_deltas, 'index.json')) as f:
                    index = json.load(f)
                at = [i for i, x in enumerate(index) if x['file'] == os.path.basename(load_state) and x['kind'] == 'base']
                if not at:
                    raise ValueError(f'{load_state} is no base file of {apply_deltas}/index.json')
                model.load_online(blob)
                blob = dict(next_event=index[at[0]]['next_event'], shifted=index[at[0]]['shifted'])
                for x in index[at[0] + 1:]:
                    if x['kind'] != 'delta':
                        break
                    model.apply_online_delta(os.path.join(apply_deltas, x['file']))
                    blob = dict(next_event=x['next_event'], shifted=x['shifted'])
                    if verbose:
                        print(f"applied {x['file']}: {model.n_nodes} node ids, {int(model.graph.tcsr.num_entry)} entries")
            else:
                model.load_online(blob['state'])
            first, shifted[0] = int(blob['next_event']), int(blob['shifted'])
            if keyed and 'idmap' not in blob:
                raise ValueError(f'{load_state} was saved by a replay without --keyed: it holds no id map')
            if verbose:
                print(f'loaded {load_state}: {model.n_nodes} node ids, {int(model.graph.tcsr.num_entry)} entries, '
                      f'continuing at event {first} of the split')
        if keyed:
            keyed = _Keyed(model, catalogue, nfeats if grow else None,
                           None if load_state is None else IdMap.from_state_dict(blob['idmap'], device))
        erasing = erase_nodes is not None or retract_eids is not None
        erased = None
        if erasing:
            before = int(model.graph.tcsr.num_entry)
            g = model.erase(nodes=erase_nodes, eids=retract_eids)
            erased = (int(g.tcsr.num_entry), before - int(g.tcsr.num_entry))
            if verbose:
                print(f'erase: {0 if erase_nodes is None else len(erase_nodes)} nodes, '
                      f'{0 if retract_eids is None else len(retract_eids)} eids: {erased[0]} entries kept, {erased[1]} dropped')
        forgot = []
        rows = []

        admitted = []
        released, recycled, compacted = [], [], []
        cache = {}

        def known():   # the items the model knows now (and their index), rebuilt when ids were admitted
            if cache.get('n') != model.n_nodes:
                items = catalogue[catalogue < model.n_nodes]
                cache.update(n=model.n_nodes, items=items, col_of=hip_ops.catalogue_index(items, model.n_nodes))
            return cache['items'], cache['col_of']

        def observe(s, d, t, e):
            if keyed:
                free = keyed.idmap.n_free
                admitted.append(keyed.observe(s, d, t, e))
                if verbose:
                    print(f'batch {len(admitted) - 1}: {admitted[-1]} keys admitted, {keyed.idmap.size - 1} known')
                if churn is not None:
                    b = first // bs + len(admitted) - 1
                    recycled.append(free - keyed.idmap.n_free)
                    gone = leaving.get(b)
                    released.append(0 if not gone else
                                    int(model.erase_keys(keyed.idmap, torch.tensor(gone, dtype=torch.int64))[1].numel()))
                    keyed._n = None   # (the catalogue's keys are looked up again: items may have left or come back)
                    if verbose:
                        print(f'batch {b}: {released[-1]} ids released, {recycled[-1]} recycled, n_nodes {model.n_nodes}')
                    m = keyed.idmap
                    if compact_at is not None and m.n_free and m.n_free / m.size > float(compact_at):
                        rows_before, slots = model.n_nodes, m.capacity
                        model.compact_keys(m)
                        compacted.append((b, rows_before, int(model.n_nodes)))
                        if verbose:
                            print(f'batch {b}: compacted: {rows_before} rows -> {model.n_nodes}, map {slots} slots -> {m.capacity}')
                return
            if not grow:
                return model.observe(s, d, t, e)
            n_old, n_new = model.n_nodes, max(model.n_nodes, int(max(s.max(), d.max())) + 1)
            model.observe(s, d, t, e, num_node='auto', nfeats=torch.from_numpy(nfeats[n_old:n_new]))
            admitted.append(model.n_nodes - n_old)
            if verbose:
                print(f'batch {len(admitted) - 1}: {admitted[-1]} node ids admitted, {model.n_nodes} known')

        def observe_and_forget(s, d, t, e):
            e = e - shifted[0]
            observe(s, d, t, e)
            before = model.graph.tcsr.num_entry
            g = model.forget(before=None if window is None else float(t[-1]) - window, keep_last=keep_last,
                             release_edge_rows=release_rows, keep_from=int(e[-1]) + 1 if release_rows else None)
            forgot.append((int(g.tcsr.num_entry), int(before - g.tcsr.num_entry)))
            if verbose:
                print(f'batch {len(forgot) - 1}: {forgot[-1][0]} entries kept, {forgot[-1][1]} dropped')
            rel = model.last_release if release_rows else None
            if rel is not None:
                shifted[0] += rel.shift
                rows.append((rel.rows_before, rel.rows))
                if verbose:
                    print(f'batch {len(forgot) - 1}: edge table {rel.rows_before} rows -> {rel.rows}')
        held, n_late, rs_late = [], [0, 0], np.random.RandomState(seed)   # (due batch, s, d, t, e); merged, batches

        def merge_due(upto):
            while held and held[0][0] <= upto:
                ev = held.pop(0)[1:]
                model.observe_late(*ev)   # (the edge table already holds their rows: no efeats)
                n_late[0] += len(ev[0])

        def observe_some_late(s, d, t, e):
            m = rs_late.uniform(size=len(s)) < float(late)
            m[0] = False
            observe(s[~m], d[~m], t[~m], e[~m])
            b = n_late[1]
            n_late[1] += 1
            if m.any():
                held.append((b + int(late_by), s[m], d[m], t[m], e[m]))
            merge_due(b)
        ingest = observe_and_forget if forgetting else (observe if late is None else observe_some_late)
        kept, dropped = [], []
        if event_keys:   # the table holds the rows of the events seen so far; the rest arrives with its events
            fg = model.raw_feat_getter
            if fg.efeats is None:
                raise ValueError('event_keys: the data have no edge table; event keys name its rows')
            table = fg.efeats
            fg.efeats = table[:n_seen + 1].clone()
            model.invalidate_struct()
            model.track_events(torch.from_numpy(scramble(np.arange(1, n_seen + 1))))
            rs_bus, last = np.random.RandomState(seed), [None]

            def ingest(s, d, t, e):
                def again(b):   # a seeded share of the events of b, all four arrays by ONE draw
                    m = rs_bus.uniform(size=len(b[0])) < float(redeliver)
                    return tuple(a[m] for a in b)
                parts = ([again(last[0])] if last[0] is not None else []) + [(s, d, t, e), again((s, d, t, e))]
                s2, d2, t2, e2 = (np.concatenate([p[i] for p in parts]) for i in range(4))
                _, adm = model.observe_events(s2, d2, t2, torch.from_numpy(scramble(e2)), efeats=table[torch.from_numpy(e2).to(device)])
                assert adm.n_kept == len(s) and np.array_equal(adm.eids[adm.keep].cpu().numpy(), e)   # (no row was released)
                kept.append(adm.n_kept)
                dropped.append(len(s2) - adm.n_kept)
                last[0] = (s, d, t, e)
                if verbose:
                    print(f'batch {len(kept) - 1}: {kept[-1]} events kept, {dropped[-1]} redelivered copies dropped')
        snap, refreshed = [None], []
        if refresh:   # the tracker first: the snapshot remembers the tracker's epoch
            model.track_changes()
            snap[0] = model.embed_catalogue(catalogue, float(full_data.ts[n_seen - 1]))

            def ingest(s, d, t, e):
                observe(s, d, t, e)
                snap[0] = model.refresh_catalogue(snap[0], float(t[-1]), max_age=max_age)
                refreshed.append(model.last_refreshed)
                if verbose:
                    print(f'batch {len(refreshed) - 1}: refreshed {refreshed[-1][0]} / {len(snap[0])} rows '
                          f'({refreshed[-1][1]} by age alone)')
        written = []
        if journal is not None:
            os.makedirs(journal, exist_ok=True)
            J, inner, at = model.journal(), ingest, [first, 0]

            def save_file():
                name = f'{len(written):06d}.pt'
                kind = J.save(os.path.join(journal, name))
                written.append(dict(file=name, kind=kind, next_event=at[0], shifted=shifted[0]))
                with open(os.path.join(journal, 'index.json'), 'w') as f:
                    json.dump(written, f)
                if verbose:
                    print(f'journal: {name} ({kind}) at event {at[0]}: {os.path.getsize(os.path.join(journal, name))} bytes')

            def ingest(s, d, t, e):
                inner(s, d, t, e)
                at[0] += len(s)
                at[1] += 1
                if at[1] % int(journal_every) == 0:
                    save_file()
            save_file()
        ids_on, online = _replay(model, test, catalogue, col_of, k, exclude_seen, bs, ingest, known=known if grow else None,
                                 first=first, stop=stop, keyed=keyed or None, snapshot=(lambda: snap[0]) if refresh else None)
        if late is not None:
            merge_due(float('inf'))
            if verbose:
                print(f'late: {n_late[0]} of {online["n_events"]} events were held back and merged by observe_late')
            got, want = (tuple(a.cpu().numpy() for a in g._tensors()) for g in (model.graph, full_graph))
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.int64), want[1].view(np.int64))
            owner = np.repeat(np.arange(len(want[0]) - 1), np.diff(want[0]))
            by_time = lambda a: a[2][np.lexsort((a[2], a[1], owner))]   # (ties of one node at one time: by neighbour)
            assert np.array_equal(by_time(got), by_time(want))
        if save_state is not None:
            done = len(test.src) if stop is None else min(stop, len(test.src))
            blob = dict(state=model.online_state(), next_event=done, shifted=shifted[0])
            if keyed:
                blob['idmap'] = keyed.idmap.state_dict()
            torch.save(blob, save_state)
            if verbose:
                print(f'saved {save_state}: {model.n_nodes} node ids, {int(model.graph.tcsr.num_entry)} entries, '
                      f'{done} events of the split replayed')
    need = max(n_neighbors, hist_len if restarter_type == 'seq' else 0)
    if ids_off is not None and not erasing and (not forgetting or (window is None and keep_last >= need and not exclude_seen)):
        # (keyed: the padding id 0 of a short list is INT64_MIN among keys)
        want = np.where(ids_off == 0, INT64_MIN, scramble(ids_off)) if keyed else ids_off
        assert np.array_equal(ids_on, want) and online == offline, (online, offline)
    if partial or save_state is not None or keyed or journal is not None or event_keys:
        online = dict(online, ids=ids_on)
    if journal is not None:
        online = dict(online, journal=[x['kind'] for x in written])
    if grow or keyed:
        online = dict(online, admitted=admitted)
    if keyed:
        online = dict(online, n_nodes=int(model.n_nodes))
    if churn is not None:
        online = dict(online, released=released, recycled=recycled)
    if compact_at is not None:
        online = dict(online, compacted=compacted)
    if erasing:
        online = dict(online, erased=erased)
    if late is not None:
        online = dict(online, late=n_late[0])
    if refresh:
        online = dict(online, refreshed=refreshed)
    if event_keys:
        online = dict(online, kept=kept, dropped=dropped)
    if forgetting:
        online = dict(online, forgot=forgot)
        if release_rows:
            online['rows'] = rows
    return online, (offline if ids_off is not None else None)


def run_cold(data, root, ckpt_path, *, k=10, exclude_seen=False, seed=0, bs=200, dim=None, n_neighbors=10, n_heads=2,
             hit_type='bin', restarter_type='seq', hist_len=40, msg_src='left', upd_src='right', strategy='recent_edges',
             device='cuda:0', verbose=True):
    """-> (metrics over the test split, restarted nodes per batch).  No replay of train + validation: memories at reset, an
    empty bitmap, `recommend(..., uptodate=bitmap)` batch by batch on the full graph."""
    device = torch.device(device)
    torch.manual_seed(seed)
    basic, (train_graph, full_graph), dls = init_data(
        data, root, seed, num_workers=0, bs=bs, warmup_steps=0, subset=1.0, strategy=strategy, n_layers=1,
        n_neighbors=n_neighbors, restarter_type=restarter_type, hist_len=hist_len, device=device)
    nfeats, efeats, full_data, test = basic[0], basic[1], basic[2], basic[5]
    model = init_model(nfeats, efeats, train_graph, full_graph, full_data, device, dim=dim, n_layers=1, n_heads=n_heads,
                       n_neighbors=n_neighbors, hit_type=hit_type, dropout=0.0, restarter_type=restarter_type,
                       hist_len=hist_len, msg_src=msg_src, upd_src=upd_src, msg_tsfm_type='id', mem_update_type='gru')
    model.load_state_dict(torch.load(ckpt_path, map_location=device))
    model.eval()
    model.graph = full_graph
    model.reset()   # the checkpoint's memories are not used: every node the scores read is restarted on first use
    catalogue = torch.from_numpy(np.unique(full_data.dst).astype(np.int64)).to(device)
    col_of = hip_ops.catalogue_index(catalogue, model.n_nodes)
    bitmap = hip_ops.new_bitmap(model.n_nodes, device)
    restarted, pos = [], []
    place = torch.arange(k, device=device)
    with torch.no_grad():
        for lo in range(0, len(test.src), bs):
            src, dst, ts, eids = (np.ascontiguousarray(getattr(test, f)[lo:lo + bs]) for f in ('src', 'dst', 'ts', 'eids'))
            q, d = torch.from_numpy(src).to(device), torch.from_numpy(dst).to(device)
            t = torch.from_numpy(ts.astype(np.float64)).to(device)
            i, _, _ = model.recommend(q, t, catalogue, k, exclude_seen=exclude_seen, col_of=col_of, uptodate=bitmap)
            restarted.append(model.last_restarted)
            hit = (i == d[:, None]) & (i != 0)
            pos.append(torch.where(hit.any(1), torch.where(hit, place, k).amin(1), -1))
            if verbose:
                print(f'batch {lo // bs}: {restarted[-1]} nodes restarted, HitRate@{k} {float((pos[-1] >= 0).float().mean()):.4f}')
            # the batch's own nodes are among the restarted ones (its sources are queries, its destinations in the catalogue)
            model.stream_step(src, dst, dst, ts.astype(np.float64), eids)
    pos = torch.cat(pos)
    listed, p = pos >= 0, pos.clamp(min=0).double()
    n = max(1, pos.numel())
    return dict(hit_rate=float(listed.sum()) / n, ndcg=float((listed / torch.log2(p + 2)).sum()) / n,
                mrr_at_k=float((listed / (p + 1)).sum()) / n, n_events=pos.numel()), restarted


if __name__ == '__main__':
    ap = argparse.ArgumentParser(description='Write top-k recommendation lists for the test split of a TIGER checkpoint.')
    ap.add_argument('-d', '--data', default='wikipedia')
    ap.add_argument('--root', default='.')
    ap.add_argument('--ckpt', required=True, help='checkpoint written by examples/link_prediction.py')
    ap.add_argument('--k', type=int, default=10)
    ap.add_argument('--exclude_seen', action='store_true', help='leave out the items a source has already interacted with')
    ap.add_argument('--out_dir', default='.')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--bs', type=int, default=200)
    ap.add_argument('--restarter_type', default='seq', choices=['seq', 'static'])
    ap.add_argument('--online', action='store_true', help='replay the test split through TIGE.observe on a graph that '
                    'starts at train + validation, beside the replay on the full graph')
    ap.add_argument('--cold', action='store_true', help='no replay: memories at reset, lazy restarts of what each batch reads '
                    '(recommend(..., uptodate=bitmap)); prints the restart count per batch')
    ap.add_argument('--snapshot', action='store_true', help='embed the catalogue once per batch at the batch\'s earliest '
                    'event time (eval_recommendation(..., catalogue_at=\'batch\')) instead of once per pair')
    ap.add_argument('--window', type=float, default=None, help='--online: after every observe, forget the entries older '
                    'than the batch\'s last time minus this many seconds (TIGE.forget)')
    ap.add_argument('--keep_last', type=int, default=None, help='--online: after every observe, keep every node\'s last M '
                    'entries (TIGE.forget)')
    ap.add_argument('--release_rows', action='store_true', help='--online with --keep_last / --window: every forget also '
                    'releases the edge-table rows of the forgotten events (TIGE.forget(..., release_edge_rows=True)) and the '
                    'eids still to come are shifted; prints the table\'s rows before and after per batch')
    ap.add_argument('--grow', action='store_true', help='--online: the model starts with the node ids of train + validation '
                    '(num_node = their largest id + 1) and admits the ids the test split brings (TIGE.observe(..., '
                    "num_node='auto')); prints the ids admitted per batch; no offline replay")
    ap.add_argument('--erase_nodes', default=None, metavar='FILE', help='--online: a .npy of node ids that are erased once '
                    'before the replay (TIGE.erase); prints the entries dropped')
    ap.add_argument('--retract_eids', default=None, metavar='FILE', help='--online: a .npy of edge ids that are retracted '
                    'once before the replay (TIGE.erase); prints the entries dropped')
    ap.add_argument('--save_state', default=None, metavar='PATH', help='--online: save the served model after the replay '
                    '(TIGE.save_online and the position in the split)')
    ap.add_argument('--save_after', type=int, default=None, metavar='N', help='--save_state: stop the replay after N batches')
    ap.add_argument('--load_state', default=None, metavar='PATH', help='--online: start from a file of --save_state instead '
                    'of train + validation (TIGE.load_online) and replay the rest of the split')
    ap.add_argument('--journal', default=None, metavar='DIR', help='--online: write incremental state files to DIR '
                    '(TIGE.journal().save: a base, then deltas that hold only the rows that changed) and index.json')
    ap.add_argument('--journal_every', type=int, default=1, metavar='N', help='--journal: a file after every N batches (default 1)')
    ap.add_argument('--apply_deltas', default=None, metavar='DIR', help='--online --load_state DIR/BASE.pt: load that base of a '
                    '--journal directory, apply the deltas behind it (TIGE.apply_online_delta) and replay the rest of the split')
    ap.add_argument('--keyed', action='store_true', help='--online: every node id becomes an external 64-bit key; the model '
                    'sits behind a device id map (observe_keys / recommend_keys) and ids.npy holds keys')
    ap.add_argument('--compact_at', type=float, default=None, metavar='F', help='--online --keyed --churn FILE: behind an erase, '
                    'when n_free / size of the id map passes F, the free ids are taken out of the id space '
                    '(TIGE.compact_keys): map, memories, mailbox, node table and graph shrink to the live keys; rows before '
                    '-> after are printed')
    ap.add_argument('--churn', default=None, metavar='FILE', help='--online --keyed: a text file of lines "batch key" - the '
                    'keys that leave behind that batch (TIGE.erase_keys); their dense ids are handed out again, and the ids '
                    'released and recycled and n_nodes are printed per batch')
    ap.add_argument('--late', type=float, default=None, metavar='FRACTION', help='--online: hold a seeded fraction of every '
                    'test batch back and hand it to TIGE.observe_late --late_by batches later; prints the late events merged')
    ap.add_argument('--late_by', type=int, default=1, metavar='BATCHES', help='--late: how many batches later (default 1)')
    ap.add_argument('--event_keys', action='store_true', help='--online: name events by external 64-bit keys and deliver every '
                    'batch at least once (TIGE.track_events / observe_events); kept / dropped are printed per batch')
    ap.add_argument('--redeliver', type=float, default=0.25, metavar='P', help='--event_keys: the fraction of every batch that '
                    'arrives a second time, with the batch itself and with the next one (default 0.25)')
    ap.add_argument('--refresh', action='store_true', help='--online --snapshot: serve the replay from ONE catalogue snapshot, '
                    'refreshed incrementally after every observe (TIGE.track_changes, TIGE.refresh_catalogue)')
    ap.add_argument('--max_age', type=float, default=None, metavar='S', help='--refresh: also re-embed rows older than S time units')
    ap.add_argument('--walk', type=int, default=None, metavar='C', help='retrieve C walk candidates per event from the graph '
                    '(TIGE.recommend_walk) instead of ranking all destination nodes; prints recall@C')
    ap.add_argument('--fanout', default='10,10,10', help='--walk: entries followed per node at each level, e.g. 10,10,10')
    ap.add_argument('--fill', type=int, default=None, metavar='T', help='--walk: back-fill short rows from the T most active '
                    'destination nodes before the batch (hip_ops.trending, hip_ops.fill_candidates)')
    ap.add_argument('--fill_window', type=float, default=None, metavar='SECONDS', help='--fill: count activity in this many '
                    'seconds before the batch\'s earliest event time (default: everything before it)')
    ap.add_argument('--similar', type=int, default=None, metavar='S', help='retrieve the S nearest snapshot rows of each '
                    "source's latest neighbour in embedding space (TIGE.recommend_similar, S <= 64); prints recall@S")
    ap.add_argument('--metric', default='cos', choices=['cos', 'ip'], help='--similar: cosine or inner product')
    a = ap.parse_args()
    if a.cold:
        m, restarted = run_cold(a.data, a.root, a.ckpt, k=a.k, exclude_seen=a.exclude_seen, seed=a.seed, bs=a.bs,
                                restarter_type=a.restarter_type)
        print(f"cold: HitRate@{a.k} {m['hit_rate']:.4f}  NDCG@{a.k} {m['ndcg']:.4f}  MRR@{a.k} {m['mrr_at_k']:.4f}  "
              f"({m['n_events']} events, {sum(restarted)} restarts over {len(restarted)} batches)")
        sys.exit(0)
    if a.refresh and not (a.online and a.snapshot):
        ap.error('--refresh keeps the snapshot of an online replay current: it needs --online --snapshot')
    if a.online:
        for name, m in zip(('online ', 'offline'), run_online(a.data, a.root, a.ckpt, k=a.k, exclude_seen=a.exclude_seen,
                                                              seed=a.seed, bs=a.bs, restarter_type=a.restarter_type,
                                                              window=a.window, keep_last=a.keep_last,
                                                              release_rows=a.release_rows, grow=a.grow,
                                                              erase_nodes=None if a.erase_nodes is None else np.load(a.erase_nodes),
                                                              retract_eids=None if a.retract_eids is None
                                                              else np.load(a.retract_eids), save_state=a.save_state,
                                                              save_after=a.save_after, load_state=a.load_state,
                                                              keyed=a.keyed, churn=a.churn, compact_at=a.compact_at,
                                                              late=a.late, late_by=a.late_by, refresh=a.refresh,
                                                              max_age=a.max_age, journal=a.journal,
                                                              journal_every=a.journal_every, apply_deltas=a.apply_deltas,
                                                              event_keys=a.event_keys, redeliver=a.redeliver)):
            if m is None:
                continue
            if a.keyed and 'ids' in m:
                np.save(os.path.join(a.out_dir, 'ids.npy'), m['ids'])   # int64 keys; INT64_MIN pads a short list
            print(f"{name}: HitRate@{a.k} {m['hit_rate']:.6f}  NDCG@{a.k} {m['ndcg']:.6f}  MRR@{a.k} {m['mrr_at_k']:.6f}  "
                  f"({m['n_events']} events)")
        sys.exit(0)
    ids, _, m = run(a.data, a.root, a.ckpt, k=a.k, exclude_seen=a.exclude_seen, out_dir=a.out_dir, seed=a.seed, bs=a.bs,
                    restarter_type=a.restarter_type, snapshot=a.snapshot, walk=a.walk, fanout=a.fanout.split(','),
                    fill=a.fill, fill_window=a.fill_window, similar=a.similar, metric=a.metric)
    print('protocol: ' + (f'the {a.similar} nearest snapshot rows ({a.metric}) of the source\'s latest neighbour, ranked on one '
                          "catalogue snapshot per batch at the batch's earliest event time"
                          if a.similar is not None else
                          f'{a.walk} walk candidates per event (fanout {a.fanout}), ranked on one catalogue snapshot per batch '
                          "at the batch's earliest event time"
                          if a.walk is not None and a.snapshot else
                          f'{a.walk} walk candidates per event (fanout {a.fanout}), each pair embedded at the query\'s time'
                          if a.walk is not None else
                          "one catalogue snapshot per batch at the batch's earliest event time (catalogue_at='batch')"
                          if a.snapshot else 'exact - every (query, item) pair embedded at the query\'s time'))
    cov = f"recall@{a.walk} {m['coverage']:.4f}" if a.walk is not None else f"coverage {m['coverage']:.4f}"
    if a.similar is not None:
        cov = f"recall@{a.similar} {m['coverage']:.4f}  seeded {m['seeded']:.4f}"
    if 'coverage_walk' in m:
        cov = f"recall@{a.walk} {m['coverage_walk']:.4f} -> {m['coverage']:.4f}  filled {m['filled']:.4f}"
    if 'in_catalogue' in m:
        cov += f"  in_catalogue {m['in_catalogue']:.4f}"
    print(f"test: HitRate@{a.k} {m['hit_rate']:.4f}  NDCG@{a.k} {m['ndcg']:.4f}  MRR@{a.k} {m['mrr_at_k']:.4f}  "
          f"{cov}  ({m['n_events']} events, {ids.shape[0]} lists written)")
