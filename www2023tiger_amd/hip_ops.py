"""Thin torch-tensor wrappers around the C ABI (one function per entry point).

Tensors are plumbing: they own device memory and name the stream; all work
happens in libtiger_hip.so.
"""
import ctypes as C_
from typing import Optional, Tuple

import torch
from torch import Tensor

from . import _lib
from ._lib import check, lib, ptr


def stream_ptr(device=None) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _i64(t: Tensor) -> Tensor:
    return t.contiguous() if t.dtype == torch.int64 else t.long().contiguous()


def new_err(device) -> Tensor:
    return torch.zeros(1, dtype=torch.int32, device=device)


def raise_if_err(err: Tensor):
    """Reads the invariant word back (one host sync) and raises the reference's ValueError."""
    _lib.raise_invariants(int(err.item()) & 0xFFFFFFFF)


def bitmap_words(n_nodes: int) -> int:
    return int(lib.tg_bitmap_words(n_nodes))


def new_bitmap(n_nodes: int, device) -> Tensor:
    return torch.zeros(bitmap_words(n_nodes), dtype=torch.int64, device=device)


def bitmap_grown(bits: Tensor, n_new: int) -> Tensor:
    """A bitmap of `new_bitmap` over n_new node ids with the bits of `bits` (a bitmap over fewer ids: TIGE.grow_nodes admitted
    new ones since) - `bits` itself while the word count stands, else a zero-padded copy.  ValueError: bits is no int64
    bitmap, or it holds more words than n_new ids take (ids are never released)."""
    W = bitmap_words(n_new)
    if not torch.is_tensor(bits) or bits.dtype != torch.int64 or bits.dim() != 1 or bits.numel() > W:
        what = f'{bits.dtype} {tuple(bits.shape)}' if torch.is_tensor(bits) else type(bits).__name__
        raise ValueError(f'bitmap_grown: {what} is no int64 bitmap of at most {W} words ({n_new} node ids)')
    if bits.numel() == W:
        return bits
    out = torch.zeros(W, dtype=torch.int64, device=bits.device)
    out[:bits.numel()] = bits
    return out


def bitmap_mark(ids: Tensor, bitmap: Tensor, n_nodes: int):
    ids = _i64(ids)
    check(lib.tg_bitmap_mark(ids.numel(), ptr(ids), ptr(bitmap), n_nodes, stream_ptr(ids.device)), 'tg_bitmap_mark')


def new_flags(n_nodes: int, device) -> Tensor:
    """zeroed byte flags, one per node (padded to a multiple of 64)"""
    return torch.zeros(int(lib.tg_flag_bytes(n_nodes)), dtype=torch.uint8, device=device)


def flags_mark(ids: Tensor, flags: Tensor, n_nodes: int):
    ids = _i64(ids)
    check(lib.tg_flags_mark(ids.numel(), ptr(ids), ptr(flags), n_nodes, stream_ptr(ids.device)), 'tg_flags_mark')


def unique_compact(bitmap: Optional[Tensor], n_nodes: int, cap: int, and_bitmap: Optional[Tensor] = None,
                   flags: Optional[Tensor] = None):
    """-> dict(bitmap, rank, ids, count [, and_rank, and_ids, and_pos, and_count]); lists have
    capacity `cap`.  Either `bitmap` (input) or `flags` (packed into a fresh bitmap) is given."""
    dev = (bitmap if bitmap is not None else flags).device
    if bitmap is None:
        bitmap = torch.empty(bitmap_words(n_nodes), dtype=torch.int64, device=dev)
    W = bitmap_words(n_nodes)
    out = dict(bitmap=bitmap, rank=torch.empty(W + 1, dtype=torch.int32, device=dev),
               ids=torch.empty(cap, dtype=torch.int64, device=dev),
               count=torch.zeros(1, dtype=torch.int32, device=dev))
    a = [None] * 4
    if and_bitmap is not None:
        out.update(and_rank=torch.empty(W + 1, dtype=torch.int32, device=dev),
                   and_ids=torch.empty(cap, dtype=torch.int64, device=dev),
                   and_pos=torch.empty(cap, dtype=torch.int32, device=dev),
                   and_count=torch.zeros(1, dtype=torch.int32, device=dev))
        a = [out['and_rank'], out['and_ids'], out['and_pos'], out['and_count']]
    nbytes = int(lib.tg_unique_compact_workspace_bytes(n_nodes))
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    check(lib.tg_unique_compact(ptr(flags), ptr(bitmap), n_nodes, ptr(out['rank']), ptr(out['ids']), ptr(out['count']), cap,
                                ptr(and_bitmap), ptr(a[0]), ptr(a[1]), ptr(a[2]), ptr(a[3]), ptr(ws), ws.numel(),
                                stream_ptr(dev)), 'tg_unique_compact')
    return out


def select_latest_nids(nids: Tensor, ts: Tensor, n_nodes: Optional[int] = None) -> Tuple[Tensor, Tensor]:
    """tiger/model/utils.py:10-16 on device: (sorted unique ids, position of the latest
    occurrence, first position among equal timestamps)."""
    nids = _i64(nids)
    dev = nids.device
    n = nids.numel()
    if n == 0:
        return nids.new_empty(0), nids.new_empty(0)
    if ts.dtype not in (torch.float32, torch.float64):
        ts = ts.double()
    ts = ts.contiguous()
    if n_nodes is None:
        n_nodes = int(nids.max().item()) + 1
    uniq = torch.empty(n, dtype=torch.int64, device=dev)
    index = torch.empty(n, dtype=torch.int64, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    nbytes = int(lib.tg_select_latest_workspace_bytes(n, n_nodes))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    check(lib.tg_select_latest(n, ptr(nids), ptr(ts), 1 if ts.dtype == torch.float64 else 0, n_nodes, ptr(uniq),
                               ptr(index), ptr(count), ptr(ws), nbytes, stream_ptr(dev)), 'tg_select_latest')
    p = int(count.item())
    return uniq[:p], index[:p]


def anonymized_reindex(hist_nids: Tensor) -> Tensor:
    """tiger/model/utils.py:19-27 on an [n, H] id matrix (H <= 64)."""
    hist_nids = _i64(hist_nids)
    out = torch.empty_like(hist_nids)
    n, H = hist_nids.shape
    check(lib.tg_anonymized_reindex(n, H, ptr(hist_nids), ptr(out), stream_ptr(hist_nids.device)),
          'tg_anonymized_reindex')
    return out


def hits(center: Tensor, nbr: Tensor) -> Tensor:
    """data_loader.py:61-67: (center[:, None] == nbr) as float32."""
    center, nbr = _i64(center), _i64(nbr)
    B, K = nbr.shape
    out = torch.empty(B, K, dtype=torch.float32, device=nbr.device)
    check(lib.tg_hits(B, K, ptr(center), ptr(nbr), ptr(out), stream_ptr(nbr.device)), 'tg_hits')
    return out


def time_encode(ts: Tensor, freq: Tensor, phase: Tensor) -> Tensor:
    """time_encoding.py:24-26."""
    flat = ts.contiguous().float().reshape(-1)
    d = freq.numel()
    out = torch.empty(flat.numel(), d, dtype=torch.float32, device=ts.device)
    check(lib.tg_time_encode(flat.numel(), ptr(flat), d, ptr(freq), ptr(phase), ptr(out), stream_ptr(ts.device)),
          'tg_time_encode')
    return out.reshape(*ts.shape, d)


def gather_rows(table: Tensor, ids: Tensor, ts_table: Optional[Tensor] = None):
    ids_f = _i64(ids).reshape(-1)
    width = table.shape[1]
    dev = ids_f.device if table.device.type == 'cpu' else table.device  # a pinned host table is read from the ids' GPU
    out = torch.empty(ids_f.numel(), width, dtype=torch.float32, device=dev)
    ts_out = torch.empty(ids_f.numel(), dtype=torch.float32, device=dev) if ts_table is not None else None
    check(lib.tg_gather_rows(ids_f.numel(), ptr(ids_f), width, ptr(table), ptr(out), ptr(ts_table), ptr(ts_out),
                             stream_ptr(dev)), 'tg_gather_rows')
    out = out.reshape(*ids.shape, width)
    if ts_table is None:
        return out
    return out, ts_out.reshape(ids.shape)


def memory_scatter(table: Tensor, ts_table: Tensor, active: Optional[Tensor], ids: Tensor, vals: Tensor, ts: Tensor,
                   src_index: Optional[Tensor] = None, check_past: bool = False, err: Optional[Tensor] = None):
    ids = _i64(ids)
    vals = vals.contiguous().float()
    ts = ts.contiguous().float()
    if src_index is not None:
        src_index = _i64(src_index)
    if check_past and err is None:
        raise ValueError('check_past needs an err word')
    check(lib.tg_memory_scatter(ids.numel(), None, ptr(ids), ptr(src_index), table.shape[1], ptr(vals), ptr(ts),
                                ptr(table), ptr(ts_table), ptr(active), 1 if check_past else 0, ptr(err),
                                stream_ptr(table.device)), 'tg_memory_scatter')


# ---- ranking evaluation (tg_rank_stats / tg_rank_stats_host) --------------------------------------------------------------
def new_rank_acc(device) -> Tuple[Tensor, Tensor]:
    """zeroed accumulators of one ranking pass: float64 [1 + TG_RANK_MAX_K] = {sum 1/rank, sum [rank <= k] per cut-off},
    int64 [2] = {events, non-finite scores}"""
    return (torch.zeros(1 + _lib.TG_RANK_MAX_K, dtype=torch.float64, device=device),
            torch.zeros(2, dtype=torch.int64, device=device))


def rank_stats(scores: Tensor, cand_ids: Tensor, dst: Tensor, *, mask: Optional[Tensor] = None, ks=(1, 3, 10), acc=None):
    """Rank of column 0 of scores [B, 1 + C] among the candidates left in (tiger_hip.h: tg_rank_stats): candidate j is left
    out when cand_ids[i, j] == dst[i], when it is the padding id 0, or when mask[i, j - 1] is false (mask: [B, C]).
    -> dict(n_greater, n_equal, n_valid: int32 [B]; rank: float64 [B]; acc: the (float64, int64) accumulators of
    `new_rank_acc`, to which this batch was added - pass them back in to fold a whole split).  Device tensors take the
    device entry, host tensors the host twin: same arithmetic."""
    dev = scores.device
    scores = scores.float().contiguous()
    B, C1 = scores.shape
    cand_ids, dst = _i64(cand_ids.to(dev)), _i64(dst.to(dev))
    if cand_ids.shape != (B, C1) or dst.shape != (B,):
        raise ValueError(f'rank_stats: scores {tuple(scores.shape)}, cand_ids {tuple(cand_ids.shape)}, dst {tuple(dst.shape)}')
    if mask is not None:
        mask = mask.to(dev).to(torch.uint8).contiguous()
        if mask.shape != (B, C1 - 1):
            raise ValueError(f'rank_stats: mask {tuple(mask.shape)} for {C1 - 1} candidates of {B} events')
    ks = [int(k) for k in ks]
    if len(ks) > _lib.TG_RANK_MAX_K or any(k < 1 for k in ks):
        raise ValueError(f'rank_stats: at most {_lib.TG_RANK_MAX_K} positive cut-offs')
    ks_host = torch.tensor(ks, dtype=torch.int32)
    acc = new_rank_acc(dev) if acc is None else acc
    i32 = dict(dtype=torch.int32, device=dev)
    out = dict(n_greater=torch.zeros(B, **i32), n_equal=torch.zeros(B, **i32), n_valid=torch.zeros(B, **i32),
               rank=torch.ones(B, dtype=torch.float64, device=dev), acc=acc)
    args = (B, C1 - 1, ptr(scores), ptr(cand_ids), ptr(dst), ptr(mask), len(ks), ptr(ks_host), ptr(out['n_greater']),
            ptr(out['n_equal']), ptr(out['n_valid']), ptr(out['rank']), ptr(acc[0]), ptr(acc[1]))
    if dev.type == 'cpu':
        check(lib.tg_rank_stats_host(*args), 'tg_rank_stats_host')
    else:
        check(lib.tg_rank_stats(*args, stream_ptr(dev)), 'tg_rank_stats')
    return out


def rank_metrics(acc, ks=(1, 3, 10)) -> dict:
    """One read-back of a pass's accumulators -> dict(mrr, hits {k: value}, n_events).  A non-finite score among the
    ranked ones raises ValueError."""
    f, i = acc[0].cpu(), acc[1].cpu()
    n, bad = int(i[0]), int(i[1])
    if bad:
        raise ValueError(f'Input contains {bad} non-finite scores.')
    nan = float('nan')
    return dict(mrr=float(f[0]) / n if n else nan, hits={int(k): (float(f[1 + q]) / n if n else nan) for q, k in enumerate(ks)},
                n_events=n)


# ---- top-k recommendation (tg_topk_rows / tg_seen_mask and their host twins) ----------------------------------------------
def topk_rows(scores: Tensor, cand_ids: Tensor, k: int, *, mask: Optional[Tensor] = None, n_seg: int = 0, acc=None) -> dict:
    """The k best columns of every row of scores [B, C] (tiger_hip.h: tg_topk_rows).  cand_ids: int64 [B, C], or [C] shared
    by all rows.  A column is left out when its id is the padding id 0, when mask[i, j] is false (mask: [B, C]) or when
    its score is not finite (counted).  Order: higher float32 score first, equal scores (-0.0 == +0.0) by ascending column.
    -> dict(ids int64 [B, k], scores float32 [B, k], cols int32 [B, k]; n_valid int32 [B]; n_nonfinite int64 [1], the
    accumulator `acc` when given - pass it back in to count over a whole pass).  Positions past min(k, n_valid) hold id 0,
    score -inf, column -1.  n_seg: column segments per row (0: the library chooses); the result does not depend on it.
    scores may be a view with a row stride above C.  Device tensors take the device entry, host tensors the host twin."""
    dev = scores.device
    if scores.dim() != 2 or scores.dtype != torch.float32:
        raise ValueError('topk_rows: scores is float32 [B, C]')
    if scores.numel() and scores.stride(1) != 1:
        scores = scores.contiguous()
    B, C = scores.shape
    ld = scores.stride(0) if B > 1 and C > 0 else C
    if ld < C:
        scores, ld = scores.contiguous(), C
    cand_ids = _i64(cand_ids.to(dev))
    shared = cand_ids.dim() == 1
    if cand_ids.shape != ((C,) if shared else (B, C)):
        raise ValueError(f'topk_rows: scores {tuple(scores.shape)}, cand_ids {tuple(cand_ids.shape)}')
    if mask is not None:
        mask = mask.to(dev).to(torch.uint8).contiguous()
        if mask.shape != (B, C):
            raise ValueError(f'topk_rows: mask {tuple(mask.shape)} for scores {tuple(scores.shape)}')
    k, n_seg = int(k), int(n_seg)
    if not 1 <= k <= _lib.TG_TOPK_MAX_K:
        raise ValueError(f'topk_rows: 1 <= k <= {_lib.TG_TOPK_MAX_K}')
    if n_seg < 0:
        raise ValueError('topk_rows: n_seg is 0 (chosen by the library) or positive')
    acc = torch.zeros(1, dtype=torch.int64, device=dev) if acc is None else acc
    out = dict(ids=torch.empty(B, k, dtype=torch.int64, device=dev), scores=torch.empty(B, k, dtype=torch.float32, device=dev),
               cols=torch.empty(B, k, dtype=torch.int32, device=dev), n_valid=torch.empty(B, dtype=torch.int32, device=dev),
               n_nonfinite=acc)
    args = (B, C, k, ptr(scores), ld, ptr(cand_ids), 1 if shared else 0, ptr(mask), n_seg, ptr(out['ids']),
            ptr(out['scores']), ptr(out['cols']), ptr(out['n_valid']), ptr(acc))
    if dev.type == 'cpu':
        check(lib.tg_topk_rows_host(*args), 'tg_topk_rows_host')
    else:
        nbytes = int(lib.tg_topk_rows_workspace_bytes(B, C, k, n_seg))
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
        check(lib.tg_topk_rows(*args, ptr(ws), ws.numel(), stream_ptr(dev)), 'tg_topk_rows')
    return out


def _rows_f32(t: Tensor, what: str) -> Tuple[Tensor, int]:
    """float32 [n, d] with unit column stride -> (tensor, row stride in floats); a view with a larger row stride is kept"""
    if t.dim() != 2 or t.dtype != torch.float32:
        raise ValueError(f'knn_rows: {what} is float32 [n, d]')
    n, d = t.shape
    if n * d and t.stride(1) != 1:
        t = t.contiguous()
    ld = t.stride(0) if n > 1 and d > 0 else d
    if ld < d:
        t, ld = t.contiguous(), d
    return t, ld


def knn_rows(q: Tensor, c: Tensor, k: int, *, ids: Optional[Tensor] = None, q_scale: Optional[Tensor] = None,
             c_scale: Optional[Tensor] = None, exclude: Optional[Tensor] = None, col_mask: Optional[Tensor] = None,
             n_split: int = 0, acc=None, _scores_out: Optional[Tensor] = None) -> dict:
    """The k nearest rows of c [C, d] for every row of q [Q, d] by inner product (tiger_hip.h: tg_knn_rows); the [Q, C]
    score matrix is never formed.  Score: the float32 fmaf chain over d, k ascending, then `* q_scale[i]`, then
    `* c_scale[j]` when given (cosine: pass reciprocal norms).  ids: int64 [C], the id of column j (None: j + 1); exclude:
    int64 [Q], an id left out of row i; col_mask: bool [C], false = left out for every row.  Id 0 and non-finite scores
    (counted) are left out as in topk_rows, whose order and padding these are.
    -> dict(ids int64 [Q, k], scores float32 [Q, k], cols int32 [Q, k]; n_valid int32 [Q]; n_nonfinite int64 [1], the
    accumulator `acc` when given).  n_split: catalogue splits per query tile (0: the library chooses); the result does not
    depend on it.  q and c may be views with a row stride above d.  Device tensors take the device entry, host tensors the
    host twin (`_scores_out`: float32 [Q, C] host tensor that receives the twin's full matrix, for tests).  ValueError for
    what the C entry refuses and for tensors on different devices."""
    dev = q.device
    q, ldq = _rows_f32(q, 'q')
    c, ldc = _rows_f32(c, 'c')
    (Q, d), C = q.shape, c.shape[0]
    if c.shape[1] != d:
        raise ValueError(f'knn_rows: q {tuple(q.shape)}, c {tuple(c.shape)}')
    if d == 0 or d % 4 or d > 512:
        raise ValueError('knn_rows: d is a positive multiple of 4, at most 512')
    k, n_split = int(k), int(n_split)
    if not 1 <= k <= _lib.TG_TOPK_MAX_K:
        raise ValueError(f'knn_rows: 1 <= k <= {_lib.TG_TOPK_MAX_K}')
    if n_split < 0:
        raise ValueError('knn_rows: n_split is 0 (chosen by the library) or positive')
    if C >= 1 << 31:
        raise ValueError('knn_rows: C < 2^31')

    def vec(t, n, dtype, what):
        if t is None:
            return None
        if t.device != dev:
            raise ValueError(f'knn_rows: {what} on {t.device}, q on {dev}')
        if t.dtype == torch.bool and dtype == torch.uint8:
            t = t.to(torch.uint8)
        if t.dtype != dtype or t.shape != (n,):
            raise ValueError(f'knn_rows: {what} is {dtype} [{n}], got {t.dtype} {tuple(t.shape)}')
        return t.contiguous()

    if c.device != dev:
        raise ValueError(f'knn_rows: c on {c.device}, q on {dev}')
    ids = vec(ids, C, torch.int64, 'ids')
    q_scale = vec(q_scale, Q, torch.float32, 'q_scale')
    c_scale = vec(c_scale, C, torch.float32, 'c_scale')
    exclude = vec(exclude, Q, torch.int64, 'exclude')
    col_mask = vec(col_mask, C, torch.uint8, 'col_mask')
    if acc is None:
        acc = torch.zeros(1, dtype=torch.int64, device=dev)
    elif acc.device != dev or acc.dtype != torch.int64:
        raise ValueError('knn_rows: acc is an int64 tensor on the device of q')
    out = dict(ids=torch.empty(Q, k, dtype=torch.int64, device=dev), scores=torch.empty(Q, k, dtype=torch.float32, device=dev),
               cols=torch.empty(Q, k, dtype=torch.int32, device=dev), n_valid=torch.empty(Q, dtype=torch.int32, device=dev),
               n_nonfinite=acc)
    args = (Q, C, d, k, ptr(q), ldq, ptr(c), ldc, ptr(ids), ptr(q_scale), ptr(c_scale), ptr(exclude), ptr(col_mask), n_split,
            ptr(out['ids']), ptr(out['scores']), ptr(out['cols']), ptr(out['n_valid']), ptr(acc))
    if dev.type == 'cpu':
        if _scores_out is not None and (_scores_out.dtype != torch.float32 or _scores_out.shape != (Q, C)
                                        or not _scores_out.is_contiguous() or _scores_out.device != dev):
            raise ValueError('knn_rows: _scores_out is a contiguous float32 [Q, C] host tensor')
        check(lib.tg_knn_rows_host(*args, ptr(_scores_out)), 'tg_knn_rows_host')
    else:
        if _scores_out is not None:
            raise ValueError('knn_rows: the device entry never forms the score matrix')
        nbytes = int(lib.tg_knn_rows_workspace_bytes(Q, C, k, n_split))
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
        check(lib.tg_knn_rows(*args, ptr(ws), ws.numel(), stream_ptr(dev)), 'tg_knn_rows')
    return out


def catalogue_index(cand: Tensor, n_nodes: int) -> Tensor:
    """int32 [n_nodes] on cand's device: the column of every node id in the shared catalogue cand [C], -1 for a node that
    is not in it (the `col_of` of seen_mask).  ValueError for an id outside [0, n_nodes) or listed twice."""
    cand = _i64(torch.as_tensor(cand)).reshape(-1)
    C = cand.numel()
    if C and (int(cand.min()) < 0 or int(cand.max()) >= n_nodes):
        raise ValueError('catalogue_index: a node id outside [0, n_nodes)')
    if C and int(torch.bincount(cand, minlength=1).max()) > 1:
        raise ValueError('catalogue_index: duplicate node ids in the catalogue')
    col_of = torch.full((int(n_nodes),), -1, dtype=torch.int32, device=cand.device)
    col_of[cand] = torch.arange(C, dtype=torch.int32, device=cand.device)
    return col_of


def seen_mask(graph, src: Tensor, ts: Tensor, col_of: Tensor, C: int, mask: Optional[Tensor] = None) -> Tensor:
    """bool [B, C]: false where column c of the catalogue is a node src[i] has an edge with (either direction) before
    ts[i] - strict float64, the sampler's cut (tiger_hip.h: tg_seen_mask) - or where the caller's `mask` already was.
    col_of: `catalogue_index(cand, graph.num_node)`.  Device tensors take the device entry over graph.tcsr, host tensors
    the host twin over the graph's host arrays.  ValueError for a source outside [0, num_node)."""
    import ctypes as C_
    dev = src.device
    src = _i64(src).reshape(-1)
    B, C = src.numel(), int(C)
    ts = ts.to(dev).double().contiguous().reshape(-1)
    col_of = col_of.to(dev).contiguous()
    if ts.numel() != B or col_of.dtype != torch.int32 or col_of.numel() != graph.num_node:
        raise ValueError(f'seen_mask: {B} sources, ts {tuple(ts.shape)}, col_of {col_of.dtype} {tuple(col_of.shape)} '
                         f'for {graph.num_node} nodes')
    if B and (int(src.min()) < 0 or int(src.max()) >= graph.num_node):
        raise ValueError('seen_mask: a source id outside [0, num_node)')
    if mask is None:
        m8 = torch.ones(B, C, dtype=torch.uint8, device=dev)
    else:
        if mask.shape != (B, C):
            raise ValueError(f'seen_mask: mask {tuple(mask.shape)} for {B} sources and {C} columns')
        m8 = mask.to(dev).ne(0).to(torch.uint8).contiguous()  # (a fresh buffer: the caller's mask is not written)
    if dev.type == 'cpu':
        h = graph._host_tcsr()
        tc = _lib.TgTcsr(graph.num_node, len(h[1]), *(ptr(a) for a in h))
        check(lib.tg_seen_mask_host(C_.byref(tc), B, ptr(src), ptr(ts), C, ptr(col_of), ptr(m8)), 'tg_seen_mask_host')
    else:
        gd = graph.device
        if gd.type != dev.type or (gd.index is not None and dev.index is not None and gd.index != dev.index):
            raise ValueError(f'seen_mask: the graph lives on {graph.device}, the queries on {dev}')
        check(lib.tg_seen_mask(C_.byref(graph.tcsr), B, ptr(src), ptr(ts), C, ptr(col_of), ptr(m8), stream_ptr(dev)),
              'tg_seen_mask')
    return m8.bool()


# ---- involved list (tg_involved_list and its host twin) -------------------------------------------------------------------
_STRATEGY_CODE = {'recent_edges': 0, 'recent_nodes': 1, 'uniform': 2}


def involved_list(graph, nids: Tensor, ts: Tensor, n_neighbors: int, n_layers: int, uptodate: Tensor, *,
                  strategy: Optional[str] = None) -> dict:
    """The nodes the embeddings of the (nids[q], ts[q]) queries will read - the set GraphCollator.collate_memory_nodes
    flags: the queries, their sampled neighbours and, with n_layers == 2, the neighbours' neighbours - that are not in
    `uptodate` yet (tiger_hip.h: tg_involved_list; no slot array is written).  uptodate: a bitmap of `new_bitmap` over
    graph.num_node ids, ORed with the whole set IN PLACE.  -> dict(ids int64 [cap]: the listed ids ascending in
    ids[:count], count int32 [1], tmin float32 [1] = the earliest query time); nothing is read back.  strategy: the graph's
    own by default; 'uniform' is refused.  Device tensors take the device entry over graph.tcsr, host tensors the host
    twin over the graph's host arrays.  ValueError for an id outside [0, num_node)."""
    import ctypes as C_
    dev = nids.device
    nids = _i64(nids).reshape(-1)
    Q, K, L = nids.numel(), int(n_neighbors), int(n_layers)
    ts = ts.to(dev).double().contiguous().reshape(-1)
    strategy = graph.strategy if strategy is None else strategy
    if strategy not in _STRATEGY_CODE:
        raise NotImplementedError(strategy)
    if strategy == 'uniform':
        raise NotImplementedError("involved_list: strategy='uniform' would make the set depend on the graph's random stream")
    n_nodes = graph.num_node
    if (ts.numel() != Q or uptodate.dtype != torch.int64 or uptodate.numel() != bitmap_words(n_nodes)
            or uptodate.device != dev or not uptodate.is_contiguous()):
        raise ValueError(f'involved_list: {Q} queries, ts {tuple(ts.shape)}, uptodate {uptodate.dtype} {tuple(uptodate.shape)} '
                         f'on {uptodate.device} for {n_nodes} nodes on {dev}')
    if not 1 <= K <= _lib.TG_INVOLVED_MAX_K or L not in (1, 2):
        raise ValueError(f'involved_list: 1 <= n_neighbors <= {_lib.TG_INVOLVED_MAX_K}, n_layers 1 or 2')
    if Q and (int(nids.min()) < 0 or int(nids.max()) >= n_nodes):
        raise ValueError('involved_list: a node id outside [0, num_node)')
    cap = min(Q * (1 + K + (K * K if L == 2 else 0)), n_nodes)
    out = dict(ids=torch.empty(max(cap, 1), dtype=torch.int64, device=dev), count=torch.zeros(1, dtype=torch.int32, device=dev),
               tmin=torch.zeros(1, dtype=torch.float32, device=dev))
    args = (Q, ptr(nids), ptr(ts), K, L, _STRATEGY_CODE[strategy], ptr(uptodate), cap, ptr(out['ids']), ptr(out['count']),
            ptr(out['tmin']))
    if dev.type == 'cpu':
        h = graph._host_tcsr()
        tc = _lib.TgTcsr(n_nodes, len(h[1]), *(ptr(a) for a in h))
        check(lib.tg_involved_list_host(C_.byref(tc), *args), 'tg_involved_list_host')
    else:
        gd = graph.device
        if gd.type != dev.type or (gd.index is not None and dev.index is not None and gd.index != dev.index):
            raise ValueError(f'involved_list: the graph lives on {graph.device}, the queries on {dev}')
        nbytes = int(lib.tg_involved_list_workspace_bytes(n_nodes, Q, K, L))
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
        check(lib.tg_involved_list(C_.byref(graph.tcsr), *args, ptr(ws), ws.numel(), stream_ptr(dev)), 'tg_involved_list')
    return out


# ---- incremental catalogue refresh (tg_snapshot_refresh.hip and its host twins) --------------------------------------------
def _graph_tcsr(what: str, graph, dev):
    """the tg_tcsr of `graph` for tensors on `dev`: host arrays for the cpu, graph.tcsr on the graph's own device"""
    if dev.type == 'cpu':
        h = graph._host_tcsr()
        return _lib.TgTcsr(graph.num_node, len(h[1]), *(ptr(a) for a in h)), h
    gd = graph.device
    if gd is None or gd.type != dev.type or (gd.index is not None and dev.index is not None and gd.index != dev.index):
        raise ValueError(f'{what}: the graph lives on {gd}, the tensors on {dev}')
    return graph.tcsr, None


def catalogue_dirty(graph, ids: Tensor, t_row, n_neighbors: int, n_layers: int, touched: Tensor, t_new: float, *,
                    max_age: Optional[float] = None, strategy: Optional[str] = None, check_ids: bool = True) -> dict:
    """Which rows of a catalogue read a changed node (tiger_hip.h: tg_catalogue_dirty)?  Row j - the query (ids[j],
    t_row[j]); t_row a float64 [C] tensor, or ONE float for all rows - is dirty iff a node of its involved set (that of
    `involved_list` for the one query) has its bit in `touched` (a `new_bitmap` over graph.num_node ids), or max_age is
    given and t_new - t_row[j] > max_age.  -> dict(rank int32 [C]: position among the dirty rows or -1, cols int32 [C]:
    the dirty rows ascending in cols[:count[0]], count int32 [2]: n_dirty and the rows dirty by age alone); nothing is
    read back - but for the ids' range check (two values; check_ids=False for ids the caller has checked already, as
    those of a CatalogueSnapshot).  Device tensors take the device entry, host tensors the host twin.  ValueError for an
    id outside [0, num_node), C >= 2^31, a NaN t_new, a negative or NaN max_age."""
    dev = ids.device
    ids = _i64(ids).reshape(-1)
    Cn, K, L = ids.numel(), int(n_neighbors), int(n_layers)
    strategy = graph.strategy if strategy is None else strategy
    if strategy not in _STRATEGY_CODE:
        raise NotImplementedError(strategy)
    if strategy == 'uniform':
        raise NotImplementedError("catalogue_dirty: strategy='uniform' would make the set depend on the graph's random stream")
    n_nodes = graph.num_node
    t_all = 0.0
    if torch.is_tensor(t_row):
        t_row = t_row.to(dev).double().contiguous().reshape(-1)
        if t_row.numel() != Cn:
            raise ValueError(f'catalogue_dirty: {Cn} rows, t_row {tuple(t_row.shape)}')
    else:
        t_all, t_row = float(t_row), None
    t_new = float(t_new)
    age = float('nan') if max_age is None else float(max_age)
    if Cn >= 2 ** 31 or t_new != t_new or t_all != t_all or (max_age is not None and not age >= 0.0):
        raise ValueError(f'catalogue_dirty: C = {Cn} (< 2^31), t_new = {t_new}, t_row = {t_all}, max_age = {max_age} (>= 0)')
    if (touched.dtype != torch.int64 or touched.numel() != bitmap_words(n_nodes) or touched.device != dev
            or not touched.is_contiguous()):
        raise ValueError(f'catalogue_dirty: touched {touched.dtype} {tuple(touched.shape)} on {touched.device} for {n_nodes} '
                         f'nodes on {dev}')
    if not 1 <= K <= _lib.TG_INVOLVED_MAX_K or L not in (1, 2):
        raise ValueError(f'catalogue_dirty: 1 <= n_neighbors <= {_lib.TG_INVOLVED_MAX_K}, n_layers 1 or 2')
    if Cn and (check_ids or dev.type == 'cpu') and (int(ids.min()) < 0 or int(ids.max()) >= n_nodes):
        raise ValueError('catalogue_dirty: a node id outside [0, num_node)')
    out = dict(rank=torch.empty(max(Cn, 1), dtype=torch.int32, device=dev)[:Cn],
               cols=torch.empty(max(Cn, 1), dtype=torch.int32, device=dev)[:Cn],
               count=torch.zeros(2, dtype=torch.int32, device=dev))
    tc, keep = _graph_tcsr('catalogue_dirty', graph, dev)
    args = (Cn, ptr(ids), ptr(t_row), t_all, K, L, _STRATEGY_CODE[strategy], ptr(touched), t_new, age, ptr(out['rank']),
            ptr(out['cols']), ptr(out['count']))
    if dev.type == 'cpu':
        check(lib.tg_catalogue_dirty_host(C_.byref(tc), *args), 'tg_catalogue_dirty_host')
    else:
        ws = torch.empty(int(lib.tg_catalogue_dirty_workspace_bytes(Cn)), dtype=torch.uint8, device=dev)
        check(lib.tg_catalogue_dirty(C_.byref(tc), *args, ptr(ws), ws.numel(), stream_ptr(dev)), 'tg_catalogue_dirty')
    return out


def catalogue_merge(rank: Tensor, n_new: int, h_old: Tensor, h_new: Tensor, t_old, t_new: float, *,
                    P_old: Optional[Tensor] = None, P_new: Optional[Tensor] = None, nb_old: Optional[Tensor] = None,
                    nb_new: Optional[Tensor] = None):
    """The row tables of a refreshed snapshot in one launch (tiger_hip.h: tg_catalogue_merge): out[j] = new[rank[j]] where
    rank[j] >= 0, else old[j] -> (h float32 [C, d], P float32 [C, d] or None, nb int64 [C, K] or None, t_row float64 [C]).
    rank int32 [C] (catalogue_dirty); *_new hold n_new rows; t_old: a float64 [C] tensor or ONE float for all old rows; new
    rows get t_new.  P and nb take part when both their tables are given.  ValueError for shapes that do not fit."""
    dev = rank.device
    Cn, n_new = rank.numel(), int(n_new)
    d = int(h_old.shape[1])

    def table(name, old, new, dtype, width):
        if (old is None) != (new is None):
            raise ValueError(f'catalogue_merge: {name}_old and {name}_new come together')
        if old is None:
            return None, None, None
        for what, x, rows in (('old', old, Cn), ('new', new, n_new)):
            if x.dtype != dtype or x.dim() != 2 or x.shape[0] < rows or x.shape[1] != width or x.device != dev:
                raise ValueError(f'catalogue_merge: {name}_{what} {x.dtype} {tuple(x.shape)} on {x.device}; wanted {dtype} '
                                 f'[>= {rows}, {width}] on {dev}')
        return old.contiguous(), new.contiguous(), torch.empty(Cn, width, dtype=dtype, device=dev)

    if rank.dtype != torch.int32 or rank.dim() != 1 or not 0 <= n_new <= Cn or d < 4 or d % 4:
        raise ValueError(f'catalogue_merge: rank {rank.dtype} {tuple(rank.shape)}, n_new {n_new}, d {d} (a multiple of 4)')
    rank = rank.contiguous()
    h_old, h_new, h_out = table('h', h_old, h_new, torch.float32, d)
    P_old, P_new, P_out = table('P', P_old, P_new, torch.float32, d)
    K = int(nb_old.shape[1]) if nb_old is not None else 0
    nb_old, nb_new, nb_out = table('nb', nb_old, nb_new, torch.int64, K)
    t_all = 0.0
    if torch.is_tensor(t_old):
        t_old = t_old.to(dev).double().contiguous().reshape(-1)
        if t_old.numel() != Cn:
            raise ValueError(f'catalogue_merge: {Cn} rows, t_old {tuple(t_old.shape)}')
    else:
        t_all, t_old = float(t_old), None
    t_out = torch.empty(Cn, dtype=torch.float64, device=dev)
    args = (Cn, n_new, d, K, ptr(rank), ptr(h_old), ptr(h_new), ptr(h_out), ptr(P_old), ptr(P_new), ptr(P_out), ptr(nb_old),
            ptr(nb_new), ptr(nb_out), ptr(t_old), t_all, float(t_new), ptr(t_out))
    if dev.type == 'cpu':
        check(lib.tg_catalogue_merge_host(*args), 'tg_catalogue_merge_host')
    else:
        check(lib.tg_catalogue_merge(*args, stream_ptr(dev)), 'tg_catalogue_merge')
    return h_out, P_out, nb_out, t_out


def bitmap_mark_degree_diff(graph_a, graph_b, bits: Tensor):
    """bits |= the ids whose T-CSR row length differs between the two graphs, an id present in only one of them counting
    with length 0 there (tiger_hip.h: tg_bitmap_mark_degree_diff).  bits: a `new_bitmap` over max(num_node) ids, IN
    PLACE; a host tensor takes the host twin over the graphs' host arrays."""
    dev = bits.device
    W = bitmap_words(max(graph_a.num_node, graph_b.num_node))
    if bits.dtype != torch.int64 or bits.dim() != 1 or bits.numel() < W or not bits.is_contiguous():
        raise ValueError(f'bitmap_mark_degree_diff: bits {bits.dtype} {tuple(bits.shape)}; wanted an int64 bitmap of at least '
                         f'{W} words')
    ta, keep_a = _graph_tcsr('bitmap_mark_degree_diff', graph_a, dev)
    tb, keep_b = _graph_tcsr('bitmap_mark_degree_diff', graph_b, dev)
    if dev.type == 'cpu':
        check(lib.tg_bitmap_mark_degree_diff_host(C_.byref(ta), C_.byref(tb), ptr(bits), bits.numel()),
              'tg_bitmap_mark_degree_diff_host')
    else:
        check(lib.tg_bitmap_mark_degree_diff(C_.byref(ta), C_.byref(tb), ptr(bits), bits.numel(), stream_ptr(dev)),
              'tg_bitmap_mark_degree_diff')


# ---- walk candidates (tg_walk_candidates and its host twin) ----------------------------------------------------------------
def _walk_plan(what: str, C: int, fanout, take) -> Tuple[Tensor, int]:
    """the refusals of tg_walk_candidates that need no tensor, each with the cap it names -> (fanout int32 host, take bits)"""
    fanout = tuple(int(f) for f in fanout)
    take = tuple(bool(b) for b in take)
    L = len(fanout)
    if not 1 <= L <= 3:
        raise ValueError(f'{what}: fanout has 1 to 3 levels, not {L}')
    if len(take) != L:
        raise ValueError(f'{what}: take {take} does not match the {L} levels of fanout {fanout}')
    if not any(take):
        raise ValueError(f'{what}: take selects no level')
    if not take[-1]:
        raise ValueError(f'{what}: the last level of fanout {fanout} is not taken - a level walked for nothing')
    if any(not 1 <= f <= _lib.TG_WALK_MAX_FANOUT for f in fanout):
        raise ValueError(f'{what}: every fan-out lies in [1, TG_WALK_MAX_FANOUT = {_lib.TG_WALK_MAX_FANOUT}], not {fanout}')
    sizes = [fanout[0]]
    for f in fanout[1:]:
        sizes.append(sizes[-1] * f)
    if max(sizes[:2]) > _lib.TG_WALK_MAX_FRONTIER:
        raise ValueError(f'{what}: the expanded frontier of fanout {fanout} has {max(sizes[:2])} entries, above '
                         f'TG_WALK_MAX_FRONTIER = {_lib.TG_WALK_MAX_FRONTIER}')
    endpoints = sum(s for s, b in zip(sizes, take) if b)
    if endpoints > _lib.TG_WALK_MAX_ENDPOINTS:
        raise ValueError(f'{what}: the taken levels of fanout {fanout} hold {endpoints} endpoints, above '
                         f'TG_WALK_MAX_ENDPOINTS = {_lib.TG_WALK_MAX_ENDPOINTS}')
    if not 1 <= C <= _lib.TG_WALK_MAX_ENDPOINTS:
        raise ValueError(f'{what}: 1 <= C <= TG_WALK_MAX_ENDPOINTS = {_lib.TG_WALK_MAX_ENDPOINTS}, not {C}')
    return torch.tensor(fanout, dtype=torch.int32), sum(1 << l for l, b in enumerate(take) if b)


def walk_candidates(graph, src: Tensor, ts: Tensor, C: int, *, fanout=(10, 10, 10), take=(True, False, True),
                    exclude_seen: bool = False, keep_self: bool = False) -> dict:
    """Per-query candidates from the graph itself (tiger_hip.h: tg_walk_candidates): the nodes reached from src[i] by walks
    over each node's last fanout[l] entries before ts[i] - every hop cut at the query's own time, strict float64 -,
    weighted by the number of walks that end in them at the levels `take` selects (one bool per level of fanout).  Left
    out: node 0, the source itself unless keep_self, and with exclude_seen every node the source has any entry with
    before ts[i].  Order: higher weight first, equal weights by ascending id; the first C.  -> dict(ids int64 [B, C] and
    counts int32 [B, C], padded with 0; n_valid int32 [B] = min(C, n_distinct); n_distinct int32 [B], the candidates
    before truncation).  The default walks src -> item -> co-user -> item and takes levels 1 and 3.  `ids` is the
    per-query `cand` of TIGE.recommend.  Works on any Graph (the recent-edges rule whatever graph.strategy is).  Device
    tensors take the device entry over graph.tcsr, host tensors the host twin over the graph's host arrays.  ValueError,
    with the cap named, for what the C entry refuses; for a source outside [0, num_node); for tensors on a device other
    than the graph's."""
    import ctypes as C_
    dev = src.device
    src = _i64(src).reshape(-1)
    B, C = src.numel(), int(C)
    ts = ts.to(dev).double().contiguous().reshape(-1)
    fan, bits = _walk_plan('walk_candidates', C, fanout, take)
    if ts.numel() != B:
        raise ValueError(f'walk_candidates: {B} sources, ts {tuple(ts.shape)}')
    if B and (int(src.min()) < 0 or int(src.max()) >= graph.num_node):
        raise ValueError('walk_candidates: a source id outside [0, num_node)')
    flags = (_lib.TG_WALK_EXCLUDE_SEEN if exclude_seen else 0) | (_lib.TG_WALK_KEEP_SELF if keep_self else 0)
    out = dict(ids=torch.zeros(B, C, dtype=torch.int64, device=dev), counts=torch.zeros(B, C, dtype=torch.int32, device=dev),
               n_valid=torch.zeros(B, dtype=torch.int32, device=dev), n_distinct=torch.zeros(B, dtype=torch.int32, device=dev))
    args = (B, ptr(src), ptr(ts), len(fan), ptr(fan), bits, C, flags, ptr(out['ids']), ptr(out['counts']), ptr(out['n_valid']),
            ptr(out['n_distinct']))
    if dev.type == 'cpu':
        h = graph._host_tcsr()
        tc = _lib.TgTcsr(graph.num_node, len(h[1]), *(ptr(a) for a in h))
        check(lib.tg_walk_candidates_host(C_.byref(tc), *args), 'tg_walk_candidates_host')
    else:
        gd = graph.device
        if gd.type != dev.type or (gd.index is not None and dev.index is not None and gd.index != dev.index):
            raise ValueError(f'walk_candidates: the graph lives on {graph.device}, the queries on {dev}')
        check(lib.tg_walk_candidates(C_.byref(graph.tcsr), *args, stream_ptr(dev)), 'tg_walk_candidates')
    return out


# ---- trending candidates (tg_trending, tg_fill_candidates and their host twins) ---------------------------------------------
def _graph_struct(what: str, graph, dev):
    """the tg_tcsr a call on `dev` runs over: the host arrays for host tensors, graph.tcsr for tensors on the graph's device
    -> (struct, whatever keeps its arrays alive)"""
    if dev.type == 'cpu':
        h = graph._host_tcsr()
        return _lib.TgTcsr(graph.num_node, len(h[1]), *(ptr(a) for a in h)), h
    gd = graph.device
    if gd.type != dev.type or (gd.index is not None and dev.index is not None and gd.index != dev.index):
        raise ValueError(f'{what}: the graph lives on {graph.device}, the tensors on {dev}')
    return graph.tcsr, None


def trending(graph, t, T: int, *, window=None, among: Optional[Tensor] = None) -> dict:
    """The T most active nodes of a time window (tiger_hip.h: tg_trending): c(v) = the T-CSR entries of v with
    t - window <= time < t - strict float64 cuts, both edge directions, multi-edges counted; window=None: everything before
    t - over the ids of `among` (int64 [M], no id twice), or every node but 0.  Order: higher c first, equal c by ascending
    id; node 0 and nodes with c == 0 are never listed.  -> dict(ids int64 [T] and counts int32 [T], padded with 0; n_valid
    int32 [1] = min(T, n_distinct); n_distinct int32 [1]), on the device of `among` (the graph's without one); nothing is
    read back.  t_lo = t - window is computed in float64 on the host.  Device tensors take the device entry over graph.tcsr,
    host tensors the host twin over the graph's host arrays.  ValueError for T outside [1, TG_TREND_MAX], a window that is
    not positive, a NaN, an id of `among` listed twice or outside [0, num_node)."""
    import ctypes as C_
    import math
    T = int(T)
    if not 1 <= T <= _lib.TG_TREND_MAX:
        raise ValueError(f'trending: 1 <= T <= TG_TREND_MAX = {_lib.TG_TREND_MAX}, not {T}')
    t_hi = float(t)
    if math.isnan(t_hi):
        raise ValueError('trending: t is NaN')
    if window is None:
        t_lo = -math.inf
    else:
        window = float(window)
        if math.isnan(window) or not window > 0:
            raise ValueError(f'trending: window is positive (or None: everything before t), not {window}')
        t_lo = t_hi - window
    if among is None:
        dev, M = torch.device(graph.device), 0
    else:
        among = _i64(torch.as_tensor(among)).reshape(-1)
        dev, M = among.device, among.numel()
        try:
            catalogue_index(among, graph.num_node)   # no id twice, every id a node
        except ValueError as e:
            raise ValueError(str(e).replace('catalogue_index', 'trending: among').replace('the catalogue', 'among')) from None
        if M == 0:   # (an empty tensor has no address, and NULL means every node)
            among = torch.zeros(1, dtype=torch.int64, device=dev)
    tc, _keep = _graph_struct('trending', graph, dev)
    out = dict(ids=torch.zeros(T, dtype=torch.int64, device=dev), counts=torch.zeros(T, dtype=torch.int32, device=dev),
               n_valid=torch.zeros(1, dtype=torch.int32, device=dev), n_distinct=torch.zeros(1, dtype=torch.int32, device=dev))
    args = (C_.byref(tc), t_lo, t_hi, ptr(among), M, T, ptr(out['ids']), ptr(out['counts']), ptr(out['n_valid']),
            ptr(out['n_distinct']))
    if dev.type == 'cpu':
        check(lib.tg_trending_host(*args), 'tg_trending_host')
    else:
        nbytes = int(lib.tg_trending_workspace_bytes(graph.num_node if among is None else M, T))
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
        check(lib.tg_trending(*args, ptr(ws), ws.numel(), stream_ptr(dev)), 'tg_trending')
    return out


def fill_candidates(graph, src: Tensor, ts: Tensor, cand: dict, trend: dict, *, exclude_seen: bool = False,
                    keep_self: bool = False) -> dict:
    """Back-fill per-query candidate rows from a shared list (tiger_hip.h: tg_fill_candidates).  cand: a `walk_candidates`
    dict (ids / counts [B, C], n_valid [B]); trend: a `trending` dict (ids [T], n_valid [1]).  For every query the ids of
    trend['ids'][:n_valid] are appended in order behind the row's n_valid candidates until it holds C, leaving out id 0,
    the source unless keep_self, what the row already holds and, with exclude_seen, every node the source has any entry
    with before ts[i] - the walk's own rules; pass the walk's flags.  Appended columns get counts == 0 (a walk candidate
    has weight >= 1).  -> dict(ids, counts, n_valid: fresh tensors, the caller's are not written; n_distinct: cand's own,
    unchanged; n_filled int32 [B], the ids appended per query).  The list's length is read on the device: no
    synchronisation.  Device tensors take the device entry, host tensors the host twin.  ValueError for shapes or dtypes that
    do not fit, a source outside [0, num_node), tensors on different devices."""
    import ctypes as C_
    dev = src.device
    src = _i64(src).reshape(-1)
    B = src.numel()
    ts = ts.to(dev).double().contiguous().reshape(-1)
    for name in ('ids', 'counts', 'n_valid'):
        if name not in cand:
            raise ValueError(f"fill_candidates: cand is a walk_candidates dict; it has no '{name}'")
    if 'ids' not in trend or 'n_valid' not in trend:
        raise ValueError("fill_candidates: trend is a trending dict with 'ids' and 'n_valid'")
    ids, counts, n_valid = cand['ids'], cand['counts'], cand['n_valid']
    fill, n_fill = trend['ids'].contiguous(), trend['n_valid'].contiguous()
    if ids.dim() != 2 or ids.dtype != torch.int64 or counts.dtype != torch.int32 or n_valid.dtype != torch.int32:
        raise ValueError('fill_candidates: cand holds ids int64 [B, C], counts int32 [B, C], n_valid int32 [B]')
    C = ids.shape[1]
    if ts.numel() != B or ids.shape[0] != B or counts.shape != ids.shape or n_valid.shape != (B,):
        raise ValueError(f'fill_candidates: {B} sources, ts {tuple(ts.shape)}, ids {tuple(ids.shape)}, counts '
                         f'{tuple(counts.shape)}, n_valid {tuple(n_valid.shape)}')
    if not 1 <= C <= _lib.TG_WALK_MAX_ENDPOINTS:
        raise ValueError(f'fill_candidates: 1 <= C <= TG_WALK_MAX_ENDPOINTS = {_lib.TG_WALK_MAX_ENDPOINTS}, not {C}')
    if fill.dim() != 1 or fill.dtype != torch.int64 or n_fill.dtype != torch.int32 or n_fill.numel() != 1:
        raise ValueError('fill_candidates: trend holds ids int64 [T] and n_valid int32 [1]')
    T = fill.numel()
    if not 1 <= T <= _lib.TG_TREND_MAX:
        raise ValueError(f'fill_candidates: 1 <= T <= TG_TREND_MAX = {_lib.TG_TREND_MAX}, not {T}')
    if any(x.device != dev for x in (ids, counts, n_valid, fill, n_fill)):
        raise ValueError(f'fill_candidates: the sources live on {dev}, cand on {ids.device}, trend on {fill.device}')
    if B and (int(src.min()) < 0 or int(src.max()) >= graph.num_node):
        raise ValueError('fill_candidates: a source id outside [0, num_node)')
    flags = (_lib.TG_WALK_EXCLUDE_SEEN if exclude_seen else 0) | (_lib.TG_WALK_KEEP_SELF if keep_self else 0)
    tc, _keep = _graph_struct('fill_candidates', graph, dev)
    out = dict(ids=ids.clone(memory_format=torch.contiguous_format), counts=counts.clone(memory_format=torch.contiguous_format),
               n_valid=n_valid.clone(memory_format=torch.contiguous_format), n_filled=torch.zeros(B, dtype=torch.int32, device=dev))
    if 'n_distinct' in cand:
        out['n_distinct'] = cand['n_distinct']
    args = (C_.byref(tc), B, ptr(src), ptr(ts), C, ptr(out['ids']), ptr(out['counts']), ptr(out['n_valid']),
            ptr(fill), ptr(n_fill), T, flags, ptr(out['n_filled']))
    if dev.type == 'cpu':
        check(lib.tg_fill_candidates_host(*args), 'tg_fill_candidates_host')
    else:
        check(lib.tg_fill_candidates(*args, stream_ptr(dev)), 'tg_fill_candidates')
    return out


def _fill_plan(what: str, fill: dict) -> dict:
    """the refusals of a `fill=dict(T=..., window=..., among=..., t=...)` argument that need no tensor -> a checked copy"""
    import math
    if not isinstance(fill, dict):
        raise ValueError(f'{what}: fill is a dict(T=..., window=..., among=..., t=...)')
    fill = dict(fill)
    unknown = set(fill) - {'T', 'window', 'among', 't'}
    if unknown:
        raise ValueError(f'{what}: fill takes T, window, among and t, not {sorted(unknown)}')
    if 'T' not in fill:
        raise ValueError(f"{what}: fill needs 'T', the length of the trending list")
    T = int(fill['T'])
    if not 1 <= T <= _lib.TG_TREND_MAX:
        raise ValueError(f'{what}: fill: 1 <= T <= TG_TREND_MAX = {_lib.TG_TREND_MAX}, not {T}')
    window = fill.get('window')
    if window is not None:
        window = float(window)
        if math.isnan(window) or not window > 0:
            raise ValueError(f'{what}: fill: window is positive (or None: everything before t), not {window}')
    return dict(T=T, window=window, among=fill.get('among'), t=fill.get('t'))


# ---- releasing edge-feature rows (tg_edge_rows_plan / _apply and their host twin) -------------------------------------------
def _pin_ids(pin, dev) -> Optional[Tensor]:
    if pin is None:
        return None
    p = torch.as_tensor(pin).to(dev, torch.int64).contiguous().reshape(-1)
    return p if p.numel() else None


def edge_rows_plan(graph, n_rows: int, keep_from: Optional[int] = None, pin=None, device=None):
    """Which rows of an edge table of `n_rows` rows does `graph` still need (tiger_hip.h: tg_edge_rows_plan)?  Live: row 0,
    every row an entry names, rows >= keep_from (default n_rows: none), the ids of `pin`.  -> (remap int32 [n_rows]: the new
    row or -1, n_live, ws - the workspace `edge_rows_apply` wants back).  Reads ONE int64 back (n_live: what the packed
    table is allocated by); ValueError if an entry or a pin names no row of the table, or for a keep_from outside
    [0, n_rows]."""
    import ctypes as C_
    dev = torch.device(graph.device if device is None else device)
    if dev.type == 'cpu':
        raise ValueError('edge_rows_plan runs on the device (host arrays: edge_rows_host)')
    n_rows = int(n_rows)
    keep = n_rows if keep_from is None else int(keep_from)
    if n_rows < 1 or not 0 <= keep <= n_rows:
        raise ValueError(f'edge_rows_plan: keep_from = {keep} for a table of {n_rows} rows')
    g, _ = _graph_struct('edge_rows_plan', graph, dev)
    p = _pin_ids(pin, dev)
    remap = torch.empty(n_rows, dtype=torch.int32, device=dev)
    n_live = torch.empty(1, dtype=torch.int64, device=dev)
    nbytes = int(lib.tg_edge_rows_workspace_bytes(n_rows, g.num_entry))
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(lib.tg_edge_rows_plan(C_.byref(g), n_rows, keep, ptr(p), 0 if p is None else p.numel(), ptr(remap), ptr(n_live),
                                    ptr(ws), nbytes, stream_ptr(dev)), 'tg_edge_rows_plan')
        n = int(n_live)  # the one read-back
    if n < 0:
        raise ValueError(f'edge_rows_plan: an entry of the graph or a pinned id names no row of the table ({n_rows} rows)')
    return remap, n, ws


def edge_rows_apply(graph, table: Optional[Tensor], remap: Tensor, n_live: int, ws: Tensor,
                    table_out: Optional[Tensor] = None) -> Tuple[Optional[Tensor], Tensor]:
    """Pack the live rows of `table` and renumber the graph's eids (tiger_hip.h: tg_edge_rows_apply) with the remap and the
    workspace of `edge_rows_plan` -> (table_out [n_live, d_e], eid_out int32 [num_entry]).  table_out: a caller's buffer of
    at least n_live rows (a backing store with head-room) whose leading rows are written; allocated exactly otherwise.
    table=None renumbers the graph alone."""
    import ctypes as C_
    dev = remap.device
    g, _ = _graph_struct('edge_rows_apply', graph, dev)
    n_rows, n_live = remap.numel(), int(n_live)
    d_e = 0
    if table is not None:
        if (table.dim() != 2 or table.dtype != torch.float32 or not table.is_contiguous() or table.shape[0] != n_rows
                or table.device != dev or table.shape[1] % 4):
            raise ValueError(f'edge_rows_apply: table {table.dtype} {tuple(table.shape)} on {table.device} for a remap of '
                             f'{n_rows} rows on {dev} (float32, contiguous, d_e % 4 == 0)')
        d_e = table.shape[1]
        if table_out is None:
            table_out = torch.empty(n_live, d_e, dtype=torch.float32, device=dev)
        elif (table_out.dim() != 2 or table_out.dtype != torch.float32 or not table_out.is_contiguous()
              or table_out.shape[0] < n_live or table_out.shape[1] != d_e or table_out.device != dev):
            raise ValueError(f'edge_rows_apply: table_out {table_out.dtype} {tuple(table_out.shape)} for {n_live} rows of {d_e}')
    eid_out = torch.empty(g.num_entry, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(lib.tg_edge_rows_apply(C_.byref(g), ptr(table), n_rows, d_e, ptr(remap), n_live,
                                     ptr(table_out) if table is not None else None, ptr(eid_out), ptr(ws), ws.numel(),
                                     stream_ptr(dev)), 'tg_edge_rows_apply')
    return (table_out[:n_live] if table is not None else None), eid_out


def edge_rows_host(graph, table, n_rows: int, keep_from: Optional[int] = None, pin=None):
    """The host twin of plan + apply (tiger_hip.h: tg_edge_rows_host) over the graph's host arrays and a numpy table
    [n_rows, d_e] (or None) -> (remap int32 [n_rows], table_out [n_live, d_e] or None, eid_out int32 [num_entry]).
    ValueError as `edge_rows_plan`."""
    import ctypes as C_
    import numpy as np
    n_rows = int(n_rows)
    keep = n_rows if keep_from is None else int(keep_from)
    if n_rows < 1 or not 0 <= keep <= n_rows:
        raise ValueError(f'edge_rows_host: keep_from = {keep} for a table of {n_rows} rows')
    g, h = _graph_struct('edge_rows_host', graph, torch.device('cpu'))
    p = None if pin is None else np.ascontiguousarray(np.asarray(pin, dtype=np.int64).reshape(-1))
    d_e, t_out = 0, None
    if table is not None:
        table = np.ascontiguousarray(table, dtype=np.float32)
        if table.ndim != 2 or table.shape[0] != n_rows or table.shape[1] % 4 or table.shape[1] == 0:
            raise ValueError(f'edge_rows_host: table {table.shape} for {n_rows} rows (d_e % 4 == 0)')
        d_e = table.shape[1]
        t_out = np.empty((n_rows, d_e), dtype=np.float32)
    remap = np.empty(n_rows, dtype=np.int32)
    eid_out = np.empty(len(h[1]), dtype=np.int32)
    n_live = C_.c_int64(0)
    rc = lib.tg_edge_rows_host(C_.byref(g), ptr(table), n_rows, d_e, keep, ptr(p), 0 if p is None else len(p), ptr(remap),
                               ptr(t_out), ptr(eid_out), C_.byref(n_live))
    if rc == _lib.TG_EINVAL:
        raise ValueError(f'edge_rows_host: an entry of the graph or a pinned id names no row of the table ({n_rows} rows)')
    check(rc, 'tg_edge_rows_host')
    return remap, (None if t_out is None else t_out[:n_live.value].copy()), eid_out


# ---- T-CSR maintenance: the arrays, and plan / one read-back / exact allocation / apply (trim, erase) -------------------------
def tcsr_arrays(num_node: int, num_entry: int, device=None):
    """The four arrays of a T-CSR, uninitialised: (indptr int64 [num_node + 1], ts float64, nbr int32, eid int32 [num_entry])
    - tensors on `device`, numpy arrays without one."""
    if device is None:
        import numpy as np
        return (np.empty(num_node + 1, dtype=np.int64), np.empty(num_entry, dtype=np.float64),
                np.empty(num_entry, dtype=np.int32), np.empty(num_entry, dtype=np.int32))
    return (torch.empty(num_node + 1, dtype=torch.int64, device=device),) + _entry_arrays(num_entry, device)


def _entry_arrays(num_entry: int, device) -> Tuple[Tensor, Tensor, Tensor]:
    return (torch.empty(num_entry, dtype=torch.float64, device=device), torch.empty(num_entry, dtype=torch.int32, device=device),
            torch.empty(num_entry, dtype=torch.int32, device=device))


def _tcsr_plan(g, dev, workspace_bytes, plan):
    """plan = (name for `check`, fn(g, indptr_out, ws, ws_bytes, stream) -> rc), then the ONE read-back -> (indptr_out, kept, ws);
    this half and `_tcsr_apply` run under the caller's torch.cuda.device(dev) (`tcsr_compacted` holds one over both)"""
    indptr = torch.empty(g.num_node + 1, dtype=torch.int64, device=dev)
    nbytes = int(workspace_bytes(g))
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    check(plan[1](C_.byref(g), ptr(indptr), ptr(ws), nbytes, stream_ptr(dev)), plan[0])
    return indptr, int(indptr[-1]), ws


def _tcsr_apply(g, dev, indptr: Tensor, num_entry_out: int, ws: Tensor, apply) -> Tuple[Tensor, Tensor, Tensor]:
    """apply = (name, fn with the signature of tg_tcsr_trim_apply) into arrays of exactly num_entry_out entries -> (ts, nbr, eid)"""
    out = _entry_arrays(num_entry_out, dev)
    # (parent arrays and workspace belong to the caching allocator: reused in stream order, no wait needed)
    check(apply[1](C_.byref(g), ptr(indptr), num_entry_out, *(ptr(t) for t in out), ptr(ws), ws.numel(), stream_ptr(dev)), apply[0])
    return out


def tcsr_compacted(graph, workspace_bytes, plan, apply) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """A device-resident graph without some of its entries, on the current stream of the device its arrays live on:
    workspace_bytes(g), plan, ONE int64 read back (the kept entries), arrays allocated exactly, apply -> (indptr, ts, nbr, eid)."""
    g, dev = graph.tcsr, graph._dev[0].device
    with torch.cuda.device(dev):
        indptr, n, ws = _tcsr_plan(g, dev, workspace_bytes, plan)
        return (indptr,) + _tcsr_apply(g, dev, indptr, n, ws, apply)


def tcsr_compacted_host(graph, name: str, twin):
    """The host twin of `tcsr_compacted`: twin(g, indptr_out, ts_out, nbr_out, eid_out, num_entry_out) -> rc writes into
    full-size arrays over the graph's host arrays -> numpy (indptr, ts, nbr, eid) cut to the kept entries."""
    g, h = _graph_struct(name, graph, torch.device('cpu'))
    out = tcsr_arrays(graph.num_node, len(h[1]))
    kept = C_.c_int64(0)
    check(twin(C_.byref(g), *(ptr(a) for a in out), C_.byref(kept)), name)
    return (out[0],) + tuple(a[:kept.value].copy() for a in out[1:])  # (copies: the full-size arrays die)


# ---- late events (tg_tcsr_merge and its host twin) ----------------------------------------------------------------------------
def tcsr_merge(graph, batch, num_node_out: Optional[int] = None) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """The arrays of a device-resident `graph` merged with a batch in ANY order and with ANY non-NaN times (tiger_hip.h:
    tg_tcsr_merge) -> (indptr int64 [num_node_out + 1], ts float64, nbr int32, eid int32), on the current stream of the
    graph's device with allocator-owned buffers, no synchronisation.  batch = (src, dst, ts, eids): contiguous int64 /
    int64 / float64 / int64 tensors of one length ON THAT DEVICE, trusted as they are (Graph.merged validates)."""
    if graph._dev is None:
        graph._tensors()
    dev = graph._dev[0].device
    g, n = graph.tcsr, int(batch[0].numel())
    n_out = graph.num_node if num_node_out is None else int(num_node_out)
    want = (torch.int64, torch.int64, torch.float64, torch.int64)
    if any(b.dtype != dt or b.device != dev or b.numel() != n or not b.is_contiguous() for b, dt in zip(batch, want)):
        raise ValueError(f'tcsr_merge: the batch is four contiguous tensors (int64, int64, float64, int64) of one length on {dev}')
    out = tcsr_arrays(n_out, g.num_entry + 2 * n, dev)
    nbytes = int(lib.tg_tcsr_merge_workspace_bytes(g.num_entry, n, g.num_node, n_out))
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(lib.tg_tcsr_merge(C_.byref(g), n_out, n, *(ptr(b) for b in batch), *(ptr(t) for t in out), ptr(ws), nbytes,
                                stream_ptr(dev)), 'tg_tcsr_merge')
    return out


def tcsr_merge_host(graph, batch, num_node_out: Optional[int] = None):
    """The host twin (tiger_hip.h: tg_tcsr_merge_host) over the graph's host arrays and a batch of contiguous numpy arrays
    (int64, int64, float64, int64) -> numpy (indptr, ts, nbr, eid).  Ids, eids and NaN times are checked by the twin."""
    g, h = _graph_struct('tcsr_merge_host', graph, torch.device('cpu'))
    n = len(batch[0])
    n_out = graph.num_node if num_node_out is None else int(num_node_out)
    out = tcsr_arrays(n_out, len(h[1]) + 2 * n)
    check(lib.tg_tcsr_merge_host(C_.byref(g), n_out, n, *(ptr(b) for b in batch), *(ptr(a) for a in out)), 'tg_tcsr_merge_host')
    return out


# ---- erasing nodes and retracting events (tg_tcsr_erase_plan / _apply and their host twin) ----------------------------------
def host_bitmap(ids, n_ids: int):
    """The bitmap of `new_bitmap` + `bitmap_mark` over n_ids ids as a numpy int64 array (the host twins' format); ids at or
    beyond n_ids are not marked, duplicates are fine."""
    import numpy as np
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    ids = ids[(ids >= 0) & (ids < n_ids)]
    bits = np.zeros(bitmap_words(n_ids), dtype=np.uint64)
    np.bitwise_or.at(bits, ids >> 6, np.uint64(1) << (ids & 63).astype(np.uint64))
    return bits.view(np.int64)


def _erase_bits(what: str, bits: Optional[Tensor], n_ids: int, dev) -> Optional[Tensor]:
    if bits is None:
        return None
    if (not torch.is_tensor(bits) or bits.dtype != torch.int64 or bits.dim() != 1 or not bits.is_contiguous()
            or bits.numel() < bitmap_words(n_ids) or bits.device != dev):
        raise ValueError(f'{what}: a bitmap over {n_ids} ids is a contiguous int64 tensor of {bitmap_words(n_ids)} words on {dev}')
    return bits


def tcsr_erase_plan(graph, node_bits: Optional[Tensor] = None, eid_bits: Optional[Tensor] = None, n_rows: int = 0, device=None):
    """Which entries of `graph` survive the erasure of the nodes of `node_bits` and the retraction of the events of
    `eid_bits` (tiger_hip.h: tg_tcsr_erase_plan)?  node_bits: a `new_bitmap` over graph.num_node ids, eid_bits: one over
    n_rows ids (an eid at or beyond n_rows is never matched); None: nothing is matched by it.  -> (indptr_out int64
    [num_node + 1], the number of kept entries, ws - the workspace `tcsr_erase_apply` wants back).  Reads ONE int64 back
    (the kept entries: what the child's arrays are allocated by).  ValueError for a negative n_rows or a bitmap of another
    dtype, size or device."""
    dev = torch.device(graph.device if device is None else device)
    if dev.type == 'cpu':
        raise ValueError('tcsr_erase_plan runs on the device (host arrays: tcsr_erase_host)')
    n_rows = int(n_rows)
    if n_rows < 0:
        raise ValueError(f'tcsr_erase_plan: n_rows = {n_rows} is negative')
    g, _ = _graph_struct('tcsr_erase_plan', graph, dev)
    dev = graph._dev[0].device  # (with its index: what the bitmaps are compared with)
    node_bits = _erase_bits('tcsr_erase_plan: node_bits', node_bits, graph.num_node, dev)
    eid_bits = _erase_bits('tcsr_erase_plan: eid_bits', eid_bits, n_rows, dev)
    plan = lambda g, *out: lib.tg_tcsr_erase_plan(g, ptr(node_bits), ptr(eid_bits), n_rows, *out)
    with torch.cuda.device(dev):
        return _tcsr_plan(g, dev, lambda g: lib.tg_tcsr_erase_workspace_bytes(g.num_node, g.num_entry), ('tg_tcsr_erase_plan', plan))


def tcsr_erase_apply(graph, indptr_out: Tensor, num_entry_out: int, ws: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """Copy the kept entries of `graph` (tiger_hip.h: tg_tcsr_erase_apply) with the indptr and the workspace of
    `tcsr_erase_plan` -> (ts float64, nbr int32, eid int32), each of exactly num_entry_out entries."""
    dev = indptr_out.device
    g, _ = _graph_struct('tcsr_erase_apply', graph, dev)
    with torch.cuda.device(dev):
        return _tcsr_apply(g, dev, indptr_out, int(num_entry_out), ws, ('tg_tcsr_erase_apply', lib.tg_tcsr_erase_apply))


def tcsr_erase_host(graph, node_bits=None, eid_bits=None, n_rows: int = 0):
    """The host twin of plan + apply (tiger_hip.h: tg_tcsr_erase_host) over the graph's host arrays and numpy int64 bitmaps
    (`host_bitmap`) -> (indptr int64 [num_node + 1], ts float64, nbr int32, eid int32: numpy arrays of the kept entries).
    ValueError as `tcsr_erase_plan`."""
    import numpy as np
    n_rows = int(n_rows)
    if n_rows < 0:
        raise ValueError(f'tcsr_erase_host: n_rows = {n_rows} is negative')
    for what, bits, n in (('node_bits', node_bits, graph.num_node), ('eid_bits', eid_bits, n_rows)):
        if bits is not None and (not isinstance(bits, np.ndarray) or bits.dtype != np.int64 or bits.ndim != 1
                                 or not bits.flags.c_contiguous or len(bits) < bitmap_words(n)):
            raise ValueError(f'tcsr_erase_host: {what} over {n} ids is a contiguous numpy int64 array of {bitmap_words(n)} words')
    return tcsr_compacted_host(graph, 'tg_tcsr_erase_host',
                               lambda g, *out: lib.tg_tcsr_erase_host(g, ptr(node_bits), ptr(eid_bits), n_rows, *out))


# ---- is this a T-CSR the library may read? (tg_tcsr_verify and its host twin) -----------------------------------------------
TCSR_VERIFY_CLASSES = ('ENDS', 'PTR_ORDER', 'TS_ORDER', 'TS_NAN', 'NBR_RANGE', 'EID_RANGE')
_TCSR_VERIFY_WHAT = ('indptr[0] != 0 or indptr[num_node] != num_entry, at row bound {i}',
                     'indptr decreases after row {i}',
                     'the times of a row decrease at entry {i}',
                     'the time of entry {i} is NaN',
                     'the neighbour of entry {i} is no node id',
                     'the edge id of entry {i} is no row of the edge table')


def TCSR_VERIFY_TEXT(code: int, first=None) -> str:
    """The message of a non-zero tcsr_verify code: every violated class by name, with its smallest violating index."""
    parts = []
    for c, (name, what) in enumerate(zip(TCSR_VERIFY_CLASSES, _TCSR_VERIFY_WHAT)):
        if code >> c & 1:
            parts.append(f'{name}: ' + what.format(i=first[c] if first is not None else '?'))
    return 'no T-CSR the library may read - ' + '; '.join(parts) if parts else 'a T-CSR the library may read'


def _verify_arrays(what: str, arrays, is_np: bool):
    """four arrays of the T-CSR dtypes, 1-d, contiguous, ts / nbr / eid of one length -> (num_node, num_entry); ValueError"""
    import numpy as np
    if len(arrays) != 4:
        raise ValueError(f'{what}: a T-CSR is (indptr, ts, nbr, eid)')
    want = (np.int64, np.float64, np.int32, np.int32) if is_np else (torch.int64, torch.float64, torch.int32, torch.int32)
    for a, dt, name in zip(arrays, want, ('indptr', 'ts', 'nbr', 'eid')):
        ok = isinstance(a, np.ndarray) and a.flags.c_contiguous if is_np else torch.is_tensor(a) and a.is_contiguous()
        if not ok or a.dtype != dt or a.ndim != 1:
            raise ValueError(f'{what}: {name} must be a contiguous 1-d {"numpy array" if is_np else "tensor"} of {dt}')
    n, P = int(arrays[0].shape[0]) - 1, int(arrays[1].shape[0])
    if n < 1 or n > 0x7FFFFFFF or P > 0xFFFFFFFF:
        raise ValueError(f'{what}: num_node = {n}, num_entry = {P} is outside what a T-CSR holds')
    if int(arrays[2].shape[0]) != P or int(arrays[3].shape[0]) != P:
        raise ValueError(f'{what}: ts, nbr and eid must have one entry each ({P}, {arrays[2].shape[0]}, {arrays[3].shape[0]})')
    return n, P


def _verify_result(out8):
    import numpy as np
    w = [int(x) for x in out8]
    return w[0], w[1:7], float(np.array([w[7]], dtype=np.int64).view(np.float64)[0])


def tcsr_verify(arrays_or_graph, eid_rows: Optional[int] = None):
    """Is this a T-CSR the library may read (tiger_hip.h: tg_tcsr_verify)?  A Graph (its device arrays) or the four device
    tensors (indptr int64 [N + 1], ts float64, nbr int32, eid int32 [P]) -> (code, first[6], t_max): code = the OR of the
    violated classes (TCSR_VERIFY_CLASSES, bit c = class c; 0: clean), first[c] = the smallest violating index or -1, t_max
    = the largest non-NaN time (-inf without one).  eid_rows: the rows of the edge table (None: the eids are not checked).
    On the arrays' device and the current stream, ONE read-back of the 8 result words.  Safe on any array CONTENTS; dtypes,
    shapes and lengths are checked here (ValueError)."""
    if hasattr(arrays_or_graph, 'tcsr'):
        g, keep = arrays_or_graph.tcsr, arrays_or_graph._dev
        dev = keep[0].device
    else:
        keep = tuple(arrays_or_graph)
        n, P = _verify_arrays('tcsr_verify', keep, False)
        dev = keep[0].device
        if dev.type == 'cpu' or any(a.device != dev for a in keep):
            raise ValueError('tcsr_verify runs on the device the four arrays share (host arrays: tcsr_verify_host)')
        g = _lib.TgTcsr(n, P, *(ptr(a) for a in keep))
    rows = -1 if eid_rows is None else int(eid_rows)
    with torch.cuda.device(dev):
        out8 = torch.empty(8, dtype=torch.int64, device=dev)
        nbytes = int(lib.tg_tcsr_verify_workspace_bytes(g.num_entry, g.num_node))
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
        check(lib.tg_tcsr_verify(C_.byref(g), rows, ptr(out8), ptr(ws), nbytes, stream_ptr(dev)), 'tg_tcsr_verify')
        return _verify_result(out8.tolist())


def tcsr_verify_host(arrays_or_graph, eid_rows: Optional[int] = None):
    """`tcsr_verify` over numpy arrays (or a Graph's host view) with the host twin (tiger_hip.h: tg_tcsr_verify_host)."""
    import numpy as np
    if hasattr(arrays_or_graph, '_host_tcsr'):
        keep = arrays_or_graph._host_tcsr()
        n, P = arrays_or_graph.num_node, len(keep[1])
    else:
        keep = tuple(arrays_or_graph)
        n, P = _verify_arrays('tcsr_verify_host', keep, True)
    g = _lib.TgTcsr(n, P, *(ptr(a) for a in keep))
    out8 = np.empty(8, dtype=np.int64)
    check(lib.tg_tcsr_verify_host(C_.byref(g), -1 if eid_rows is None else int(eid_rows), ptr(out8)), 'tg_tcsr_verify_host')
    return _verify_result(out8)


# ---- the device id map: external int64 keys -> dense int32 ids (tg_idmap_* and their host twins) ---------------------------
IDMAP_EMPTY = _lib.TG_IDMAP_EMPTY
_IDMAP_CLASSES = ((_lib.TG_IDMAP_ERR_PROBE, 'PROBE: a probe ran through the whole table'),
                  (_lib.TG_IDMAP_ERR_DUP, 'DUP: the key stands in an earlier row too'),
                  (_lib.TG_IDMAP_ERR_EMPTY_KEY, 'EMPTY_KEY: INT64_MIN is the key of the padding id 0 alone'),
                  (_lib.TG_IDMAP_ERR_TABLE, 'TABLE: a slot holds no id of this map'),
                  (_lib.TG_IDMAP_ERR_FREE, 'FREE: the bitmap of free ids and key_of disagree'))


def IDMAP_ERR_TEXT(word: int) -> str:
    """The message of a non-zero tg_idmap error word: the classes by name and, from a rebuild, the smallest offending row."""
    word = int(word)
    names = '; '.join(text for bit, text in _IDMAP_CLASSES if word & bit)
    return names + (f', at row {0x7FFFFFFF - (word >> 8)} of key_of' if word >> 8 else '')


def idmap_tables(capacity: int, key_rows: int, device) -> Tuple[Tensor, Tensor, Tensor]:
    """an empty table of `capacity` slots and a reverse table of key_rows rows that holds the padding id alone"""
    slot_key = torch.full((capacity,), IDMAP_EMPTY, dtype=torch.int64, device=device)
    slot_id = torch.full((capacity,), -1, dtype=torch.int32, device=device)
    key_of = torch.full((key_rows,), IDMAP_EMPTY, dtype=torch.int64, device=device)
    return slot_key, slot_id, key_of


def _idmap_struct(what: str, tables, keys: Optional[Tensor] = None):
    slot_key, slot_id, key_of = tables
    dev = slot_key.device
    for t, dt, name in ((slot_key, torch.int64, 'slot_key'), (slot_id, torch.int32, 'slot_id'), (key_of, torch.int64, 'key_of')):
        if not torch.is_tensor(t) or t.dtype != dt or t.dim() != 1 or not t.is_contiguous() or t.device != dev:
            raise ValueError(f'{what}: {name} must be a contiguous 1-d tensor of {dt} on {dev}')
    if slot_id.numel() != slot_key.numel():
        raise ValueError(f'{what}: slot_key and slot_id must have one entry per slot')
    if keys is not None and not (torch.is_tensor(keys) and keys.dtype == torch.int64 and keys.dim() == 1
                                 and keys.is_contiguous() and keys.device == dev):
        raise ValueError(f'{what}: keys must be a contiguous 1-d int64 tensor on {dev}')
    return _lib.TgIdmap(slot_key.numel(), key_of.numel(), ptr(slot_key), ptr(slot_id), ptr(key_of)), dev


def idmap_lookup(tables, keys: Tensor) -> Tensor:
    """tiger_hip.h: tg_idmap_lookup (tables on the CPU: its host twin) -> ids int32 [n]: -1 for a key the map does not
    hold, 0 for INT64_MIN.  Read-only, no read-back."""
    m, dev = _idmap_struct('idmap_lookup', tables, keys)
    n = keys.numel()
    ids = torch.empty(n, dtype=torch.int32, device=dev)
    if dev.type == 'cpu':
        check(lib.tg_idmap_lookup_host(C_.byref(m), ptr(keys), n, ptr(ids)), 'tg_idmap_lookup_host')
    else:
        with torch.cuda.device(dev):
            check(lib.tg_idmap_lookup(C_.byref(m), ptr(keys), n, ptr(ids), stream_ptr(dev)), 'tg_idmap_lookup')
    return ids


def idmap_assign(tables, size: int, keys: Tensor) -> Tuple[Tensor, int, int]:
    """tiger_hip.h: tg_idmap_assign (tables on the CPU: its host twin) -> (ids int32 [n], new size, error word).  The tables
    are updated in place; ONE read-back, of the two result words.  The entry refuses a table that would pass half full or
    a key_of too short for size + n (TigerHipError): IdMap.assign grows first."""
    m, dev = _idmap_struct('idmap_assign', tables, keys)
    n = keys.numel()
    ids = torch.empty(n, dtype=torch.int32, device=dev)
    out2 = torch.empty(2, dtype=torch.int64, device=dev)
    if dev.type == 'cpu':
        check(lib.tg_idmap_assign_host(C_.byref(m), size, ptr(keys), n, ptr(ids), ptr(out2)), 'tg_idmap_assign_host')
    else:
        with torch.cuda.device(dev):
            nbytes = int(lib.tg_idmap_assign_workspace_bytes(n))
            ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
            check(lib.tg_idmap_assign(C_.byref(m), size, ptr(keys), n, ptr(ids), ptr(out2), ptr(ws), nbytes, stream_ptr(dev)),
                  'tg_idmap_assign')
    new_size, err = out2.tolist()
    return ids, int(new_size), int(err)


def idmap_rebuild(tables, size: int, read_back: bool = True):
    """tiger_hip.h: tg_idmap_rebuild (tables on the CPU: its host twin): fills the EMPTY table from key_of[1 .. size) -> the
    error word (0: clean; IDMAP_ERR_TEXT), or with read_back=False the two device words {size, error word} unread - a
    caller that knows its keys distinct (a growth) reads nothing."""
    m, dev = _idmap_struct('idmap_rebuild', tables)
    out2 = torch.empty(2, dtype=torch.int64, device=dev)
    if dev.type == 'cpu':
        check(lib.tg_idmap_rebuild_host(C_.byref(m), size, ptr(out2)), 'tg_idmap_rebuild_host')
    else:
        with torch.cuda.device(dev):
            check(lib.tg_idmap_rebuild(C_.byref(m), size, ptr(out2), stream_ptr(dev)), 'tg_idmap_rebuild')
    return int(out2[1].item()) if read_back else out2


# ---- removing keys and recycling dense ids (tg_idmap_remove / _assign_recycle / _rebuild_free and their host twins) --------
def idmap_free_bits(key_rows: int, device) -> Tensor:
    """the bitmap of free ids over key_rows dense ids, none free: 64-bit words (held as int64)"""
    return torch.zeros((int(key_rows) + 63) // 64, dtype=torch.int64, device=device)


def _idmap_bits(what: str, free_bits: Tensor, dev) -> Tensor:
    if not (torch.is_tensor(free_bits) and free_bits.dtype == torch.int64 and free_bits.dim() == 1
            and free_bits.is_contiguous() and free_bits.device == dev):
        raise ValueError(f'{what}: free_bits must be a contiguous 1-d int64 tensor on {dev}')
    return free_bits


def idmap_remove(tables, size: int, free_bits: Tensor, keys: Tensor) -> Tuple[Tensor, Tensor, int, int]:
    """tiger_hip.h: tg_idmap_remove (tables on the CPU: its host twin) -> (ids int32 [n]: the id each key had, -1 for a key
    the map does not hold, 0 for INT64_MIN; released int32 [n]: each released id at one position, INT32_MAX elsewhere; the
    number of distinct ids released; error bits).  Tables and bitmap are updated in place; ONE read-back."""
    m, dev = _idmap_struct('idmap_remove', tables, keys)
    _idmap_bits('idmap_remove', free_bits, dev)
    n = keys.numel()
    ids = torch.empty(n, dtype=torch.int32, device=dev)
    released = torch.empty(n, dtype=torch.int32, device=dev)
    out2 = torch.empty(2, dtype=torch.int64, device=dev)
    if dev.type == 'cpu':
        check(lib.tg_idmap_remove_host(C_.byref(m), size, ptr(free_bits), free_bits.numel(), ptr(keys), n, ptr(ids),
                                       ptr(released), ptr(out2)), 'tg_idmap_remove_host')
    else:
        with torch.cuda.device(dev):
            nbytes = int(lib.tg_idmap_remove_workspace_bytes(n))
            ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
            check(lib.tg_idmap_remove(C_.byref(m), size, ptr(free_bits), free_bits.numel(), ptr(keys), n, ptr(ids),
                                      ptr(released), ptr(out2), ptr(ws), nbytes, stream_ptr(dev)), 'tg_idmap_remove')
    n_released, err = out2.tolist()
    return ids, released, int(n_released), int(err)


def idmap_assign_recycle(tables, size: int, occupied: int, free_bits: Tensor, n_free: int,
                         keys: Tensor) -> Tuple[Tensor, Tensor, int, int]:
    """tiger_hip.h: tg_idmap_assign_recycle (tables on the CPU: its host twin) -> (ids int32 [n], free_list int32
    [min(n_free, n)]: the smallest free ids before the call, ascending; n_new: the new keys of the batch; error bits).
    Tables and bitmap are updated in place; ONE read-back, of the two result words."""
    m, dev = _idmap_struct('idmap_assign_recycle', tables, keys)
    _idmap_bits('idmap_assign_recycle', free_bits, dev)
    n = keys.numel()
    ids = torch.empty(n, dtype=torch.int32, device=dev)
    free_list = torch.empty(max(min(int(n_free), n), 0), dtype=torch.int32, device=dev)
    out2 = torch.empty(2, dtype=torch.int64, device=dev)
    if dev.type == 'cpu':
        check(lib.tg_idmap_assign_recycle_host(C_.byref(m), size, occupied, ptr(free_bits), free_bits.numel(), n_free, ptr(keys),
                                               n, ptr(ids), ptr(free_list), ptr(out2)), 'tg_idmap_assign_recycle_host')
    else:
        with torch.cuda.device(dev):
            nbytes = int(lib.tg_idmap_assign_recycle_workspace_bytes(n, size))
            ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
            check(lib.tg_idmap_assign_recycle(C_.byref(m), size, occupied, ptr(free_bits), free_bits.numel(), n_free, ptr(keys),
                                              n, ptr(ids), ptr(free_list), ptr(out2), ptr(ws), nbytes, stream_ptr(dev)),
                  'tg_idmap_assign_recycle')
    end, err = out2.tolist()
    return ids, free_list, int(end) - int(size), int(err)


def idmap_rebuild_free(tables, size: int, live: int, free_bits: Tensor, read_back: bool = True):
    """tiger_hip.h: tg_idmap_rebuild_free (tables on the CPU: its host twin): idmap_rebuild for a key_of with holes; live =
    the rows that hold a key, the padding row included -> the error word, or with read_back=False the device words unread."""
    m, dev = _idmap_struct('idmap_rebuild_free', tables)
    _idmap_bits('idmap_rebuild_free', free_bits, dev)
    out2 = torch.empty(2, dtype=torch.int64, device=dev)
    if dev.type == 'cpu':
        check(lib.tg_idmap_rebuild_free_host(C_.byref(m), size, live, ptr(free_bits), free_bits.numel(), ptr(out2)),
              'tg_idmap_rebuild_free_host')
    else:
        with torch.cuda.device(dev):
            check(lib.tg_idmap_rebuild_free(C_.byref(m), size, live, ptr(free_bits), free_bits.numel(), ptr(out2),
                                            stream_ptr(dev)), 'tg_idmap_rebuild_free')
    return int(out2[1].item()) if read_back else out2


# ---- event keys: external int64 event keys -> edge-table rows (tg_events_* and their host twins) ---------------------------
EVENTS_ERR_KEY = _lib.TG_EVENTS_ERR_KEY
_EVENTS_CLASSES = _IDMAP_CLASSES + ((_lib.TG_EVENTS_ERR_KEY, 'KEY: INT64_MIN is the key of the padding row alone'),)


def EVENTS_ERR_TEXT(word: int) -> str:
    """The message of a non-zero tg_events_screen error word: the classes by name."""
    return '; '.join(text for bit, text in _EVENTS_CLASSES if int(word) & bit)


def _events_screen(tables, rows: int, keys: Tensor, host: bool):
    m, dev = _idmap_struct('events_screen', tables, keys)
    if (dev.type == 'cpu') != host:
        raise ValueError(f'events_screen{"_host" if host else ""}: the tables live on {dev}')
    n = keys.numel()
    eids = torch.empty(n, dtype=torch.int32, device=dev)
    keep = torch.empty(n, dtype=torch.int64, device=dev)
    out2 = torch.empty(2, dtype=torch.int64, device=dev)
    if host:
        check(lib.tg_events_screen_host(C_.byref(m), rows, ptr(keys), n, ptr(eids), ptr(keep), ptr(out2)),
              'tg_events_screen_host')
    else:
        with torch.cuda.device(dev):
            nbytes = int(lib.tg_events_screen_workspace_bytes(n))
            ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
            check(lib.tg_events_screen(C_.byref(m), rows, ptr(keys), n, ptr(eids), ptr(keep), ptr(out2), ptr(ws), nbytes,
                                       stream_ptr(dev)), 'tg_events_screen')
    m_kept, err = out2.tolist()
    return eids, keep[:max(0, min(int(m_kept), n))], int(err)


def events_screen(tables, rows: int, keys: Tensor) -> Tuple[Tensor, Tensor, int]:
    """tiger_hip.h: tg_events_screen -> (eids int32 [n]: the row each key has or would get, -1 where the error word says
    why; keep int64 [m]: the positions of the first occurrences of the keys the map does not hold, ascending; error
    word: EVENTS_ERR_TEXT).  The tables are only read; ONE read-back, of the two result words."""
    return _events_screen(tables, rows, keys, False)


def events_screen_host(tables, rows: int, keys: Tensor) -> Tuple[Tensor, Tensor, int]:
    """tiger_hip.h: tg_events_screen_host: events_screen over CPU tensors, bit for bit"""
    return _events_screen(tables, rows, keys, True)


def _events_repack(key_of_old, keyless_old, remap, rows_before, key_of_new, keyless_new, rows_new, host: bool):
    what = 'events_repack_host' if host else 'events_repack'
    dev = key_of_old.device
    rows_before, rows_new = int(rows_before), int(rows_new)
    for t, dt, least, name in ((key_of_old, torch.int64, rows_before, 'key_of_old'),
                               (keyless_old, torch.int64, (rows_before + 63) // 64, 'keyless_old'),
                               (remap, torch.int32, rows_before, 'remap'), (key_of_new, torch.int64, rows_new, 'key_of_new'),
                               (keyless_new, torch.int64, (rows_new + 63) // 64, 'keyless_new')):
        if not (torch.is_tensor(t) and t.dtype == dt and t.dim() == 1 and t.is_contiguous() and t.device == dev
                and t.numel() >= least):
            raise ValueError(f'{what}: {name} must be a contiguous 1-d tensor of {dt} with at least {least} entries on {dev}')
    if (dev.type == 'cpu') != host:
        raise ValueError(f'{what}: the tables live on {dev}')
    if host:
        check(lib.tg_events_repack_host(ptr(key_of_old), ptr(keyless_old), ptr(remap), rows_before, ptr(key_of_new),
                                        ptr(keyless_new), rows_new), 'tg_events_repack_host')
    else:
        with torch.cuda.device(dev):
            check(lib.tg_events_repack(ptr(key_of_old), ptr(keyless_old), ptr(remap), rows_before, ptr(key_of_new),
                                       ptr(keyless_new), rows_new, stream_ptr(dev)), 'tg_events_repack')


def events_repack(key_of_old: Tensor, keyless_old: Tensor, remap: Tensor, rows_before: int, key_of_new: Tensor,
                  keyless_new: Tensor, rows_new: int):
    """tiger_hip.h: tg_events_repack: key_of_new[remap[r]] = key_of_old[r] and the keyless bit with it, for the rows a
    release of edge rows kept (remap: EdgeRowsRelease.remap).  keyless_*: 64-bit words held as int64.  Nothing is read
    back."""
    _events_repack(key_of_old, keyless_old, remap, rows_before, key_of_new, keyless_new, rows_new, False)


def events_repack_host(key_of_old: Tensor, keyless_old: Tensor, remap: Tensor, rows_before: int, key_of_new: Tensor,
                       keyless_new: Tensor, rows_new: int):
    """tiger_hip.h: tg_events_repack_host: events_repack over CPU tensors, bit for bit"""
    _events_repack(key_of_old, keyless_old, remap, rows_before, key_of_new, keyless_new, rows_new, True)


# ---- compacting the node id space (tg_node_compact_plan / tg_node_rows_compact / tg_bitmap_compact and their host twins) ---
NODE_COMPACT_CLASSES = ('ID0', 'SPARE', 'ROW', 'NBR')
_NODE_COMPACT_WHAT = ('node id 0 is the padding id and never leaves',
                      'bit {i} is set, at or beyond the {n} ids the bitmap covers',
                      'node {i} is dropped but still owns entries of the graph: erase it first',
                      'entry {i} of the graph names a dropped node as its neighbour: erase that node first')


def NODE_COMPACT_TEXT(cls: int, first=None, n_ids=None) -> str:
    """The message of a non-zero error class of node_compact_plan: the class by name and its smallest offender."""
    cls = int(cls)
    if not 1 <= cls <= len(NODE_COMPACT_CLASSES):
        return 'a clean compaction plan' if cls == 0 else f'unknown error class {cls}'
    what = _NODE_COMPACT_WHAT[cls - 1].format(i='?' if first is None else int(first), n='?' if n_ids is None else int(n_ids))
    return f'{NODE_COMPACT_CLASSES[cls - 1]}: {what}'


class NodeCompaction:
    """What a compaction of the node id space did: remap int32 [n_old] - the new id of an old one, -1 for a
    dropped id; monotone, so kept ids keep their order and remap[0] == 0 -, old_of int32 [n_new], its inverse list, ascending.
    n_graph_old / n_graph_new: the ids the planned graph covered before and after (ids beyond it - keys assigned and never
    admitted - own no row anywhere).  indptr / nbr: the arrays `Graph.compacted` adopts (None for a plan without a graph).
    Tensors on the plan's device; a plan of the host twin holds CPU tensors (indptr / nbr numpy arrays)."""

    def __init__(self, remap, old_of, n_old, n_new, n_graph_old=1, n_graph_new=1, indptr=None, nbr=None, code=0, first=-1):
        self.remap, self.old_of = remap, old_of
        self.n_old, self.n_new = int(n_old), int(n_new)
        self.n_graph_old, self.n_graph_new = int(n_graph_old), int(n_graph_new)
        self.indptr, self.nbr = indptr, nbr
        self.code, self.first = int(code), int(first)

    @property
    def device(self):
        return self.remap.device

    @property
    def identity(self) -> bool:
        return self.n_new == self.n_old

    def translate(self, ids: Tensor) -> Tensor:
        """old ids -> new ids, of the shape and dtype of ids (a gather of remap on the plan's device): -1 for a dropped id.
        ValueError: an id outside [0, n_old) (one read-back), ids that are no int32 / int64 tensor."""
        ids = torch.as_tensor(ids, device=self.device)
        if ids.dtype not in (torch.int32, torch.int64):
            raise ValueError('NodeCompaction.translate: ids are int32 or int64')
        if ids.numel() and bool(((ids < 0) | (ids >= self.n_old)).any()):
            raise ValueError(f'NodeCompaction.translate: an id outside [0, {self.n_old})')
        return self.remap[ids.long()].to(ids.dtype)

    def bitmap(self, bits: Tensor, n_ids: Optional[int] = None) -> Tensor:
        """A `new_bitmap` over the new ids with the bits of `bits`, a bitmap over the old ones (an `uptodate` bitmap, the
        mailbox's has_msg bits): new bit j = old bit old_of[j].  n_ids: the old ids `bits` covers (default: all it has words
        for, at most n_old); the result covers the kept ids below it."""
        return bitmap_compacted(bits, self, n_ids)

    def rows_below(self, n_ids: int) -> int:
        """the kept ids below n_ids <= n_old: the rows a table of n_ids rows keeps (a prefix of old_of: the remap is monotone)"""
        n_ids = int(n_ids)
        if not 0 <= n_ids <= self.n_old:
            raise ValueError(f'NodeCompaction.rows_below: {n_ids} is outside [0, {self.n_old}]')
        if n_ids == self.n_old:
            return self.n_new
        if n_ids == self.n_graph_old:
            return self.n_graph_new
        return int(torch.searchsorted(self.old_of, torch.tensor([n_ids], dtype=torch.int32, device=self.device))[0])


def _drop_bitmap(what: str, drop_bits, N: int, dev, is_np: bool):
    import numpy as np
    W = (N + 63) // 64
    if is_np:
        ok = isinstance(drop_bits, np.ndarray) and drop_bits.dtype in (np.int64, np.uint64) and drop_bits.ndim == 1 \
            and drop_bits.flags.c_contiguous and len(drop_bits) >= W
    else:
        ok = torch.is_tensor(drop_bits) and drop_bits.dtype == torch.int64 and drop_bits.dim() == 1 \
            and drop_bits.is_contiguous() and drop_bits.numel() >= W and drop_bits.device == dev
    if not ok:
        raise ValueError(f'{what}: drop_bits over {N} ids is a contiguous 1-d int64 bitmap of at least {W} words'
                         + ('' if is_np else f' on {dev}'))


def node_compact_plan(graph, drop_bits: Tensor, n_ids: Optional[int] = None, strict: bool = True) -> NodeCompaction:
    """Renumber the node ids densely without the ids of `drop_bits` (tiger_hip.h: tg_node_compact_plan).  drop_bits: 64-bit
    words over n_ids ids (default graph.num_node; at least that), a set bit = the id leaves - an IdMap's free_bits goes in as
    it is.  graph=None plans the ids alone (an id map without a model).  On the bitmap's device and the current stream, ONE
    read-back of the four result words.  ValueError (strict=True): the error classes ID0 / SPARE / ROW / NBR with the
    smallest offender (NODE_COMPACT_TEXT); strict=False leaves them in plan.code / plan.first, the arrays are then not to
    be used."""
    if not torch.is_tensor(drop_bits) or drop_bits.device.type == 'cpu':
        raise ValueError('node_compact_plan runs on the device (host arrays: node_compact_host)')
    dev = drop_bits.device
    with torch.cuda.device(dev):
        if graph is None:
            keep = torch.zeros(2, dtype=torch.int64, device=dev)
            g = _lib.TgTcsr(1, 0, ptr(keep), None, None, None)
        else:
            g, keep = _graph_struct('node_compact_plan', graph, dev)
        N = int(g.num_node if n_ids is None else n_ids)
        if N < g.num_node or N > 0x7FFFFFFF:
            raise ValueError(f'node_compact_plan: n_ids = {N} must lie in [num_node = {g.num_node}, 2^31 - 1]')
        _drop_bitmap('node_compact_plan', drop_bits, N, dev, False)
        remap = torch.empty(N, dtype=torch.int32, device=dev)
        old_of = torch.empty(N, dtype=torch.int32, device=dev)
        indptr = torch.empty(g.num_node + 1, dtype=torch.int64, device=dev)
        nbr = torch.empty(g.num_entry, dtype=torch.int32, device=dev)
        out4 = torch.empty(4, dtype=torch.int64, device=dev)
        nbytes = int(lib.tg_node_compact_workspace_bytes(N))
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
        check_rc = lib.tg_node_compact_plan(C_.byref(g), ptr(drop_bits), drop_bits.numel(), N, ptr(remap), ptr(old_of), ptr(indptr),
                                            ptr(nbr), ptr(out4), ptr(ws), nbytes, stream_ptr(dev))
        check(check_rc, 'tg_node_compact_plan')
        n_new, n_graph, code, first = out4.tolist()  # the one read-back
    if code and strict:
        raise ValueError('node_compact_plan: ' + NODE_COMPACT_TEXT(code, first, N))
    return NodeCompaction(remap, old_of[:n_new], N, n_new, g.num_node, n_graph, indptr[:n_graph + 1] if graph is not None else None,
                          nbr if graph is not None else None, code, first)


def node_compact_host(graph, drop_bits, n_ids: Optional[int] = None, strict: bool = True) -> NodeCompaction:
    """`node_compact_plan` with the host twin (tiger_hip.h: tg_node_compact_plan_host) over the graph's host arrays and a
    numpy int64 bitmap (`host_bitmap`) -> a NodeCompaction of CPU tensors (indptr / nbr: numpy arrays)."""
    import numpy as np
    if torch.is_tensor(drop_bits):
        drop_bits = drop_bits.numpy()
    if graph is None:
        keep = (np.zeros(2, dtype=np.int64),)
        g = _lib.TgTcsr(1, 0, ptr(keep[0]), None, None, None)
    else:
        g, keep = _graph_struct('node_compact_host', graph, torch.device('cpu'))
    N = int(g.num_node if n_ids is None else n_ids)
    if N < g.num_node or N > 0x7FFFFFFF:
        raise ValueError(f'node_compact_host: n_ids = {N} must lie in [num_node = {g.num_node}, 2^31 - 1]')
    _drop_bitmap('node_compact_host', drop_bits, N, None, True)
    remap, old_of = np.empty(N, dtype=np.int32), np.empty(N, dtype=np.int32)
    indptr, nbr = np.empty(g.num_node + 1, dtype=np.int64), np.empty(g.num_entry, dtype=np.int32)
    out4 = np.empty(4, dtype=np.int64)
    check_rc = lib.tg_node_compact_plan_host(C_.byref(g), ptr(drop_bits), len(drop_bits), N, ptr(remap), ptr(old_of), ptr(indptr),
                                             ptr(nbr), ptr(out4))
    check(check_rc, 'tg_node_compact_plan_host')
    n_new, n_graph, code, first = (int(x) for x in out4)
    if code and strict:
        raise ValueError('node_compact_host: ' + NODE_COMPACT_TEXT(code, first, N))
    return NodeCompaction(torch.from_numpy(remap), torch.from_numpy(old_of[:n_new].copy()), N, n_new, g.num_node, n_graph,
                          indptr[:n_graph + 1].copy() if graph is not None else None, nbr if graph is not None else None,
                          code, first)


def node_rows_compact(tables, old_of: Tensor):
    """ONE launch that compacts up to 8 per-node tables by `old_of` (tiger_hip.h: tg_node_rows_compact; CPU tensors: its host
    twin).  tables: (src, dst) pairs of contiguous tensors of one dtype and trailing shape on old_of's device; for j <
    dst.shape[0] <= old_of.numel(): dst[j] = src[old_of[j]], bit for bit.  A row is the bytes of src[i]: a multiple of 16, or
    8, 4 or 1.  dst may be the leading rows of a larger backing store; src and dst must not overlap.  ValueError: more than
    8 tables, tensors of other shapes / dtypes / devices, another row width."""
    tables = list(tables)
    dev = old_of.device
    if not (torch.is_tensor(old_of) and old_of.dtype == torch.int32 and old_of.dim() == 1 and old_of.is_contiguous()):
        raise ValueError('node_rows_compact: old_of must be a contiguous 1-d int32 tensor')
    if len(tables) > _lib.TG_NODE_ROWS_MAX:
        raise ValueError(f'node_rows_compact: {len(tables)} tables in one call (at most {_lib.TG_NODE_ROWS_MAX})')
    descs = (_lib.TgNodeRows * max(len(tables), 1))()
    for i, (src, dst) in enumerate(tables):
        if not (torch.is_tensor(src) and torch.is_tensor(dst) and src.dim() >= 1 and src.is_contiguous() and dst.is_contiguous()
                and src.dtype == dst.dtype and src.shape[1:] == dst.shape[1:] and src.device == dev and dst.device == dev):
            raise ValueError(f'node_rows_compact: table {i} must be a (src, dst) pair of contiguous tensors of one dtype and '
                             f'row shape on {dev}')
        row_bytes = src.element_size()
        for s in src.shape[1:]:
            row_bytes *= int(s)
        if dst.shape[0] > old_of.numel() or src.shape[0] < 1:
            raise ValueError(f'node_rows_compact: table {i} wants {dst.shape[0]} rows, old_of has {old_of.numel()}')
        if row_bytes not in (1, 4, 8) and (row_bytes < 16 or row_bytes % 16):
            raise ValueError(f'node_rows_compact: table {i} has rows of {row_bytes} bytes (a multiple of 16, or 8, 4 or 1)')
        descs[i] = _lib.TgNodeRows(ptr(src), ptr(dst), row_bytes, dst.shape[0], src.shape[0])
    if dev.type == 'cpu':
        check(lib.tg_node_rows_compact_host(descs, len(tables), ptr(old_of), old_of.numel()), 'tg_node_rows_compact_host')
    else:
        with torch.cuda.device(dev):
            check(lib.tg_node_rows_compact(descs, len(tables), ptr(old_of), old_of.numel(), stream_ptr(dev)), 'tg_node_rows_compact')


def bitmap_compacted(bits: Tensor, plan, n_ids: Optional[int] = None) -> Tensor:
    """A `new_bitmap` over the ids a compaction kept with the bits of `bits`, a bitmap over the old ids (tiger_hip.h:
    tg_bitmap_compact; CPU tensors: its host twin): new bit j = old bit plan.old_of[j]; spare bits zero.  n_ids: the old
    ids `bits` covers (default min(64 * words, plan.n_old)); the result covers plan.rows_below(n_ids) ids.  ValueError: bits
    is no int64 bitmap on the plan's device, or holds fewer words than n_ids take."""
    dev = plan.device
    if not (torch.is_tensor(bits) and bits.dtype == torch.int64 and bits.dim() == 1 and bits.is_contiguous() and bits.device == dev):
        raise ValueError(f'bitmap_compacted: bits must be a contiguous 1-d int64 bitmap on {dev}')
    n_in = min(64 * bits.numel(), plan.n_old) if n_ids is None else int(n_ids)
    if n_in < 0 or n_in > plan.n_old or bitmap_words(n_in) > bits.numel():
        raise ValueError(f'bitmap_compacted: {bits.numel()} words for {n_in} ids of a plan over {plan.n_old}')
    return bitmap_compact(bits, plan.old_of, n_in, plan.rows_below(n_in))


def bitmap_compact(bits: Tensor, old_of: Tensor, n_in: int, n_out: int, out: Optional[Tensor] = None) -> Tensor:
    """tiger_hip.h: tg_bitmap_compact (CPU tensors: its host twin) over a bitmap of n_in ids and the first n_out entries of
    old_of -> `out` (a zeroed bitmap of at least bitmap_words(n_out) words, e.g. a store with head-room; allocated exactly
    otherwise), its first bitmap_words(n_out) words written."""
    dev = old_of.device
    W = bitmap_words(n_out)
    if out is None:
        out = torch.zeros(W, dtype=torch.int64, device=dev)
    if (bits.dtype != torch.int64 or bits.device != dev or bits.numel() < bitmap_words(n_in) or not bits.is_contiguous()
            or old_of.dtype != torch.int32 or old_of.numel() < n_out or not old_of.is_contiguous()
            or out.dtype != torch.int64 or out.device != dev or out.numel() < W or not out.is_contiguous()):
        raise ValueError(f'bitmap_compact: int64 bitmaps over {n_in} and {n_out} ids and an int32 old_of of {n_out} entries on {dev}')
    if dev.type == 'cpu':
        check(lib.tg_bitmap_compact_host(ptr(bits), n_in, ptr(old_of), n_out, ptr(out)), 'tg_bitmap_compact_host')
    else:
        with torch.cuda.device(dev):
            check(lib.tg_bitmap_compact(ptr(bits), n_in, ptr(old_of), n_out, ptr(out), stream_ptr(dev)), 'tg_bitmap_compact')
    return out


# ---- incremental online state files: pack / splice T-CSR rows, scatter rows and bits (tg_journal.hip and its host twins) ---
SPLICE_CLASSES = ('ROWS', 'OFF', 'PTR')
_SPLICE_WHAT = ('rows[{i}] is no id below the new node count or does not ascend',
                'off[{i}] is no offset into the pack (off[0] == 0, non-decreasing, off[D] == the packed length)',
                'row {i} of the old graph has no valid bounds')


def SPLICE_TEXT(cls: int, first=None) -> str:
    """The message of a non-zero tcsr_rows_splice class."""
    if not 1 <= cls <= len(SPLICE_CLASSES):
        return 'a clean splice' if cls == 0 else f'error class {cls}'
    return f'{SPLICE_CLASSES[cls - 1]}: ' + _SPLICE_WHAT[cls - 1].format(i='?' if first is None else first)


def _journal_tcsr(what: str, arrays_or_graph):
    """a Graph (its device arrays) or four tensors (indptr int64 [N + 1], ts float64, nbr int32, eid int32 [P]) on one
    device - CPU tensors take the host twins -> (struct, the tensors that keep it alive, device)"""
    if hasattr(arrays_or_graph, 'tcsr'):
        g = arrays_or_graph.tcsr
        return g, arrays_or_graph._dev, arrays_or_graph._dev[0].device
    keep = tuple(arrays_or_graph)
    n, P = _verify_arrays(what, keep, False)
    dev = keep[0].device
    if any(a.device != dev for a in keep):
        raise ValueError(f'{what}: the four arrays of a T-CSR live on one device')
    return _lib.TgTcsr(n, P, *(ptr(a) for a in keep)), keep, dev


def _journal_list(what: str, name: str, t, dtype, dev, numel=None) -> Tensor:
    if not (torch.is_tensor(t) and t.dtype == dtype and t.dim() == 1 and t.is_contiguous() and t.device == dev
            and (numel is None or t.numel() == numel)):
        got = f'{t.dtype} {tuple(t.shape)} on {t.device}' if torch.is_tensor(t) else type(t).__name__
        raise ValueError(f'{what}: {name} must be a contiguous 1-d {dtype} tensor'
                         + (f' of {numel} entries' if numel is not None else '') + f' on {dev} (got {got})')
    return t


def tcsr_rows_pack(arrays_or_graph, rows: Tensor) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """The rows `rows` (int32, ascending, distinct) of a T-CSR, one after the other (tiger_hip.h: tg_tcsr_rows_pack_plan /
    _apply; CPU tensors: the host twin) -> (off int64 [D + 1], ts float64, nbr int32, eid int32 [off[D]]).  On the arrays'
    device and the current stream; ONE int64 is read back (the packed length), the outputs are allocated exactly."""
    what = 'tcsr_rows_pack'
    g, keep, dev = _journal_tcsr(what, arrays_or_graph)
    rows = _journal_list(what, 'rows', rows, torch.int32, dev)
    D = int(rows.numel())
    if D > g.num_node:
        raise ValueError(f'{what}: {D} rows of a graph of {g.num_node} nodes')
    off = torch.empty(D + 1, dtype=torch.int64, device=dev)
    if dev.type == 'cpu':
        r = rows.long()
        ok = (r >= 0) & (r < g.num_node)
        ip = keep[0]
        cap = int((ip[r[ok] + 1] - ip[r[ok]]).clamp_(min=0).sum()) if D else 0
        out = _entry_arrays(min(cap, g.num_entry), dev)
        check(lib.tg_tcsr_rows_pack_host(C_.byref(g), ptr(rows), D, ptr(off), *(ptr(t) for t in out)), 'tg_tcsr_rows_pack_host')
        n = int(off[-1])
        return (off,) + tuple(t[:n].clone() if t.numel() != n else t for t in out)
    with torch.cuda.device(dev):
        nbytes = int(lib.tg_tcsr_rows_pack_workspace_bytes(D))
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
        check(lib.tg_tcsr_rows_pack_plan(C_.byref(g), ptr(rows), D, ptr(off), ptr(ws), nbytes, stream_ptr(dev)),
              'tg_tcsr_rows_pack_plan')
        n = int(off[-1])  # the one read-back
        out = _entry_arrays(n, dev)
        check(lib.tg_tcsr_rows_pack_apply(C_.byref(g), ptr(rows), D, ptr(off), n, *(ptr(t) for t in out), stream_ptr(dev)),
              'tg_tcsr_rows_pack_apply')
    return (off,) + out


def tcsr_rows_splice(arrays_or_graph, n_new: int, rows: Tensor, off: Tensor, pack, strict: bool = True):
    """A NEW T-CSR over n_new >= num_node ids: row rows[j] is row j of the pack (off, and pack = (ts, nbr, eid) as
    `tcsr_rows_pack` returns them), every other row the old one, empty for ids at and beyond the old num_node (tiger_hip.h:
    tg_tcsr_rows_splice_plan / _apply; CPU tensors: the host twin) -> (code, first, arrays): code 0 and arrays = (indptr,
    ts, nbr, eid), or a class of SPLICE_CLASSES (1-based) with its smallest offender and arrays None.  rows / off / pack are
    untrusted as far as their CONTENTS go (dtypes, shapes and devices are checked here: ValueError); strict: a non-zero
    code raises ValueError.  ONE read-back of three words.  The result still has to pass `tcsr_verify`."""
    what = 'tcsr_rows_splice'
    g, keep, dev = _journal_tcsr(what, arrays_or_graph)
    n_new = int(n_new)
    if n_new < g.num_node or n_new > 0x7FFFFFFF:
        raise ValueError(f'{what}: n_new = {n_new} is outside [{g.num_node}, 2^31)')
    rows = _journal_list(what, 'rows', rows, torch.int32, dev)
    D = int(rows.numel())
    if D > n_new:
        raise ValueError(f'{what}: {D} rows for {n_new} node ids')
    off = _journal_list(what, 'off', off, torch.int64, dev, D + 1)
    if len(pack) != 3:
        raise ValueError(f'{what}: the pack is (ts, nbr, eid)')
    n_pack = int(pack[0].numel()) if torch.is_tensor(pack[0]) else -1
    pack = tuple(_journal_list(what, name, t, dt, dev, n_pack)
                 for name, t, dt in zip(('ts', 'nbr', 'eid'), pack, (torch.float64, torch.int32, torch.int32)))
    if g.num_entry + n_pack > 0xFFFFFFFF:
        raise ValueError(f'{what}: {g.num_entry} + {n_pack} entries are more than a T-CSR holds')
    indptr = torch.empty(n_new + 1, dtype=torch.int64, device=dev)
    if dev.type == 'cpu':
        out3 = torch.empty(3, dtype=torch.int64)
        out = _entry_arrays(g.num_entry + n_pack, dev)
        check(lib.tg_tcsr_rows_splice_host(C_.byref(g), n_new, ptr(rows), D, ptr(off), n_pack, *(ptr(t) for t in pack),
                                           ptr(indptr), *(ptr(t) for t in out), ptr(out3)), 'tg_tcsr_rows_splice_host')
        n, code, first = (int(x) for x in out3)
        if not code:
            out = tuple(t[:n].clone() for t in out)
    else:
        with torch.cuda.device(dev):
            out3 = torch.empty(3, dtype=torch.int64, device=dev)
            nbytes = int(lib.tg_tcsr_rows_splice_workspace_bytes(n_new))
            ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
            check(lib.tg_tcsr_rows_splice_plan(C_.byref(g), n_new, ptr(rows), D, ptr(off), n_pack, ptr(indptr), ptr(out3),
                                               ptr(ws), nbytes, stream_ptr(dev)), 'tg_tcsr_rows_splice_plan')
            n, code, first = out3.tolist()  # the one read-back
            if not code:
                out = _entry_arrays(n, dev)
                check(lib.tg_tcsr_rows_splice_apply(C_.byref(g), n_new, ptr(indptr), n, n_pack, *(ptr(t) for t in pack),
                                                    *(ptr(t) for t in out), ptr(ws), nbytes, stream_ptr(dev)),
                      'tg_tcsr_rows_splice_apply')
    if code:
        if strict:
            raise ValueError(f'{what}: ' + SPLICE_TEXT(code, first))
        return code, first, None
    return 0, -1, (indptr,) + tuple(out)


def node_rows_scatter(tables, ids: Tensor):
    """ONE launch that scatters up to 8 packed per-node tables back by `ids` (tiger_hip.h: tg_node_rows_scatter, the inverse
    of `node_rows_compact`; CPU tensors: its host twin).  tables: (src, dst) pairs of contiguous tensors of one dtype and
    trailing shape on ids' device; for j < src.shape[0] <= ids.numel(): dst[ids[j]] = src[j], bit for bit; an id that is
    no row of dst stores nothing.  ids: int32, distinct.  A row is the bytes of src[j]: a multiple of 16, or 8, 4 or 1.  dst
    may be the leading rows of a larger backing store; src and dst must not overlap.  ValueError: more than 8 tables,
    tensors of other shapes / dtypes / devices, another row width."""
    what = 'node_rows_scatter'
    tables = list(tables)
    if not (torch.is_tensor(ids) and ids.dtype == torch.int32 and ids.dim() == 1 and ids.is_contiguous()):
        raise ValueError(f'{what}: ids must be a contiguous 1-d int32 tensor')
    dev = ids.device
    if len(tables) > _lib.TG_NODE_ROWS_MAX:
        raise ValueError(f'{what}: {len(tables)} tables in one call (at most {_lib.TG_NODE_ROWS_MAX})')
    descs = (_lib.TgNodeRows * max(len(tables), 1))()
    for i, (src, dst) in enumerate(tables):
        if not (torch.is_tensor(src) and torch.is_tensor(dst) and src.dim() >= 1 and src.is_contiguous() and dst.is_contiguous()
                and src.dtype == dst.dtype and src.shape[1:] == dst.shape[1:] and src.device == dev and dst.device == dev):
            raise ValueError(f'{what}: table {i} must be a (src, dst) pair of contiguous tensors of one dtype and row shape on {dev}')
        row_bytes = src.element_size()
        for s in src.shape[1:]:
            row_bytes *= int(s)
        if src.shape[0] > ids.numel() or dst.shape[0] < 1:
            raise ValueError(f'{what}: table {i} brings {src.shape[0]} rows, ids has {ids.numel()}')
        if row_bytes not in (1, 4, 8) and (row_bytes < 16 or row_bytes % 16):
            raise ValueError(f'{what}: table {i} has rows of {row_bytes} bytes (a multiple of 16, or 8, 4 or 1)')
        descs[i] = _lib.TgNodeRows(ptr(src), ptr(dst), row_bytes, dst.shape[0], src.shape[0])
    if dev.type == 'cpu':
        check(lib.tg_node_rows_scatter_host(descs, len(tables), ptr(ids), ids.numel()), 'tg_node_rows_scatter_host')
    else:
        with torch.cuda.device(dev):
            check(lib.tg_node_rows_scatter(descs, len(tables), ptr(ids), ids.numel(), stream_ptr(dev)), 'tg_node_rows_scatter')


def bitmap_scatter(flags: Tensor, ids: Tensor, bits: Tensor, n_ids: int):
    """bit ids[j] of `bits` (a `new_bitmap` over n_ids ids, IN PLACE) = (flags[j] != 0); every other bit keeps its value
    (tiger_hip.h: tg_bitmap_scatter; CPU tensors: its host twin).  flags uint8 [n], ids int32 [n], distinct; an id outside
    [0, n_ids) stores nothing."""
    what = 'bitmap_scatter'
    dev = bits.device
    n_ids = int(n_ids)
    ids = _journal_list(what, 'ids', ids, torch.int32, dev)
    flags = _journal_list(what, 'flags', flags, torch.uint8, dev, ids.numel())
    if bits.dtype != torch.int64 or bits.dim() != 1 or not bits.is_contiguous() or n_ids < 1 or bits.numel() < bitmap_words(n_ids):
        raise ValueError(f'{what}: bits must be a contiguous int64 bitmap of at least {bitmap_words(max(n_ids, 1))} words '
                         f'({n_ids} ids)')
    if dev.type == 'cpu':
        check(lib.tg_bitmap_scatter_host(ptr(flags), ptr(ids), ids.numel(), ptr(bits), n_ids), 'tg_bitmap_scatter_host')
    else:
        with torch.cuda.device(dev):
            check(lib.tg_bitmap_scatter(ptr(flags), ptr(ids), ids.numel(), ptr(bits), n_ids, stream_ptr(dev)), 'tg_bitmap_scatter')
