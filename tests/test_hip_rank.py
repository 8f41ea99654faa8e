"""Ranking evaluation (one-vs-many) on the GPU: TIGE.rank_scores / tg_rank_scores against the CPU oracle, tg_rank_stats
against numpy on the device's own scores, eval_edge_ranking end to end.

The oracle has no one-vs-many call: column 1 + j of the score matrix is, by definition, `neg_scores` of the oracle's
contrast_learning on a COPY of its state with the negatives cand[:, j], column 0 its `pos_scores`.  Scores: float32 within
1e-4 under both measures of _util.assert_close.  Ranks are checked against the device's own scores, exactly - so no
tolerance on rank flips exists or is needed.  State: bit for bit."""
import copy

import numpy as np
import pytest
import torch

from _rank_ref import numpy_ranks
from _util import assert_close

pytestmark = pytest.mark.gpu
TOL = 1e-4
WARM = [0, 5, 37, 101]   # ragged warm-up batches (5, 32, 64 events), flush_msg after the second
KS = (1, 3, 10)


def dev():
    return torch.device('cuda', 0)


def build(d, d_e, K, hit='bin', *, nh=2, L=1, E=200, n_u=60, n_i=15, T=5000.0, seed=0, strategy='recent_edges'):
    """as tests/test_hip_heads_widths.py::build, with the hit type as a parameter"""
    import bench
    from oracle import tiger_oracle as O
    from www2023tiger_amd.data.graph import Graph
    from www2023tiger_amd.model.feature_getter import NumericalFeature
    from www2023tiger_amd.model.restarters import StaticRestarter
    from www2023tiger_amd.model.tiger import TIGER
    st = bench.make_stream(n_u, n_i, E, T, seed=seed, d_e=d_e, with_efeats=True)
    n_nodes = st['n_nodes']
    g = Graph.from_arrays(st['src'], st['dst'], st['ts'], st['eids'], strategy=strategy, seed=0,
                          max_node_id=n_nodes - 1, device=dev())
    nf = (np.random.RandomState(seed + 1).standard_normal((n_nodes, d)) * 0.3).astype(np.float32)
    nf[0] = 0
    torch.manual_seed(seed)
    fg = NumericalFeature(torch.from_numpy(nf), torch.from_numpy(st['efeats']), dim=d, device=dev())
    fg.n_nodes, fg.n_edges = n_nodes, E
    rst = StaticRestarter(raw_feat_getter=fg, graph=g)
    model = TIGER(raw_feat_getter=fg, graph=g, restarter=rst, n_neighbors=K, hit_type=hit, n_layers=L, n_head=nh,
                  dropout=0.0, msg_src='left', upd_src='right').to(dev())
    with torch.no_grad():
        model.time_encoder.phase.uniform_(-0.5, 0.5)
        rst.left_emb.weight.normal_(0, 0.1)
        rst.right_emb.weight.normal_(0, 0.1)
        if hit in ('bin', 'count'):
            model.hit_embedding.weight.normal_(0, 0.5)   # classes that move a score well above the tolerance
    model.eval()
    og = O.OracleGraph(st['src'], st['dst'], st['ts'], st['eids'], max_node_id=n_nodes - 1)
    params = {k: v.detach().cpu().numpy() for k, v in model.named_parameters()}
    orc = O.OracleTIGER(params, og, n_nodes=n_nodes, dim=d, nfeats=nf, efeats=st['efeats'], n_neighbors=K,
                        msg_src='left', upd_src='right', restarter='static', hist_len=None, n_head=nh, hit_type=hit)
    return model, orc, st


def batch(st, lo, hi):
    return [st[k][lo:hi] for k in ('src', 'dst', 'neg', 'ts', 'eids')]


def warm(model, orc, st, K, with_oracle=True):
    """a few ragged stream batches and a flush in between: non-trivial memories and mailbox, pending messages"""
    from oracle import tiger_oracle as O
    for b, (lo, hi) in enumerate(zip(WARM[:-1], WARM[1:])):
        a = batch(st, lo, hi)
        model.stream_step(*a)
        if with_oracle:
            orc.contrast_learning(*a, O.collate(orc.graph, a[0], a[1], a[2], a[3], K, 'static'))
        if b == 1:
            model.flush_msg()
            if with_oracle:
                orc.flush_msg()
    assert bool(model.msg_store.has_msg_mask().any())


def candidates(orc, st, lo, hi, K, C, seed=5):
    """[B, C] candidate ids: random nodes, and in fixed columns (as many as C has room for) a sampled neighbour of the
    source (its hit class differs from the row's), the pad id 0, dst[i] itself, src[i], a node with no history before t,
    and an id twice"""
    rs = np.random.RandomState(seed)
    src, dst, ts = st['src'][lo:hi], st['dst'][lo:hi], st['ts'][lo:hi]
    n_nodes, B = st['n_nodes'], hi - lo
    cand = rs.randint(1, n_nodes, (B, C)).astype(np.int64)
    nb = orc.graph.sample_temporal_neighbor(src, ts, K, strategy='recent_edges')[0]
    seen = np.union1d(st['src'][:hi], st['dst'][:hi])
    unseen = np.setdiff1d(np.arange(1, n_nodes), seen)
    assert len(unseen) > 0
    has_nb = nb.max(1) > 0
    assert has_nb.any()
    info = dict(nbr_col=0, rows_with_nbr=np.nonzero(has_nb)[0])
    cand[has_nb, 0] = nb[has_nb, -1]   # lists are left-padded: the last slot is the most recent neighbour
    if C >= 5:
        cand[:, 1] = 0
        cand[:, 2] = dst
        cand[:, 3] = src
        cand[:, 4] = unseen[rs.randint(0, len(unseen), B)]
    if C >= 7:
        cand[:, 6] = cand[:, 5]
        info['dup'] = (5, 6)
    return cand, info


_REF = {}


def case(d, d_e, K, B, C, hit, forms=()):
    """model (warmed), the ranked batch, its candidates, the oracle's score matrix (computed once per configuration)"""
    from oracle import tiger_oracle as O
    model, orc, st = build(d, d_e, K, hit, seed=d + K)
    if 'fused' in forms:
        model.fuse_attention()
    if 'eager' in forms:
        model.eager_updates()
    key = (d, d_e, K, B, C, hit)
    warm(model, orc, st, K, with_oracle=key not in _REF)
    lo, hi = WARM[-1], WARM[-1] + B
    src, dst, _, ts, eids = batch(st, lo, hi)
    if key not in _REF:
        cand, info = candidates(orc, st, lo, hi, K, C)
        ref = np.zeros((B, 1 + C), dtype=np.float32)
        for j in range(C):
            o2 = copy.deepcopy(orc)
            out = o2.contrast_learning(src, dst, cand[:, j], ts, eids, O.collate(o2.graph, src, dst, cand[:, j], ts, K, 'static'))
            ref[:, 1 + j] = out['neg_scores'].detach().numpy()
            if j == 0:   # (the positives of the other calls differ from these in the last bit at most: other involved sets)
                ref[:, 0] = out['pos_scores'].detach().numpy()
        _REF[key] = (cand, info, ref)
    cand, info, ref = _REF[key]
    t = lambda x, dt=torch.int64: torch.as_tensor(x).to(dev(), dt)
    return dict(model=model, st=st, lo=lo, hi=hi, src=t(src), dst=t(dst), ts=t(ts, torch.float64), cand=t(cand),
                cand_np=cand, info=info, ref=ref, K=K)


def check_against_oracle(got, ref):
    got = got.cpu().numpy()
    assert got.shape == ref.shape and np.isfinite(got).all()
    for j in range(ref.shape[1]):
        assert_close(got[:, j], ref[:, j], 'pos_scores' if j == 0 else f'candidate column {j - 1}', TOL)


def state_of(model):
    L, R, S = model.left_memory, model.right_memory, model.msg_store
    ts = dict(left_vals=L.vals, left_ts=L.update_ts, left_active=L.active_mask, right_vals=R.vals, right_ts=R.update_ts,
              right_active=R.active_mask, msg_vals=S.node_msg_vals, msg_ts=S.node_msg_ts, has_msg=S.has_msg_bits)
    for name in ('_pending', '_gtab', '_ctab', '_fused'):
        if getattr(model, name, None) is not None:
            ts[name] = getattr(model, name)
    return {k: v.clone() for k, v in ts.items()}


def assert_same_state(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k


# ------------------------------------------------------------------------------------------ scores against the oracle
SHAPES = [  # (d, d_e, K, B, C)
    (16, 16, 10, 5, 7),     # 40 pair rows: neither 32 nor 64
    (16, 16, 10, 32, 33),   # an event's 34 pairs straddle the 32-row tiles
    (172, 4, 10, 29, 5),    # hidden width no multiple of 32 (two column passes, a partly filled last tile), 4-wide edges
    (8, 8, 5, 3, 1),        # the smallest
]
CASES = [SHAPES[0] + (h,) for h in ('bin', 'count', 'vec', 'none')] + [s + ('bin',) for s in SHAPES[1:]]


@pytest.mark.parametrize('d,d_e,K,B,C,hit', CASES, ids=[f'd{c[0]}-e{c[1]}-K{c[2]}-B{c[3]}-C{c[4]}-{c[5]}' for c in CASES])
def test_scores_match_the_oracle_column_by_column(d, d_e, K, B, C, hit):
    c = case(d, d_e, K, B, C, hit)
    before = state_of(c['model'])
    got = c['model'].rank_scores(c['src'], c['dst'], c['ts'], c['cand'])
    check_against_oracle(got, c['ref'])
    assert_same_state(before, state_of(c['model']))


@pytest.mark.parametrize('forms', [('eager', 'fused'), ('fused',), ('eager',)], ids=lambda f: '+'.join(f))
def test_a_streaming_model_passes_the_same_check(forms):
    """eager_updates() / fuse_attention() on: the same oracle check, and the derived tables are left as they were"""
    c = case(*SHAPES[0], 'bin', forms=forms)
    m = c['model']
    assert (m._pending is not None) == ('eager' in forms) and (m._fused is not None) == ('fused' in forms)
    before = state_of(m)
    check_against_oracle(m.rank_scores(c['src'], c['dst'], c['ts'], c['cand']), c['ref'])
    assert_same_state(before, state_of(m))
    c = case(*SHAPES[2], 'bin', forms=forms)
    check_against_oracle(c['model'].rank_scores(c['src'], c['dst'], c['ts'], c['cand']), c['ref'])


# ------------------------------------------------------------------------------------------ ranks
def test_device_ranks_equal_numpy_on_the_device_scores():
    from www2023tiger_amd import hip_ops
    c = case(*SHAPES[1], 'bin')
    scores = c['model'].rank_scores(c['src'], c['dst'], c['ts'], c['cand'])
    ids = torch.cat([c['dst'][:, None], c['cand']], 1)
    mask = torch.ones_like(c['cand'], dtype=torch.bool)
    mask[::3, 7:11] = False
    a, b = c['info']['dup']
    s = scores.cpu().numpy()
    assert np.array_equal(s[:, 1 + a].view(np.uint32), s[:, 1 + b].view(np.uint32))   # equal pairs, equal bits
    for mk in (None, mask):
        st = hip_ops.rank_stats(scores, ids, c['dst'], mask=mk, ks=KS)
        g, e, v, r = numpy_ranks(s, ids.cpu().numpy(), c['dst'].cpu().numpy(), None if mk is None else mk.cpu().numpy())
        np.testing.assert_array_equal(st['n_greater'].cpu().numpy(), g)
        np.testing.assert_array_equal(st['n_equal'].cpu().numpy(), e)
        np.testing.assert_array_equal(st['n_valid'].cpu().numpy(), v)
        np.testing.assert_array_equal(st['rank'].cpu().numpy(), r)
        m = hip_ops.rank_metrics(st['acc'], KS)
        assert m['n_events'] == len(r) and abs(m['mrr'] - float(np.mean(1.0 / r))) < 1e-12
        for k in KS:
            assert abs(m['hits'][k] - float(np.mean(r <= k))) < 1e-12
        # dst itself, the pad id and (every third row) four masked columns are left out
        assert (v <= c['cand'].shape[1] - 2).all()
        # the host twin on the same scores: the same numbers
        h = hip_ops.rank_stats(scores.cpu(), ids.cpu(), c['dst'].cpu(), mask=None if mk is None else mk.cpu(), ks=KS)
        for k in ('n_greater', 'n_equal', 'n_valid', 'rank'):
            assert torch.equal(h[k], st[k].cpu()), k
    # the duplicated candidate ties with itself: a positive placed on it would see two equal scores - here through the
    # ranks of a matrix whose column 0 IS that candidate
    s2 = scores.clone()
    s2[:, 0] = s2[:, 1 + a]
    st = hip_ops.rank_stats(s2, ids, c['dst'], ks=KS)
    left_in = ((c['cand'][:, a] != c['dst']) & (c['cand'][:, a] != 0)).cpu().numpy()
    assert (st['n_equal'].cpu().numpy()[left_in] >= 2).all() and left_in.any()


# ------------------------------------------------------------------------------------------ state, chunks, shared form
def test_a_step_after_ranking_equals_a_twin_that_never_ranked():
    c = case(*SHAPES[0], 'bin')
    twin = case(*SHAPES[0], 'bin')
    assert_same_state(state_of(c['model']), state_of(twin['model']))   # twins: same build, same warm-up
    c['model'].rank_scores(c['src'], c['dst'], c['ts'], c['cand'])
    a = batch(c['st'], c['lo'], c['hi'])
    h1 = c['model'].stream_step(*a).h.clone()
    h2 = twin['model'].stream_step(*a).h.clone()
    assert torch.equal(h1, h2)
    assert_same_state(state_of(c['model']), state_of(twin['model']))


def test_chunked_equals_unchunked_bit_for_bit():
    c = case(*SHAPES[1], 'bin')
    B, C = c['cand'].shape
    whole = c['model'].rank_scores(c['src'], c['dst'], c['ts'], c['cand'])
    per_chunk = 10 * (C + 2)   # 10 events per chunk: 4 chunks of 32 events
    assert -(-B // 10) >= 3
    parts = c['model'].rank_scores(c['src'], c['dst'], c['ts'], c['cand'], chunk_queries=per_chunk)
    assert torch.equal(whole, parts)
    single = c['model'].rank_scores(c['src'], c['dst'], c['ts'], c['cand'], chunk_queries=1)   # one event per chunk
    assert torch.equal(whole, single)


def test_chunked_equals_unchunked_where_row_counts_straddle_kernel_choices():
    """d = 172, 48 events x 301 pairs.  Embedded among its own rows, a one-event chunk (302 queries) would take fc1
    (k = 3 d = 516) as K-split blocks (tg_gemm.hip: k_gemm_ks16, at most 1100 48-row tiles), the whole call (14 496
    queries) as plain 64 x 64 blocks that sum k in one order, a 16-event chunk (4 832) in between: other bits.
    rank_scores embeds every query in a call of RANK_EMBED_ROWS rows, so all three agree bit for bit."""
    d, K, B, C = 172, 10, 48, 300
    model, orc, st = build(d, 4, K, 'bin', seed=d + K)
    warm(model, orc, st, K, with_oracle=False)
    lo, hi = WARM[-1], WARM[-1] + B
    src, dst, _, ts, _ = batch(st, lo, hi)
    cand = np.random.RandomState(11).randint(1, st['n_nodes'], (B, C)).astype(np.int64)
    t = lambda x, dt=torch.int64: torch.as_tensor(x).to(dev(), dt)
    src, dst, ts, cand = t(src), t(dst), t(ts, torch.float64), t(cand)
    R = model.RANK_EMBED_ROWS
    assert (C + 2) < R < 16 * (C + 2) < B * (C + 2)   # a chunk below one unit, one of two units, a call of four
    before = state_of(model)
    whole = model.rank_scores(src, dst, ts, cand)
    assert torch.isfinite(whole).all() and whole.unique().numel() > B
    for per_chunk in (1, 16 * (C + 2)):
        parts = model.rank_scores(src, dst, ts, cand, chunk_queries=per_chunk)
        assert torch.equal(whole, parts), per_chunk
    assert_same_state(before, state_of(model))


def test_shared_candidates_equal_the_broadcast_form():
    c = case(*SHAPES[0], 'bin')
    shared = c['cand'][0].clone()
    B = c['src'].numel()
    one = c['model'].rank_scores(c['src'], c['dst'], c['ts'], shared)
    two = c['model'].rank_scores(c['src'], c['dst'], c['ts'], shared.unsqueeze(0).expand(B, -1).contiguous())
    assert one.shape == (B, shared.numel() + 1) and torch.equal(one, two)


def test_float32_times_give_the_scores_of_float64_times_here():
    """(the stream's times are integers: float32 holds them exactly) - the argument's dtype alone changes nothing"""
    c = case(*SHAPES[3], 'bin')
    a = c['model'].rank_scores(c['src'], c['dst'], c['ts'], c['cand'])
    b = c['model'].rank_scores(c['src'], c['dst'], c['ts'].float(), c['cand'])
    assert torch.equal(a, b)
    check_against_oracle(a, c['ref'])


# ------------------------------------------------------------------------------------------ refusals
def test_refusals_come_before_anything_runs():
    from www2023tiger_amd.data.graph import Graph
    from www2023tiger_amd.eval_utils import eval_edge_ranking
    c = case(*SHAPES[3], 'bin')
    m, st = c['model'], c['st']
    before = state_of(m)
    uni = Graph.from_arrays(st['src'], st['dst'], st['ts'], st['eids'], strategy='uniform', seed=0,
                            max_node_id=st['n_nodes'] - 1, device=dev())
    mt = uni._mt_state().clone()
    with pytest.raises(NotImplementedError, match='uniform'):
        m.rank_scores(c['src'], c['dst'], c['ts'], c['cand'], graph=uni)
    assert torch.equal(mt, uni._mt_state())   # the graph's random stream was not consumed
    with pytest.raises(NotImplementedError, match='restart'):
        eval_edge_ranking(m, None, dev(), c['cand'], restart_mode=True)
    m.train()
    with pytest.raises(RuntimeError, match='eval'):
        m.rank_scores(c['src'], c['dst'], c['ts'], c['cand'])
    m.eval()
    with pytest.raises(ValueError, match='node id'):
        m.rank_scores(c['src'], c['dst'], c['ts'], torch.full_like(c['cand'], st['n_nodes']))
    assert_same_state(before, state_of(m))
    n = st['n_nodes']
    m.partition_state(torch.arange(n, dtype=torch.int32), n)
    with pytest.raises(RuntimeError, match='partitioned'):
        m.rank_scores(c['src'], c['dst'], c['ts'], c['cand'])
    with pytest.raises(RuntimeError, match='partitioned'):
        eval_edge_ranking(m, None, dev(), c['cand'])


def test_vec_hits_with_unaligned_pair_rows_refuse():
    """2 (d + K) not a multiple of 4: refused as the one-call evaluation step refuses it, by the method and by the library"""
    import ctypes as C
    from www2023tiger_amd._lib import TG_EUNSUPPORTED, lib
    from www2023tiger_amd.model.training import score_struct
    model, _, st = build(8, 8, 5, 'vec')
    assert not model._fused_eval_ok()
    a = batch(st, 0, 4)
    t = lambda x, dt=torch.int64: torch.as_tensor(x).to(dev(), dt)
    with pytest.raises(NotImplementedError, match='vec'):
        model.rank_scores(t(a[0]), t(a[1]), t(a[3], torch.float64), t(a[2])[:, None])
    sp = score_struct(model)
    assert lib.tg_rank_scores(4, 1, 8, 5, C.byref(sp), *([None] * 8), 0, None) == TG_EUNSUPPORTED


# ------------------------------------------------------------------------------------------ end to end
def loader(model, st, K, bs=50):
    from www2023tiger_amd.data.data_loader import BatchLoader, GraphCollator, InteractionData
    E = len(st['src'])
    data = InteractionData(st['src'], st['dst'], st['ts'], st['eids'], np.zeros(E, dtype=np.int64), seed=0, eval=True,
                           neg_dst=st['neg'])
    return BatchLoader(data, bs, GraphCollator(model.graph, K, 1, restarter='static'))


@pytest.mark.parametrize('resident', ['0', '1'], ids=['per-batch-eval', 'resident-eval'])
def test_eval_edge_ranking_end_to_end(resident, monkeypatch):
    """200 events at batch 50 with 11 candidates: the event count, MRR / Hits against float64 numpy on the per-batch device
    scores of a twin loop, and the state afterwards against eval_edge_prediction's over the same loader on a twin model -
    bit for bit against its per-batch loop (TG_EVAL_RESIDENT=0), to float32 rounding against its resident pass, which
    streams with eager updates and pre-multiplied weights (tests/test_hip_eval.py states that pass's own tolerance)."""
    from www2023tiger_amd.eval_utils import eval_edge_prediction, eval_edge_ranking
    monkeypatch.setenv('TG_EVAL_RESIDENT', resident)
    d, K, C = 16, 10, 11
    built = [build(d, d, K, 'bin', seed=3) for _ in range(3)]
    models, st = [b[0] for b in built], built[0][2]
    E = len(st['src'])
    cand = np.random.RandomState(9).randint(0, st['n_nodes'], (E, C)).astype(np.int64)
    cand[::7, 0] = st['dst'][::7]
    cand[:, 5] = cand[:, 4]
    out = eval_edge_ranking(models[0], loader(models[0], st, K), dev(), cand, ks=KS, return_ranks=True)
    assert out['n_events'] == E and out['ranks'].shape == (E,)
    # the twin loop: scores of the state before each batch, then the batch
    ranks, lo = [], 0
    with torch.no_grad():
        for src, dst, neg, ts, eids, _, cg in loader(models[1], st, K):
            c = torch.from_numpy(cand[lo:lo + len(src)]).to(dev())
            s = models[1].rank_scores(src.to(dev()), dst.to(dev()), cg.ts64, c).cpu().numpy()
            ids = np.concatenate([dst.cpu().numpy()[:, None], cand[lo:lo + len(src)]], 1)
            ranks.append(numpy_ranks(s, ids, dst.cpu().numpy())[3])
            models[1].contrast_learning(src.to(dev()), dst.to(dev()), neg.to(dev()), ts.to(dev()), eids.to(dev()), cg)
            lo += len(src)
    r = np.concatenate(ranks)
    np.testing.assert_array_equal(out['ranks'].cpu().numpy(), r)
    assert abs(out['mrr'] - float(np.mean(1.0 / r))) < 1e-12
    for k in KS:
        assert abs(out['hits'][k] - float(np.mean(r <= k))) < 1e-12
    assert 0.0 < out['mrr'] <= 1.0 and (r > 1).any()
    assert_same_state(state_of(models[0]), state_of(models[1]))
    eval_edge_prediction(models[2], loader(models[2], st, K), dev(), False)
    got, want = state_of(models[0]), state_of(models[2])
    if resident == '0':
        assert_same_state(got, want)
    else:
        for k in ('left_ts', 'right_ts', 'msg_ts', 'has_msg', 'left_active', 'right_active'):
            assert torch.equal(got[k], want[k]), k
        for k in ('left_vals', 'right_vals', 'msg_vals'):
            assert_close(got[k].cpu().numpy(), want[k].cpu().numpy(), k, TOL)
