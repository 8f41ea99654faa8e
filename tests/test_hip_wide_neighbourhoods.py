"""Neighbour counts 17 .. 64 through the streaming step, the training step and ranking, against the CPU oracle.

The library takes any n_neighbors up to one wavefront (64); K = 16 is where the samplers switch from 16 lanes per query to a
whole wavefront (sample_batch_launch, sample_edges_f32_launch, tg_sample_recent_edges), where the collate prefetch stops
applying (tg_stream_step: `K <= 16`) and the uniform sampler refuses, and lane 15 is the highest lane the rest of the
suite fills in k_attn_core / k_attn_core_bwd / k_build_pairs / tg_rank_scores (one key per lane, `lane < K`).
K = 17, 20, 33, 64 are 1, 0, 1, 0 mod 4; 2, 2, 0, 1 mod 3; 5, 2, 3, 4 mod 6 and odd / even: every depth PD of
k_attn_core's register ring (csrc/tg_attn.hip: 2 / 3 / 4 / 6 by <NV, W, FS>) meets a last round that is cut short by
`min(k + PD, K - 1)`, and - but for PD = 6 - a full one.

Stream: bench.make_stream(40, 6, 640, 5000.0, seed=3): 40 users on 6 items, so lists fill up fast.  Live keys per query of
the whole stream (recent_edges; a query's list depends on (node, t) alone, not on the batching):

      K | none | 1 - 16 | 17 .. K-1 | exactly K
     17 |   52 |    614 |         - |      1254
     20 |   52 |    614 |        72 |      1182
     33 |   52 |    614 |       304 |       950
     64 |   52 |    614 |       734 |       520

Every test asserts from the ORACLE's lists that each class that exists for its K, strategy and part of the stream occurred:
a run that never fills lane 16 proves nothing.  (recent_nodes lists hold distinct neighbours: an item has at most 40, a
user at most 6 - no list of 64 is full, the longest has 37.)

Indices bit-exact; float32 within 1e-4 under both measures of _util.assert_close; training: the tolerances of
test_hip_train.test_training_other_shapes (losses 1e-4 relative, grad_err < 3e-4); tg_rank_scores itself: the derived bound
of tests/_rank_ref.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from _util import assert_close
from test_hip_heads_widths import _run_stream, build, dev

pytestmark = pytest.mark.gpu
TOL = 1e-4
STREAM = dict(n_u=40, n_i=6, E=640, T=5000.0, seed=3)
EDGES = [0, 5, 37, 101, 130, 192, 256, 320, 384, 448, 512, 576, 640]        # ragged, then batches of 64
EDGES32 = [0, 5, 37, 66, 98, 130, 161, 192, 224, 256, 288, 320]             # at most 32 events (two layers)
FILL = {17: (52, 614, 0, 1254), 20: (52, 614, 72, 1182), 33: (52, 614, 304, 950), 64: (52, 614, 734, 520)}
KEYS = ('src', 'dst', 'neg', 'ts', 'eids')


def fill_classes(lists, K):
    """queries with (no, 1 .. 16, 17 .. K - 1, exactly K) live keys in the [Q, K] neighbour-id arrays `lists`"""
    n = np.concatenate([(np.asarray(x).reshape(-1, K) != 0).sum(1) for x in lists])
    return int((n == 0).sum()), int(((n >= 1) & (n <= 16)).sum()), int(((n > 16) & (n < K)).sum()), int((n == K).sum())


def assert_fill(lists, K, full=True):
    """every class that exists occurred: 17 .. K - 1 needs K > 17, `full` is false where no list can hold K keys"""
    c = fill_classes(lists, K)
    assert c[0] > 0 and c[1] > 0, c
    assert c[2] > 0 or K == 17, c
    assert c[3] > 0 or not full, c
    assert c[2] + c[3] > 0, c   # lane 16 and above held a key
    return c


def batch(st, lo, hi):
    return [st[k][lo:hi] for k in KEYS]


def to(x, dt):
    return torch.as_tensor(x).to(dev(), dt)


# ------------------------------------------------------------------------------ 1. streaming step, K = 17 / 20 / 33 / 64
STREAM_CASES = [  # (n_head, d, d_e, K, node table, edge table, form, pre-multiplied weights) -> k_attn_core<NH, NV, W, FS>, PD
    (2, 64, 20, 17, True, True, 'lazy', False),           # <2,1,2,2>  PD 4, 17 = 4 * 4 + 1
    (2, 64, 20, 20, True, True, 'lazy', False),           #            PD 4, full last round
    (2, 64, 20, 64, True, True, 'eager', False),          #            PD 4, every lane of the wavefront
    (1, 132, 4, 33, True, True, 'lazy', False),           # <1,1,4,2>  PD 3, full last round
    (1, 132, 4, 20, True, True, 'lazy', False),           #            PD 3, 20 = 6 * 3 + 2
    (1, 132, 4, 64, True, True, 'eager', False),          #            PD 3, 64 = 21 * 3 + 1
    (2, 300, 300, 17, True, True, 'lazy', False),         # <2,2,4,2>  PD 2, odd
    (2, 300, 300, 64, True, True, 'lazy', False),         #            PD 2, even
    (2, 300, 300, 20, True, True, 'eager-lean', True),    # <2,2,4,1>  PD 2, even (node rows from the centre-row table)
    (2, 300, 300, 33, True, True, 'eager-lean', True),    #            PD 2, odd
    (4, 32, 4, 17, False, True, 'eager', False),          # <4,1,2,1>  PD 4 (no node table)
    (4, 32, 4, 20, True, True, 'eager-lean', True),       # <4,1,2,1>  PD 4
    (1, 16, 16, 64, True, True, 'eager-lean', True),      # <1,1,2,1>  PD 4
    (2, 172, 4, 33, True, True, 'eager-lean', True),      # <2,1,4,1>  PD 4, 33 = 8 * 4 + 1 (the MOOC layout)
    (2, 64, 64, 20, False, False, 'lazy', True),          # <2,1,2,0>  PD 6, 20 = 3 * 6 + 2
    (4, 136, 136, 64, True, False, 'eager', True),        # <4,1,4,0>  PD 6, 64 = 10 * 6 + 4 (centre-row table, no edge table)
    (2, 300, 300, 17, False, False, 'lazy', True),        # <2,2,4,0>  PD 3, 17 = 5 * 3 + 2
    (2, 300, 300, 33, False, False, 'lazy', True),        #            PD 3, full last round
]
# eager + lean + pre-multiplied cases (d, d_e <= 256), one per K, run once more without the query-row table (TG_GTAB=0)
NO_GTAB_CASES = [(2, 64, 20, 17, True, True, 'eager-lean', True)] + [c for c in STREAM_CASES if c[6] == 'eager-lean' and c[1] <= 256]


def case_id(c):
    return f"K{c[3]}-h{c[0]}-d{c[1]}-e{c[2]}{'-n' if c[4] else ''}{'-E' if c[5] else ''}-{c[6]}{'-f' if c[7] else ''}"


def run_stream_case(nh, d, d_e, K, nfeats, efeats, form, fuse):
    """-> the model after the whole stream: lists bit-exact, embeddings within TOL, a flush_msg in the middle, the final
    state (test_hip_heads_widths._run_stream), and the fill classes of the table"""
    model, orc, st = build(nh, d, d_e, nfeats=nfeats, efeats=efeats, K=K, **STREAM)
    assert model.model_struct().d_e == (d_e if efeats else d)
    if fuse:
        model.fuse_attention()
        assert model.model_struct().attn_fused
    if form != 'lazy':
        model.eager_updates()
    lists = []
    _run_stream(model, orc, st, K, form, edges=EDGES, lists=lists)
    assert fill_classes([cg['l1_nids'] for cg in lists], K) == FILL[K]
    return model


@pytest.mark.parametrize('nh,d,d_e,K,nfeats,efeats,form,fuse', STREAM_CASES, ids=[case_id(c) for c in STREAM_CASES])
def test_stream_step_with_wide_neighbourhoods(nh, d, d_e, K, nfeats, efeats, form, fuse):
    run_stream_case(nh, d, d_e, K, nfeats, efeats, form, fuse)


def no_gtab_child():
    """body of the child process of test_stream_step_without_query_row_table_with_wide_neighbourhoods"""
    assert sorted(c[3] for c in NO_GTAB_CASES) == [17, 20, 33, 64]
    done = 0
    for c in NO_GTAB_CASES:
        print('no-gtab case', case_id(c), flush=True)
        run_stream_case(*c)
        done += 1
    print(f'NO GTAB CASES OK {done}', flush=True)


def test_stream_step_without_query_row_table_with_wide_neighbourhoods():
    """Without the query-row table (TG_GTAB=0, read once per process, so the cases run in a child process) the eager + lean +
    pre-multiplied step runs the G product per batch: k_attn_core reads G from the workspace instead of tg_model.g_table and
    the centres launch copies the centre rows.  One case per K, the same checks as above."""
    env = dict(os.environ, TG_GTAB='0')
    env.setdefault('OMP_NUM_THREADS', '4')
    here = os.path.dirname(os.path.abspath(__file__))
    code = (f'import sys; sys.path[:0] = [{os.path.dirname(here)!r}, {here!r}]; '
            'import test_hip_wide_neighbourhoods as t; t.no_gtab_child()')
    r = subprocess.run([sys.executable, '-c', code], env=env, cwd=os.path.dirname(here), capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and f'NO GTAB CASES OK {len(NO_GTAB_CASES)}' in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ------------------------------------------------------------------------------ 2. two layers, K = 17 / 20
@pytest.mark.parametrize('form', ['lazy', 'eager-fused-lean'])
@pytest.mark.parametrize('strategy', ['recent_edges', 'recent_nodes'])
@pytest.mark.parametrize('K', [17, 20], ids=['K17', 'K20'])
def test_two_layer_stream_step_with_wide_neighbourhoods(K, strategy, form):
    """--n_layers 2: the second hop (sample_edges_f32_launch<64> / sample_nodes_f32_launch: Q K queries at the neighbours'
    float32 times) and the inner attention layer over Q K centres with K keys each.  The lists of the first hop bit-exact;
    those of the second through the involved set (full step) and through the embeddings, which read every one of them."""
    from oracle import tiger_oracle as O
    from test_hip_parity import compare_state_with_oracle
    model, orc, st = build(2, 16, 4, K=K, L=2, strategy=strategy, **STREAM)
    lean = 'lean' in form
    if 'eager' in form:
        model.eager_updates()
        model.fuse_attention()
        assert model.model_struct(0).attn_fused and model.model_struct(1).attn_fused
    hop1, hop2 = [], []
    for b, (lo, hi) in enumerate(zip(EDGES32[:-1], EDGES32[1:])):
        a = batch(st, lo, hi)
        cg = O.collate(orc.graph, a[0], a[1], a[2], a[3], K, 'static', n_layers=2)
        hop1.append(cg['l1_nids'])
        hop2.append(cg['hop2_nids'])
        ref = orc.contrast_learning(*a, cg)['h_left'].detach().numpy()
        buf = model.stream_step(*a, lean=lean)
        np.testing.assert_array_equal(buf.l1_nids.cpu().numpy(), cg['l1_nids'])
        np.testing.assert_array_equal(buf.l1_eids.cpu().numpy(), cg['l1_eids'])
        np.testing.assert_array_equal(buf.l1_ts.cpu().numpy(), cg['l1_ts'])
        if not lean:
            cnt = buf.counts.cpu().numpy()
            np.testing.assert_array_equal(buf.involved.cpu().numpy()[:cnt[0]], cg['involved'])   # second hop included
        assert_close(buf.h[:2 * (hi - lo)].cpu().numpy(), ref, 'h_left', TOL)
        if b == 3:
            model.flush_msg()
            orc.flush_msg()
    assert_fill(hop1, K)
    assert_fill(hop2, K)
    compare_state_with_oracle(model, orc)


# ------------------------------------------------------------------------------ 3. recent_nodes, one layer, K = 20 / 64
@pytest.mark.parametrize('lean', [False, True], ids=['full', 'lean'])
@pytest.mark.parametrize('K', [20, 64], ids=['K20', 'K64'])
def test_recent_nodes_step_with_wide_neighbourhoods(K, lean):
    """--strategy recent_nodes inside the step: k_sample_recent_nodes (one wavefront per query, the last occurrence of
    each distinct neighbour) and k_mark_lists, eager + pre-multiplied as
    test_hip_parity.test_fused_step_with_the_recent_nodes_strategy_matches_oracle"""
    from oracle import tiger_oracle as O
    from test_hip_parity import compare_state_with_oracle
    model, orc, st = build(2, 64, 20, K=K, strategy='recent_nodes', **STREAM)
    model.fuse_attention()
    model.eager_updates()
    lists, differs = [], False
    for b, (lo, hi) in enumerate(zip(EDGES[:-1], EDGES[1:])):
        a = batch(st, lo, hi)
        cg = O.collate(orc.graph, a[0], a[1], a[2], a[3], K, 'static')
        lists.append(cg['l1_nids'])
        ref = orc.stream_step(*a, cg).numpy()
        buf = model.stream_step(*a, lean=lean)
        np.testing.assert_array_equal(buf.l1_nids.cpu().numpy(), cg['l1_nids'])
        np.testing.assert_array_equal(buf.l1_eids.cpu().numpy(), cg['l1_eids'])
        np.testing.assert_array_equal(buf.l1_ts.cpu().numpy(), cg['l1_ts'])
        if not lean:
            cnt = buf.counts.cpu().numpy()
            np.testing.assert_array_equal(buf.involved.cpu().numpy()[:cnt[0]], cg['involved'])
        assert_close(buf.h[:2 * (hi - lo)].cpu().numpy(), ref, 'h_left', TOL)
        edges = orc.graph.sample_temporal_neighbor(np.concatenate(a[:3]), np.tile(a[3], 3), K, strategy='recent_edges')[0]
        differs = differs or not np.array_equal(edges, cg['l1_nids'])
        if b == 3:
            model.flush_msg()
            orc.flush_msg()
    assert differs   # the strategy really samples other lists than recent_edges
    assert_fill(lists, K, full=K <= 37)   # 40 users: the longest list of distinct neighbours has 37 entries
    compare_state_with_oracle(model, orc)


# ------------------------------------------------------------------------------ 4. training step
def repeat_a_pair(lo, hi):
    """edit(st) for build: events [lo, hi) all join the pair of event lo, so that up to min(K, hi - lo) of the most recent
    neighbours of either node are the other one ('count' hits above 16); timestamps stay sorted"""
    def edit(st):
        st['src'][lo:hi] = st['src'][lo]
        st['dst'][lo:hi] = st['dst'][lo]
    return edit


def set_hit_embedding(model, orc):
    """classes that move a score well above the tolerance (as test_hip_rank.build), on both sides"""
    with torch.no_grad():
        model.hit_embedding.weight.normal_(0, 0.5)
    orc.p['hit_embedding.weight'] = model.hit_embedding.weight.detach().cpu().clone()


TRAIN_CASES = [  # (K, hit, strategy, layers)
    (20, 'bin', 'recent_edges', 1), (20, 'count', 'recent_edges', 1), (20, 'vec', 'recent_edges', 1),
    (64, 'count', 'recent_edges', 1), (64, 'vec', 'recent_edges', 1),
    (20, 'bin', 'recent_nodes', 1),    # hit_lists runs a sampler launch of its own (tg_sample_recent_edges, 64 lanes)
    (20, 'bin', 'recent_edges', 2),
]


@pytest.mark.parametrize('K,hit,strategy,L', TRAIN_CASES, ids=[f'K{c[0]}-{c[1]}-{c[2]}-L{c[3]}' for c in TRAIN_CASES])
def test_training_step_with_wide_neighbourhoods(K, hit, strategy, L):
    """forward, both losses and every gradient of the mutual-learning step (k_attn_core_bwd, k_build_pairs and its backward,
    the d + K wide score products of 'vec') against the oracle's autograd, on the last five batches of 64 of the stream"""
    from oracle import tiger_oracle as O
    from test_hip_train import sync_params
    from test_oracle_golden import grad_err
    from www2023tiger_amd.model.training import TrainBuffers
    B, first = 64, 5
    d, d_e = (32, 20) if L == 1 else (16, 4)
    model, orc, st = build(2, d, d_e, K=K, L=L, hit=hit, strategy=strategy,
                           edit=repeat_a_pair(400, 445) if hit == 'count' else None, **STREAM)
    if hit in ('bin', 'count'):
        set_hit_embedding(model, orc)
    model.train()
    tb = TrainBuffers(model, B, mutual=True)
    hop1, hop2, most_hits = [], [], 0
    for b in range(first, first + 5):
        a = batch(st, b * B, (b + 1) * B)
        cg = O.collate(orc.graph, a[0], a[1], a[2], a[3], K, 'static', n_layers=L)
        hop1.append(cg['l1_nids'])
        if L == 2:
            hop2.append(cg['hop2_nids'])
        most_hits = max([most_hits] + [int(cg[k].sum(1).max()) for k in ('src_hits', 'dst_hits', 'neg_src_hits', 'neg_dst_hits')])
        sync_params(model, orc)
        c, ml, grads = orc.train_step(*a, cg, lr=1e-3, mutual_coef=1.0)
        tb.sb.load(to(a[0], torch.int64), to(a[1], torch.int64), to(a[2], torch.int64), to(a[3], torch.float64),
                   to(a[4], torch.int64))
        tb.launch()
        assert int(tb.sb.err.item()) == 0
        print(f'batch {b}: losses {float(tb.losses[0]):.6f} / {c:.6f}, {float(tb.losses[1]):.6f} / {ml:.6f}')
        assert abs(float(tb.losses[0]) - c) < TOL * max(1.0, abs(c)), b
        assert abs(float(tb.losses[1]) - ml) < TOL * max(1.0, abs(ml)), b
        worst = max((grad_err(g_.cpu().numpy(), grads[k].numpy()), k) for k, g_ in tb.grads.items())
        print(f'batch {b}: worst gradient error {worst[0]:.2e} ({worst[1]})')
        assert worst[0] < 3e-4, (b, worst)
    assert_fill(hop1, K)
    if L == 2:
        assert_fill(hop2, K)
    if hit == 'count':
        assert most_hits > 16, most_hits   # hit_emb rows 17 .. K were read
    elif hit == 'vec':
        assert most_hits > 0


# ------------------------------------------------------------------------------ 5. ranking at K = 20
@pytest.mark.parametrize('hit', ['count', 'vec'])
def test_rank_scores_with_wide_neighbourhoods(hit):
    """TIGE.rank_scores column by column against the oracle, as test_hip_rank.test_scores_match_the_oracle_column_by_column
    (same candidates, same bound), and the ranks of tests/_rank_ref.numpy_ranks on the device's scores; the stream repeats
    one pair 61 times before the ranked batch, whose first rows have that source: hit counts above 16"""
    import copy
    from _rank_ref import numpy_ranks
    from oracle import tiger_oracle as O
    from test_hip_rank import WARM, assert_same_state, candidates, check_against_oracle, state_of, warm
    from www2023tiger_amd import hip_ops
    d, K, B, C = 16, 20, 5, 7
    lo, hi = WARM[-1], WARM[-1] + B

    def edit(st):
        repeat_a_pair(40, lo)(st)
        st['src'][lo:lo + 2] = st['src'][40]   # ranked rows whose source is the pair's: candidate column 0 is its partner

    model, orc, st = build(2, d, d, K=K, hit=hit, edit=edit, n_u=60, n_i=15, E=200, T=5000.0, seed=d + K)
    if hit == 'count':
        set_hit_embedding(model, orc)
    warm(model, orc, st, K)
    src, dst, _, ts, eids = batch(st, lo, hi)
    cand, info = candidates(orc, st, lo, hi, K, C)
    ref = np.zeros((B, 1 + C), dtype=np.float32)
    most_hits = 0
    for j in range(C):
        o2 = copy.deepcopy(orc)
        cg = O.collate(o2.graph, src, dst, cand[:, j], ts, K, 'static')
        most_hits = max([most_hits] + [int(cg[k].sum(1).max()) for k in ('src_hits', 'dst_hits', 'neg_src_hits', 'neg_dst_hits')])
        out = o2.contrast_learning(src, dst, cand[:, j], ts, eids, cg)
        ref[:, 1 + j] = out['neg_scores'].detach().numpy()
        if j == 0:
            ref[:, 0] = out['pos_scores'].detach().numpy()
    assert most_hits > 16, most_hits
    c = fill_classes([orc.graph.sample_temporal_neighbor(np.concatenate([src, cand.ravel()]), np.concatenate([ts, np.repeat(ts, C)]),
                                                         K, strategy='recent_edges')[0]], K)
    assert c[1] > 0 and c[3] > 0, c   # short and full hit windows among the 40 queries
    before = state_of(model)
    got = model.rank_scores(to(src, torch.int64), to(dst, torch.int64), to(ts, torch.float64), to(cand, torch.int64))
    check_against_oracle(got, ref)
    assert_same_state(before, state_of(model))
    ids = np.concatenate([dst[:, None], cand], 1)
    stats = hip_ops.rank_stats(got, to(ids, torch.int64), to(dst, torch.int64), ks=(1, 3, 10))
    g, e, v, r = numpy_ranks(got.cpu().numpy(), ids, dst)
    np.testing.assert_array_equal(stats['n_greater'].cpu().numpy(), g)
    np.testing.assert_array_equal(stats['n_equal'].cpu().numpy(), e)
    np.testing.assert_array_equal(stats['rank'].cpu().numpy(), r)


@pytest.mark.parametrize('key', [(16, 20, 5, 7, 'count'), (16, 20, 5, 7, 'vec'), (32, 64, 9, 7, 'count'), (32, 64, 9, 7, 'vec')],
                         ids=lambda k: 'd{}-K{}-B{}-C{}-{}'.format(*k))
def test_rank_score_kernel_with_wide_hit_windows(key, request):
    """tg_rank_scores itself on the constructed cases of tests/_rank_ref.py (every hit column, every class 0 .. K) within
    the derived bound of the float64 reference, as test_hip_rank_ops.test_scores_within_the_derived_bound_of_float64"""
    from _rank_ref import REF_ARGS, make_case, pair_hits, score_bound, score_ref
    from test_hip_rank_ops import run_scores
    c = make_case(*key)
    sh, dh = pair_hits(c['nbr_src'], c['nbr_cand'], c['src'], c['cand_ids'])
    K = key[1]
    assert sh.sum(2).max() == K and dh.sum(2).max() == K   # all K lanes of a window hit, on either side
    assert ((sh.sum(2) > 16) & (sh.sum(2) < K)).any()
    ref, A = score_ref(*[c[k] for k in REF_ARGS])
    bound = score_bound(A, c['d'], c['W'])
    rc, got = run_scores(c)
    assert rc == 0
    got = got.cpu().numpy().astype(np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all()
    ratio = np.abs(got - ref) / bound
    print(f'{request.node.callspec.id}: worst err / bound {float(ratio.max()):.3e} (err {np.abs(got - ref).max():.2e})')
    assert ratio.max() <= 1.0, (float(ratio.max()), int(ratio.argmax()))


# ------------------------------------------------------------------------------ 6. prefetch requested, not applicable
def test_requested_prefetch_does_not_apply_above_16_neighbours():
    """The collate prefetch (tg_step_io.prefetch_state) serves K <= 16: a resident stream that asks for it at K = 20, in
    the form bench.py times (lean, eager, pre-multiplied), collates in every step instead - the flag stays 0, the offset
    advances, lists and embeddings follow the oracle; then a flag left at 1 (as a prefetch made for this buffer would leave
    it) is discarded by the next step."""
    from oracle import tiger_oracle as O
    from test_hip_parity import compare_state_with_oracle
    from test_hip_timed_form import _resident
    B, K = 64, 20
    model, orc, st = build(2, 64, 20, K=K, **STREAM)
    model.fuse_attention()
    model.eager_updates()
    buf = model.StepBuffers(model, B, False, resident=_resident(st), prefetch=True, debug_lists=True)
    buf.io.lean = 1
    lists = []
    for b in range(STREAM['E'] // B):
        if b == 6:
            buf._pf_state.value = 1   # an unused flag: the step must discard it and collate itself
        model.launch_step(buf)
        torch.cuda.synchronize()
        assert int(buf.err.item()) == 0
        assert buf._pf_state.value == 0
        assert int(buf.offset.item()) == (b + 1) * B
        a = batch(st, b * B, (b + 1) * B)
        cg = O.collate(orc.graph, a[0], a[1], a[2], a[3], K, 'static')
        lists.append(cg['l1_nids'])
        ref = orc.stream_step(*a, cg).numpy()
        np.testing.assert_array_equal(buf.dbg_l1_nids.cpu().numpy(), cg['l1_nids'])
        np.testing.assert_array_equal(buf.dbg_l1_eids.cpu().numpy(), cg['l1_eids'])
        np.testing.assert_array_equal(buf.dbg_l1_ts.cpu().numpy(), cg['l1_ts'])
        cnt = buf.counts.tolist()
        assert cnt[0] == -1 and cnt[2] == len(cg['rd_nids'])   # the lean form was taken
        model.note_rows(cnt[1], cnt[2])
        assert_close(buf.h[:2 * B].cpu().numpy(), ref, f'h_left, batch {b}', TOL)
    assert fill_classes(lists, K) == FILL[K]
    compare_state_with_oracle(model, orc)


# ------------------------------------------------------------------------------ 7. refusals
@pytest.mark.parametrize('step', ['stream', 'train'])
def test_more_neighbours_than_a_wavefront_refuse(step):
    """n_neighbors = 65: the K counterpart of test_hip_heads_widths.test_configurations_outside_the_dispatch_refuse"""
    import ctypes as C
    from www2023tiger_amd._lib import lib
    from www2023tiger_amd.model.training import TrainBuffers
    model, _, st = build(2, 16, 16, E=40, n_u=10, n_i=5, K=65)
    m = model.model_struct()
    assert lib.tg_stream_step_workspace_bytes2(C.byref(m), 20, 1) == 0
    assert lib.tg_temporal_attn_workspace_bytes(C.byref(m), 20) == 0
    a = batch(st, 0, 20)
    before = model.left_memory.vals.clone(), model.right_memory.vals.clone()
    with pytest.raises((RuntimeError, NotImplementedError), match='unsupported model'):
        if step == 'stream':
            model.stream_step(*a)
        else:
            model.train()
            TrainBuffers(model, 20, mutual=True).launch()
    torch.cuda.synchronize()
    assert torch.equal(before[0], model.left_memory.vals) and torch.equal(before[1], model.right_memory.vals)


def test_uniform_sampling_above_16_neighbours_refuses_and_leaves_everything_as_it_was():
    """numpy's argsort of the K draws is stable only up to 16 elements, so `uniform` stops there: at K = 17 the streaming
    and the training step raise, the state (memories, mailbox rows, timestamps, has-message set) and the graph's random
    stream keep their bits, and the same model and step buffers go on with a supported graph as if nothing had happened."""
    from oracle import tiger_oracle as O
    from test_hip_parity import compare_state_with_oracle
    from test_hip_rank import assert_same_state, state_of
    from www2023tiger_amd.data.graph import Graph
    from www2023tiger_amd.model.training import TrainBuffers
    K, B = 17, 64
    model, orc, st = build(2, 16, 16, K=K, **STREAM)
    recent = model.graph
    uniform = Graph.from_arrays(st['src'], st['dst'], st['ts'], st['eids'], strategy='uniform', seed=5,
                                max_node_id=st['n_nodes'] - 1, device=dev())
    lists = []

    def step(b):
        a = batch(st, b * B, (b + 1) * B)
        cg = O.collate(orc.graph, a[0], a[1], a[2], a[3], K, 'static')
        lists.append(cg['l1_nids'])
        ref = orc.stream_step(*a, cg).numpy()
        buf = model.stream_step(*a)
        np.testing.assert_array_equal(buf.l1_nids.cpu().numpy(), cg['l1_nids'])
        np.testing.assert_array_equal(buf.l1_eids.cpu().numpy(), cg['l1_eids'])
        cnt = buf.counts.cpu().numpy()
        np.testing.assert_array_equal(buf.involved.cpu().numpy()[:cnt[0]], cg['involved'])
        assert_close(buf.h[:2 * B].cpu().numpy(), ref, f'h_left, batch {b}', TOL)

    for b in range(6):
        step(b)
    assert bool(model.msg_store.has_msg_mask().any())
    before, mt = state_of(model), uniform._mt_state().clone()
    a = batch(st, 6 * B, 7 * B)
    model.graph = uniform
    with pytest.raises((RuntimeError, NotImplementedError)):
        model.stream_step(*a)
    torch.cuda.synchronize()
    assert_same_state(before, state_of(model))
    model.train()
    tb = TrainBuffers(model, B, mutual=True)
    tb.sb.load(to(a[0], torch.int64), to(a[1], torch.int64), to(a[2], torch.int64), to(a[3], torch.float64),
               to(a[4], torch.int64))
    with pytest.raises((RuntimeError, NotImplementedError)):
        tb.launch()
    torch.cuda.synchronize()
    model.eval()
    assert_same_state(before, state_of(model))
    assert torch.equal(mt, uniform._mt_state())   # no draw was consumed
    model.graph = recent
    for b in range(6, 10):   # the step buffers of the refused call (same batch size) serve again
        step(b)
    assert fill_classes(lists, K) == FILL[K]
    compare_state_with_oracle(model, orc)
