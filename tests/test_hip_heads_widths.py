"""Every instance of the head-count / row-width dispatch against the CPU oracle, on small synthetic streams.

The kernels branch on the number of attention heads and on the widths of the node memory (d) and of the edge
features (d_e):
  k_attn_core<NH, NV, W, FS>  (csrc/tg_attn.hip, launch_attn_core): NH = n_head; W = 2 columns per lane when
      max(d, d_e) <= 128, else 4; NV = float4 per lane, 2 when max(d, d_e) > 256; FS = feature streams per key
      (2: node + edge tables, 1: edge table only - no node table, or the node rows come from the per-node table of
      centre rows of the eager + pre-multiplied form - 0: no edge table and no node stream)
  k_attn_core_bwd<NH, NV>      (csrc/tg_train.hip)
  k_seq_scores<HP, V2>, k_seq_scores_bwd<HP, V2>  (csrc/tg_restart.hip): HP = 32 / 64 / 128 history rows per block,
      V2 = the restarter's head width (4 d + d_e) / n_head is even
The reference fixtures (tests/golden: *_h1 / *_h4) pin the oracle's semantics at 1 and 4 heads and at edge widths other
than d; this module pins each kernel instance to that oracle.  Configurations outside the dispatch must refuse before
anything runs.  Indices bit-exact, float32 within 1e-4 under both measures of _util.assert_close; training: the
tolerances of test_hip_train.test_training_other_shapes."""
import numpy as np
import pytest
import torch

from _util import assert_close

pytestmark = pytest.mark.gpu
TOL = 1e-4


def dev():
    return torch.device('cuda', 0)


def build(nh, d, d_e, *, nfeats=True, efeats=True, restarter='static', H=None, L=1, K=10, E=200, n_u=40, n_i=15,
          T=5000.0, seed=0, msg_src='left', upd_src='right', hit='bin', strategy='recent_edges', edit=None):
    """A HIP model of the given head count and widths on a synthetic stream (bench.make_stream) and the oracle carrying
    the same weights.  nfeats: a random node-feature table (else none); efeats: an edge-feature table of width d_e (else
    none, and the model's edge width is d).  hit: the score head's hit features; strategy: the sampling strategy of both
    graphs; edit(st): changes the stream in place before the graphs are built from it."""
    import bench
    from oracle import tiger_oracle as O
    from www2023tiger_amd.data.graph import Graph
    from www2023tiger_amd.model.feature_getter import NumericalFeature
    from www2023tiger_amd.model.restarters import SeqRestarter, StaticRestarter
    from www2023tiger_amd.model.tiger import TIGER
    st = bench.make_stream(n_u, n_i, E, T, seed=seed, d_e=d_e, with_efeats=efeats)
    if edit is not None:
        edit(st)
    n_nodes = st['n_nodes']
    g = Graph.from_arrays(st['src'], st['dst'], st['ts'], st['eids'], strategy=strategy, seed=0,
                          max_node_id=n_nodes - 1, device=dev())
    nf = None
    if nfeats:
        nf = (np.random.RandomState(seed + 1).standard_normal((n_nodes, d)) * 0.3).astype(np.float32)
        nf[0] = 0
    torch.manual_seed(seed)
    fg = NumericalFeature(None if nf is None else torch.from_numpy(nf),
                          None if st['efeats'] is None else torch.from_numpy(st['efeats']), dim=d, device=dev())
    fg.n_nodes, fg.n_edges = n_nodes, E
    rst = (SeqRestarter(raw_feat_getter=fg, graph=g, hist_len=H, n_head=nh, dropout=0.0) if restarter == 'seq'
           else StaticRestarter(raw_feat_getter=fg, graph=g))
    model = TIGER(raw_feat_getter=fg, graph=g, restarter=rst, n_neighbors=K, hit_type=hit, n_layers=L, n_head=nh,
                  dropout=0.0, msg_src=msg_src, upd_src=upd_src).to(dev())
    with torch.no_grad():  # non-trivial time-encoder phase and static restarter rows
        model.time_encoder.phase.uniform_(-0.5, 0.5)
        if restarter == 'static':
            rst.left_emb.weight.normal_(0, 0.1)
            rst.right_emb.weight.normal_(0, 0.1)
    model.eval()
    og = O.OracleGraph(st['src'], st['dst'], st['ts'], st['eids'], strategy=strategy, seed=0, max_node_id=n_nodes - 1)
    params = {k: v.detach().cpu().numpy() for k, v in model.named_parameters()}
    orc = O.OracleTIGER(params, og, n_nodes=n_nodes, dim=d, nfeats=nf, efeats=st['efeats'], n_neighbors=K,
                        msg_src=msg_src, upd_src=upd_src, restarter=restarter, hist_len=H, n_head=nh, hit_type=hit)
    return model, orc, st


# ------------------------------------------------------------------------------ inference step, every (NH, NV, W, FS)
SHAPES = [  # (n_head, d, d_e, K): the instance with an edge table / without one (d_e = d then)
    (1, 16, 16, 10),     # k_attn_core<1,1,2>
    (1, 100, 172, 10),   # <1,1,4>: edge rows wider than 128 (TGN MOOC / Wikipedia edges, --dim 100) / <1,1,2>
    (1, 132, 4, 5),      # <1,1,4>: node rows wider than 128, 4-wide edges
    (2, 300, 300, 10),   # <2,2,4>
    (2, 100, 300, 16),   # <2,2,4> through the edge width alone / <2,1,2>
    (2, 172, 4, 10),     # <2,1,4>: the MOOC layout (172-wide node rows, 4-wide edges)
    (4, 32, 4, 10),      # <4,1,2>
    (4, 136, 136, 10),   # <4,1,4>
    (2, 64, 20, 10),     # <2,1,2>
]
# (node table, edge table, form, pre-multiplied weights) -> FS
VARIANTS = [
    (True, True, 'lazy', False),        # FS 2
    (True, True, 'eager-lean', True),   # FS 1: node rows from the centre-row table (eager + fused)
    (False, True, 'eager', False),      # FS 1: no node table
    (False, False, 'lazy', True),       # FS 0
    (True, False, 'eager', True),       # FS 0: centre-row table, no edge table
]
STREAM_CASES = [s + v for i, s in enumerate(SHAPES) for v in VARIANTS[:3] + [VARIANTS[3 + i % 2]]]


def _run_stream(model, orc, st, K, form, L=1, edges=None, lists=None):
    """edges: the batch boundaries (default: the ragged ones of the 200-event streams); lists: a list that receives the
    oracle's collation of every batch"""
    from oracle import tiger_oracle as O
    from test_hip_parity import compare_state_with_oracle
    if edges is None:
        edges = [0, 5, 37, 101, 130, 192, 200]   # ragged: 5, 32, 64, 29, 62, 8 events
    for b, (lo, hi) in enumerate(zip(edges[:-1], edges[1:])):
        a = [st[k][lo:hi] for k in ('src', 'dst', 'neg', 'ts', 'eids')]
        n = hi - lo
        buf = model.stream_step(*a, lean=(form == 'eager-lean'))
        if L == 1:
            assert (int(buf.counts[0]) == -1) == (form == 'eager-lean')   # the lean form really ran (or not)
        cg = O.collate(orc.graph, a[0], a[1], a[2], a[3], K, 'static', n_layers=L)
        if lists is not None:
            lists.append(cg)
        ref = orc.contrast_learning(*a, cg)['h_left'].detach().numpy()
        np.testing.assert_array_equal(buf.l1_nids.cpu().numpy()[:3 * n], cg['l1_nids'])
        np.testing.assert_array_equal(buf.l1_eids.cpu().numpy()[:3 * n], cg['l1_eids'])
        assert_close(buf.h[:2 * n].cpu().numpy(), ref, 'h_left', TOL)
        if b == 3:  # flush_msg in the middle: pending messages consumed on both sides
            model.flush_msg()
            orc.flush_msg()
    compare_state_with_oracle(model, orc)


@pytest.mark.parametrize('nh,d,d_e,K,nfeats,efeats,form,fuse', STREAM_CASES,
                         ids=[f"h{c[0]}-d{c[1]}-e{c[2]}{'-n' if c[4] else ''}{'-E' if c[5] else ''}-{c[6]}{'-f' if c[7] else ''}"
                              for c in STREAM_CASES])
def test_stream_step_heads_and_widths(nh, d, d_e, K, nfeats, efeats, form, fuse):
    model, orc, st = build(nh, d, d_e, nfeats=nfeats, efeats=efeats, K=K, seed=d + nh)
    assert model.model_struct().d_e == (d_e if efeats else d)
    if fuse:
        model.fuse_attention()
        assert model.model_struct().attn_fused
    if form != 'lazy':
        model.eager_updates()
    _run_stream(model, orc, st, K, form)


@pytest.mark.parametrize('form', ['lazy', 'eager-fused-lean'])
def test_two_layer_stream_step_at_four_heads(form):
    """--n_layers 2 at 4 heads with 4-wide edges: the outer layer reads the inner layer's embeddings as key rows"""
    model, orc, st = build(4, 32, 4, K=5, L=2, seed=7)
    if 'eager' in form:
        model.eager_updates()
        model.fuse_attention()
    _run_stream(model, orc, st, 5, 'eager-lean' if 'lean' in form else 'lazy', L=2)


# ------------------------------------------------------------------------------ sequence restarter, odd head width
@pytest.mark.parametrize('nh,d,d_e,H', [
    (4, 32, 4, 12),    # head width (4*32 + 4)/4 = 33: k_seq_scores<32,false>
    (4, 32, 4, 40),    # <32,false> + <64,false> (histories of 33 .. 64 events take the second launch)
    (4, 8, 12, 80),    # head width 11: <128,false>
])
def test_seq_restarter_with_odd_head_width(nh, d, d_e, H):
    """SeqRestarter forward (restart path) on nodes whose histories fill every row class, at times with no, some and
    all of the stream behind them; restart() leaves the oracle's memories"""
    from test_hip_parity import compare_state_with_oracle
    assert (4 * d + d_e) % nh == 0 and ((4 * d + d_e) // nh) % 2 == 1
    model, orc, st = build(nh, d, d_e, restarter='seq', H=H, E=600, K=5, seed=H)
    n_nodes = st['n_nodes']
    deg = np.bincount(np.concatenate([st['src'], st['dst']]), minlength=n_nodes)
    assert deg.max() > H and (deg[1:] <= 32).any()   # long and short histories in the same call
    tmax = float(np.float32(st['ts'].max()))
    nids = np.arange(1, n_nodes, dtype=np.int64)
    for t in (0.0, 0.5 * tmax, tmax + 1.0):
        ts = np.full(len(nids), np.float32(t), dtype=np.float32)
        with torch.no_grad():
            hl, hr, pt = model.restarter_fn(torch.from_numpy(nids).to(dev()), torch.from_numpy(ts).to(dev()))
        rl, rr, rp = orc.restarter_forward(nids, ts)
        assert_close(hl.cpu().numpy(), rl.detach().numpy(), 'restart h_left', TOL)
        assert_close(hr.cpu().numpy(), rr.detach().numpy(), 'restart h_right', TOL)
        np.testing.assert_array_equal(pt.cpu().numpy(), rp.numpy())
    ts = np.full(len(nids), np.float32(tmax + 1.0), dtype=np.float32)
    model.restart(torch.from_numpy(nids).to(dev()), torch.from_numpy(ts).to(dev()))
    orc.restart(nids, ts)
    compare_state_with_oracle(model, orc)


# ------------------------------------------------------------------------------ training step, every k_attn_core_bwd
@pytest.mark.parametrize('nh,d,d_e,restarter,H', [
    (2, 64, 20, 'static', None),   # k_attn_core_bwd<2,1>
    (2, 320, 320, 'static', None),   # <2,2>: 256 < d <= 512
    (1, 16, 16, 'static', None),   # <1,1>
    (4, 32, 4, 'seq', 40),         # <4,1>; restarter backward at head width 33: k_seq_scores_bwd<32,false> + <64,false>
])
def test_training_step_heads_and_widths(nh, d, d_e, restarter, H):
    """forward, both losses and every gradient of the mutual-learning step against the oracle's autograd"""
    from oracle import tiger_oracle as O
    from test_hip_train import sync_params
    from test_oracle_golden import grad_err
    from www2023tiger_amd.model.training import TrainBuffers
    B, K = 64, 6
    model, orc, st = build(nh, d, d_e, restarter=restarter, H=H, E=5 * B, K=K, T=400.0, seed=d)
    model.train()
    tb = TrainBuffers(model, B, mutual=True)
    to = lambda x, dt: torch.as_tensor(x).to(dev(), dt)
    long_hist = False
    for b in range(5):
        a = [st[k][b * B:(b + 1) * B] for k in ('src', 'dst', 'neg', 'ts', 'eids')]
        cg = O.collate(orc.graph, a[0], a[1], a[2], a[3], K, restarter, hist_len=H)
        if restarter == 'seq':
            long_hist = long_hist or bool(((cg['rd_hist_nids'] != 0).sum(1) > 32).any())
        sync_params(model, orc)
        c, ml, grads = orc.train_step(*a, cg, lr=1e-3, mutual_coef=1.0)
        tb.sb.load(to(a[0], torch.int64), to(a[1], torch.int64), to(a[2], torch.int64), to(a[3], torch.float64),
                   to(a[4], torch.int64))
        tb.launch()
        assert int(tb.sb.err.item()) == 0
        assert abs(float(tb.losses[0]) - c) < TOL * max(1.0, abs(c)), b
        assert abs(float(tb.losses[1]) - ml) < TOL * max(1.0, abs(ml)), b
        worst = max((grad_err(g_.cpu().numpy(), grads[k].numpy()), k) for k, g_ in tb.grads.items())
        assert worst[0] < 3e-4, (b, worst)
    assert restarter != 'seq' or long_hist   # the 64-row class of the backward really ran


# ------------------------------------------------------------------------------ refusals
REFUSED = [  # (n_head, d, d_e)
    (3, 12, 12),      # head width 2d/3 = 8 passes the width rule; there is no 3-head instance
    (8, 32, 32),      # no 8-head instance
    (4, 172, 172),    # head width 86 is not a multiple of 4
    (4, 320, 4),      # two float4 per lane: 2 heads only
    (2, 516, 4),      # rows wider than 512 floats (training: > NVS * 64)
]


@pytest.mark.parametrize('step', ['stream', 'train'])
@pytest.mark.parametrize('nh,d,d_e', REFUSED, ids=[f'h{c[0]}-d{c[1]}-e{c[2]}' for c in REFUSED])
def test_configurations_outside_the_dispatch_refuse(nh, d, d_e, step):
    """a configuration no kernel instance serves raises from the streaming / training step before anything runs: the
    workspace-size queries already refuse it (no launch reaches the dispatch)"""
    import ctypes as C
    from www2023tiger_amd._lib import lib
    from www2023tiger_amd.model.training import TrainBuffers
    model, _, st = build(nh, d, d_e, E=40, n_u=10, n_i=5, K=5)
    m = model.model_struct()
    assert lib.tg_stream_step_workspace_bytes2(C.byref(m), 20, 1) == 0
    assert lib.tg_temporal_attn_workspace_bytes(C.byref(m), 20) == 0
    a = [st[k][:20] for k in ('src', 'dst', 'neg', 'ts', 'eids')]
    before = model.left_memory.vals.clone(), model.right_memory.vals.clone()
    with pytest.raises((RuntimeError, NotImplementedError), match='unsupported model'):
        if step == 'stream':
            model.stream_step(*a)
        else:
            model.train()
            TrainBuffers(model, 20, mutual=True).launch()
    torch.cuda.synchronize()
    assert torch.equal(before[0], model.left_memory.vals) and torch.equal(before[1], model.right_memory.vals)


# ------------------------------------------------------------------------------ the pre-multiplied weights' blob
@pytest.mark.parametrize('efeats', [True, False], ids=['E', 'noE'])
@pytest.mark.parametrize('nh,d,d_e', [(2, 8, 4), (1, 16, 16), (4, 32, 4)], ids=lambda v: str(v))
def test_fused_blob_has_the_documented_size_and_is_written_whole(nh, d, d_e, efeats):
    """tg_attn_fuse's output (include/tiger_hip.h): [Wqk [nk, d] | gconst [nk] | W1f [d, nk + d] | b1 [d] | c1 [d]] with
    nk = n_head (2 d + d_e), or n_head 2 d without an edge table (the compact form) - tg_attn_fused_floats is exactly
    that, every float of it is written (random weights: none stays NaN) and nothing behind it is touched.  The smallest
    shapes that cover the three head counts, the compact path and d != d_e."""
    import ctypes as C
    from www2023tiger_amd._lib import check, lib, ptr
    from www2023tiger_amd.hip_ops import stream_ptr
    model, _, _ = build(nh, d, d_e, efeats=efeats, E=40, n_u=10, n_i=5, K=5)
    m = model.model_struct()
    nk = nh * (2 * d + d_e) if efeats else nh * 2 * d
    n = int(lib.tg_attn_fused_floats(C.byref(m)))
    assert n == nk * d + nk + d * (nk + d) + 2 * d
    guard = 64
    blob = torch.full((n + guard,), float('nan'), dtype=torch.float32, device=dev())
    nbytes = int(lib.tg_attn_fuse_workspace_bytes(C.byref(m)))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev())
    check(lib.tg_attn_fuse(C.byref(m), ptr(blob), ptr(ws), nbytes, stream_ptr(dev())), 'tg_attn_fuse')
    torch.cuda.synchronize()
    assert bool(torch.isfinite(blob[:n]).all()), int((~torch.isfinite(blob[:n])).sum())
    assert bool(torch.isnan(blob[n:]).all())
    assert lib.tg_attn_tile_applies(C.byref(m)) == 0
