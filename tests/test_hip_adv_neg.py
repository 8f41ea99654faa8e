"""Historical / inductive negative sampling on the device (csrc/tg_adv.hip): the pair index and the sampler against
their host twins bit for bit, AdversarialEdgeSampler's device and host paths, and link evaluation on `hist`
negatives through the resident stream against the per-batch loop."""
import os
import sys

import numpy as np
import pytest
import torch

from _util import load, parse_cfg
from test_adv_neg_host import chunk_windows, golden, sampler
from test_hip_parity import build_hip_model, dev

pytestmark = pytest.mark.gpu


def _streams():
    """the fixture stream; a Wikipedia-shaped synthetic stream (popular sources with thousands of entries); one source
    with more than 10^5 out-entries"""
    import bench
    z = golden()
    wiki = bench.make_stream(8227, 1000, 157474, 2.68e6, seed=0, with_efeats=False)
    rs = np.random.RandomState(7)
    E = 150000
    src = np.where(rs.uniform(size=E) < 0.8, 1, rs.randint(2, 200, E)).astype(np.int64)
    dst = rs.randint(200, 700, E).astype(np.int64)
    ts = np.floor(np.sort(rs.uniform(0, 1e5, E)))
    return {'fixture': (z['src'], z['dst'], z['ts']), 'wiki': (wiki['src'], wiki['dst'], wiki['ts']),
            'hub': (src, dst, ts)}


STREAMS = {}


def stream(name):
    if not STREAMS:
        STREAMS.update(_streams())
    return STREAMS[name]


@pytest.mark.parametrize('name', ['fixture', 'wiki', 'hub'])
def test_device_index_equals_the_host_index(name):
    src, dst, ts = stream(name)
    d = sampler(src, dst, ts, 100, 'hist', device=dev())
    h = sampler(src, dst, ts, 100, 'hist', device='cpu')
    dn, df = (t.cpu().numpy() for t in d._index())
    hn, hf = h._index()
    np.testing.assert_array_equal(dn.view(np.uint64), hn.view(np.uint64))
    np.testing.assert_array_equal(df.view(np.uint64), hf.view(np.uint64))
    if name == 'hub':
        indptr = h.graph._host_tcsr()[0]
        assert indptr[2] - indptr[1] > 10 ** 5


@pytest.mark.parametrize('name', ['wiki', 'hub'])
@pytest.mark.parametrize('mode', ['hist', 'ind'])
def test_device_draws_equal_the_host_draws(name, mode):
    """60000 random queries (several grid strides of 16384 wavefronts): out_dst and out_count bit for bit; ids outside
    the graph fall back; a query with t0 > t1 is marked -1 on the device"""
    src, dst, ts = stream(name)
    n_test = len(src) // 7
    d = sampler(src, dst, ts, n_test, mode, seed=17, device=dev())
    h = sampler(src, dst, ts, n_test, mode, seed=17, device='cpu')
    rs = np.random.RandomState(3)
    n = 60000
    q = rs.randint(0, len(src), n)
    srcs = src[q].copy()
    srcs[:50] = rs.randint(len(h.graph._host_tcsr()[0]), 10 ** 7, 50)  # beyond num_node
    srcs[50:60] = -3
    t0 = ts[q].astype(np.float64)
    t1 = ts[np.minimum(q + rs.randint(0, 400, n), len(ts) - 1)].astype(np.float64)
    m = {'hist': 0, 'ind': 1}[mode]
    for counter in (0, 5):
        out_d, cnt_d = d._launch(m, srcs, t0, t1, counter, out_count=True)
        out_h, cnt_h = h._launch(m, srcs, t0, t1, counter, out_count=True)
        np.testing.assert_array_equal(cnt_d, cnt_h)
        np.testing.assert_array_equal(out_d, out_h)
    assert (cnt_h[:60] == 0).all() and (cnt_h > 0).sum() > (n // 4 if mode == 'hist' else 1000)
    assert cnt_h.max() > (64 if mode == 'hist' else 4)
    t0b = t0.copy()
    t0b[100] = t1[100] + 1.0
    out_b, cnt_b = d._launch(m, srcs, t0b, t1, 0, out_count=True)
    assert out_b[100] == -1 and cnt_b[100] == -1
    mask = np.arange(n) != 100
    np.testing.assert_array_equal(out_b[mask], d._launch(m, srcs, t0, t1, 0)[mask])


@pytest.mark.parametrize('mode', ['hist', 'ind'])
@pytest.mark.parametrize('bs', [200, 37])
def test_sampler_device_and_host_paths_agree(mode, bs):
    z = golden()
    n = int(z['n_test'])
    d = sampler(z['src'], z['dst'], z['ts'], n, mode, seed=21, device=dev())
    h = sampler(z['src'], z['dst'], z['ts'], n, mode, seed=21, device='cpu')
    x = d.pre_sample_neg_dsts(n, bs=bs)
    np.testing.assert_array_equal(x, h.pre_sample_neg_dsts(n, bs=bs))
    np.testing.assert_array_equal(x, d.pre_sample_neg_dsts(n, bs=bs))
    vals, off = z[f'{mode}_{bs}_vals'], z[f'{mode}_{bs}_off']
    for q in range(n):
        ref = vals[off[q]:off[q + 1]]
        assert x[q] in (ref if len(ref) else z['full_dst_distinct'])
    t0, t1 = chunk_windows(d.test_ts, bs)
    np.testing.assert_array_equal(d.sample(d.test_srcs[:bs], t0[0], t1[0])[1], h.sample(h.test_srcs[:bs], t0[0], t1[0])[1])


def test_link_eval_on_hist_negatives_resident_equals_the_loop(monkeypatch):
    """eval_edge_prediction on a BatchLoader whose test split carries `hist` negatives: AP / AUC of the resident stream
    (the model's own forms) equal the per-batch loop's, the streaming form agrees within 2e-4 (as for random negatives)"""
    from www2023tiger_amd import eval_utils
    from www2023tiger_amd.data.adversarial import AdversarialEdgeSampler
    from www2023tiger_amd.data.data_loader import BatchLoader, InteractionData
    z = load('eval_static_ll_d16')
    cfg = parse_cfg(z)
    model, _, coll = build_hip_model(z, cfg, dropout=0.0)
    B = cfg['B']
    N = len(z['src'])
    n = min(12 * B + B // 3, N // 2)
    sl = slice(N - n, N)
    adv = AdversarialEdgeSampler(z['src'], z['dst'], z['ts'], z['src'][sl], z['ts'][sl], 'hist', seed=0, device=dev())
    neg = adv.pre_sample_neg_dsts(n)
    assert not np.array_equal(neg, InteractionData(z['src'][sl], z['dst'][sl], z['ts'][sl], z['eids'][sl],
                                                   np.zeros(n, dtype=np.int64), seed=5, eval=True).neg_dst)
    mk = lambda: BatchLoader(InteractionData(z['src'][sl], z['dst'][sl], z['ts'][sl], z['eids'][sl],
                                             np.zeros(n, dtype=np.int64), seed=5, eval=True, neg_dst=neg), B, coll)
    taken = []
    real = eval_utils._eval_resident
    monkeypatch.setattr(eval_utils, '_eval_resident', lambda *a: (taken.append(1), real(*a))[1])
    out = {}
    for form, env in (('loop', dict(TG_EVAL_RESIDENT='0')), ('resident', dict(TG_EVAL_RESIDENT='1', TG_EVAL_STREAM='0')),
                      ('stream', dict(TG_EVAL_RESIDENT='1', TG_EVAL_STREAM='1'))):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        model.reset()
        out[form] = eval_utils.eval_edge_prediction(model, mk(), dev(), restart_mode=False,
                                                    mean_over_n_samples=cfg['chunk'])
    assert len(taken) == 2
    assert out['loop'] == out['resident']
    assert abs(out['loop'][0] - out['stream'][0]) < 2e-4 and abs(out['loop'][1] - out['stream'][1]) < 2e-4


def test_link_prediction_example_with_hist_negatives(tmp_path):
    """examples/link_prediction.run(neg_sample='hist' / 'ind') on toy JODIE files evaluates the test splits on the
    sampler's negatives: finite AP / AUC, different from the random-negative run"""
    from test_input_side import write_files
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, 'examples'))
    import link_prediction as lp
    z0 = load('input_side')
    z = {k: z0[k] for k in ('src', 'dst', 'ts')}
    z['labels'] = np.zeros(len(z['src']), dtype=np.int64)
    write_files(str(tmp_path), 'toy', z, with_feats=False)
    kw = dict(seed=0, bs=100, dim=8, n_neighbors=4, hist_len=6, restarter_type='static', n_epochs=1, lr=1e-3,
              restart_prob=0.0)
    res = {m: lp.run('toy', str(tmp_path), neg_sample=m, **kw)[0] for m in ('rnd', 'hist', 'ind')}
    for m, r in res.items():
        assert all(np.isfinite(r[k]) and 0.0 <= r[k] <= 1.0 for k in ('test_ap', 'test_auc', 'ind_test_ap', 'ind_test_auc')), m
    assert res['hist']['test_ap'] != res['rnd']['test_ap']
