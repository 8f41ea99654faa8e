"""Node classification on the device: the MLP decoder (tg_decoder_fwd / tg_decoder_bwd) against float64 torch,
its dropout masks, the whole-split AUC (tg_roc_auc) against sklearn, eval_node_classification's resident stream
against the literal loop, and the reference's train_supervised.py flow end to end."""
import os
import sys

import numpy as np
import pytest
import torch
from torch import nn

from _util import load, parse_cfg, rel_err
from test_hip_parity import build_hip_model, dev
from test_node_task_host import dropout_keep, torch_decoder

pytestmark = pytest.mark.gpu


def _mlp(d, p, seed=0):
    from www2023tiger_amd.model.basic_modules import MLP
    torch.manual_seed(seed)
    return MLP(d, dropout=p).to(dev())


def _reference64(m, x, masks=None, p=0.0):
    """float64 torch with the module's weights; masks = (keep1 [n, 80], keep2 [n, 10]) or None"""
    w = [t.detach().double().requires_grad_(True) for t in m.params()]
    x64 = x.detach().double().requires_grad_(True)
    a = torch.relu(x64 @ w[0].T + w[1])
    if masks is not None:
        a = a * torch.as_tensor(masks[0], device=x.device, dtype=torch.float64) / (1 - p)
    a = torch.relu(a @ w[2].T + w[3])
    if masks is not None:
        a = a * torch.as_tensor(masks[1], device=x.device, dtype=torch.float64) / (1 - p)
    y = (a @ w[4].T + w[5]).squeeze(-1)
    return y, x64, w


def _grads(m, x):
    return [t.grad.detach().clone() for t in m.params()] + [x.grad.detach().clone()]


@pytest.mark.parametrize('d', [8, 100, 172, 256, 512])
@pytest.mark.parametrize('n', [1, 63, 100, 1000, 5000])
def test_decoder_matches_float64_torch(d, n):
    m = _mlp(d, 0.0, seed=d + n)
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, d, generator=g).to(dev()).requires_grad_(True)
    dy = torch.randn(n, generator=g).to(dev())
    y = m(x)
    assert y.shape == (n,)
    y.backward(dy)
    y64, x64, w64 = _reference64(m, x)
    y64.backward(dy.double())
    assert rel_err(y.detach().cpu(), y64.detach().cpu()) < 1e-5
    for name, got, ref in zip(('w1', 'b1', 'w2', 'b2', 'w3', 'b3', 'x'), _grads(m, x), [t.grad for t in w64] + [x64.grad]):
        assert rel_err(got.cpu(), ref.cpu()) < 1e-5, name
    with torch.no_grad():  # inference: no pre-activations kept, same logits
        assert torch.equal(m(x), y.detach())


def test_decoder_gradients_are_deterministic():
    m = _mlp(172, 0.0)
    x = torch.randn(5000, 172, device=dev())
    runs = []
    for _ in range(2):
        m.zero_grad()
        xx = x.clone().requires_grad_(True)
        m(xx).square().sum().backward()
        runs.append(_grads(m, xx))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


@pytest.mark.parametrize('p', [0.1, 0.3])
def test_decoder_dropout(p):
    n, d = 1000, 100
    m = _mlp(d, p).train()
    x = torch.randn(n, d, device=dev()).requires_grad_(True)
    dy = torch.randn(n, device=dev())
    y = m(x)
    y.backward(dy)
    seed, counter = (int(v) for v in m._rng.cpu())
    assert counter == 1  # one tick per training forward
    keep1 = dropout_keep(seed, 0, 5, np.arange(n * 80), p).reshape(n, 80)
    keep2 = dropout_keep(seed, 0, 6, np.arange(n * 10), p).reshape(n, 10)
    for k in (keep1, keep2):
        assert abs(1 - k.mean() - p) < 0.02
    # the forward applied exactly these masks, scaled by 1 / (1 - p), and the backward used them again
    y64, x64, w64 = _reference64(m, x, (keep1, keep2), p)
    y64.backward(dy.double())
    assert rel_err(y.detach().cpu(), y64.detach().cpu()) < 1e-5
    for name, got, ref in zip(('w1', 'b1', 'w2', 'b2', 'w3', 'b3', 'x'), _grads(m, x), [t.grad for t in w64] + [x64.grad]):
        assert rel_err(got.cpu(), ref.cpu()) < 1e-5, name
    # without the masks the result is different: they did something
    assert rel_err(y.detach().cpu(), _reference64(m, x)[0].detach().cpu()) > 1e-3
    with torch.no_grad():
        y2 = m(x)  # the next training forward draws new masks
        assert not torch.equal(y2, y.detach())
        assert int(m._rng[1]) == 2
        m.eval()  # no dropout in eval(), and no tick
        y3 = m(x)
        assert int(m._rng[1]) == 2
    assert rel_err(y3.cpu(), _reference64(m, x)[0].detach().cpu()) < 1e-5


def test_decoder_fallbacks_match_the_kernel():
    """CPU tensors and widths the kernel does not take run `fn` on plain torch"""
    m = _mlp(6, 0.0)
    x = torch.randn(50, 6, device=dev())
    assert not m.hip_ok(x)
    assert torch.allclose(m(x), m.fn(x).squeeze(-1))
    m = _mlp(16, 0.0)
    x = torch.randn(50, 16)
    out_gpu = m(x.to(dev())).cpu()
    assert rel_err(m.cpu()(x).detach(), out_gpu.detach()) < 1e-5


def _auc(scores, labels):
    from www2023tiger_amd.eval_utils import roc_auc
    return roc_auc(torch.as_tensor(scores).to(dev()), torch.as_tensor(labels).to(dev()))


@pytest.mark.parametrize('n', [2, 1000, 2 ** 20 + 7])
def test_roc_auc_matches_sklearn(n):
    from sklearn.metrics import roc_auc_score
    rs = np.random.RandomState(n % 1000)
    lab = (rs.uniform(size=n) < 0.5).astype(np.float32)
    lab[0], lab[-1] = 1, 0
    s = rs.normal(size=n).astype(np.float32)
    assert abs(_auc(s, lab) - roc_auc_score(lab, s)) < 1e-12
    # heavy ties: saturated sigmoids and duplicated values across the classes
    t = (1 / (1 + np.exp(-8 * rs.normal(size=n)))).astype(np.float32)
    t[::3] = np.float32(1.0)
    t[1::7] = np.float32(0.0)
    t[n // 2:] = t[: n - n // 2]
    assert abs(_auc(t, lab) - roc_auc_score(lab, t)) < 1e-12
    # negative zero equals zero
    z = np.where(rs.uniform(size=n) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    assert abs(_auc(z, lab) - roc_auc_score(lab, z)) < 1e-12


def test_roc_auc_imbalanced_nonfinite_and_one_class():
    from sklearn.metrics import roc_auc_score
    from www2023tiger_amd._lib import lib, ptr
    from www2023tiger_amd.hip_ops import stream_ptr
    rs = np.random.RandomState(1)
    n = 100000
    lab = (rs.uniform(size=n) < 0.01).astype(np.float32)  # 1 % positives
    s = (rs.normal(size=n) + lab).astype(np.float32)
    assert abs(_auc(s, lab) - roc_auc_score(lab, s)) < 1e-12
    s[10:20] = np.nan
    s[30] = np.inf
    s[40] = -np.inf
    with pytest.raises(ValueError, match='non-finite'):
        _auc(s, lab)
    # the kernel itself: counted, and left out of the score
    ws = torch.empty(int(lib.tg_roc_auc_workspace_bytes(n)), dtype=torch.uint8, device=dev())
    auc = torch.zeros(1, dtype=torch.float64, device=dev())
    bad = torch.zeros(1, dtype=torch.int32, device=dev())
    st, lt = torch.from_numpy(s).to(dev()), torch.from_numpy(lab).to(dev())
    assert lib.tg_roc_auc(n, ptr(st), ptr(lt), ptr(auc), ptr(bad), ptr(ws), ws.numel(), stream_ptr(dev())) == 0
    ok = np.isfinite(s)
    assert int(bad.item()) == 12
    assert abs(float(auc.item()) - roc_auc_score(lab[ok], s[ok])) < 1e-12
    with pytest.raises(ValueError, match='one class'):
        _auc(np.arange(10, dtype=np.float32), np.ones(10, dtype=np.float32))
    with pytest.raises(ValueError, match='one class'):
        _auc(np.arange(10, dtype=np.float32), np.zeros(10, dtype=np.float32))


def test_eval_node_classification_resident_equals_the_loop(monkeypatch):
    """eval_node_classification over a BatchLoader takes the resident stream of eval_edge_prediction with the decoder
    as a per-batch hook.  With the model's own forms (TG_EVAL_STREAM=0) logits and AUC equal the per-batch loop's bit
    for bit, and the memories after the pass too; by default (eager updates, pre-multiplied weights) they agree to
    float32 rounding.  The loop's AUC is sklearn's on its predictions, and the reference's loop restated with a torch
    decoder gives it too.  Full batches plus a ragged tail; labels drawn at random."""
    from sklearn.metrics import roc_auc_score
    from www2023tiger_amd import eval_utils
    from www2023tiger_amd.data.data_loader import BatchLoader, InteractionData
    z = load('eval_static_ll_d16')
    cfg = parse_cfg(z)
    model, _, coll = build_hip_model(z, cfg, dropout=0.0)
    B = cfg['B']
    n = 12 * B + B // 3
    labels = (np.random.RandomState(3).uniform(size=n) < 0.4).astype(np.int64)
    mk = lambda: BatchLoader(InteractionData(z['src'][:n], z['dst'][:n], z['ts'][:n], z['eids'][:n], labels, seed=5,
                                             eval=True), B, coll)
    decoder = _mlp(cfg['d'], 0.1)
    taken, seen = [], []
    real_res, real_auc = eval_utils._eval_resident, eval_utils.roc_auc
    monkeypatch.setattr(eval_utils, '_eval_resident', lambda *a, **k: (taken.append(1), real_res(*a, **k))[1])
    monkeypatch.setattr(eval_utils, 'roc_auc', lambda s, l: (seen.append((s.cpu().clone(), l.cpu().clone())),
                                                             real_auc(s, l))[1])
    out = {}
    for form, env in (('loop', dict(TG_EVAL_RESIDENT='0')), ('resident', dict(TG_EVAL_RESIDENT='1', TG_EVAL_STREAM='0')),
                      ('stream', dict(TG_EVAL_RESIDENT='1', TG_EVAL_STREAM='1'))):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        model.reset()
        auc = eval_utils.eval_node_classification(model, decoder, mk(), dev())
        assert not decoder.training
        out[form] = (auc, seen[-1][0], seen[-1][1], model.left_memory.vals.clone(), model.right_memory.vals.clone(),
                     model.left_memory.update_ts.clone(), model.msg_store.node_msg_vals.clone())
    assert len(taken) == 2
    np.testing.assert_array_equal(out['loop'][2].numpy(), labels.astype(np.float32))
    assert torch.equal(out['loop'][2], out['resident'][2]) and torch.equal(out['loop'][2], out['stream'][2])
    assert out['loop'][0] == out['resident'][0]
    assert torch.equal(out['loop'][1], out['resident'][1])
    for a, b in zip(out['loop'][3:], out['resident'][3:]):
        assert torch.equal(a, b)
    assert abs(out['loop'][0] - out['stream'][0]) < 2e-4
    assert rel_err(out['stream'][1].numpy(), out['loop'][1].numpy()) < 1e-4
    assert torch.equal(out['loop'][5], out['stream'][5])
    for a, b in zip(out['loop'][3:], out['stream'][3:]):
        assert rel_err(b.cpu().numpy(), a.cpu().numpy()) < 1e-5
    assert abs(out['loop'][0] - roc_auc_score(labels, out['loop'][1].numpy())) < 1e-12
    # the reference's 15 lines (eval_utils.py:81-98) with a plain torch decoder holding the same weights
    ref_dec = torch_decoder(cfg['d']).to(dev())
    ref_dec.load_state_dict(decoder.state_dict())
    ref_dec.eval()
    model.reset()
    model.eval()
    preds, trues = [], []
    with torch.no_grad():
        for src_ids, dst_ids, neg_dst_ids, ts, eids, lab, comp_graph in mk():
            bs = len(src_ids)
            _, h, *_ = model.contrast_learning(src_ids.long().to(dev()), dst_ids.long().to(dev()),
                                               neg_dst_ids.long().to(dev()), ts.float().to(dev()), eids.long().to(dev()),
                                               comp_graph)
            preds.append(ref_dec(h[:bs]).sigmoid().cpu().numpy())
            trues.append(lab.numpy())
    model._poll_train_errors()
    ref_auc = roc_auc_score(np.concatenate(trues), np.concatenate(preds))
    assert abs(ref_auc - out['loop'][0]) < 2e-4


def test_node_classification_recipe_end_to_end(tmp_path):
    """examples/link_prediction.run writes a checkpoint on toy JODIE files; examples/node_classification.run (the
    reference's train_supervised.py flow) trains the decoder on it for two epochs against labels that follow a node
    property: the loss falls and the test AUC is a finite number in [0, 1]."""
    from test_input_side import write_files
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, 'examples'))
    import link_prediction as lp
    import node_classification as nc
    z0 = load('input_side')
    z = {k: z0[k] for k in ('src', 'dst', 'ts')}
    z['labels'] = (z['src'] % 3 == 0).astype(np.int64)  # a property of the source node
    write_files(str(tmp_path), 'toy', z, with_feats=False)
    ckpt = str(tmp_path / 'model.pt')
    kw = dict(seed=0, bs=100, dim=8, n_neighbors=4, hist_len=6, restarter_type='static')
    lp.run('toy', str(tmp_path), n_epochs=1, lr=1e-3, restart_prob=0.0, ckpt_path=ckpt, **kw)
    out, encoder, decoder = nc.run('toy', str(tmp_path), ckpt, n_epochs=2, lr=1e-2, dropout=0.1, **kw)
    e0, e1 = out['epochs']
    assert np.isfinite([e0['loss'], e1['loss']]).all() and e1['loss'] < e0['loss']
    assert 0.0 <= out['test_auc'] <= 1.0
    assert decoder.hip_ok(torch.zeros(1, encoder.nfeat_dim, device=dev()))  # the fused kernels did the work
    out2, _, _ = nc.run('toy', str(tmp_path), ckpt, n_epochs=2, lr=1e-2, dropout=0.1, use_valid=True, patience=1, **kw)
    assert 0.0 <= out2['test_auc'] <= 1.0
