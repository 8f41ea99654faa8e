"""The decoder's tile loops and chunk edges, and the AUC's tile edges.

tg_decoder_fwd launches at most DEC_FWD_TILES row tiles and tg_decoder_bwd at most DEC_BWD_PARTS partial-sum workgroups;
past n = 65 536 / 16 384 rows a workgroup takes a second tile, with W1 staged in LDS (d <= DEC_KC: once; beyond: per tile
and chunk) and the partial sums kept in registers across tiles.  The C entries are called directly: guard words stand
behind every output and the workspace starts as 0xFF bytes of exactly the size asked for.  The reference is float64
torch (_reference64 of test_hip_node_task.py).

Bounds.  The forward keeps rel_err < 1e-5: a row's arithmetic does not depend on n.  The weight gradients are float32 sums
over up to 65 553 rows in a fixed order, so their bound is derived from the reference alone: _cap_ref.decoder_emulation
evaluates the same sums in float32 on the CPU in the documented order, its rel_err against float64 is measured, and the
kernel is allowed max(1e-5, 4 x that) - the factor 4 covers fused multiply-add against separate rounding.  For dW1 and dx,
in addition, no element may be off by more than 4 x the emulation's own worst element: a single dropped row shows there.
Inputs keep every pre-activation 1e-4 away from zero (decoder_inputs), so float32 and float64 agree on every ReLU.

Measured rel_err, emulation | kernel on an MI355X, of the row-count cases (the d, n edge cases: all below 8e-7):
       n    d    p              dw1              db1              dw2              db2              dw3              db3               dx
   16384    8    0  2.3e-06|2.2e-06  6.1e-07|6.1e-07  3.7e-07|3.6e-07  6.3e-07|6.3e-07  4.0e-07|1.8e-07  3.1e-07|3.1e-07  6.6e-08|6.6e-08
   16384  196    0  4.0e-06|4.5e-06  5.2e-07|5.2e-07  7.1e-07|6.7e-07  1.9e-07|1.9e-07  9.5e-07|6.7e-07  3.3e-07|3.3e-07  2.7e-08|2.7e-08
   16385    8    0  3.8e-06|4.0e-06  2.8e-07|2.8e-07  3.8e-07|3.4e-07  3.6e-07|3.6e-07  4.1e-07|2.6e-07  1.6e-05|1.6e-05  5.7e-08|5.7e-08
   16385  196    0  2.8e-06|3.0e-06  6.7e-07|6.7e-07  3.4e-07|3.5e-07  1.2e-07|1.2e-07  1.2e-07|2.6e-07  7.4e-08|7.4e-08  3.7e-08|3.7e-08
   32833    8    0  4.0e-06|3.9e-06  4.5e-07|4.5e-07  3.7e-07|4.4e-07  4.2e-07|4.2e-07  2.6e-07|2.4e-07  4.8e-07|4.8e-07  7.7e-08|7.7e-08
   32833  196    0  3.1e-06|3.0e-06  4.6e-07|4.6e-07  4.9e-07|4.0e-07  1.4e-07|1.4e-07  4.2e-07|4.2e-07  2.4e-07|2.4e-07  1.9e-08|1.9e-08
   65553    8    0  5.3e-06|5.5e-06  3.1e-07|3.1e-07  4.5e-07|3.7e-07  1.7e-07|1.7e-07  3.4e-07|1.4e-07  3.9e-07|3.9e-07  7.3e-08|7.3e-08
   65553  196    0  6.1e-06|5.9e-06  9.2e-07|9.2e-07  4.7e-07|4.4e-07  2.0e-07|2.0e-07  2.9e-07|3.1e-07  6.2e-08|6.2e-08  3.0e-08|3.0e-08
   65553    8  0.3  2.7e-06|2.8e-06  7.0e-07|7.0e-07  3.7e-07|3.5e-07  2.2e-07|2.2e-07  1.2e-07|2.2e-07  3.9e-07|3.9e-07  1.2e-07|1.2e-07
(n = 16 385, d = 8: the db3 reference, the sum of dy, is -1.5 where the sum of |dy| is 13 117 - both stand at 1.6e-5.)
"""
import ctypes as C

import numpy as np
import pytest
import torch

import _cap_ref as R
from _util import rel_err
from test_hip_node_task import _auc, _mlp, _reference64
from test_node_task_host import dropout_keep

pytestmark = pytest.mark.gpu

GUARD = 0x5A          # guard bytes behind every output
GUARD_BYTES = 256
NAMES = R.GRAD_NAMES + ('x',)


def dev():
    return torch.device('cuda', 0)


def _guarded(nbytes, fill=GUARD):
    """uint8 [nbytes + GUARD_BYTES] filled with `fill`; nbytes is a multiple of 4"""
    return torch.full((nbytes + GUARD_BYTES,), fill, dtype=torch.uint8, device=dev())


def _view(buf, shape):
    n = int(np.prod(shape))
    return buf[:4 * n].view(torch.float32).reshape(shape)


def _intact(buf, nbytes, fill=GUARD):
    return bool((buf[nbytes:] == fill).all())


def _module(d, p, params):
    m = _mlp(d, p)
    with torch.no_grad():
        for t, a in zip(m.params(), params):
            t.copy_(torch.from_numpy(a))
    return m


def raw_forward(m, x, p=0.0, key=None, keep=True):
    """tg_decoder_fwd -> (y, z1, z2); z1 / z2 are None with keep=False (inference).  Guard bytes are checked."""
    from www2023tiger_amd._lib import TgDecoder, lib, ptr
    from www2023tiger_amd.hip_ops import stream_ptr
    n, d = x.shape
    shapes = [(n,), (n, R.DEC_H1), (n, R.DEC_H2)] if keep else [(n,)]
    bufs = [_guarded(4 * int(np.prod(s))) for s in shapes]
    outs = [_view(b, s) for b, s in zip(bufs, shapes)] + [None, None]
    w = TgDecoder(*(ptr(t) for t in m.params()))
    rc = lib.tg_decoder_fwd(n, ptr(x), d, C.byref(w), float(p), ptr(key), ptr(outs[0]), ptr(outs[1]), ptr(outs[2]),
                            stream_ptr(dev()))
    torch.cuda.synchronize()
    assert rc == 0
    for b, s, nm in zip(bufs, shapes, ('y', 'z1', 'z2')):
        assert _intact(b, 4 * int(np.prod(s))), f'{nm}: bytes behind the array were written'
    return outs[0], outs[1], outs[2]


def raw_backward(m, x, z1, z2, dy, p=0.0, key=None):
    """tg_decoder_bwd -> dict(w1 .. b3, x): workspace of exactly tg_decoder_bwd_workspace_bytes, 0xFF at the start"""
    from www2023tiger_amd._lib import TgDecoder, lib, ptr
    from www2023tiger_amd.hip_ops import stream_ptr
    n, d = x.shape
    shapes = [tuple(t.shape) for t in m.params()] + [(n, d)]
    bufs = [_guarded(4 * int(np.prod(s))) for s in shapes]
    outs = [_view(b, s) for b, s in zip(bufs, shapes)]
    nbytes = int(lib.tg_decoder_bwd_workspace_bytes(n, d))
    assert nbytes == 4 * (n * R.DEC_H1 + min(-(-n // R.DEC_ROWS), R.DEC_BWD_PARTS) * R.DEC_PART)
    ws = _guarded(nbytes, 0xFF)
    w, g = TgDecoder(*(ptr(t) for t in m.params())), TgDecoder(*(ptr(t) for t in outs[:6]))
    rc = lib.tg_decoder_bwd(n, ptr(x), d, C.byref(w), float(p), ptr(key), ptr(z1), ptr(z2), ptr(dy), C.byref(g), ptr(outs[6]),
                            ptr(ws), nbytes, stream_ptr(dev()))
    torch.cuda.synchronize()
    assert rc == 0
    for b, s, nm in zip(bufs, shapes, NAMES):
        assert _intact(b, 4 * int(np.prod(s))), f'd{nm}: bytes behind the array were written'
    assert _intact(ws, nbytes, 0xFF), 'bytes behind the workspace were written'
    return dict(zip(NAMES, outs))


def reference(m, x, dy, masks=None, p=0.0):
    """float64 torch -> dict(y, w1 .. b3, x) of numpy arrays"""
    y64, x64, w64 = _reference64(m, x, masks, p)
    y64.backward(dy.double())
    out = {nm: t.grad.cpu().numpy() for nm, t in zip(NAMES, w64 + [x64])}
    out['y'] = y64.detach().cpu().numpy()
    return out


def check_forward(y, ref):
    e = rel_err(y.cpu().numpy(), ref['y'])
    assert e < 1e-5, ('y', e)
    return e


def check_backward(got, ref, emu, what):
    """-> {name: (emulation rel_err, kernel rel_err)}, asserted as the module's docstring says"""
    seen = {}
    for nm in NAMES:
        g, r, e = got[nm].cpu().numpy(), ref[nm], emu['dx' if nm == 'x' else nm]
        assert g.shape == r.shape == e.shape, nm
        seen[nm] = (rel_err(e, r), rel_err(g, r))
    print(what, ' '.join(f'd{nm} {a:.1e}|{b:.1e}' for nm, (a, b) in seen.items()))
    for nm in NAMES:
        g, r, e = got[nm].cpu().numpy(), ref[nm], emu['dx' if nm == 'x' else nm]
        bound = max(1e-5, 4 * seen[nm][0])
        assert seen[nm][1] <= bound, (what, nm, seen[nm], bound)
        if nm in ('w1', 'x'):
            off, emu_off = R.worst(g, r), R.worst(e, r)
            assert off <= bound * np.abs(r).max(), (what, nm, 'worst element', off, bound * np.abs(r).max())
            assert off <= 4 * emu_off, (what, nm, 'worst element', off, 'emulation', emu_off)
    return seen


def run_case(n, d, p=0.0, seed=None):
    """forward (training and inference form) and backward of one (n, d) through the C entries against float64 torch"""
    key, masks = None, None
    if p > 0:
        seed_, counter = 1234567, 3
        key = torch.tensor([seed_, counter], dtype=torch.int64, device=dev())
        # the mask index is row * 80 + col (row * 10 + col): it does not depend on which pass took the row
        masks = (dropout_keep(seed_, counter, 5, np.arange(n * R.DEC_H1), p).reshape(n, R.DEC_H1),
                 dropout_keep(seed_, counter, 6, np.arange(n * R.DEC_H2), p).reshape(n, R.DEC_H2))
    x_h, dy_h, params = R.decoder_inputs(n, d, n + d if seed is None else seed, masks[0] if masks else None, p)
    m = _module(d, p, params)
    x, dy = torch.from_numpy(x_h).to(dev()), torch.from_numpy(dy_h).to(dev())
    ref = reference(m, x, dy, masks, p)
    y, z1, z2 = raw_forward(m, x, p, key)
    check_forward(y, ref)
    y_inf, _, _ = raw_forward(m, x, p, key, keep=False)
    assert torch.equal(y_inf, y), 'the inference form (no pre-activations kept) gives other logits'
    return m, x, dy, key, masks, params, ref, (y, z1, z2)


# ---- forward: second and third tile per workgroup -----------------------------------------------------------------------
@pytest.mark.parametrize('d', R.DEC_D_TILES)
@pytest.mark.parametrize('n', R.DEC_FWD_N)
def test_forward_past_the_tile_cap(n, d):
    """n = 65 536: every workgroup one tile.  65 536 + 17: workgroup 0 takes a second tile whose wavefront 0 is full,
    wavefront 1 holds one row, wavefronts 2 and 3 are empty.  2 * 65 536 + 64 * 3 + 1: a third pass of four tiles, the last
    with one row.  The saved pre-activations are compared too."""
    m, x, dy, key, masks, params, ref, (y, z1, z2) = run_case(n, d)
    w = [t.astype(np.float64) for t in params]
    z1_64 = x.cpu().numpy().astype(np.float64) @ w[0].T + w[1]
    z2_64 = np.maximum(z1_64, 0) @ w[2].T + w[3]
    assert rel_err(z1.cpu().numpy(), z1_64) < 1e-5 and rel_err(z2.cpu().numpy(), z2_64) < 1e-5
    assert np.array_equal(z1.cpu().numpy() > 0, z1_64 > 0) and np.array_equal(z2.cpu().numpy() > 0, z2_64 > 0)


def test_module_under_no_grad_equals_the_training_forward_past_the_cap():
    n, d = R.DEC_FWD_N[1], 172
    x_h, _, params = R.decoder_inputs(n, d, seed=5)
    m = _module(d, 0.0, params)
    x = torch.from_numpy(x_h).to(dev()).requires_grad_(True)
    y = m(x)
    assert y.requires_grad
    with torch.no_grad():
        assert torch.equal(m(x), y.detach())


# ---- backward: partial sums carried over tiles ----------------------------------------------------------------------------
@pytest.mark.parametrize('d', [8, 196])
@pytest.mark.parametrize('n', R.DEC_BWD_N)
def test_backward_past_the_partial_sum_cap(n, d):
    """n = 16 384: every workgroup one tile.  + 1: workgroup 0 adds a one-row tile to its sums.  2 * 16 384 + 65: two full
    passes and a third of two tiles, one of them a single row.  65 536 + 17: five tiles for workgroup 0, four for the rest."""
    m, x, dy, key, masks, params, ref, (y, z1, z2) = run_case(n, d)
    got = raw_backward(m, x, z1, z2, dy)
    emu = R.decoder_emulation(x.cpu().numpy(), dy.cpu().numpy(), params)
    check_backward(got, ref, emu, f'n={n} d={d}')


def test_backward_twice_gives_the_same_bits():
    n, d = R.DEC_BWD_N[2], 196
    m, x, dy, key, masks, params, ref, (y, z1, z2) = run_case(n, d)
    a = raw_backward(m, x, z1, z2, dy)
    b = raw_backward(m, x, z1, z2, dy)
    for nm in NAMES:
        assert torch.equal(a[nm], b[nm]), nm


def test_dropout_masks_do_not_depend_on_the_pass():
    """p = 0.3 at n = 65 536 + 17 against the host-mirror masks: rows of the second to fifth tile of a workgroup take the
    mask of their own row index"""
    n, d, p = R.DEC_FWD_N[1], 8, 0.3
    m, x, dy, key, masks, params, ref, (y, z1, z2) = run_case(n, d, p)
    for k in masks:
        assert abs(1 - k.mean() - p) < 0.01
    got = raw_backward(m, x, z1, z2, dy, p, key)
    emu = R.decoder_emulation(x.cpu().numpy(), dy.cpu().numpy(), params, masks, p)
    check_backward(got, ref, emu, f'n={n} d={d} p={p}')
    assert rel_err(y.cpu().numpy(), reference(m, x, dy)['y']) > 1e-3   # without the masks the result is different


# ---- chunk and tile edges at small n -----------------------------------------------------------------------------------
@pytest.mark.parametrize('n', R.DEC_N_EDGES)
@pytest.mark.parametrize('d', R.DEC_D_EDGES)
def test_chunk_and_tile_edges(d, n):
    """d around the W1 chunk (DEC_KC = 192 columns) and its multiples, n around a wavefront's 16 rows and a tile's 64"""
    m, x, dy, key, masks, params, ref, (y, z1, z2) = run_case(n, d)
    got = raw_backward(m, x, z1, z2, dy)
    emu = R.decoder_emulation(x.cpu().numpy(), dy.cpu().numpy(), params)
    check_backward(got, ref, emu, f'n={n} d={d}')


# ---- AUC: tile edges ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', R.AUC_N)
def test_roc_auc_at_the_tile_edges(n):
    """AUC_TILE - 1, AUC_TILE, AUC_TILE + 1 and 2 AUC_TILE + 1 keys: the last tile of the radix passes holds one key.
    Scores over both signs, the largest finite float, denormals, both zeros and heavy ties."""
    from sklearn.metrics import roc_auc_score
    s, lab = R.auc_scores(n, seed=n)
    with np.errstate(invalid='ignore'):   # (sklearn's finiteness check adds the scores up: max - max)
        want = roc_auc_score(lab, s)
    assert abs(_auc(s, lab) - want) < 1e-12
    # the two orderings with AUC exactly 1 and exactly 0: every positive above / below every negative
    order = ((np.arange(n) - n // 2) * 0.25).astype(np.float32)   # n distinct scores, ascending, both signs
    order[0], order[-1] = -np.finfo(np.float32).max, np.finfo(np.float32).max
    up = (np.arange(n) >= n // 3).astype(np.float32)
    perm = np.random.RandomState(n + 1).permutation(n)
    assert _auc(order[perm], up[perm]) == 1.0 == roc_auc_score(up[perm], order[perm])
    assert _auc(order[perm], 1 - up[perm]) == 0.0 == roc_auc_score(1 - up[perm], order[perm])
