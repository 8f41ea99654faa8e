"""The four-launch streaming step (include/tiger_hip.h: TG_FORM_FC2_DEFERRED): the merger's fc2 as a second product of the
step's last launch, the updater's blend form that reads fc1's output through the folded weights (tg_gru_fc2_fold), and the
snapshot-free STEP 5.
  1. the blend form of k_gru_direct16 alone, against float64 on the host;
  2. two products in one launch, each bit-equal to the same product launched alone, without a rider and with a stand-in
     for the collate rider behind them (the real one runs in every whole-step case of 3-5 where the form is taken);
  3. whole steps on a stream with few nodes against the oracle and against a child process with TG_FC2_DEFER=0;
  4. a graph of three captured steps against three eager steps;
  5. parameters changed in place: the step follows them after train() / eval()."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from _util import assert_close

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
TOL = 1e-4  # the bar of tests/test_hip_timed_form.py


def dev():
    return torch.device('cuda', 0)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


# --------------------------------------------------------------------------------------------- 1. the updater form
def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def _gru64(x, h, w_ih, w_hh, b_ih, b_hh):
    d = h.shape[1]
    gi, gh = x @ w_ih.T + b_ih, h @ w_hh.T + b_hh
    r = _sigmoid(gi[:, :d] + gh[:, :d])
    z = _sigmoid(gi[:, d:2 * d] + gh[:, d:2 * d])
    n = np.tanh(gi[:, 2 * d:] + r * gh[:, 2 * d:])
    return (1.0 - z) * n + z * h


@pytest.mark.parametrize('d', [16, 172])
@pytest.mark.parametrize('P', [1, 47, 48, 49, 97, 1200])
def test_blend_form_of_the_updater_against_float64(P, d):
    """GRU(W_ih, W_hh)(x, W2 t[index] + b2) in float64 against the blend form (memory operand t, folded weights, fifth
    plane) and against the present form of the same kernel fed the float32 rows h = W2 t[index] + b2.  d = 172: a partial
    last k-chunk and a partial 16-column tile; P around the 48-row block; index with repeats, out of order.  P = 1 200 at
    d = 172 is more than 256 blocks of 48 rows: the large instance (k_gru_direct16<6, true>, 64-row blocks), the one a C2
    step runs while its row bound lies above ~1 100.
    Bar: twice the present form's error on the same inputs (the blend form has one rounding fewer on h and one
    re-associated product)."""
    from www2023tiger_amd._lib import check, lib, ptr
    from www2023tiger_amd.hip_ops import stream_ptr
    rs = np.random.RandomState(1000 * d + P)
    xw, nt = 4 * d, 64
    x = rs.standard_normal((P, xw)).astype(np.float32)
    t = np.maximum(rs.standard_normal((nt, d)), 0).astype(np.float32)  # fc1's output is behind a ReLU
    index = rs.randint(0, nt, P).astype(np.int64)
    if P > 2:
        index[1] = index[0]  # a repeat for certain
    w_ih = (rs.standard_normal((3 * d, xw)) / np.sqrt(xw)).astype(np.float32)
    w_hh = (rs.standard_normal((3 * d, d)) / np.sqrt(d)).astype(np.float32)
    b_ih, b_hh = (0.1 * rs.standard_normal(3 * d)).astype(np.float32), (0.1 * rs.standard_normal(3 * d)).astype(np.float32)
    w2 = (rs.standard_normal((d, d)) / np.sqrt(d)).astype(np.float32)
    b2 = (0.1 * rs.standard_normal(d)).astype(np.float32)
    f8 = lambda a: a.astype(np.float64)
    h64 = f8(t)[index] @ f8(w2).T + f8(b2)
    ref = _gru64(f8(x), h64, f8(w_ih), f8(w_hh), f8(b_ih), f8(b_hh))
    whh2 = (f8(w_hh) @ f8(w2)).astype(np.float32)
    bhh2 = (f8(w_hh) @ f8(b2) + f8(b_hh)).astype(np.float32)
    g = {k: _t(v) for k, v in dict(x=x, t=t, index=index, w_ih=w_ih, w_hh=w_hh, b_ih=b_ih, b_hh=b_hh, w2=w2, b2=b2, whh2=whh2,
                                   bhh2=bhh2, h32=h64.astype(np.float32)).items()}
    out_b = torch.full((P, d), float('nan'), dtype=torch.float32, device=dev())
    out_p = torch.full((P, d), float('nan'), dtype=torch.float32, device=dev())
    s = stream_ptr(dev())
    check(lib.tg_gru_blend_fwd(P, ptr(g['x']), xw, ptr(g['t']), ptr(g['index']), d, ptr(g['w_ih']), ptr(g['whh2']), ptr(g['b_ih']),
                               ptr(g['bhh2']), ptr(g['w2']), ptr(g['b2']), ptr(out_b), s), 'tg_gru_blend_fwd')
    check(lib.tg_gru_fwd(P, ptr(g['x']), xw, ptr(g['h32']), d, ptr(g['w_ih']), ptr(g['w_hh']), ptr(g['b_ih']), ptr(g['b_hh']),
                         ptr(out_p), s), 'tg_gru_fwd')
    torch.cuda.synchronize()
    e_blend = float(np.abs(out_b.cpu().numpy() - ref).max())
    e_present = float(np.abs(out_p.cpu().numpy() - ref).max())
    print(f'P={P} d={d}: blend form {e_blend:.3e}, present form {e_present:.3e}')
    assert np.isfinite(e_blend) and e_blend <= 2.0 * e_present, f'blend form {e_blend:.3e} against present form {e_present:.3e}'


# ------------------------------------------------------------------------------------- 2. two products in one launch
def _probe(a, w, bias, c, c_rows=None):
    from www2023tiger_amd import _lib
    from www2023tiger_amd._lib import ptr
    M, K = a.shape
    N = w.shape[0]
    return _lib.TgGemmProbe(m_cap=M, n=N, k=K, a0=ptr(a), a0_ld=K, a0_w=K, w=ptr(w), ldw=K, bias=ptr(bias), alpha=1.0, c=ptr(c),
                            ldc=N, nbatch=1, c_rows=ptr(c_rows) if c_rows is not None else None)


SHAPES2 = [(M1, M2, N) for M1 in (1, 65, 200) for M2 in (3, 192, 3 * 64 + 1) for N in (16, 172, 1032)]
SHAPES2 += [(1100, 192, 1032), (1100, 3 * 64 + 1, 1032)]  # 18 x 17 = 306 tiles of 64 x 64: the first product's 32 x 48 wave tiles


@pytest.mark.parametrize('rider', [0, 24], ids=['no_rider', 'rider'])
@pytest.mark.parametrize('M1,M2,N', SHAPES2, ids=[f'{a}-{b}-{c}' for a, b, c in SHAPES2])
def test_second_product_of_a_launch_is_bit_equal_to_its_own_launch(M1, M2, N, rider):
    """K = 172 (11 chunk slots, the last one partial).  The first product has N columns (M1 = 1 100: more than 256 tiles, the
    wide instance beside the second product's 2 x 2 one), the second N too; the second one also scatters its rows with a non-negative entry in the row list to a second destination (as fc2 stores
    STEP 6's rows).  rider: 24 workgroups of a stand-in behind the two products, as the collate rider sits in the step's
    last launch; every word of its buffer must carry the stamp of the one workgroup that owns it.  Both results, and the
    scattered copies, against the same products through a launch of their own."""
    from www2023tiger_amd import _lib
    from www2023tiger_amd._lib import check, lib, ptr
    from www2023tiger_amd.hip_ops import stream_ptr
    K = 172
    gen = torch.Generator(device='cpu').manual_seed(M1 * 100003 + M2 * 101 + N)
    rnd = lambda *s: torch.randn(*s, generator=gen).to(dev())
    a1, w1, b1 = rnd(M1, K), rnd(N, K), rnd(N)
    a2, w2, b2 = rnd(M2, K), rnd(N, K), rnd(N)
    rows = torch.full((M2,), -1, dtype=torch.int32)
    pick = torch.randperm(M2, generator=gen)[:max(1, M2 // 3)]
    rows[pick] = torch.randperm(M2 + 5, generator=gen)[:pick.numel()].to(torch.int32)  # distinct targets
    rows = rows.to(dev())
    nan = lambda *s: torch.full(s, float('nan'), dtype=torch.float32, device=dev())
    c1, c2, c2b, alone1, alone2 = nan(M1, N), nan(M2, N), nan(M2 + 5, N), nan(M1, N), nan(M2, N)
    n_stamp = 3 * 256 * max(rider, 1) + 77
    stamps = torch.zeros(n_stamp + 16, dtype=torch.int32, device=dev())
    s = stream_ptr(dev())
    hosted = C.c_int32(-1)
    check(lib.tg_debug_gemm2(C.byref(_probe(a1, w1, b1, c1)), C.byref(_probe(a2, w2, b2, c2, rows)), ptr(c2b), C.byref(hosted),
                             ptr(stamps) if rider else None, n_stamp if rider else 0, rider, s), 'tg_debug_gemm2')
    form = C.c_char_p()
    check(lib.tg_debug_gemm(C.byref(_probe(a1, w1, b1, alone1)), C.byref(form), s), 'tg_debug_gemm')
    check(lib.tg_debug_gemm(C.byref(_probe(a2, w2, b2, alone2)), C.byref(form), s), 'tg_debug_gemm')
    torch.cuda.synchronize()
    assert hosted.value == 1
    assert torch.equal(c1, alone1) and torch.equal(c2, alone2)
    assert bool(torch.isfinite(alone1).all()) and bool(torch.isfinite(alone2).all())
    live = torch.nonzero(rows >= 0).flatten()
    assert torch.equal(c2b[rows[live].long()], alone2[live])
    untouched = torch.ones(M2 + 5, dtype=torch.bool, device=dev())
    untouched[rows[live].long()] = False
    assert bool(torch.isnan(c2b[untouched]).all())
    if rider:
        i = torch.arange(n_stamp, device=dev())
        assert torch.equal(stamps[:n_stamp].long(), 0x10000 + (i // 256) % rider)
        assert not bool(stamps[n_stamp:].any())


# -------------------------------------------------------------------------------------------------- 3. whole steps
NB = 8
CASES = [(16, 64), (172, 64), (172, 1024)]  # (d, B); the library takes the form at (172, 1024) only: the write-back
#                                             rider shares fc1's launch from 48-row blocks on (3B > 2048 rows at d = 172)


def _expected(d, B):
    return (d, B) == (172, 1024)


@pytest.mark.parametrize('upd_src', ['left', 'right'])
@pytest.mark.parametrize('d,B', CASES, ids=[f'd{d}-B{B}' for d, B in CASES])
def test_whole_steps_against_oracle_and_the_five_launch_chain(d, B, upd_src, tmp_path):
    import _fc2_defer_case as case
    from oracle import tiger_oracle as O
    worst = [0.0]

    def on_step(b, stream, orc, buf):
        a = [stream[k][b * B:(b + 1) * B] for k in ('src', 'dst', 'neg', 'ts', 'eids')]
        cg = O.collate(orc.graph, a[0], a[1], a[2], a[3], case.K, 'static')
        ref = orc.stream_step(*a, cg).numpy()
        np.testing.assert_array_equal(buf.dbg_l1_nids.cpu().numpy(), cg['l1_nids'])
        worst[0] = max(worst[0], *assert_close(buf.h[:2 * B].cpu().numpy(), ref, f'h_left, batch {b}', TOL))

    got, model, orc = case.run(d, B, upd_src, NB, on_step=on_step)
    from test_hip_parity import compare_state_with_oracle
    compare_state_with_oracle(model, orc)
    for b in range(NB):
        assert bool(got[f'form{b}'] & case.FORM_FC2_DEFERRED) == _expected(d, B), (b, int(got[f'form{b}']))
    # the five-launch chain in a process of its own
    path = str(tmp_path / 'chain.npz')
    env = dict(os.environ, TG_FC2_DEFER='0')
    env.setdefault('OMP_NUM_THREADS', '4')
    r = subprocess.run([sys.executable, os.path.join(HERE, '_fc2_defer_case.py'), str(d), str(B), upd_src, str(NB), path], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'FC2-DEFER-CASE OK' in r.stdout, (r.stdout + r.stderr)[-3000:]
    ref = np.load(path)
    for b in range(NB):
        assert not (int(ref[f'form{b}']) & case.FORM_FC2_DEFERRED)
        for k in ('l1n', 'l1e', 'l1t'):
            np.testing.assert_array_equal(got[f'{k}{b}'], ref[f'{k}{b}'])
    np.testing.assert_array_equal(got['h0'], ref['h0'])  # equal state in: the same tile code, the same bits
    np.testing.assert_array_equal(got['has_msg'], ref['has_msg'])
    for k in ('left_ts', 'right_ts', 'msg_ts'):
        np.testing.assert_array_equal(got[k], ref[k])
    for k in ('left', 'right', 'mailbox', 'pending'):
        assert_close(got[k], ref[k], f'{k} against the five-launch chain', 1e-5)
    for b in range(1, NB):
        assert_close(got[f'h{b}'], ref[f'h{b}'], f'h, batch {b}, against the five-launch chain', 1e-5)


def _form_of(d, B, mutate):
    """the form bit the library reports for a (172, 1024) step buffer after `mutate(model, buf)`"""
    import _fc2_defer_case as case
    stream, model, _, buf = case.make(d, B, 'left', 2)
    model.launch_step(buf)
    torch.cuda.synchronize()
    assert case.form_bits(model, buf) & case.FORM_FC2_DEFERRED
    keep = mutate(model, buf)
    bits = case.form_bits(model, buf)
    del keep
    return bits


def test_form_bit_is_not_reported_for_the_excluded_cases():
    import _fc2_defer_case as case
    d, B = 172, 1024
    F = case.FORM_FC2_DEFERRED

    def h_new(model, buf):
        t = torch.empty(2 * B, d, dtype=torch.float32, device=dev())
        buf.io.h_new = t.data_ptr()
        return t

    def lazy(model, buf):
        trig = np.zeros(8, dtype=np.uint8)
        buf.enable_lazy_restart(model, trig)

    def not_lean(model, buf):
        buf.io.lean = 0

    assert not (_form_of(d, B, h_new) & F)
    assert not (_form_of(d, B, lazy) & F)
    assert not (_form_of(d, B, not_lean) & F)

    def two_layers(model, buf):  # (a second attention layer travels in tg_step_io.inner)
        buf._inner = model.model_struct()
        buf.io.inner = C.addressof(buf._inner)

    assert not (_form_of(d, B, two_layers) & F)
    # dropout (the training step's forward pass shares the step's code and its form decision): the same buffer asked with
    # and without it
    from www2023tiger_amd._lib import lib
    stream, model, _, buf = case.make(d, B, 'left', 2)
    model.launch_step(buf)
    torch.cuda.synchronize()
    m = model.model_struct()
    assert lib.tg_stream_step_form2(C.byref(m), C.byref(buf.io), 0) & F
    assert lib.tg_stream_step_form2(C.byref(m), C.byref(buf.io), 0) == lib.tg_stream_step_form(C.byref(m), C.byref(buf.io))
    assert not (lib.tg_stream_step_form2(C.byref(m), C.byref(buf.io), 1) & (F | 8))


# ------------------------------------------------------------------------------------- 4. graph replay against eager
def test_graph_of_three_captured_steps_is_bit_equal_to_three_eager_steps():
    import _fc2_defer_case as case
    d, B, pre = 172, 1024, 2
    outs = []
    for captured in (False, True):
        stream, model, _, buf = case.make(d, B, 'left', pre + 3)
        for _ in range(pre):
            model.launch_step(buf)
        torch.cuda.synchronize()
        assert case.form_bits(model, buf) & case.FORM_FC2_DEFERRED
        if captured:
            side = torch.cuda.Stream()
            snap = buf.offset.clone()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                for _ in range(3):
                    model.launch_step(buf)
            buf.offset.copy_(snap)
            torch.cuda.synchronize()
            graph.replay()
        else:
            for _ in range(3):
                model.launch_step(buf)
        torch.cuda.synchronize()
        assert int(buf.err.item()) == 0 and int(buf.offset.item()) == (pre + 3) * B
        outs.append([buf.h.clone(), model.left_memory.vals.clone(), model.right_memory.vals.clone(), model._pending.clone(),
                     model.msg_store.node_msg_vals.clone(), model._gtab.clone(), model._ctab.clone()])
    for a, b in zip(*outs):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------ 5. stale-parameter guard
def test_step_follows_fc2_weights_changed_in_place():
    """W2 scaled through .data (no version counter moves), then train() / eval(): the parameter epoch rebuilds the
    pre-multiplied weights, the fold and the tables before the next step.  Against a second model that is told explicitly
    (fuse_attention(), invalidate_pending()): same bits; and the fold equals the float64 product of the NEW weights."""
    import _fc2_defer_case as case
    d, B = 172, 1024
    res = []
    for explicit in (False, True):
        stream, model, _, buf = case.make(d, B, 'left', 4)
        for _ in range(2):
            model.launch_step(buf)
        torch.cuda.synchronize()
        fc2 = model.temporal_embedding_fn.fns[0].merger.fc2
        fold_before = model._fc2_fold.clone()
        with torch.no_grad():
            fc2.weight.data.mul_(1.25)
            fc2.bias.data.add_(0.01)
        if explicit:
            model.fuse_attention()
            model.invalidate_pending()
        else:
            model.train()
            model.eval()
        for _ in range(2):
            model.launch_step(buf)
        torch.cuda.synchronize()
        assert int(buf.err.item()) == 0
        assert case.form_bits(model, buf) & case.FORM_FC2_DEFERRED
        assert not torch.equal(model._fc2_fold, fold_before)
        cell = model.right_mem_updater.cell
        f8 = lambda p: p.detach().cpu().numpy().astype(np.float64)
        want = np.concatenate([(f8(cell.weight_hh) @ f8(fc2.weight)).ravel(), f8(cell.weight_hh) @ f8(fc2.bias) + f8(cell.bias_hh)])
        got = model._fc2_fold.cpu().numpy()
        assert np.abs(got - want).max() <= 2.0 ** -23 * max(1.0, np.abs(want).max())  # one rounding of a float64 sum
        res.append([buf.h.clone(), model.left_memory.vals.clone(), model._pending.clone()])
    for a, b in zip(*res):
        assert torch.equal(a, b)
