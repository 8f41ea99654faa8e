"""The sizes and references of the past-the-cap GPU tests (tests/_cap_ref.py), checked without a GPU: every size lies
where its label says relative to the cap it is derived from, the float32 emulation of the decoder's sums agrees with
float64 within the error bound of recursive summation, and the references agree with the host twins that the suite
already trusts at the new sizes."""
import ctypes as C

import numpy as np
import pytest
import torch

import _cap_ref as R
from _append_ref import assert_same, host_build
from _topk_ref import numpy_seen_mask, seen_graph


@pytest.mark.parametrize('name', list(R.SIZES))
def test_sizes_lie_at_and_past_their_caps(name):
    blocks, per_block, at, past = R.SIZES[name]
    cap = blocks * per_block
    grid = lambda items: min(-(-items // per_block), blocks)   # flat_grid / the decoder's min(cdiv(n, 64), cap)
    assert at <= cap and grid(at) == blocks, 'at: the whole grid, and no item left for a second pass'
    assert cap - at < per_block, 'at: the last block is the only one not full'
    assert past > cap and grid(past) == blocks
    assert 0 < past - cap < cap // 100, 'past: a ragged second pass, not a full one'


def test_derived_sizes():
    assert 2 * R.TCSR_E_AT == R.CAP_THREAD and 2 * R.TCSR_E_PAST == R.CAP_THREAD + 300
    assert R.TCSR_DEG_E_AT == R.CAP_THREAD and R.TCSR_DEG_E_PAST == R.CAP_THREAD + 150   # k_degree: one thread per EVENT
    assert (R.Q_WAVE_AT, R.Q_WAVE_PAST) == (R.CAP_WAVE, R.CAP_WAVE + 5)
    assert (R.Q_LANE16_AT, R.Q_LANE16_PAST) == (R.CAP_16_LANES, R.CAP_16_LANES + 5)
    assert R.TRAJ_NODES_AT * R.TRAJ_D == R.CAP_THREAD < R.TRAJ_NODES_PAST * R.TRAJ_D == 8200 * 128
    assert R.BM_NODES_AT == 64 * R.CAP_WAVE and -(-R.BM_NODES_PAST // 64) > R.CAP_WAVE and R.BM_NODES_PAST % 64
    assert R.HITS_B_AT * R.HITS_K <= R.CAP_THREAD < (R.HITS_B_AT + 1) * R.HITS_K and R.HITS_B_PAST == 26300
    assert R.ROWS_AT * (R.ROW_W // 4) <= R.CAP_THREAD < (R.ROWS_AT + 1) * (R.ROW_W // 4) and R.ROWS_PAST == 24500
    assert R.ROWS_PAST < R.ROW_TABLE
    assert R.TE_ROWS_AT * R.TE_D <= R.CAP_THREAD < (R.TE_ROWS_AT + 1) * R.TE_D and R.TE_ROWS_PAST == 6100
    assert R.DEC_FWD_N == (65536, 65536 + 17, 2 * 65536 + 64 * 3 + 1)
    assert R.DEC_BWD_N == (16384, 16384 + 1, 2 * 16384 + 65, 65536 + 17)
    assert R.DEC_D_EDGES == (4, 188, 192, 196, 384, 388, 512) and R.DEC_N_EDGES == (15, 16, 17, 64, 65)
    assert R.AUC_N == (4095, 4096, 4097, 8193)
    # the second pass of the forward at 65 536 + 17: one tile; wavefront 0 full, wavefront 1 one row, 2 and 3 empty
    left = R.DEC_FWD_N[1] - R.CAP_DEC_FWD
    assert -(-left // R.DEC_ROWS) == 1 and left - 16 == 1


def _torch_reference(x, dy, params, masks, p):
    w = [torch.from_numpy(t).double().requires_grad_(True) for t in params]
    x64 = torch.from_numpy(x).double().requires_grad_(True)
    a = torch.relu(x64 @ w[0].T + w[1])
    if masks is not None:
        a = a * torch.from_numpy(masks[0]).double() / (1 - p)
    a = torch.relu(a @ w[2].T + w[3])
    if masks is not None:
        a = a * torch.from_numpy(masks[1]).double() / (1 - p)
    y = (a @ w[4].T + w[5]).squeeze(-1)
    y.backward(torch.from_numpy(dy).double())
    out = {nm: t.grad.numpy() for nm, t in zip(R.GRAD_NAMES, w)}
    out.update(y=y.detach().numpy(), dx=x64.grad.numpy())
    return out


@pytest.mark.parametrize('p', [0.0, 0.3])
def test_float64_chain_is_torch_autograd(p):
    n, d = 300, 20
    rs = np.random.RandomState(0)
    masks = (rs.uniform(size=(n, 80)) >= p, rs.uniform(size=(n, 10)) >= p) if p else None
    x, dy, params = R.decoder_inputs(n, d, 1, masks[0] if p else None, p)
    ref, want = R.decoder_reference(x, dy, params, masks, p), _torch_reference(x, dy, params, masks, p)
    for k in want:
        assert ref[k].shape == want[k].shape, k
        np.testing.assert_allclose(ref[k], want[k], rtol=1e-12, atol=1e-12, err_msg=k)


def test_decoder_inputs_keep_the_pre_activations_off_zero():
    x, dy, params = R.decoder_inputs(5000, 172, 2)
    c = R.decoder_chain(x, dy, params)
    assert np.abs(c['z1']).min() >= 1e-4 and np.abs(c['z2']).min() >= 1e-4
    c32 = R.decoder_chain(x, dy, params, dtype=np.float32)
    assert np.array_equal(c32['z1'] > 0, c['z1'] > 0) and np.array_equal(c32['z2'] > 0, c['z2'] > 0)


def test_float32_emulation_is_within_the_bound_of_recursive_summation():
    """n = 5 000 rows (79 tiles: one per workgroup, the partials added in workgroup order).  A float32 sum of m terms
    added one at a time is off by at most (m - 1) u sum |term| / (1 - (m - 1) u), u = 2^-24, and each term by u |term|
    for its product: (m + 1) u sum |term| in all, and a little for the float32 rounding of the factors themselves (each
    factor is off by a few u relative: 16 u allowed).  The emulation must meet that bound element by element - and must
    not be exact either: it has to round as float32 does."""
    n, d = 5000, 172
    x, dy, params = R.decoder_inputs(n, d, 3)
    emu, ref = R.decoder_emulation(x, dy, params), R.decoder_reference(x, dy, params)
    c = R.decoder_chain(x, dy, params)
    mass = dict(w1=np.abs(c['dz1']).T @ np.abs(c['x']), b1=np.abs(c['dz1']).sum(0), w2=np.abs(c['dz2']).T @ np.abs(c['a1']),
                b2=np.abs(c['dz2']).sum(0), w3=(np.abs(c['dy']) @ np.abs(c['a2']))[None, :], b3=np.abs(c['dy']).sum(keepdims=True))
    u = 2.0 ** -24
    for k in R.GRAD_NAMES:
        assert emu[k].dtype == np.float32 and emu[k].shape == ref[k].shape, k
        err = np.abs(emu[k].astype(np.float64) - ref[k])
        assert (err <= (n + 1 + 16) * u * mass[k]).all(), k
        assert err.max() > 0, k
    # order matters to the emulation: the same rows in another order round differently
    perm = np.random.RandomState(0).permutation(n)
    other = R.decoder_emulation(x[perm], dy[perm], params)
    assert not np.array_equal(other['w1'], emu['w1']) and not np.array_equal(other['w2'], emu['w2'])


def test_emulation_takes_the_workgroups_tiles_in_the_documented_order():
    """n = 2 * 16 384 + 65 rows, a single hidden unit live: the sums are plain float32 sums of known numbers, recomputed
    here with an explicit loop over workgroups and their tiles"""
    n = R.DEC_BWD_N[2]
    rs = np.random.RandomState(1)
    v = rs.standard_normal(n).astype(np.float32)
    c = dict(x=np.ones((n, 4), np.float32), dy=v, a2=np.ones((n, R.DEC_H2), np.float32), a1=np.ones((n, R.DEC_H1), np.float32),
             dz2=np.repeat(v[:, None], R.DEC_H2, 1), dz1=np.repeat(v[:, None], R.DEC_H1, 1))
    got = R.decoder_sums_f32(c)
    ntile = -(-n // R.DEC_ROWS)
    parts = []
    for b in range(R.DEC_BWD_PARTS):
        s = np.float32(0)
        for tile in range(b, ntile, R.DEC_BWD_PARTS):
            for r in range(tile * R.DEC_ROWS, min(n, (tile + 1) * R.DEC_ROWS)):
                s = np.float32(s + v[r])
        parts.append(s)
    want = np.float32(0)
    for s in parts:
        want = np.float32(want + s)
    for k in ('b2', 'w3', 'b3', 'b1', 'w2'):
        assert (got[k].view(np.uint32) == want.view(np.uint32)).all(), k
    plain = np.float32(0)
    for t in v:
        plain = np.float32(plain + t)
    assert (got['w1'].view(np.uint32) == plain.view(np.uint32)).all()
    assert plain.view(np.uint32) != want.view(np.uint32)   # the two orders are told apart by this input


# ---- the references against the host twins, at the new sizes -----------------------------------------------------------
def test_tcsr_host_build_equals_the_oracle_past_the_cap():
    from oracle.tiger_oracle import OracleGraph
    s = R.tcsr_stream(R.TCSR_E_PAST)
    assert 2 * len(s[0]) == 2 ** 20 + 300
    assert (s[0] == s[1]).any() and (np.diff(s[2]) == 0).any() and np.bincount(s[0]).argmax() == 7
    g = OracleGraph(*s, max_node_id=R.TCSR_N - 1)
    assert_same(host_build(R.TCSR_N, *s), R.oracle_arrays(g), 'P = 2^20 + 300')


def test_seen_mask_host_equals_the_numpy_loop_on_the_checked_rows():
    from www2023tiger_amd._lib import TgTcsr, lib, ptr
    ev_src, ev_dst, ev_ts, n_nodes = seen_graph()
    src, ts, cat, rows = R.seen_case(R.Q_WAVE_PAST)
    assert len(src) == R.Q_WAVE_PAST and len(rows) == 200 and set(range(len(src) - 5, len(src))) <= set(rows.tolist())
    h = host_build(n_nodes, ev_src, ev_dst, ev_ts, np.arange(1, len(ev_src) + 1, dtype=np.int64))
    col_of = np.full(n_nodes, -1, dtype=np.int32)
    col_of[cat] = np.arange(len(cat), dtype=np.int32)
    m8 = np.ones((len(src), len(cat)), dtype=np.uint8)
    tc = TgTcsr(n_nodes, len(h[1]), *(ptr(a) for a in h))
    assert lib.tg_seen_mask_host(C.byref(tc), len(src), ptr(src), ptr(ts), len(cat), ptr(col_of), ptr(m8)) == 0
    want = numpy_seen_mask(ev_src, ev_dst, ev_ts, src[rows], ts[rows], cat)
    np.testing.assert_array_equal(m8[rows].astype(bool), want)
    assert not want.all() and want.any()
