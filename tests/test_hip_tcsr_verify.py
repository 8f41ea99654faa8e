"""tg_tcsr_verify on the GPU against the numpy reference: the cases of the host test, and the shapes at which the kernel
can go wrong - tile edges, a pair that straddles two tiles, a hub row over three tiles, a tile that spans more rows than
the LDS window holds, the node pass's block edges, an empty graph, a non-monotone indptr.  Every call goes out with guard
words behind out8 and behind the workspace.  No corrupted graph is handed to a sampler or to any other kernel: the
refusal is what is tested."""
import ctypes as C
import io

import numpy as np
import pytest
import torch

from _verify_ref import (CLEAN, EID_RANGE, ENDS, NBR_RANGE, PTR_ORDER, TS_NAN, TS_ORDER, changed, clean, one_word_cases,
                         random_rows, same_result, synthetic, verify_numpy)
from www2023tiger_amd import hip_ops
from www2023tiger_amd._lib import TG_EWORKSPACE, TgTcsr, lib, ptr
from www2023tiger_amd.data.graph import Graph

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TILE, WIN, BLOCK = 2048, 2048, 256   # entries per tile, rows of the LDS window, row bounds per workgroup of the node pass
GUARD = -0x0123456789ABCDEF


def dev_verify(h, eid_rows=-1, short_by=0):
    """tg_tcsr_verify over host arrays h, uploaded -> (rc, (code, first, t_max)); asserts the guard words"""
    d = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in h)
    N, P = len(h[0]) - 1, len(h[1])
    g = TgTcsr(N, P, *(ptr(a) for a in d))
    nbytes = int(lib.tg_tcsr_verify_workspace_bytes(P, N))
    assert nbytes > 0 and nbytes % 16 == 0
    out = torch.full((16,), GUARD, dtype=torch.int64, device=DEV)
    ws = torch.full((nbytes // 8 + 8,), GUARD, dtype=torch.int64, device=DEV)
    rc = lib.tg_tcsr_verify(C.byref(g), int(eid_rows), ptr(out), ptr(ws), nbytes - short_by, hip_ops.stream_ptr(DEV))
    torch.cuda.synchronize()
    o, w = out.cpu().numpy(), ws.cpu().numpy()
    assert (o[8:] == GUARD).all(), 'written behind out8'
    assert (w[nbytes // 8:] == GUARD).all(), 'written behind the workspace'
    if rc != 0:
        assert (o == GUARD).all() and (w == GUARD).all(), 'something was launched'
        return rc, None
    for a, b in zip(d, h):
        np.testing.assert_array_equal(a.cpu().numpy().view(np.int64 if b.itemsize == 8 else np.int32),
                                      b.view(np.int64 if b.itemsize == 8 else np.int32), err_msg='the input is only read')
    return rc, (int(o[0]), [int(x) for x in o[1:7]], float(o[7:8].view(np.float64)[0]))


def check(h, eid_rows, what):
    rc, got = dev_verify(h, eid_rows)
    assert rc == 0, what
    want = verify_numpy(h, eid_rows)
    same_result(got, want, what)
    return got


@pytest.mark.parametrize('name', list(CLEAN))
def test_clean_graphs_and_one_changed_word(name):
    N, ev, rows, h = clean(name)
    got = check(h, rows, name)
    assert got[0] == 0
    for label, arrays, r, cls in one_word_cases(h, rows):
        got = check(arrays, r, f'{name} {label}')
        assert (got[0] & cls) if cls else got[0] == 0, f'{name} {label}: {got}'


@pytest.mark.parametrize('P', [TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1])
def test_tile_edges(P):
    h = synthetic(random_rows(37, P, seed=P), rows=500, seed=P)
    assert check(h, 500, f'P={P}')[0] == 0
    for p in sorted({0, P - 1, min(TILE - 1, P - 1), min(TILE, P - 1)}):
        got = check(changed(h, 2, p, -1), 500, f'P={P} nbr at {p}')
        assert got[0] == NBR_RANGE and got[1][4] == p
        got = check(changed(h, 1, p, np.nan), 500, f'P={P} nan at {p}')
        assert got[0] & TS_NAN and got[1][3] == p
        got = check(changed(h, 3, p, 500), 500, f'P={P} eid at {p}')
        assert got[0] == EID_RANGE and got[1][5] == p
    # two of one class in different tiles: the smaller index wins
    if P > TILE:
        a = changed(changed(h, 2, P - 1, 37), 2, 5, 37)
        assert check(a, 500, f'P={P} two')[1][4] == 5


@pytest.mark.parametrize('row_start_at_seam', [False, True])
def test_a_pair_that_straddles_two_tiles(row_start_at_seam):
    P = 2 * TILE + 1
    h = synthetic([0, 1000, TILE if row_start_at_seam else 3000, P], seed=3)
    h[1][1000:] = np.arange(1000, P) * 0.25   # ascending over the seam, whichever row it falls in
    assert check(h, 1000, 'clean')[0] == 0
    a = changed(h, 1, TILE, float(h[1][TILE - 1]) - 1.0)   # the entry in front belongs to the tile before
    got = check(a, 1000, f'seam, row start {row_start_at_seam}')
    if row_start_at_seam:
        assert got[0] == 0
    else:
        assert got[0] == TS_ORDER and got[1][2] == TILE
    a = changed(h, 1, TILE - 1, float(h[1][TILE - 2]) - 1.0)   # the last entry of the first tile, inside a row either way
    got = check(a, 1000, 'last entry of a tile')
    assert got[0] == TS_ORDER and got[1][2] == TILE - 1


def test_a_hub_row_over_three_tiles():
    P = 3 * TILE + 6
    h = synthetic([0, 5, 5, 5 + 3 * TILE, P], seed=4)
    assert check(h, 1000, 'hub')[0] == 0
    for p in (6, TILE + 17, 2 * TILE, 3 * TILE + 4):
        got = check(changed(h, 1, p, float(h[1][p - 1]) - 1.0), 1000, f'hub, decrease at {p}')
        assert got[0] == TS_ORDER and got[1][2] == p
    a = changed(changed(h, 1, 2 * TILE + 9, -1.0), 1, TILE + 3, -1.0)
    assert check(a, 1000, 'hub, two decreases')[1][2] == TILE + 3


def test_a_tile_that_spans_more_rows_than_the_window():
    N = 2 * WIN + 300   # rows 1 and N - 2 hold 50 entries each, every other row is empty: one tile over N - 2 rows
    indptr = np.zeros(N + 1, dtype=np.int64)
    indptr[2:N - 1] = 50
    indptr[N - 1:] = 100
    h = synthetic(indptr, seed=5)
    h[1][:50], h[1][50:] = np.arange(50) + 100.0, np.arange(50)   # down across the rows in between: legal
    assert check(h, 1000, 'wide tile')[0] == 0
    lo, hi = changed(h, 1, 10, float(h[1][9]) - 1.0), changed(h, 1, 70, float(h[1][69]) - 1.0)
    got = check(lo, 1000, 'decrease in front of the empty rows')
    assert got[0] == TS_ORDER and got[1][2] == 10
    got = check(hi, 1000, 'decrease behind the empty rows')
    assert got[0] == TS_ORDER and got[1][2] == 70
    both = changed(lo, 1, 70, float(h[1][69]) - 1.0)
    assert check(both, 1000, 'both')[1][2] == 10
    # the same rows inside the window's capacity: the staged path on the same entries
    M = 300
    ind2 = np.concatenate([indptr[:2], np.full(M - 3, 50), indptr[N - 1:]]).astype(np.int64)
    h2 = (ind2, h[1], (h[2] % M).astype(np.int32), h[3])
    assert check(h2, 1000, 'narrow tile')[0] == 0
    assert check(changed(h2, 1, 70, float(h[1][69]) - 1.0), 1000, 'narrow, decrease')[1][2] == 70


@pytest.mark.parametrize('n_bounds', [BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 1])
def test_node_pass_block_edges(n_bounds):
    N = n_bounds - 1
    h = synthetic(random_rows(N, 700, seed=N), seed=N)
    assert check(h, 1000, f'N={N}')[0] == 0
    got = check(changed(h, 0, N, 701), 1000, f'N={N} end')
    assert got[0] == ENDS and got[1][0] == N
    got = check(changed(h, 0, N, int(h[0][N - 1]) - 1), 1000, f'N={N} last pair')
    assert got[0] == ENDS | PTR_ORDER and got[1][:2] == [N, N - 1]
    for v in sorted({0, BLOCK - 2, BLOCK - 1, min(BLOCK, N - 2)}):
        if v + 1 < N:
            got = check(changed(h, 0, v + 1, int(h[0][v]) - 1), 1000, f'N={N} pair at {v}')
            assert got[0] & PTR_ORDER and got[1][1] == v and got[1][2] == -1


def test_an_empty_graph():
    for N in (1, 5, BLOCK):
        h = synthetic(np.zeros(N + 1, dtype=np.int64))
        got = check(h, 10, f'empty N={N}')
        assert got == (0, [-1] * 6, -np.inf)
    got = check(changed(synthetic(np.zeros(6, dtype=np.int64)), 0, 5, 1), 10, 'empty, end')
    assert got[0] == ENDS and got[1][0] == 5


def test_a_non_monotone_indptr_with_entry_violations():
    rs = np.random.RandomState(9)
    N, P = 3000, 3 * TILE + 11
    h = synthetic(random_rows(N, P, seed=9), seed=9)
    for trial in range(3):
        a = [x.copy() for x in h]
        if trial == 0:
            a[0][:] = rs.permutation(a[0])
        elif trial == 1:
            a[0][:] = rs.randint(-2 ** 62, 2 ** 62, N + 1)
        else:
            a[0][1:N] = a[0][1:N][::-1]   # the ends hold, everything in between descends
        a[1][[100, 5000]] = np.nan
        a[1][4000] = -7.0
        a[2][[TILE, 17]] = [N + 5, -2 ** 31]
        a[3][P - 1] = 0x7FFFFFFF
        got = check(a, 1000, f'garbage indptr {trial}')
        assert got[0] & PTR_ORDER and not got[0] & TS_ORDER and got[1][2] == -1
        assert got[1][3:] == [100, 17, P - 1] and got[0] & (TS_NAN | NBR_RANGE | EID_RANGE) == TS_NAN | NBR_RANGE | EID_RANGE


def test_a_short_workspace_launches_nothing():
    h = synthetic(random_rows(40, TILE + 5, seed=1), seed=1)
    for short in (1, 16, 64):
        rc, got = dev_verify(h, 1000, short_by=short)
        assert rc == TG_EWORKSPACE and got is None
    assert dev_verify(h, 1000)[0] == 0


def test_wrapper_results_and_refusals():
    N, ev, rows, h = clean('N65-E200')
    a = changed(changed(h, 2, 9, N), 1, 30, np.nan)
    d = tuple(torch.from_numpy(x).to(DEV) for x in a)
    same_result(hip_ops.tcsr_verify(d, rows), verify_numpy(a, rows), 'wrapper')
    same_result(hip_ops.tcsr_verify(d), verify_numpy(a, -1), 'wrapper, no table')
    with pytest.raises(ValueError, match='nbr'):
        hip_ops.tcsr_verify((d[0], d[1], d[2].long(), d[3]))
    with pytest.raises(ValueError, match='one entry each'):
        hip_ops.tcsr_verify((d[0], d[1], d[2][:-1].contiguous(), d[3]))
    with pytest.raises(ValueError, match='device'):
        hip_ops.tcsr_verify(tuple(torch.from_numpy(x) for x in a))


def device_children(N, ev, rows):
    g = Graph.from_arrays(*ev, strategy='recent_edges', seed=3, max_node_id=N - 1, device=DEV)
    g.tcsr
    t = g._t_last
    new = tuple(torch.tensor(x, device=DEV) for x in ([0, N - 1], [N - 1, N + 2], [t, t + 1.0], [rows, rows + 1]))
    ext = g.extended(*new, num_node='auto')
    remap, n_live, ws = hip_ops.edge_rows_plan(ext, rows + 2)
    _, eid_out = hip_ops.edge_rows_apply(ext, None, remap, n_live, ws)
    return g, [('extended', ext, rows + 2), ('trimmed', ext.trimmed(keep_last=2), rows + 2),
               ('without', ext.without(nodes=[N // 2], eids=[1, 2]), rows + 2),
               ('renumbered', ext.renumbered(remap, eid_out), n_live)]


def test_device_resident_children_verify_clean():
    N, ev, rows, h = clean('N9228-E5000')
    g, kids = device_children(N, ev, rows)
    for label, child, r in [('root', g, rows)] + kids:
        assert child._dev is not None
        got = hip_ops.tcsr_verify(child, r)
        hc = tuple(t.cpu().numpy() for t in child._dev)
        same_result(got, verify_numpy(hc, r), label)
        assert got[0] == 0, f'{label}: {hip_ops.TCSR_VERIFY_TEXT(got[0], got[1])}'


# ---- Graph.state_dict / from_state_dict on the device ----------------------------------------------------------------
def through_a_file(sd):
    f = io.BytesIO()
    torch.save(sd, f)
    f.seek(0)
    return torch.load(f, weights_only=True)


@pytest.mark.parametrize('strategy', ['recent_edges', 'recent_nodes', 'uniform'])
def test_loaded_graph_samples_and_extends_as_the_original(strategy):
    N, ev, rows, h = clean('N65-E200')
    g, kids = device_children(N, ev, rows)
    rs = np.random.RandomState(1)
    q_n = torch.from_numpy(rs.randint(0, N, 64)).to(DEV)
    q_t = torch.from_numpy(rs.uniform(0, float(ev[2].max()) + 2.0, 64)).to(DEV)
    for label, src, r in kids:
        if strategy == 'uniform':
            src.sample_device(q_n, q_t, 5, 'uniform')   # somewhere inside the device stream of draws
        sd = through_a_file(src.state_dict())
        assert all(not v.is_cuda for v in sd.values() if torch.is_tensor(v))
        back = Graph.from_state_dict(sd, device=DEV, eid_rows=r)
        assert back._dev is not None and back.serial != src.serial and back.num_node == src.num_node
        assert back._t_last == float(src._t_last) and back.strategy == src.strategy
        for a, b in zip(back._dev, src._dev):
            assert a.dtype == b.dtype and a.data_ptr() != b.data_ptr() and torch.equal(a, b), label
        for x, y in zip(back._host_tcsr(), tuple(t.cpu().numpy() for t in src._dev)):
            np.testing.assert_array_equal(x, y)
        for rep in range(2):   # 'uniform': the draws continue one stream on both sides
            for a, b in zip(back.sample_device(q_n, q_t, 7, strategy), src.sample_device(q_n, q_t, 7, strategy)):
                assert torch.equal(a, b), f'{label} {strategy} {rep}'
        t = float(src._t_last)
        new = ([1, 2], [2, N + 1], [t, t + 3.0], [5, 6])
        for a, b in zip(back.extended(*new)._tensors(), src.extended(*new)._tensors()):
            assert torch.equal(a, b), f'{label}: extended'


def test_loading_on_the_device_refuses_before_anything_else_runs():
    N, ev, rows, h = clean('N65-E200')
    g = Graph.from_arrays(*ev, max_node_id=N - 1, device=DEV)
    sd = g.state_dict()
    for key, index, value, pattern in (('nbr', 40, N, r'NBR_RANGE.*entry 40'), ('ts', 7, float('nan'), r'TS_NAN.*entry 7'),
                                       ('indptr', N, 2 * len(ev[0]) - 1, r'ENDS.*row bound 65'),
                                       ('indptr', 8, -4, r'PTR_ORDER.*row 7'), ('eid', 3, rows, r'EID_RANGE.*entry 3')):
        bad = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in sd.items()}
        bad[key][index] = value
        with pytest.raises(ValueError, match=pattern):
            Graph.from_state_dict(bad, device=DEV, eid_rows=rows)
    bad = dict(sd, t_last=float(ev[2].max()) - 0.5)
    with pytest.raises(ValueError, match='below the largest time'):
        Graph.from_state_dict(bad, device=DEV)
    assert Graph.from_state_dict(dict(sd, t_last=float(ev[2].max()) + 9.0), device=DEV)._t_last == float(ev[2].max()) + 9.0
