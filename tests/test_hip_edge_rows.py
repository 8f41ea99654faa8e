"""Releasing edge-feature rows on the GPU: tg_edge_rows_plan + tg_edge_rows_apply against the host twin (which
tests/test_edge_rows_host.py holds against numpy), remap, packed table and renumbered eids bit for bit; row counts at the
seams of the scan's 2048-row chunk (and, at 255 / 256 / 257 rows, of a thread's 8-row group inside one chunk), past 256
chunks, where a workgroup strides over the chunk totals; live counts at the seams of the copy tile; entry counts at the seams of the
2048-entry workgroups of mark and eid remap; nothing written outside the outputs or into the inputs; the samplers, the
seen mask and the row gather on the renumbered graph against the parent's results pushed through the remap.

The copy tile is a whole number of OUTPUT rows: min(2048, max(1, 4096 // (d_e / 4))) - 2048 rows at d_e = 4 and 8, 95 at
d_e = 172 (43 float4 a row), 64 at 256, 32 at 512 (tg_edge_rows.hip: ER_TILE_F4, ER_TILE_ROWS).  No grid is capped: every
workgroup owns one chunk / tile, so there is no size past a cap to test."""
import ctypes as C

import numpy as np
import pytest
import torch

from _edge_rows_ref import flagged, host_release, patterns, release_numpy, row_stream, table_of

pytestmark = pytest.mark.gpu

ER_CHUNK, ER_ENTRIES = 2048, 2048   # tg_edge_rows.hip: rows per scan workgroup, entries per mark / remap workgroup
GUARD = 0x5A


def dev():
    return torch.device('cuda', 0)


def tile_rows(d_e):
    return min(2048, max(1, 4096 // (d_e // 4)))


def raw_release(eid, table, n_rows, keep_from=None, pin=None, *, ws_bytes=None, n_live=None):
    """plan + read-back + apply on device copies, 64 guard bytes behind remap, table_out and eid_out
    -> dict(rc_plan, rc_apply, n_live, remap, table_out, eid_out as numpy, guards_ok, inputs_ok, ws)"""
    from www2023tiger_amd._lib import TgTcsr, lib, ptr
    from www2023tiger_amd.hip_ops import stream_ptr
    d = dev()
    eid = np.ascontiguousarray(eid, dtype=np.int32)
    P = len(eid)
    eid_d = torch.from_numpy(eid).to(d)
    tab_d = None if table is None else torch.from_numpy(table).to(d)
    pin_d = None if pin is None or len(pin) == 0 else torch.as_tensor(pin, dtype=torch.int64).to(d)
    g = TgTcsr(1, P, None, None, None, ptr(eid_d) if P else None)
    need = int(lib.tg_edge_rows_workspace_bytes(n_rows, P))
    nbytes = need if ws_bytes is None else ws_bytes
    ws = torch.full((need + 64,), GUARD, dtype=torch.uint8, device=d)
    remap = torch.full((4 * n_rows + 64,), GUARD, dtype=torch.uint8, device=d)
    nl = torch.full((1,), -7, dtype=torch.int64, device=d)
    out = dict(ws=ws, need=need)
    out['rc_plan'] = lib.tg_edge_rows_plan(C.byref(g), n_rows, n_rows if keep_from is None else keep_from, ptr(pin_d),
                                           0 if pin_d is None else pin_d.numel(), ptr(remap), ptr(nl), ptr(ws), nbytes,
                                           stream_ptr(d))
    torch.cuda.synchronize()
    out['n_live'] = int(nl)
    out['remap_raw'] = remap
    out['remap'] = remap[:4 * n_rows].view(torch.int32).cpu().numpy()
    out['guards_ok'] = bool((remap[4 * n_rows:] == GUARD).all()) and bool((ws[need:] == GUARD).all())
    if out['rc_plan'] != 0 or out['n_live'] < 0:
        return out
    n = out['n_live'] if n_live is None else n_live
    d_e = 0 if table is None else table.shape[1]
    t_out = torch.full((4 * n * d_e + 64,), GUARD, dtype=torch.uint8, device=d)
    e_out = torch.full((4 * P + 64,), GUARD, dtype=torch.uint8, device=d)
    out['rc_apply'] = lib.tg_edge_rows_apply(C.byref(g), ptr(tab_d), n_rows, d_e, ptr(remap), n, ptr(t_out), ptr(e_out),
                                             ptr(ws), nbytes, stream_ptr(d))
    torch.cuda.synchronize()
    out['table_out'] = t_out[:4 * n * d_e].view(torch.int32).reshape(n, d_e).cpu().numpy() if d_e else None
    out['eid_out'] = e_out[:4 * P].view(torch.int32).cpu().numpy()
    out['guards_ok'] = (out['guards_ok'] and bool((t_out[4 * n * d_e:] == GUARD).all()) and bool((e_out[4 * P:] == GUARD).all())
                        and bool((ws[need:] == GUARD).all()))
    out['inputs_ok'] = (np.array_equal(eid_d.cpu().numpy(), eid)
                        and (table is None or np.array_equal(tab_d.cpu().numpy().view(np.int32), table.view(np.int32))))
    return out


def check(eid, n_rows, d_e, keep_from=None, pin=None, what=''):
    table = table_of(n_rows, d_e, seed=n_rows % 1000 + d_e, special=True)   # NaN payloads, denormals, -0.0
    r = raw_release(eid, table, n_rows, keep_from, pin)
    assert r['rc_plan'] == 0 and r['rc_apply'] == 0, what
    rc, remap, t_out, eid_out, n_live = host_release(eid, table, n_rows, keep_from, pin)
    assert rc == 0
    assert r['n_live'] == n_live, what
    np.testing.assert_array_equal(r['remap'], remap, err_msg=what)
    np.testing.assert_array_equal(r['eid_out'], eid_out, err_msg=what)
    np.testing.assert_array_equal(r['table_out'], t_out.view(np.int32), err_msg=what)
    assert r['guards_ok'], f'{what}: bytes behind an output were written'
    assert r['inputs_ok'], f'{what}: eids or the old table changed'
    # bit 31 is carried over
    np.testing.assert_array_equal(r['eid_out'].view(np.uint32) >> 31, np.asarray(eid, dtype=np.int32).view(np.uint32) >> 31)
    return r


ROWS = [255, 256, 257, ER_CHUNK - 1, ER_CHUNK, ER_CHUNK + 1, 2 * ER_CHUNK + 1]


@pytest.mark.parametrize('d_e', [4, 8])
@pytest.mark.parametrize('n_rows', ROWS)
def test_row_counts_at_the_seams_of_the_scan_chunk_and_the_copy_tile(n_rows, d_e):
    """2047 / 2048 / 2049 / 4097 rows are seams of the scan chunk and, all live at d_e = 4 and 8, of the 2048-row copy tile"""
    p = patterns(n_rows)
    check(p['all-live'], n_rows, d_e, what='all-live')
    check(p['random-third'], n_rows, d_e, keep_from=n_rows - 3, pin=[1, n_rows - 5, 1], what='random-third')
    check(p['alternating'], n_rows, d_e, what='alternating')


@pytest.mark.parametrize('d_e', [172, 256, 512])
def test_live_counts_at_the_seams_of_the_copy_tile_of_wide_rows(d_e):
    t = tile_rows(d_e)
    assert t == {172: 95, 256: 64, 512: 32}[d_e]
    for n in (t - 1, t, t + 1, 2 * t + 1):
        check(patterns(n)['all-live'], n, d_e, what=f'{n} live rows')
    n = 3 * t + 5
    check(patterns(3 * n)['random-third'], 3 * n, d_e, keep_from=3 * n - t - 1, what='a third and a tail')


def test_past_256_scan_workgroups_the_totals_in_front_are_summed_in_strides():
    n_rows = 256 * ER_CHUNK + ER_CHUNK + 3   # 258 chunks: workgroups 257 and 258 stride twice over the totals
    rs = np.random.RandomState(1)
    eid = flagged(rs.randint(0, n_rows, n_rows // 3), 1)
    r = check(eid, n_rows, 4, keep_from=n_rows - 7, what='258 chunks')
    assert 0 < r['n_live'] < n_rows // 2


@pytest.mark.parametrize('P', [0, 1, ER_ENTRIES - 1, ER_ENTRIES + 1])
def test_entry_counts_at_the_seams_of_the_entry_workgroups(P):
    n_rows = 700
    eid = flagged(np.random.RandomState(P).randint(0, n_rows, P), P)
    r = check(eid, n_rows, 8, what=f'{P} entries')
    assert r['n_live'] == len(np.unique(np.concatenate([[0], eid.view(np.uint32) & np.uint32(0x7FFFFFFF)])))
    if P == 1:   # more pins than entries: the pins alone size the grid of the mark kernel
        check(eid, n_rows, 8, pin=list(range(100, 100 + 500)) * 5, what='2500 pins, one entry')
    if P == 0:
        check(eid, n_rows, 8, keep_from=0, what='everything pending')
        check(eid, n_rows, 8, pin=[699], what='a pin and no entry')


@pytest.mark.parametrize('name', list(patterns(300)))
def test_live_patterns(name):
    for d_e in (4, 172):
        r = check(patterns(300)[name], 300, d_e, what=name)
    if name == 'none-but-0':
        assert r['n_live'] == 1
    if name == 'last-only':
        assert r['n_live'] == 2 and r['remap'][-1] == 1
    if name == 'all-live':
        assert r['n_live'] == 300 and r['remap'].tolist() == list(range(300))


def test_a_graph_only_release_renumbers_without_a_table():
    eid = patterns(500)['random-third']
    r = raw_release(eid, None, 500, 450, [7])
    rc, remap, _, eid_out, n_live = host_release(eid, None, 500, 450, [7])
    assert r['rc_plan'] == 0 and r['rc_apply'] == 0 and r['n_live'] == n_live and r['guards_ok']
    np.testing.assert_array_equal(r['remap'], remap)
    np.testing.assert_array_equal(r['eid_out'], eid_out)


def test_a_short_workspace_writes_nothing_and_bad_arguments_are_refused():
    from www2023tiger_amd import _lib
    n_rows = 3000
    eid = patterns(n_rows)['random-third']
    table = table_of(n_rows, 8)
    need = int(_lib.lib.tg_edge_rows_workspace_bytes(n_rows, len(eid)))
    for short in (0, 16, need - 1):
        r = raw_release(eid, table, n_rows, ws_bytes=short)
        assert r['rc_plan'] == _lib.TG_EWORKSPACE and r['n_live'] == -7
        assert bool((r['remap_raw'] == GUARD).all()) and bool((r['ws'] == GUARD).all()), 'something was launched'
    for kf in (-1, n_rows + 1):
        r = raw_release(eid, table, n_rows, kf)
        assert r['rc_plan'] == _lib.TG_EINVAL and bool((r['remap_raw'] == GUARD).all()) and bool((r['ws'] == GUARD).all())
    ok = raw_release(eid, table, n_rows)
    for bad in (0, n_rows + 1):
        r = raw_release(eid, table, n_rows, n_live=bad)
        assert r['rc_apply'] == _lib.TG_EINVAL
        assert (r['eid_out'].view(np.uint8) == GUARD).all() and r['guards_ok']
    assert ok['rc_apply'] == 0


@pytest.mark.parametrize('where', ['entry', 'entry-with-flag', 'pin'])
def test_an_id_that_names_no_row_gives_minus_one_and_an_unwritten_remap(where):
    n_rows = 5000   # three scan chunks: every one of them sees the flag
    eid = patterns(n_rows)['random-third'].copy()
    pin = None
    if where == 'entry':
        eid[1234] = n_rows
    elif where == 'entry-with-flag':
        eid[-1] = np.int32(n_rows + 17) | np.int32(-0x80000000)
    else:
        pin = [3, n_rows, 5]
    r = raw_release(eid, table_of(n_rows, 4), n_rows, None, pin)
    assert r['rc_plan'] == 0 and r['n_live'] == -1
    assert bool((r['remap_raw'] == GUARD).all()), 'remap was written'
    assert r['guards_ok']
    assert host_release(eid, None, n_rows, None, pin)[0] != 0   # the twin refuses the same input


# ------------------------------------------------------------------------------------------------- graphs and consumers
def resident(N, ev, **kw):
    from www2023tiger_amd.data.graph import Graph
    g = Graph.from_arrays(*ev, max_node_id=N - 1, device=dev(), **kw)
    g._tensors()
    return g


def release(g, table, keep_from=None, pin=None):
    """hip_ops plan + apply + Graph.renumbered on a device-resident graph -> (child, remap, table_out)"""
    from www2023tiger_amd import hip_ops
    remap, n_live, ws = hip_ops.edge_rows_plan(g, table.shape[0], keep_from, pin)
    t_out, eid_out = hip_ops.edge_rows_apply(g, table, remap, n_live, ws)
    assert t_out.shape[0] == n_live and t_out.untyped_storage().nbytes() == 4 * n_live * table.shape[1]   # allocated exactly
    return g.renumbered(remap, eid_out), remap, t_out


def test_a_hub_whose_eids_are_scattered_and_the_parent_stays_what_it_was():
    N, E = 300, 6000
    ev = row_stream(N, E, seed=8, hub=7)
    parent = resident(N, ev, strategy='recent_edges', seed=2).trimmed(keep_last=128)
    before = [t.clone() for t in parent._tensors()]
    table = torch.from_numpy(table_of(E + 1, 8, special=True)).to(dev())
    t0 = table.clone()
    child, remap, t_out = release(parent, table, keep_from=E - 20)
    h = [t.cpu().numpy() for t in before]
    w_remap, w_table, w_eid = release_numpy(h[3], t0.cpu().numpy(), E + 1, E - 20)
    live = np.flatnonzero(w_remap >= 0)
    assert 200 < len(live) < E // 2 and np.diff(live).max() > 8   # scattered: runs of dead rows in between
    np.testing.assert_array_equal(remap.cpu().numpy(), w_remap)
    np.testing.assert_array_equal(t_out.cpu().numpy().view(np.int32), w_table.view(np.int32))
    c = child._tensors()
    np.testing.assert_array_equal(c[3].cpu().numpy(), w_eid)
    for i in range(3):
        assert c[i] is parent._tensors()[i]   # indptr, ts, nbr: the same tensors
    for a, b in zip(parent._tensors(), before):
        assert torch.equal(a, b)   # the parent graph, bit for bit
    assert torch.equal(table.view(torch.int32), t0.view(torch.int32))   # the old table, bit for bit
    assert child.serial != parent.serial and child.tcsr.serial == child.serial and child._mt is parent._mt
    assert child._events is None and child._t_last == parent._t_last
    for a, b in zip(child._host_tcsr(), (h[0], h[1], h[2], w_eid)):
        np.testing.assert_array_equal(a, b)   # the host view is downloaded from the child's own arrays
    # extended works on it; the caller's pending eids go through - shift
    shift = E + 1 - t_out.shape[0]
    more = (ev[0][:5], ev[1][:5], ev[2][-1] + np.arange(5.0), np.arange(E - 19, E - 14) - shift)
    assert child.extended(*more).tcsr.num_entry == child.tcsr.num_entry + 10


def test_plan_raises_for_an_entry_that_names_no_row_and_for_a_bad_keep_from():
    from www2023tiger_amd import hip_ops
    N, E = 50, 400
    g = resident(N, row_stream(N, E, seed=3))
    with pytest.raises(ValueError, match='names no row'):
        hip_ops.edge_rows_plan(g, E)   # eid E is row E: one row short
    with pytest.raises(ValueError, match='names no row'):
        hip_ops.edge_rows_plan(g, E + 1, pin=[E + 1])
    with pytest.raises(ValueError, match='keep_from'):
        hip_ops.edge_rows_plan(g, E + 1, keep_from=E + 2)
    remap, n_live, ws = hip_ops.edge_rows_plan(g, E + 1)
    assert n_live == E + 1
    with pytest.raises(ValueError, match='table'):
        hip_ops.edge_rows_apply(g, torch.zeros(E + 1, 6, device=dev()), remap, n_live, ws)
    with pytest.raises(ValueError, match='table_out'):
        hip_ops.edge_rows_apply(g, torch.zeros(E + 1, 8, device=dev()), remap, n_live, ws,
                                table_out=torch.zeros(E, 8, device=dev()))


@pytest.mark.parametrize('strategy', ['recent_edges', 'recent_nodes', 'uniform'])
def test_consumers_on_the_renumbered_graph_equal_the_parents_results_pushed_through_the_remap(strategy):
    from www2023tiger_amd import hip_ops
    from www2023tiger_amd.data.graph import Graph
    N, E = 300, 4000
    ev = row_stream(N, E, seed=5, hub=7)
    t_cut = float(np.median(ev[2]))
    # 'uniform' advances the graph's random stream: two parents with one seed, one of them renumbered
    parent = resident(N, ev, strategy=strategy, seed=5).trimmed(before=t_cut, keep_last=40)
    other = resident(N, ev, strategy=strategy, seed=5).trimmed(before=t_cut, keep_last=40)
    table = torch.from_numpy(table_of(E + 1, 172, special=True)).to(dev())
    child, remap, t_out = release(other, table)
    assert t_out.shape[0] < E // 2
    rs = np.random.RandomState(3)
    q = torch.from_numpy(np.concatenate([rs.randint(0, N, 500), ev[0][-200:], ev[1][-200:]])).to(dev())
    qt = torch.from_numpy(np.concatenate([rs.uniform(t_cut, ev[2][-1] + 2, 500), ev[2][-200:], ev[2][-200:] + 1])).to(dev())
    r64 = remap.long()
    for K in (1, 10):
        for _ in range(2):
            got, want = child.sample_device(q, qt, K), parent.sample_device(q, qt, K)
            for i, nm in ((0, 'nbr'), (2, 'ts'), (3, 'dir')):
                assert torch.equal(got[i], want[i]), f'{strategy} K={K} {nm}'
            assert torch.equal(got[1], r64[want[1]]), f'{strategy} K={K} eid'   # (a padded slot: row 0 -> row 0)
            assert int(got[1].min()) >= 0
            a = hip_ops.gather_rows(t_out, got[1])
            b = hip_ops.gather_rows(table, want[1])
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f'{strategy} K={K} rows'
    assert bool((got[0] != 0).any()) and not torch.equal(got[1], want[1])
    if strategy == 'recent_edges':
        qn, tn = q.cpu().numpy(), qt.cpu().numpy()
        hg, hw = child.get_history(qn, tn, 7), parent.get_history(qn, tn, 7)
        for i in (0, 2, 3):
            np.testing.assert_array_equal(hg[i], hw[i])
        np.testing.assert_array_equal(hg[1], remap.cpu().numpy().astype(np.int64)[hw[1]])
        cand = torch.arange(1, N, 3, device=dev())
        col_of = hip_ops.catalogue_index(cand, N)
        a = hip_ops.seen_mask(child, q, qt, col_of, cand.numel())
        assert torch.equal(a, hip_ops.seen_mask(parent, q, qt, col_of, cand.numel())) and not bool(a.all())
