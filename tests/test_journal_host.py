"""The journal primitives without a GPU: the host twins (tg_tcsr_rows_pack_host, tg_tcsr_rows_splice_host,
tg_node_rows_scatter_host, tg_bitmap_scatter_host) through the wrappers of hip_ops on CPU tensors, against the numpy
reference of _journal_ref.py, bit for bit."""
import numpy as np
import pytest
import torch

from _journal_ref import (CASE_NAMES, HUB, HUB_LEN, N_BIG, SCATTER_ROWS, assert_arrays, big, bit_scatter_ref, children, events,
                          graph_cases, pack_ref, scatter_case, scatter_ref, splice_ref, tensors)
from www2023tiger_amd import _lib, hip_ops
from www2023tiger_amd._lib import TigerHipError

DEV = 'cpu'


def test_the_case_graph_is_what_the_cases_promise():
    ip = big()[0]
    deg = np.diff(ip)
    assert len(deg) == N_BIG and deg[HUB] == HUB_LEN > 2 * 2048 and (deg == 0).sum() > 100
    for name in ('D2049', 'all-dirty', 'grown-dirty-new-ids'):
        rows = graph_cases()[name][2]
        assert rows[0] == 0 and HUB in rows and N_BIG - 1 in rows


@pytest.mark.parametrize('name', CASE_NAMES)
def test_pack_equals_the_reference(name):
    _, n_new, rows, new = graph_cases()[name]
    ref = pack_ref(new, rows)
    got = hip_ops.tcsr_rows_pack(tensors(new, DEV), torch.from_numpy(rows).to(DEV))
    assert_arrays(got, ref, name)
    assert int(got[0][-1]) == got[1].numel() == got[2].numel() == got[3].numel()


@pytest.mark.parametrize('name', CASE_NAMES)
def test_splice_of_a_pack_gives_the_new_graph(name):
    old, n_new, rows, new = graph_cases()[name]
    before = [a.copy() for a in old]
    off, *pack = pack_ref(new, rows)
    assert_arrays(tensors(splice_ref(old, n_new, rows, off, pack)), new, name + ' (the reference itself)')
    r = torch.from_numpy(rows).to(DEV)
    code, first, got = hip_ops.tcsr_rows_splice(tensors(old, DEV), n_new, r, *tensors((off,), DEV), tensors(pack, DEV))
    assert (code, first) == (0, -1)
    assert_arrays(got, new, name)
    assert hip_ops.tcsr_verify_host(tuple(a.numpy() for a in got))[0] == 0
    for a, b in zip(old, before):
        assert np.array_equal(a, b), 'the parent is only read'


@pytest.mark.parametrize('child', ['extended', 'merged', 'trimmed', 'without'])
def test_round_trip_over_the_rows_the_degree_diff_marks(child):
    from www2023tiger_amd.data.graph import Graph
    N, E = 300, 700
    g = Graph.from_arrays(*events(N, E, 20), strategy='recent_edges', seed=0, max_node_id=N - 1, device='cpu')
    new = children(g, N, E)[child]
    bits = torch.zeros(hip_ops.bitmap_words(N), dtype=torch.int64)
    hip_ops.bitmap_mark_degree_diff(g, new, bits)
    rows = np.flatnonzero(np.unpackbits(bits.numpy().view(np.uint8), bitorder='little')[:N]).astype(np.int32)
    assert 0 < len(rows) < N
    old_a, new_a = g._host_tcsr(), new._host_tcsr()
    off, *pack = hip_ops.tcsr_rows_pack(tensors(new_a), torch.from_numpy(rows))
    code, _, got = hip_ops.tcsr_rows_splice(tensors(old_a), N, torch.from_numpy(rows), off, pack)
    assert code == 0
    assert_arrays(got, new_a, child)


def test_every_refusal_of_the_splice_names_its_smallest_offender():
    old, n_new, rows, new = graph_cases()['D65']
    off, *pack = pack_ref(new, rows)
    T = lambda *a: tensors(a, DEV)

    def run(rows_=rows, off_=off, pack_=pack, old_=old, strict=False):
        return hip_ops.tcsr_rows_splice(T(*old_), n_new, *T(rows_), *T(off_), T(*pack_), strict=strict)[:2]

    assert run() == (0, -1)
    bad = rows.copy(); bad[[20, 40]] = bad[[40, 20]]          # does not ascend: the smaller j
    assert run(rows_=bad) == (_lib.TG_SPLICE_ROWS, 21)
    bad = rows.copy(); bad[7] = bad[6]                        # a duplicate
    assert run(rows_=bad) == (_lib.TG_SPLICE_ROWS, 7)
    bad = rows.copy(); bad[-1] = n_new                        # no id below the new count
    assert run(rows_=bad) == (_lib.TG_SPLICE_ROWS, len(rows) - 1)
    bad = rows.copy(); bad[0] = -1
    assert run(rows_=bad) == (_lib.TG_SPLICE_ROWS, 0)
    bad = off.copy(); bad[0] = 1
    assert run(off_=bad) == (_lib.TG_SPLICE_OFF, 0)
    bad = off.copy(); bad[30] = bad[29] - 1; bad[50] = bad[49] - 1
    assert run(off_=bad)[0] == _lib.TG_SPLICE_OFF and run(off_=bad)[1] == 30
    bad = off.copy(); bad[-1] += 1                            # beyond the packed length
    assert run(off_=bad) == (_lib.TG_SPLICE_OFF, len(rows))
    assert run(off_=off[:-1].copy(), rows_=rows[:-1].copy()) == (_lib.TG_SPLICE_OFF, len(rows) - 1)  # a truncated off
    ip = old[0].copy(); ip[100] = ip[101] + 1; ip[300] = ip[301] + 1   # rows 100 and 300 of the old graph end before they begin
    assert run(old_=(ip,) + old[1:]) == (_lib.TG_SPLICE_PTR, 100)
    bad = rows.copy(); bad[7] = bad[6]                        # several classes at once: ROWS is reported first
    assert run(rows_=bad, old_=(ip,) + old[1:]) == (_lib.TG_SPLICE_ROWS, 7)
    with pytest.raises(ValueError, match='ROWS: rows\\[7\\]'):
        bad = rows.copy(); bad[7] = bad[6]
        run(rows_=bad, strict=True)
    # what the wrapper refuses before the library sees it
    with pytest.raises(ValueError, match='n_new'):
        hip_ops.tcsr_rows_splice(T(*old), N_BIG - 1, *T(rows), *T(off), T(*pack))
    with pytest.raises(ValueError, match='off must be'):
        hip_ops.tcsr_rows_splice(T(*old), n_new, *T(rows), *T(off[:-1].copy()), T(*pack))
    with pytest.raises(ValueError, match='nbr must be'):
        hip_ops.tcsr_rows_splice(T(*old), n_new, *T(rows), *T(off), T(pack[0], pack[1][:-1].copy(), pack[2]))


@pytest.mark.parametrize('nbytes', sorted(SCATTER_ROWS))
@pytest.mark.parametrize('D', [0, 1, 65, 300])
def test_scatter_equals_the_reference_at_every_row_width(nbytes, D):
    dst, ids, src = scatter_case(nbytes, 301, D, nbytes + D)
    ref = scatter_ref(dst.numpy(), ids.numpy(), src.numpy())
    dst, ids, src = dst.to(DEV), ids.to(DEV), src.to(DEV)
    hip_ops.node_rows_scatter([(src, dst)], ids)
    got = dst.cpu().numpy()
    assert got.tobytes() == ref.tobytes()


def test_scatter_takes_eight_tables_and_checks_every_id():
    cases = [scatter_case(nb, 2500, 2100, i) for i, nb in enumerate(sorted(SCATTER_ROWS))]
    ids = cases[0][1]
    refs = [scatter_ref(d.numpy(), ids.numpy(), s.numpy()) for d, _, s in cases]
    tabs = [(s.to(DEV), d.to(DEV)) for d, _, s in cases]
    hip_ops.node_rows_scatter(tabs, ids.to(DEV))
    for (_, d), ref in zip(tabs, refs):
        assert d.cpu().numpy().tobytes() == ref.tobytes()
    # ids that are no row of the destination store nothing; a shorter table reads a prefix of ids
    src = scatter_case(688, 2500, 2100, 3)[2]
    dst = torch.full((50, 172), 7.0)
    ref = scatter_ref(dst.numpy(), ids.numpy(), src.numpy())
    dst, src = dst.to(DEV), src.to(DEV)
    ref10 = scatter_ref(tabs[7][1].cpu().numpy(), ids.numpy()[:10], src[:10].cpu().numpy())
    hip_ops.node_rows_scatter([(src, dst), (src[:10].clone(), tabs[7][1])], ids.to(DEV))
    assert dst.cpu().numpy().tobytes() == ref.tobytes() and tabs[7][1].cpu().numpy().tobytes() == ref10.tobytes()
    with pytest.raises(ValueError, match='at most 8'):
        hip_ops.node_rows_scatter(tabs + tabs[:1], ids.to(DEV))
    with pytest.raises(ValueError, match='rows of 12 bytes'):
        hip_ops.node_rows_scatter([(torch.zeros(3, 3, device=DEV), torch.zeros(9, 3, device=DEV))], ids.to(DEV))
    with pytest.raises(TigerHipError, match='invalid argument'):   # overlap
        t = torch.zeros(40, 4, device=DEV)
        hip_ops.node_rows_scatter([(t[:10], t)], ids.to(DEV))


@pytest.mark.parametrize('n_ids', [66, 128, 129, 1000])
def test_bit_scatter_across_word_boundaries(n_ids):
    rs = np.random.RandomState(n_ids)
    W = hip_ops.bitmap_words(n_ids)
    for ids in (np.array([62, 63, 64, 65, n_ids - 1]), np.arange(n_ids), np.zeros(0, dtype=np.int64),
                np.sort(rs.choice(n_ids, n_ids // 3, replace=False))):
        ids = np.unique(ids).astype(np.int32)
        for flags in (np.ones(len(ids), np.uint8), np.zeros(len(ids), np.uint8), rs.randint(0, 3, len(ids)).astype(np.uint8)):
            for start in (np.zeros(W, np.int64), hip_ops.host_bitmap(rs.choice(n_ids, n_ids // 2, replace=False), n_ids)):
                ref = bit_scatter_ref(start, ids, flags, n_ids)
                bits = torch.from_numpy(start.copy()).to(DEV)
                hip_ops.bitmap_scatter(torch.from_numpy(flags).to(DEV), torch.from_numpy(ids).to(DEV), bits, n_ids)
                assert np.array_equal(bits.cpu().numpy(), ref)
                spare = np.unpackbits(bits.cpu().numpy().view(np.uint8), bitorder='little')[n_ids:]
                assert not spare.any(), 'the spare bits of the last word stay zero'
    bits = torch.zeros(W, dtype=torch.int64, device=DEV)
    hip_ops.bitmap_scatter(torch.ones(2, dtype=torch.uint8, device=DEV), torch.tensor([n_ids, -1], dtype=torch.int32, device=DEV),
                           bits, n_ids)
    assert not bits.any(), 'an id that is no bit of the bitmap stores nothing'


def test_new_symbols_resolve_and_the_abi_version_stands():
    assert _lib.lib.tg_abi_version() == 9
    for name in ('tg_tcsr_rows_pack_workspace_bytes', 'tg_tcsr_rows_pack_plan', 'tg_tcsr_rows_pack_apply',
                 'tg_tcsr_rows_splice_workspace_bytes', 'tg_tcsr_rows_splice_plan', 'tg_tcsr_rows_splice_apply',
                 'tg_node_rows_scatter', 'tg_bitmap_scatter', 'tg_tcsr_rows_pack_host', 'tg_tcsr_rows_splice_host',
                 'tg_node_rows_scatter_host', 'tg_bitmap_scatter_host'):
        assert name in _lib.SIGNATURES and getattr(_lib.lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert _lib.lib.tg_tcsr_rows_pack_workspace_bytes(-1) == 0 and _lib.lib.tg_tcsr_rows_pack_workspace_bytes(5000) >= 12
    assert _lib.lib.tg_tcsr_rows_splice_workspace_bytes(0) == 0 and _lib.lib.tg_tcsr_rows_splice_workspace_bytes(1000) >= 12000
