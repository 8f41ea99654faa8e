"""The journal kernels on the GPU (tg_journal.hip): pack / splice of T-CSR rows, the row scatter and the bit scatter, each
against its host twin with torch.equal - the cases of tests/test_journal_host.py, where the twins are held against numpy."""
import numpy as np
import pytest
import torch

from _journal_ref import (CASE_NAMES, SCATTER_ROWS, children, events, graph_cases, pack_ref, scatter_case, tensors)
from test_hip_rank import dev
from www2023tiger_amd import _lib, hip_ops
from www2023tiger_amd._lib import TigerHipError

pytestmark = pytest.mark.gpu


def same(got, ref, what):
    assert len(got) == len(ref)
    for a, b in zip(got, ref):
        a = a.cpu()
        assert a.dtype == b.dtype and a.shape == b.shape, what
        v = torch.int64 if a.dtype == torch.float64 else a.dtype
        assert torch.equal(a.view(v), b.view(v)), what


@pytest.mark.parametrize('name', CASE_NAMES)
def test_pack_and_splice_equal_the_host_twins(name):
    old, n_new, rows, new = graph_cases()[name]
    r = torch.from_numpy(rows)
    ref = hip_ops.tcsr_rows_pack(tensors(new), r)
    got = hip_ops.tcsr_rows_pack(tensors(new, dev()), r.to(dev()))
    same(got, ref, f'{name}: pack')
    code, first, ref_g = hip_ops.tcsr_rows_splice(tensors(old), n_new, r, ref[0], ref[1:])
    old_d = tensors(old, dev())
    before = [t.clone() for t in old_d]
    code_d, first_d, got_g = hip_ops.tcsr_rows_splice(old_d, n_new, r.to(dev()), got[0], got[1:])
    assert (code, first, code_d, first_d) == (0, -1, 0, -1)
    same(got_g, ref_g, f'{name}: splice')
    same(got_g, tensors(new), f'{name}: splice gives the new graph')
    same(old_d, [t.cpu() for t in before], 'the parent is only read')
    assert hip_ops.tcsr_verify(got_g)[0] == 0


def test_rows_among_thousands_of_empty_rows_search_global_memory():
    """a tile whose entries span more than 2 048 rows (the window does not fit the LDS): 6 000 empty rows between two hubs"""
    from _journal_ref import arrays_of, random_row, rewritten
    rs = np.random.RandomState(5)
    N = 6100
    per = [random_row(rs, 0, N)] * N
    for v, n in ((3, 700), (6050, 900), (6099, 2)):
        per[v] = random_row(rs, n, N)
    old = arrays_of(per)
    rows = np.arange(N, dtype=np.int32)
    new = rewritten(old, [3, 6050], 6, N)
    got = hip_ops.tcsr_rows_pack(tensors(new, dev()), torch.from_numpy(rows).to(dev()))
    same(got, hip_ops.tcsr_rows_pack(tensors(new), torch.from_numpy(rows)), 'pack')
    _, _, g = hip_ops.tcsr_rows_splice(tensors(old, dev()), N, torch.from_numpy(rows).to(dev()), got[0], got[1:])
    same(g, tensors(new), 'splice')


@pytest.mark.parametrize('child', ['extended', 'merged', 'trimmed', 'without'])
def test_round_trip_over_the_rows_the_degree_diff_marks(child):
    from www2023tiger_amd.data.graph import Graph
    N, E = 300, 700
    g = Graph.from_arrays(*events(N, E, 20), strategy='recent_edges', seed=0, max_node_id=N - 1, device=dev())
    g.tcsr
    new = children(g, N, E)[child]
    bits = hip_ops.new_bitmap(N, dev())
    hip_ops.bitmap_mark_degree_diff(g, new, bits)
    rows = hip_ops.unique_compact(bits, N, N)
    n = int(rows['count'])
    rows = rows['ids'][:n].int()
    assert 0 < n < N
    off, *pack = hip_ops.tcsr_rows_pack(new, rows)
    code, _, got = hip_ops.tcsr_rows_splice(g, N, rows, off, pack)
    assert code == 0
    same(got, [t.cpu() for t in new._tensors()], child)


def test_every_refusal_of_the_splice_equals_the_host_twin():
    old, n_new, rows, new = graph_cases()['D65']
    off, *pack = pack_ref(new, rows)
    ip = old[0].copy(); ip[100] = ip[101] + 1; ip[300] = ip[301] + 1
    swapped = rows.copy(); swapped[[20, 40]] = swapped[[40, 20]]
    dup = rows.copy(); dup[7] = dup[6]
    big_id = rows.copy(); big_id[-1] = n_new
    neg = rows.copy(); neg[0] = -1
    off0 = off.copy(); off0[0] = 1
    dec = off.copy(); dec[30] = dec[29] - 1; dec[50] = dec[49] - 1
    end = off.copy(); end[-1] += 1
    far = off.copy(); far[10] = 1 << 40; far[11] = -5                 # offsets that are no index of anything
    cases = dict(swapped=(old, swapped, off), dup=(old, dup, off), big_id=(old, big_id, off), neg=(old, neg, off),
                 off0=(old, rows, off0), dec=(old, rows, dec), end=(old, rows, end), far=(old, rows, far),
                 truncated=(old, rows[:-1].copy(), off[:-1].copy()), ptr=((ip,) + old[1:], rows, off),
                 both=((ip,) + old[1:], dup, dec))
    for name, (o, r, f) in cases.items():
        ref = hip_ops.tcsr_rows_splice(tensors(o), n_new, *tensors((r, f)), tensors(pack), strict=False)
        got = hip_ops.tcsr_rows_splice(tensors(o, dev()), n_new, *tensors((r, f), dev()), tensors(pack, dev()), strict=False)
        assert ref[0] != 0 and got[:2] == ref[:2] and got[2] is None, f'{name}: {got[:2]} != {ref[:2]}'
    with pytest.raises(ValueError, match='ROWS: rows\\[7\\]'):
        hip_ops.tcsr_rows_splice(tensors(old, dev()), n_new, *tensors((dup, off), dev()), tensors(pack, dev()))


@pytest.mark.parametrize('nbytes', sorted(SCATTER_ROWS))
def test_scatter_equals_the_host_twin_at_every_row_width(nbytes):
    for D in (0, 1, 65, 300, 2100):
        dst, ids, src = scatter_case(nbytes, max(301, D + 37), D, nbytes + D)
        ref = dst.clone()
        hip_ops.node_rows_scatter([(src, ref)], ids)
        got = dst.to(dev())
        hip_ops.node_rows_scatter([(src.to(dev()), got)], ids.to(dev()))
        assert got.cpu().numpy().tobytes() == ref.numpy().tobytes(), f'{nbytes} bytes, {D} rows'


def test_scatter_takes_eight_tables_and_checks_every_id():
    cases = [scatter_case(nb, 5000, 4300, i) for i, nb in enumerate(sorted(SCATTER_ROWS))]
    ids = cases[0][1]
    refs = [d.clone() for d, _, _ in cases]
    hip_ops.node_rows_scatter([(s, r) for (_, _, s), r in zip(cases, refs)], ids)
    tabs = [(s.to(dev()), d.to(dev())) for d, _, s in cases]
    hip_ops.node_rows_scatter(tabs, ids.to(dev()))
    for (_, d), ref in zip(tabs, refs):
        assert d.cpu().numpy().tobytes() == ref.numpy().tobytes()
    src = cases[7][2]
    ref = torch.full((50, 172), 7.0)
    got = ref.to(dev())
    hip_ops.node_rows_scatter([(src, ref)], ids)
    hip_ops.node_rows_scatter([(src.to(dev()), got)], ids.to(dev()))          # most ids are no row of this destination
    assert got.cpu().numpy().tobytes() == ref.numpy().tobytes() and not torch.equal(ref, torch.full((50, 172), 7.0))
    with pytest.raises(TigerHipError, match='invalid argument'):              # overlap
        t = torch.zeros(40, 4, device=dev())
        hip_ops.node_rows_scatter([(t[:10], t)], ids.to(dev()))


@pytest.mark.parametrize('n_ids', [66, 129, 70001])
def test_bit_scatter_equals_the_host_twin(n_ids):
    rs = np.random.RandomState(n_ids)
    for ids in (np.array([62, 63, 64, 65, n_ids - 1]), np.arange(n_ids), np.zeros(0, dtype=np.int64),
                np.sort(rs.choice(n_ids, n_ids // 3, replace=False))):
        ids = torch.from_numpy(np.unique(ids).astype(np.int32))
        flags = torch.from_numpy(rs.randint(0, 3, ids.numel()).astype(np.uint8))
        for start in (np.zeros(hip_ops.bitmap_words(n_ids), np.int64),
                      hip_ops.host_bitmap(rs.choice(n_ids, n_ids // 2, replace=False), n_ids)):
            ref = torch.from_numpy(start.copy())
            hip_ops.bitmap_scatter(flags, ids, ref, n_ids)
            got = torch.from_numpy(start.copy()).to(dev())
            hip_ops.bitmap_scatter(flags.to(dev()), ids.to(dev()), got, n_ids)
            assert torch.equal(got.cpu(), ref)
