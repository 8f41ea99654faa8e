"""The integer and bit-exact kernels past their grid caps.

flat_grid() launches at most FLAT_BLOCKS = 4096 workgroups; a kernel with more work strides over the rest.  Every case
here (but `uniform`, whose kernel is a single wavefront and has no capped grid) runs a kernel exactly at its cap (the last
size without a second pass) and a few items past it (a ragged second pass) - sizes from tests/_cap_ref.py, each derived
from the work items of the kernel's own launch site - and compares the whole result with numpy, the CPU oracle or the
library's host twin.  Every comparison is exact, except tg_time_encode's (the bound of test_time_encode_rounding)."""
import ctypes as C

import numpy as np
import pytest
import torch

import _cap_ref as R
from _append_ref import assert_same, host_build
from _topk_ref import numpy_seen_mask, seen_graph

pytestmark = pytest.mark.gpu


def dev():
    return torch.device('cuda', 0)


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def bits(a):
    """the bit pattern of a float array (numpy or tensor) as integers"""
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.itemsize])


# ---- T-CSR build and adversarial index: k_degree, k_tcsr_fill, k_adv_keys, k_adv_owner_keys, k_adv_fill -----------------
# k_tcsr_fill and k_adv_* take one thread per ENTRY (P = 2 E): cap P = 2^20.  k_degree takes one thread per EVENT: cap
# E = 2^20, where the entry kernels are at the end of their second pass and (+ 150 events) in a ragged third one.
@pytest.fixture(scope='module', params=[R.TCSR_E_AT, R.TCSR_E_PAST, R.TCSR_DEG_E_AT, R.TCSR_DEG_E_PAST],
                ids=['P=2^20', 'P=2^20+300', 'E=2^20', 'E=2^20+150'])
def big(request):
    """(stream, device graph, host arrays): built once per size"""
    from www2023tiger_amd.data.graph import Graph
    s = R.tcsr_stream(request.param)
    g = Graph.from_arrays(*s, strategy='recent_edges', max_node_id=R.TCSR_N - 1, device=dev())
    return s, g, host_build(R.TCSR_N, *s)


def test_tcsr_build_at_and_past_the_cap(big):
    s, g, want = big
    assert g._time_ordered and g._host is None
    got = [t.cpu().numpy() for t in g._tensors()]   # tg_tcsr_build_device
    assert g._host is None, 'the host builder ran instead'
    assert len(got[1]) == 2 * len(s[0]) >= R.CAP_THREAD
    # indptr is k_degree's counts, scanned: every node's degree, the events of a second pass included
    deg = np.bincount(s[0], minlength=R.TCSR_N) + np.bincount(s[1], minlength=R.TCSR_N)
    np.testing.assert_array_equal(np.diff(got[0]), deg, err_msg='degrees')
    assert_same(got, want, f'P = {len(got[1])}')


def test_adversarial_index_at_and_past_the_cap(big):
    from www2023tiger_amd._lib import TgTcsr, check, lib, ptr
    from www2023tiger_amd.hip_ops import stream_ptr
    s, g, h = big
    P = len(h[1])
    tc_h = TgTcsr(R.TCSR_N, P, *(ptr(a) for a in h))
    want = np.empty(P, dtype=np.float64), np.empty(P, dtype=np.float64)
    check(lib.tg_adv_index_build_host(C.byref(tc_h), ptr(want[0]), ptr(want[1])), 'tg_adv_index_build_host')
    tc = g.tcsr
    assert int(tc.num_entry) == P
    got = [torch.full((P + 8,), -7.0, dtype=torch.float64, device=dev()) for _ in range(2)]   # 64 guard bytes behind each
    nbytes = int(lib.tg_adv_index_build_device_workspace_bytes(P, R.TCSR_N))
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev())
    check(lib.tg_adv_index_build_device(C.byref(tc), ptr(got[0]), ptr(got[1]), ptr(ws), nbytes, stream_ptr(dev())),
          'tg_adv_index_build_device')
    torch.cuda.synchronize()
    for a, b, nm in zip(got, want, ('next_ts', 'first_ts')):
        assert bool((a[P:] == -7.0).all()), f'{nm}: words behind the array were written'
        np.testing.assert_array_equal(bits(a[:P]), bits(b), err_msg=nm)


# ---- samplers -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def small():
    return R.small_graph()


def _pair(small, strategy, seed=4):
    from oracle.tiger_oracle import OracleGraph
    from www2023tiger_amd.data.graph import Graph
    N, *ev = small
    return (Graph.from_arrays(*ev, strategy=strategy, seed=seed, max_node_id=N - 1, device=dev()),
            OracleGraph(*ev, strategy=strategy, seed=seed, max_node_id=N - 1))


def _same_samples(got, want, what):
    for a, b, nm in zip(got, want, ('nbr', 'eid', 'ts', 'dir')):
        assert a.dtype == b.dtype and a.shape == b.shape, (what, nm)
        np.testing.assert_array_equal(a, b, err_msg=f'{what} {nm}')


@pytest.mark.parametrize('Q', [R.Q_WAVE_AT, R.Q_WAVE_PAST])
def test_recent_nodes_one_wavefront_per_query(small, Q):
    """k_sample_recent_nodes against the oracle's per-query loop"""
    g, o = _pair(small, 'recent_nodes')
    q, t = R.queries(small[0], Q, small[3][-1], seed=Q)
    got, want = g.sample_temporal_neighbor(q, t, 5), o.sample_temporal_neighbor(q, t, 5)
    _same_samples(got, want, f'recent_nodes Q={Q}')
    assert (want[0][-5:] != 0).any(1).all()   # the last five queries - the second pass - are not empty


@pytest.mark.parametrize('Q', [R.Q_WAVE_AT, R.Q_WAVE_PAST])
def test_uniform_follows_the_mt19937_stream(small, Q):
    """k_sample_uniform against the oracle's per-query loop, two consecutive calls.  This kernel has NO capped grid: it is
    launched as one wavefront that walks all queries in order (the random stream is sequential), so nothing strides here;
    the case checks the MT19937 stream over 16 384 (+ 5) queries, far more than any other test draws.  Rows with equal
    timestamps may come in another order than numpy's argsort gives (test_sampler_uniform_mt19937_stream): such rows are
    compared as time-sorted multisets"""
    g, o = _pair(small, 'uniform')
    q, t = R.queries(small[0], Q, small[3][-1], seed=Q + 1)
    for rep in range(2):
        got, want = g.sample_temporal_neighbor(q, t, 5), o.sample_temporal_neighbor(q, t, 5)
        np.testing.assert_array_equal(got[2], want[2], err_msg=f'rep {rep} ts')   # timestamps: sorted, identical
        other = np.nonzero(np.any([(a != b).any(1) for a, b in zip(got, want)], axis=0))[0]
        for r in other:
            a = sorted(zip(got[2][r].tolist(), got[1][r].tolist(), got[0][r].tolist(), got[3][r].tolist()))
            b = sorted(zip(want[2][r].tolist(), want[1][r].tolist(), want[0][r].tolist(), want[3][r].tolist()))
            assert a == b, (rep, r)
        assert len(other) < Q // 2


# tg_graph.hip, tg_sample_recent_edges: `if (K <= 16)` takes k_sample_recent_edges<16> (sixteen lanes per query, cap
# 4096 * 16 = 65 536 queries), any larger K takes k_sample_recent_edges<64> (one wavefront per query, cap 16 384)
K_16_LANES, K_64_LANES = 10, 20


@pytest.mark.parametrize('Q,K', [(R.Q_WAVE_AT, K_64_LANES), (R.Q_WAVE_PAST, K_64_LANES),          # K = 20 > 16: the 64-lane form
                                 (R.Q_LANE16_AT, K_16_LANES), (R.Q_LANE16_PAST, K_16_LANES)])     # K = 10 <= 16: the 16-lane form
def test_recent_edges_both_forms(small, Q, K):
    """k_sample_recent_edges<64> and <16> against the oracle's vectorised form"""
    g, o = _pair(small, 'recent_edges')
    q, t = R.queries(small[0], Q, small[3][-1], seed=Q + K)
    got, want = g.sample_temporal_neighbor(q, t, K), o._sample_recent_edges_vectorised(q, t, K)
    _same_samples(got, want, f'recent_edges Q={Q} K={K}')
    assert (want[0][-5:] != 0).any(1).all()


# ---- seen mask: k_seen_mask, one wavefront per query -----------------------------------------------------------------------
@pytest.mark.parametrize('B', [R.Q_WAVE_AT, R.Q_WAVE_PAST])
def test_seen_mask_at_and_past_the_cap(B):
    from www2023tiger_amd import hip_ops
    from www2023tiger_amd._lib import check, lib, ptr
    from www2023tiger_amd.data.graph import Graph
    ev_src, ev_dst, ev_ts, n_nodes = seen_graph()
    eids = np.arange(1, len(ev_src) + 1, dtype=np.int64)
    src, ts, cat, rows = R.seen_case(B)
    Cn = len(cat)
    assert len(src) == B
    g_dev = Graph.from_arrays(ev_src, ev_dst, ev_ts, eids, strategy='recent_edges', max_node_id=n_nodes - 1, device=dev())
    g_host = Graph.from_arrays(ev_src, ev_dst, ev_ts, eids, strategy='recent_edges', max_node_id=n_nodes - 1)
    col_of = hip_ops.catalogue_index(torch.from_numpy(cat), n_nodes)
    want = hip_ops.seen_mask(g_host, torch.from_numpy(src), torch.from_numpy(ts), col_of, Cn).numpy()   # tg_seen_mask_host
    m8 = torch.ones(B * Cn + 64, dtype=torch.uint8, device=dev())
    m8[B * Cn:] = 0x5A                                                                                  # 64 guard bytes
    d_src, d_ts, d_col = to_dev(src), to_dev(ts), col_of.to(dev())
    check(lib.tg_seen_mask(C.byref(g_dev.tcsr), B, ptr(d_src), ptr(d_ts), Cn, ptr(d_col), ptr(m8), hip_ops.stream_ptr(dev())),
          'tg_seen_mask')
    torch.cuda.synchronize()
    assert bool((m8[B * Cn:] == 0x5A).all()), 'bytes behind the mask were written'
    got = m8[:B * Cn].reshape(B, Cn).cpu().numpy()
    assert set(np.unique(got).tolist()) <= {0, 1}
    np.testing.assert_array_equal(got.astype(bool), want)
    np.testing.assert_array_equal(got[rows].astype(bool), numpy_seen_mask(ev_src, ev_dst, ev_ts, src[rows], ts[rows], cat))
    assert not want[-5:].all() and want[-5:].any()   # the second pass cleared some columns and left some


# ---- trajectory finish: k_trajectory_finish -----------------------------------------------------------------------------
@pytest.mark.parametrize('n_nodes', [R.TRAJ_NODES_AT, R.TRAJ_NODES_PAST])
def test_trajectory_finish(n_nodes):
    from www2023tiger_amd._lib import check, lib, ptr
    from www2023tiger_amd.hip_ops import stream_ptr
    d = R.TRAJ_D
    rs = np.random.RandomState(n_nodes)
    table = rs.standard_normal((n_nodes, d)) * np.exp(rs.uniform(-20, 20, (n_nodes, 1)))
    counts = rs.randint(0, 6, n_nodes).astype(np.float64)   # zeros among them: a division by 1e-7
    counts[-3:] = (3.0, 0.0, 7.0)
    want = table / (counts[:, None] + 1e-7)
    t = torch.full((n_nodes * d + 8,), -7.0, dtype=torch.float64, device=dev())
    t[:n_nodes * d] = to_dev(table).reshape(-1)
    d_counts = to_dev(counts)
    check(lib.tg_trajectory_finish(n_nodes, d, ptr(t), ptr(d_counts), stream_ptr(dev())), 'tg_trajectory_finish')
    torch.cuda.synchronize()
    assert bool((t[n_nodes * d:] == -7.0).all())
    np.testing.assert_array_equal(bits(t[:n_nodes * d]), bits(want.reshape(-1)))


# ---- bitmap and flags: k_mark, k_mark_flags, k_bm_emit -----------------------------------------------------------------------
def _id_sets(n_ids, n_nodes, seed):
    """n_ids ids with many duplicates (half of them among 5 000 values, a run of one value) and the first and last id of
    the range, and a second set to intersect with"""
    rs = np.random.RandomState(seed)
    ids = rs.randint(0, n_nodes, n_ids).astype(np.int64)
    dup = rs.uniform(size=n_ids) < 0.5
    ids[dup] = rs.randint(0, 5000, int(dup.sum())) * 200 + 64
    ids[1000:3000] = 77
    ids[0], ids[-1], ids[-2] = n_nodes - 1, 0, n_nodes - 2     # the last ids: the ragged second pass marks them
    other = np.unique(np.concatenate([ids[::3], rs.randint(0, n_nodes, 100000), [n_nodes - 1]]))
    return ids, other


def _words(uniq, n_nodes):
    W = -(-n_nodes // 64)
    w = np.zeros(W, dtype=np.uint64)
    np.bitwise_or.at(w, uniq >> 6, np.uint64(1) << (uniq & 63).astype(np.uint64))
    return w


def _prefix(words):
    pop = np.array([bin(int(x)).count('1') for x in words], dtype=np.int64)
    return np.concatenate([[0], np.cumsum(pop)])


@pytest.mark.parametrize('n_ids,n_nodes', [(R.MARK_IDS_AT, R.BM_NODES_AT), (R.MARK_IDS_PAST, R.BM_NODES_PAST)])
def test_mark_and_unique_compact(n_ids, n_nodes):
    """tg_bitmap_mark / tg_flags_mark over 2^20 (+ 300) ids, tg_unique_compact over 16 384 (+ 6) bitmap words, against
    np.unique: ids, count, rank; with an and_bitmap the intersection and its positions; the same from byte flags"""
    from www2023tiger_amd import hip_ops
    ids, other = _id_sets(n_ids, n_nodes, seed=n_ids % 1000)
    uniq = np.unique(ids)
    W = hip_ops.bitmap_words(n_nodes)
    assert W == -(-n_nodes // 64) and W >= R.CAP_WAVE
    bm = hip_ops.new_bitmap(n_nodes, dev())
    hip_ops.bitmap_mark(to_dev(ids), bm, n_nodes)
    want_bm = _words(uniq, n_nodes)
    np.testing.assert_array_equal(bm.cpu().numpy().view(np.uint64), want_bm)
    flags = hip_ops.new_flags(n_nodes, dev())
    hip_ops.flags_mark(to_dev(ids), flags, n_nodes)
    want_flags = np.zeros(flags.numel(), dtype=np.uint8)
    want_flags[uniq] = 1
    np.testing.assert_array_equal(flags.cpu().numpy(), want_flags)

    cap = len(uniq) + 10
    rank = _prefix(want_bm)

    def check_list(out, what):
        assert int(out['count']) == len(uniq), what
        np.testing.assert_array_equal(out['ids'][:len(uniq)].cpu().numpy(), uniq, err_msg=what)
        np.testing.assert_array_equal(out['rank'].cpu().numpy().view(np.uint32), rank, err_msg=what)
        np.testing.assert_array_equal(out['bitmap'].cpu().numpy().view(np.uint64), want_bm, err_msg=what)

    check_list(hip_ops.unique_compact(bm, n_nodes, cap), 'bitmap')
    hm = hip_ops.new_bitmap(n_nodes, dev())
    hip_ops.bitmap_mark(to_dev(other), hm, n_nodes)
    out = hip_ops.unique_compact(bm, n_nodes, cap, and_bitmap=hm)
    check_list(out, 'with and_bitmap')
    both = np.intersect1d(uniq, other)
    assert 0 < len(both) < len(uniq) and both[-1] == n_nodes - 1
    assert int(out['and_count']) == len(both)
    np.testing.assert_array_equal(out['and_ids'][:len(both)].cpu().numpy(), both)
    np.testing.assert_array_equal(out['and_pos'][:len(both)].cpu().numpy(), np.searchsorted(uniq, both))
    np.testing.assert_array_equal(out['and_rank'].cpu().numpy().view(np.uint32), _prefix(_words(both, n_nodes)))
    check_list(hip_ops.unique_compact(None, n_nodes, cap, flags=flags), 'from flags')


# ---- hits: k_hits ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B', [R.HITS_B_AT, R.HITS_B_PAST])
def test_hits(B):
    from www2023tiger_amd import hip_ops
    rs = np.random.RandomState(B % 1000)
    center = rs.randint(0, 30, B).astype(np.int64) + (1 << 33)    # ids that differ in the high word only do not hit
    nbr = rs.randint(0, 30, (B, R.HITS_K)).astype(np.int64) + (1 << 33)
    nbr[rs.uniform(size=nbr.shape) < 0.1] -= 1 << 33
    nbr[-1] = center[-1]
    out = hip_ops.hits(to_dev(center), to_dev(nbr)).cpu().numpy()
    np.testing.assert_array_equal(out, (center[:, None] == nbr).astype(np.float32))


# ---- anonymized_reindex: k_anon_reindex (H <= 64), k_anon_reindex2 (H > 64) ---------------------------------------------------
@pytest.mark.parametrize('H', [8, 64, 100])
@pytest.mark.parametrize('n', [R.Q_WAVE_AT, R.Q_WAVE_PAST])
def test_anonymized_reindex(n, H):
    from oracle import tiger_oracle as O
    from www2023tiger_amd import hip_ops
    rs = np.random.RandomState(n + H)
    hist = rs.randint(1, max(3, H // 2), (n, H)).astype(np.int64) * 1000003   # duplicates in every row
    hist[rs.uniform(size=hist.shape) < 0.2] = 0                              # padding
    hist[-1, :] = np.arange(1, H + 1)                                        # the last row: all distinct
    hist[-2, :] = 0
    out = hip_ops.anonymized_reindex(to_dev(hist)).cpu().numpy()
    np.testing.assert_array_equal(out, O.anonymized_reindex(hist))


# ---- gather_rows / memory_scatter: k_gather_rows, k_memory_scatter -------------------------------------------------------------
NAN_PAYLOAD = 0x7FC12345


def _payload_table(rows, width, seed):
    """float32 [rows, width]: random values with NaN payloads, infinities and both zeros among them"""
    rs = np.random.RandomState(seed)
    t = rs.standard_normal((rows, width)).astype(np.float32)
    odd = rs.uniform(size=t.shape) < 0.02
    t.view(np.uint32)[odd] = np.array([NAN_PAYLOAD, 0xFFC00001, 0x7F800000, 0x80000000, 0x00000001],
                                      dtype=np.uint32)[rs.randint(0, 5, int(odd.sum()))]
    return t


@pytest.mark.parametrize('with_ts', [False, True])
@pytest.mark.parametrize('n', [R.ROWS_AT, R.ROWS_PAST])
def test_gather_rows(n, with_ts):
    from www2023tiger_amd import hip_ops
    rs = np.random.RandomState(n)
    table = _payload_table(R.ROW_TABLE, R.ROW_W, 1)
    ts_table = _payload_table(R.ROW_TABLE, 1, 2).reshape(-1)
    ids = rs.randint(0, R.ROW_TABLE, n).astype(np.int64)
    ids[-3:] = (R.ROW_TABLE - 1, 0, ids[0])
    res = hip_ops.gather_rows(to_dev(table), to_dev(ids), to_dev(ts_table) if with_ts else None)
    out = res[0] if with_ts else res
    assert out.shape == (n, R.ROW_W)
    np.testing.assert_array_equal(bits(out), bits(table[ids]))
    if with_ts:
        np.testing.assert_array_equal(bits(res[1]), bits(ts_table[ids]))


@pytest.mark.parametrize('n', [R.ROWS_AT, R.ROWS_PAST])
def test_memory_scatter(n):
    """tiger_hip.h promises table[ids[i]] = vals[src_index[i]], ts likewise, active = 1, and nothing about ids listed
    twice: the ids are distinct.  Rows not named keep their bit pattern (a NaN payload)."""
    from www2023tiger_amd import hip_ops
    rs = np.random.RandomState(n + 1)
    ids = np.append(rs.permutation(R.ROW_TABLE - 1)[:n - 1], R.ROW_TABLE - 1).astype(np.int64)   # the last item: the last row
    assert len(np.unique(ids)) == n
    src_index = rs.permutation(n).astype(np.int64)
    vals = _payload_table(n, R.ROW_W, 3)
    ts = _payload_table(n, 1, 4).reshape(-1)
    table = np.full((R.ROW_TABLE, R.ROW_W), NAN_PAYLOAD, dtype=np.uint32)
    ts_table = np.full(R.ROW_TABLE, NAN_PAYLOAD, dtype=np.uint32)
    active = np.zeros(R.ROW_TABLE, dtype=np.uint8)
    d_table, d_ts = to_dev(table.view(np.float32)), to_dev(ts_table.view(np.float32))
    d_active = to_dev(active)
    hip_ops.memory_scatter(d_table, d_ts, d_active, to_dev(ids), to_dev(vals), to_dev(ts), src_index=to_dev(src_index))
    table[ids] = vals.view(np.uint32)[src_index]
    ts_table[ids] = ts.view(np.uint32)[src_index]
    active[ids] = 1
    np.testing.assert_array_equal(bits(d_table), table)
    np.testing.assert_array_equal(bits(d_ts), ts_table)
    np.testing.assert_array_equal(d_active.cpu().numpy(), active)
    assert (table[np.setdiff1d(np.arange(R.ROW_TABLE), ids)] == NAN_PAYLOAD).all()


# ---- time_encode: k_time_encode ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [R.TE_ROWS_AT, R.TE_ROWS_PAST])
def test_time_encode(n):
    """The rounding test_time_encode_rounding pins - the float32 product, then the phase added in float32, as torch does -
    and its bound, 5e-7 with ts <= 3e6; the cosine itself is float64's of that float32 argument, rounded to float32."""
    from www2023tiger_amd import hip_ops
    d = R.TE_D
    rs = np.random.RandomState(n)
    w = (1 / 10 ** np.linspace(0, 9, d)).astype(np.float32)
    phi = np.linspace(-0.5, 0.5, d).astype(np.float32)
    ts = np.concatenate([[0.0, 1.0, 12345.678, 2.3e6, 2.68e6, 3.0e6], rs.uniform(0, 3e6, n - 6)]).astype(np.float32)
    ts[-2:] = (2.9999e6, 7.25)
    arg = (ts[:, None] * w[None, :]).astype(np.float32) + phi[None, :]
    assert arg.dtype == np.float32
    ref = np.cos(arg.astype(np.float64)).astype(np.float32)
    out = hip_ops.time_encode(to_dev(ts), to_dev(w), to_dev(phi)).cpu().numpy()
    assert out.shape == (n, d)
    err = np.abs(out.astype(np.float64) - ref.astype(np.float64))
    print(f'time_encode n={n}: max error {err.max():.2e}, in the second pass {err.reshape(-1)[R.CAP_THREAD:].max(initial=0):.2e}')
    assert err.max() < 5e-7
