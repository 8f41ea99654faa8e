"""The T-CSR verifier without a GPU: tg_tcsr_verify_host against the numpy reference on clean graphs, their children and
graphs with one word changed - every comparison exact -, and Graph.state_dict / from_state_dict on host-only graphs: what
round-trips, what continues, what is refused."""
import io

import numpy as np
import pytest
import torch

from _verify_ref import (CLEAN, ENDS, EID_RANGE, NBR_RANGE, PTR_ORDER, TS_NAN, TS_ORDER, changed, clean, host_verify,
                         inner_entry, one_word_cases, same_result, verify_numpy)
from www2023tiger_amd import hip_ops
from www2023tiger_amd._lib import lib
from www2023tiger_amd.data.graph import Graph

NAMES = list(CLEAN)


def host_graph(name, strategy='recent_nodes', seed=None):
    N, ev, rows, _ = clean(name)
    return Graph.from_arrays(*ev, strategy=strategy, seed=seed, max_node_id=N - 1), ev, rows


def children(name):
    """-> list of (label, host-only child graph, eid_rows) over the clean graph `name`"""
    g, ev, rows = host_graph(name)
    N, E = g.num_node, len(ev[0])
    t = g._t_last if E else 0.0
    new = (np.array([0, N - 1]), np.array([N - 1, N - 1]), np.array([t, t + 1.0]), np.array([rows, rows + 1]))
    out = [('extended', g.extended(*new), rows + 2), ('trimmed', g.trimmed(keep_last=1), rows)]
    if N > 2:
        out.append(('without', g.without(nodes=[N // 2], eids=[1]), rows))
    remap, _, eid_out = hip_ops.edge_rows_host(g, None, rows)
    out.append(('renumbered', g.renumbered(remap, eid_out), rows))
    return out


@pytest.mark.parametrize('name', NAMES)
def test_clean_graphs_and_their_children_are_clean(name):
    N, ev, rows, h = clean(name)
    before = [a.copy() for a in h]
    rc, got = host_verify(h, rows)
    assert rc == 0
    same_result(got, verify_numpy(h, rows), name)
    assert got[0] == 0 and got[1] == [-1] * 6
    assert got[2] == (float(ev[2].max()) if len(ev[2]) else -np.inf)
    for a, b in zip(h, before):
        np.testing.assert_array_equal(a, b, err_msg='the input is only read')
    for label, child, r in children(name):
        hc = child._host_tcsr()
        rc, got = host_verify(hc, r)
        assert rc == 0
        same_result(got, verify_numpy(hc, r), f'{name} {label}')
        assert got[0] == 0, f'{name} {label}: {hip_ops.TCSR_VERIFY_TEXT(got[0], got[1])}'
        same_result(hip_ops.tcsr_verify_host(child, r), got, f'{name} {label} (hip_ops)')


@pytest.mark.parametrize('name', NAMES)
def test_one_changed_word(name):
    N, ev, rows, h = clean(name)
    cases = one_word_cases(h, rows)
    assert len(cases) >= 6
    for label, arrays, r, cls in cases:
        rc, got = host_verify(arrays, r)
        assert rc == 0
        want = verify_numpy(arrays, r)
        same_result(got, want, f'{name} {label}')
        if cls:
            assert got[0] & cls, f'{name} {label}: class {cls} is not raised ({got})'
        else:
            assert got[0] == 0, f'{name} {label}: a legal change is refused ({got})'


def test_the_changes_hit_every_class_somewhere():
    seen = 0
    for name in NAMES:
        N, ev, rows, h = clean(name)
        for label, arrays, r, cls in one_word_cases(h, rows):
            seen |= host_verify(arrays, r)[1][0]
    assert seen == 63


def test_the_smaller_index_wins_and_classes_combine():
    N, ev, rows, h = clean('N65-E200')
    P = len(h[1])
    a = [x.copy() for x in h]
    a[2][[7, 300]] = [N, -5]           # NBR_RANGE twice
    a[1][[11, 399]] = np.nan           # TS_NAN twice
    a[3][[350, 20]] = [rows + 9, rows]  # EID_RANGE twice
    p, b, e = inner_entry(h, 3)
    a[1][p] = h[1][p - 1] - 0.5        # TS_ORDER
    p2, _, _ = inner_entry(h, 6)
    a[1][p2] = h[1][p2 - 1] - 0.5
    rc, got = host_verify(a, rows)
    assert rc == 0
    same_result(got, verify_numpy(a, rows), 'several classes')
    assert got[0] == TS_ORDER | TS_NAN | NBR_RANGE | EID_RANGE
    assert got[1] == [-1, -1, p, 11, 7, 20] and p < p2
    # a decrease right behind a NaN is no violation (a comparison with a NaN), nor is the NaN itself one of this class
    a = changed(h, 1, p - 1, np.nan)
    rc, got = host_verify(a, rows)
    same_result(got, verify_numpy(a, rows), 'nan in front')
    assert got[0] == TS_NAN and got[1][3] == p - 1


@pytest.mark.parametrize('break_', ['ends', 'ptr'])
def test_ts_order_is_suppressed_without_row_bounds(break_):
    N, ev, rows, h = clean('N65-E200')
    p, b, e = inner_entry(h, 2)
    a = [x.copy() for x in changed(h, 1, p, h[1][p - 1] - 1.0)]
    assert host_verify(a, rows)[1][0] == TS_ORDER
    if break_ == 'ends':
        a[0][N] += 1
    else:
        v = N - 3
        a[0][v + 1] = a[0][v] - 1
    rc, got = host_verify(a, rows)
    assert rc == 0
    same_result(got, verify_numpy(a, rows), break_)
    assert got[0] == (ENDS if break_ == 'ends' else PTR_ORDER) and got[1][2] == -1


def test_max_time_of_signed_zeros_and_no_time():
    N, ev, rows, h = clean('tiny')
    for vals in ((-0.0,), (-0.0, 0.0), (np.nan,), (-np.inf,)):
        a = [x.copy() for x in h]
        a[1][:] = vals[0]
        a[1][-1] = vals[-1]
        rc, got = host_verify(a, rows)
        same_result(got, verify_numpy(a, rows), str(vals))


def test_symbols_and_abi():
    assert lib.tg_abi_version() == 9
    for name in ('tg_tcsr_verify', 'tg_tcsr_verify_host', 'tg_tcsr_verify_workspace_bytes'):
        assert getattr(lib, name) is not None
    assert lib.tg_tcsr_verify_workspace_bytes(0, 1) == 64                # no tile, one chunk of row bounds
    assert lib.tg_tcsr_verify_workspace_bytes(2049, 256) == 64 * (2 + 2)  # 257 row bounds
    assert lib.tg_tcsr_verify_workspace_bytes(5, 0) == 0 and lib.tg_tcsr_verify_workspace_bytes(-1, 5) == 0
    N, ev, rows, h = clean('tiny')
    from www2023tiger_amd._lib import TG_EINVAL
    import ctypes as C
    from www2023tiger_amd._lib import TgTcsr, ptr
    g = TgTcsr(N, len(h[1]), *(ptr(a) for a in h))
    assert lib.tg_tcsr_verify_host(C.byref(g), -1, None) == TG_EINVAL
    text = hip_ops.TCSR_VERIFY_TEXT(NBR_RANGE | TS_NAN, [-1, -1, -1, 4, 9, -1])
    assert 'NBR_RANGE' in text and 'entry 9' in text and 'TS_NAN' in text and 'entry 4' in text and 'ENDS' not in text


def test_wrapper_refuses_wrong_arrays():
    N, ev, rows, h = clean('tiny')
    with pytest.raises(ValueError, match='nbr'):
        hip_ops.tcsr_verify_host((h[0], h[1], h[2].astype(np.int64), h[3]))
    with pytest.raises(ValueError, match='one entry each'):
        hip_ops.tcsr_verify_host((h[0], h[1], h[2][:-1].copy(), h[3]))
    with pytest.raises(ValueError):
        hip_ops.tcsr_verify_host((h[0][:1], h[1], h[2], h[3]))


# ---- Graph.state_dict / from_state_dict on host-only graphs -----------------------------------------------------------
def through_a_file(sd):
    f = io.BytesIO()
    torch.save(sd, f)
    f.seek(0)
    return torch.load(f, weights_only=True)


def arrays_equal(a, b, what=''):
    for x, y in zip(a._host_tcsr(), b._host_tcsr()):
        assert x.dtype == y.dtype and x.shape == y.shape, what
        np.testing.assert_array_equal(x.view(np.int64 if x.itemsize == 8 else np.int32),
                                      y.view(np.int64 if y.itemsize == 8 else np.int32), err_msg=what)


@pytest.mark.parametrize('name', NAMES)
def test_state_dict_round_trip(name):
    g, ev, rows = host_graph(name, strategy='recent_edges', seed=5)
    g.rng.randint(0, 10, size=7)   # somewhere inside the stream
    for label, src, r in [('root', g, rows)] + children(name):
        src.alpha = 0.25
        sd = through_a_file(src.state_dict())
        assert sd['format'] == 'tiger-graph' and sd['version'] == 1
        back = Graph.from_state_dict(sd, device='cpu', eid_rows=r)
        arrays_equal(back, src, f'{name} {label}')
        assert back.num_node == src.num_node and back._t_last == float(src._t_last)
        assert back._time_ordered == src._time_ordered
        assert (back.strategy, back.seed, back.alpha) == (src.strategy, src.seed, 0.25)
        assert back.serial != src.serial and back._events is None and back._dev is None
        a, b = src.rng.get_state(), back.rng.get_state()
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]
        assert back.rng is not src.rng
        np.testing.assert_array_equal(back.rng.randint(0, 1 << 30, size=5), src.rng.randint(0, 1 << 30, size=5))


def test_t_last_above_the_maximum_survives_a_trim():
    g, ev, rows = host_graph('N65-E200')
    t = g.trimmed(before=float(np.median(ev[2]))).trimmed(keep_last=0)
    assert len(t._host_tcsr()[1]) == 0 and t._t_last == float(ev[2].max())
    back = Graph.from_state_dict(through_a_file(t.state_dict()), device='cpu')
    assert back._t_last == float(ev[2].max())
    with pytest.raises(ValueError, match='before the latest event'):
        back.extended([1], [2], [back._t_last - 1.0], [7])
    arrays_equal(back.extended([1], [2], [back._t_last], [7]), t.extended([1], [2], [t._t_last], [7]), 'extended after')


def test_extended_on_the_loaded_graph_equals_extended_on_the_original():
    g, ev, rows = host_graph('N65-E200')
    g = g.without(nodes=[3]).trimmed(keep_last=4)
    back = Graph.from_state_dict(through_a_file(g.state_dict()), device='cpu', eid_rows=rows)
    t = g._t_last
    batch = (np.array([3, 9, 64]), np.array([9, 9, 70]), np.array([t, t + 1.0, t + 1.0]), np.array([300, 301, 302]))
    a, b = g.extended(*batch, num_node='auto'), back.extended(*batch, num_node='auto')
    assert a.num_node == b.num_node == 71
    arrays_equal(a, b, 'extended')
    arrays_equal(a.trimmed(keep_last=2), b.trimmed(keep_last=2), 'trimmed after')


def test_refusals_name_class_and_index():
    g, ev, rows = host_graph('N65-E200')
    sd = g.state_dict()
    P = sd['ts'].numel()

    def bad(**kw):
        out = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in sd.items()}
        for k, v in kw.items():
            if isinstance(v, tuple):
                out[k][v[0]] = v[1]
            else:
                out[k] = v
        return out

    p, b, e = inner_entry(g._host_tcsr(), 1)
    cases = [(bad(nbr=(17, 65)), r'NBR_RANGE.*entry 17'), (bad(nbr=(0, -1)), r'NBR_RANGE.*entry 0'),
             (bad(ts=(33, float('nan'))), r'TS_NAN.*entry 33'),
             (bad(ts=(p, float(sd['ts'][p - 1]) - 1.0)), rf'TS_ORDER.*entry {p}\b'),
             (bad(indptr=(0, 1)), r'ENDS.*row bound 0'), (bad(indptr=(65, P + 2)), r'ENDS.*row bound 65'),
             (bad(indptr=(10, int(sd['indptr'][9]) - 1)), r'PTR_ORDER.*row 9'),
             (bad(eid=(5, rows)), r'EID_RANGE.*entry 5'),
             (bad(format='tiger'), 'not a saved graph'), (bad(version=2), 'version 2'),
             (bad(num_node=64), 'num_node'), (bad(nbr=sd['nbr'].long()), 'nbr'), (bad(ts=sd['ts'][:-1]), 'one entry each'),
             (bad(indptr=sd['indptr'][:-1]), 'num_node'), (bad(t_last=float(ev[2].max()) - 1.0), 'below the largest time'),
             (bad(t_last=float('nan')), 'below the largest time'), (bad(rng_key=sd['rng_key'][:5]), 'MT19937')]
    for case, pattern in cases:
        with pytest.raises(ValueError, match=pattern):
            Graph.from_state_dict(case, device='cpu', eid_rows=rows)
    Graph.from_state_dict(bad(eid=(5, rows)), device='cpu')                       # no table named: the eids are not checked
    Graph.from_state_dict(bad(t_last=float(ev[2].max()) + 5.0), device='cpu')     # above the maximum is legal
    Graph.from_state_dict(bad(t_last=float(ev[2].max()) - 1.0), device='cpu', verify=False)   # trusted
    sd2 = dict(sd)
    del sd2['alpha']
    with pytest.raises(ValueError, match='alpha'):
        Graph.from_state_dict(sd2, device='cpu')
