"""tg_walk_candidates_host (the host twin of the walk-candidate entry) against the numpy / dict reference of
tests/_walk_ref.py, array for array: ids, counts, n_valid, n_distinct.  The argument errors of both entries come back
before any launch, so they need no GPU either.  The check_* functions take the device the queries live on: 'cpu' runs the
host twin, tests/test_hip_walk.py runs the same cases through the kernel."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import _walk_ref as R


def run_case(N, ev, ref, src, ts, Cn, fanout, take, device, what, **flags):
    """one call on `device` (and, off the CPU, the host twin as well) against the reference -> the reference's rows"""
    want = ref.rows(src, ts, Cn, fanout, take, **flags)
    R.assert_same(R.library_rows(R.library_graph(N, ev, device), src, ts, Cn, fanout, take, device, **flags), want, what)
    if str(device) != 'cpu':
        R.assert_same(R.library_rows(R.library_graph(N, ev, 'cpu'), src, ts, Cn, fanout, take, 'cpu', **flags), want,
                      what + ' (host twin)')
    return want


def check_small(walk, Cn, exclude_seen, device):
    N, ev, ref, src, ts = R.small_case()
    fanout, take = walk
    want = run_case(N, ev, ref, src, ts, Cn, fanout, take, device, f'{R.walk_id(walk)} C={Cn} seen={exclude_seen}',
                    exclude_seen=exclude_seen)
    n = want['n_distinct']
    # what the generator has to keep covering
    if Cn == 512:
        assert (n <= Cn).all()                                   # nothing is truncated
    if not exclude_seen:
        assert 41 <= int((n == 0).sum()) <= 47                   # node 0, nodes without entries, times before everything
    if walk == R.DEFAULT and not exclude_seen and Cn in (16, 64):
        cut = np.flatnonzero(n > Cn)
        full = ref.rows(src[cut], ts[cut], Cn + 1, fanout, take)['counts']
        inside = full[:, Cn - 1] == full[:, Cn]                  # the cut falls inside a run of equal weights
        assert len(cut) > (n > 0).sum() // 2 and inside.sum() > len(cut) // 2
        if Cn == 64:
            assert (len(cut), int(inside.sum())) == (217, 210)
    return want


@pytest.mark.parametrize('exclude_seen', (False, True), ids=('all', 'exclude-seen'))
@pytest.mark.parametrize('Cn', R.CS)
@pytest.mark.parametrize('walk', R.WALKS, ids=R.walk_id)
def test_host_twin_equals_the_reference(walk, Cn, exclude_seen):
    check_small(walk, Cn, exclude_seen, 'cpu')


def check_keep_self(device):
    N, ev, ref, _, _ = R.small_case()
    src, ts = R.self_loop_queries()
    assert len(src) >= 10
    for walk in (((64,), (True,)), R.DEFAULT):
        kept = run_case(N, ev, ref, src, ts, 512, *walk, device, 'keep_self', keep_self=True)
        dropped = run_case(N, ev, ref, src, ts, 512, *walk, device, 'self dropped')
        assert ((kept['ids'] == src[:, None]).sum(1) == 1).all() and not (dropped['ids'] == src[:, None]).any()
        assert (kept['n_distinct'] == dropped['n_distinct'] + 1).all()
    both = run_case(N, ev, ref, src, ts, 512, *R.DEFAULT, device, 'both flags', keep_self=True, exclude_seen=True)
    assert not (both['ids'] == src[:, None]).any()               # a self loop makes the source one of its own seen nodes


def test_keep_self_on_the_self_loops():
    check_keep_self('cpu')


def check_sweep(n, device):
    N, ev, src, ts = R.sweep_case(n)
    ref = R.WalkRef(N, *ev[:3])
    assert len(ref.prefix(R.SWEEP_S, ts[0])) == n
    plain = run_case(N, ev, ref, src, ts, 64, R.SWEEP_FANOUT, R.SWEEP_TAKE, device, f'prefix {n}')
    seen = run_case(N, ev, ref, src, ts, 64, R.SWEEP_FANOUT, R.SWEEP_TAKE, device, f'prefix {n} exclude_seen', exclude_seen=True)
    if n:
        level1 = set(ref.last(R.SWEEP_S, ts[0], 4).tolist())
        assert R.SWEEP_X not in level1                           # X is reached at level 3 only, and seen long ago
        assert {R.SWEEP_X, R.SWEEP_Y} <= set(plain['ids'][0].tolist())
        assert seen['ids'][0].tolist()[:2] == [R.SWEEP_Y, 0] and seen['n_distinct'][0] == 1
    else:
        assert plain['n_distinct'][0] == 0 and seen['n_distinct'][0] == 0


@pytest.mark.parametrize('n', R.SWEEP_PREFIXES)
def test_exclude_seen_sweeps_the_whole_prefix(n):
    check_sweep(n, 'cpu')


def check_degrees(device):
    N, ev, src, ts = R.degree_case()
    ref = R.WalkRef(N, *ev[:3])
    want = run_case(N, ev, ref, src, ts, 64, (64,), (True,), device, 'degrees 63 / 64 / 65')
    assert want['n_distinct'].tolist() == [63, 64, 64]
    assert want['ids'][2, 0] == 301 and 300 not in want['ids'][2]    # the oldest of 65 entries is not among the last 64


def test_degrees_around_the_largest_fan_out():
    check_degrees('cpu')


def check_at_caps(device):
    N, ev, ref, src, ts = R.small_case()
    pick = np.r_[0:40, 295:300]
    for fanout, take in R.AT_CAPS:
        run_case(N, ev, ref, src[pick], ts[pick], R.MAX_ENDPOINTS, fanout, take, device, f'at the cap {fanout}')


def test_fan_outs_exactly_at_the_caps():
    check_at_caps('cpu')


def check_strides(device):
    N, ev, src, ts = R.stride_case()
    ref = R.WalkRef(N, *ev[:3])
    want = run_case(N, ev, ref, src, ts, R.MAX_ENDPOINTS, R.STRIDE_FANOUT, R.STRIDE_TAKE, device, 'strides')
    assert want['n_distinct'][0] >= 1500 and (want['counts'][0, :want['n_valid'][0]] == 1).all()
    run_case(N, ev, ref, src, ts, 100, R.STRIDE_FANOUT, R.STRIDE_TAKE, device, 'strides, truncated')


def test_power_of_two_strides_fill_the_table():
    check_strides('cpu')


def check_derived_graphs(device):
    """Graph.trimmed(keep_last=M) and Graph.extended(batch) against the reference over the surviving / concatenated events"""
    N, ev, ref, src, ts = R.small_case()
    src, ts = src[-60:], ts[-60:]
    g = R.library_graph(N, ev, device)
    if str(device) != 'cpu':
        g.tcsr   # resident: trimmed and extended then run on the device
    for M in (3, 12):
        want = ref.trimmed(M).rows(src, ts, 64, *R.DEFAULT, exclude_seen=True)
        R.assert_same(R.library_rows(g.trimmed(keep_last=M), src, ts, 64, *R.DEFAULT, device, exclude_seen=True), want, f'trimmed {M}')
        assert not np.array_equal(want['ids'], ref.rows(src, ts, 64, *R.DEFAULT, exclude_seen=True)['ids'])
    cut = len(ev[0]) - 500
    old, new = tuple(a[:cut] for a in ev), tuple(a[cut:] for a in ev)
    parent = R.library_graph(N, old, device)
    if str(device) != 'cpu':
        parent.tcsr
    child = parent.extended(*(torch.from_numpy(a).to(device) for a in new))
    R.assert_same(R.library_rows(child, src, ts, 64, *R.DEFAULT, device), ref.rows(src, ts, 64, *R.DEFAULT), 'extended')
    R.assert_same(R.library_rows(parent, src, ts, 64, *R.DEFAULT, device), R.WalkRef(N, *old[:3]).rows(src, ts, 64, *R.DEFAULT),
                  'the parent stays')


def test_trimmed_and_extended_graphs():
    check_derived_graphs('cpu')


def _tcsr(g):
    from www2023tiger_amd import _lib
    from www2023tiger_amd._lib import ptr
    h = g._host_tcsr()
    return _lib.TgTcsr(g.num_node, len(h[1]), *(ptr(a) for a in h)), h


def test_argument_errors_of_both_entries():
    """every refusal comes back before anything is launched or written: the device entry is called here with HOST
    pointers, which it never dereferences on these paths"""
    from www2023tiger_amd import _lib
    from www2023tiger_amd._lib import lib, ptr
    N, ev, _, src, ts = R.small_case()
    tc, _keep = _tcsr(R.library_graph(N, ev))
    Cn = 16
    ids, counts = np.full((3, Cn), -7, np.int64), np.full((3, Cn), -7, np.int32)
    nv, nd = np.full(3, -7, np.int32), np.full(3, -7, np.int32)
    i32 = lambda *v: np.array(v, np.int32)

    def call(entry, g=C.byref(tc), B=3, s=ptr(src), t=ptr(ts), L=3, fan=i32(10, 10, 10), take=5, Cc=Cn, flags=0, o_ids=ptr(ids),
             o_counts=ptr(counts), o_nv=ptr(nv), o_nd=ptr(nd)):
        args = (g, B, s, t, L, None if fan is None else ptr(fan), take, Cc, flags, o_ids, o_counts, o_nv, o_nd)
        return entry(*args) if entry is lib.tg_walk_candidates_host else entry(*args, None)

    bad = [dict(B=-1), dict(g=None), dict(s=None), dict(t=None), dict(fan=None), dict(o_ids=None), dict(o_counts=None),
           dict(o_nv=None), dict(o_nd=None), dict(L=0), dict(L=4), dict(take=0), dict(take=8), dict(take=-1),
           dict(take=3),                                        # level 3 walked for nothing
           dict(L=2, fan=i32(3, 2), take=1), dict(L=2, fan=i32(3, 2), take=4), dict(Cc=0), dict(Cc=R.MAX_ENDPOINTS + 1),
           dict(flags=4), dict(flags=-1), dict(fan=i32(10, 0, 10)), dict(fan=i32(10, 10, R.MAX_FANOUT + 1))]
    bad += [dict(L=len(f), fan=i32(*f), take=sum(1 << l for l, b in enumerate(tk) if b)) for f, tk, _ in R.PAST_CAPS]
    for entry in (lib.tg_walk_candidates_host, lib.tg_walk_candidates):
        for kw in bad:
            assert call(entry, **kw) == _lib.TG_EINVAL, (entry.__name__, kw)
        assert call(entry, B=0, s=None, t=None, o_ids=None, o_counts=None, o_nv=None, o_nd=None) == _lib.TG_OK   # B == 0 is valid
    assert (ids == -7).all() and (counts == -7).all() and (nv == -7).all() and (nd == -7).all()
    for f, tk in R.AT_CAPS:
        assert call(lib.tg_walk_candidates_host, L=len(f), fan=i32(*f), take=sum(1 << l for l, b in enumerate(tk) if b)) == _lib.TG_OK
    # a source outside the graph is a node without entries, in both entries (the Python wrapper refuses it)
    out = np.array([1, N, -1], np.int64)
    assert call(lib.tg_walk_candidates_host, s=ptr(out)) == _lib.TG_OK
    assert nd.tolist()[1:] == [0, 0] and (ids[1:] == 0).all() and (counts[1:] == 0).all()


def test_python_wrapper_refusals_name_the_cap():
    from www2023tiger_amd import hip_ops
    N, ev, _, src, ts = R.small_case()
    g = R.library_graph(N, ev)
    s, t = torch.from_numpy(src[:3]), torch.from_numpy(ts[:3])
    for fanout, take, cap in R.PAST_CAPS:
        with pytest.raises(ValueError, match=cap):
            hip_ops.walk_candidates(g, s, t, 16, fanout=fanout, take=take)
    with pytest.raises(ValueError, match='TG_WALK_MAX_ENDPOINTS'):
        hip_ops.walk_candidates(g, s, t, R.MAX_ENDPOINTS + 1)
    with pytest.raises(ValueError, match='TG_WALK_MAX_ENDPOINTS'):
        hip_ops.walk_candidates(g, s, t, 0)
    for kw in (dict(fanout=(3, 2)),                              # the default take names a third level
               dict(fanout=(3, 2, 2), take=(True, True, False)), dict(take=(False, False, False)), dict(fanout=()),
               dict(fanout=(2, 2, 2, 2), take=(True,) * 4)):
        with pytest.raises(ValueError, match='walk_candidates'):
            hip_ops.walk_candidates(g, s, t, 16, **kw)
    with pytest.raises(ValueError, match='source id'):
        hip_ops.walk_candidates(g, torch.tensor([1, N, 2]), t, 16)
    with pytest.raises(ValueError, match='source id'):
        hip_ops.walk_candidates(g, torch.tensor([1, -1, 2]), t, 16)
    with pytest.raises(ValueError, match='3 sources'):
        hip_ops.walk_candidates(g, s, t[:2], 16)


def test_no_queries():
    from www2023tiger_amd import hip_ops
    N, ev, _, _, _ = R.small_case()
    out = hip_ops.walk_candidates(R.library_graph(N, ev), torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.float64), 16)
    assert out['ids'].shape == (0, 16) and out['counts'].shape == (0, 16) and out['n_valid'].shape == (0,)
    assert out['ids'].dtype == torch.int64 and out['counts'].dtype == torch.int32 and out['n_distinct'].dtype == torch.int32


def test_symbols_caps_and_abi_version():
    from www2023tiger_amd import _lib
    from www2023tiger_amd._lib import lib
    for name in ('tg_walk_candidates', 'tg_walk_candidates_host', 'tg_walk_candidates_lds_bytes'):
        assert getattr(lib, name) is not None
    assert lib.tg_abi_version() == 9
    assert (_lib.TG_WALK_MAX_FANOUT, _lib.TG_WALK_MAX_FRONTIER, _lib.TG_WALK_MAX_ENDPOINTS) == (R.MAX_FANOUT, R.MAX_FRONTIER,
                                                                                               R.MAX_ENDPOINTS)
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include', 'tiger_hip.h')).read()
    for name, v in (('FANOUT', R.MAX_FANOUT), ('FRONTIER', R.MAX_FRONTIER), ('ENDPOINTS', R.MAX_ENDPOINTS)):
        assert f'#define TG_WALK_MAX_{name} {v}\n' in header


def test_lds_budget():
    """at most 64 KiB per workgroup whatever the fan-out; at the default fan-out at least four workgroups fit into a
    compute unit's 160 KiB"""
    from www2023tiger_amd._lib import lib, ptr
    lds = lambda f, tk: int(lib.tg_walk_candidates_lds_bytes(len(f), ptr(np.array(f, np.int32)), sum(1 << l for l, b in enumerate(tk) if b)))
    for f, tk in R.AT_CAPS + R.WALKS:
        assert 0 < lds(f, tk) <= 64 * 1024 and lds(f, tk) % 16 == 0, (f, tk)
    assert 4 * lds(*R.DEFAULT) <= 160 * 1024
    for f, tk, _ in R.PAST_CAPS:
        assert lds(f, tk) == 0


def test_eval_recommendation_and_recommend_walk_signatures():
    import inspect
    from www2023tiger_amd import eval_utils
    from www2023tiger_amd.model.tiger import TIGE
    p = inspect.signature(eval_utils.eval_recommendation).parameters
    assert p['catalogue'].default is None and p['walk'].default is None and p['walk'].kind is inspect.Parameter.KEYWORD_ONLY
    q = inspect.signature(TIGE.recommend_walk).parameters
    assert q['C'].default == 256 and q['chunk_queries'].default == 65536 and q['uptodate'].default is None
    with pytest.raises(ValueError, match='walk'):
        eval_utils.eval_recommendation(None, None, 'cpu', [1, 2], walk=dict(C=16))
    with pytest.raises(ValueError, match='walk'):
        eval_utils.eval_recommendation(None, None, 'cpu')
    with pytest.raises(ValueError, match='walk'):
        eval_utils.eval_recommendation(None, None, 'cpu', walk=dict(C=16), catalogue_at='batch')
