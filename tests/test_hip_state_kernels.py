"""The state write-back kernels through their C ABI entry points, one by one, against the NumPy state machine of
tests/_state_ref.py: tg_store_events, tg_consume_update_right(_rows), tg_mailbox_consume_gather, tg_gather_eff_rows,
tg_serve_rows, tg_adopt_rows, tg_restart_apply and tg_stream_writeback (in-call dedup and planned winners; owner
filter; rows from the caller or from the pending table; both message sources, i.e. both launch splits).

Every table is filled with distinct bit patterns - NaN payloads, infinities, both zeros - and whole tables are
compared bit for bit after every call, so a row nobody named must be untouched.  (Where node features are added to a
memory row the summands are ordinary numbers: which payload a sum of NaNs carries is not defined.)  The invariant
word is compared as a whole with the reference's, never through a mask.

The one inexact value is the mailbox's time segment, cos(fl32(fl32(dt w) + phi)): the bound is the project's own for
this cosine, 5e-7 absolute (test_hip_parity.test_time_encode_rounding), valid while |argument| <= 3e6, which the
tests assert of the reference's arguments.  Measured maximum on an MI355X over the whole module: 1.19e-7
(two units in the last place of a value below 1)."""
import ctypes as C

import numpy as np
import pytest
import torch

import _cap_ref
import _state_ref as S
from www2023tiger_amd import _lib

pytestmark = pytest.mark.gpu

TE_BOUND, TE_ARG_MAX = 5e-7, 3.0e6
T_STATE, T_EVENT = 1000.0, 2.9e6      # memory and message times lie in [0, T_STATE], event times in (T_STATE, T_EVENT]
WIDTHS = [(4, 4), (8, 20), (64, 64), (64, 68), (172, 172), (260, 4)]
NAN_PAYLOAD = 0x7FC12345
MEASURED = {'te': 0.0}
lib, ptr = _lib.lib, _lib.ptr


def dev():
    return torch.device('cuda:0')


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def payload(shape, rs, plain=False):
    """float32 values, all different with near certainty; unless `plain`, NaN payloads, infinities, both zeros and a
    denormal among them"""
    t = rs.standard_normal(shape).astype(np.float32)
    if not plain:
        odd = rs.uniform(size=t.shape) < 0.03
        t.view(np.uint32)[odd] = np.array([NAN_PAYLOAD, 0xFFC00001, 0x7F800000, 0x80000000, 0x00000001],
                                          dtype=np.uint32)[rs.randint(0, 5, int(odd.sum()))]
    return t


def up(x):
    return np.nextafter(np.float32(x), np.float32(np.inf))


def make_state(n_nodes, d, d_e, msg_src, with_nf=False, with_ef=False, n_edges=64, seed=0, pending=None):
    """a mid-stream state: every table full of payload, about half of the nodes with a pending message whose times are
    consistent (right time <= message time = left time with msg_src = left, memory times <= message time)"""
    rs = np.random.RandomState(seed)
    freq = (1 / 10 ** np.linspace(0, 9, d)).astype(np.float32)
    phase = np.linspace(-0.5, 0.5, d).astype(np.float32)
    nf = payload((n_nodes, d), rs, plain=True) if with_nf else None
    ef = payload((n_edges + 1, d_e), rs) if with_ef else None
    st = S.State(n_nodes, d, d_e, msg_src, freq, phase, nf, ef)
    for k in ('left_vals', 'right_vals', 'pending_vals'):
        getattr(st, k)[:] = payload((n_nodes, d), rs, plain=with_nf)
    st.msg_vals[:] = payload(st.msg_vals.shape, rs)
    st.has_msg[:] = (rs.uniform(size=n_nodes) < 0.5) if pending is None else pending
    st.left_ts[:] = np.floor(rs.uniform(0, T_STATE, n_nodes) * 8) / 8
    st.right_ts[:] = np.floor(st.left_ts * rs.uniform(0, 1, n_nodes))
    st.msg_ts[:] = np.where(st.has_msg, st.left_ts, np.floor(st.left_ts / 2))
    st.left_active[:] = rs.uniform(size=n_nodes) < 0.5
    st.right_active[:] = rs.uniform(size=n_nodes) < 0.5
    return st


def set_pending(st, ids, flag):
    """give / take a pending message, with times that satisfy every invariant"""
    st.has_msg[ids] = flag
    if flag:
        st.msg_ts[ids] = st.left_ts[ids]


class DevState:
    """a State on the device behind a raw tg_model that carries only what the state kernels read"""

    def __init__(self, st):
        self.n = st.n_nodes
        words = np.zeros((st.n_nodes + 63) // 64 * 64, np.uint8)
        words[:st.n_nodes] = st.has_msg
        self.t = {k: to_dev(v) for k, v in st.tables().items() if k != 'has_msg'}
        self.t['has_msg'] = to_dev(np.packbits(words, bitorder='little').view(np.int64))
        self.const = [None if a is None else to_dev(a) for a in (st.nfeats, st.efeats, st.te_freq, st.te_phase)]
        m = _lib.TgModel()
        m.n_nodes, m.d, m.d_e, m.n_neighbors, m.n_head = st.n_nodes, st.d, st.d_e, 1, 2
        m.msg_src = 0 if st.msg_src == 'left' else 1
        for k, v in self.t.items():
            setattr(m, k, ptr(v))
        m.nfeats, m.efeats, m.te_freq, m.te_phase = (ptr(a) for a in self.const)
        self.m = m
        self.err = torch.zeros(1, dtype=torch.int32, device=dev())

    def word(self):
        return int(self.err.item()) & 0xFFFFFFFF

    def has_msg_words(self):
        return self.t['has_msg'].cpu().numpy().view(np.uint64)

    def tables(self):
        torch.cuda.synchronize()
        out = {k: v.cpu().numpy() for k, v in self.t.items()}
        out['has_msg'] = np.unpackbits(out['has_msg'].view(np.uint8), bitorder='little').astype(bool)
        return out


def assert_state(ds, ref, before, what, named=None):
    """whole tables bit for bit; the mailbox time segments that the reference changed (and those of the `named` nodes,
    where a rewrite may leave the same bits): within TE_BOUND"""
    got = ds.tables()
    d, d_e = ref.d, ref.d_e
    assert ref.max_te_arg <= TE_ARG_MAX, ref.max_te_arg
    for k, exp in ref.tables().items():
        a = got[k]
        if k == 'has_msg':
            assert not a[ref.n_nodes:].any(), f'{what}: has-message bits past n_nodes'
            np.testing.assert_array_equal(np.nonzero(a[:ref.n_nodes])[0], np.nonzero(exp)[0], err_msg=f'{what}: {k}')
            continue
        if k != 'msg_vals':
            np.testing.assert_array_equal(bits(a), bits(exp), err_msg=f'{what}: {k}')
            continue
        np.testing.assert_array_equal(bits(a[:, :2 * d + d_e]), bits(exp[:, :2 * d + d_e]), err_msg=f'{what}: mailbox rows')
        te, te_exp, te_old = a[:, 2 * d + d_e:], exp[:, 2 * d + d_e:], before.msg_vals[:, 2 * d + d_e:]
        written = (bits(te_exp) != bits(te_old)).any(1)
        if named is not None:
            written[named] = True
        np.testing.assert_array_equal(bits(te[~written]), bits(te_exp[~written]), err_msg=f'{what}: unnamed time segments')
        if written.any():
            assert np.isfinite(te[written]).all(), what
            err = float(np.abs(te[written].astype(np.float64) - te_exp[written]).max())
            MEASURED['te'] = max(MEASURED['te'], err)
            print(f'{what}: time segment max abs err {err:.3e} (bound {TE_BOUND:.0e}, module max {MEASURED["te"]:.3e})')
            assert err <= TE_BOUND, (what, err)


# ---- batches -----------------------------------------------------------------------------------------------------------
def make_batch(kind, n_nodes=129, seed=0):
    """-> dict(src, dst, ts (float64), ts32, eids).  Nodes 0, 63, 64, 127 and 128 - the first and last bits of the
    has-message words - are positive nodes of every batch that has room for them."""
    rs = np.random.RandomState(seed)
    if kind == 'one':
        src, dst, ts = [63], [64], [T_EVENT]
    elif kind == 'loop':
        src, dst, ts = [128], [128], [5000.5]
    elif kind == 'three':            # 2B = 6: no multiple of a block's four wavefronts; node 63 twice
        src, dst, ts = [0, 63, 127], [64, 128, 63], [2000.0, 2000.0, 2.5e6]
    elif kind.startswith('hub'):     # node 64 in every event, on either side
        B = 40
        a = rs.randint(0, n_nodes, B)
        a[:4] = (0, 63, 127, 128)
        a[a == 64] = 65
        a[7] = 64                    # one self-loop of the hub
        side = np.arange(B) % 2 == 0
        src, dst = np.where(side, 64, a), np.where(side, a, 64)
        ts = {'hub_inc': 3000.0 + 17.25 * np.arange(B), 'hub_eq': np.full(B, 7777.0),
              'hub_collapse': 2.5e6 + 0.05 * np.arange(B)}[kind]
    elif kind == 'cap':              # more winners than wavefronts of a capped grid
        B = (_cap_ref.CAP_WAVE + 6) // 2
        p = rs.permutation(np.arange(1, 2 * B + 1))
        src, dst, ts = p[:B], p[B:], np.floor(rs.uniform(T_STATE + 1, T_EVENT, B))
    else:
        raise KeyError(kind)
    src, dst, ts = np.asarray(src, np.int64), np.asarray(dst, np.int64), np.asarray(ts, np.float64)
    eids = rs.permutation(len(src)).astype(np.int64) + 1
    return dict(src=src, dst=dst, ts=ts, ts32=ts.astype(np.float32), eids=eids)


def bitmap_rank(ids, n_nodes):
    """(bitmap words, exclusive rank per word) of a node set, as tg_unique_compact leaves them"""
    W = (n_nodes + 63) // 64
    flags = np.zeros(W * 64, np.uint8)
    flags[ids] = 1
    bm = np.packbits(flags, bitorder='little').view(np.int64)
    rank = np.concatenate([[0], np.cumsum(flags.reshape(W, 64).sum(1))]).astype(np.int32)
    return bm, rank


# ---- the calls ---------------------------------------------------------------------------------------------------------
def call_store_events(ds, batch, upos, index, n_upos):
    keep = [to_dev(batch[k]) for k in ('src', 'dst', 'ts32', 'eids')] + [to_dev(upos), to_dev(index),
                                                                          to_dev(np.array([n_upos], np.int32))]
    rc = lib.tg_store_events(C.byref(ds.m), len(batch['src']), *(ptr(t) for t in keep), ptr(ds.err), None)
    assert rc == _lib.TG_OK
    return ds.word()


def call_consume(ds, upos, n_upos, rows, involved=None, row_index=None):
    keep = [to_dev(upos), to_dev(np.array([n_upos], np.int32)), to_dev(rows)]
    if row_index is None:
        keep += [to_dev(a) for a in bitmap_rank(involved, ds.n)]
        rc = lib.tg_consume_update_right(C.byref(ds.m), ptr(keep[0]), ptr(keep[1]), len(upos), ptr(keep[2]), ptr(keep[3]),
                                         ptr(keep[4]), ptr(ds.err), None)
    else:
        keep.append(to_dev(row_index))
        rc = lib.tg_consume_update_right_rows(C.byref(ds.m), ptr(keep[0]), ptr(keep[1]), len(upos), ptr(keep[2]),
                                              ptr(keep[3]), ptr(ds.err), None)
    assert rc == _lib.TG_OK
    return ds.word()


def call_writeback(ds, batch, rows, new_row, left_row, *, planned=None, owner=None, my_rank=0, new_from_pending=False,
                   offset=None, advance=0, stream=None):
    """planned = (upos, index, n_upos): the planned-winner form on the batch itself; otherwise the in-call dedup, on the
    batch or - offset: a device int64 - on the resident `stream` arrays"""
    arrays = stream if stream is not None else batch
    B = len(batch['src'])
    keep = [to_dev(arrays[k]) for k in ('src', 'dst', 'ts', 'eids')] + [to_dev(rows), to_dev(left_row)]
    io = _lib.TgWritebackIo()
    io.Bg = B
    io.src, io.dst, io.ts, io.eids, io.rows, io.left_row = (ptr(t) for t in keep)
    if new_row is not None:
        keep.append(to_dev(new_row))
        io.new_row = ptr(keep[-1])
    io.err = ptr(ds.err)
    io.new_from_pending = int(new_from_pending)
    if offset is not None:
        io.offset_dev, io.advance = ptr(offset), advance
    if owner is not None:
        keep.append(to_dev(np.asarray(owner, np.int32)))
        io.owner, io.my_rank = ptr(keep[-1]), my_rank
    if planned is not None:
        upos, index, n_upos = planned
        keep += [to_dev(np.array([n_upos], np.int32)), to_dev(np.tile(batch['ts32'], 2))]
        io.n_upos_dev, io.ts32 = ptr(keep[-2]), ptr(keep[-1])
        if len(upos):
            keep += [to_dev(upos), to_dev(index)]
            io.upos, io.index = ptr(keep[-2]), ptr(keep[-1])
    nbytes = int(lib.tg_stream_writeback_workspace_bytes(C.byref(ds.m), B))
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev())
    rc = lib.tg_stream_writeback(C.byref(ds.m), C.byref(io), ptr(ws), nbytes, None)
    assert rc == _lib.TG_OK
    torch.cuda.synchronize()
    return ds.word()


def call_consume_gather(ds, involved, count, out0):
    keep = [to_dev(involved), to_dev(np.array([count], np.int32)), to_dev(out0)]
    assert lib.tg_mailbox_consume_gather(C.byref(ds.m), ptr(keep[0]), ptr(keep[1]), len(involved), ptr(keep[2]), None) == 0
    return keep[2].cpu().numpy()


def call_gather_eff(ds, ids, rows0, ts0):
    keep = [to_dev(ids), to_dev(rows0), to_dev(ts0)]
    assert lib.tg_gather_eff_rows(C.byref(ds.m), len(ids), ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), None) == 0
    return keep[1].cpu().numpy(), keep[2].cpu().numpy()


def call_serve(ds, eff, eff_pos, msg, msg_pos, buf0):
    keep = [to_dev(a) for a in (eff, eff_pos, msg, msg_pos, buf0)]
    assert lib.tg_serve_rows(C.byref(ds.m), len(eff), ptr(keep[0]), ptr(keep[1]), len(msg), ptr(keep[2]), ptr(keep[3]),
                             ptr(keep[4]), None) == 0
    return keep[4].cpu().numpy()


def call_adopt(ds, eff, eff_pos, msg, msg_pos, buf):
    keep = [to_dev(a) for a in (eff, eff_pos, msg, msg_pos, buf)]
    assert lib.tg_adopt_rows(C.byref(ds.m), len(eff), ptr(keep[0]), ptr(keep[1]), len(msg), ptr(keep[2]), ptr(keep[3]),
                             ptr(keep[4]), None) == 0
    torch.cuda.synchronize()


def call_restart(ds, nids, hl, hr, pt):
    keep = [to_dev(a) for a in (nids, hl, hr, pt)]
    assert lib.tg_restart_apply(C.byref(ds.m), len(nids), *(ptr(t) for t in keep), None) == 0
    torch.cuda.synchronize()


def gathered_rows(st, batch, rs, plain):
    """rows [4B + 3, d] with h(t-) and h(t'+) of every position at permuted places -> (rows, new_row, left_row)"""
    B2 = 2 * len(batch['src'])
    rows = payload((2 * B2 + 3, st.d), rs, plain=plain)
    p = rs.permutation(2 * B2 + 3)
    return rows, p[:B2].astype(np.int64), p[B2:2 * B2].astype(np.int64)


# ---- every entry point at every width, with and without the feature tables --------------------------------------------
def run_entry_points(st0, batch, seed, tag):
    """every entry point once on the batch, each from the same initial state, each compared with the reference"""
    rs = np.random.RandomState(seed)
    n, d = st0.n_nodes, st0.d
    plain = st0.nfeats is not None
    pos = np.concatenate([batch['src'], batch['dst']])
    upos, index = S.winners(batch['src'], batch['dst'], batch['ts32'])
    perm = rs.permutation(len(upos))
    upos, index = upos[perm], index[perm]
    # an unnamed tail behind the live count: valid nodes outside the batch, which must stay untouched
    rest = np.setdiff1d(np.arange(n), pos)[:3]
    upos_t = np.concatenate([upos, rest])
    index_t = np.concatenate([index, np.zeros(len(rest), np.int64)])
    involved = np.unique(np.concatenate([pos, rs.randint(0, n, 9)]))

    # STEP 2's copy, capacity above the live count
    ds = DevState(st0)
    out0 = payload((len(involved) + 2, d), rs)
    out = call_consume_gather(ds, np.concatenate([involved, [0, 0]]), len(involved), out0)
    exp = out0.copy()
    exp[:len(involved)] = S.mailbox_consume_gather(st0, involved)
    np.testing.assert_array_equal(bits(out), bits(exp), err_msg=f'{tag}: consume_gather')
    assert_state(ds, st0, st0, f'{tag}: consume_gather leaves the state alone')

    # STEP 4, rank form and row-index form
    reprs = payload((len(involved), d), rs, plain=plain)
    for form in ('rank', 'rows'):
        ds, ref = DevState(st0), st0.copy()
        if form == 'rank':
            word = call_consume(ds, upos_t, len(upos), reprs, involved=involved)
            exp_word = S.consume_update_right(ref, upos, reprs, involved=involved)
        else:
            ri = rs.permutation(len(involved))[:len(upos_t)] if len(involved) >= len(upos_t) else \
                rs.randint(0, len(involved), len(upos_t))
            word = call_consume(ds, upos_t, len(upos), reprs, row_index=ri.astype(np.int64))
            exp_word = S.consume_update_right(ref, upos, reprs, row_index=ri[:len(upos)])
        assert word == exp_word == 0, (tag, form, word, exp_word)
        assert_state(ds, ref, st0, f'{tag}: consume_update_right[{form}]')
    after4 = ref

    # STEP 5 behind STEP 4 (clean), and on the initial state (pending positive nodes: unused messages)
    for name, start in (('after STEP 4', after4), ('unconsumed', st0)):
        ds, ref = DevState(start), start.copy()
        word = call_store_events(ds, batch, upos_t, index_t, len(upos))
        exp_word = S.store_events(ref, batch['src'], batch['dst'], batch['ts32'], batch['eids'], upos, index)
        assert word == exp_word, (tag, name, word, exp_word)
        assert exp_word == (S.ERR_UNUSED_MESSAGE if start.has_msg[upos].any() else 0)
        assert_state(ds, ref, start, f'{tag}: store_events {name}')

    # effective rows; serve into unaligned rows of d + 1 floats at permuted positions with gaps; adopt elsewhere
    ids = rs.permutation(n)[:min(n, 37)].astype(np.int64)
    assert st0.has_msg[ids].any() and not st0.has_msg[ids].all()
    ds = DevState(st0)
    o_rows, o_ts = call_gather_eff(ds, ids, payload((len(ids), d), rs), payload(len(ids), rs))
    e_rows, e_ts = S.gather_eff_rows(st0, ids)
    np.testing.assert_array_equal(bits(o_rows), bits(e_rows), err_msg=f'{tag}: gather_eff_rows')
    np.testing.assert_array_equal(bits(o_ts), bits(e_ts), err_msg=f'{tag}: gather_eff_rows times')
    n_eff = len(ids) * 2 // 3
    eff, msg = ids[:n_eff], ids[n_eff // 2:]          # some nodes in both lists
    slots = rs.permutation(2 * len(ids) + 5).astype(np.int64)
    eff_pos, msg_pos = slots[:len(eff)], slots[len(eff):len(eff) + len(msg)]
    buf0 = payload((2 * len(ids) + 5, d + 1), rs)
    served = call_serve(ds, eff, eff_pos, msg, msg_pos, buf0)
    exp = buf0.copy()
    S.serve_rows(st0, eff, eff_pos, msg, msg_pos, exp)
    np.testing.assert_array_equal(bits(served), bits(exp), err_msg=f'{tag}: serve_rows')
    assert_state(ds, st0, st0, f'{tag}: serve_rows leaves the state alone')
    st1 = make_state(n, d, st0.d_e, st0.msg_src, st0.nfeats is not None, st0.efeats is not None, seed=seed + 77)
    # (adopt takes disjoint lists: a node in both would be written twice in the message-source = right memory)
    msg_only = np.isin(msg, eff, invert=True)
    ds1, ref1 = DevState(st1), st1.copy()
    call_adopt(ds1, eff, eff_pos, msg[msg_only], msg_pos[msg_only], served)
    S.adopt_rows(ref1, eff, eff_pos, msg[msg_only], msg_pos[msg_only], exp)
    assert_state(ds1, ref1, st1, f'{tag}: adopt_rows')
    got1 = ds1.tables()   # the round trip, spelled out: the named rows and times arrive bit for bit
    np.testing.assert_array_equal(bits(got1['right_vals'][eff]), bits(e_rows[:n_eff]))
    np.testing.assert_array_equal(bits(got1['right_ts'][eff]), bits(e_ts[:n_eff]))
    mo = msg[msg_only]
    src_rows = (st0.left_vals[mo], st0.left_ts[mo]) if st0.msg_src == 'left' else S.gather_eff_rows(st0, mo)
    which = 'left' if st0.msg_src == 'left' else 'right'
    np.testing.assert_array_equal(bits(got1[which + '_vals'][mo]), bits(src_rows[0]))
    np.testing.assert_array_equal(bits(got1[which + '_ts'][mo]), bits(src_rows[1]))

    # restart
    nids = rs.permutation(n)[:min(n, 21)].astype(np.int64)
    hl, hr, pt = payload((len(nids), d), rs), payload((len(nids), d), rs), payload(len(nids), rs)
    ds, ref = DevState(st0), st0.copy()
    call_restart(ds, nids, hl, hr, pt)
    S.restart_apply(ref, nids, hl, hr, pt)
    assert_state(ds, ref, st0, f'{tag}: restart_apply')

    # STEP 4-6 as one call: in-call dedup and planned winners (a live count below the lists), rows given / from pending
    rows, new_row, left_row = gathered_rows(st0, batch, rs, plain)
    for form in ('dedup', 'planned', 'planned-pending', 'dedup-pending'):
        ds, ref = DevState(st0), st0.copy()
        pend = form.endswith('pending')
        if form.startswith('planned'):
            word = call_writeback(ds, batch, rows, None if pend else new_row, left_row, new_from_pending=pend,
                                  planned=(upos_t, index_t, len(upos)))
        else:
            word = call_writeback(ds, batch, rows, None if pend else new_row, left_row, new_from_pending=pend)
        exp_word = S.writeback(ref, batch, rows, new_row, left_row, new_from_pending=pend)
        assert word == exp_word == 0, (tag, form, word, exp_word)
        assert_state(ds, ref, st0, f'{tag}: stream_writeback[{form}]')


@pytest.mark.parametrize('msg_src', ['left', 'right'])
@pytest.mark.parametrize('with_ef', [False, True], ids=['noef', 'ef'])
@pytest.mark.parametrize('with_nf', [False, True], ids=['nonf', 'nf'])
@pytest.mark.parametrize('d,d_e', WIDTHS)
def test_entry_points_at_row_widths(d, d_e, with_nf, with_ef, msg_src):
    st0 = make_state(129, d, d_e, msg_src, with_nf, with_ef, seed=d + d_e)
    run_entry_points(st0, make_batch('hub_inc', seed=3), d * 7 + d_e, f'd={d} d_e={d_e} {msg_src}')


@pytest.mark.parametrize('msg_src', ['left', 'right'])
@pytest.mark.parametrize('kind', ['one', 'loop', 'three', 'hub_inc', 'hub_eq', 'hub_collapse'])
def test_entry_points_on_batch_shapes(kind, msg_src):
    st0 = make_state(129, 8, 20, msg_src, True, True, seed=11)
    batch = make_batch(kind, seed=5)
    if kind == 'hub_collapse':
        assert len(np.unique(batch['ts'])) == 40 and len(np.unique(batch['ts32'])) < 12
    run_entry_points(st0, batch, 23, f'{kind} {msg_src}')


def test_dedup_ties_go_to_the_first_position():
    """what the in-call dedup of tg_stream_writeback must have picked shows in the state: the hub's mailbox row names
    the first event among equal float32 times (edge features and the other endpoint's row), its left row is h(t-) of
    that position"""
    for kind in ('hub_eq', 'hub_collapse'):
        batch = make_batch(kind, seed=5)
        upos, index = S.winners(batch['src'], batch['dst'], batch['ts32'])
        first = int(index[upos == 64][0])
        assert first == (0 if kind == 'hub_eq' else 38) and batch['src'][first] == 64
        if kind == 'hub_collapse':   # ... while in float64 the LAST event, with the hub as its destination, is the latest
            assert np.argmax(batch['ts']) == 39 and batch['dst'][39] == 64 and batch['ts32'][38] == batch['ts32'][39]
        st0 = make_state(129, 8, 8, 'left', False, True, seed=2)
        rs = np.random.RandomState(1)
        rows, new_row, left_row = gathered_rows(st0, batch, rs, False)
        ds, ref = DevState(st0), st0.copy()
        assert call_writeback(ds, batch, rows, new_row, left_row) == S.writeback(ref, batch, rows, new_row, left_row) == 0
        assert_state(ds, ref, st0, f'ties {kind}')
        got = ds.tables()
        np.testing.assert_array_equal(bits(got['left_vals'][64]), bits(rows[left_row[first]]))
        np.testing.assert_array_equal(bits(got['msg_vals'][64, 16:24]), bits(st0.efeats[batch['eids'][first]]))


@pytest.mark.parametrize('msg_src', ['left', 'right'])
def test_past_the_wavefront_cap(msg_src):
    """2B = 16 384 + 6 distinct positive nodes: more winners than wavefronts in the capped grid of the one-wavefront-
    per-node kernels; 4-float rows keep it quick"""
    batch = make_batch('cap', seed=8)
    B = len(batch['src'])
    n = 2 * B + 70
    st0 = make_state(n, 4, 4, msg_src, False, True, n_edges=B, seed=4)
    rs = np.random.RandomState(6)
    pos = np.concatenate([batch['src'], batch['dst']])
    upos, index = S.winners(batch['src'], batch['dst'], batch['ts32'])
    assert len(upos) == 2 * B == _cap_ref.CAP_WAVE + 6
    perm = rs.permutation(len(upos))
    upos, index = upos[perm], index[perm]
    reprs = payload((len(upos), 4), rs)
    ds, ref = DevState(st0), st0.copy()
    assert call_consume(ds, upos, len(upos), reprs, involved=pos) == S.consume_update_right(ref, upos, reprs, involved=pos) == 0
    assert_state(ds, ref, st0, 'cap: consume_update_right')
    after4 = ref
    ds, ref = DevState(after4), after4.copy()
    word = call_store_events(ds, batch, upos, index, len(upos))
    assert word == S.store_events(ref, batch['src'], batch['dst'], batch['ts32'], batch['eids'], upos, index) == 0
    assert_state(ds, ref, after4, 'cap: store_events')
    rows, new_row, left_row = gathered_rows(st0, batch, rs, False)
    for planned in (False, True):
        ds, ref = DevState(st0), st0.copy()
        word = call_writeback(ds, batch, rows, new_row, left_row, planned=(upos, index, len(upos)) if planned else None)
        assert word == S.writeback(ref, batch, rows, new_row, left_row) == 0
        assert_state(ds, ref, st0, f'cap: stream_writeback planned={planned}')


@pytest.mark.parametrize('msg_src', ['left', 'right'])
def test_all_64_nodes_of_a_bitmap_word(msg_src):
    """nodes 64..127 - one has-message word - are all positive nodes of one batch, half of them pending before it, the
    batch spread over 32 workgroups: consuming clears bits and storing sets bits of the same word from many wavefronts.
    Repeated from fresh state a few times within the call: a lost update is a race, not a certainty."""
    n, B = 200, 64
    rs = np.random.RandomState(12)
    pending = np.zeros(n, bool)
    pending[64:128:2] = True
    pending[130:190:3] = True
    st0 = make_state(n, 4, 4, msg_src, False, False, seed=9, pending=pending)
    for rep in range(6):
        src = rs.permutation(np.arange(64, 128)).astype(np.int64)
        dst = rs.permutation(np.arange(128, 192)).astype(np.int64)
        ts = np.floor(rs.uniform(T_STATE + 1, T_EVENT, B))
        batch = dict(src=src, dst=dst, ts=ts, ts32=ts.astype(np.float32), eids=np.arange(1, B + 1, dtype=np.int64))
        rows, new_row, left_row = gathered_rows(st0, batch, rs, False)
        ds, ref = DevState(st0), st0.copy()
        assert call_writeback(ds, batch, rows, new_row, left_row) == S.writeback(ref, batch, rows, new_row, left_row) == 0
        assert ref.has_msg[64:192].all()
        words = ds.has_msg_words()
        exp_words = np.packbits(np.concatenate([ref.has_msg, np.zeros(56, bool)]), bitorder='little').view(np.uint64)
        np.testing.assert_array_equal(words, exp_words, err_msg=f'has-message words, repeat {rep}')
        assert_state(ds, ref, st0, f'word of 64, repeat {rep}')
        # the two kernels apart: consume clears exactly the pending half, store sets all
        upos, index = S.winners(src, dst, batch['ts32'])
        ds, ref = DevState(st0), st0.copy()
        reprs = payload((len(upos), 4), rs)
        assert call_consume(ds, upos, len(upos), reprs, involved=upos) == 0
        S.consume_update_right(ref, upos, reprs, involved=upos)
        assert not ref.has_msg[64:128].any()
        assert_state(ds, ref, st0, f'word of 64, consume, repeat {rep}')
        mid = ref
        ds, ref = DevState(mid), mid.copy()
        assert call_store_events(ds, batch, upos, index, len(upos)) == 0
        S.store_events(ref, src, dst, batch['ts32'], batch['eids'], upos, index)
        assert_state(ds, ref, mid, f'word of 64, store, repeat {rep}')


# ---- tg_stream_writeback: resident stream, owners ----------------------------------------------------------------------
@pytest.mark.parametrize('new_from_pending', [False, True], ids=['rows', 'pending'])
@pytest.mark.parametrize('msg_src', ['left', 'right'])
def test_writeback_over_a_resident_stream(msg_src, new_from_pending):
    """three batches of a resident stream through the device offset: the row maps are read at 2 * offset, the offset
    advances by B per call"""
    B, n = 12, 129
    rs = np.random.RandomState(31)
    src, dst = rs.randint(0, 40, 3 * B).astype(np.int64), rs.randint(30, n, 3 * B).astype(np.int64)
    src[::5] = 64
    ts = T_STATE + 1 + np.floor(np.sort(rs.uniform(0, 900, 3 * B)) / 4) * 4     # ties
    stream = dict(src=src, dst=dst, ts=ts, eids=rs.permutation(3 * B).astype(np.int64) + 1)
    st0 = make_state(n, 8, 20, msg_src, True, True, seed=3)
    rows = payload((12 * B + 5, 8), rs, plain=True)
    p = rs.permutation(12 * B + 5).astype(np.int64)
    new_row, left_row = p[:6 * B], p[6 * B:12 * B]
    ds, ref = DevState(st0), st0.copy()
    offset = torch.zeros(1, dtype=torch.int64, device=dev())
    for b in range(3):
        sl, sl2 = slice(b * B, (b + 1) * B), slice(2 * b * B, 2 * (b + 1) * B)
        batch = dict(src=src[sl], dst=dst[sl], ts32=ts[sl].astype(np.float32), eids=stream['eids'][sl])
        word = call_writeback(ds, batch, rows, None if new_from_pending else new_row, left_row, offset=offset, advance=1,
                              stream=stream, new_from_pending=new_from_pending)
        exp_word = S.writeback(ref, batch, rows, new_row[sl2], left_row[sl2], new_from_pending=new_from_pending)
        assert word == exp_word == 0, (b, word, exp_word)
        # (named: every node written so far - the device keeps its own cosines of the earlier batches)
        assert_state(ds, ref, st0, f'resident batch {b}', named=np.concatenate([src[:(b + 1) * B], dst[:(b + 1) * B]]))
        assert int(offset.item()) == (b + 1) * B
    # advance = 0 leaves the offset
    ds2 = DevState(st0)
    off2 = torch.full((1,), B, dtype=torch.int64, device=dev())
    call_writeback(ds2, batch, rows, new_row, left_row, offset=off2, advance=0, stream=stream)
    assert int(off2.item()) == B


@pytest.mark.parametrize('form', ['dedup', 'planned'])
@pytest.mark.parametrize('new_from_pending', [False, True], ids=['rows', 'pending'])
@pytest.mark.parametrize('msg_src', ['left', 'right'])
def test_writeback_owner_filter(msg_src, new_from_pending, form):
    """three ranks; rank 2 owns no positive node of the batch: nothing changes for it, the word stays 0 - also when a
    node of ANOTHER rank violates an invariant"""
    n = 129
    batch = make_batch('hub_inc', seed=3)
    pos = np.unique(np.concatenate([batch['src'], batch['dst']]))
    owner = np.full(n, 2, np.int32)
    owner[pos] = np.arange(len(pos)) % 2
    owner[64] = 1
    st0 = make_state(n, 8, 20, msg_src, True, True, seed=13)
    rs = np.random.RandomState(2)
    rows, new_row, left_row = gathered_rows(st0, batch, rs, True)
    upos, index = S.winners(batch['src'], batch['dst'], batch['ts32'])
    bad = st0.copy()                    # rank 1's hub: left time and message-source time after its events
    bad.left_ts[64] = bad.right_ts[64] = bad.msg_ts[64] = up(batch['ts32'].max())
    for state, label in ((st0, 'clean'), (bad, 'violation on rank 1')):
        for rank in range(3):
            ds, ref = DevState(state), state.copy()
            mine = owner[upos] == rank
            planned = (upos[mine], index[mine], int(mine.sum())) if form == 'planned' else None
            word = call_writeback(ds, batch, rows, None if new_from_pending else new_row, left_row, owner=owner,
                                  my_rank=rank, new_from_pending=new_from_pending, planned=planned)
            exp_word = S.writeback(ref, batch, rows, new_row, left_row, owner=owner, my_rank=rank,
                                   new_from_pending=new_from_pending)
            assert word == exp_word, (label, rank, word, exp_word)
            assert (word != 0) == (label != 'clean' and rank == 1), (label, rank, word)
            assert_state(ds, ref, state, f'owner {label} rank {rank}')
            if rank == 2:
                assert_state(ds, state, state, f'owner {label}: rank 2 owns nothing')


# ---- the invariant word: equal times, one float32 step on the wrong side, clean -------------------------------------------
# (entry point, check it can raise).  tg_store_events also raises UNUSED_MESSAGE: the test below.  The gathers, serve,
# adopt and restart check nothing.
INV_CASES = [('store_events', 'event_before_mem_winner'), ('store_events', 'event_before_mem_loser'),
             ('consume', 'right_after_message'), ('consume_rows', 'right_after_message')] + \
    [(e, c) for e in ('writeback', 'writeback_planned')
     for c in ('event_before_mem_winner', 'event_before_mem_loser', 'right_after_message', 'left_after_event')]


@pytest.mark.parametrize('entry,case', INV_CASES)
@pytest.mark.parametrize('msg_src', ['left', 'right'])
def test_invariant_bits(msg_src, entry, case):
    """per entry point and check: the two times equal -> 0; one float32 step on the wrong side -> exactly the bits of
    that time's checks; clean -> 0.  Always the whole word, against the reference's."""
    batch = make_batch('hub_inc', seed=3)
    src, dst, ts32 = batch['src'], batch['dst'], batch['ts32']
    pos = np.concatenate([src, dst])
    upos, index = S.winners(src, dst, ts32)
    rs = np.random.RandomState(4)
    base = make_state(129, 8, 8, msg_src, False, False, seed=21)
    if entry == 'store_events':
        set_pending(base, upos, False)            # alone, without STEP 4 before it: no unused messages
    elif entry.startswith('consume'):
        set_pending(base, upos, True)
    rows, new_row, left_row = gathered_rows(base, batch, rs, False)
    reprs = payload((len(upos), 8), rs)
    mem_ts = 'left_ts' if msg_src == 'left' else 'right_ts'
    v = 128                                       # an ordinary node: one position, which wins
    assert (pos == v).sum() == 1 and (pos == 64).sum() == 41
    tv = np.tile(ts32, 2)[pos == v][0]
    hub_first, hub_last = ts32[0], ts32[-1]       # the hub is in every event; times increase
    wb = entry.startswith('writeback')
    if case == 'event_before_mem_winner':
        # STEP 5 reads the message-source time of every position.  msg_src = right: behind STEP 4, so the node has no
        # pending message; msg_src = left: the same time is the one STEP 6 checks
        field, node, edge, bit = mem_ts, v, tv, S.ERR_EVENT_BEFORE_MEM
        if msg_src == 'right':
            set_pending(base, [v], False)
        elif wb:
            bit |= S.ERR_PAST_MEMORY
    elif case == 'event_before_mem_loser':
        # after the hub's FIRST event only - a position of the batch that is no winner; fine for the winning one
        field, node, edge, bit = mem_ts, 64, hub_first, S.ERR_EVENT_BEFORE_MEM
        assert up(hub_first) < ts32[1] and index[upos == 64][0] != 0
        if msg_src == 'right':
            set_pending(base, [64], False)
    elif case == 'right_after_message':           # STEP 4
        set_pending(base, [v], True)
        field, node, edge, bit = 'right_ts', v, base.msg_ts[v], S.ERR_PAST_MEMORY
    else:                                         # STEP 6
        field, node, edge, bit = 'left_ts', v, tv, S.ERR_PAST_MEMORY
        if msg_src == 'left':
            bit |= S.ERR_EVENT_BEFORE_MEM
    seen = {}
    for name in ('clean', 'equal', 'wrong'):
        st = base.copy()
        if name != 'clean':
            getattr(st, field)[node] = edge if name == 'equal' else up(edge)
            if field == 'left_ts' and msg_src == 'left' and st.has_msg[node]:
                st.msg_ts[node] = st.left_ts[node]    # (keeps the message's own invariant)
        ds, ref = DevState(st), st.copy()
        if entry == 'store_events':
            word = call_store_events(ds, batch, upos, index, len(upos))
            exp = S.store_events(ref, src, dst, ts32, batch['eids'], upos, index)
        elif entry == 'consume':
            word = call_consume(ds, upos, len(upos), reprs, involved=upos)
            exp = S.consume_update_right(ref, upos, reprs, involved=upos)
        elif entry == 'consume_rows':
            ri = rs.permutation(len(upos)).astype(np.int64)
            word = call_consume(ds, upos, len(upos), reprs, row_index=ri)
            exp = S.consume_update_right(ref, upos, reprs, row_index=ri)
        else:
            planned = (upos, index, len(upos)) if entry == 'writeback_planned' else None
            word = call_writeback(ds, batch, rows, new_row, left_row, planned=planned)
            exp = S.writeback(ref, batch, rows, new_row, left_row)
        assert word == exp, (name, word, exp)
        assert_state(ds, ref, st, f'{entry} {case} {name}')   # the writes happen all the same
        seen[name] = word
    assert seen == {'clean': 0, 'equal': 0, 'wrong': bit}, (seen, bit)


@pytest.mark.parametrize('msg_src', ['left', 'right'])
def test_unused_message_without_a_preceding_consume(msg_src):
    batch = make_batch('three', seed=1)
    upos, index = S.winners(batch['src'], batch['dst'], batch['ts32'])
    base = make_state(129, 8, 8, msg_src, False, False, seed=5)
    base.has_msg[upos] = False
    for node, expect in ((None, 0), (128, S.ERR_UNUSED_MESSAGE), (1, 0)):   # node 1 is pending but not in the batch
        st = base.copy()
        if node is not None:
            st.has_msg[node] = True
        ds, ref = DevState(st), st.copy()
        word = call_store_events(ds, batch, upos, index, len(upos))
        assert word == S.store_events(ref, batch['src'], batch['dst'], batch['ts32'], batch['eids'], upos, index) == expect
        assert_state(ds, ref, st, f'unused message {node}')


def test_planned_writeback_with_empty_lists():
    batch = make_batch('three', seed=1)
    st0 = make_state(129, 8, 8, 'left', False, False, seed=5)
    rs = np.random.RandomState(0)
    rows, new_row, left_row = gathered_rows(st0, batch, rs, False)
    empty = np.zeros(0, np.int64)
    ds = DevState(st0)
    assert call_writeback(ds, batch, rows, new_row, left_row, planned=(empty, empty, 0)) == 0      # NULL lists
    assert_state(ds, st0, st0, 'empty planned lists')
    upos, index = S.winners(batch['src'], batch['dst'], batch['ts32'])
    ds = DevState(st0)
    assert call_writeback(ds, batch, rows, new_row, left_row, planned=(upos, index, 0)) == 0       # lists, live count 0
    assert_state(ds, st0, st0, 'planned lists with a live count of 0')


def test_report_measured_time_segment_error():
    """(last in the module) the figure the docstring quotes"""
    print(f'time segment: max abs err over the module {MEASURED["te"]:.3e}, bound {TE_BOUND:.0e}')
    assert MEASURED['te'] <= TE_BOUND
