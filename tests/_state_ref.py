"""A NumPy state machine for the node state of the streaming step: left and right memory, their times, the mailbox,
the has-message set and the table of pending updater rows - written from the semantics of tiger.py:229-255,396-442,
594-609 / memory.py:41-52,77-138 and the contracts in include/tiger_hip.h, not from the kernels.

Every mutating function works on a `State` in place and returns the invariant word it must raise: all violated
checks OR-ed (the reference raises at the first one; the device reports all of them).  Comparisons are strict `>`:
equal times raise nothing.  Everything is a copy, plus one float32 add where node features join a memory row - exact
in NumPy - except the time segment of a mailbox row: cos in float64 of the float32 argument fl32(fl32(dt * w) + phi),
rounded to float32 (time_encoding.py:24-26).

tests/test_state_ref_host.py checks this module against the oracle; tests/test_hip_state_kernels.py and
tests/test_hip_step_invariants.py compare the HIP kernels with it."""
import numpy as np

F32 = np.float32
ERR_PAST_MEMORY, ERR_DUPLICATE_IDS, ERR_UNUSED_MESSAGE = 1, 2, 4            # include/tiger_hip.h: TG_ERR_*
ERR_MSG_BEFORE_MEM, ERR_MSG_TS_MISMATCH, ERR_EVENT_BEFORE_MEM = 8, 16, 32

_TABLES = ('left_vals', 'left_ts', 'left_active', 'right_vals', 'right_ts', 'right_active', 'msg_vals', 'msg_ts',
           'has_msg', 'pending_vals')


class State:
    """Tables of n_nodes rows.  nfeats [n_nodes, d] / efeats [n_edges + 1, d_e] may be None (zeros); d_e is the width of
    the mailbox's edge segment either way.  msg_src: 'left' or 'right', the memory a raw message is built from."""

    def __init__(self, n_nodes, d, d_e, msg_src, te_freq, te_phase, nfeats=None, efeats=None):
        assert msg_src in ('left', 'right')
        self.n_nodes, self.d, self.d_e, self.msg_src = n_nodes, d, d_e, msg_src
        self.left_vals = np.zeros((n_nodes, d), F32)
        self.left_ts = np.zeros(n_nodes, F32)
        self.left_active = np.zeros(n_nodes, np.uint8)
        self.right_vals = np.zeros((n_nodes, d), F32)
        self.right_ts = np.zeros(n_nodes, F32)
        self.right_active = np.zeros(n_nodes, np.uint8)
        self.msg_vals = np.zeros((n_nodes, 3 * d + d_e), F32)
        self.msg_ts = np.zeros(n_nodes, F32)
        self.has_msg = np.zeros(n_nodes, bool)
        self.pending_vals = np.zeros((n_nodes, d), F32)
        self.nfeats = None if nfeats is None else np.asarray(nfeats, F32)
        self.efeats = None if efeats is None else np.asarray(efeats, F32)
        self.te_freq, self.te_phase = np.asarray(te_freq, F32), np.asarray(te_phase, F32)
        self.max_te_arg = 0.0   # largest |argument| any time segment was evaluated at

    def copy(self):
        s = State.__new__(State)
        s.__dict__.update(self.__dict__)
        for k in _TABLES:
            setattr(s, k, getattr(self, k).copy())
        return s

    def tables(self):
        return {k: getattr(self, k) for k in _TABLES}

    def mem(self, which=None):
        """(values, times) of the message-source memory, or of the named one"""
        which = which or self.msg_src
        return (self.left_vals, self.left_ts) if which == 'left' else (self.right_vals, self.right_ts)


def time_segment(state, dt):
    """TimeEncode of float32 time differences dt [n] -> float32 [n, d]: cos evaluated in float64 at the float32
    argument fl32(fl32(dt * w) + phi)"""
    dt = np.asarray(dt, F32)
    arg = (dt[:, None] * state.te_freq[None, :]).astype(F32) + state.te_phase[None, :]
    assert arg.dtype == F32
    if arg.size:
        state.max_te_arg = max(state.max_te_arg, float(np.abs(arg).max()))
    return np.cos(arg.astype(np.float64)).astype(F32)


def winners(src, dst, ts32):
    """select_latest_nids (utils.py:10-16) on cat[src, dst] with the float32 event times tiled twice: per unique node the
    position with the largest time, the FIRST such position among ties.  -> (nodes sorted, positions)"""
    pos = np.concatenate([np.asarray(src, np.int64), np.asarray(dst, np.int64)])
    ts2 = np.tile(np.asarray(ts32, F32), 2)
    nodes = np.unique(pos)
    index = np.empty(len(nodes), np.int64)
    for j, v in enumerate(nodes):
        where = np.nonzero(pos == v)[0]
        index[j] = where[np.argmax(ts2[where])]   # argmax: the first of equal maxima
    return nodes, index


def sort_by_node(upos, index):
    """a winner list in any order -> sorted by node (the result of a dedup is order-free)"""
    upos, index = np.asarray(upos, np.int64), np.asarray(index, np.int64)
    o = np.argsort(upos, kind='stable')
    return upos[o], index[o]


def _feat(table, ids, width):
    return np.zeros((len(ids), width), F32) if table is None else table[ids]


def mailbox_consume_gather(state, involved):
    """STEP 2's copy (tiger.py:214): the right-memory rows of the involved nodes"""
    return state.right_vals[np.asarray(involved, np.int64)].copy()


def gather_eff_rows(state, ids):
    """effective right memory: the row and time STEP 4 would leave if the node's pending message were consumed now
    -> (rows [n, d], times [n])"""
    ids = np.asarray(ids, np.int64)
    p = state.has_msg[ids]
    return (np.where(p[:, None], state.pending_vals[ids], state.right_vals[ids]),
            np.where(p, state.msg_ts[ids], state.right_ts[ids]))


def serve_rows(state, eff_ids, eff_pos, msg_ids, msg_pos, out):
    """out [*, d + 1] in place: row eff_pos[i] = effective right row of eff_ids[i] and its time; row msg_pos[j] = the
    message-source memory row of msg_ids[j] (left memory, or the effective right row) and its time"""
    d = state.d
    rows, ts = gather_eff_rows(state, eff_ids)
    out[np.asarray(eff_pos, np.int64), :d], out[np.asarray(eff_pos, np.int64), d] = rows, ts
    msg_ids = np.asarray(msg_ids, np.int64)
    if state.msg_src == 'left':
        rows, ts = state.left_vals[msg_ids], state.left_ts[msg_ids]
    else:
        rows, ts = gather_eff_rows(state, msg_ids)
    out[np.asarray(msg_pos, np.int64), :d], out[np.asarray(msg_pos, np.int64), d] = rows, ts


def adopt_rows(state, eff_ids, eff_pos, msg_ids, msg_pos, rows):
    """the inverse on the receiving side: rows[eff_pos[i]] overwrites the right memory row / time of eff_ids[i],
    rows[msg_pos[j]] the message-source memory row / time of msg_ids[j]"""
    d = state.d
    eff_ids, msg_ids = np.asarray(eff_ids, np.int64), np.asarray(msg_ids, np.int64)
    state.right_vals[eff_ids] = rows[np.asarray(eff_pos, np.int64), :d]
    state.right_ts[eff_ids] = rows[np.asarray(eff_pos, np.int64), d]
    vals, tss = state.mem()
    vals[msg_ids] = rows[np.asarray(msg_pos, np.int64), :d]
    tss[msg_ids] = rows[np.asarray(msg_pos, np.int64), d]


def consume_update_right(state, upos, rows, row_index=None, involved=None):
    """STEP 4 (tiger.py:230-241, memory.py:41-52,128-138): every node of upos with a pending message gets its new right
    memory row, the message's time and loses the message.  Row of node upos[p]: rows[row_index[p]], or - the rank form -
    rows[number of involved nodes with a smaller id] (the node's local index in the sorted involved set)."""
    upos = np.asarray(upos, np.int64)
    if row_index is None:
        row_index = np.searchsorted(np.unique(np.asarray(involved, np.int64)), upos)
    row_index = np.asarray(row_index, np.int64)
    word = 0
    for p, v in enumerate(upos):
        if not state.has_msg[v]:
            continue
        if state.right_ts[v] > state.msg_ts[v]:
            word |= ERR_PAST_MEMORY
        state.right_vals[v] = rows[row_index[p]]
        state.right_ts[v] = state.msg_ts[v]
        state.right_active[v] = 1
        state.has_msg[v] = False
    return word


def store_events(state, src, dst, ts32, eids, upos=None, index=None, owner=None, my_rank=0):
    """STEP 5 (tiger.py:422-442, memory.py:77-106): the raw message [own | other | edge | time] of the winning event of
    every unique positive node.  upos / index: the winners to write (default: all of them); owner: only nodes of
    my_rank are checked and written."""
    src, dst, eids = (np.asarray(a, np.int64) for a in (src, dst, eids))
    ts32 = np.asarray(ts32, F32)
    B = len(src)
    pos, ts2 = np.concatenate([src, dst]), np.tile(ts32, 2)
    vals, tss = state.mem()
    mine = np.ones(2 * B, bool) if owner is None else (np.asarray(owner)[pos] == my_rank)
    word = ERR_EVENT_BEFORE_MEM if (tss[pos][mine] > ts2[mine]).any() else 0
    if upos is None:
        upos, index = winners(src, dst, ts32)
    upos, index = np.asarray(upos, np.int64), np.asarray(index, np.int64)
    if owner is not None:
        keep = np.asarray(owner)[upos] == my_rank
        upos, index = upos[keep], index[keep]
    if not len(upos):
        return word
    e = index % B
    other = np.where(index < B, dst[e], src[e])
    assert (pos[index] == upos).all()
    # no node-feature table: the rows are copied, not added to zeros (the two differ in one bit pattern: -0 + 0 = +0)
    own_row = vals[upos] if state.nfeats is None else vals[upos] + state.nfeats[upos]
    other_row = vals[other] if state.nfeats is None else vals[other] + state.nfeats[other]
    t = ts32[e]
    row = np.concatenate([own_row, other_row, _feat(state.efeats, eids[e], state.d_e),
                          time_segment(state, t - tss[upos])], 1)
    if state.has_msg[upos].any():
        word |= ERR_UNUSED_MESSAGE
    state.msg_vals[upos] = row
    state.msg_ts[upos] = t
    state.has_msg[upos] = True
    return word


def update_left(state, upos, index, ts32, rows, left_row):
    """STEP 6 (tiger.py:253-255): left memory <- h(t-) of the winning position, time <- the event's"""
    ts2 = np.tile(np.asarray(ts32, F32), 2)
    upos, index = np.asarray(upos, np.int64), np.asarray(index, np.int64)
    word = ERR_PAST_MEMORY if (state.left_ts[upos] > ts2[index]).any() else 0
    state.left_vals[upos] = rows[np.asarray(left_row, np.int64)[index]]
    state.left_ts[upos] = ts2[index]
    state.left_active[upos] = 1
    return word


def restart_apply(state, nids, h_left, h_right, prev_ts):
    """TIGER.restart's state update (tiger.py:603,608-609): both memories and times, no check; messages dropped"""
    nids = np.asarray(nids, np.int64)
    state.left_vals[nids], state.right_vals[nids] = h_left, h_right
    state.left_ts[nids] = state.right_ts[nids] = np.asarray(prev_ts, F32)
    state.left_active[nids] = state.right_active[nids] = 1
    state.has_msg[nids] = False
    return 0


def writeback(state, batch, rows, new_row, left_row, owner=None, my_rank=0, new_from_pending=False, upos=None,
              index=None):
    """STEP 4, 5, 6 of one batch in reference order.  batch: dict(src, dst, ts32, eids).  Position i of cat[src, dst]
    reads h(t'+) at rows[new_row[i]] (or, new_from_pending, at pending_vals[node]) and h(t-) at rows[left_row[i]].
    upos / index: planned winners (default: the dedup of the batch); owner: only my_rank's nodes are touched."""
    src, dst, ts32, eids = batch['src'], batch['dst'], np.asarray(batch['ts32'], F32), batch['eids']
    if upos is None:
        upos, index = winners(src, dst, ts32)
    upos, index = np.asarray(upos, np.int64), np.asarray(index, np.int64)
    if owner is not None:
        keep = np.asarray(owner)[upos] == my_rank
        upos, index = upos[keep], index[keep]
    if new_from_pending:
        word = consume_update_right(state, upos, state.pending_vals, row_index=upos)
    else:
        word = consume_update_right(state, upos, rows, row_index=np.asarray(new_row, np.int64)[index])
    word |= store_events(state, src, dst, ts32, eids, upos, index, owner, my_rank)
    word |= update_left(state, upos, index, ts32, rows, left_row)
    return word


def step_invariants(state, batch, involved):
    """the message / memory time checks of STEP 1 (message_modules.py:158-159, tiger.py:325-327) over the involved
    nodes with a pending message"""
    ids = np.unique(np.asarray(involved, np.int64))
    ids = ids[state.has_msg[ids]]
    mem_ts, mts = state.mem()[1][ids], state.msg_ts[ids]
    word = ERR_MSG_BEFORE_MEM if (mem_ts > mts).any() else 0
    if state.msg_src == 'left' and not (mts == mem_ts).all():
        word |= ERR_MSG_TS_MISMATCH
    return word
