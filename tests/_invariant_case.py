"""The invariant word of whole streaming steps, in a process of its own (the library reads its knobs once per process):
  python _invariant_case.py MSG_SRC eager|lazy
Run by tests/test_hip_step_invariants.py with one knob setting in the environment.

Two clean steps, each compared table by table with the NumPy state machine (tests/_state_ref.py: STEP 4-6 from the
state before the step and the embeddings the step produced).  Then, for the next batch, a series of corrupted TIMES -
never ids, counts or row maps - each on a copy of the state: one step, the whole word against
step_invariants + writeback of the reference on the same corrupted state, the reference's ValueError, and after the
restore a clean step with word 0.  Prints one JSON line (forms, words) and `INVARIANT-CASE OK`."""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import bench  # noqa: E402
import _state_ref as S  # noqa: E402
from oracle import tiger_oracle as O  # noqa: E402
from www2023tiger_amd import _lib  # noqa: E402

# the shapes at which tests/_fc2_defer_case.py gets the four-launch form, on a stream with enough nodes that a batch
# leaves some of them out: those turn up as neighbours only
D, B, K = 172, 1024, 10
N_U, N_I = 600, 150
TE_BOUND, TE_ARG_MAX = 5e-7, 3.0e6   # test_hip_parity.test_time_encode_rounding


def up(x):
    return np.nextafter(np.float32(x), np.float32(np.inf))


def down(x):
    return np.nextafter(np.float32(x), np.float32(-np.inf))


def state_tensors(model):
    L, R, M = model.left_memory, model.right_memory, model.msg_store
    t = dict(left_vals=L.vals, left_ts=L.update_ts, right_vals=R.vals, right_ts=R.update_ts, msg_vals=M.node_msg_vals,
             msg_ts=M.node_msg_ts, has_msg=M.has_msg_bits)
    if model._pending is not None:
        t['pending_vals'] = model._pending
    return t


def pull(model, stream, msg_src):
    """device state -> reference State"""
    n = stream['n_nodes']
    st = S.State(n, D, D, msg_src, model.time_encoder.basis_freq.detach().cpu().numpy().reshape(-1),
                 model.time_encoder.phase.detach().cpu().numpy().reshape(-1), np.zeros((n, D), np.float32), stream['efeats'])
    torch.cuda.synchronize()
    for k, t in state_tensors(model).items():
        a = t.detach().cpu().numpy()
        if k == 'has_msg':
            a = np.unpackbits(a.view(np.uint8), bitorder='little')[:n].astype(bool)
        getattr(st, k)[...] = a
    return st


def compare(st, ref, eager, what):
    """everything STEP 4-6 write, bit for bit; the mailbox's time segment within the project's bound for its cosine"""
    worst = 0.0
    assert ref.max_te_arg <= TE_ARG_MAX
    for k in ('left_vals', 'left_ts', 'right_vals', 'right_ts', 'msg_ts', 'has_msg', 'msg_vals'):
        a, b = getattr(st, k), getattr(ref, k)
        if k == 'msg_vals':
            te_a, te_b = a[:, 3 * D:].astype(np.float64), b[:, 3 * D:].astype(np.float64)
            worst = float(np.abs(te_a - te_b).max())
            assert worst <= TE_BOUND, (what, worst)
            a, b = a[:, :3 * D], b[:, :3 * D]
        if a.dtype == np.float32:
            a, b = a.view(np.uint32), b.view(np.uint32)
        np.testing.assert_array_equal(a, b, err_msg=f'{what}: {k}')
    return worst


def main():
    msg_src, mode = sys.argv[1], sys.argv[2]
    eager = mode == 'eager'
    nb = 4
    E = (nb + 2) * B
    stream = bench.make_stream(N_U, N_I, E, 50.0 * E, seed=5, d_e=D)
    model, orc = bench.build_models(stream, D, K, msg_src, 'right', with_oracle=True)   # (the oracle: its graph, for collate)
    model.fuse_attention()
    if eager:
        model.eager_updates()
    res = tuple(torch.from_numpy(stream[k]).to(model.device) for k in ('src', 'dst', 'neg', 'ts', 'eids'))
    # no collate prefetch: a prefetched batch carries times taken before the corruption below
    buf = model.StepBuffers(model, B, False, resident=res, prefetch=False)
    buf.io.lean = 1 if eager else 0
    model.note_rows(0, N_U + N_I)
    out = dict(msg_src=msg_src, mode=mode, forms=[], words={}, te_err=0.0)

    def batch_of(b):
        sl = slice(b * B, (b + 1) * B)
        d = {k: stream[k][sl] for k in ('src', 'dst', 'neg', 'ts', 'eids')}
        d['ts32'] = d['ts'].astype(np.float32)
        return d

    def step():
        buf.err.zero_()
        model.launch_step(buf)
        buf.io.rows_hint = model.rows_bound()
        form = int(_lib.lib.tg_stream_step_form(C.byref(model.model_struct()), C.byref(buf.io)))
        torch.cuda.synchronize()
        return int(buf.err.item()) & 0xFFFFFFFF, form

    def reference_writeback(st, batch, h, new_rows):
        """STEP 4-6 on st; STEP 4's rows: the pending table (eager), or `new_rows` [n_nodes, d] by node"""
        pos = np.concatenate([batch['src'], batch['dst']])
        rows = h if new_rows is None else np.concatenate([h, new_rows])
        return S.writeback(st, batch, rows, None if new_rows is None else 2 * B + pos, np.arange(2 * B),
                           new_from_pending=new_rows is None)

    # ---- two clean steps, each against the reference
    for b in range(2):
        before = pull(model, stream, msg_src)
        word, form = step()
        assert word == 0, f'clean step {b}: word {word}'
        out['forms'].append(form)
        after = pull(model, stream, msg_src)
        h = buf.h[:2 * B].cpu().numpy()
        ref = before.copy()
        # lazy: h(t'+) is computed on the fly and kept nowhere else - STEP 4's rows are taken from the result
        exp = reference_writeback(ref, batch_of(b), h, None if eager else after.right_vals)
        assert exp == 0
        out['te_err'] = max(out['te_err'], compare(after, ref, eager, f'clean step {b}'))
        assert int(buf.offset.item()) == (b + 1) * B

    # ---- corruptions of the state the third batch meets
    batch = batch_of(2)
    cg = O.collate(orc.graph, batch['src'], batch['dst'], batch['neg'], batch['ts'], K, 'static')
    involved = cg['involved']
    st0 = pull(model, stream, msg_src)
    pos = np.concatenate([batch['src'], batch['dst']])
    ts2 = np.tile(batch['ts32'], 2)
    nodes, counts = np.unique(pos, return_counts=True)
    once = nodes[counts == 1]                                      # one position: it wins
    t_of = {int(v): ts2[pos == v][0] for v in once}
    pend_pos = [int(v) for v in once if st0.has_msg[v]]
    free_pos = [int(v) for v in once if not st0.has_msg[v]]
    nbr_only = [int(u) for u in involved if st0.has_msg[u] and u not in set(nodes.tolist())]
    pend_any = [int(u) for u in involved if st0.has_msg[u]]
    assert pend_pos and nbr_only and pend_any, (len(pend_pos), len(free_pos), len(nbr_only))
    mem_ts = 'left_ts' if msg_src == 'left' else 'right_ts'
    cases = {}
    v = pend_pos[0]
    cases['a: message-source time past the event (pending node)'] = [(mem_ts, v, up(t_of[v]))]
    cases['a: the same, the message moved along'] = [(mem_ts, v, up(t_of[v])), ('msg_ts', v, up(t_of[v]))]
    if free_pos:
        w = free_pos[0]
        cases['a: message-source time past the event (no pending message)'] = [(mem_ts, w, up(t_of[w]))]
    cases['a: message-source time equal to the event'] = [(mem_ts, v, t_of[v]), ('msg_ts', v, t_of[v])]
    cases['b: left time past the event'] = [('left_ts', v, up(t_of[v]))] + \
        ([('msg_ts', v, up(t_of[v]))] if msg_src == 'left' else [])
    cases['c: right time past the message'] = [('right_ts', v, up(st0.msg_ts[v]))]
    cases['c: right time equal to the message'] = [('right_ts', v, st0.msg_ts[v])]
    u = nbr_only[0]
    cases['d: message before memory, neighbour only'] = [('msg_ts', u, down(getattr(st0, mem_ts)[u]))]
    if msg_src == 'left':
        cases['e: message time unequal to the left time'] = [('msg_ts', pend_any[-1], up(st0.msg_ts[pend_any[-1]]))]

    tens = state_tensors(model)
    keep = dict(tens)
    for k in ('_gtab', '_ctab'):         # the per-node tables a step refreshes for its positive nodes
        if getattr(model, k, None) is not None:
            keep[k] = getattr(model, k)
    saved = {k: t.detach().clone() for k, t in keep.items()}
    off = buf.offset.clone()

    def restore():
        for k, t in keep.items():
            t.data.copy_(saved[k])       # (.data: the host-side version counters stay - nothing is rebuilt for a time)
        buf.offset.copy_(off)

    zeros = np.zeros((2 * B, D), np.float32)
    some = 0
    for name, edits in cases.items():
        st = st0.copy()
        for field, node, value in edits:
            getattr(st, field)[node] = value
            tens[field].data[node] = float(value)
        exp = S.step_invariants(st, batch, involved)
        exp |= reference_writeback(st, batch, zeros, None if eager else np.zeros((st.n_nodes, D), np.float32))
        word, form = step()
        out['words'][name] = [word, exp]
        assert word == exp, f'{name}: word {word}, reference {exp}'
        assert (' equal to ' in name) == (exp == 0), (name, exp)   # (the cases named `... equal to ...` violate nothing)
        if exp:
            some |= exp
            try:
                _lib.raise_invariants(word)
            except ValueError:
                pass
            else:
                raise AssertionError(f'{name}: raise_invariants did not raise on {word}')
        restore()
    restore()
    word, form = step()
    assert word == 0, f'after the restore: word {word}'
    out['forms'].append(form)
    want = S.ERR_PAST_MEMORY | S.ERR_MSG_BEFORE_MEM | S.ERR_EVENT_BEFORE_MEM | (S.ERR_MSG_TS_MISMATCH if msg_src == 'left' else 0)
    assert some & want == want, some
    print(json.dumps(out))
    print('INVARIANT-CASE OK', flush=True)


if __name__ == '__main__':
    main()
