"""One streaming run on a stream with few nodes (most positions of a batch lose the positive-node dedup, winners repeat
from batch to batch): resident stream, lean eager step with pre-multiplied weights, per-node tables and collate prefetch.
tests/test_hip_fc2_deferred.py runs it in-process (the four-launch form, TG_FORM_FC2_DEFERRED, where the library takes it)
and - the library reads its knobs once per process - as a child process with TG_FC2_DEFER=0 (the five-launch chain):
  python _fc2_defer_case.py D B UPD_SRC N_BATCHES OUT.npz"""
import ctypes as C
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.dirname(HERE) not in sys.path:
    sys.path.insert(0, os.path.dirname(HERE))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

N_U, N_I, K = 40, 12, 10
FORM_FC2_DEFERRED = 16


def make(d, B, upd_src, nb, with_oracle=False, seed=5, dropout=0.1):
    import bench
    E = (nb + 2) * B
    stream = bench.make_stream(N_U, N_I, E, 50.0 * E, seed=seed, d_e=d)
    model, orc = bench.build_models(stream, d, K, 'left', upd_src, with_oracle=with_oracle, dropout=dropout)
    model.fuse_attention()
    model.eager_updates()
    res = tuple(torch.from_numpy(stream[k]).to(model.device) for k in ('src', 'dst', 'neg', 'ts', 'eids'))
    buf = model.StepBuffers(model, B, False, resident=res, prefetch=True, debug_lists=True)
    buf.io.lean = 1
    model.note_rows(0, N_U + N_I)  # the bound on a batch's unique positive nodes: every node (selects the small launches)
    _ = model.graph.tcsr, model.model_struct()
    return stream, model, orc, buf


def form_bits(model, buf):
    from www2023tiger_amd._lib import lib
    buf.io.rows_hint = model.rows_bound()
    return int(lib.tg_stream_step_form(C.byref(model.model_struct()), C.byref(buf.io)))


def run(d, B, upd_src, nb, on_step=None):
    """nb steps; per step h of cat[src, dst, neg], the consumed neighbour lists and the form the library reported; the final
    state.  on_step(b, stream, orc, buf): the caller's per-step check."""
    stream, model, orc, buf = make(d, B, upd_src, nb, with_oracle=on_step is not None)
    out = {}
    for b in range(nb):
        model.launch_step(buf)
        out[f'form{b}'] = np.int64(form_bits(model, buf))
        torch.cuda.synchronize()
        assert int(buf.err.item()) == 0, f'invariant word {int(buf.err.item())} at batch {b}'
        out[f'h{b}'] = buf.h.cpu().numpy().copy()
        out[f'l1n{b}'] = buf.dbg_l1_nids.cpu().numpy().copy()
        out[f'l1e{b}'] = buf.dbg_l1_eids.cpu().numpy().copy()
        out[f'l1t{b}'] = buf.dbg_l1_ts.cpu().numpy().copy()
        if on_step is not None:
            on_step(b, stream, orc, buf)
    out['has_msg'] = model.msg_store.has_msg_mask().cpu().numpy()
    for k, t in (('left', model.left_memory.vals), ('right', model.right_memory.vals), ('left_ts', model.left_memory.update_ts),
                 ('right_ts', model.right_memory.update_ts), ('mailbox', model.msg_store.node_msg_vals),
                 ('msg_ts', model.msg_store.node_msg_ts), ('pending', model._pending)):
        out[k] = t.cpu().numpy().copy()
    return out, model, orc


if __name__ == '__main__':
    d, B, upd_src, nb, path = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], int(sys.argv[4]), sys.argv[5]
    res, _, _ = run(d, B, upd_src, nb)
    np.savez(path, **res)
    print('FC2-DEFER-CASE OK', flush=True)
