"""tests/_gru_ref.py's Problems through tg_debug_gru on the device (run_on_device, check_case: shared with
tests/test_hip_gru_forms.py), and - run as a script - the cases of ONE knob setting in a process of its own: the library
reads its knobs once per process, and k_gru_direct / k_gru<1, 4> run only under TG_GRU_D16=0 (tests/_gru_ref.py: the case
table).  The setting is read from TG_GRU_KNOB_CASE and must already be in the environment; prints one line per case and
`GRU-KNOB-CASE OK <cases> ...` on success."""
import ctypes as C
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import _gru_ref as R  # noqa: E402


def dev():
    return torch.device('cuda:0')


def run_on_device(p, expect_rc=0):
    """the Problem through tg_debug_gru: (form, out, out2, gates) - the three arenas after the call (None where absent)"""
    from www2023tiger_amd import _lib
    from www2023tiger_amd.hip_ops import stream_ptr
    keep = []

    def up(a):
        if a is None:
            return None
        t = torch.from_numpy(a).to(dev())
        keep.append((t, a))
        return t.data_ptr()

    arenas = [None if a is None else torch.from_numpy(a).to(dev()) for a in (p.out, p.out2, p.gates)]
    inside = lambda t: None if t is None else t.data_ptr() + 4 * R.GUARD
    x_idx = up(p.x_idx)
    probe = _lib.TgGruProbe(
        cap=p.cap, n_dev=up(np.array([p.n_dev], np.int32)) if p.n_dev is not None else None, d=p.d, xw=p.xw,
        x=up(p.x), x_ld=p.x_ld, x_w=p.xw, x_idx=x_idx,
        h=up(p.h), h_ld=p.h_ld, h_w=p.d, h_idx=x_idx if p.h_idx is p.x_idx else up(p.h_idx),
        w_ih=up(p.w_ih), w_hh=up(p.w_hh), b_ih=up(p.b_ih), b_hh=up(p.b_hh),
        out=inside(arenas[0]), ldo=p.ldo, out_rows=up(p.out_rows), gates=inside(arenas[2]),
        out2=inside(arenas[1]), add2=up(p.add2), out2_by_row=p.out2_by_row,
        rows_hint=p.rows_hint, x_skip_at=p.skip_at, x_skip_n=p.skip_n, w_blend=up(p.w_blend), b_blend=up(p.b_blend))
    form = C.c_char_p()
    rc = _lib.lib.tg_debug_gru(C.byref(probe), C.byref(form), stream_ptr(dev()))
    if expect_rc == 0:
        _lib.check(rc, 'tg_debug_gru')
    else:
        assert rc == expect_rc, rc
    torch.cuda.synchronize()
    for t, a in keep:  # the operands are read only
        assert np.array_equal(t.cpu().numpy().view(np.uint8), a.view(np.uint8))
    return (form.value.decode() if form.value else None, *(None if t is None else t.cpu().numpy() for t in arenas))


def check_case(c, kind):
    """the form the case was sized for ran; every arena against the float64 reference.  Returns the worst fractions."""
    p = R.build(c, kind)
    form, out, out2, gates = run_on_device(p)
    assert form == c.form, f'{c.id}: sized for {c.form}, but gru_launch picked {form}'
    return R.compare(p, R.reference(p), out, out2, gates)


def main():
    setting = os.environ.get('TG_GRU_KNOB_CASE', '')
    for kv in setting.split():
        k, v = kv.split('=')
        assert os.environ.get(k) == v, f'{k} must be set for the whole process'
    cases = [c for c in R.CASES if c.env == setting]
    assert setting and cases
    worst = {}
    for c in cases:
        for kind in ('dyadic', 'gauss'):
            w = check_case(c, kind)
            if c.n_dev == 0:
                p = R.build(c, kind)
                form, out, out2, gates = run_on_device(p)
                for a, b in ((out, p.out), (out2, p.out2), (gates, p.gates)):
                    assert a is None or np.array_equal(a.view(np.int32), b.view(np.int32)), c.id
            for key, v in w.items():
                worst[key] = max(worst.get(key, 0.0), v)
            print(f'  {c.id} [{kind}]: ' + ' '.join(f'{k} {v:.3f}' for k, v in w.items()), flush=True)
    forms = sorted({c.form for c in cases})
    print(f'GRU-KNOB-CASE OK {len(cases)} cases, forms {" ".join(forms)}; WORST fractions: ' +
          ' '.join(f'{k} {v:.3f}' for k, v in sorted(worst.items())), flush=True)


if __name__ == '__main__':
    main()
