"""Every kernel body of the fused GRU cell (csrc/tg_gru.hip: gru_launch) x every operand / epilogue feature of GruArgs,
against the float64 reference of the whole contract (tests/_gru_ref.py), through tg_debug_gru - one cell straight into
gru_launch, which also reports the family and instance it picked.

Each case of _gru_ref.CASES names the form it was sized for; the test first asserts that this form ran, so a retuned
threshold fails here instead of silently moving the case to another body.  Then two kinds of data:
  * dyadic: multiples of 1/8 with sparse weights - every pre-activation is exact in float32 whatever the k order, the
    k-split or the MFMA grouping, so the saved h_n plane equals the reference bit for bit, r and z carry the error of
    fast_sigmoid alone, and n that of fast_tanh once its argument is formed from the device's own saved r;
  * gaussian times a per-row scale exp(U(-2, 2)): the whole derived elementwise bound (linear part, propagation through
    the gate and blend expressions, function evaluation) - tests/_gru_ref.py states the derivation.
out, out2 and gates lie in NaN arenas with 64 guard floats on each side: guards, rows at or past the live count, rows
out_rows does not name, columns [d, ldo) and the gates / out2 rows of dead launch rows must keep their bits; the operands
sit in tables with NaN wherever the cell must not read and are unchanged after the call.
k_gru_direct and k_gru<1, 4> run only under TG_GRU_D16=0 (the 16 x 16 condition holds wherever `micro` does): their cases,
and two that put k_gru_direct16 where it never runs by itself, go through tests/_gru_knob_case.py in one child process per
setting.  Run with -s to see the worst observed fraction of each allowance per family."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _gru_ref as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
HERE_CASES = [c for c in R.CASES if not c.env]
WORST = {}  # (family, allowance) -> worst observed fraction


@pytest.mark.parametrize('kind', ['dyadic', 'gauss'])
@pytest.mark.parametrize('c', HERE_CASES, ids=[c.id for c in HERE_CASES])
def test_gru_form(c, kind):
    from _gru_knob_case import check_case
    worst = check_case(c, kind)
    fam = R.family(c.form)
    for key, v in worst.items():
        WORST[fam, key] = max(WORST.get((fam, key), 0.0), v)
    print(f'  WORST fraction of the allowances ({c.form}, {kind}): ' + ' '.join(f'{k} {v:.3f}' for k, v in worst.items()) +
          f'; {fam} so far: ' + ' '.join(f'{k} {v:.3f}' for (f, k), v in sorted(WORST.items()) if f == fam))


def test_nothing_is_written_without_live_rows():
    """*n_dev = 0 in every family that runs without a knob: all three arenas keep every bit"""
    from _gru_knob_case import run_on_device
    forms = set()
    for c in HERE_CASES:
        if c.n_dev == 0:
            p = R.build(c, 'dyadic')
            form, out, out2, gates = run_on_device(p)
            assert form == c.form
            for a, b in ((out, p.out), (out2, p.out2), (gates, p.gates)):
                assert a is None or np.array_equal(a.view(np.int32), b.view(np.int32)), c.id
            forms.add(c.form)
    assert forms >= {'direct16<3>', 'direct16<6>', 'direct16<3,blend>', 'gru<2,4>', 'gru<3,4>', 'gru<3,4,tail16>', 'gru<4,2>',
                     'gru<4,1>'}


def test_blend_with_gates_is_refused_and_writes_nothing():
    from www2023tiger_amd import _lib
    from _gru_knob_case import run_on_device
    c = next(c for c in HERE_CASES if c.blend and c.cap == 100 and c.out2)
    p = R.build(c, 'dyadic')
    p.gates = np.full(2 * R.GUARD + p.cap * 4 * p.d, np.nan, dtype=np.float32)
    form, out, out2, gates = run_on_device(p, expect_rc=_lib.TG_EUNSUPPORTED)
    assert form is None
    for a, b in ((out, p.out), (out2, p.out2), (gates, p.gates)):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.parametrize('setting', R.KNOB_SETTINGS, ids=[s.replace(' ', ',') for s in R.KNOB_SETTINGS])
def test_gru_forms_under_knob(setting):
    """the cases of one knob setting in a fresh child process (one at a time), which prints an OK line"""
    env = dict(os.environ)
    for kv in setting.split():
        k, v = kv.split('=')
        env[k] = v
    env['TG_GRU_KNOB_CASE'] = setting
    r = subprocess.run([sys.executable, os.path.join(HERE, '_gru_knob_case.py')], env=env, capture_output=True, text=True,
                       timeout=300)
    ok = [l for l in r.stdout.splitlines() if l.startswith('GRU-KNOB-CASE OK')]
    assert r.returncode == 0 and len(ok) == 1, f'{setting}:\n{(r.stdout + r.stderr)[-3000:]}'
    want = sorted({c.form for c in R.CASES if c.env == setting})
    assert f'forms {" ".join(want)};' in ok[0]
    print('  ' + ok[0])


def test_every_form_of_gru_launch_is_the_expected_form_of_a_case():
    assert {c.form for c in R.CASES} == set(R.ALL_FORMS) and len(R.ALL_FORMS) == 11
    assert {c.form for c in HERE_CASES} == set(R.ALL_FORMS) - set(R.KNOB_ONLY)
