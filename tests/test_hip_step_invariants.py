"""The invariant word of WHOLE streaming steps, per step form.  The one-pass write-back, the rider with a snapshot and the
snapshot-free rider are reachable only through tg_stream_step, and the library reads its knobs once per process: every
setting runs tests/_invariant_case.py in a child process (at most four at a time, each under its own time limit; every
exit status is checked).  The child compares two clean steps table by table with tests/_state_ref.py, then corrupts
single TIMES of the state the next batch meets and compares the whole word with the reference's
step_invariants + writeback on the same state."""
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
DIRECT, FUSED_WB, LEAN, TABLES, FC2_DEFERRED = 1, 2, 4, 8, 16   # include/tiger_hip.h: TG_FORM_*

# (knobs, message source, eager | lazy, form bits that must be set, form bits that must be clear)
CASES = [
    ('', 'left', 'eager', DIRECT | FUSED_WB | LEAN | FC2_DEFERRED, 0),            # snapshot-free rider, four launches
    ('TG_FC2_DEFER=0', 'left', 'eager', DIRECT | FUSED_WB | LEAN, FC2_DEFERRED),  # rider with a snapshot, on fc1's launch
    ('TG_FC2_DEFER=0 TG_WB_RIDER_FC1=0', 'left', 'eager', DIRECT | FUSED_WB | LEAN, FC2_DEFERRED),   # ... on fc2's
    ('TG_WB_RIDER=0', 'left', 'eager', DIRECT | FUSED_WB | LEAN, FC2_DEFERRED),   # k_writeback_fused
    ('TG_EAGER_DIRECT=0', 'left', 'eager', 0, DIRECT | FUSED_WB | LEAN | FC2_DEFERRED),   # two launches behind the gather
    ('TG_EAGER_DIRECT=0', 'right', 'eager', 0, DIRECT | FUSED_WB | LEAN | FC2_DEFERRED),
    ('', 'left', 'lazy', 0, DIRECT | FUSED_WB | LEAN | TABLES | FC2_DEFERRED),    # no table of pending rows
    ('', 'right', 'lazy', 0, DIRECT | FUSED_WB | LEAN | TABLES | FC2_DEFERRED),
    ('', 'right', 'eager', DIRECT | FUSED_WB | LEAN, FC2_DEFERRED),               # msg_src = right never defers fc2
]
IDS = [f'{k.replace(" ", ",") or "default"}-{src}-{mode}' for k, src, mode, _, _ in CASES]
GROUP = 4  # child processes at a time


def _run_case(case):
    knobs, msg_src, mode = case[:3]
    env = dict(os.environ)
    for kv in knobs.split():
        k, v = kv.split('=')
        env[k] = v
    env.setdefault('OMP_NUM_THREADS', '4')
    env.setdefault('MKL_NUM_THREADS', '4')
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, '_invariant_case.py'), msg_src, mode], env=env,
                           capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired as e:
        return 124, str(e.stdout or ''), str(e.stderr or '') + '\ntime limit'
    return r.returncode, r.stdout, r.stderr


_RESULTS = {}


def _result(i):
    if i not in _RESULTS:
        from concurrent.futures import ThreadPoolExecutor
        group = list(range(i - i % GROUP, min(i - i % GROUP + GROUP, len(CASES))))
        with ThreadPoolExecutor(max_workers=GROUP) as ex:
            _RESULTS.update(zip(group, ex.map(_run_case, [CASES[j] for j in group])))
    return _RESULTS[i]


@pytest.mark.gpu
@pytest.mark.parametrize('i', range(len(CASES)), ids=IDS)
def test_invariant_word_per_step_form(i):
    rc, out, err = _result(i)
    tail = (out + err)[-3000:]
    assert rc == 0 and 'INVARIANT-CASE OK' in out, f'{IDS[i]}:\n{tail}'
    res = json.loads([l for l in out.splitlines() if l.startswith('{')][-1])
    must, must_not = CASES[i][3:]
    print(f'{IDS[i]}: forms {res["forms"]}, time segment max abs err {res["te_err"]:.3e}, words {res["words"]}')
    for form in res['forms']:
        assert form & must == must and not (form & must_not), (IDS[i], form)
    assert len(res['words']) >= 7 and all(got == exp for got, exp in res['words'].values())
