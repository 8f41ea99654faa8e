"""The float64 reference of the fused GRU cell's whole contract (csrc/tg_dense.h: GruArgs, include/tiger_hip.h:
tg_debug_gru), a Python mirror of its dispatcher (csrc/tg_gru.hip: gru_launch), the case table of
tests/test_hip_gru_forms.py, the derived elementwise bound and the comparator - all of it host code, checked without a GPU
by tests/test_gru_ref_host.py.

A Problem holds the operands AS THEY LIE IN MEMORY: x, h, add2 and the blend operand sit in tables larger than what the
cell reads, NaN wherever it must not read (table rows nobody indexes, the row dead index entries point at, columns past a
row's width, rows at or past the live count, the message columns of skipped k-tiles, which the reference takes as
zero); out, out2 and gates lie in NaN arenas with 64 guard floats on each side.

For each live row m < M = min(cap, n_dev), xr = x[x_idx[m] or m], hr = h[h_idx[m] or m], o = out_rows[m] or m:
    r = sigmoid(W_ir xr + b_ir + W_hr hr + b_hr)     z likewise     h_n = W_hn hr + b_hn
    n = tanh(W_in xr + b_in + r h_n)                 v = (1 - z) n + z hb,   hb = hr, or w_blend hr + b_blend (blend form:
    out[o * ldo + j] = v                                                     the handed w_hh / b_hh are used as given)
    gates[m, 0..3, j] = r, z, n, h_n                 out2[(o if out2_by_row else m) * d + j] = v + add2[o * d + j]
Every other float of the three arenas keeps its bits.

THE BOUND (derived, nothing in it is measured from the kernels).  u = 2^-24 (one float32 rounding is at most u |result|).
  Linear part.  A float32 inner product of k terms summed in any order, any k-split, any MFMA grouping, is within
  k u sum|a_i w_i| of the exact value (each term passes through at most k additions, each rounded once; the MFMA does
  not round the products; -ffp-contract=off keeps every other operation a separately rounded one).  The kernels add at
  most three k-group folds, the sum b_ih + b_hh and the bias add on top, and one unit covers the second-order terms:
      eps_p = (k_p + 6) u mag_p,   mag_p = sum |a||w| + |biases|
  with k = xw' + d for r and z, xw' for i_n (xw' = xw less the skipped columns), d for h_n and for the rebuilt h of the
  blend form.  On `dyadic` data (below) every pre-activation is exact and eps_p = 0.
  Function evaluation, from the code of fast_sigmoid / fast_tanh (csrc/tg_common.h) under the premise stated there: the
  hardware exp2 and reciprocal (v_exp_f32, v_rcp_f32) are within 1 ulp, i.e. 2 u relative.  (The reciprocal the build
  emits for __frcp_rn is in fact the correctly rounded division, u; the premise is kept, it is the weaker one.  The
  guides of this project state no other accuracy for the two instructions.)
    __expf(y) = exp2(fl(L y)), L = 0x1.715476p+0 = log2(e) (1 - 0.22 u): the argument is y log2(e) (1 + eta), |eta| <=
    1.25 u, so the result is e^y (1 + ee), |ee| <= 1.25 u |y| + 2 u - the argument's rounding grows with |y|.
    sigmoid(x) = rcp(fl(1 + E')), E' ~ E = e^-x: d ln s = -(E / (1 + E)) ee - d_add + d_rcp, so
        |s' - s| <= s [(1 - s)(1.25 |x| + 2) + 3] u                                  =: E_sig(x)
    tanh(x) = sign(x) fl(fl(1 - E') rcp(fl(1 + E'))), E = e^-2|x| (the product by -2 is exact), T = tanh|x|:
    d ln T = -(2 E / (1 - E^2)) ee + d_sub - d_add + d_rcp + d_mul, and T 2 E / (1 - E^2) = (1 - T^2) / 2, so
        |t' - t| <= [(1 - T^2) / 2 (2.5 |x| + 2) + 5 T] u                            =: E_tanh(x)
    Results below 2^-126 are flushed: both allowances carry + 2^-126.  (Near x = 0 E_tanh is u absolute, not relative:
    that is how 1 - e behaves, and the bound says so.)
  Propagation (sigmoid' <= 1/4, tanh' <= 1, one rounding per float32 add or multiply of the gate and blend expressions):
      D_r = eps_r / 4 + E_sig(a_r)        D_z likewise        D_hn = eps_hn
      p = (i_n + b_in) + r h_n:  D_p = eps_in + |r| eps_hn + |h_n| D_r + u |r h_n| + u |p|
      D_n = D_p + E_tanh(p)
      v = (1 - z) n + z hb:      D_v = |hb - n| D_z + u |1 - z| |n| + |1 - z| D_n + u |(1 - z) n| + z eps_hb + u |z hb| + u |v|
      out2 with add2:            D_v + u |v + add|
  and the whole is multiplied by 1.01 for the second-order terms (all of them products of two of the above, each
  below 1e-4 relative at the magnitudes of these cases).
  Isolation on dyadic data: r and z then carry E_sig alone.  The n plane does too once its pre-activation is formed in
  float64 from the DEVICE's saved r and the exact h_n: p' = (i_n + b_in) + r_dev h_n, three roundings (the bias add, the
  product, the sum) u (|i_n + b_in| + |r_dev h_n| + |p'|), then E_tanh(p').  The saved h_n plane must equal the
  reference bit for bit.
"""
from types import SimpleNamespace

import numpy as np

GUARD = 64
U24 = 2.0 ** -24
FLUSH = 2.0 ** -126
SLACK = 1.01
BK = 32
T16_ROWS = 144
KNOBS = ('TG_GRU_NW', 'TG_GRU_D16', 'TG_GRU_MICRO', 'TG_GRU_DIRECT', 'TG_GRU_KS')


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------------------------
# gru_launch, restated (csrc/tg_gru.hip): the form a launch takes from (cap, rows_hint, d), the blend flag and the knobs
# ------------------------------------------------------------------------------------------------------------------
def dispatch(cap, rows_hint, d, blend=False, gates=False, env=None):
    """the name tg_debug_gru reports; None: nothing is launched; 'unsupported': TG_EUNSUPPORTED"""
    env = env or {}
    nw, d16 = int(env.get('TG_GRU_NW', 0)), int(env.get('TG_GRU_D16', 1))
    micro_knob, direct_knob, ks_knob = int(env.get('TG_GRU_MICRO', 1)), int(env.get('TG_GRU_DIRECT', 1)), int(env.get('TG_GRU_KS', 0))
    if cap <= 0:
        return None
    rows = min(rows_hint, cap) if rows_hint > 0 else cap
    NT, NT16 = cdiv(d, 32), cdiv(d, 16)
    d16_ok = nw == 0 and d16 != 0 and (d16 == 3 or cdiv(rows, 96) * NT16 <= 256)
    if blend and (gates or not d16_ok):
        return 'unsupported'
    if d16_ok:
        rt3 = cdiv(rows, 48) * NT16 <= 256
        return f'direct16<{3 if rt3 else 6}{",blend" if blend else ""}>'
    use_tail = 0 < d % 32 <= 16
    small = cdiv(rows, 96) * (NT - use_tail) + (cdiv(rows, T16_ROWS) if use_tail else 0) + 8 <= 256
    tiny = cdiv(cdiv(rows, 64), 8) * NT <= 32
    micro = cdiv(cdiv(rows, 32), 8) * NT <= 40
    if nw == 1 or (nw == 0 and micro and micro_knob):
        return 'direct' if direct_knob else 'gru<1,4>'
    if nw == 2 or (nw == 0 and tiny):
        return 'gru<2,4>'
    if nw == 3 or (nw == 0 and small):
        return 'gru<3,4,tail16>' if use_tail else 'gru<3,4>'
    grid = 8 * cdiv(cdiv(cap, 128), 8) * NT
    live = cdiv(min(rows_hint, cap), 128) * NT if rows_hint > 0 else grid
    return 'gru<4,2>' if ks_knob == 2 or (ks_knob == 0 and live <= (320 if rows_hint > 0 else 256)) else 'gru<4,1>'


def direct16_rt(M, d, rtm):
    """rows / 16 of the blocks k_gru_direct16<rtm> forms for M live rows"""
    NT = cdiv(d, 16)
    if cdiv(M, 16) * NT <= 256:
        return 1
    if cdiv(M, 32) * NT <= 256:
        return 2
    if rtm > 3 and cdiv(M, 48) * NT <= 256:
        return 3
    if rtm > 3 and cdiv(M, 64) * NT <= 256:
        return 4
    return rtm


STAGES = ('direct16', 'gru<2,4>', 'gru<3,4', 'gru<4,2>', 'gru<4,1>')   # the order the forms follow one another as cap grows


def first_cap(d, stage):
    """the smallest cap (no rows_hint, no knob) at which gru_launch is at or past `stage`; None if it never gets there
    below 2^20 rows (every condition of the dispatcher is monotone in the row count)"""
    at = lambda cap: max(i for i, s in enumerate(STAGES) if dispatch(cap, 0, d).startswith(s))
    want = STAGES.index(stage)
    lo, hi = 1, 1 << 20
    if at(hi) < want:
        return None
    while lo < hi:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if at(mid) >= want else (mid + 1, hi)
    return lo


# ------------------------------------------------------------------------------------------------------------------
# the case table.  Which forms a launch reaches WITHOUT a knob: `micro` (ceil(ceil(rows / 32) / 8) NT <= 40) implies the
# 16 x 16 condition (ceil(rows / 96) NT16 <= 256): with a = ceil(rows / 32) <= 8 floor(40 / NT) and NT16 <= 2 NT,
# ceil(a / 3) 2 NT <= (640 + 4 NT) / 3 <= 256 for NT <= 32, and for 32 < NT <= 40 a <= 8 gives 3 * 2 * 40 = 240
# (tests/test_gru_ref_host.py also checks it by enumeration).  So k_gru_direct ('direct') and k_gru<1, 4> run only under
# TG_GRU_D16=0 and TG_GRU_D16=0 TG_GRU_DIRECT=0; their cases carry that setting in `env` and run in a child process.
# Everything else is reached by the row count alone (first_cap), at small d and xw so that tens of thousands of rows
# stay cheap.  d = 4: one 16-column tile; `tiny` then lies inside the 16 x 16 condition and k_gru<3, 4> runs the tail
# blocks ONLY (no 32-column tile at all), which also hides k_gru<4, 2> without a hint.
# ------------------------------------------------------------------------------------------------------------------
DEFAULTS = dict(n_dev=None, rows_hint=0, gather=None, pad=0, out_rows=False, ldo_pad=0, gates=False, out2=None,
                skip=None, blend=False, env='')
OUT2 = (None, 'dense', 'add2', 'by_row', 'by_row_add2')
CASES = []


def case(form, cap, d, xw, **feat):
    bad = set(feat) - set(DEFAULTS)
    assert not bad, bad
    c = SimpleNamespace(form=form, cap=cap, d=d, xw=xw, **{**DEFAULTS, **feat})
    assert c.out2 in OUT2 and c.gather in (None, 'x', 'h', 'same')
    tags = [f'{key}={feat[key]}'.replace(' ', '+') if not isinstance(feat[key], bool) else key for key in feat if key != 'env']
    c.id = f'{form}-{cap}x{d}x{xw}' + ('-' + '-'.join(tags) if tags else '') + ('-' + c.env.replace(' ', '+') if c.env else '')
    CASES.append(c)


def env_of(c):
    return dict(kv.split('=') for kv in c.env.split())


def expected_form(c):
    return dispatch(c.cap, c.rows_hint, c.d, c.blend, c.gates, env_of(c))


# feature sets dealt round robin over the shape sweeps (every form meets each of them at some shape)
FEATS = [
    dict(),
    dict(gather='same', out_rows=True, ldo_pad=4, gates=True, pad=4),                   # the updater's use
    dict(gather='x', out2='dense'),
    dict(gather='h', out_rows=True, out2='add2', pad=8),                                # add2 by the OUTPUT row
    dict(out_rows=True, ldo_pad=8, out2='by_row'),
    dict(gather='same', out_rows=True, out2='by_row_add2', gates=True),
    dict(gates=True, out2='add2'),
    dict(gather='h', gates=True, ldo_pad=4),
]
_deal = [0]


def feat(**more):
    f = dict(FEATS[_deal[0] % len(FEATS)])
    _deal[0] += 1
    f.update(more)
    return f


def _row_edges(form, cap, d, xw, tile, **kw):
    """1, tile - 1, tile, tile + 1 live rows, then 0, a count past cap (clamped: the whole capacity) and no count at all"""
    for nd in (1, tile - 1, tile, tile + 1):
        case(form, cap, d, xw, **feat(n_dev=nd, **kw))
    case(form, cap, d, xw, **feat(n_dev=0, **kw))
    case(form, cap, d, xw, **feat(n_dev=cap + 5, **kw))
    case(form, cap, d, xw, **feat(**kw))


def _skips(form, cap, d, nd, **kw):
    """zero k-tiles skipped: at the first message tile and in the middle, runs of 1 and 3, a partial tile behind the run"""
    case(form, cap, d, 36, **feat(n_dev=nd, skip=(0, 1), **kw))
    case(form, cap, d, 100, **feat(n_dev=nd, skip=(0, 3), **kw))
    case(form, cap, d, 100, **feat(n_dev=nd, skip=(1, 1), **kw))
    case(form, cap, d, 164, **feat(n_dev=nd, skip=(1, 3), **kw))
    case(form, cap, d, 128, **feat(n_dev=nd, skip=(2, 1), **kw))   # whole tiles behind the run


# -- k_gru_direct16: d = 20 (NT16 = 2): the <3> instance while cap <= 6 144, <6> to 12 288; rt from the LIVE count: 1 to
#    2 048 rows, 2 to 4 096, (<6>: 3 to 6 144, 4 to 8 192,) then RTM
assert first_cap(20, 'gru<2,4>') == 12289 and dispatch(6144, 0, 20) == 'direct16<3>' and dispatch(6145, 0, 20) == 'direct16<6>'
_row_edges('direct16<3>', 4200, 20, 36, 16)                                   # rt = 1
for _nd in (2079, 2080, 2081):                                                # rt = 2: 32-row blocks
    case('direct16<3>', 4200, 20, 36, **feat(n_dev=_nd))
for _nd in (4127, 4128, 4129):                                                # rt = 3 = RTM: 48-row blocks
    case('direct16<3>', 4200, 20, 36, **feat(n_dev=_nd))
case('direct16<3>', 17, 20, 36, **feat())                                     # a grid of 8 blocks
case('direct16<3>', 1, 4, 4, **feat())
case('direct16<3>', 50, 4, 20, **feat(n_dev=33))                              # d = 4, xw < 32
case('direct16<3>', 30000, 20, 36, **feat(rows_hint=1000, n_dev=13000))       # 542 tiles of 48 rows on 256 blocks
case('direct16<3>', 30000, 20, 64, **feat(rows_hint=6144))                    # the hint picks the instance; 30 000 live rows
_row_edges('direct16<6>', 8300, 20, 36, 16)                                   # the large instance on few live rows: rt = 1
for _nd in (2079, 2080, 2081, 4127, 4128, 4129, 6207, 6208, 6209, 8255, 8256, 8257):   # rt = 2, 3, 4, 6
    case('direct16<6>', 8300, 20, 36, **feat(n_dev=_nd))
case('direct16<6>', 50000, 20, 36, **feat(rows_hint=7000, n_dev=33))          # large cap and hint, few live rows
case('direct16<6>', 30000, 20, 36, **feat(rows_hint=7000, n_dev=25000))       # 522 tiles of 96 rows: second and third tiles
case('direct16<6>', 12288, 20, 64, **feat())                                  # the last 16 x 16 launch at this width
for _d, _xw in ((36, 64), (44, 36), (48, 20), (52, 100), (60, 36), (64, 64), (172, 36)):   # d % 16 != 0 and = 0; several k-tiles
    _c3 = first_cap(_d, 'gru<2,4>') - 1
    _rt3 = 48 * (256 // cdiv(_d, 16))                                          # the last launch of the small instance
    case('direct16<3>', _rt3, _d, _xw, **feat(n_dev=_rt3 - 47))
    case('direct16<6>', _c3, _d, _xw, **feat(n_dev=_c3 - 95))
_skips('direct16<3>', 100, 20, 49)
_skips('direct16<6>', 8300, 20, 8257)
_skips('direct16<3>', 100, 44, 97)
# the blend form: h.idx lists rows of t, out2 / add2 by out_rows; both instances at their last launch and on few rows
for _d, _xw, _f in ((20, 36, dict(gather='h', ldo_pad=4)), (44, 64, dict(gather='same', out2='by_row_add2', pad=4)),
                    (36, 36, dict(gather='h', out2='add2', skip=(0, 1))), (172, 36, dict(gather='h', out2='add2'))):
    _c3, _c6 = 48 * (256 // cdiv(_d, 16)), first_cap(_d, 'gru<2,4>') - 1
    case('direct16<3,blend>', _c3, _d, _xw, out_rows=True, blend=True, n_dev=_c3 - 47, **_f)
    case('direct16<3,blend>', 100, _d, _xw, out_rows=True, blend=True, n_dev=49, **_f)
    case('direct16<6,blend>', _c6, _d, _xw, out_rows=True, blend=True, n_dev=_c6 - 95, **_f)
    case('direct16<6,blend>', _c6, _d, _xw, out_rows=True, blend=True, n_dev=17, **_f)
case('direct16<3,blend>', 4200, 20, 36, gather='h', out_rows=True, blend=True, n_dev=0)

# -- the LDS-staged blocks: 64-, 96- (+ 144-row tail), 128-row tiles.  The shape sweep takes every d % 32 in
#    {0, 4, 12, 16, 20, 28}: the padded column tile, the 16-column tail (gru<3,4,tail16>: 4, 12, 16) and no tail.
_STAGED = (('gru<2,4>', 'gru<2,4>', 64), ('gru<3,4>', 'gru<3,4', 96), ('gru<3,4,tail16>', 'gru<3,4', 96),
           ('gru<4,2>', 'gru<4,2>', 128), ('gru<4,1>', 'gru<4,1>', 128))
for _form, _stage, _tile in _STAGED:
    _tail = _form.endswith('tail16>')
    _d0 = 44 if _tail else 20
    _cap = first_cap(_d0, _stage)
    assert dispatch(_cap, 0, _d0) == _form, (_form, _cap, dispatch(_cap, 0, _d0))
    _row_edges(_form, _cap, _d0, 36, _tile)
    if _tail:
        for _nd in (T16_ROWS - 1, T16_ROWS, T16_ROWS + 1, 8 * 96 + 5):         # the tail's own row tile; every XCD a row tile
            case(_form, _cap, _d0, 36, **feat(n_dev=_nd))
    for _d, _xw in ((36, 64), (44, 36), (48, 20), (52, 100), (60, 36), (64, 64), (4, 36)):
        if (0 < _d % 32 <= 16) != _tail and _stage == 'gru<3,4':
            continue
        _lo = first_cap(_d, _stage)
        if _lo is None or dispatch(_lo, 0, _d) != _form:
            continue                                                          # (d = 4: see above)
        _nxt = STAGES.index(_stage) + 1
        _hi = first_cap(_d, STAGES[_nxt]) - 1 if _nxt < len(STAGES) else _lo + 700
        case(_form, _hi, _d, _xw, **feat(n_dev=2 * _tile + _tile // 2 + 3))     # the last launch of the form at this width
    case(_form, _cap, _d0, 20, **feat(n_dev=_tile + 1))                       # xw < 32
    _skips(_form, _cap, _d0, _tile + 7)
# rows_hint where it changes the pick
case('gru<4,2>', first_cap(20, 'gru<4,1>') + 4000, 20, 36, **feat(rows_hint=first_cap(20, 'gru<4,1>'), n_dev=300))
case('gru<3,4>', first_cap(20, 'gru<4,1>') + 4000, 20, 36, **feat(rows_hint=first_cap(20, 'gru<3,4'), n_dev=300))
case('gru<2,4>', first_cap(64, 'gru<4,1>'), 64, 36, **feat(rows_hint=first_cap(64, 'gru<2,4>'), n_dev=130))

# -- the knob-only forms (32-row blocks), each setting in ONE child process
for _form, _env in (('direct', 'TG_GRU_D16=0'), ('gru<1,4>', 'TG_GRU_D16=0 TG_GRU_DIRECT=0')):
    _row_edges(_form, 200, 20, 36, 32, env=_env)
    for _d, _xw in ((4, 20), (36, 64), (44, 36), (48, 20), (52, 100), (60, 36), (64, 64)):
        case(_form, 300, _d, _xw, **feat(n_dev=32 * 8 + 17, env=_env))         # every XCD a row tile, a ragged last one
    _skips(_form, 100, 20, 39, env=_env)
# the 16 x 16 blocks on a shape they never get otherwise (TG_GRU_D16=3: always): more tiles than any hint would allow
case('direct16<6>', 16000, 44, 36, env='TG_GRU_D16=3', **feat())
case('direct16<3,blend>', 300, 44, 36, env='TG_GRU_D16=3', gather='h', out_rows=True, blend=True, rows_hint=100, out2='add2')

ALL_FORMS = ['direct16<3>', 'direct16<6>', 'direct16<3,blend>', 'direct16<6,blend>', 'direct', 'gru<1,4>', 'gru<2,4>',
             'gru<3,4>', 'gru<3,4,tail16>', 'gru<4,2>', 'gru<4,1>']
KNOB_ONLY = ['direct', 'gru<1,4>']
FAMILIES = ['direct16', 'direct', 'gru']
KNOB_SETTINGS = sorted({c.env for c in CASES if c.env})


def family(form):
    return form.split('<')[0]


# ------------------------------------------------------------------------------------------------------------------
# a case's operands, as they lie in memory
# ------------------------------------------------------------------------------------------------------------------
def live_rows(c):
    return c.cap if c.n_dev is None else max(0, min(c.cap, c.n_dev))


def _acts(rs, kind, rows, cols):
    if kind == 'dyadic':
        return (rs.randint(-8, 9, size=(rows, cols)) / 8.0).astype(np.float32)
    return (rs.standard_normal((rows, cols)) * np.exp(rs.uniform(-2, 2, (rows, 1)))).astype(np.float32)


def _weights(rs, kind, rows, cols, k_total):
    """dyadic: multiples of 1/8 in [-1, 1], about 48 of a row's k_total columns non-zero (pre-activations mostly in
    [-8, 8]); gauss: N(0, 1 / k_total)"""
    if kind == 'dyadic':
        keep = rs.random_sample((rows, cols)) < min(1.0, 48.0 / k_total)
        return (rs.randint(-8, 9, size=(rows, cols)) / 8.0 * keep).astype(np.float32)
    return (rs.standard_normal((rows, cols)) / np.sqrt(k_total)).astype(np.float32)


def _bias(rs, kind, n):
    v = rs.randint(-8, 9, size=n) / 8.0 if kind == 'dyadic' else rs.standard_normal(n)
    return np.concatenate([v, np.full(4, np.nan)]).astype(np.float32)     # a NaN tail behind the last element


def _table(vals, ld, rows_total):
    t = np.full((rows_total, ld), np.nan, dtype=np.float32)
    t[:vals.shape[0], :vals.shape[1]] = vals
    return t


def _index(rs, cap, M, T):
    """row indices into a table of T value rows + one NaN row (tests/_gemm_ref.py: _index): the LAST value row first, a
    descending run with every fifth entry repeating its predecessor, then random rows; dead rows point at the NaN row"""
    idx = np.full(cap, T, dtype=np.int64)
    m = np.arange(M)
    live = (T - 1 - m) % T
    far = m >= 2 * T
    live[far] = rs.randint(0, T, size=int(far.sum()))
    rep = (m % 5 == 4)
    live[rep] = live[np.maximum(m[rep] - 1, 0)]
    idx[:M] = live
    return idx


def build(c, kind, seed=0):
    """the Problem of case `c` with 'dyadic' or 'gauss' data"""
    assert kind in ('dyadic', 'gauss')
    rs = np.random.RandomState((c.cap * 1000003 + c.d * 1009 + c.xw * 31 + len(c.id) + seed * 7919) % (2 ** 31))
    M, d, xw, cap = live_rows(c), c.d, c.xw, c.cap
    p = SimpleNamespace(case=c, kind=kind, cap=cap, M=M, n_dev=c.n_dev, d=d, xw=xw, rows_hint=c.rows_hint,
                        out2_by_row=int(c.out2 in ('by_row', 'by_row_add2')))
    p.skip_at, p.skip_n = c.skip or (0, 0)
    skipped = np.zeros(xw, dtype=bool)
    skipped[p.skip_at * BK:(p.skip_at + p.skip_n) * BK] = True
    p.skipped = skipped
    k_total = int((~skipped).sum()) + d
    T = max(1, min(M, 37))
    shared = _index(rs, cap, M, T) if c.gather else None
    p.x_idx = shared if c.gather in ('x', 'same') else None
    p.h_idx = shared if c.gather in ('h', 'same') else None
    p.x_ld, p.h_ld = xw + c.pad, d + c.pad

    def operand(width, ld, idx):
        if idx is not None:
            return _table(_acts(rs, kind, T, width), ld, T + 1)
        return _table(_acts(rs, kind, M, width), ld, cap)

    p.x = operand(xw, p.x_ld, p.x_idx)
    p.x[:, :xw][:, skipped] = np.nan
    p.h = operand(d, p.h_ld, p.h_idx)
    p.x, p.h = p.x.reshape(-1), p.h.reshape(-1)
    # (the weight columns of skipped tiles hold values: the contract only says that nobody multiplies by them)
    p.w_ih = _table(_weights(rs, kind, 3 * d, xw, k_total), xw, 3 * d + 1).reshape(-1)
    p.w_hh = _table(_weights(rs, kind, 3 * d, d, k_total), d, 3 * d + 1).reshape(-1)
    p.b_ih, p.b_hh = _bias(rs, kind, 3 * d), _bias(rs, kind, 3 * d)
    p.w_blend = p.b_blend = None
    if c.blend:
        p.w_blend = _table(_weights(rs, kind, d, d, 3 * d), d, d + 1).reshape(-1)
        p.b_blend = _bias(rs, kind, d)
    # out: an arena of cap (+ 7 with out_rows) rows of ldo floats between two guard bands
    p.ldo = d + c.ldo_pad
    p.arena_rows = cap + (7 if c.out_rows else 0)
    p.out_rows = rs.permutation(p.arena_rows)[:cap].astype(np.int32) if c.out_rows else None
    p.out = np.full(2 * GUARD + p.arena_rows * p.ldo, np.nan, dtype=np.float32)
    p.gates = np.full(2 * GUARD + cap * 4 * d, np.nan, dtype=np.float32) if c.gates else None
    p.out2 = p.add2 = None
    if c.out2:
        p.out2 = np.full(2 * GUARD + (p.arena_rows if p.out2_by_row else cap) * d, np.nan, dtype=np.float32)
    if c.out2 in ('add2', 'by_row_add2'):   # a per-node table: only the rows live outputs name hold values
        t = np.full((p.arena_rows + 1, d), np.nan, dtype=np.float32)
        t[output_rows(p)] = _acts(rs, kind, M, d) if kind == 'gauss' else (rs.randint(-8, 9, size=(M, d)) / 8.0)
        p.add2 = t.reshape(-1)
    return p


def output_rows(p):
    return (np.arange(p.M) if p.out_rows is None else p.out_rows[:p.M]).astype(np.int64)


def check_problem(p):
    """what the library and the exactness argument need of a Problem (tests/test_gru_ref_host.py runs it on every case)"""
    c = p.case
    assert 0 <= p.M <= p.cap and p.d % 4 == 0 and p.xw % 4 == 0 and p.x_ld % 4 == 0 and p.h_ld % 4 == 0
    assert p.x_ld >= p.xw and p.h_ld >= p.d and p.ldo >= p.d
    if p.skip_n:
        assert (p.skip_at + p.skip_n) * BK <= p.xw and p.skip_n * BK < p.xw
    for tab, ld, w, idx in ((p.x, p.x_ld, p.xw, p.x_idx), (p.h, p.h_ld, p.d, p.h_idx)):
        rows = tab.size // ld
        if idx is None:
            assert rows >= p.cap
            continue
        assert idx.shape == (p.cap,) and idx.min() >= 0 and idx.max() < rows
        if p.M:
            assert (idx[:p.M] < rows - 1).all() and (idx[p.M:] == rows - 1).all(), 'dead entries point at the NaN row'
        if p.M >= 12:
            live = idx[:p.M]
            assert (np.diff(live) < 0).any() and (np.diff(live) == 0).any(), 'descending and repeated entries'
    if c.gather == 'same':
        assert p.x_idx is p.h_idx
    if p.out_rows is not None:
        assert len(np.unique(p.out_rows)) == p.cap and p.out_rows.min() >= 0 and p.out_rows.max() < p.arena_rows
        assert p.cap < 3 or ((np.diff(p.out_rows) < 0).any() and p.ldo >= p.d), 'out_rows is a non-monotone scatter'
    if c.blend:
        assert p.h_idx is not None and p.out_rows is not None and p.gates is None
    if p.kind == 'dyadic':
        # every operand is a multiple of 1/8 in [-1, 1]: products are multiples of 1/64, every partial sum of a plane is a
        # multiple of 1/64 below xw + d + 2 <= 2^18 = 2^24 / 64, so exact in float32 in any order
        assert p.xw + p.d + 2 < 2 ** 18
        for a in (p.x, p.h, p.w_ih, p.w_hh, p.b_ih, p.b_hh, p.w_blend, p.b_blend, p.add2):
            if a is not None:
                f = a[np.isfinite(a)] * 8.0
                assert np.array_equal(f, np.rint(f)) and (np.abs(f) <= 8).all()
    return c


# ------------------------------------------------------------------------------------------------------------------
# reference and bound
# ------------------------------------------------------------------------------------------------------------------
def _sigmoid(x):
    return np.where(x >= 0, 1.0 / (1.0 + np.exp(-np.abs(x))), np.exp(-np.abs(x)) / (1.0 + np.exp(-np.abs(x))))


def e_sig(x):
    """the allowance of fast_sigmoid at pre-activation x (module docstring)"""
    s = _sigmoid(x)
    return SLACK * s * ((1.0 - s) * (1.25 * np.abs(x) + 2.0) + 3.0) * U24 + FLUSH


def e_tanh(x):
    """the allowance of fast_tanh at pre-activation x (module docstring)"""
    t = np.tanh(np.abs(x))
    return SLACK * ((1.0 - t * t) / 2.0 * (2.5 * np.abs(x) + 2.0) + 5.0 * t) * U24 + FLUSH


def _gathered(p, tab, ld, w, idx):
    r = np.arange(p.M) if idx is None else idx[:p.M]
    return tab.reshape(-1, ld)[r, :w].astype(np.float64)


def reference(p):
    """the contract's values in float64 and their allowances: out / d_out [M, d], gates / d_gates [M, 4, d] (r, z, n,
    h_n), out2 / d_out2 [M, d] (None without out2), and pre_in = i_n + b_in for the isolation of the n plane"""
    d, xw, M = p.d, p.xw, p.M
    X = _gathered(p, p.x, p.x_ld, xw, p.x_idx)
    H = _gathered(p, p.h, p.h_ld, d, p.h_idx)
    Wi = p.w_ih.reshape(-1, xw)[:3 * d].astype(np.float64)
    X[:, p.skipped] = 0.0
    Wh = p.w_hh.reshape(-1, d)[:3 * d].astype(np.float64)
    bi, bh = p.b_ih[:3 * d].astype(np.float64), p.b_hh[:3 * d].astype(np.float64)
    exact = p.kind == 'dyadic'
    kx = int((~p.skipped).sum())
    gi, gh = X @ Wi.T, H @ Wh.T
    mi, mh = np.abs(X) @ np.abs(Wi).T, np.abs(H) @ np.abs(Wh).T
    sl = lambda a, q: a[..., q * d:(q + 1) * d]

    def eps(k, mag):
        return np.zeros_like(mag) if exact else (k + 6) * U24 * mag

    a_r = sl(gi, 0) + sl(gh, 0) + sl(bi, 0) + sl(bh, 0)
    a_z = sl(gi, 1) + sl(gh, 1) + sl(bi, 1) + sl(bh, 1)
    e_r = eps(kx + d, sl(mi, 0) + sl(mh, 0) + np.abs(sl(bi, 0)) + np.abs(sl(bh, 0)))
    e_z = eps(kx + d, sl(mi, 1) + sl(mh, 1) + np.abs(sl(bi, 1)) + np.abs(sl(bh, 1)))
    pre_in = sl(gi, 2) + sl(bi, 2)
    e_in = eps(kx, sl(mi, 2) + np.abs(sl(bi, 2)))
    hn = sl(gh, 2) + sl(bh, 2)
    e_hn = eps(d, sl(mh, 2) + np.abs(sl(bh, 2)))
    r, z = _sigmoid(a_r), _sigmoid(a_z)
    D_r, D_z = e_r / 4.0 + e_sig(a_r), e_z / 4.0 + e_sig(a_z)
    pn = pre_in + r * hn
    D_p = e_in + np.abs(r) * e_hn + np.abs(hn) * D_r + U24 * np.abs(r * hn) + U24 * np.abs(pn)
    n = np.tanh(pn)
    D_n = SLACK * D_p + e_tanh(pn)
    if p.w_blend is not None:
        Wb = p.w_blend.reshape(-1, d)[:d].astype(np.float64)
        bb = p.b_blend[:d].astype(np.float64)
        hb = H @ Wb.T + bb
        e_hb = eps(d, np.abs(H) @ np.abs(Wb).T + np.abs(bb))
    else:
        hb, e_hb = H, np.zeros_like(H)
    v = (1.0 - z) * n + z * hb
    D_v = SLACK * (np.abs(hb - n) * D_z + U24 * np.abs(1.0 - z) * np.abs(n) + np.abs(1.0 - z) * D_n + U24 * np.abs((1.0 - z) * n) +
                   z * e_hb + U24 * np.abs(z * hb) + U24 * np.abs(v))
    ref = SimpleNamespace(out=v, d_out=D_v, gates=np.stack([r, z, n, hn], axis=1),
                          d_gates=np.stack([D_r, D_z, D_n, e_hn], axis=1), pre_in=pre_in, out2=None, d_out2=None)
    if p.out2 is not None:
        ref.out2, ref.d_out2 = v, D_v
        if p.add2 is not None:
            add = p.add2.reshape(-1, d)[output_rows(p)].astype(np.float64)
            ref.out2, ref.d_out2 = v + add, D_v + SLACK * U24 * np.abs(v + add)
    return ref


# ------------------------------------------------------------------------------------------------------------------
# comparator
# ------------------------------------------------------------------------------------------------------------------
def positions(p):
    """flat arena positions of the live outputs: out [M, d], out2 [M, d] or None, gates [M, 4, d] or None"""
    j = np.arange(p.d, dtype=np.int64)
    orow, m = output_rows(p), np.arange(p.M, dtype=np.int64)
    out = GUARD + orow[:, None] * p.ldo + j[None, :]
    out2 = GUARD + (orow if p.out2_by_row else m)[:, None] * p.d + j[None, :] if p.out2 is not None else None
    gates = (GUARD + m[:, None, None] * 4 * p.d + np.arange(4, dtype=np.int64)[None, :, None] * p.d + j[None, None, :]
             if p.gates is not None else None)
    return out, out2, gates


def _untouched(p, name, before, after, pos):
    assert after.shape == before.shape and after.dtype == np.float32
    keep = np.ones(after.size, dtype=bool)
    keep[pos.reshape(-1)] = False
    assert after.size - int(keep.sum()) == pos.size, 'two outputs share an address: the case is wrong'
    same = after.view(np.int32)[keep] == before.view(np.int32)[keep]
    if not same.all():
        where = np.flatnonzero(keep)[~same]
        raise AssertionError(f'{p.case.id}: {len(where)} floats of `{name}` outside the outputs were written, first at arena '
                             f'offsets {where[:6].tolist()} (rows start at {GUARD})')


def _within(p, name, got, want, bound):
    bad = np.argwhere(~np.isfinite(got))
    assert bad.size == 0, (p.case.id, name, 'non-finite outputs', len(bad), bad[:6].tolist())
    err = np.abs(got.astype(np.float64) - want)
    frac = float((err / np.maximum(bound, np.finfo(np.float64).tiny)).max()) if err.size else 0.0
    over = np.argwhere(err > bound)
    assert over.size == 0, (p.case.id, name, 'fraction of the allowance', frac, len(over), over[:6].tolist())
    return frac


def compare(p, ref, out, out2=None, gates=None):
    """the three arenas after the call.  Everything but the live outputs keeps its bits; every live output is finite and
    within its allowance.  Returns the worst observed fractions: 'out' (out and out2), 'gates' (the general bound of the
    saved r, z, n), and on dyadic data with gates 'sigmoid' and 'tanh' (the function-evaluation allowances alone)."""
    po, po2, pg = positions(p)
    worst = {}
    _untouched(p, 'out', p.out, out, po)
    worst['out'] = _within(p, 'out', out[po], ref.out, ref.d_out)
    assert (out2 is None) == (p.out2 is None) and (gates is None) == (p.gates is None)
    if out2 is not None:
        _untouched(p, 'out2', p.out2, out2, po2)
        worst['out'] = max(worst['out'], _within(p, 'out2', out2[po2], ref.out2, ref.d_out2))
    if gates is not None:
        _untouched(p, 'gates', p.gates, gates, pg)
        g = gates[pg]
        worst['gates'] = _within(p, 'gates r, z, n', g[:, :3], ref.gates[:, :3], ref.d_gates[:, :3])
        if p.kind == 'dyadic':
            want = ref.gates[:, 3].astype(np.float32)
            assert np.array_equal(want.astype(np.float64), ref.gates[:, 3]), 'h_n is not representable: the case is wrong'
            bad = np.argwhere(g[:, 3] != want)
            assert bad.size == 0, (p.case.id, 'the saved h_n plane is exact on dyadic data', len(bad), bad[:6].tolist())
            worst['sigmoid'] = worst['gates'] if not p.M else max(
                _within(p, 'r (sigmoid alone)', g[:, 0], ref.gates[:, 0], ref.d_gates[:, 0]),
                _within(p, 'z (sigmoid alone)', g[:, 1], ref.gates[:, 1], ref.d_gates[:, 1]))
            r_dev, hn = g[:, 0].astype(np.float64), ref.gates[:, 3]
            pn = ref.pre_in + r_dev * hn
            allow = SLACK * U24 * (np.abs(ref.pre_in) + np.abs(r_dev * hn) + np.abs(pn)) + e_tanh(pn)
            worst['tanh'] = _within(p, 'n (tanh alone, from the saved r)', g[:, 2], np.tanh(pn), allow)
        else:
            _within(p, 'gates h_n', g[:, 3], ref.gates[:, 3], np.maximum(ref.d_gates[:, 3], 0.0))
    return worst


def passing(p, ref):
    """the three arenas as a correct kernel leaves them (the reference rounded to float32)"""
    po, po2, pg = positions(p)
    out = p.out.copy()
    out[po] = ref.out.astype(np.float32)
    out2 = gates = None
    if p.out2 is not None:
        out2 = p.out2.copy()
        out2[po2] = ref.out2.astype(np.float32)
    if p.gates is not None:
        gates = p.gates.copy()
        gates[pg] = ref.gates.astype(np.float32)
    return out, out2, gates
