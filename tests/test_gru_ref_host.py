"""tests/_gru_ref.py without a GPU: the float64 reference of the GruArgs contract against torch.nn.GRUCell and against the
blend identity, the exactness of the dyadic data, the comparator against results that must not pass, the case table and
the mirror of the dispatcher, and tg_debug_gru's argument checks (they run before anything touches the GPU)."""
import copy
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _gru_ref as R


def tiny(**feat):
    c = SimpleNamespace(form=None, cap=feat.pop('cap', 9), d=feat.pop('d', 12), xw=feat.pop('xw', 40), **{**R.DEFAULTS, **feat})
    c.id = f'tiny{c.cap}x{c.d}x{c.xw}' + ''.join(f'-{k}={v}' if not isinstance(v, bool) else f'-{k}' for k, v in feat.items())
    return c


PLAIN = [tiny(), tiny(gather='x'), tiny(gather='h', pad=4), tiny(gather='same', out_rows=True, ldo_pad=4), tiny(n_dev=5),
         tiny(n_dev=0), tiny(n_dev=30), tiny(d=4, xw=4), tiny(cap=40, d=20, xw=36, gather='same', n_dev=33, pad=8)]


def _torch_cell(p, zero_skipped=True):
    """torch.nn.GRUCell in float64 on the case's gathered rows: (new h [M, d], r, z, n, h_n)"""
    d, xw = p.d, p.xw
    X = R._gathered(p, p.x, p.x_ld, xw, p.x_idx)
    X[:, p.skipped] = 0.0
    H = R._gathered(p, p.h, p.h_ld, d, p.h_idx)
    cell = torch.nn.GRUCell(xw, d).double()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    with torch.no_grad():
        cell.weight_ih.copy_(t(p.w_ih.reshape(-1, xw)[:3 * d]))
        cell.weight_hh.copy_(t(p.w_hh.reshape(-1, d)[:3 * d]))
        cell.bias_ih.copy_(t(p.b_ih[:3 * d]))
        cell.bias_hh.copy_(t(p.b_hh[:3 * d]))
        return cell(t(X), t(H)).numpy() if p.M else np.zeros((0, d))


@pytest.mark.parametrize('kind', ['dyadic', 'gauss'])
@pytest.mark.parametrize('c', PLAIN, ids=[c.id for c in PLAIN])
def test_reference_is_torch_grucell_in_float64(c, kind):
    p = R.build(c, kind)
    R.check_problem(p)
    ref = R.reference(p)
    np.testing.assert_allclose(ref.out, _torch_cell(p), rtol=1e-12, atol=1e-13)
    assert ref.out.shape == (p.M, p.d) and ref.gates.shape == (p.M, 4, p.d) and (ref.d_out > 0).all()
    # the comparator accepts the reference itself, rounded to float32
    worst = R.compare(p, ref, *R.passing(p, ref))
    assert all(v <= 1.0 for v in worst.values()), worst


@pytest.mark.parametrize('c', [tiny(skip=(0, 1)), tiny(xw=100, skip=(1, 2), gather='x'), tiny(xw=100, skip=(0, 3), gates=True)],
                         ids=lambda c: c.id)
def test_reference_takes_skipped_tiles_as_zero(c):
    p = R.build(c, 'gauss')
    R.check_problem(p)
    assert np.isnan(p.x.reshape(-1, p.x_ld)[0, p.skip_at * 32]) and np.isfinite(p.w_ih.reshape(-1, p.xw)[:3 * p.d]).all()
    np.testing.assert_allclose(R.reference(p).out, _torch_cell(p), rtol=1e-12, atol=1e-13)


def test_reference_second_output_and_gate_planes():
    """out2 dense / by output row, add2 by the OUTPUT row; gates [cap, 4, d] = r, z, n, h_n + b_hn - one scalar at a time"""
    for out2 in R.OUT2[1:]:
        c = tiny(gather='h', out_rows=True, out2=out2, gates=True, n_dev=7, ldo_pad=4)
        p = R.build(c, 'gauss')
        R.check_problem(p)
        ref = R.reference(p)
        out, o2, gates = R.passing(p, ref)
        d = p.d
        f8 = np.float64
        for m in range(p.M):
            o = int(p.out_rows[m])
            xr = p.x.reshape(-1, p.x_ld)[m, :p.xw].astype(f8)
            hr = p.h.reshape(-1, p.h_ld)[int(p.h_idx[m]), :d].astype(f8)
            wi, wh = p.w_ih.reshape(-1, p.xw).astype(f8), p.w_hh.reshape(-1, d).astype(f8)
            for j in range(d):
                sg = lambda v: 1.0 / (1.0 + np.exp(-v))
                r = sg(wi[j] @ xr + p.b_ih[j] + wh[j] @ hr + p.b_hh[j])
                z = sg(wi[d + j] @ xr + p.b_ih[d + j] + wh[d + j] @ hr + p.b_hh[d + j])
                hn = wh[2 * d + j] @ hr + f8(p.b_hh[2 * d + j])
                n = np.tanh(wi[2 * d + j] @ xr + p.b_ih[2 * d + j] + r * hn)
                v = (1 - z) * n + z * hr[j]
                assert abs(out[R.GUARD + o * p.ldo + j] - v) < 1e-6
                g = gates[R.GUARD + m * 4 * d + j:][:4 * d:d]
                np.testing.assert_allclose(g, [r, z, n, hn], rtol=1e-6, atol=1e-6)
                add = f8(p.add2[o * d + j]) if 'add2' in out2 else 0.0
                assert np.isfinite(add)
                assert abs(o2[R.GUARD + (o if 'by_row' in out2 else m) * d + j] - (v + add)) < 1e-6
        assert np.isnan(out).sum() == out.size - p.M * d and np.isnan(gates).sum() == gates.size - p.M * 4 * d


def test_reference_blend_form_is_the_cell_on_the_affine_image():
    """tests/test_hip_fc2_deferred.py's identity: with w_hh = W_hh W2 and b_hh = W_hh b2 + b_hh handed in, the blend form on t
    is the plain cell on h = W2 t + b2 (integer-valued weights: the fold is exact in float32)"""
    c = tiny(cap=11, d=8, xw=12, gather='h', out_rows=True, blend=True, out2='add2')
    p = R.build(c, 'gauss')
    rs = np.random.RandomState(5)
    d = p.d
    W_hh, W2 = rs.randint(-2, 3, (3 * d, d)).astype(np.float64), rs.randint(-2, 3, (d, d)).astype(np.float64)
    b_hh, b2 = rs.randint(-2, 3, 3 * d).astype(np.float64), rs.randint(-2, 3, d).astype(np.float64)
    p.w_blend[:d * d], p.b_blend[:d] = W2.reshape(-1), b2
    p.w_hh[:3 * d * d], p.b_hh[:3 * d] = (W_hh @ W2).reshape(-1), W_hh @ b2 + b_hh
    ref = R.reference(p)
    T = p.h.reshape(-1, p.h_ld)[p.h_idx[:p.M], :d].astype(np.float64)
    h64 = T @ W2.T + b2
    X = R._gathered(p, p.x, p.x_ld, p.xw, p.x_idx)
    Wi, bi = p.w_ih.reshape(-1, p.xw)[:3 * d].astype(np.float64), p.b_ih[:3 * d].astype(np.float64)
    gi, gh = X @ Wi.T + bi, h64 @ W_hh.T + b_hh
    sg = lambda v: 1.0 / (1.0 + np.exp(-v))
    r, z = sg(gi[:, :d] + gh[:, :d]), sg(gi[:, d:2 * d] + gh[:, d:2 * d])
    want = (1 - z) * np.tanh(gi[:, 2 * d:] + r * gh[:, 2 * d:]) + z * h64
    np.testing.assert_allclose(ref.out, want, rtol=1e-12, atol=1e-12)
    assert ref.out2 is not None


@pytest.mark.parametrize('c', [R.CASES[1], tiny(cap=50, d=44, xw=164, skip=(1, 3)),
                               tiny(cap=20, d=36, xw=64, gather='h', out_rows=True, blend=True)], ids=lambda c: c.id)
def test_dyadic_data_is_exact_in_any_order(c):
    """float32 sums of the products of a pre-activation, in several random orders and splits, are identical and equal the
    float64 value"""
    p = R.build(c, 'dyadic')
    R.check_problem(p)
    ref = R.reference(p)
    d, rs = p.d, np.random.RandomState(3)
    X = R._gathered(p, p.x, p.x_ld, p.xw, p.x_idx).astype(np.float32)
    X[:, p.skipped] = 0
    H = R._gathered(p, p.h, p.h_ld, d, p.h_idx).astype(np.float32)
    Wi, Wh = p.w_ih.reshape(-1, p.xw)[:3 * d], p.w_hh.reshape(-1, d)[:3 * d]
    for m in range(min(p.M, 3)):
        for j in (0, d - 1):
            terms = (H[m] * Wh[2 * d + j]).astype(np.float32)   # h_n
            full = np.concatenate([X[m] * Wi[j], H[m] * Wh[j], p.b_ih[j:j + 1], p.b_hh[j:j + 1]]).astype(np.float32)   # r
            for t, want in ((terms, ref.gates[m, 3, j] - np.float64(p.b_hh[2 * d + j])), (full, None)):
                sums = set()
                for _ in range(6):
                    acc = np.float32(0)
                    for v in rs.permutation(t):
                        acc = np.float32(acc + v)
                    halves = np.float32(np.float32(t[::2].sum(dtype=np.float32)) + np.float32(t[1::2].sum(dtype=np.float32)))
                    sums |= {float(acc), float(halves)}
                assert len(sums) == 1
                assert want is None or sums == {float(want)}
    if p.w_blend is not None:   # the rebuilt h is exact too: the blend input
        hb = H.astype(np.float64) @ p.w_blend.reshape(-1, d)[:d].astype(np.float64).T + p.b_blend[:d]
        assert np.array_equal(hb.astype(np.float32).astype(np.float64), hb) and (np.abs(hb * 64) == np.rint(np.abs(hb * 64))).all()


REJECT = [tiny(cap=37, d=20, xw=100, gather='h', out_rows=True, ldo_pad=4, n_dev=33, gates=True, out2='add2', skip=(1, 1)),
          tiny(cap=37, d=20, xw=100, gather='same', out_rows=True, ldo_pad=4, n_dev=33, gates=True, out2='by_row_add2', skip=(0, 1))]


@pytest.mark.parametrize('kind', ['dyadic', 'gauss'])
@pytest.mark.parametrize('c', REJECT, ids=[c.id for c in REJECT])
def test_comparator_rejects_planted_faults(c, kind):
    p = R.build(c, kind)
    ref = R.reference(p)
    out, out2, gates = R.passing(p, ref)
    R.compare(p, ref, out, out2, gates)
    po, po2, pg = R.positions(p)
    m, j = p.M - 1, p.d - 1

    def rejected(o=out, o2=out2, g=gates, match=None):
        with pytest.raises(AssertionError, match=match):
            R.compare(p, ref, o, o2, g)

    # one element at twice its bound, in each arena
    for arena, pos, want, bound in ((out, po[m, j], ref.out[m, j], ref.d_out[m, j]), (out2, po2[m, j], ref.out2[m, j], ref.d_out2[m, j]),
                                    (gates, pg[m, 0, j], ref.gates[m, 0, j], ref.d_gates[m, 0, j]),
                                    (gates, pg[m, 2, j], ref.gates[m, 2, j], ref.d_gates[m, 2, j])):
        bad = arena.copy()
        bad[pos] = np.float32(want + 2.0 * bound + 2 * np.spacing(np.float32(want)))
        rejected(**{('o' if arena is out else 'o2' if arena is out2 else 'g'): bad})
    # two gate planes swapped: r <-> z, and n <-> h_n
    for a, b in ((0, 1), (2, 3)):
        bad = gates.copy()
        bad[pg[:, a]], bad[pg[:, b]] = gates[pg[:, b]], gates[pg[:, a]]
        rejected(g=bad)
    # add2 taken by launch row instead of output row
    add = p.add2.reshape(-1, p.d)
    bad = out2.copy()
    bad[po2] = (ref.out + np.nan_to_num(add[:p.M].astype(np.float64), nan=0.5)).astype(np.float32)
    rejected(o2=bad)
    # a skipped tile shifted by one: the kernel multiplies what lies in the zero tile and skips a tile that counts
    q = copy.copy(p)
    q.x = p.x.copy()
    xt = q.x.reshape(-1, p.x_ld)
    finite_rows = np.isfinite(xt[:, 0]) | np.isfinite(xt[:, p.xw - 1])
    lo = p.skip_at * 32
    xt[finite_rows, lo:lo + 32] = (np.random.RandomState(1).randint(1, 9, size=(int(finite_rows.sum()), 32)) / 8.0)
    q.skipped = np.roll(p.skipped, 32)
    shifted = R.reference(q)
    rejected(*R.passing(p, shifted))
    # a store at row *n_dev; a changed guard word; a write in column d of `out` (ldo > d); an output never written
    for arena, pos, key in ((out, R.GUARD + int(p.out_rows[p.M]) * p.ldo, 'o'), (gates, R.GUARD + p.M * 4 * p.d, 'g'),
                            (out2, R.GUARD + (int(p.out_rows[p.M]) if p.out2_by_row else p.M) * p.d, 'o2')):
        bad = arena.copy()
        bad[pos] = 1.0
        rejected(**{key: bad}, match='outside the outputs')
        for at in (0, R.GUARD - 1, arena.size - R.GUARD, arena.size - 1):
            bad = arena.copy()
            bad.view(np.int32)[at] ^= 1
            rejected(**{key: bad}, match='outside the outputs')
    assert p.ldo > p.d
    bad = out.copy()
    bad[po[0, p.d - 1] + 1] = 0.0
    rejected(o=bad, match='outside the outputs')
    bad = out.copy()
    bad[po[0, 0]] = np.nan
    rejected(o=bad, match='non-finite')
    if kind == 'dyadic':   # the exact plane, one unit in the last place off
        bad = gates.copy()
        bad[pg[m, 3, j]] = np.nextafter(bad[pg[m, 3, j]], np.float32(np.inf))
        rejected(g=bad, match='h_n')


def test_function_allowances_cover_a_float32_model_of_the_code():
    """fast_sigmoid / fast_tanh restated in numpy float32 with correctly rounded exp2 and division (no worse than the 1 ulp
    premise): within the allowances, which in turn stay within a few units of 2^-24 of the issue's estimate"""
    f32 = np.float32
    x = np.concatenate([np.linspace(-30, 30, 20001), np.random.RandomState(0).standard_normal(20000) * 4]).astype(f32)
    L = f32(float.fromhex('0x1.715476p+0'))
    ex = lambda y: np.exp2((L * y.astype(f32)).astype(np.float64)).astype(f32)
    sig = (f32(1) / (f32(1) + ex(-x))).astype(f32)
    e = ex(f32(-2) * np.abs(x))
    th = np.copysign(((f32(1) - e) * (f32(1) / (f32(1) + e))).astype(f32), x)
    x8 = x.astype(np.float64)
    assert (np.abs(sig - R._sigmoid(x8)) <= R.e_sig(x8)).all()
    assert (np.abs(th - np.tanh(x8)) <= R.e_tanh(x8)).all()
    assert (R.e_sig(x8) <= (2 * np.abs(x8) + 5) * R.U24).all() and (R.e_tanh(x8) <= (2 * np.abs(x8) + 6) * R.U24).all()


def test_case_table_names_every_form_and_the_mirror_agrees():
    ids = [c.id for c in R.CASES]
    assert len(ids) == len(set(ids))
    assert {c.form for c in R.CASES} == set(R.ALL_FORMS), {c.form for c in R.CASES} ^ set(R.ALL_FORMS)
    for c in R.CASES:
        assert R.expected_form(c) == c.form, (c.id, R.expected_form(c))
        assert set(R.env_of(c)) <= set(R.KNOBS)
        if c.form in R.KNOB_ONLY:
            assert c.env, 'a knob-only form needs its setting'
            assert R.dispatch(c.cap, c.rows_hint, c.d) not in R.KNOB_ONLY
    for form in R.ALL_FORMS:   # *n_dev = 0 for every form but the large blend instance (same kernel text as the small one)
        assert form == 'direct16<6,blend>' or any(c.form == form and c.n_dev == 0 for c in R.CASES), form
    assert len(R.KNOB_SETTINGS) <= 3


def test_knob_only_forms_by_enumeration():
    """`micro` implies the 16 x 16 condition: without a knob gru_launch never reaches k_gru_direct / k_gru<1, 4>"""
    for d in list(range(4, 260, 4)) + [300, 512, 1000, 1024, 1028, 1280, 1284, 2048]:
        for rows in range(1, 10240 // R.cdiv(d, 32) + 400, 16):   # (`micro` needs rows <= 10 240 / NT)
            for r in (rows - 1, rows, rows + 1):
                if r > 0:
                    assert R.dispatch(r, 0, d) not in R.KNOB_ONLY and R.dispatch(1 << 20, r, d) not in R.KNOB_ONLY
    assert R.dispatch(200, 0, 20, env={'TG_GRU_D16': '0'}) == 'direct'
    assert R.dispatch(200, 0, 20, env={'TG_GRU_D16': '0', 'TG_GRU_DIRECT': '0'}) == 'gru<1,4>'


def test_direct16_cases_pick_every_block_height():
    """k_gru_direct16 picks 16 / 32 / 48 / 64 / 96-row blocks from the live count: every choice of both instances is a case,
    the large instance also on few live rows, past one round of the largest blocks, and on a grid below 256 blocks"""
    seen = {(3, rt): 0 for rt in (1, 2, 3)}
    seen.update({(6, rt): 0 for rt in (1, 2, 3, 4, 6)})
    for c in R.CASES:
        if c.form in ('direct16<3>', 'direct16<6>') and R.live_rows(c):
            rtm = int(c.form[9])
            seen[rtm, R.direct16_rt(R.live_rows(c), c.d, rtm)] += 1
    assert all(seen.values()), seen
    d16 = [c for c in R.CASES if c.form.startswith('direct16') and not c.env]
    assert any(R.cdiv(R.live_rows(c), 96) * R.cdiv(c.d, 16) > 256 for c in d16 if c.form == 'direct16<6>')
    assert any(R.cdiv(R.live_rows(c), 48) * R.cdiv(c.d, 16) > 256 for c in d16 if c.form == 'direct16<3>')
    assert any(R.cdiv(c.cap, 16) * R.cdiv(c.d, 16) < 248 for c in d16)
    assert any(c.form == 'direct16<6>' and c.cap >= 50000 and R.live_rows(c) < 100 for c in d16)


@pytest.mark.parametrize('c', R.CASES, ids=[c.id for c in R.CASES])
def test_case_table(c):
    for kind in ('dyadic', 'gauss'):
        p = R.build(c, kind)
        R.check_problem(p)
        assert sum(a.nbytes for a in (p.x, p.h, p.out, p.out2, p.gates, p.add2) if a is not None) <= (64 << 20)
    assert 2.0 * R.live_rows(c) * 3 * c.d * (c.xw + c.d) <= 1.0e9   # the reference stays cheap


def test_debug_gru_refuses_bad_arguments_before_any_device_call():
    """the pointers are host arrays that are never dereferenced: every refusal comes before the first HIP call"""
    from www2023tiger_amd import _lib
    lib, ptr = _lib.lib, _lib.ptr
    d, xw, n = 8, 40, 4
    x, h, out = np.zeros((n, xw), np.float32), np.zeros((n, d), np.float32), np.zeros((n, d), np.float32)
    w_ih, w_hh, b = np.zeros((3 * d, xw), np.float32), np.zeros((3 * d, d), np.float32), np.zeros(3 * d, np.float32)
    o2, wb, gates = np.zeros((n, d), np.float32), np.zeros((d, d), np.float32), np.zeros((n, 4, d), np.float32)
    form = C.c_char_p(b'unset')

    def call(**kw):
        f = dict(cap=n, d=d, xw=xw, x=ptr(x), x_ld=xw, x_w=xw, h=ptr(h), h_ld=d, h_w=d, w_ih=ptr(w_ih), w_hh=ptr(w_hh),
                 b_ih=ptr(b), b_hh=ptr(b), out=ptr(out), ldo=d)
        f.update(kw)
        return lib.tg_debug_gru(C.byref(_lib.TgGruProbe(**f)), C.byref(form), None)

    assert lib.tg_debug_gru(None, C.byref(form), None) == _lib.TG_EINVAL
    for field in ('x', 'h', 'w_ih', 'w_hh', 'b_ih', 'b_hh', 'out'):
        assert call(**{field: None}) == _lib.TG_EINVAL, field
    for bad in (dict(d=0, h_w=0), dict(d=6, h_w=6), dict(d=-4, h_w=-4), dict(xw=0, x_w=0), dict(xw=42, x_w=42, x_ld=44),
                dict(x_w=36), dict(h_w=4), dict(x_ld=36), dict(x_ld=42), dict(h_ld=4), dict(h_ld=10), dict(ldo=4),
                dict(cap=-1), dict(rows_hint=-1)):
        assert call(**bad) == _lib.TG_EINVAL, bad
    # a skipped run outside the message's whole k-tiles (xw = 40: one whole tile), or one that leaves nothing
    for bad in (dict(x_skip_at=-1, x_skip_n=1), dict(x_skip_n=-1), dict(x_skip_at=1, x_skip_n=1), dict(x_skip_at=0, x_skip_n=2),
                dict(xw=32, x_w=32, x_ld=32, x_skip_at=0, x_skip_n=1)):
        assert call(**bad) == _lib.TG_EINVAL, bad
    assert call(out2_by_row=1) == _lib.TG_EINVAL
    assert call(add2=ptr(o2)) == _lib.TG_EINVAL
    # the dispatcher's own refusals: the blend form with gates, without its bias, or where the 16 x 16 kernel does not apply
    assert call(w_blend=ptr(wb), b_blend=ptr(b), gates=ptr(gates)) == _lib.TG_EUNSUPPORTED
    assert call(w_blend=ptr(wb)) == _lib.TG_EUNSUPPORTED
    assert call(w_blend=ptr(wb), b_blend=ptr(b), cap=1 << 20) == _lib.TG_EUNSUPPORTED
    assert R.dispatch(1 << 20, 0, d, blend=True) == 'unsupported' and R.dispatch(n, 0, d, blend=True, gates=True) == 'unsupported'
    assert form.value is None                                    # a refusal names no kernel
    assert call(cap=0) == _lib.TG_OK and form.value is None      # nothing to do: nothing is launched
    assert call(cap=0, out2=ptr(o2), add2=ptr(o2), x_skip_at=0, x_skip_n=1) == _lib.TG_OK
    assert not out.any() and not o2.any() and not gates.any()
