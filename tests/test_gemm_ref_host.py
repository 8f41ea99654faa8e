"""tests/_gemm_ref.py without a GPU: the float64 reference of the GemmArgs contract against a plain triple loop over the
flat operands, the case table of tests/test_hip_gemm_forms.py against what the library and the exactness argument need,
the comparator against results that must not pass, and tg_debug_gemm's argument checks (they run before anything
touches the GPU)."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import _gemm_ref as R


def tiny(**feat):
    c = SimpleNamespace(form=None, m_cap=feat.pop('m_cap', 5), n=feat.pop('n', 8), k=feat.pop('k', 12), **{**R.DEFAULTS, **feat})
    c.id = f'tiny{c.m_cap}x{c.n}x{c.k}' + ''.join(f'-{k}={v}' if not isinstance(v, bool) else f'-{k}' for k, v in feat.items())
    return c


TINY = [
    tiny(), tiny(idx=True), tiny(a_pad=4), tiny(a1_w=4), tiny(a1_w=8, idx1=True), tiny(a1_w=4, idx=True, idx1=True, a_pad=8),
    tiny(m_dev=3), tiny(m_dev=0), tiny(m_dev=9), tiny(m_dev=3, m_hint=2), tiny(c_rows=True), tiny(c_rows=True, idx=True, m_dev=4),
    tiny(alpha=0.5), tiny(alpha=-2.0, relu=1), tiny(relu=1), tiny(c_pad=3), tiny(w_pad=8), tiny(bias=False),
    tiny(bias2=True), tiny(bias_rs=True), tiny(row_valid=True), tiny(relu_mask=True), tiny(accumulate=True),
    tiny(w_kmajor=True), tiny(w_kmajor=True, w_pad=8, n=4), tiny(nbatch=3), tiny(nbatch=4, n=3, c_pad=5),
    # the combinations of the case table
    tiny(relu_mask=True, accumulate=True, w_kmajor=True, bias=False), tiny(bias_rs=True, nbatch=3, n=3),
    tiny(bias_rs=True, nbatch=4, n=3, idx=True, relu=1), tiny(row_valid=True, c_rows=True, m_dev=4, idx=True),
    tiny(bias2=True, a1_w=4, idx1=True, alpha=-2.0), tiny(accumulate=True, c_rows=True, alpha=0.5),
    tiny(a1_w=8, idx=True, idx1=True, bias2=True, relu=1), tiny(a1_w=4, bias2=True, c_rows=True, idx1=True, c_pad=4),
    tiny(idx=True, c_rows=True, alpha=-2.0, relu=1, c_pad=4, a_pad=8, w_pad=8), tiny(w_kmajor=True, relu_mask=True),
]


def triple_loop(p):
    """the contract, one scalar at a time over the flat arrays, exactly as include/tiger_hip.h words it; returns the whole
    arena as float64"""
    out = p.arena.astype(np.float64)
    M = p.m_cap if p.m_dev is None else min(p.m_cap, p.m_dev)
    for z in range(p.nbatch):
        for m in range(M):
            r0 = m if p.idx0 is None else int(p.idx0[m])
            r1 = m if p.idx1 is None else int(p.idx1[m])
            for n in range(p.n):
                acc = 0.0
                for kk in range(p.k):
                    if kk < p.a0_w:
                        a = p.a0[p.a0_off + z * p.a0_bs + r0 * p.a0_ld + kk]
                    else:
                        a = p.a1[p.a1_off + r1 * p.a1_ld + (kk - p.a0_w)]
                    w = p.w[p.w_off + z * p.w_bs + (kk * p.ldw + n if p.w_kmajor else n * p.ldw + kk)]
                    acc += float(a) * float(w)
                be = 0.0
                if p.bias is not None:
                    be = float(p.bias[z * p.bias_bs + n])
                    if p.bias_rs is not None:
                        be *= float(p.bias_rs[m * p.ld_brs + z])
                if p.bias2 is not None and p.bias2_valid[m]:
                    be += float(p.bias2[n])
                v = p.alpha * (acc + be)
                if p.relu:
                    v = max(v, 0.0)
                if p.row_valid is not None and not p.row_valid[m]:
                    v = 0.0
                if p.relu_mask is not None and not p.relu_mask[m * p.ld_mask + n] > 0:
                    v = 0.0
                at = p.c_off + z * p.c_bs + (m if p.c_rows is None else int(p.c_rows[m])) * p.ldc + n
                if p.accumulate:
                    v += float(p.arena[at])
                out[at] = v
    return out


@pytest.mark.parametrize('kind', ['int', 'gauss'])
@pytest.mark.parametrize('c', TINY, ids=[c.id for c in TINY])
def test_reference_is_the_triple_loop(c, kind):
    p = R.build(c, kind)
    R.check_problem(p)
    want = triple_loop(p)
    ref, mag = R.reference(p)
    have = p.arena.astype(np.float64)
    have[R.output_positions(p)] = ref
    written = np.zeros(have.size, dtype=bool)
    written[R.output_positions(p).reshape(-1)] = True
    assert np.array_equal(np.isnan(want), np.isnan(have))
    assert np.isfinite(have[written]).all()
    if kind == 'int':
        assert np.array_equal(want[written], have[written])
    else:
        np.testing.assert_allclose(have[written], want[written], rtol=1e-12, atol=1e-12)
    assert np.array_equal(want[~written], p.arena.astype(np.float64)[~written], equal_nan=True)
    assert (mag >= np.abs(ref) - 1e-9).all()
    # and the comparator accepts the reference itself
    after = p.arena.copy()
    after[R.output_positions(p)] = ref.astype(np.float32)
    assert R.compare(p, ref, mag, after) <= 1.0 / (p.k + 4)   # (one rounding of the result: at most 2^-24 |ref| <= 2^-24 mag)


def test_case_ids_are_unique_and_every_form_is_expected_somewhere():
    ids = [c.id for c in R.CASES]
    assert len(ids) == len(set(ids))
    forms = {c.form for c in R.CASES}
    assert forms == set(R.ALL_FORMS), (forms ^ set(R.ALL_FORMS))
    for fam in ('gemm', 'rb', 'astat8', 'wstat', 'astat', 'direct', 'ks16'):   # m_dev = 0 for every family
        assert any(c.form.startswith(fam + '<') and c.m_dev == 0 for c in R.CASES), fam


@pytest.mark.parametrize('c', R.CASES, ids=[c.id for c in R.CASES])
def test_case_table(c):
    for kind in ('int', 'gauss'):
        p = R.build(c, kind)
        R.check_problem(p)
        assert p.arena.nbytes + p.a0.nbytes <= (300 << 20)
    # the reference stays cheap: live rows only (the two full-capacity wstat cases are the largest, 4.3 GFLOP)
    assert 2.0 * R.live_rows(c) * c.n * c.k * c.nbatch <= 4.5e9


def _passing(c, kind):
    p = R.build(c, kind)
    ref, mag = R.reference(p)
    after = p.arena.copy()
    after[R.output_positions(p)] = ref.astype(np.float32)
    R.compare(p, ref, mag, after)
    return p, ref, mag, after


REJECT = [tiny(m_cap=37, n=20, k=36, c_rows=True, c_pad=4, m_dev=33), tiny(m_cap=37, n=20, k=36, nbatch=3, bias_rs=True),
          tiny(m_cap=37, n=20, k=36, accumulate=True)]


@pytest.mark.parametrize('c', REJECT, ids=[c.id for c in REJECT])
def test_comparator_rejects_wrong_results(c):
    for kind in ('int', 'gauss'):
        p, ref, mag, after = _passing(c, kind)
        pos = R.output_positions(p)
        # one element off by twice its bound (integer data: by one unit in the last place)
        z, m, n = p.nbatch - 1, p.M - 1, p.n - 1
        bad = after.copy()
        if kind == 'int':
            bad[pos[z, m, n]] = np.nextafter(bad[pos[z, m, n]], np.float32(np.inf))
        else:
            bad[pos[z, m, n]] = np.float32(ref[z, m, n] + 2.0 * (p.k + 4) * R.U24 * mag[z, m, n] + 2 * np.spacing(np.float32(ref[z, m, n])))
        with pytest.raises(AssertionError):
            R.compare(p, ref, mag, bad)
        # two output rows swapped
        bad = after.copy()
        bad[pos[0, 1]], bad[pos[0, 2]] = after[pos[0, 2]], after[pos[0, 1]]
        with pytest.raises(AssertionError):
            R.compare(p, ref, mag, bad)
        # one guard word changed; a float in the padding columns; a row at or past the live count; an output not written
        for at in (0, R.GUARD - 1, after.size - 1, after.size - R.GUARD):
            bad = after.copy()
            bad.view(np.int32)[at] ^= 1
            with pytest.raises(AssertionError, match='outside the outputs'):
                R.compare(p, ref, mag, bad)
        if p.ldc > p.nbatch * p.n:
            bad = after.copy()
            bad[pos[0, 0, p.n - 1] + 1] = 0.0
            with pytest.raises(AssertionError, match='outside the outputs'):
                R.compare(p, ref, mag, bad)
        if p.M < p.m_cap:
            bad = after.copy()
            bad[p.c_off + int(p.c_rows[p.M]) * p.ldc] = 1.0
            with pytest.raises(AssertionError, match='outside the outputs'):
                R.compare(p, ref, mag, bad)
        if not p.accumulate:
            bad = after.copy()
            bad[pos[0, 0, 0]] = np.nan
            with pytest.raises(AssertionError, match='non-finite'):
                R.compare(p, ref, mag, bad)


def test_debug_gemm_refuses_bad_arguments_before_any_device_call():
    """the pointers are host arrays that are never dereferenced: every refusal comes before the first HIP call"""
    from www2023tiger_amd import _lib
    lib, ptr = _lib.lib, _lib.ptr
    a, w, c = np.zeros((4, 16), np.float32), np.zeros((8, 16), np.float32), np.zeros((4, 8), np.float32)
    b2, valid = np.zeros(8, np.float32), np.ones(4, np.uint8)
    form = C.c_char_p(b'unset')

    def call(**kw):
        f = dict(m_cap=4, n=8, k=16, a0=ptr(a), a0_ld=16, a0_w=16, w=ptr(w), ldw=16, alpha=1.0, c=ptr(c), ldc=8, nbatch=1)
        f.update(kw)
        return lib.tg_debug_gemm(C.byref(_lib.TgGemmProbe(**f)), C.byref(form), None)

    assert lib.tg_debug_gemm(None, C.byref(form), None) == _lib.TG_EINVAL
    for field in ('a0', 'w', 'c'):
        assert call(**{field: None}) == _lib.TG_EINVAL, field
    assert call(k=14, a0_w=14) == _lib.TG_EINVAL
    assert call(a0_w=14, a1=ptr(a), a1_w=2, a1_ld=16) == _lib.TG_EINVAL
    assert call(a0_w=12, a1=ptr(a), a1_w=2, a1_ld=16) == _lib.TG_EINVAL
    assert call(a0_w=10, a1=ptr(a), a1_w=6, a1_ld=16) == _lib.TG_EINVAL
    assert call(ldw=18) == _lib.TG_EINVAL
    assert call(bias2=ptr(b2)) == _lib.TG_EINVAL
    for nb in (0, -1):
        assert call(nbatch=nb) == _lib.TG_EINVAL
    assert call(a0_w=12) == _lib.TG_EINVAL                       # the segments do not add up to k
    assert call(a0_w=8, a1=ptr(a), a1_w=4, a1_ld=16) == _lib.TG_EINVAL
    assert call(w_kmajor=1, n=6) == _lib.TG_EINVAL               # k-major weights are read four columns at a time
    assert form.value is None                                    # a refusal names no kernel
    assert call(m_cap=0) == _lib.TG_OK and form.value is None    # nothing to do: nothing is launched
    assert call(m_cap=0, bias2=ptr(b2), bias2_valid=ptr(valid)) == _lib.TG_OK
    assert not c.any()
