"""Every kernel form of the forward GEMM engine (csrc/tg_gemm.hip: gemm_launch) x every operand / epilogue feature of
GemmArgs that the form implements, against the float64 reference of the whole contract (tests/_gemm_ref.py), through
tg_debug_gemm - one product straight into gemm_launch, which also reports the family and instance it picked.

Each case of _gemm_ref.CASES names the form it was sized for; the test first asserts that this form ran, so a retuned
threshold fails here instead of silently moving the case to another kernel.  Then two kinds of data:
  * integer-valued float32 in {-3 .. 3} with alpha in {1, 0.5, -2}: every product and partial sum is an integer (a
    half-integer after alpha = 0.5) far below 2^24, so the float32 result is exact whatever the order of summation, the
    k-split or the MFMA grouping -> np.array_equal;
  * gaussian times a per-row scale exp(U(-3, 3)): elementwise |got - ref| <= (k + 4) 2^-24 mag, mag = |alpha| (|A| |W| +
    |bias terms|) + |old| - the any-order bound of a length-k float32 inner product (tests/test_hip_dense_bwd.py) plus
    the roundings of the bias adds, the alpha product and the C +=.  Derived, not measured; the build has
    -ffp-contract=off.
C lies in a NaN-filled arena (integers for C +=) with 64 guard floats on each side: guards, rows at or past the live
count, rows that c_rows does not name and columns in [n, ldc) must keep their bits.  A and W sit in tables larger than
what a product reads, NaN wherever it must not read.  Run with -s to see the worst observed fraction of the bound."""
import ctypes as C

import numpy as np
import pytest
import torch

import _gemm_ref as R

pytestmark = pytest.mark.gpu

WORST = {}  # family -> worst observed fraction of the gaussian bound


def dev():
    return torch.device('cuda:0')


def run_on_device(p):
    """the Problem through tg_debug_gemm: (form, arena after the call)"""
    from www2023tiger_amd import _lib
    from www2023tiger_amd.hip_ops import stream_ptr
    keep = []

    def up(a, off=0):
        if a is None:
            return None
        t = torch.from_numpy(a).to(dev())
        keep.append((t, a))
        return t.data_ptr() + off * t.element_size()

    arena = torch.from_numpy(p.arena).to(dev())
    m_dev = up(np.array([p.m_dev], np.int32)) if p.m_dev is not None else None
    probe = _lib.TgGemmProbe(
        m_cap=p.m_cap, m_dev=m_dev, m_hint=p.m_hint, n=p.n, k=p.k,
        a0=up(p.a0, p.a0_off), a0_ld=p.a0_ld, a0_w=p.a0_w, a0_idx=up(p.idx0),
        a1=up(p.a1, p.a1_off), a1_ld=p.a1_ld, a1_w=p.a1_w, a1_idx=up(p.idx1),
        w=up(p.w, p.w_off), ldw=p.ldw, w_kmajor=p.w_kmajor,
        bias=up(p.bias), bias2=up(p.bias2), bias2_valid=up(p.bias2_valid), bias_rs=up(p.bias_rs), ld_brs=p.ld_brs,
        row_valid=up(p.row_valid), relu_mask=up(p.relu_mask), ld_mask=p.ld_mask,
        c_rows=up(p.c_rows), accumulate=p.accumulate, alpha=p.alpha, relu=p.relu,
        c=arena.data_ptr() + 4 * p.c_off, ldc=p.ldc,
        nbatch=p.nbatch, a0_bs=p.a0_bs, w_bs=p.w_bs, bias_bs=p.bias_bs, c_bs=p.c_bs)
    form = C.c_char_p()
    _lib.check(_lib.lib.tg_debug_gemm(C.byref(probe), C.byref(form), stream_ptr(dev())), 'tg_debug_gemm')
    torch.cuda.synchronize()
    for t, a in keep:  # the operands are read only
        assert np.array_equal(t.cpu().numpy().view(np.uint8), a.view(np.uint8))
    return (form.value.decode() if form.value else None), arena.cpu().numpy()


@pytest.mark.parametrize('kind', ['int', 'gauss'])
@pytest.mark.parametrize('c', R.CASES, ids=[c.id for c in R.CASES])
def test_gemm_form(c, kind):
    p = R.build(c, kind)
    form, after = run_on_device(p)
    assert form == c.form, f'{c.id}: sized for {c.form}, but gemm_launch picked {form}'
    ref, mag = R.reference(p)
    frac = R.compare(p, ref, mag, after)
    if kind == 'gauss':
        fam = c.form.split('<')[0]
        WORST[fam] = max(WORST.get(fam, 0.0), frac)
        print(f'  WORST fraction of the (k + 4) 2^-24 mag bound: {frac:.3f} ({c.form}; {fam} so far {WORST[fam]:.3f})')


def test_nothing_is_written_without_live_rows():
    """m_dev = 0 in every family: the arena keeps every bit (compare() has no outputs to excuse)"""
    fams = set()
    for c in R.CASES:
        if c.m_dev == 0:
            p = R.build(c, 'int')
            form, after = run_on_device(p)
            assert form == c.form
            assert np.array_equal(after.view(np.int32), p.arena.view(np.int32)), c.id
            fams.add(c.form.split('<')[0])
    assert fams == {'gemm', 'rb', 'astat8', 'wstat', 'astat', 'direct', 'ks16'}


def test_every_form_of_gemm_launch_is_the_expected_form_of_a_case():
    """every family and instance gemm_launch can pick without an environment knob, a rider or a stream-K operand"""
    assert {c.form for c in R.CASES} == set(R.ALL_FORMS)
    assert len(R.ALL_FORMS) == 34
