"""tg_adam_step (k_adam_tick, k_adam) on its own: one call, then two more, each checked from the state the device itself
produced (downloaded), so no bound compounds.

  * steps[g] goes up by exactly 1 for enabled groups, segments of disabled groups keep p, m, v bit for bit, g is never
    written, the NaN ends of the four buffers stay;
  * m and v are BIT-EXACT against a numpy float32 emulation in the kernel's operation order
        gg = g * (global * segment scale)      (0 means 1; powers of two: exact)
        mm = m + (gg - m) * (1f - b1)
        vv = (v * b2) + (((1f - b2) * gg) * gg)
    (the build has -ffp-contract=off: separately rounded IEEE + - x, which numpy float32 reproduces; 1f - b is exact for
    b in [0.5, 1) by Sterbenz's lemma);
  * p against float64 from the same float32 inputs (b, lr, eps widened from float32; bc1 = 1 - b1^t, bc2 = 1 - b2^t,
    S = lr / bc1, D = sqrt(vv) / sqrt(bc2) + eps):
        |p - p_ref| <= 2^-24 |p_ref| + 16 * 2^-24 * S (|m_old| + |gg|) / D
    16 covers the at most 13 counted roundings: sqrt, two divisions, two additions, one product, the float casts of S
    and sqrt(bc2), m's own error <= 3 * 2^-24 (|m_old| + |gg|), and v's through the square root.  A float32 emulation
    alone stays within 4.5 of these 16 units; run with -s to see the worst observed number of units per test.  If it
    exceeds 8, look for the cause - do not raise the constant.

Segments are packed back to back in one flat buffer each for p, g, m, v: starts are not 16-byte aligned and every
segment's neighbours are its guard bands.  Lengths sit at the edges of 256 (one block), 65 536 (one grid sweep: the
u = 1 slot of the four-in-flight loop) and 4 * 65 536 (the loop's second pass)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

GUARD = 64
U24 = 2.0 ** -24
LENGTHS = [1, 3, 255, 256, 257, 65535, 65536, 65537, 131073, 262143, 262144, 262145, 300001]
N_GROUPS = 4
SEG_SCALE = (0.0, 1.0, 0.5, 2.0)  # segment i: SEG_SCALE[i % 4]; 0 means 1
STARTS = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
TOTAL = int(STARTS[-1])
# (lr, beta1, beta2, eps, steps before the call, global grad_scale)
PARAMS = {
    'first_step': (1e-3, 0.9, 0.999, 1e-8, [0, 0, 0, 0], 1.0),
    'second_step_scaled': (1e-3, 0.9, 0.999, 1e-8, [1, 1, 1, 1], 0.25),
    'mixed_large_t': (1e-2, 0.8, 0.95, 1e-6, [999, 0, 99999, 7], 1.0),
    # the default betas at t = 1000: bc2 = 0.63 there, so a wrong large-t correction moves p by far more than the bound
    'default_betas_large_t': (1e-3, 0.9, 0.999, 1e-8, [999, 0, 99999, 7], 1.0),
}
ENABLED = {'null': None, 'all': [1, 1, 1, 1], 'alternate': [1, 0, 1, 0], 'none': [0, 0, 0, 0]}


def seg_of():
    """group and scale of every element of the flat buffers"""
    group = np.empty(TOTAL, dtype=np.int64)
    scale = np.empty(TOTAL, dtype=np.float32)
    for i, n in enumerate(LENGTHS):
        group[STARTS[i]:STARTS[i + 1]] = i % N_GROUPS
        scale[STARTS[i]:STARTS[i + 1]] = SEG_SCALE[i % 4] if SEG_SCALE[i % 4] != 0.0 else 1.0
    return group, scale


GROUP, SCALE = seg_of()


@functools.lru_cache(maxsize=None)
def make_state(random_state, seed):
    """p, g, m, v of every test (shared: nobody writes into them)"""
    rs = np.random.RandomState(seed)
    g = (rs.standard_normal(TOTAL) * np.exp(rs.uniform(-13, 7, TOTAL))).astype(np.float32)
    g[::7] = 0.0
    p = rs.standard_normal(TOTAL).astype(np.float32)
    if random_state:
        m = (rs.standard_normal(TOTAL) * np.exp(rs.uniform(-9, 5, TOTAL))).astype(np.float32)
        v = ((rs.standard_normal(TOTAL) * np.exp(rs.uniform(-9, 5, TOTAL))) ** 2).astype(np.float32)
    else:
        m = np.zeros(TOTAL, dtype=np.float32)
        v = np.zeros(TOTAL, dtype=np.float32)
    for a in (p, g, m, v):
        a.setflags(write=False)
    return p, g, m, v


def emulate(p, g, m, v, t, lr, b1, b2, eps, gscale):
    """one step on the CPU.  t: the step count AFTER the increment, per element (float64).  Returns the float32 m and v
    the kernel must produce bit for bit, the float64 p and the bound on |p - p_ref|."""
    b1f, b2f = np.float32(b1), np.float32(b2)
    gg = g * (np.float32(gscale) * SCALE)
    assert np.array_equal(gg.astype(np.float64), g.astype(np.float64) * float(gscale) * SCALE.astype(np.float64))  # exact
    mm = m + (gg - m) * (np.float32(1) - b1f)
    vv = (v * b2f) + (((np.float32(1) - b2f) * gg) * gg)
    assert mm.dtype == np.float32 and vv.dtype == np.float32
    for a in (gg, mm, vv, (np.float32(1) - b2f) * gg):  # no subnormal intermediate: denormal handling is not under test
        nz = np.abs(a[a != 0])
        assert nz.size == 0 or nz.min() >= np.finfo(np.float32).tiny
    b1d, b2d, lrd, epsd = float(b1f), float(b2f), float(np.float32(lr)), float(np.float32(eps))
    g64, m64, v64 = gg.astype(np.float64), m.astype(np.float64), v.astype(np.float64)
    mm64 = m64 + (g64 - m64) * (1.0 - b1d)
    vv64 = v64 * b2d + (1.0 - b2d) * g64 * g64
    t = np.maximum(t, 1.0)  # (t = 0: a group that never stepped and is disabled now; its elements are not compared)
    S = lrd / (1.0 - b1d ** t)
    D = np.sqrt(vv64) / np.sqrt(1.0 - b2d ** t) + epsd
    p_ref = p.astype(np.float64) - S * mm64 / D
    unit = U24 * S * (np.abs(m64) + np.abs(g64)) / D
    return mm, vv, p_ref, unit


def units_used(p, p_ref, unit):
    """how many of the 16 units the worst element uses (after the 2^-24 |p_ref| of the final subtraction)"""
    excess = np.abs(p.astype(np.float64) - p_ref) - U24 * np.abs(p_ref)
    pos = unit > 0
    assert (excess[~pos] <= 0).all(), 'p moved where the update is exactly zero'
    return float(np.maximum(excess[pos] / unit[pos], 0.0).max()) if pos.any() else 0.0


def dev():
    return torch.device('cuda:0')


class Buffers:
    def __init__(self, p, g, m, v):
        from www2023tiger_amd._lib import TgAdamSeg
        pad = np.full(GUARD, np.nan, dtype=np.float32)
        self.t = {k: torch.from_numpy(np.concatenate([pad, a, pad])).to(dev())
                  for k, a in (('p', p), ('g', g), ('m', m), ('v', v))}
        segs = (TgAdamSeg * len(LENGTHS))()
        for i, n in enumerate(LENGTHS):
            for k in 'pgmv':
                setattr(segs[i], k, self.t[k].data_ptr() + 4 * (GUARD + int(STARTS[i])))
            segs[i].n, segs[i].group, segs[i].grad_scale = n, i % N_GROUPS, SEG_SCALE[i % 4]
        raw = np.frombuffer(ctypes.string_at(ctypes.addressof(segs), ctypes.sizeof(segs)), dtype=np.uint8).copy()
        self.segs = torch.from_numpy(raw).to(dev())

    def download(self):
        out = {}
        for k, t in self.t.items():
            h = t.cpu().numpy()
            ends = np.concatenate([h[:GUARD], h[-GUARD:]]).view(np.int32)
            assert (ends == 0x7FC00000).all(), f'the NaN ends of {k} were written'
            out[k] = h[GUARD:-GUARD].copy()
        return out


@pytest.mark.gpu
@pytest.mark.parametrize('random_state', [False, True], ids=['zero_state', 'random_state'])
@pytest.mark.parametrize('params,flags', [(q, f) for q in list(PARAMS)[:3] for f in ENABLED] +
                         [('default_betas_large_t', 'all')])
def test_adam_step(params, flags, random_state):
    from www2023tiger_amd._lib import check, lib, ptr
    from www2023tiger_amd.hip_ops import stream_ptr
    lr, b1, b2, eps, steps0, gscale = PARAMS[params]
    enabled = ENABLED[flags]
    on = np.ones(N_GROUPS, dtype=bool) if enabled is None else np.array(enabled, dtype=bool)
    p, g, m, v = make_state(random_state, seed=11)
    buf = Buffers(p, g, m, v)
    steps_d = torch.tensor(steps0, dtype=torch.int32, device=dev())
    en_d = None if enabled is None else torch.tensor(enabled, dtype=torch.int32, device=dev())
    steps = np.array(steps0, dtype=np.int64)
    live = on[GROUP]
    worst = 0.0
    for call in range(3):
        check(lib.tg_adam_step(ptr(buf.segs), len(LENGTHS), N_GROUPS, ptr(en_d), ptr(steps_d), lr, b1, b2, eps, gscale,
                               stream_ptr(dev())), 'tg_adam_step')
        torch.cuda.synchronize()
        got = buf.download()
        steps = steps + on
        np.testing.assert_array_equal(steps_d.cpu().numpy(), steps, err_msg=f'step counts, call {call}')
        np.testing.assert_array_equal(got['g'].view(np.int32), g.view(np.int32), err_msg='g was written')
        if live.any():
            mm, vv, p_ref, unit = emulate(p, g, m, v, steps[GROUP].astype(np.float64), lr, b1, b2, eps, gscale)
        else:
            mm, vv = m, v
        for k, old, new in (('m', m, mm), ('v', v, vv)):
            want = np.where(live, new, old)
            bad = np.flatnonzero(got[k].view(np.int32) != want.view(np.int32))
            assert bad.size == 0, (k, 'not bit-exact', f'call {call}', len(bad), bad[:6].tolist(),
                                   got[k][bad[:6]].tolist(), want[bad[:6]].tolist())
        bad = np.flatnonzero(got['p'].view(np.int32)[~live] != p.view(np.int32)[~live])
        assert bad.size == 0, ('p of a disabled group changed', f'call {call}', len(bad))
        if live.any():
            err = np.abs(got['p'][live].astype(np.float64) - p_ref[live])
            bound = U24 * np.abs(p_ref[live]) + 16 * unit[live]
            u = units_used(got['p'][live], p_ref[live], unit[live])
            worst = max(worst, u)
            over = np.flatnonzero(err > bound)
            assert over.size == 0, ('p', f'call {call}', 'units used', u, len(over), np.flatnonzero(live)[over[:6]].tolist())
        p, m, v = got['p'], got['m'], got['v']  # the next call is checked from what the device produced
    print(f'  WORST units of 2^-24 S (|m| + |gg|) / D used by p (16 allowed): {worst:.2f}')
    assert worst <= 16


def test_emulation_is_torch_adam():
    """ties the emulation to the definition: torch.optim.Adam on the CPU in float32 (first parameter set, first three
    segments) gives p within the same bound of the float64 reference"""
    lr, b1, b2, eps, steps0, gscale = PARAMS['first_step']
    p, g, m, v = make_state(False, seed=11)
    n = int(STARTS[3])
    _, _, p_ref, unit = emulate(p, g, m, v, np.ones(TOTAL), lr, b1, b2, eps, gscale)
    params = [torch.nn.Parameter(torch.from_numpy(p[STARTS[i]:STARTS[i + 1]].copy())) for i in range(3)]
    for i, q in enumerate(params):
        q.grad = torch.from_numpy(g[STARTS[i]:STARTS[i + 1]] * (np.float32(gscale) * SCALE[STARTS[i]:STARTS[i + 1]]))
    torch.optim.Adam(params, lr=lr, betas=(b1, b2), eps=eps).step()
    got = np.concatenate([q.detach().numpy() for q in params])
    err = np.abs(got.astype(np.float64) - p_ref[:n])
    assert (err <= U24 * np.abs(p_ref[:n]) + 16 * unit[:n]).all()
    assert units_used(got, p_ref[:n], unit[:n]) <= 8
