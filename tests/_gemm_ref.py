"""The float64 reference of the forward GEMM engine's whole contract (csrc/tg_dense.h: GemmArgs, tg_gemm.hip:
gemm_epilogue), the case table of tests/test_hip_gemm_forms.py and its comparator - all of it host code, checked
without a GPU by tests/test_gemm_ref_host.py.

A Problem holds the operands AS THEY LIE IN MEMORY (flat float32 arrays with the pointer offset, row stride and batch
stride the library is given), not as tidy matrices: tables are larger than what a product reads, and everything a
product must not read - table rows nobody indexes, columns past a row's width, rows of A at or past the live count,
index entries of dead rows (they point at a NaN row) - is NaN, so a kernel that reads one of them shows it.

For each live row m < M = min(m_cap, m_dev) and each batch z:
    A[m]  = [a0[idx0[m]] | a1[idx1[m]]]
    be    = bias[n] * (bias_rs[m * ld_brs + z] if given else 1) + (bias2[n] if bias2_valid[m])
    v     = alpha * (A . W + be);  ReLU;  row_valid;  relu_mask > 0;  += old
    C[z * c_bs + (c_rows[m] or m) * ldc + n] = v            every other float of the arena keeps its bits
"""
from types import SimpleNamespace

import numpy as np

GUARD = 64
U24 = 2.0 ** -24
NAN_BITS = 0x7FC00000
ALPHAS = (1.0, 0.5, -2.0)


# ------------------------------------------------------------------------------------------------------------------
# the case table.  Thresholds, from gemm_launch / gemm_ks16_launch (BK = 32, 64 x 64 tiles MT x NT):
#   many = ceil(m_cap / 128) * NT >= 4096: m_cap >= 130 945 (NT 4), 174 721 (NT 3), 262 017 (NT 2), 65 409 (NT 8),
#          52 353 (NT 10), 32 641 (NT 16), 16 257 (NT 32)
#   ks16   plain + a1 / idx (+ bias2 when the caller offers the product itself), no c_rows: N <= 64 (CT 4) / <= 112 (CT 7): K >= 384, <= 1 100 blocks of 32 rows, 16-row
#          blocks while ceil(m / 16) <= 256; else 48-column tiles: K >= 320 when ceil(m / 48) ceil(N / 48) <= 256, else
#          K >= 512, <= 1 100 tiles; rows per block 16 / 32 / 48 by ceil(m / 16 | 32) ceil(N / 48) <= 256
#   wstat  many, plain (c_rows, idx), 64 <= K <= 256, N <= 256; NS by ceil(K / 16): <= 8, <= 11, else 16
#   astat8 many, plain (c_rows, idx), 4 / 6 / 8 k-tiles
#   rb     many, plain + a1 / bias2; <2,2> when N % 128 == 0 and K >= 512
#   direct plain (c_rows, idx), K <= 192, tiles of min(m_hint, m_cap) x N <= 512; NS by ceil(K / 16): <= 7, <= 11, 12;
#          32 x 48 wave tiles above 256 tiles (NS <= 11)
#   astat  plain (c_rows, idx), NT >= 8, 4 / 6 / 8 k-tiles, MT NT <= 1 024
#   gemm   everything else; two k-groups when the grid 8 ceil(MT / 8) NT nbatch <= 256 and K >= 512
# ------------------------------------------------------------------------------------------------------------------
MANY = {4: 130945, 3: 174721, 2: 262017, 8: 65409, 10: 52353, 16: 32641, 32: 16257}
for _nt, _m in MANY.items():
    assert -(-_m // 128) * _nt >= 4096 > -(-(_m - 1) // 128) * _nt

DEFAULTS = dict(m_dev=None, m_hint=0, idx=False, a_pad=0, a1_w=0, idx1=False, c_rows=False, alpha=1.0, relu=0, c_pad=0,
                w_pad=0, bias=True, bias2=False, bias_rs=False, row_valid=False, relu_mask=False, accumulate=False,
                w_kmajor=False, nbatch=1)
CASES = []


def case(form, m_cap, n, k, **feat):
    bad = set(feat) - set(DEFAULTS)
    assert not bad, bad
    c = SimpleNamespace(form=form, m_cap=m_cap, n=n, k=k, **{**DEFAULTS, **feat})
    tags = [f'{key}={feat[key]}' if not isinstance(feat[key], bool) else key for key in feat]
    c.id = f'{form}-{m_cap}x{n}x{k}' + ('-' + '-'.join(tags) if tags else '')
    CASES.append(c)


# -- direct: K at the edges of the three chunk-slot counts, rows and columns around the 16 / 32 / 64 edges
for _i, _k in enumerate((4, 28, 112, 116, 176, 180, 192)):
    _ns = '7' if _k <= 112 else '11' if _k <= 176 else '12'
    for _j, (_m, _n) in enumerate(((1, 4), (31, 17), (33, 33), (65, 70))):
        _f = [dict(), dict(alpha=0.5, relu=1), dict(c_pad=8, a_pad=4), dict(alpha=-2.0, w_pad=8)][(_i + _j) % 4]
        case(f'direct<{_ns},2x2>', _m, _n, _k, **_f)
for _k, _ns in ((112, '7'), (176, '11'), (192, '12')):
    case(f'direct<{_ns},2x2>', 65, 70, _k, idx=True, bias=False)
    case(f'direct<{_ns},2x2>', 65, 70, _k, c_rows=True, relu=1)
    case(f'direct<{_ns},2x2>', 65, 70, _k, idx=True, c_rows=True, alpha=0.5, c_pad=4, a_pad=8)
    for _md in (0, 1, 64, 65):
        case(f'direct<{_ns},2x2>', 65, 70, _k, m_dev=_md, idx=_md == 64, c_rows=_md == 1)
case('direct<7,2x2>', 5000, 70, 112, m_dev=5000, m_hint=64)   # many more live tiles than the launch was sized for
case('direct<11,2x2>', 5000, 33, 176, m_dev=4999, m_hint=64, idx=True, c_rows=True)
case('direct<7,2x2>', 8192, 70, 112)                          # 256 tiles: the last launch of 32 x 32 wave tiles
case('direct<7,2x3>', 8193, 70, 112, idx=True, alpha=0.5, relu=1, a_pad=4, bias=False)   # 258 tiles
case('direct<11,2x3>', 8257, 70, 176, idx=True, c_rows=True, alpha=-2.0, relu=1, c_pad=4)
case('direct<11,2x3>', 8257, 100, 116, m_dev=8200, a_pad=4, w_pad=8)
case('direct<7,2x3>', 16384, 70, 112, m_dev=0)                # 512 tiles: the last direct launch
case('direct<7,2x3>', 16384, 65, 28, m_hint=20000, c_rows=True)
case('gemm<ks1,d2>', 16385, 70, 112, m_dev=130)               # 514 tiles
case('gemm<ks1,d2>', 65, 70, 196)                             # 13 chunk slots

# -- astat: more than seven column tiles, 4 / 6 / 8 k-tiles, at most 1 024 tiles, shapes direct does not take
case('astat<4>', 4097, 452, 100, idx=True)                    # 65 x 8 = 520 tiles
case('astat<4>', 2100, 1000, 128, c_rows=True, alpha=0.5, relu=1, w_pad=8)     # 33 x 16 = 528
case('astat<6>', 3638, 516, 164, m_dev=3601, relu=1)          # 57 x 9 = 513: odd NT, the last block has one column tile
case('astat<6>', 4097, 452, 192, idx=True, c_rows=True, c_pad=12, a_pad=4)
case('astat<8>', 33, 452, 228, bias=False)
case('astat<8>', 65, 1000, 256, c_rows=True, m_dev=64, w_pad=8)
case('astat<8>', 1, 516, 256, idx=True, alpha=-2.0)
case('astat<8>', 8192, 512, 256, m_dev=70)                    # 1 024 tiles: the last astat launch
case('gemm<ks1,d2>', 8193, 512, 256, m_dev=70)                # 1 032
case('astat<4>', 4097, 452, 100, m_dev=0)
case('direct<7,2x3>', 4096, 452, 100)                         # 512 tiles: still direct

# -- ks16: one column tile of 64 / 112 columns (K >= 384), else 48-column tiles (K >= 320 in one round, else 512)
case('ks16<1,4,4>', 4096, 64, 384)
case('ks16<2,4,4>', 4097, 64, 384, idx=True)
case('ks16<1,4,4>', 17, 4, 388, alpha=0.5, relu=1)
case('gemm<ks1,d2>', 17, 64, 380)
case('ks16<2,4,4>', 35200, 60, 384, m_dev=35199, a_pad=4)      # 1 100 blocks: the last launch
case('gemm<ks1,d2>', 35201, 60, 384, m_dev=100)
case('ks16<1,7,4>', 4096, 65, 384, a1_w=148, idx1=True)
case('ks16<2,7,4>', 4097, 112, 384, m_dev=4081)
case('ks16<1,7,4>', 600, 100, 500, a1_w=100, idx=True, idx1=True, c_pad=4)
case('ks16<1,3,4>', 1024, 172, 320, bias=False)
case('ks16<2,3,4>', 1025, 172, 324, a1_w=176, idx1=True)       # segments of 148 + 176: neither a multiple of 32
case('ks16<2,3,4>', 2048, 113, 320, idx=True, alpha=-2.0)
case('ks16<3,3,4>', 2049, 172, 320, m_dev=2017)
case('ks16<3,3,4>', 3072, 172, 1204, a1_w=172, idx=True, idx1=True, relu=1)  # 64 x 4 blocks: one per CU, one round
case('gemm<ks1,d2>', 3073, 172, 320, m_dev=100)                # two rounds need K >= 512
case('ks16<3,3,4>', 3073, 172, 512, m_dev=3073)
case('ks16<1,3,4>', 33, 172, 1204, a1_w=688, m_dev=0)
case('ks16<1,3,4>', 1, 130, 324, w_pad=8)
# (a second bias reaches ks16 the way the fused attention's fc1 does: offered to gemm_ks16_launch before gemm_launch)
case('ks16<1,3,4>', 100, 172, 1204, a1_w=172, idx=True, idx1=True, bias2=True, relu=1)
case('ks16<3,3,4>', 3072, 172, 1204, a1_w=172, bias2=True, m_dev=3001, alpha=0.5)
case('ks16<2,7,4>', 4100, 100, 400, bias2=True, idx=True, c_pad=4)
case('ks16<1,4,4>', 50, 64, 384, bias2=True, alpha=-2.0, bias=False)

# -- wstat: many rows, 64 <= K <= 256, N <= 256; all four <CROWS, IDX> instances of each slot count
_W = MANY[4]
case('wstat<8>', _W, 256, 64, m_dev=17)
case('wstat<8>', _W + 5, 256, 64)                             # full capacity, 130 950 = 16 * 8 184 + 6 rows
case('wstat<8>', _W, 256, 64, m_dev=0)
case('wstat<8>', _W, 256, 64, m_dev=4097, m_hint=64, alpha=0.5, relu=1)
case('gemm<ks1,d2>', _W - 1, 256, 64, m_dev=33)               # one row short of `many`
case('wstat<8,crows>', _W, 256, 68, m_dev=15, c_rows=True, c_pad=4)        # 17 chunks: not a multiple of 4
case('wstat<8,idx>', _W, 256, 128, m_dev=3001, idx=True)
case('wstat<8,crows,idx>', _W, 256, 128, m_dev=1, c_rows=True, idx=True)
case('wstat<8,crows,idx>', MANY[3], 172, 100, m_dev=2049, c_rows=True, idx=True, alpha=-2.0, a_pad=4, w_pad=8)
case('wstat<11>', _W, 256, 132, m_dev=2049, relu=1, bias=False)
case('wstat<11,crows>', MANY[2], 100, 176, m_dev=17, c_rows=True)
case('wstat<11,idx>', MANY[3], 172, 176, m_dev=4113, idx=True, c_pad=4)
case('wstat<11,crows,idx>', _W, 256, 140, m_dev=15, c_rows=True, idx=True)
case('wstat<11,idx>', _W, 200, 176, m_dev=0, idx=True)
case('wstat<16>', _W, 256, 180, m_dev=1, alpha=-2.0, relu=1, bias=False)
case('wstat<16,crows>', _W, 256, 256, m_dev=2063, c_rows=True, alpha=0.5)
case('wstat<16,idx>', MANY[2], 100, 256, m_dev=17, idx=True, relu=1)
case('wstat<16,crows,idx>', MANY[3], 172, 180, m_dev=3001, c_rows=True, idx=True)
case('wstat<8,crows,idx>', _W + 5, 256, 64, c_rows=True, idx=True)    # full capacity through a gather and a scatter
case('wstat<16,crows,idx>', _W, 256, 256, m_dev=4099, c_rows=True, idx=True, c_pad=4)
case('wstat<16>', _W, 256, 256, m_dev=0)

# -- astat8: as wstat, N > 256
_A = MANY[32]
case('astat8<4>', _A + 4, 2048, 100, m_dev=8069, c_rows=True, relu=1)              # 63 full 128-row blocks and a ragged one
case('astat8<4>', _A, 2048, 128, m_dev=129, idx=True, bias=False)
case('astat8<6>', _A, 2048, 164, m_dev=1, c_rows=True)
case('astat8<6>', MANY[16], 1000, 192, m_dev=2000, idx=True, c_rows=True, alpha=0.5, relu=1)
case('astat8<8>', MANY[10], 580, 228, m_dev=257, c_pad=4)     # ten column tiles: a block of eight and a block of two
case('astat8<8>', MANY[8], 452, 256, m_dev=127, idx=True, a_pad=4, w_pad=8)
case('astat8<8>', _A, 2048, 256, m_dev=0)
case('gemm<ks1,d2>', _A - 1, 2048, 256, m_dev=64)             # one row short of `many`, and far too many tiles for astat

# -- rb: many rows, K outside the short-K sets, or a second segment / second bias
case('rb<2,1>', _W, 256, 32, m_dev=133, bias=False)
case('rb<2,1>', _W, 256, 36, m_dev=2565, idx=True, a_pad=4, w_pad=8)   # a ragged last 128-row block
case('rb<2,1>', _W, 256, 288, m_dev=127, c_rows=True, alpha=0.5)
case('rb<2,1>', _W, 256, 128, m_dev=300, a1_w=68, idx=True, idx1=True)
case('rb<2,1>', _W, 256, 128, m_dev=300, bias2=True, relu=1)
case('rb<2,1>', MANY[3], 172, 324, m_dev=129, a1_w=176, bias2=True, c_rows=True, idx1=True, c_pad=4)
case('rb<2,1>', MANY[2], 100, 516, m_dev=65, idx=True)        # K >= 512 but N is no multiple of 128
case('rb<2,1>', _W, 256, 32, m_dev=0)
case('rb<2,2>', _W, 256, 512, m_dev=2565, idx=True, relu=1, c_pad=4, a_pad=4, w_pad=8, bias=False)
case('rb<2,2>', MANY[2], 128, 516, m_dev=129, idx=True, a1_w=176, idx1=True, bias2=True, c_rows=True, alpha=-2.0)
case('rb<2,2>', _W, 256, 512, m_dev=0, idx=True)

# -- the generic kernel: every feature no other family takes, alone and in the callers' combinations
for _n in (4, 60, 68):
    case('gemm<ks1,d2>', 65, _n, 96, w_kmajor=True)
for _k in (4, 28, 32, 36, 96, 516):  # k-tile edges x rows and columns one float4 either side of a 64 x 64 tile
    for _m, _n in ((60, 68), (64, 64), (68, 60)):
        case('gemm<ks2>' if _k >= 512 else 'gemm<ks1,d2>', _m, _n, _k, row_valid=True, idx=_m == 68, a_pad=4 if _n == 68 else 0)
case('gemm<ks1,d2>', 65, 68, 36, row_valid=True)
case('gemm<ks1,d2>', 65, 68, 36, relu_mask=True)
case('gemm<ks1,d2>', 65, 68, 36, accumulate=True, alpha=0.5)
case('gemm<ks1,d2>', 65, 68, 36, bias_rs=True)
case('gemm<ks1,d2>', 65, 68, 36, bias2=True)
case('gemm<ks1,d2>', 130, 68, 96, relu_mask=True, accumulate=True, w_kmajor=True, bias=False)   # backward
case('gemm<ks1,d2>', 61, 33, 32, bias_rs=True, nbatch=3)                                        # restarter value product
case('gemm<ks1,d2>', 65, 33, 28, bias_rs=True, nbatch=4, idx=True, relu=1)
case('gemm<ks1,d2>', 67, 33, 36, nbatch=3, c_pad=5)
case('gemm<ks1,d2>', 68, 60, 28, row_valid=True, c_rows=True)
case('gemm<ks1,d2>', 60, 64, 32, row_valid=True, c_rows=True, m_dev=59, idx=True)
case('gemm<ks1,d2>', 64, 68, 96, bias2=True, a1_w=36, idx1=True, alpha=-2.0)
case('gemm<ks2>', 61, 60, 540, row_valid=True, bias=False)
case('gemm<ks2>', 64, 64, 516, accumulate=True, c_rows=True, alpha=-2.0, c_pad=4, w_pad=8)
case('gemm<ks2>', 68, 68, 516, w_kmajor=True, relu_mask=True)
case('gemm<ks2>', 100, 172, 1204, a1_w=172, idx=True, idx1=True, bias2=True, c_rows=True, relu=1)
case('gemm<ks2>', 33, 130, 512, c_rows=True, m_dev=0)
case('gemm<ks2>', 8129, 68, 516, bias_rs=True, m_dev=130)      # 8 x 16 x 2 = 256 blocks: the last launch with two k-groups
case('gemm<ks1,d2>', 8193, 68, 516, bias_rs=True, m_dev=130)   # 272 blocks
case('gemm<ks1,d2>', 65, 68, 36, row_valid=True, m_dev=0)

# every form gemm_launch can pick without an environment knob, a rider or a stream-K operand
ALL_FORMS = (['gemm<ks1,d2>', 'gemm<ks2>', 'rb<2,1>', 'rb<2,2>'] +
             [f'astat8<{t}>' for t in (4, 6, 8)] + [f'astat<{t}>' for t in (4, 6, 8)] +
             [f'wstat<{ns}{f}>' for ns in (8, 11, 16) for f in ('', ',crows', ',idx', ',crows,idx')] +
             ['direct<7,2x2>', 'direct<7,2x3>', 'direct<11,2x2>', 'direct<11,2x3>', 'direct<12,2x2>'] +
             [f'ks16<{rt},{ct},4>' for rt, ct in ((1, 4), (2, 4), (1, 7), (2, 7), (1, 3), (2, 3), (3, 3))])


# ------------------------------------------------------------------------------------------------------------------
# a case's operands, as they lie in memory
# ------------------------------------------------------------------------------------------------------------------
def live_rows(c):
    return c.m_cap if c.m_dev is None else min(c.m_cap, c.m_dev)


def _values(rs, kind, rows, cols):
    """[rows, cols] float32: integers in {-3 .. 3}, or gaussian times a per-row scale exp(U(-3, 3))"""
    if kind == 'int':
        return rs.randint(-3, 4, size=(rows, cols)).astype(np.float32)
    return (rs.standard_normal((rows, cols)) * np.exp(rs.uniform(-3, 3, (rows, 1)))).astype(np.float32)


def _table(vals, ld, rows_total):
    """vals [r, w] at the top left of a NaN table [rows_total, ld], flat"""
    t = np.full((rows_total, ld), np.nan, dtype=np.float32)
    t[:vals.shape[0], :vals.shape[1]] = vals
    return t.reshape(-1)


def _index(rs, m_cap, M, T):
    """row indices into a table of T value rows + one NaN row: live rows get the LAST value row first, then a descending
    run with every fifth entry repeating its predecessor, then random rows; dead rows point at the NaN row"""
    idx = np.full(m_cap, T, dtype=np.int64)
    m = np.arange(M)
    live = (T - 1 - m) % T
    far = m >= 2 * T
    live[far] = rs.randint(0, T, size=int(far.sum()))
    rep = (m % 5 == 4)
    live[rep] = live[np.maximum(m[rep] - 1, 0)]
    idx[:M] = live
    return idx


def _segment(rs, kind, c, M, width, gathered, pad, nbatch):
    """one A segment: (flat, ld, idx).  Dense: m_cap rows, the dead ones NaN.  Gathered: a table of min(M, 37) + 1 rows."""
    ld = nbatch * width + pad
    if gathered:
        T = max(1, min(M, 37))
        return _table(_values(rs, kind, T, nbatch * width), ld, T + 1), ld, _index(rs, c.m_cap, M, T)
    return _table(_values(rs, kind, M, nbatch * width), ld, c.m_cap), ld, None


def build(c, kind, seed=0):
    """the Problem of case `c` with integer ('int') or gaussian ('gauss') data"""
    rs = np.random.RandomState((c.m_cap * 1000003 + c.n * 1009 + c.k * 31 + len(c.id) + seed * 7919) % (2 ** 31))
    M, n, k, nb = live_rows(c), c.n, c.k, c.nbatch
    p = SimpleNamespace(case=c, kind=kind, m_cap=c.m_cap, M=M, m_dev=c.m_dev, m_hint=c.m_hint, n=n, k=k, nbatch=nb,
                        alpha=float(c.alpha), relu=int(c.relu), accumulate=int(c.accumulate), w_kmajor=int(c.w_kmajor))
    assert not (c.a1_w and nb > 1)
    p.a0_w = k - c.a1_w
    p.a0, p.a0_ld, p.idx0 = _segment(rs, kind, c, M, p.a0_w, c.idx, c.a_pad, nb)
    p.a0_off, p.a0_bs = 0, (p.a0_w if nb > 1 else 0)
    p.a1 = p.idx1 = None
    p.a1_w, p.a1_ld, p.a1_off = c.a1_w, 0, 0
    if c.a1_w:
        p.a1, p.a1_ld, p.idx1 = _segment(rs, kind, c, M, c.a1_w, c.idx1, c.a_pad, 1)
    # W: [nbatch * n, k] row-major or [k, n] k-major inside a NaN table with w_pad more columns and one more row; the
    # pointer sits w_pad / 2 columns in
    assert c.w_pad % 8 == 0 and not (c.w_kmajor and nb > 1)
    wv = _values(rs, kind, nb * n, k)
    p.w_off = c.w_pad // 2
    if c.w_kmajor:
        p.ldw = n + c.w_pad
        t = np.full((k + 1, p.ldw), np.nan, dtype=np.float32)
        t[:k, p.w_off:p.w_off + n] = wv.T
    else:
        p.ldw = k + c.w_pad
        t = np.full((nb * n + 1, p.ldw), np.nan, dtype=np.float32)
        t[:nb * n, p.w_off:p.w_off + k] = wv
    p.w, p.w_bs = t.reshape(-1), (n * p.ldw if nb > 1 else 0)
    small = lambda *s: (rs.randint(-3, 4, size=s) if kind == 'int' else rs.standard_normal(s)).astype(np.float32)
    p.bias, p.bias_bs = (small(nb * n) if c.bias else None), (n if nb > 1 else 0)
    p.bias2 = small(n) if c.bias2 else None
    flags = lambda: np.where(np.arange(c.m_cap) < M, rs.choice(np.array([0, 1, 0, 255, 2], np.uint8), c.m_cap), 1).astype(np.uint8)
    p.bias2_valid = flags() if c.bias2 else None
    p.row_valid = flags() if c.row_valid else None
    p.ld_brs = nb + 1
    p.bias_rs = _table(small(M, nb), p.ld_brs, max(M, 1)) if c.bias_rs else None
    p.ld_mask = n + 4
    p.relu_mask = _table(rs.randint(-1, 2, size=(M, n)).astype(np.float32), p.ld_mask, max(M, 1)) if c.relu_mask else None
    # C: an arena of m_cap (+ 7 with c_rows) rows of ldc floats between two guard bands; NaN, or integers for C +=
    p.ldc = nb * n + c.c_pad
    p.c_bs = n if nb > 1 else 0
    p.arena_rows = c.m_cap + (7 if c.c_rows else 0)
    p.c_rows = rs.permutation(p.arena_rows)[:c.m_cap].astype(np.int32) if c.c_rows else None
    p.c_off = GUARD
    size = 2 * GUARD + p.arena_rows * p.ldc
    if c.accumulate:
        p.arena = rs.randint(-3, 4, size=size).astype(np.float32)
    else:
        p.arena = np.full(size, np.nan, dtype=np.float32)
    return p


def check_problem(p):
    """what the library and the exactness argument need of a Problem (tests/test_gemm_ref_host.py runs it on every case)"""
    c = p.case
    assert 0 <= p.M <= p.m_cap and p.a0_w + p.a1_w == p.k and p.a0_w > 0
    for v in (p.k, p.a0_w, p.a1_w, p.ldw, p.a0_ld, p.a1_ld, p.a0_off, p.a1_off, p.w_off, p.a0_bs, p.w_bs):
        assert v % 4 == 0, 'strides and offsets of the float4 operands are multiples of 4 floats'
    if p.w_kmajor:
        assert p.n % 4 == 0
    for tab, ld, w, idx, off in ((p.a0, p.a0_ld, p.nbatch * p.a0_w, p.idx0, p.a0_off), (p.a1, p.a1_ld, p.a1_w, p.idx1, p.a1_off)):
        if tab is None:
            continue
        rows = (tab.size - off) // ld
        assert ld >= w
        if idx is None:
            assert rows >= p.m_cap
        else:
            assert idx.shape == (p.m_cap,) and idx.min() >= 0 and idx.max() < rows
            if p.M:
                live = idx[:p.M]
                assert live[0] == rows - 2, 'the last value row of the table is read'
                assert np.isfinite(tab[off:].reshape(rows, ld)[live, :w]).all()
            if p.M >= 12:
                assert (np.diff(live) < 0).any() and (np.diff(live) == 0).any(), 'descending and repeated entries'
    if p.c_rows is not None:
        assert p.c_rows.shape == (p.m_cap,) and len(np.unique(p.c_rows)) == p.m_cap, 'c_rows is injective'
        assert p.c_rows.min() >= 0 and p.c_rows.max() < p.arena_rows
        assert p.m_cap < 2 or (np.diff(p.c_rows) != 1).any(), 'c_rows is a scatter'
    assert p.ldc >= p.nbatch * p.n and p.arena.size == 2 * GUARD + p.arena_rows * p.ldc
    assert p.c_off == GUARD and (p.nbatch - 1) * p.c_bs + p.n <= p.ldc
    if p.kind == 'int':
        # |A . W| <= 9 k, |bias * rs| <= 9, |bias2| <= 3, |alpha| <= 2, |old| <= 3: every partial sum, in any order, is an
        # integer (or, with alpha = 0.5, a half-integer) far below 2^24
        assert p.alpha in ALPHAS and 2 * (9 * p.k + 9 + 3) + 3 < 2 ** 24
        for a in (p.a0, p.a1, p.w, p.bias, p.bias2, p.bias_rs, p.arena if p.accumulate else None):
            if a is not None:
                f = a[np.isfinite(a)]
                assert np.array_equal(f, np.rint(f)) and (np.abs(f) <= 3).all()
    return c


def _rows(p, z, tab, off, ld, w, idx, bs):
    r = np.arange(p.M) if idx is None else idx[:p.M]
    return tab[off + z * bs + r[:, None] * ld + np.arange(w)[None, :]].astype(np.float64)


def _weights(p, z):
    """W of batch z as [n, k] float64"""
    n_i, k_i = np.arange(p.n)[:, None], np.arange(p.k)[None, :]
    at = k_i * p.ldw + n_i if p.w_kmajor else n_i * p.ldw + k_i
    return p.w[p.w_off + z * p.w_bs + at].astype(np.float64)


def reference(p):
    """(ref, mag), both [nbatch, M, n] float64: the contract's values and the magnitude sums the gaussian bound scales
    with, mag = |alpha| (|A| |W| + |bias rs| + |bias2|) + |old|"""
    ref = np.zeros((p.nbatch, p.M, p.n))
    mag = np.zeros_like(ref)
    old = output_positions(p)
    for z in range(p.nbatch):
        A = _rows(p, z, p.a0, p.a0_off, p.a0_ld, p.a0_w, p.idx0, p.a0_bs)
        if p.a1 is not None:
            A = np.concatenate([A, _rows(p, 0, p.a1, p.a1_off, p.a1_ld, p.a1_w, p.idx1, 0)], axis=1)
        W = _weights(p, z)
        be = np.zeros((p.M, p.n))
        if p.bias is not None:
            b = p.bias[z * p.bias_bs:z * p.bias_bs + p.n].astype(np.float64)[None, :]
            if p.bias_rs is not None:
                b = b * p.bias_rs[np.arange(p.M) * p.ld_brs + z].astype(np.float64)[:, None]
            be = be + b
        bm = np.abs(be)
        if p.bias2 is not None:
            b2 = p.bias2.astype(np.float64)[None, :] * (p.bias2_valid[:p.M] != 0)[:, None]
            be, bm = be + b2, bm + np.abs(b2)
        v = p.alpha * (A @ W.T + be)
        g = abs(p.alpha) * (np.abs(A) @ np.abs(W).T + bm)
        if p.relu:
            v = np.maximum(v, 0.0)
        if p.row_valid is not None:
            v = v * (p.row_valid[:p.M] != 0)[:, None]
        if p.relu_mask is not None:
            v = v * (p.relu_mask[np.arange(p.M)[:, None] * p.ld_mask + np.arange(p.n)[None, :]] > 0)
        if p.accumulate:
            o = p.arena[old[z]].astype(np.float64)
            v, g = v + o, g + np.abs(o)
        ref[z], mag[z] = v, g
    return ref, mag


def output_positions(p):
    """[nbatch, M, n] flat arena positions of the outputs"""
    orow = (np.arange(p.M) if p.c_rows is None else p.c_rows[:p.M]).astype(np.int64)
    z = np.arange(p.nbatch, dtype=np.int64)[:, None, None]
    return p.c_off + z * p.c_bs + orow[None, :, None] * p.ldc + np.arange(p.n, dtype=np.int64)[None, None, :]


def compare(p, ref, mag, after):
    """`after`: the arena after the call (flat float32).  Everything but the outputs keeps its bits; the outputs are
    finite and equal the reference (integer data: exactly) or lie within (k + 4) 2^-24 mag of it, element by element.
    Returns the worst fraction of that bound (0 for integer data)."""
    assert after.shape == p.arena.shape and after.dtype == np.float32
    pos = output_positions(p)
    untouched = np.ones(after.size, dtype=bool)
    untouched[pos.reshape(-1)] = False
    assert after.size - int(untouched.sum()) == pos.size, 'two outputs share an address: the case is wrong'
    same = after.view(np.int32)[untouched] == p.arena.view(np.int32)[untouched]
    if not same.all():
        where = np.flatnonzero(untouched)[~same]
        raise AssertionError(f'{p.case.id}: {len(where)} floats outside the outputs were written, first at arena offsets '
                             f'{where[:6].tolist()} (outputs start at {p.c_off}, ldc {p.ldc})')
    got = after[pos]
    bad = np.argwhere(~np.isfinite(got))
    assert bad.size == 0, (p.case.id, 'non-finite outputs [batch, row, column]', len(bad), bad[:6].tolist())
    if p.kind == 'int':
        exact = ref.astype(np.float32)
        assert np.array_equal(exact.astype(np.float64), ref), 'the reference is not representable: the case is wrong'
        bad = np.argwhere(got != exact)
        assert bad.size == 0, (p.case.id, 'wrong outputs [batch, row, column]', len(bad), bad[:6].tolist(),
                               got[tuple(bad[0])], exact[tuple(bad[0])])
        return 0.0
    bound = (p.k + 4) * U24 * mag
    err = np.abs(got.astype(np.float64) - ref)
    over = np.argwhere(err > bound)
    frac = float((err / np.maximum(bound, np.finfo(np.float64).tiny)).max()) if err.size else 0.0
    assert over.size == 0, (p.case.id, 'fraction of the bound', frac, len(over), over[:6].tolist())
    return frac
