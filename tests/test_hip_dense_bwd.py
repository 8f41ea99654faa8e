"""tg_linear_bwd (dx = dy W through the k-major weight staging of gemm_tile, dw = dy^T x with db riding on it through
k_gemm_tn / k_tn_reduce, db alone through k_colsum / k_colsum_reduce) against exact and float64 products, at the tile,
chunk and split edges of the three kernels.

Two kinds of data for every shape:
  * integer-valued float32 in {-3 .. 3}: every product and partial sum is an integer below 2^24 (9 * max(n, out_f) < 2^24),
    so the float32 result is exact whatever the summation order, split count or MFMA grouping -> np.array_equal;
  * gaussian times a per-row scale exp(U(-3, 3)): elementwise |got - ref| <= (L + 2) 2^-24 (|A|^T |B|), the any-order
    bound of a length-L float32 inner product (L = n for dw and db, out_f for dx), each element against its own
    magnitude sum - not against the matrix maximum.  The build has -ffp-contract=off and a float32 MFMA rounds no more
    often than separately rounded operations.
The workspace is refilled with NaN before every call (a partial that nobody wrote shows up), and the three outputs lie
in one NaN-filled arena with 64 guard floats around each: guards, and outputs that were not asked for, must keep their
bits.  Run with -s to see the worst observed fraction of the gaussian bound per test."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 64
U24 = 2.0 ** -24
NAN_BITS = 0x7FC00000

# TN_T = 64 (output tile), TN_MC = 32 (rows per staged chunk), BK = 32 (k-tile of gemm_tile).
# weight gradient: splits = max(1, min(ceil(768 / tiles), 16, ceil(n / 64))), rows per split = ceil(n / splits) rounded up to 32
CASES = [
    # -- dw, one 64 x 64 tile: row edges of the chunk-pair loop and of the splits
    (1, 64, 64, 'a tail chunk only'),
    (31, 64, 64, 'one ragged chunk'),
    (32, 64, 64, 'one whole chunk'),
    (33, 64, 64, 'one chunk pair, the second holds one row'),
    (64, 64, 64, 'one whole pair'),
    (65, 64, 64, 'two splits: 64 + 1'),
    (96, 64, 64, 'two splits: 64 + 32'),
    (97, 64, 64, 'two splits: 64 + 33'),
    (128, 64, 64, 'two whole splits'),
    (129, 64, 64, 'three splits: 64, 64, 1'),
    (961, 64, 64, '16 splits, the last holds one row'),
    (1025, 64, 64, '16 splits of 96 rows: ten full, one of 65, five EMPTY (exact zeros)'),
    # -- dw at the benchmarked widths
    (1060, 688, 172, '33 tiles, 16 splits of 96 rows: split 11 has 4 rows, 12-15 are empty'),
    (1060, 1032, 344, '8 splits'),
    # -- ragged columns (n = 70); db comes from the kt == 0 blocks only
    (70, 4, 4, 'the min(n0 + sc, n - 4) clamp on every thread'),
    (70, 4, 68, 'output rows one past a tile'),
    (70, 68, 4, 'input columns one past a tile'),
    (70, 60, 100, 'both ragged, one k-tile'),
    (70, 100, 60, 'both ragged, two k-tiles: db from the first only'),
    (70, 128, 64, 'two whole k-tiles'),
    (70, 172, 344, 'three k-tiles, six row tiles'),
    # -- dx in the generic kernel: K (= out_f) against BK and the depth-2 prefetch (n = 65, in_f = 68)
    (65, 68, 4, 'K far below one k-tile'),
    (65, 68, 28, 'K one float4 short of a k-tile'),
    (65, 68, 32, 'K one whole k-tile'),
    (65, 68, 36, 'K one float4 past a k-tile'),
    (65, 68, 64, 'two k-tiles: one pass of the paired loop'),
    (65, 68, 68, 'two k-tiles and a ragged third'),
    (65, 68, 96, 'three k-tiles: the odd remainder after the paired loop'),
    (65, 68, 172, 'six k-tiles, the last ragged'),
    # -- dx output columns (= in_f) against the 64-wide tile and the N - 4 clamp of wrow (n = 130, out_f = 100)
    (130, 4, 100, 'every weight column clamped'),
    (130, 60, 100, 'one ragged column tile'),
    (130, 64, 100, 'one whole column tile'),
    (130, 68, 100, 'one float4 into the second column tile'),
    (130, 172, 100, 'three column tiles, the last ragged'),
    # -- dx with two k-groups (grid <= 256 and out_f >= 512)
    (100, 172, 516, 'two k-groups, 17 k-tiles, the last holds 4'),
    (1, 4, 512, 'two k-groups, one row, four columns'),
    (63, 60, 540, 'two k-groups, 17 k-tiles with the last one ragged'),
    # -- dx, long K in the generic kernel because the grid is large
    (2100, 688, 516, 'grid of 440 blocks: one k-group over 17 k-tiles'),
    # -- row edges for dx
    (63, 64, 64, 'one row short of a row tile'),
    # -- the shapes every output subset runs on
    (97, 68, 60, 'subset shape: ragged everywhere'),
]
LONG_CASE = (200, 1536, 2048)  # 768 tiles -> ONE split, seven chunks (three pairs and a tail); integer data only
SUBSET_SHAPES = [(97, 68, 60), (1025, 64, 64), (70, 4, 4)]
SUBSETS = ['dx', 'dw', 'dw+db', 'db']
# db alone (colsum_launch): splits = min(ceil(512 / ceil(out_f / 64)), 16, ceil(n / 64)), rows per split NOT rounded
COLSUM_N = [1, 63, 64, 65, 1025]
COLSUM_OUT = [4, 60, 64, 68, 2048]


def dev():
    return torch.device('cuda:0')


def make_data(kind, n, in_f, out_f, seed=0):
    rs = np.random.RandomState((n * 1000003 + in_f * 1009 + out_f + seed * 7919) % (2 ** 31))
    if kind == 'int':
        assert 9 * max(n, out_f) < 2 ** 24
        mk = lambda *s: rs.randint(-3, 4, size=s).astype(np.float32)
    else:
        mk = lambda *s: (rs.standard_normal(s) * np.exp(rs.uniform(-3, 3, (s[0], 1)))).astype(np.float32)
    return mk(n, in_f), mk(out_f, in_f), mk(n, out_f)  # x, w, dy


def reference(x, w, dy):
    """float64 products of the float32 inputs and the magnitude sums the bound scales with"""
    x64, w64, dy64 = x.astype(np.float64), w.astype(np.float64), dy.astype(np.float64)
    ref = {'dx': dy64 @ w64, 'dw': dy64.T @ x64, 'db': dy64.sum(0)}
    mag = {'dx': np.abs(dy64) @ np.abs(w64), 'dw': np.abs(dy64).T @ np.abs(x64), 'db': np.abs(dy64).sum(0)}
    return ref, mag


class Arena:
    """[guard | dx | guard | dw | guard | db | guard], all NaN before the call"""

    def __init__(self, n, in_f, out_f):
        self.shape = {'dx': (n, in_f), 'dw': (out_f, in_f), 'db': (out_f,)}
        self.off, o = {}, GUARD
        for k in ('dx', 'dw', 'db'):
            self.off[k] = o
            o += int(np.prod(self.shape[k])) + GUARD
        self.buf = torch.full((o,), float('nan'), dtype=torch.float32, device=dev())

    def ptr(self, k):
        return self.buf.data_ptr() + 4 * self.off[k]

    def fill(self, k, a):
        self.buf[self.off[k]:self.off[k] + a.size] = torch.from_numpy(np.ascontiguousarray(a).ravel()).to(dev())

    def read(self):
        host = self.buf.cpu().numpy()
        bits = host.view(np.int32)
        out, rest = {}, np.ones(host.size, dtype=bool)
        for k in ('dx', 'dw', 'db'):
            sz = int(np.prod(self.shape[k]))
            out[k] = host[self.off[k]:self.off[k] + sz].reshape(self.shape[k])
            rest[self.off[k]:self.off[k] + sz] = False
        return out, bits, rest


_shared_ws = []  # one buffer for the small shapes, grown on demand


def nan_workspace(in_f, out_f):
    """the workspace tg_linear_bwd_workspace_bytes asks for, every float of it NaN"""
    from www2023tiger_amd._lib import lib
    nbytes = lib.tg_linear_bwd_workspace_bytes(in_f, out_f)
    assert nbytes >= 16 * out_f * (in_f + 1) * 4
    if nbytes > (32 << 20):  # (the 200 MB of LONG_CASE are not kept)
        return torch.full((nbytes // 4,), float('nan'), dtype=torch.float32, device=dev()), nbytes
    if not _shared_ws or _shared_ws[0].numel() < nbytes // 4:
        _shared_ws[:] = [torch.empty(nbytes // 4, dtype=torch.float32, device=dev())]
    ws = _shared_ws[0][:nbytes // 4]
    ws.fill_(float('nan'))
    return ws, nbytes


def call_bwd(arena, x, w, dy, want, with_ws=True):
    """tg_linear_bwd with the outputs in `want` set and the others NULL; x, w, dy: numpy float32"""
    from www2023tiger_amd._lib import check, lib, ptr
    from www2023tiger_amd.hip_ops import stream_ptr
    n, in_f = x.shape
    out_f = w.shape[0]
    xd, wd, dyd = (torch.from_numpy(a).to(dev()) for a in (x, w, dy))
    ws, nbytes = nan_workspace(in_f, out_f) if with_ws else (None, 0)
    check(lib.tg_linear_bwd(n, ptr(xd), in_f, ptr(wd), out_f, ptr(dyd),
                            arena.ptr('dx') if 'dx' in want else None, arena.ptr('dw') if 'dw' in want else None,
                            arena.ptr('db') if 'db' in want else None, ptr(ws), nbytes, stream_ptr(dev())), 'tg_linear_bwd')
    torch.cuda.synchronize()
    for a, b in ((xd, x), (wd, w), (dyd, dy)):  # the inputs are read only
        np.testing.assert_array_equal(a.cpu().numpy(), b)


def check_outputs(arena, kind, x, w, dy, want, untouched_bits=None):
    """every wanted output against its reference; everything else in the arena keeps its bits.  Returns the worst
    fraction of the gaussian bound per output."""
    out, bits, rest = arena.read()
    expect_rest = np.full(bits.shape, NAN_BITS, dtype=np.int32) if untouched_bits is None else untouched_bits
    for k in ('dx', 'dw', 'db'):
        if k not in want:
            sz = int(np.prod(arena.shape[k]))
            rest[arena.off[k]:arena.off[k] + sz] = True
    assert np.array_equal(bits[rest], expect_rest[rest]), 'a guard band or an output that was not asked for was written'
    ref, mag = reference(x, w, dy)
    n, out_f = dy.shape
    worst = {}
    for k in want:
        got = out[k]
        assert np.isfinite(got).all(), (k, 'non-finite values', np.argwhere(~np.isfinite(got))[:4])
        if kind == 'int':
            exact = np.rint(ref[k]).astype(np.int64)  # the float64 product of small integers IS the int64 product
            assert np.array_equal(ref[k], exact.astype(np.float64))
            bad = np.argwhere(got.astype(np.int64) != exact)
            assert np.array_equal(got, exact.astype(np.float32)) and bad.size == 0, (k, len(bad), bad[:6].tolist())
        else:
            L = out_f if k == 'dx' else n
            bound = (L + 2) * U24 * mag[k]
            err = np.abs(got.astype(np.float64) - ref[k])
            frac = float((err / np.maximum(bound, np.finfo(np.float64).tiny)).max())
            worst[k] = frac
            over = np.argwhere(err > bound)
            assert over.size == 0, (k, 'fraction of the bound', frac, len(over), over[:6].tolist())
    return worst


def report(worst):
    if worst:
        print('  WORST fraction of the (L + 2) 2^-24 |A|^T|B| bound: ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()))


def run_case(n, in_f, out_f, kind, want=('dx', 'dw', 'db'), with_ws=True):
    x, w, dy = make_data(kind, n, in_f, out_f)
    arena = Arena(n, in_f, out_f)
    call_bwd(arena, x, w, dy, want, with_ws)
    worst = check_outputs(arena, kind, x, w, dy, want)
    report(worst)
    return worst


@pytest.mark.parametrize('kind', ['int', 'gauss'])
@pytest.mark.parametrize('n,in_f,out_f,why', CASES, ids=[f'{c[0]}x{c[1]}x{c[2]}' for c in CASES])
def test_linear_bwd_all_outputs(n, in_f, out_f, why, kind):
    run_case(n, in_f, out_f, kind)


def test_linear_bwd_one_split_long_chunk_loop():
    """768 tiles: one split that walks all seven chunks (three pairs and a tail); dx runs 64 k-tiles in the generic kernel"""
    run_case(*LONG_CASE, 'int')


@pytest.mark.parametrize('kind', ['int', 'gauss'])
@pytest.mark.parametrize('want', SUBSETS)
@pytest.mark.parametrize('n,in_f,out_f', SUBSET_SHAPES, ids=[f'{c[0]}x{c[1]}x{c[2]}' for c in SUBSET_SHAPES])
def test_linear_bwd_output_subsets(n, in_f, out_f, want, kind):
    """dx only (no workspace at all), dw only, dw + db, db only (k_colsum): what is not asked for is not written"""
    run_case(n, in_f, out_f, kind, tuple(want.split('+')), with_ws=want != 'dx')


@pytest.mark.parametrize('kind', ['int', 'gauss'])
@pytest.mark.parametrize('out_f', COLSUM_OUT)
@pytest.mark.parametrize('n', COLSUM_N)
def test_linear_bwd_bias_only_is_the_column_sum_kernel(n, out_f, kind):
    """db alone: 1 .. 16 splits of unrounded row counts, 1 .. 32 column tiles, ragged last tile"""
    run_case(n, 8, out_f, kind, ('db',))


@pytest.mark.parametrize('kind', ['int', 'gauss'])
@pytest.mark.parametrize('n,in_f,out_f', SUBSET_SHAPES, ids=[f'{c[0]}x{c[1]}x{c[2]}' for c in SUBSET_SHAPES])
def test_linear_bwd_second_call_overwrites(n, in_f, out_f, kind):
    """a second call with other data, outputs still holding the first result: dw and db are overwritten, nothing
    accumulates in the outputs or survives in the (NaN-refilled) workspace"""
    arena = Arena(n, in_f, out_f)
    x, w, dy = make_data(kind, n, in_f, out_f)
    call_bwd(arena, x, w, dy, ('dx', 'dw', 'db'))
    check_outputs(arena, kind, x, w, dy, ('dx', 'dw', 'db'))
    x2, w2, dy2 = make_data(kind, n, in_f, out_f, seed=1)
    assert not np.array_equal(dy, dy2)
    call_bwd(arena, x2, w2, dy2, ('dx', 'dw', 'db'))
    report(check_outputs(arena, kind, x2, w2, dy2, ('dx', 'dw', 'db')))
    # ... and a third that asks for db alone leaves dx and dw of the second call as they are
    _, before, _ = arena.read()
    call_bwd(arena, x, w, dy, ('db',))
    check_outputs(arena, kind, x, w, dy, ('db',), untouched_bits=before.copy())
