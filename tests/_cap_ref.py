"""Sizes, inputs and references of the tests that run the capped-grid kernels past their caps
(tests/test_cap_ref_host.py, tests/test_hip_past_grid_cap.py, tests/test_hip_decoder_tiles.py).

A kernel with a capped grid loops over the rest of its input: past the cap a workgroup takes a second tile or index.
Every size here is `cap * per_block + r`: r = 0 is the last size without a second pass, r > 0 a ragged second pass of
r items.  The references are numpy, float64 torch or the host twins of the library; nothing here touches a GPU."""
import numpy as np

from _append_ref import stream

# ---- the caps, each with the source line it mirrors ------------------------------------------------------------------
FLAT_BLOCKS = 4096     # tg_common.h: flat_grid(): `if (g > 256 * 16) g = 256 * 16;`
DEC_FWD_TILES = 1024   # tg_decoder.hip: tg_decoder_fwd: `std::min<int64_t>(cdiv(n, DEC_ROWS), 1024)`
DEC_BWD_PARTS = 256    # tg_decoder.hip: dec_bwd_parts(): `std::min<int64_t>(cdiv(n, DEC_ROWS), 256)`
DEC_ROWS = 64          # tg_decoder.hip: `constexpr int DEC_ROWS = 64;`
DEC_KC = 192           # tg_decoder.hip: `constexpr int DEC_KC = 192;`
DEC_H1, DEC_H2 = 80, 10   # tg_decoder.hip: `constexpr int DEC_H1 = 80, DEC_H2 = 10;`
DEC_PART = 904         # tg_decoder.hip: `constexpr int DEC_PART = 904;` (floats of a workgroup's partial sums)
AUC_TILE = 4096        # tg_decoder.hip: `constexpr int AUC_TILE = 4096;`

# work items a block of 256 threads takes at the launch site: flat_grid(items, per_block)
PER_THREAD = 256       # one item per thread
PER_16_LANES = 16      # sixteen lanes per item: k_sample_recent_edges<16>
PER_WAVE = 4           # one wavefront per item

CAP_THREAD = FLAT_BLOCKS * PER_THREAD      # 2^20 items: k_degree (EVENTS, tg_build.hip: `flat_grid(E, 256)`), k_tcsr_fill and
#                                            k_adv_* (ENTRIES P = 2 E: `flat_grid(P, 256)`), k_mark, k_mark_flags, k_hits,
#                                            k_time_encode, k_gather_rows, k_memory_scatter, k_trajectory_finish
CAP_16_LANES = FLAT_BLOCKS * PER_16_LANES  # 65 536 queries: k_sample_recent_edges<16>
CAP_WAVE = FLAT_BLOCKS * PER_WAVE          # 16 384 items: k_sample_recent_edges<64>, k_sample_recent_nodes, k_seen_mask,
#                                            k_anon_reindex, k_anon_reindex2, k_bm_emit (bitmap words)
CAP_DEC_FWD = DEC_FWD_TILES * DEC_ROWS     # 65 536 rows
CAP_DEC_BWD = DEC_BWD_PARTS * DEC_ROWS     # 16 384 rows


def past(cap, r):
    """r items past the cap: a ragged second pass, far from a full one"""
    assert 0 < r < cap // 100
    return cap + r


def last_multiple(cap, unit):
    """the largest multiple of `unit` (a row of the input) that is at most `cap`: exactly the cap where unit divides it"""
    return cap // unit * unit


# name -> (blocks at the cap, items per block, items `at` the cap - the last size without a second pass -, items `past`)
SIZES = {
    'tcsr_entries': (FLAT_BLOCKS, PER_THREAD, CAP_THREAD, past(CAP_THREAD, 300)),             # P = 2 E: k_tcsr_fill, k_adv_*
    'tcsr_events': (FLAT_BLOCKS, PER_THREAD, CAP_THREAD, past(CAP_THREAD, 150)),              # E: k_degree
    'wave_queries': (FLAT_BLOCKS, PER_WAVE, CAP_WAVE, past(CAP_WAVE, 5)),
    'lane16_queries': (FLAT_BLOCKS, PER_16_LANES, CAP_16_LANES, past(CAP_16_LANES, 5)),
    'trajectory': (FLAT_BLOCKS, PER_THREAD, last_multiple(CAP_THREAD, 128), past(CAP_THREAD, 8 * 128)),   # n_nodes * d
    'mark_ids': (FLAT_BLOCKS, PER_THREAD, CAP_THREAD, past(CAP_THREAD, 300)),
    'bitmap_words': (FLAT_BLOCKS, PER_WAVE, CAP_WAVE, past(CAP_WAVE, 6)),
    'hits': (FLAT_BLOCKS, PER_THREAD, last_multiple(CAP_THREAD, 40), past(CAP_THREAD, 3424)),             # B * K
    'row_float4s': (FLAT_BLOCKS, PER_THREAD, last_multiple(CAP_THREAD, 43), past(CAP_THREAD, 4924)),      # n * width / 4
    'time_encode': (FLAT_BLOCKS, PER_THREAD, last_multiple(CAP_THREAD, 172), past(CAP_THREAD, 624)),      # n * d
    'dec_fwd_rows': (DEC_FWD_TILES, DEC_ROWS, CAP_DEC_FWD, past(CAP_DEC_FWD, 17)),
    'dec_bwd_rows': (DEC_BWD_PARTS, DEC_ROWS, CAP_DEC_BWD, past(CAP_DEC_BWD, 1)),
}

# T-CSR build and adversarial index: E events give P = 2 E entries
TCSR_N = 3000
TCSR_E_AT, TCSR_E_PAST = SIZES['tcsr_entries'][2] // 2, SIZES['tcsr_entries'][3] // 2      # 2^19, 2^19 + 150
# k_degree loops over the events: its cap is E = 2^20, where the entry kernels are in their second and third pass
TCSR_DEG_E_AT, TCSR_DEG_E_PAST = SIZES['tcsr_events'][2:]                                   # 2^20, 2^20 + 150
# samplers and seen mask
Q_WAVE_AT, Q_WAVE_PAST = SIZES['wave_queries'][2:]                                          # 16 384, 16 384 + 5
Q_LANE16_AT, Q_LANE16_PAST = SIZES['lane16_queries'][2:]                                    # 65 536, 65 536 + 5
# trajectory finish
TRAJ_D = 128
TRAJ_NODES_AT, TRAJ_NODES_PAST = (v // TRAJ_D for v in SIZES['trajectory'][2:])             # 8 192, 8 200
# bitmap and flags: ids marked, and nodes (64 per bitmap word)
MARK_IDS_AT, MARK_IDS_PAST = SIZES['mark_ids'][2:]                                          # 2^20, 2^20 + 300
BM_NODES_AT = SIZES['bitmap_words'][2] * 64                                                 # 1 048 576: 16 384 words
BM_NODES_PAST = (SIZES['bitmap_words'][3] - 1) * 64 + 3                                     # 1 048 576 + 323: 16 390 words
# hits
HITS_K = 40
HITS_B_AT, HITS_B_PAST = (v // HITS_K for v in SIZES['hits'][2:])                           # 26 214, 26 300 rows
# gather_rows / memory_scatter: width 172 = 43 float4s
ROW_W = 172
ROWS_AT, ROWS_PAST = (v // (ROW_W // 4) for v in SIZES['row_float4s'][2:])                  # 24 385, 24 500 rows
ROW_TABLE = 30000
# time_encode
TE_D = 172
TE_ROWS_AT, TE_ROWS_PAST = (v // TE_D for v in SIZES['time_encode'][2:])                    # 6 096, 6 100 rows
# decoder
DEC_FWD_N = (CAP_DEC_FWD, past(CAP_DEC_FWD, 17), 2 * CAP_DEC_FWD + DEC_ROWS * 3 + 1)
DEC_BWD_N = (CAP_DEC_BWD, past(CAP_DEC_BWD, 1), 2 * CAP_DEC_BWD + DEC_ROWS + 1, past(CAP_DEC_FWD, 17))
DEC_D_TILES = (8, 172, 196)    # one chunk; one chunk with a ragged 16-wide block; two chunks re-staged per tile
DEC_D_EDGES = (4, DEC_KC - 4, DEC_KC, DEC_KC + 4, 2 * DEC_KC, 2 * DEC_KC + 4, 512)
DEC_N_EDGES = (15, 16, 17, DEC_ROWS, DEC_ROWS + 1)
AUC_N = (AUC_TILE - 1, AUC_TILE, AUC_TILE + 1, 2 * AUC_TILE + 1)


# ---- graphs ----------------------------------------------------------------------------------------------------------
def tcsr_stream(E):
    """E events over TCSR_N nodes: a hub, floored (duplicate) timestamps, self loops (_append_ref.stream)"""
    return stream(TCSR_N, E, seed=E % 1000, hub=7)


def oracle_arrays(g):
    """OracleGraph -> (indptr, ts, nbr, eid) in the layout of tg_tcsr_build_host: eid carries the direction in bit 31"""
    eid = (g.eid.astype(np.int64) | (g.dir.astype(np.int64) << 31)).astype(np.uint32).view(np.int32)
    return g.indptr.astype(np.int64), g.ts.astype(np.float64), g.nbr.astype(np.int32), eid


def small_graph(seed=3):
    """A few thousand events for the sampler cases (the size under test is Q): 400 nodes, duplicate timestamps, self
    loops, node 0 and some others without entries.  -> (N, src, dst, ts, eids)"""
    N, E = 400, 4000
    rs = np.random.RandomState(seed)
    src, dst = rs.randint(1, N - 20, E).astype(np.int64), rs.randint(1, N - 20, E).astype(np.int64)
    heavy = rs.uniform(size=E) < 0.2   # node 9 has a long list: the binary search goes deep
    src[heavy] = 9
    loops = rs.uniform(size=E) < 0.05
    dst[loops] = src[loops]
    ts = np.floor(np.sort(rs.uniform(0, E / 3.0, E)))
    eids = np.arange(1, E + 1, dtype=np.int64)
    return N, src, dst, ts, eids


def queries(N, Q, t_max, seed):
    """Q queries: random nodes and times, among them times equal to an event's (the strict cut), times before and after
    everything; the last five (the ragged second pass) are ordinary non-empty queries of the heavy node and others"""
    rs = np.random.RandomState(seed)
    q = rs.randint(0, N, Q).astype(np.int64)
    t = np.floor(rs.uniform(-2, t_max + 3, Q) * 2) / 2   # half of them whole numbers: equal to event times
    q[-5:] = (9, 9, 17, 33, 9)
    t[-5:] = (t_max + 1, t_max / 2, t_max, t_max / 3, 50.0)
    return q, t


def seen_case(B):
    """B queries (16 384 or 16 384 + 5) over _topk_ref.seen_graph() with the catalogue of seen_queries(): the hand-made queries
    first, then random sources (with and without entries, inside and outside the catalogue) at random times, half of them
    an entry's own time (the strict cut).  -> (src, ts, cat, rows): `rows` are the 200 rows that are also checked against
    the numpy loop - the last five, which are the ragged second pass, among them."""
    from _topk_ref import seen_queries
    s0, t0, cat = seen_queries()
    rs = np.random.RandomState(11)
    src = rs.choice(np.array([1, 2, 3, 4, 4, 4, 5, 10, 17, 25, 36, 40], dtype=np.int64), B)
    ts = np.floor(rs.uniform(0, 104, B) * 2) / 2
    src[:len(s0)], ts[:len(s0)] = s0, t0
    src[-5:], ts[-5:] = (4, 3, 2, 1, 10), (60.0, 33.0, 20.5, 1000.0, 1000.0)
    rows = np.sort(np.concatenate([rs.choice(B - 5, 195, replace=False), np.arange(B - 5, B)]))
    return src, ts, cat, rows


# ---- decoder: float64 chain, float32 emulation in the kernels' order ---------------------------------------------------
def decoder_inputs(n, d, seed, keep1=None, p=0.0, margin=1e-4):
    """x [n, d], dy [n], the six parameters (nn.Linear's default ranges), all float32.  Rows of x are redrawn until no
    pre-activation of the float64 forward lies within `margin` of zero: a float32 forward then takes the same side of
    every ReLU as the float64 reference (its pre-activations are off by about 1e-6 at most), so the comparison measures
    rounding and not a flipped unit.  keep1 [n, 80], p: the first dropout mask, which the second pre-activation depends on."""
    rs = np.random.RandomState(seed)
    u = lambda fan_in, *shape: rs.uniform(-1, 1, shape).astype(np.float32) / np.float32(np.sqrt(fan_in))
    params = [u(d, DEC_H1, d), u(d, DEC_H1), u(DEC_H1, DEC_H2, DEC_H1), u(DEC_H1, DEC_H2), u(DEC_H2, 1, DEC_H2), u(DEC_H2, 1)]
    x = rs.standard_normal((n, d)).astype(np.float32)
    dy = rs.standard_normal(n).astype(np.float32)
    w = [t.astype(np.float64) for t in params]
    bad = np.arange(n)
    for _ in range(50):
        z1 = x[bad].astype(np.float64) @ w[0].T + w[1]
        a1 = np.maximum(z1, 0) if keep1 is None else np.maximum(z1, 0) * keep1[bad] / (1.0 - p)
        z2 = a1 @ w[2].T + w[3]
        close = (np.abs(z1) < margin).any(1) | (np.abs(z2) < margin).any(1)
        bad = bad[close]
        if not len(bad):
            break
        x[bad] = rs.standard_normal((len(bad), d)).astype(np.float32)
    assert not len(bad)
    return x, dy, params


def decoder_chain(x, dy, params, masks=None, p=0.0, dtype=np.float64):
    """Forward and backward of the decoder in `dtype`, every intermediate kept.  masks = (keep1 [n, 80], keep2 [n, 10]) or
    None.  In float64 this is the reference (test_cap_ref_host.py checks it against torch autograd); in float32 it is the
    first half of the emulation: the per-row arithmetic, rounded as a float32 kernel rounds it."""
    f = lambda a: np.asarray(a, dtype=dtype)
    w1, b1, w2, b2, w3, b3 = (f(t) for t in params)
    x, dy = f(x), f(dy)
    scale = dtype(1.0 / (1.0 - p)) if masks is not None else dtype(1.0)
    m1 = f(masks[0]) * scale if masks is not None else dtype(1.0)
    m2 = f(masks[1]) * scale if masks is not None else dtype(1.0)
    z1 = x @ w1.T + b1
    r1 = (z1 > 0) * m1                      # the factor of unit j: 0, or 1 / (1 - p) where it is kept
    a1 = z1 * r1
    z2 = a1 @ w2.T + b2
    r2 = (z2 > 0) * m2
    a2 = z2 * r2
    y = a2 @ w3[0] + b3[0]
    dz2 = dy[:, None] * w3[0][None, :] * r2
    dz1 = (dz2 @ w2) * r1
    dx = dz1 @ w1
    return dict(x=x, dy=dy, z1=z1, z2=z2, a1=f(a1), a2=f(a2), y=y, dz2=f(dz2), dz1=f(dz1), dx=dx)


def decoder_grads64(c):
    """the six weight gradients of a float64 chain, summed in float64 -> dict(w1, b1, w2, b2, w3, b3)"""
    return dict(w1=c['dz1'].T @ c['x'], b1=c['dz1'].sum(0), w2=c['dz2'].T @ c['a1'], b2=c['dz2'].sum(0),
                w3=(c['dy'] @ c['a2'])[None, :], b3=c['dy'].sum(keepdims=True))


def _sum_rows_in_order_f32(terms):
    """float32 sum over axis 0 in row order, one rounding per addition (the order of k_decoder_bwd_w1's one thread)"""
    acc = np.zeros(terms.shape[1:], dtype=np.float32)
    for row in terms:
        acc += row
    return acc


def decoder_sums_f32(c):
    """The weight-gradient sums of tg_decoder_bwd evaluated in float32 on the chain c (float32) in the documented order:
    dW2, db2, dW3, db3, db1 per workgroup over its tiles (workgroup b of `parts` takes tiles b, b + parts, ...) in row
    order, then the partials added in workgroup order; dW1 over all rows in row order.  Products are rounded before they
    are added (the kernel fuses them: the factor 4 of the bound covers that)."""
    assert c['x'].dtype == np.float32
    n = len(c['x'])
    ntile = -(-n // DEC_ROWS)
    parts = min(ntile, DEC_BWD_PARTS)
    per = {'w2': lambda r: c['dz2'][r][:, :, None] * c['a1'][r][:, None, :], 'b2': lambda r: c['dz2'][r],
           'w3': lambda r: c['dy'][r][:, None] * c['a2'][r], 'b3': lambda r: c['dy'][r][:, None], 'b1': lambda r: c['dz1'][r]}
    shape = {'w2': (DEC_H2, DEC_H1), 'b2': (DEC_H2,), 'w3': (DEC_H2,), 'b3': (1,), 'b1': (DEC_H1,)}
    acc = {k: np.zeros((parts,) + shape[k], dtype=np.float32) for k in per}
    b = np.arange(parts)
    for s in range(-(-ntile // parts)):
        for rl in range(DEC_ROWS):
            rows = (b + s * parts) * DEC_ROWS + rl
            live = rows < n
            if not live.any():
                continue
            for k, f in per.items():
                acc[k][live] += f(rows[live])
    out = {k: _sum_rows_in_order_f32(a) for k, a in acc.items()}   # the partials, in workgroup order
    out['w3'] = out['w3'][None, :]
    w1 = np.zeros((DEC_H1, c['x'].shape[1]), dtype=np.float32)
    buf = np.empty_like(w1)
    for i in range(n):
        np.multiply(c['dz1'][i][:, None], c['x'][i][None, :], out=buf)
        w1 += buf
    out['w1'] = w1
    return out


def decoder_emulation(x, dy, params, masks=None, p=0.0):
    """the float32 emulation of tg_decoder_fwd / tg_decoder_bwd -> dict(y, dx, w1, b1, w2, b2, w3, b3)"""
    c = decoder_chain(x, dy, params, masks, p, np.float32)
    return dict(decoder_sums_f32(c), y=c['y'], dx=c['dx'])


def decoder_reference(x, dy, params, masks=None, p=0.0):
    """the same in float64 numpy (the GPU tests take float64 torch autograd; test_cap_ref_host.py checks the two equal)"""
    c = decoder_chain(x, dy, params, masks, p, np.float64)
    return dict(decoder_grads64(c), y=c['y'], dx=c['dx'])


GRAD_NAMES = ('w1', 'b1', 'w2', 'b2', 'w3', 'b3')


def worst(a, b):
    """max |a - b| over the elements"""
    return float(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).max()) if np.size(a) else 0.0


# ---- AUC ---------------------------------------------------------------------------------------------------------------
def auc_scores(n, seed):
    """float32 scores over both signs with the largest finite floats, denormals, both zeros and heavy ties; labels with
    both classes.  -> (scores, labels)"""
    rs = np.random.RandomState(seed)
    big, tiny = np.finfo(np.float32).max, np.float32(1e-45)
    pool = np.array([big, -big, tiny, -tiny, 3 * tiny, np.finfo(np.float32).tiny, 0.0, -0.0, 1.0, -1.0, 0.5, 0.5, 0.5],
                    dtype=np.float32)
    s = rs.standard_normal(n).astype(np.float32)
    pick = rs.uniform(size=n) < 0.6
    s[pick] = pool[rs.randint(0, len(pool), int(pick.sum()))]
    lab = (rs.uniform(size=n) < 0.4).astype(np.float32)
    lab[0], lab[-1] = 1, 0
    s[-1] = big   # the last key of the last (one-key, at n = k AUC_TILE + 1) tile is the largest one
    return s, lab
