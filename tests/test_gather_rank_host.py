"""CPU-only checks of the gathered score head's boundary (include/tiger_hip.h: tg_rank_scores_gathered): the symbols
resolve, the ABI version stands, the workspace size, the argument refusals that need no device, CatalogueSnapshot.col_of on
host tensors, and the header as C."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE, VEC, BIN, COUNT = 0, 1, 2, 3   # TG_HIT_*


def score_params(hit_type, n_hit_rows, arrays):
    from www2023tiger_amd._lib import TgLinear, TgScoreParams, ptr
    return TgScoreParams(hit_type, n_hit_rows, ptr(arrays['emb']), TgLinear(ptr(arrays['w1']), ptr(arrays['b1'])),
                         TgLinear(ptr(arrays['w2']), ptr(arrays['b2'])))


def host_arrays(d=8, K=4, B=3, Cn=5, Cq=6):
    z = lambda *s: np.zeros(s, np.float32)
    return dict(emb=z(K + 1, d), w1=z(d, 2 * (d + K)), b1=z(d), w2=z(1, d), b2=z(1), h_src=z(B, d), P=z(Cn, d),
                nbr_src=np.zeros((B, K), np.int64), nbr_cat=np.zeros((Cn, K), np.int64), src=np.zeros(B, np.int64),
                cat=np.zeros(Cn, np.int64), col=np.zeros((B, Cq), np.int32), scores=np.full((B, Cq), 7.0, np.float32))


def test_the_new_symbols_resolve_and_the_abi_version_stands():
    """(fails without the feature: the library has no tg_rank_scores_gathered)"""
    from www2023tiger_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ('tg_rank_scores_gathered', 'tg_rank_scores_gathered_workspace_bytes'):
        assert hasattr(raw, name) and name in _lib.SIGNATURES
        assert callable(getattr(_lib.lib, name))
    assert _lib.lib.tg_abi_version() == 9


def test_workspace_bytes_is_monotone_and_zero_on_bad_arguments():
    from www2023tiger_amd._lib import lib
    a = host_arrays()
    sizes = []
    for hit_type, rows in ((NONE, 0), (BIN, 2), (COUNT, 5)):
        sp = score_params(hit_type, rows, a)
        f = lambda B, d: int(lib.tg_rank_scores_gathered_workspace_bytes(B, d, C.byref(sp)))
        got = [f(B, 8) for B in (0, 1, 2, 31, 32, 33, 1000)]
        assert got == sorted(got) and len(set(got)) == len(got)
        assert f(5, 8) >= (5 + 2 * rows) * 8 * 4 and f(5, 16) > f(5, 8)
        assert f(5, 8) == int(lib.tg_rank_scores_shared_workspace_bytes(5, 8, C.byref(sp)))
        assert f(-1, 8) == 0 and f(5, 0) == 0 and f(5, -8) == 0
        sizes.append(f(5, 8))
    assert sizes == sorted(sizes) and sizes[0] < sizes[2]   # more class rows, more table bytes
    assert int(lib.tg_rank_scores_gathered_workspace_bytes(5, 8, None)) == 0


def test_argument_refusals_come_before_any_device_call():
    """host arrays stand in for device memory: a refused call dereferences nothing and writes nothing"""
    from www2023tiger_amd._lib import TG_EINVAL, TG_EUNSUPPORTED, TG_OK, lib, ptr
    d, K, B, Cn, Cq = 8, 4, 3, 5, 6
    a = host_arrays(d, K, B, Cn, Cq)
    sp = score_params(COUNT, K + 1, a)
    need = int(lib.tg_rank_scores_gathered_workspace_bytes(B, d, C.byref(sp)))
    ws = np.zeros(need, np.uint8)

    def call(B=B, Cn=Cn, Cq=Cq, d=d, K=K, sp=sp, ld=Cq, ws_bytes=need, **null):
        p = {k: (None if null.pop(k, 1) is None else ptr(v)) for k, v in dict(a, ws=ws).items()}
        assert not null
        return lib.tg_rank_scores_gathered(B, Cn, Cq, d, K, None if sp is None else C.byref(sp), p['h_src'], p['P'],
                                           p['nbr_src'], p['nbr_cat'], p['src'], p['cat'], p['col'], p['scores'], ld, p['ws'],
                                           ws_bytes, None)

    for kw in (dict(B=-1), dict(Cn=-1), dict(Cq=-1), dict(d=0), dict(K=-1), dict(sp=None), dict(ld=Cq - 1),
               dict(Cn=2 ** 31 - 1), dict(B=2 ** 20, Cq=2 ** 11, ld=2 ** 11), dict(col=None), dict(scores=None),
               dict(h_src=None), dict(P=None), dict(ws=None), dict(nbr_src=None), dict(nbr_cat=None), dict(src=None),
               dict(cat=None), dict(K=0), dict(ws_bytes=need - 1)):
        assert call(**kw) == TG_EINVAL, kw
    assert call(sp=score_params(COUNT, K, a)) == TG_EINVAL      # 'count' needs K + 1 class rows
    assert call(sp=score_params(BIN, 1, a)) == TG_EINVAL        # 'bin' needs 2
    assert call(sp=score_params(7, 0, a)) == TG_EINVAL          # no such hit type
    assert call(sp=score_params(BIN, 2, dict(a, emb=None))) == TG_EINVAL
    assert call(sp=score_params(NONE, 0, dict(a, w1=None))) == TG_EINVAL
    vec = score_params(VEC, 0, a)
    assert call(sp=vec, d=7, K=5) == TG_EUNSUPPORTED        # an odd d
    assert call(sp=vec, d=8, K=5) == TG_EUNSUPPORTED        # 2 (d + K) = 26
    assert call(B=0) == TG_OK and call(Cq=0, ld=0) == TG_OK
    assert call(B=0, col=None, scores=None, h_src=None, P=None, ws=None) == TG_OK   # nothing to do: nothing is looked at
    assert (a['scores'] == 7.0).all()


class _Owner:
    pass


class _Graph:
    def __init__(self, n):
        self.num_node = n


def test_col_of_maps_ids_to_rows_and_refuses_duplicates():
    from www2023tiger_amd.model.tiger import CatalogueSnapshot
    owner = _Owner()
    ids = torch.tensor([7, 0, 3, 11], dtype=torch.int64)
    snap = CatalogueSnapshot(owner, ids, torch.zeros(4, 8), None, 5.0, _Graph(12), None)
    col_of = snap.col_of
    assert col_of.dtype == torch.int32 and col_of.shape == (12,) and col_of.device.type == 'cpu'
    want = np.full(12, -1, np.int32)
    want[[7, 0, 3, 11]] = np.arange(4)
    np.testing.assert_array_equal(col_of.numpy(), want)
    assert snap.col_of is col_of                                   # built once
    sub = torch.tensor([[3, 5, 11], [0, 7, 7]])
    np.testing.assert_array_equal(col_of[sub].numpy(), [[2, -1, 3], [1, 0, 0]])
    empty = CatalogueSnapshot(owner, ids[:0], torch.zeros(0, 8), None, 5.0, _Graph(12), None)
    assert (empty.col_of == -1).all() and empty.col_of.shape == (12,)
    twice = CatalogueSnapshot(owner, torch.tensor([7, 3, 7]), torch.zeros(3, 8), None, 5.0, _Graph(12), None)
    with pytest.raises(ValueError, match='duplicate'):
        twice.col_of
    with pytest.raises(ValueError, match='duplicate'):            # and again: a failed build is not cached as a success
        twice.col_of


def test_the_header_still_compiles_as_c(tmp_path):
    """gcc, C99, every warning an error: the two prototypes are assigned to function pointers of the documented types
    (inside sizeof: type-checked, never linked), and the program prints the ABI version"""
    src = tmp_path / 'gathered.c'
    src.write_text('#include <stdio.h>\n#include "tiger_hip.h"\n'
                   'typedef size_t (*ws_fn)(int64_t, int32_t, const tg_score_params*);\n'
                   'typedef int (*run_fn)(int64_t, int64_t, int64_t, int32_t, int32_t, const tg_score_params*, const float*,\n'
                   '                      const float*, const int64_t*, const int64_t*, const int64_t*, const int64_t*,\n'
                   '                      const int32_t*, float*, int64_t, void*, size_t, void*);\n'
                   'int main(void) {\n  ws_fn a = 0;\n  run_fn b = 0;\n'
                   '  printf("%d %d\\n", TG_ABI_VERSION, (int)(sizeof(a = tg_rank_scores_gathered_workspace_bytes) ==\n'
                   '                                          sizeof(b = tg_rank_scores_gathered)));\n  return 0;\n}\n')
    exe = tmp_path / 'gathered'
    subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)],
                   check=True)
    assert subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split() == ['9', '1']
