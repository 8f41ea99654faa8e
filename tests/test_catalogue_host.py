"""Catalogue snapshots without a GPU: the new library entries are bound, their argument checks that need no device refuse
before any launch, and the Python interface has the agreed shape."""
import ctypes as C
import inspect

import pytest


def score_params(hit, n_hit_rows=0, emb=True):
    """a tg_score_params whose pointers are non-null but never dereferenced: every call below is refused before a launch"""
    from www2023tiger_amd._lib import TgLinear, TgScoreParams
    p = C.c_void_p(16)
    return TgScoreParams(hit, n_hit_rows, p if emb else None, TgLinear(p, p), TgLinear(p, p))


def test_the_new_symbols_resolve_and_the_abi_is_9():
    from www2023tiger_amd import _lib
    for name in ('tg_rank_cand_half', 'tg_rank_scores_shared_workspace_bytes', 'tg_rank_scores_shared'):
        assert name in _lib.SIGNATURES
        assert getattr(_lib.lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert _lib.lib.tg_abi_version() == 9
    assert len(_lib.SIGNATURES['tg_rank_cand_half'][1]) == 7 and len(_lib.SIGNATURES['tg_rank_scores_shared'][1]) == 16


def test_workspace_bytes():
    from www2023tiger_amd._lib import lib
    none, cnt = score_params(0), score_params(3, 11)
    assert lib.tg_rank_scores_shared_workspace_bytes(7, 172, C.byref(none)) >= 7 * 172 * 4
    assert lib.tg_rank_scores_shared_workspace_bytes(7, 172, C.byref(cnt)) >= (7 + 22) * 172 * 4
    assert lib.tg_rank_scores_shared_workspace_bytes(-1, 172, C.byref(none)) == 0
    assert lib.tg_rank_scores_shared_workspace_bytes(7, 0, C.byref(none)) == 0
    assert lib.tg_rank_scores_shared_workspace_bytes(7, 8, None) == 0


def shared(B, Cn, d, K, sp, *, h_src=16, P=16, nbr_src=16, nbr_cat=16, src=16, cat=16, scores=16, ld=None, ws=16, ws_bytes=None):
    from www2023tiger_amd._lib import lib
    v = lambda a: None if a is None else C.c_void_p(a)
    if ws_bytes is None:
        ws_bytes = int(lib.tg_rank_scores_shared_workspace_bytes(max(B, 0), d, C.byref(sp))) if sp is not None else 0
    return lib.tg_rank_scores_shared(B, Cn, d, K, None if sp is None else C.byref(sp), v(h_src), v(P), v(nbr_src), v(nbr_cat),
                                     v(src), v(cat), v(scores), Cn if ld is None else ld, v(ws), ws_bytes, None)


def test_tg_rank_scores_shared_refuses_bad_arguments_before_any_launch():
    from www2023tiger_amd._lib import TG_EINVAL, TG_EUNSUPPORTED, TG_OK, lib
    none, vec, cnt, bn = score_params(0), score_params(1), score_params(3, 7), score_params(2, 2)
    assert shared(-1, 4, 8, 5, none) == TG_EINVAL                      # negative sizes
    assert shared(3, -1, 8, 5, none) == TG_EINVAL
    assert shared(3, 4, 0, 5, none) == TG_EINVAL
    assert shared(3, 4, 8, -1, none) == TG_EINVAL
    assert shared(3, 4, 8, 5, None) == TG_EINVAL
    assert shared(1 << 16, 1 << 15, 8, 5, none) == TG_EINVAL           # B C = 2^31
    assert shared(1 << 31, 1, 8, 5, none) == TG_EINVAL
    assert shared(3, 4, 8, 5, none, ld=3) == TG_EINVAL                 # ld < C
    for k in ('h_src', 'P', 'scores', 'ws'):                           # pointers every hit type needs
        assert shared(3, 4, 8, 5, none, **{k: None}) == TG_EINVAL, k
    for sp in (bn, cnt, score_params(1)):                              # pointers the hit types need
        for k in ('nbr_src', 'nbr_cat', 'src', 'cat'):
            assert shared(3, 4, 8, 6, sp, **{k: None}) == TG_EINVAL, k
        assert shared(3, 4, 8, 0, sp) == TG_EINVAL                     # hits without neighbours
    assert shared(3, 4, 8, 5, score_params(3, 5)) == TG_EINVAL         # 'count' with fewer rows than classes
    assert shared(3, 4, 8, 5, score_params(2, 1)) == TG_EINVAL
    assert shared(3, 4, 8, 5, score_params(2, 2, emb=False)) == TG_EINVAL
    assert shared(3, 4, 8, 5, score_params(4)) == TG_EINVAL            # no such hit type
    for sp in (cnt, none):                                             # a workspace one byte short
        need = int(lib.tg_rank_scores_shared_workspace_bytes(3, 8, C.byref(sp)))
        assert shared(3, 4, 8, 5, sp, ws_bytes=need - 1) == TG_EINVAL
    assert shared(3, 4, 7, 5, vec) == TG_EUNSUPPORTED                  # 'vec', odd d (2 (d + K) = 24 is aligned)
    assert shared(3, 4, 8, 5, vec) == TG_EUNSUPPORTED                  # 'vec', 2 (d + K) = 26
    assert shared(0, 4, 7, 5, vec) == TG_EUNSUPPORTED                  # before the empty-call shortcut, as tg_rank_scores
    # B = 0 or C = 0: TG_OK, nothing launched - no pointer is looked at
    none_ptrs = dict(h_src=None, P=None, nbr_src=None, nbr_cat=None, src=None, cat=None, scores=None, ws=None, ws_bytes=0)
    assert shared(0, 4, 8, 5, cnt, **none_ptrs) == TG_OK
    assert shared(3, 0, 8, 5, cnt, **none_ptrs) == TG_OK
    assert shared(0, 0, 8, 6, vec, **none_ptrs) == TG_OK


def test_tg_rank_cand_half_refuses_bad_arguments_before_any_launch():
    from www2023tiger_amd._lib import TG_EINVAL, TG_EUNSUPPORTED, TG_OK, lib
    none, vec = score_params(0), score_params(1)
    p = C.c_void_p(16)
    assert lib.tg_rank_cand_half(-1, 8, 5, C.byref(none), p, p, None) == TG_EINVAL
    assert lib.tg_rank_cand_half(1 << 31, 8, 5, C.byref(none), p, p, None) == TG_EINVAL
    assert lib.tg_rank_cand_half(4, 0, 5, C.byref(none), p, p, None) == TG_EINVAL
    assert lib.tg_rank_cand_half(4, 8, -1, C.byref(none), p, p, None) == TG_EINVAL
    assert lib.tg_rank_cand_half(4, 8, 5, None, p, p, None) == TG_EINVAL
    assert lib.tg_rank_cand_half(4, 8, 5, C.byref(none), None, p, None) == TG_EINVAL
    assert lib.tg_rank_cand_half(4, 8, 5, C.byref(none), p, None, None) == TG_EINVAL
    assert lib.tg_rank_cand_half(4, 7, 5, C.byref(vec), p, p, None) == TG_EUNSUPPORTED
    assert lib.tg_rank_cand_half(4, 8, 5, C.byref(vec), p, p, None) == TG_EUNSUPPORTED
    assert lib.tg_rank_cand_half(0, 8, 5, C.byref(none), None, None, None) == TG_OK


def test_signatures():
    from www2023tiger_amd.eval_utils import eval_recommendation
    from www2023tiger_amd.model.tiger import TIGE, TIGER, CatalogueSnapshot
    e = inspect.signature(TIGE.embed_catalogue).parameters
    assert list(e) == ['self', 'cand', 't', 'graph', 'uptodate']
    assert all(e[k].kind is inspect.Parameter.KEYWORD_ONLY and e[k].default is None for k in ('graph', 'uptodate'))
    assert inspect.signature(TIGE.embed_catalogue).return_annotation is CatalogueSnapshot
    assert TIGER.embed_catalogue is TIGE.embed_catalogue
    r = inspect.signature(TIGE.recommend).parameters
    names = list(r)
    assert names[:5] == ['self', 'src_ids', 'ts', 'cand', 'k']
    assert names[-2:] == ['catalogue_at', 'stale_ok']                  # appended behind the existing ones
    assert names[5:-2] == ['mask', 'exclude_seen', 'graph', 'chunk_queries', 'col_of', 'uptodate']
    assert all(r[k].kind is inspect.Parameter.KEYWORD_ONLY for k in names[5:])
    assert r['catalogue_at'].default is None and r['stale_ok'].default is False
    v = inspect.signature(eval_recommendation).parameters
    assert list(v)[-1] == 'catalogue_at' and v['catalogue_at'].default is None
    assert v['catalogue_at'].kind is inspect.Parameter.KEYWORD_ONLY


def test_eval_recommendation_refuses_an_unknown_protocol_before_anything_runs():
    from www2023tiger_amd.eval_utils import eval_recommendation
    with pytest.raises(ValueError, match='batch'):
        eval_recommendation(None, None, None, None, catalogue_at='event')
