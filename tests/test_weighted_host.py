"""CPU: per-row weights on liked-row queries (ebert.h 0.8.0) -- the new symbols, the argument
checks that need no GPU, distributed.split_liked's weights and W_b, RecBatcher.submit's
per-request checks and the two weighting helpers of lib.py.

The weighted score is sum_l w_l cos(x_l, x) / sum_l |w_l|; the oracle of the batcher test is
built from oracle.restatement (cosine_similarity, topk_from_scores). The GPU paths are covered in
test_gpu_weighted.py."""
import ctypes
import math
import os

import numpy as np
import pytest

from oracle import restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "robot_ebert_amd", "libebert.so")
NEW = ("ebt_query_liked_wsum", "ebt_cosine_topk_weighted", "ebt_cosine_topk_weighted_submit",
       "ebt_cosine_topk_sharded_weighted", "ebt_cosine_topk_sharded_weighted_submit")


def test_new_symbols_and_version():
    from robot_ebert_amd import _lib
    lib = _lib.load()
    for s in NEW:
        assert hasattr(lib, s), s
        assert s in _lib._SIGNATURES, s
    assert lib.ebt_version() >= 800
    with open(os.path.join(ROOT, "include", "ebert.h")) as f:
        header = f.read()
    for s in NEW:
        assert s + "(" in header, s
    assert "0.8.0" in header and "lib.py:47-52" in header


def test_weighted_entries_reject_bad_arguments_without_a_gpu():
    """Host checks that run before any HIP call: NULL pointers of ebt_query_liked_wsum, and an
    invalid catalog of the _weighted entries (EBT_EINVAL = -1 and a message)."""
    h = ctypes.CDLL(LIB)
    h.ebt_last_error.restype = ctypes.c_char_p
    VP, I32, I64, SZ = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_size_t
    h.ebt_query_liked_wsum.argtypes = [VP, ctypes.c_int, I32, I64, VP, I64, VP, VP, VP, VP, VP]
    assert h.ebt_query_liked_wsum(None, 3, 8, 8, None, 1, None, None, None, None, None) == -1
    assert b"ebt_query_liked_wsum" in h.ebt_last_error()
    h.ebt_cosine_topk_weighted.argtypes = [VP, VP, ctypes.c_int, I64, I64, VP, VP, I32, VP, VP,
                                           VP, VP, SZ, VP, VP, VP, VP, VP, VP]
    assert h.ebt_cosine_topk_weighted(None, None, 0, 1, 0, None, None, 1, None, None, None, None,
                                      0, None, None, None, None, None, None) == -1
    assert h.ebt_last_error() != b""
    h.ebt_cosine_topk_sharded_weighted.argtypes = [VP, VP, VP, ctypes.c_int, I64, I64, VP, VP,
                                                   I32, VP, VP, VP, VP, SZ, VP, VP, VP, VP, VP]
    assert h.ebt_cosine_topk_sharded_weighted(None, None, None, 0, 1, 0, None, None, 1, None,
                                              None, None, None, 0, None, None, None, None,
                                              None) == -1


def test_python_signatures_take_the_keywords():
    import inspect
    from robot_ebert_amd import batcher, distributed, lib, search
    for fn in (search.score_topk, search.score_topk_submit, search.score_topk_stages):
        p = inspect.signature(fn).parameters
        assert p["liked_weights"].default is None and p["liked_wsum"].default is None, fn
    p = inspect.signature(search.prepare_queries).parameters
    assert "liked_weights" in p and "liked_wsum" in p
    assert "liked_weights" in inspect.signature(distributed.score_topk_sharded).parameters
    assert "liked_weights" in inspect.signature(distributed.ShardedTopk.submit).parameters
    assert inspect.signature(batcher.RecBatcher.submit).parameters["weights"].default is None
    for fn in (lib.get_user_recs, lib.get_user_recs_batched):
        assert inspect.signature(fn).parameters["weighting"].default is None


def test_abs_weight_sums_are_sequential():
    """W_b is the left-to-right float64 sum of |w| (what the C host check and the device kernel
    compute), not numpy's pairwise sum."""
    from robot_ebert_amd.search import abs_weight_sums
    rng = np.random.default_rng(0)
    w = rng.standard_normal(1000) * 10.0 ** rng.integers(-8, 8, 1000)
    off = np.array([0, 1, 300, 1000])
    want = []
    for s, e in zip(off[:-1], off[1:]):
        acc = 0.0
        for x in w[s:e]:
            acc += abs(float(x))
        want.append(acc)
    got = abs_weight_sums(off, w)
    assert got.tolist() == want


def test_weight_checks_name_the_query():
    from robot_ebert_amd import EbertError
    from robot_ebert_amd.search import check_weights
    off = np.array([0, 2, 4, 5])
    assert check_weights(off, np.array([1.0, -2.0, 0.5, 0.5, 3.0])).tolist() == [3.0, 1.0, 3.0]
    with pytest.raises(EbertError, match="query 1"):
        check_weights(off, np.array([1.0, -2.0, float("nan"), 0.5, 3.0]))
    with pytest.raises(EbertError, match="query 2"):
        check_weights(off, np.array([1.0, -2.0, 0.5, 0.5, float("inf")]))
    with pytest.raises(EbertError, match="query 0"):
        check_weights(off, np.array([0.0, -0.0, 0.5, 0.5, 3.0]))


def test_split_liked_weights_and_wsum():
    from robot_ebert_amd import EbertError
    from robot_ebert_amd.distributed import split_liked
    liked = [[1, 5, 9, 5], [2], [7, 8]]
    w = [[1.0, -2.0, 0.5, 0.25], [3.0], [-1.0, -1.0]]
    assert split_liked(liked, 0, 6) == ([[1, 5, 5], [2], []], [4, 1, 2])   # unchanged
    local, counts, lw, W = split_liked(liked, 0, 6, w)
    assert local == [[1, 5, 5], [2], []] and counts == [4, 1, 2]
    assert lw == [[1.0, -2.0, 0.25], [3.0], []]
    assert W == [3.75, 3.0, 2.0]       # over the WHOLE list, whatever the shard holds
    local, counts, lw, W2 = split_liked(liked, 6, 10, w)
    assert local == [[9], [], [7, 8]] and lw == [[0.5], [], [-1.0, -1.0]] and W2 == W
    with pytest.raises(EbertError, match="query 1"):
        split_liked(liked, 0, 6, [[1.0, -2.0, 0.5, 0.25], [3.0, 1.0], [-1.0, -1.0]])
    with pytest.raises(EbertError, match="query 2"):
        split_liked(liked, 0, 6, [[1.0, -2.0, 0.5, 0.25], [3.0], [0.0, 0.0]])
    with pytest.raises(EbertError, match="query 0"):
        split_liked(liked, 0, 6, [[1.0, float("nan"), 0.5, 0.25], [3.0], [1.0, 0.0]])
    with pytest.raises(EbertError):
        split_liked(liked, 0, 6, w[:2])


class _Cat:
    def __init__(self, x):
        self.x, self.d, self.n, self.row_offset = x, x.shape[1], x.shape[0], 0


def _weighted_oracle(x, liked, w, k, excl):
    S = R.cosine_similarity(x[liked], x)
    w = np.asarray(w, dtype=np.float64)
    scores = (w[:, None] * S).sum(0) / np.abs(w).sum()
    return R.topk_from_scores(scores, k, excl)


def test_batcher_checks_weights_per_request():
    """A wrong length, a non-finite value or W = 0 fails that request alone; a batch with a
    weighted request carries liked_weights= with 1.0 for its unweighted members, one without
    carries no keyword."""
    from robot_ebert_amd.batcher import RecBatcher
    rng = np.random.default_rng(3)
    cat = _Cat(rng.standard_normal((200, 12)))
    seen = []

    def score(cat, k, liked, exclude, liked_weights=None):
        seen.append(liked_weights)
        ws = liked_weights if liked_weights is not None else [[1.0] * len(l) for l in liked]
        out = [_weighted_oracle(cat.x, l, w, k, e) for l, w, e in zip(liked, ws, exclude)]
        return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])

    b = RecBatcher(cat, max_batch=8, max_wait_ms=200.0, score_fn=score)
    bad = [b.submit([1, 2, 3], [], 5, weights=[1.0, 2.0]),
           b.submit([1, 2, 3], [], 5, weights=[1.0, float("nan"), 2.0]),
           b.submit([1, 2, 3], [], 5, weights=[1.0, float("inf"), 2.0]),
           b.submit([1, 2, 3], [], 5, weights=[0.0, 0.0, -0.0]),
           b.submit([1, 2, 3], [], 5, weights=[1.0, "x", 2.0])]
    good_w = b.submit([4, 9, 17], [9, 30], 5, weights=[2.0, -1.0, 0.5])
    good_u = b.submit([4, 9, 17], [9, 30], 5)
    for f in bad:
        assert isinstance(f.exception(timeout=10), ValueError)
    s, r = good_w.result(timeout=10)
    ws, wr = _weighted_oracle(cat.x, [4, 9, 17], [2.0, -1.0, 0.5], 5, [9, 30])
    np.testing.assert_array_equal(r, wr)
    np.testing.assert_allclose(s, ws, rtol=0, atol=1e-15)
    s, r = good_u.result(timeout=10)
    us, ur = _weighted_oracle(cat.x, [4, 9, 17], [1.0, 1.0, 1.0], 5, [9, 30])
    np.testing.assert_array_equal(r, ur)
    np.testing.assert_allclose(s, us, rtol=0, atol=1e-15)
    # (the two usually share one batch; whichever way they were grouped, the weighted request's
    # batch carried the keyword, with 1.0 for an unweighted member)
    with_kw = [lw for lw in seen if lw is not None]
    assert len(with_kw) == 1 and with_kw[0][0] == [2.0, -1.0, 0.5]
    assert with_kw[0][1:] in ([], [[1.0, 1.0, 1.0]])
    seen.clear()
    b.submit([4, 9], [], 3).result(timeout=10)
    assert seen == [None]           # no weighted member: the call as it always was
    b.close()


def test_weighting_helpers():
    from robot_ebert_amd import lib
    assert lib.LIKED_MOVIE_SCORE == 3.5
    assert [lib.weight_by_rating(r) for r in (0.5, 3.0, 3.5, 4.0, 5.0)] == [0, 0, 3.5, 4.0, 5.0]
    assert [lib.weight_centered(r) for r in (0.5, 3.5, 5.0)] == [-3.0, 0.0, 1.5]
    assert all(isinstance(lib.weight_by_rating(r), float) and math.isfinite(lib.weight_centered(r))
               for r in (0.5, 1, 2.5, 5))


def test_liked_weights_need_liked_rows():
    """Argument errors raised before anything touches a device."""
    from robot_ebert_amd import EbertError, search

    class Cat:   # never reached
        device = None
    with pytest.raises(EbertError, match="liked"):
        search.score_topk_submit(Cat(), 5, queries=object(), liked_weights=[[1.0]])
