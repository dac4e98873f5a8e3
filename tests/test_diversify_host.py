"""CPU: diversified top-k (ebert.h 0.10.0) -- the new symbols, the argument checks that run before
any HIP call, the workspace sizing, the numpy restatement of the greedy selection on a hand-worked
case, and lib.get_user_recs_diverse / its route on a stub.

The GPU paths (the Gram matrix against oracle.restatement, the selection bitwise against
mmr_ref, the end-to-end rules) are covered in test_gpu_diversify.py."""
import ctypes
import os

import numpy as np
import pytest
import torch

from mmr_ref import mmr_ref
from test_explain_host import _StubCatalog, _fake_catalog, _movie

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ebt_mmr_workspace_bytes", "ebt_pool_gram", "ebt_mmr_select", "ebt_mmr_topk")
EBT_EINVAL = -1
P = 1 << 30    # a fake device pointer: never dereferenced by a host check


def test_new_symbols_and_version():
    from robot_ebert_amd import _lib
    lib = _lib.load()
    for s in NEW:
        assert hasattr(lib, s), s
        assert s in _lib._SIGNATURES, s
    assert lib.ebt_version() >= 1000
    with open(os.path.join(ROOT, "include", "ebert.h")) as f:
        header = f.read()
    for s in NEW:
        assert s + "(" in header, s
    assert "0.10.0" in header and "lib.py:51-55" in header and "EBT_MMR_POOL_MAX 512" in header
    assert "#define EBT_NUM_STAGES 10" in header          # no new timer stage
    assert _lib.EBT_MMR_POOL_MAX == 512
    import robot_ebert_amd as ebt
    assert ebt.diversify_topk is ebt.diversify.diversify_topk
    assert ebt.Diversified is ebt.diversify.Diversified
    assert ebt.Diversified._fields == ("rows", "scores", "mmr", "pos")


def test_argument_errors_return_einval_without_a_gpu():
    """Each EBT_EINVAL case of the three entries -- a null pointer, p or k out of range, lam
    outside [0, 1] or NaN, a catalog whose ld < d, a workspace that is too small -- with the
    entry's name first in the message, before any HIP call (the pointers are fake)."""
    from robot_ebert_amd import _lib
    lib = _lib.load()
    cat = ctypes.byref(_fake_catalog())
    nan = float("nan")

    def err():
        return lib.ebt_last_error().decode()

    # ebt_pool_gram(cat, B, rows, p, gram, status, stream)
    good = [cat, 4, P, 100, P, P, None]
    assert lib.ebt_pool_gram(cat, 0, P, 100, P, P, None) == 0          # an empty batch: no launch
    for i in (0, 2, 4, 5):
        a = list(good)
        a[i] = None
        assert lib.ebt_pool_gram(*a) == EBT_EINVAL, i
        assert err() == "ebt_pool_gram: null pointer", (i, err())
    for field in ("data", "gnorm64"):
        assert lib.ebt_pool_gram(ctypes.byref(_fake_catalog(**{field: None})),
                                 *good[1:]) == EBT_EINVAL
        assert err() == "ebt_pool_gram: null pointer"
    assert lib.ebt_pool_gram(ctypes.byref(_fake_catalog(ld=32)), *good[1:]) == EBT_EINVAL
    assert err().startswith("ebt_pool_gram: bad catalog") and "ld=32" in err()
    for p in (0, -1, 513, 100000):
        a = list(good)
        a[3] = p
        assert lib.ebt_pool_gram(*a) == EBT_EINVAL
        assert err().startswith("ebt_pool_gram: bad arguments") and f"p={p}" in err()
    a = list(good)
    a[1] = -1
    assert lib.ebt_pool_gram(*a) == EBT_EINVAL and "B=-1" in err()
    # ebt_mmr_select(gram, rel, rows, B, p, k, lam, status, pos, rows, rel, mmr, stream)
    good = [P, P, P, 4, 100, 10, 0.7, None, P, P, P, P, None]          # (status may be NULL)
    assert lib.ebt_mmr_select(P, P, P, 0, 100, 10, 0.7, None, P, P, P, P, None) == 0
    for i in (0, 1, 2, 8, 9, 10, 11):
        a = list(good)
        a[i] = None
        assert lib.ebt_mmr_select(*a) == EBT_EINVAL, i
        assert err() == "ebt_mmr_select: null pointer", (i, err())
    for p in (0, 513):
        a = list(good)
        a[4] = p
        assert lib.ebt_mmr_select(*a) == EBT_EINVAL
        assert err().startswith("ebt_mmr_select: bad arguments") and f"p={p}" in err()
    for k in (0, -2, 101):
        a = list(good)
        a[5] = k
        assert lib.ebt_mmr_select(*a) == EBT_EINVAL
        assert err() == f"ebt_mmr_select: k={k} is outside [1, p=100]"
    for lam in (-0.001, 1.5, nan, float("inf")):
        a = list(good)
        a[6] = lam
        assert lib.ebt_mmr_select(*a) == EBT_EINVAL
        assert err().startswith("ebt_mmr_select: lam=") and err().endswith("is outside [0, 1]")
    # ebt_mmr_topk(cat, B, rel, rows, p, k, lam, ws, ws_bytes, pos, rows, rel, mmr, status, stream)
    need = lib.ebt_mmr_workspace_bytes(4, 100)
    good = [cat, 4, P, P, 100, 10, 0.7, P, need, P, P, P, P, P, None]
    for i in (0, 2, 3, 7, 9, 10, 11, 12, 13):
        a = list(good)
        a[i] = None
        assert lib.ebt_mmr_topk(*a) == EBT_EINVAL, i
        assert err() == "ebt_mmr_topk: null pointer", (i, err())
    assert lib.ebt_mmr_topk(ctypes.byref(_fake_catalog(ld=63)), *good[1:]) == EBT_EINVAL
    assert err().startswith("ebt_mmr_topk: bad catalog") and "ld=63" in err()
    for i, v, pat in ((4, 513, "p=513"), (4, 0, "p=0"), (5, 0, "k=0 is outside [1, p=100]"),
                      (5, 101, "k=101 is outside"), (6, 1.0000001, "is outside [0, 1]"),
                      (6, nan, "is outside [0, 1]"), (1, -4, "B=-4")):
        a = list(good)
        a[i] = v
        assert lib.ebt_mmr_topk(*a) == EBT_EINVAL, (i, v)
        assert err().startswith("ebt_mmr_topk: ") and pat in err(), err()
    for short in (0, need - 1):
        a = list(good)
        a[8] = short
        assert lib.ebt_mmr_topk(*a) == EBT_EINVAL
        assert err() == (f"ebt_mmr_topk: workspace {short} < {need} bytes "
                         "(ebt_mmr_workspace_bytes)")


def test_workspace_bytes():
    """8 B p^2 rounded up to 256: aligned, monotone in B and in p, 0 for invalid sizes."""
    from robot_ebert_amd import _lib
    f = _lib.load().ebt_mmr_workspace_bytes
    Bs = [1, 2, 3, 7, 64, 1000, 4096, 10 ** 7]
    ps = [1, 2, 15, 16, 17, 100, 101, 511, 512]
    for p in ps:
        prev = 0
        for B in Bs:
            b = f(B, p)
            assert b % 256 == 0 and 256 <= b and 8 * B * p * p <= b < 8 * B * p * p + 256, (B, p)
            assert b >= prev
            prev = b
    for B in Bs:
        prev = 0
        for p in ps:
            assert f(B, p) >= prev
            prev = f(B, p)
    assert f(1, 1) == 256 and f(1, 512) == 2 << 20           # one query always fits: 2 MiB
    assert f(4096, 100) == 327_680_000                       # the C3-like request
    assert f(4096, 513) == 0 and f(4096, 0) == 0 and f(0, 100) == 0 and f(-1, 100) == 0
    assert f(2 ** 62, 100) == 0                              # would overflow


def test_python_argument_errors_before_any_device_work():
    from robot_ebert_amd import EbertError, diversify

    class Shard:
        n, n_global, row_offset, device = 500, 1000, 500, None

    rows = torch.zeros((2, 20), dtype=torch.int64)           # host tensors: never reach a launch
    scores = torch.zeros((2, 20), dtype=torch.float64)
    with pytest.raises(EbertError, match="on one device"):
        diversify.diversify_topk(Shard(), scores, rows, 5)
    with pytest.raises(EbertError, match="on one device"):
        diversify.pool_gram(Shard(), rows)

    class Cat:
        n, n_global, row_offset, device, d = 1000, 1000, 0, "cpu", 8

    for lam in (-0.1, 1.01, float("nan")):
        with pytest.raises(EbertError, match=r"outside \[0, 1\]"):
            diversify.diversify_topk(Cat(), scores, rows, 5, lam=lam)
        with pytest.raises(EbertError, match=r"outside \[0, 1\]"):
            diversify.mmr_select(torch.zeros((2, 20, 20), dtype=torch.float64), scores, rows, 5,
                                 lam)
    wide = torch.zeros((2, 513), dtype=torch.int64)
    with pytest.raises(EbertError, match="p=513"):
        diversify.diversify_topk(Cat(), torch.zeros((2, 513), dtype=torch.float64), wide, 5)
    with pytest.raises(EbertError, match="p=513"):
        diversify.pool_gram(Cat(), wide)
    for k in (0, 21):
        with pytest.raises(EbertError, match=f"k={k} is outside"):
            diversify.diversify_topk(Cat(), scores, rows, k)
    with pytest.raises(EbertError, match=r"\[B, p\]"):
        diversify.diversify_topk(Cat(), scores, rows[0], 5)
    with pytest.raises(EbertError, match="no CPU path"):     # the last host check
        diversify.diversify_topk(Cat(), scores, rows, 5)


def test_mmr_ref_on_a_hand_worked_case():
    """Four candidates, lam = 0.5: slot 1 is a near copy of slot 0 (cosine 0.9).
    t = 0: v = (.5, .45, .4, .25): slot 0. pen = (1, .9, .1, 0).
    t = 1: v_1 = .45 - .45 = 0, v_2 = .4 - .05 = .35, v_3 = .25: slot 2. pen = (., .9, ., .5).
    t = 2: v_1 = 0, v_3 = .25 - .25 = 0: a tie, the lower position: slot 1.
    t = 3: slot 3 (its pen stays .5: S(1, 3) = 0)."""
    S = np.array([[1.0, 0.9, 0.1, 0.0], [0.9, 1.0, 0.2, 0.0], [0.1, 0.2, 1.0, 0.5],
                  [0.0, 0.0, 0.5, 1.0]])
    rel = np.array([1.0, 0.9, 0.8, 0.5])
    rows = np.array([40, 41, 42, 43])
    pos, r, s, v = mmr_ref(S, rel, rows, 4, 0.5)
    assert pos.tolist() == [0, 2, 1, 3] and r.tolist() == [40, 42, 41, 43]
    assert s.tolist() == [1.0, 0.8, 0.9, 0.5]
    assert v[0] == 0.5 and abs(v[1] - 0.35) < 1e-15 and v[2] == 0.0 and v[3] == 0.0
    # lam = 1: the pool's order; lam = 0: the first, then the least similar to those picked
    assert mmr_ref(S, rel, rows, 3, 1.0)[0].tolist() == [0, 1, 2]
    assert mmr_ref(S, rel, rows, 3, 0.0)[0].tolist() == [0, 3, 2]
    # an empty slot and a NaN relevance are no candidates; the tail is -1 / -1 / NaN / NaN
    pos, r, s, v = mmr_ref(S, np.array([1.0, np.nan, 0.8, 0.5]), np.array([40, 41, -1, 43]), 4, 0.5)
    assert pos.tolist() == [0, 3, -1, -1] and r.tolist() == [40, 43, -1, -1]
    assert np.isnan(s[2:]).all() and np.isnan(v[2:]).all() and v[1] == 0.25
    assert pos.dtype == np.int32 and r.dtype == np.int64


# ------------------------------------------------------- lib.get_user_recs_diverse, on a stub ----
@pytest.fixture
def stub_lib(monkeypatch):
    from sqlalchemy import create_engine, insert
    from sqlalchemy.pool import StaticPool
    from robot_ebert_amd import diversify, lib, tables
    cat = _StubCatalog()
    engine = create_engine("sqlite://", connect_args={"check_same_thread": False},
                           poolclass=StaticPool)
    tables.ratings.create(engine)
    ratings = [("9", 5.0), ("10", 4.0), ("404", 5.0), ("2", 1.0), ("33", 3.5)]
    with engine.begin() as cnx:
        for t, rt in ratings:
            cnx.execute(insert(tables.ratings).values(user_id="u", tmdb_id=t, rating=rt))
        cnx.execute(insert(tables.ratings).values(user_id="cold", tmdb_id="2", rating=1.0))
    calls = {}
    # the pool: rows 5, 2, 8, 6, 7 = ids "4", "100", "7", "55", "6", scores descending
    rows = torch.tensor([[5, 2, 8, 6, 7, -1]])
    scores = torch.tensor([[0.9, 0.8, 0.7, 0.6, 0.5, float("nan")]], dtype=torch.float64)

    def score_topk(c, k, liked=None, exclude=None, **kw):
        calls["score"] = (k, liked, exclude, kw)
        return scores[:, :k], rows[:, :k]

    def diversify_topk(c, s, r, k, lam=0.7, ws_budget=1 << 30):
        calls["diversify"] = (tuple(r.shape), k, lam)
        order = [p for p in (0, 3, 1, 4, 2, 5) if p < r.shape[1]][:k]   # the stub's "selection"
        pos = torch.tensor([order], dtype=torch.int32)
        return diversify.Diversified(r[:, order], s[:, order], s[:, order] * lam, pos)

    monkeypatch.setattr(lib, "score_topk", score_topk)
    monkeypatch.setattr(diversify, "diversify_topk", diversify_topk)
    monkeypatch.setattr(lib, "engine", engine)
    monkeypatch.setattr(lib, "movies_collab_catalog", cat)
    return lib, cat, calls


def test_get_user_recs_diverse_selection_order_and_id_pairing(stub_lib, monkeypatch):
    lib, cat, calls = stub_lib
    # get_movies answers ORDER BY tmdb_id, not in the order asked for
    monkeypatch.setattr(lib, "_get_movies_override", lambda ids: [_movie(t) for t in sorted(ids)])
    got = lib.get_user_recs_diverse("u", k=4, lam=0.5, pool=6)
    liked = calls["score"][1][0]
    assert sorted(liked) == sorted(cat.rows_of(["9", "10", "33"]))        # get_user_recs' sets
    assert sorted(calls["score"][2][0]) == sorted(cat.rows_of(["9", "10", "2", "33"]))
    assert calls["score"][0] == 6 and calls["score"][3] == {}
    assert calls["diversify"] == ((1, 6), 4, 0.5)
    # selection order (pool positions 0, 3, 1, 4), each movie with ITS relevance
    assert [(g.movie.tmdb_id, g.score) for g in got] == [("4", 0.9), ("55", 0.6), ("100", 0.8),
                                                         ("6", 0.5)]
    # the pool defaults to min(10 k, 512, catalog rows) = the stub's 10 rows
    lib.get_user_recs_diverse("u", k=4)
    assert calls["score"][0] == 10 and calls["diversify"][1:] == (4, 0.7)
    lib.get_user_recs_diverse("u", k=1)
    assert calls["score"][0] == 10
    # k beyond the pool: the pool's width; an empty slot (-1) is dropped
    got = lib.get_user_recs_diverse("u", k=9, pool=6)
    assert calls["diversify"][1] == 6
    assert [g.movie.tmdb_id for g in got] == ["4", "55", "100", "6", "7"]
    # a weighting goes to the search, as in get_user_recs
    lib.get_user_recs_diverse("u", k=2, weighting=lib.weight_centered)
    rws, w = calls["score"][1][0], calls["score"][3]["liked_weights"][0]
    weight = {"9": 1.5, "10": 0.5, "2": -2.5}
    assert sorted(rws) == sorted(cat.rows_of(list(weight)))
    assert w == [weight[cat.id_of(r)] for r in rws]


def test_a_missing_movie_is_dropped_not_shifted(stub_lib, monkeypatch):
    """`movies` lacks "55" (SURVEY a-8): the others keep their own scores and their order."""
    lib, cat, calls = stub_lib
    monkeypatch.setattr(lib, "_get_movies_override",
                        lambda ids: [_movie(t) for t in sorted(ids) if t != "55"])
    got = lib.get_user_recs_diverse("u", k=4, lam=0.5, pool=6)
    assert [(g.movie.tmdb_id, g.score) for g in got] == [("4", 0.9), ("100", 0.8), ("6", 0.5)]


def test_diverse_errors_match_get_user_recs(stub_lib, monkeypatch):
    lib, cat, calls = stub_lib
    monkeypatch.setattr(lib, "_get_movies_override", lambda ids: [_movie(t) for t in sorted(ids)])
    assert lib.get_user_recs_diverse("nobody") == [] and lib.get_user_recs("nobody") == []
    with pytest.raises(ValueError, match="0 sample") as ei:               # no liked movie
        lib.get_user_recs_diverse("cold")
    with pytest.raises(ValueError) as ei0:
        lib.get_user_recs("cold")
    assert str(ei.value) == str(ei0.value)
    assert "diversify" not in calls                                       # raised before the GPU


def test_route(monkeypatch):
    from fastapi.testclient import TestClient
    from robot_ebert_amd import api, lib
    from robot_ebert_amd.models import Recommendation
    paths = {rt.path for rt in api.router.routes}
    assert "/users/{user_id}/recommendations/diverse/" in paths
    assert "/users/{user_id}/recommendations/explained/" in paths
    assert "/users/{user_id}/recommendations/" in paths
    calls = []

    def fake(user_id, k=10, lam=0.7, pool=None, weighting=None):
        calls.append((user_id, k, lam, pool))
        if user_id == "nolike":
            raise ValueError("Found array with 0 sample(s)")
        return [Recommendation(movie=_movie(str(i)), score=1.0 - i / 10) for i in range(k)]
    monkeypatch.setattr(lib, "get_user_recs_diverse", fake)
    c = TestClient(api.app(), raise_server_exceptions=False)
    url = "/users/u1/recommendations/diverse/"
    got = c.get(url)
    assert got.status_code == 200 and len(got.json()) == 10 and calls[-1] == ("u1", 10, 0.7, None)
    got = c.get(url, params={"k": 2, "lam": 0.25, "pool": 50}).json()
    assert calls[-1] == ("u1", 2, 0.25, 50) and [x["movie"]["tmdb_id"] for x in got] == ["0", "1"]
    assert c.get(url, params={"lam": 0}).status_code == 200 and calls[-1][2] == 0.0
    assert c.get(url, params={"lam": 1}).status_code == 200
    n = len(calls)
    for bad in ({"lam": 1.5}, {"lam": -0.1}, {"lam": "x"}, {"pool": 0}, {"pool": 513},
                {"k": "x"}):
        assert c.get(url, params=bad).status_code == 422, bad
    assert len(calls) == n                                   # rejected before the handler
    assert c.get("/users/nolike/recommendations/diverse/").status_code == 500
