"""CPU: explanations (ebert.h 0.9.0) -- the new symbols, the argument checks that run before any
HIP call, the workspace sizing, and the id pairing of lib.get_user_recs_explained on a stub.

The GPU paths (the contribution matrix against oracle.restatement, the selection, the invariants)
are covered in test_gpu_explain.py."""
import ctypes
import datetime
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ebt_explain_workspace_bytes", "ebt_liked_contrib", "ebt_explain_select",
       "ebt_explain_topk")
EBT_EINVAL = -1
P = 1 << 30    # a fake device pointer: never dereferenced by a host check


def _fake_catalog(**kw):
    from robot_ebert_amd import _lib
    f = dict(data=P, dtype=_lib.EBT_F32, d=64, n=1000, ld=64, row_offset=0, gnorm64=P, inv32=P,
             image=P, cscale=None, img_dtype=_lib.EBT_F16, ld_img=64, d_pad=64, native=0,
             u_cat=2.0 ** -11)
    f.update(kw)
    return _lib.EbtCatalog(**f)


def test_new_symbols_and_version():
    from robot_ebert_amd import _lib
    lib = _lib.load()
    for s in NEW:
        assert hasattr(lib, s), s
        assert s in _lib._SIGNATURES, s
    assert lib.ebt_version() >= 900
    with open(os.path.join(ROOT, "include", "ebert.h")) as f:
        header = f.read()
    for s in NEW:
        assert s + "(" in header, s
    assert "0.9.0" in header and "lib.py:51-52" in header and "EBT_EXPLAIN_M_MAX 64" in header
    assert "#define EBT_NUM_STAGES 10" in header          # no new timer stage
    assert _lib.EBT_EXPLAIN_M_MAX == 64
    import robot_ebert_amd as ebt
    assert ebt.explain_topk is ebt.explain.explain_topk
    assert ebt.Explanation._fields == ("contrib", "pos", "liked_row", "total")


def test_argument_errors_return_einval_without_a_gpu():
    """Each EBT_EINVAL case of the three entries -- a null pointer, k < 1, m out of range, a
    workspace that is too small -- with the entry's name in the message, before any HIP call
    (the pointers are fake)."""
    from robot_ebert_amd import _lib
    lib = _lib.load()
    cat = ctypes.byref(_fake_catalog())

    def err():
        return lib.ebt_last_error().decode()

    # ebt_liked_contrib(cat, B, off, rows, w, result rows, k, out, status, stream)
    good = [cat, 4, P, P, None, P, 10, P, P, None]
    for i in (0, 2, 3, 5, 7, 8):
        a = list(good)
        a[i] = None
        assert lib.ebt_liked_contrib(*a) == EBT_EINVAL, i
        assert err() == "ebt_liked_contrib: null pointer", (i, err())
    for field in ("data", "gnorm64"):
        assert lib.ebt_liked_contrib(ctypes.byref(_fake_catalog(**{field: None})),
                                     *good[1:]) == EBT_EINVAL
        assert err() == "ebt_liked_contrib: null pointer"
    for k in (0, -3):
        a = list(good)
        a[6] = k
        assert lib.ebt_liked_contrib(*a) == EBT_EINVAL
        assert err().startswith("ebt_liked_contrib: bad arguments") and f"k={k}" in err()
    assert lib.ebt_liked_contrib(ctypes.byref(_fake_catalog(ld=32)), *good[1:]) == EBT_EINVAL
    assert err().startswith("ebt_liked_contrib: bad catalog")
    # ebt_explain_select(contrib, B, off, rows, k, m, largest, val, pos, row, total, stream)
    good = [P, 4, P, P, 10, 3, 1, P, P, P, None, None]       # (out_total may be NULL)
    for i in (0, 2, 3, 7, 8, 9):
        a = list(good)
        a[i] = None
        assert lib.ebt_explain_select(*a) == EBT_EINVAL, i
        assert err() == "ebt_explain_select: null pointer"
    a = list(good)
    a[4] = 0
    assert lib.ebt_explain_select(*a) == EBT_EINVAL and "k=0" in err()
    for m in (0, -1, 65, 1000):
        a = list(good)
        a[5] = m
        assert lib.ebt_explain_select(*a) == EBT_EINVAL
        assert err() == f"ebt_explain_select: m={m} is outside [1, 64]"
    # ebt_explain_topk(cat, B, off, rows, w, nnz, result rows, k, m, largest, ws, ws_bytes, val,
    #                  pos, row, total, status, stream)
    nnz, k = 340, 10
    need = lib.ebt_explain_workspace_bytes(nnz, k)
    good = [cat, 4, P, P, None, nnz, P, k, 3, 1, P, need, P, P, P, None, P, None]
    for i in (0, 2, 3, 6, 10, 12, 13, 14, 16):
        a = list(good)
        a[i] = None
        assert lib.ebt_explain_topk(*a) == EBT_EINVAL, i
        assert err() == "ebt_explain_topk: null pointer", (i, err())
    for i, v, pat in ((7, 0, "k=0"), (5, -1, "nnz=-1")):
        a = list(good)
        a[i] = v
        assert lib.ebt_explain_topk(*a) == EBT_EINVAL and pat in err(), err()
    for m in (0, 65):
        a = list(good)
        a[8] = m
        assert lib.ebt_explain_topk(*a) == EBT_EINVAL
        assert err() == f"ebt_explain_topk: m={m} is outside [1, 64]"
    for short in (0, need - 1):
        a = list(good)
        a[11] = short
        assert lib.ebt_explain_topk(*a) == EBT_EINVAL
        assert err() == (f"ebt_explain_topk: workspace {short} < {need} bytes "
                         "(ebt_explain_workspace_bytes)")


def test_workspace_bytes():
    """Monotone in nnz and in k, 256-aligned, at least 8 k nnz; 0 for invalid sizes."""
    from robot_ebert_amd import _lib
    lib = _lib.load()
    f = lib.ebt_explain_workspace_bytes
    nnzs = [0, 1, 2, 31, 32, 33, 85, 1000, 4096 * 85, 10 ** 9]
    ks = [1, 2, 3, 10, 17, 100, 101, 4096]
    for k in ks:
        prev = 0
        for nnz in nnzs:
            b = f(nnz, k)
            assert b % 256 == 0 and b >= 8 * k * nnz and b >= 256, (nnz, k, b)
            assert b < 8 * k * nnz + 512
            assert b >= prev
            prev = b
    for nnz in nnzs:
        prev = 0
        for k in ks:
            assert f(nnz, k) >= prev
            prev = f(nnz, k)
    assert f(4096 * 85, 100) == 8 * 100 * 4096 * 85          # the C3-like request: 278.5 MB
    assert f(-1, 10) == 0 and f(10, 0) == 0 and f(10, -1) == 0
    assert f(2 ** 62, 100) == 0                               # would overflow


def test_python_argument_errors_before_any_device_work():
    from robot_ebert_amd import EbertError, explain

    class Shard:
        n, n_global, row_offset, device = 500, 1000, 500, None

    with pytest.raises(EbertError, match="on one device"):
        explain.explain_topk(Shard(), None, [[1]])
    with pytest.raises(EbertError, match="on one device"):
        explain.liked_contrib(Shard(), None, [[1]])

    class Cat:
        n, n_global, row_offset, device, d = 1000, 1000, 0, "cpu", 8

    for m in (0, 65):
        with pytest.raises(EbertError, match="outside"):
            explain.explain_topk(Cat(), None, [[1]], m=m)
    with pytest.raises(EbertError, match="query 1"):
        explain.explain_topk(Cat(), None, [[1], [2, 3]], liked_weights=[[1.0], [1.0]])
    with pytest.raises(EbertError, match="query 0"):
        explain.explain_topk(Cat(), None, [[1], [2, 3]], liked_weights=[[0.0], [1.0, 1.0]])
    with pytest.raises(EbertError, match="weight lists"):
        explain.explain_topk(Cat(), None, [[1], [2, 3]], liked_weights=[[1.0]])
    with pytest.raises(ValueError, match="0 sample"):
        explain.explain_topk(Cat(), None, [[1], []])


# ---------------------------------------------------------------- the id pairing, on a stub ----
class _StubCatalog:
    """Ten movies whose string ids sort differently from their rows ("10" < "9")."""
    d, row_offset = 4, 0

    def __init__(self):
        self.ids = [str(v) for v in (9, 10, 100, 2, 33, 4, 55, 6, 7, 81)]
        self.n = self.n_global = len(self.ids)
        self.index_pos = {t: i for i, t in enumerate(self.ids)}

    def rows_of(self, tmdb_ids):
        return [self.index_pos[t] for t in tmdb_ids]

    def id_of(self, row):
        return self.ids[row]


def _movie(t):
    from robot_ebert_amd.models import Movie
    return Movie(tmdb_id=t, tmdb_homepage="", title=t, language="en",
                 release_date=datetime.date(2000, 1, 1), runtime=90, director="d", actors=None,
                 genres=None, keywords=None, overview="", budget=0, revenue=0, popularity=1.0,
                 vote_average=0.0, vote_count=0)


@pytest.fixture
def stub_lib(monkeypatch):
    from sqlalchemy import create_engine, insert
    from sqlalchemy.pool import StaticPool
    from robot_ebert_amd import explain, lib, tables
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
    # rows 5, 2, 8, 6 = ids "4", "100", "7", "55", scores descending in that order
    rows = torch.tensor([[5, 2, 8, 6, -1]])
    scores = torch.tensor([[0.9, 0.8, 0.7, 0.6, float("nan")]], dtype=torch.float64)

    def score_topk(c, k, liked=None, exclude=None, **kw):
        calls["score"] = (k, liked, exclude, kw)
        return scores, rows

    def explain_topk(c, r, liked, liked_weights=None, m=3, largest=True):
        calls["explain"] = (r, liked, liked_weights, m)
        L = len(liked[0])
        # result slot j's best positions are (j, j + 1, ...) mod L; value 0.1 (j + 1) / (t + 1)
        pos = torch.tensor([[[(j + t) % L if t < L else -1 for t in range(m)]
                             for j in range(5)]], dtype=torch.int32)
        val = torch.tensor([[[0.1 * (j + 1) / (t + 1) if t < L else float("nan")
                              for t in range(m)] for j in range(5)]], dtype=torch.float64)
        pos[0, 4], val[0, 4] = -1, float("nan")
        lr = torch.where(pos >= 0, torch.tensor(liked[0])[pos.clamp(min=0).long()], -1)
        return explain.Explanation(val, pos, lr, scores)

    monkeypatch.setattr(lib, "score_topk", score_topk)
    monkeypatch.setattr(explain, "explain_topk", explain_topk)
    monkeypatch.setattr(lib, "engine", engine)
    monkeypatch.setattr(lib, "movies_collab_catalog", cat)
    return lib, cat, calls


def test_get_user_recs_explained_pairs_reasons_by_id(stub_lib, monkeypatch):
    lib, cat, calls = stub_lib
    monkeypatch.setattr(lib, "_get_movies_override", lambda ids: [_movie(t) for t in sorted(ids)])
    got = lib.get_user_recs_explained("u", k=5, m=2)
    # the liked list is lib.py:47's: catalog movies rated >= 3.5, in the order of the fetch
    liked = calls["score"][1][0]
    assert sorted(liked) == sorted(cat.rows_of(["9", "10", "33"]))
    assert calls["score"][0] == 5 and calls["score"][3] == {}
    assert sorted(calls["score"][2][0]) == sorted(cat.rows_of(["9", "10", "2", "33"]))
    assert calls["explain"][1:] == ([liked], None, 2)
    assert [g.movie.tmdb_id for g in got] == ["4", "100", "7", "55"]
    assert [g.score for g in got] == [0.9, 0.8, 0.7, 0.6]
    rating = {"9": 5.0, "10": 4.0, "33": 3.5}
    for j, g in enumerate(got):        # result slot j: positions j, j + 1 of the liked list
        want = [cat.id_of(liked[(j + t) % 3]) for t in range(2)]
        assert [r.tmdb_id for r in g.reasons] == want, (j, g.reasons)
        assert [r.contribution for r in g.reasons] == [0.1 * (j + 1), 0.1 * (j + 1) / 2]
        assert [r.rating for r in g.reasons] == [rating[t] for t in want]
    # the same movies, scores and order as get_user_recs
    plain = lib.get_user_recs("u", k=5)
    assert [(p.movie.tmdb_id, p.score) for p in plain] == [(g.movie.tmdb_id, g.score) for g in got]
    # m larger than the liked list: three reasons, the padding dropped
    got = lib.get_user_recs_explained("u", k=5, m=5)
    assert all(len(g.reasons) == 3 for g in got)


def test_reasons_follow_their_movie_when_a_movie_row_is_missing(stub_lib, monkeypatch):
    """SURVEY a-8: `movies` lacks a row, get_movies returns one movie fewer and lib.py:58-62's zip
    shifts the scores down the id-sorted list -- as the reference does, and as get_user_recs
    does. The reasons were keyed by tmdb_id before that and still sit on their own movie."""
    lib, cat, calls = stub_lib
    monkeypatch.setattr(lib, "_get_movies_override",
                        lambda ids: [_movie(t) for t in sorted(ids) if t != "4"])
    got = lib.get_user_recs_explained("u", k=5, m=1)
    plain = lib.get_user_recs("u", k=5)
    assert [(p.movie.tmdb_id, p.score) for p in plain] == [(g.movie.tmdb_id, g.score) for g in got]
    # sort_index order "100" < "4" < "55" < "7": without "4", "55" takes 4's score and "7" 55's
    assert {g.movie.tmdb_id: g.score for g in got} == {"100": 0.8, "55": 0.9, "7": 0.6}
    liked = calls["score"][1][0]
    slot = {"100": 1, "7": 2, "55": 3}     # the result slot each movie really had
    for g in got:
        j = slot[g.movie.tmdb_id]
        assert [r.tmdb_id for r in g.reasons] == [cat.id_of(liked[j % 3])], g
        assert [r.contribution for r in g.reasons] == [0.1 * (j + 1)]


def test_explained_errors_and_weighting(stub_lib, monkeypatch):
    lib, cat, calls = stub_lib
    monkeypatch.setattr(lib, "_get_movies_override", lambda ids: [_movie(t) for t in sorted(ids)])
    assert lib.get_user_recs_explained("nobody") == []                    # no ratings
    with pytest.raises(ValueError, match="0 sample") as ei:               # no liked movie
        lib.get_user_recs_explained("cold")
    with pytest.raises(ValueError) as ei0:
        lib.get_user_recs("cold")
    assert str(ei.value) == str(ei0.value)
    got = lib.get_user_recs_explained("u", k=5, m=3, weighting=lib.weight_centered)
    # weight_centered: every rated catalog movie with a non-zero weight is a term ("33" is 0)
    rows, w = calls["score"][1][0], calls["score"][3]["liked_weights"][0]
    weight = {"9": 1.5, "10": 0.5, "2": -2.5}
    assert sorted(rows) == sorted(cat.rows_of(list(weight)))
    assert w == [weight[cat.id_of(r)] for r in rows]
    assert calls["explain"][1:] == ([rows], [w], 3)
    rating = {"9": 5.0, "10": 4.0, "2": 1.0}
    assert [r.rating for r in got[0].reasons] == [rating[cat.id_of(r)] for r in rows]


def test_user_terms_are_the_lists_get_user_recs_scores_from(stub_lib):
    """_user_terms keeps the ratings beside the lists of _user_request (weighting None) and
    _user_request_weighted, entry for entry."""
    lib, cat, _ = stub_lib
    liked, rated, w, ratings = lib._user_terms("u", None)
    assert (liked, rated) == lib._user_request("u") and w is None
    assert ratings == [{"9": 5.0, "10": 4.0, "33": 3.5}[cat.id_of(r)] for r in liked]
    liked, rated, w, ratings = lib._user_terms("u", lib.weight_centered)
    assert (liked, rated, w) == lib._user_request_weighted("u", lib.weight_centered)
    assert [lib.weight_centered(r) for r in ratings] == w
    assert lib._user_terms("nobody", None) is None


def test_models_and_route(monkeypatch):
    from fastapi.testclient import TestClient
    from robot_ebert_amd import api, lib
    from robot_ebert_amd.models import ExplainedRecommendation, Reason
    r = Reason(tmdb_id="9", contribution=0.25, rating=4.5)
    e = ExplainedRecommendation(movie=_movie("4"), score=0.5, reasons=[r])
    assert e.reasons[0].tmdb_id == "9" and e.score == 0.5
    paths = {rt.path for rt in api.router.routes}
    assert "/users/{user_id}/recommendations/explained/" in paths
    assert "/users/{user_id}/recommendations/" in paths
    calls = []

    def fake(user_id, k=10, m=3):
        calls.append((user_id, k, m))
        if user_id == "nolike":
            raise ValueError("Found array with 0 sample(s)")
        return [ExplainedRecommendation(movie=_movie(str(i)), score=1.0 - i / 10,
                                        reasons=[r] * m) for i in range(k)]
    monkeypatch.setattr(lib, "get_user_recs_explained", fake)
    c = TestClient(api.app(), raise_server_exceptions=False)
    got = c.get("/users/u1/recommendations/explained/")
    assert got.status_code == 200 and len(got.json()) == 10 and calls[-1] == ("u1", 10, 3)
    got = c.get("/users/u1/recommendations/explained/", params={"k": 2, "m": 1}).json()
    assert calls[-1] == ("u1", 2, 1) and [x["movie"]["tmdb_id"] for x in got] == ["0", "1"]
    assert got[0]["reasons"] == [{"tmdb_id": "9", "contribution": 0.25, "rating": 4.5}]
    assert c.get("/users/nolike/recommendations/explained/").status_code == 500
    assert c.get("/users/u1/recommendations/explained/", params={"m": "x"}).status_code == 422
