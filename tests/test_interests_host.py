"""CPU: multi-interest top-k (ebert.h 0.11.0) -- the new symbols, the argument checks that run
before any HIP call, the workspace sizing, the numpy restatements (tests/interest_ref.py) on
hand-worked cases, lib.get_user_recs_interests / its route on a stub, and the two kernels'
register metadata in the built library.

The GPU paths (the kernels bitwise against interest_ref, the invariances, the oracle, the
end-to-end rules) are covered in test_gpu_interests.py."""
import ctypes
import os

import numpy as np
import pytest
import torch

from interest_ref import cluster_ref, dhondt_seats, interleave_ref, planted
from test_explain_host import _StubCatalog, _fake_catalog, _movie
from test_kernel_resources_host import _gfx950_code_objects, _kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ebt_interest_workspace_bytes", "ebt_interest_cluster", "ebt_liked_interests",
       "ebt_interest_interleave")
EBT_EINVAL = -1
P = 1 << 30    # a fake device pointer: never dereferenced by a host check


def test_new_symbols_and_version():
    from robot_ebert_amd import _lib
    lib = _lib.load()
    for s in NEW:
        assert hasattr(lib, s), s
        assert s in _lib._SIGNATURES, s
    assert lib.ebt_version() >= 1100
    with open(os.path.join(ROOT, "include", "ebert.h")) as f:
        header = f.read()
    for s in NEW:
        assert s + "(" in header, s
    assert "0.11.0" in header and "lib.py:51-52" in header
    assert "#define EBT_NUM_STAGES 10" in header          # no new timer stage
    for name, v in (("EBT_INTEREST_MAX", 8), ("EBT_INTEREST_ITERS", 16),
                    ("EBT_INTEREST_K_MAX", 512)):
        assert f"#define {name} {v} " in header or f"#define {name} {v}\n" in header, name
        assert getattr(_lib, name) == v
    import robot_ebert_amd as ebt
    assert ebt.multi_interest_topk is ebt.interests.multi_interest_topk
    assert ebt.cluster_liked is ebt.interests.cluster_liked
    assert ebt.Interests._fields == ("label", "size", "medoid", "iters", "rows")
    assert ebt.MultiInterest._fields == ("rows", "scores", "cluster", "pos", "size", "medoid_row")


def test_argument_errors_return_einval_without_a_gpu():
    """Each EBT_EINVAL case of the three entries -- a null pointer, p, c or k out of range,
    B < 0, a catalog whose ld < d, a workspace that is too small -- with the entry's name first
    in the message, before any HIP call (the pointers are fake); B == 0 is EBT_OK."""
    from robot_ebert_amd import _lib
    lib = _lib.load()
    cat = ctypes.byref(_fake_catalog())

    def err():
        return lib.ebt_last_error().decode()

    # ebt_interest_cluster(gram, rows, B, p, c, status, label, size, medoid, iters, stream)
    good = [P, P, 4, 100, 3, None, P, P, P, P, None]                   # (status may be NULL)
    assert lib.ebt_interest_cluster(P, P, 0, 100, 3, None, P, P, P, P, None) == 0
    for i in (0, 1, 6, 7, 8, 9):
        a = list(good)
        a[i] = None
        assert lib.ebt_interest_cluster(*a) == EBT_EINVAL, i
        assert err() == "ebt_interest_cluster: null pointer", (i, err())
    for i, v, pat in ((3, 0, "p=0"), (3, -1, "p=-1"), (3, 513, "p=513"), (4, 0, "c=0"),
                      (4, 9, "c=9"), (4, -2, "c=-2"), (2, -1, "B=-1")):
        a = list(good)
        a[i] = v
        assert lib.ebt_interest_cluster(*a) == EBT_EINVAL, (i, v)
        assert err().startswith("ebt_interest_cluster: bad arguments") and pat in err(), err()
    # ebt_liked_interests(cat, B, rows, p, c, ws, ws_bytes, label, size, medoid, iters, status,
    #                     stream)
    need = lib.ebt_interest_workspace_bytes(4, 100)
    good = [cat, 4, P, 100, 3, P, need, P, P, P, P, P, None]
    assert lib.ebt_liked_interests(cat, 0, P, 100, 3, P, 0, P, P, P, P, P, None) == 0
    for i in (0, 2, 5, 7, 8, 9, 10, 11):
        a = list(good)
        a[i] = None
        assert lib.ebt_liked_interests(*a) == EBT_EINVAL, i
        assert err() == "ebt_liked_interests: null pointer", (i, err())
    for field in ("data", "gnorm64"):
        assert lib.ebt_liked_interests(ctypes.byref(_fake_catalog(**{field: None})),
                                       *good[1:]) == EBT_EINVAL
        assert err() == "ebt_liked_interests: null pointer"
    assert lib.ebt_liked_interests(ctypes.byref(_fake_catalog(ld=63)), *good[1:]) == EBT_EINVAL
    assert err().startswith("ebt_liked_interests: bad catalog") and "ld=63" in err()
    for i, v, pat in ((3, 513, "p=513"), (3, 0, "p=0"), (4, 0, "c=0"), (4, 9, "c=9"),
                      (1, -4, "B=-4")):
        a = list(good)
        a[i] = v
        assert lib.ebt_liked_interests(*a) == EBT_EINVAL, (i, v)
        assert err().startswith("ebt_liked_interests: bad arguments") and pat in err(), err()
    for short in (0, need - 1):
        a = list(good)
        a[6] = short
        assert lib.ebt_liked_interests(*a) == EBT_EINVAL
        assert err() == (f"ebt_liked_interests: workspace {short} < {need} bytes "
                         "(ebt_interest_workspace_bytes)")
    # ebt_interest_interleave(size, list_rows, list_scores, B, c, k, rows, scores, cluster, pos,
    #                         stream)
    good = [P, P, P, 4, 3, 10, P, P, P, P, None]
    assert lib.ebt_interest_interleave(P, P, P, 0, 3, 10, P, P, P, P, None) == 0
    for i in (0, 1, 2, 6, 7, 8, 9):
        a = list(good)
        a[i] = None
        assert lib.ebt_interest_interleave(*a) == EBT_EINVAL, i
        assert err() == "ebt_interest_interleave: null pointer", (i, err())
    for i, v, pat in ((4, 0, "c=0"), (4, 9, "c=9"), (5, 0, "k=0"), (5, 513, "k=513"),
                      (5, -1, "k=-1"), (3, -1, "B=-1")):
        a = list(good)
        a[i] = v
        assert lib.ebt_interest_interleave(*a) == EBT_EINVAL, (i, v)
        assert err().startswith("ebt_interest_interleave: bad arguments") and pat in err(), err()


def test_workspace_bytes_equal_the_mmr_sizing():
    from robot_ebert_amd import _lib
    lib = _lib.load()
    f, g = lib.ebt_interest_workspace_bytes, lib.ebt_mmr_workspace_bytes
    for B in (-1, 0, 1, 2, 7, 64, 4096, 10 ** 7, 2 ** 62):
        for p in (-1, 0, 1, 15, 16, 17, 85, 100, 511, 512, 513):
            assert f(B, p) == g(B, p), (B, p)
    assert f(1, 512) == 2 << 20 and f(4096, 85) == 4096 * 85 * 85 * 8 and f(4096, 513) == 0


def test_python_argument_errors_before_any_device_work():
    from robot_ebert_amd import EbertError, interests

    class Shard:
        n, n_global, row_offset, device, d = 500, 1000, 500, None, 8

    with pytest.raises(EbertError, match="on one device"):
        interests.cluster_liked(Shard(), [[501, 502]])
    with pytest.raises(EbertError, match="on one device"):
        interests.multi_interest_topk(Shard(), 5, [[501, 502]])

    class Cat:
        n, n_global, row_offset, device, d = 1000, 1000, 0, "cpu", 8

    for c in (0, 9, -1):
        with pytest.raises(EbertError, match=f"c={c} clusters is outside"):
            interests.cluster_liked(Cat(), [[1, 2]], c=c)
        with pytest.raises(EbertError, match=f"c={c} clusters is outside"):
            interests.multi_interest_topk(Cat(), 5, [[1, 2]], c=c)
    for k in (0, 513):
        with pytest.raises(EbertError, match=f"k={k} is outside"):
            interests.multi_interest_topk(Cat(), k, [[1, 2]])
    with pytest.raises(ValueError, match=r"Found array with 0 sample\(s\) \(shape=\(0, 8\)\)"):
        interests.cluster_liked(Cat(), [[1, 2], []])
    with pytest.raises(EbertError, match="query 1: 513 liked rows"):
        interests.cluster_liked(Cat(), [[1, 2], list(range(513))])
    for bad in (1000, -1, 10 ** 12):
        with pytest.raises(EbertError, match="query 2: a liked row is outside"):
            interests.cluster_liked(Cat(), [[1, 2], [5], [3, bad]])
    with pytest.raises(EbertError, match="exclude holds 1 lists for 2 queries"):
        interests.multi_interest_topk(Cat(), 5, [[1, 2], [3]], exclude=[[4]])
    with pytest.raises(EbertError, match="no CPU path"):      # the last host check
        interests.cluster_liked(Cat(), [[1, 2], [3]])
    with pytest.raises(EbertError, match="no CPU path"):
        interests.interleave(torch.zeros((1, 3), dtype=torch.int32),
                             torch.zeros((1, 3, 4), dtype=torch.int64),
                             torch.zeros((1, 3, 4), dtype=torch.float64))


# ------------------------------------------------------------- interest_ref, hand-worked ----
def _two_groups():
    """Six slots: 0, 1, 2 and 3, 4, 5 are two obvious groups (0.9 inside, 0.1 across; slot 1 and
    slot 4 are the most central: 0.95 to their neighbours)."""
    S = np.full((6, 6), 0.1)
    S[:3, :3] = S[3:, 3:] = 0.9
    S[0, 1] = S[1, 0] = S[1, 2] = S[2, 1] = 0.95
    S[3, 4] = S[4, 3] = S[4, 5] = S[5, 4] = 0.95
    np.fill_diagonal(S, 1.0)
    return S


def test_cluster_ref_two_obvious_groups():
    """tot = (2.15, 2.2, 2.15, ...): slots 1 and 4 tie, the lower position seeds; the farthest
    row from it (0.1: slots 3, 4, 5 tie, the lowest) seeds cluster 1; one pass confirms the
    labels; equal sizes are numbered by their lowest member; the medoids are the central rows."""
    S = _two_groups()
    label, size, medoid, iters = cluster_ref(S, np.arange(6) + 40, 2)
    assert label.tolist() == [0, 0, 0, 1, 1, 1] and size.tolist() == [3, 3]
    assert medoid.tolist() == [1, 4] and iters == 1
    assert label.dtype == np.int32 and size.dtype == np.int32 and medoid.dtype == np.int32
    # c = 1: one cluster, whose medoid is the row with the largest total (the seed)
    label, size, medoid, iters = cluster_ref(S, np.arange(6), 1)
    assert label.tolist() == [0] * 6 and size.tolist() == [6] and medoid.tolist() == [1]
    assert iters == 1
    # the larger cluster comes first whatever its position
    S5, rows5 = S[1:, 1:], np.arange(5)
    label, size, medoid, _ = cluster_ref(S5, rows5, 2)
    assert label.tolist() == [1, 1, 0, 0, 0] and size.tolist() == [3, 2]
    assert medoid.tolist() == [3, 0]      # (0.95 to slot 0 = old slot 1: a tie, the lower)


def test_cluster_ref_ties_by_position_and_by_m():
    """Everything equal: every arg max is decided by position, every assignment by m."""
    S = np.full((4, 4), 0.5)
    label, size, medoid, iters = cluster_ref(S, np.arange(4), 2)
    # seeds 0 and 1; S(seed_m, i) ties -> m = 0, the seed 1 keeps m = 1; then the pass: row 1's
    # means tie (0.5, 0.5) -> m = 0: cluster 1 empties
    assert label.tolist() == [0, 0, 0, 0] and size.tolist() == [4, 0]
    assert medoid.tolist() == [0, -1] and iters == 2
    # -0.0 equals +0.0
    Z = np.zeros((3, 3))
    Z[0, 1] = Z[1, 0] = -0.0
    label, size, medoid, _ = cluster_ref(Z, np.arange(3), 3)
    assert label.tolist() == [0, 0, 0] and size.tolist() == [3, 0, 0]
    assert medoid.tolist() == [0, -1, -1]


def test_cluster_ref_c_above_L_empty_slots_and_an_emptied_cluster():
    S = _two_groups()
    # c > L: two rows, c = 8: each is its own cluster; the rest are empty
    rows = np.array([7, -1, -1, 9, -1, -1])
    M = np.where((rows >= 0)[:, None] & (rows >= 0)[None, :], S, np.nan)
    label, size, medoid, iters = cluster_ref(M, rows, 8)
    assert label.tolist() == [0, -1, -1, 1, -1, -1]
    assert size.tolist() == [1, 1, 0, 0, 0, 0, 0, 0] and medoid.tolist() == [0, 3] + [-1] * 6
    # a -1 slot in the middle changes nothing but the positions
    rows = np.array([40, 41, -1, 42, 43, 44, 45])
    keep = np.array([0, 1, 3, 4, 5, 6])
    M = np.full((7, 7), np.nan)
    M[np.ix_(keep, keep)] = S
    label, size, medoid, iters = cluster_ref(M, rows, 2)
    assert label.tolist() == [0, 0, -1, 0, 1, 1, 1] and size.tolist() == [3, 3]
    assert medoid.tolist() == [1, 5] and iters == 1
    # nothing valid
    label, size, medoid, iters = cluster_ref(np.full((3, 3), np.nan), np.full(3, -1), 2)
    assert label.tolist() == [-1] * 3 and size.tolist() == [0, 0]
    assert medoid.tolist() == [-1, -1] and iters == 0
    # three seeds among two tight groups: a singleton's mean to itself is 1.0, the largest
    # cosine there is, so the third cluster survives (a cluster of rows EQUAL to another's
    # empties instead: the all-equal case of the test above, size [4, 0])
    label, size, medoid, iters = cluster_ref(S, np.arange(6), 3)
    assert sorted(size.tolist(), reverse=True) == size.tolist() and size.sum() == 6
    assert (size > 0).sum() == 3 and set(label.tolist()) == {0, 1, 2}
    # a cluster that empties: rows 1 and 2 are copies (cosine 1.0), row 0 is apart. Seeds 1 (the
    # largest total, the lower of the copies), then 0 (the farthest), then 2; in the first pass
    # row 2's means tie at 1.0 between its copy's cluster and its own: the lower m takes it
    C = np.array([[1.0, 0.2, 0.2], [0.2, 1.0, 1.0], [0.2, 1.0, 1.0]])
    label, size, medoid, iters = cluster_ref(C, np.arange(3), 3)
    assert label.tolist() == [1, 0, 0] and size.tolist() == [2, 1, 0]
    assert medoid.tolist() == [1, 0, -1] and iters == 2


def test_cluster_ref_recovers_planted_groups():
    from oracle import restatement as R
    x, group = planted(0, 3, 32, 85, 0.7)
    label, size, medoid, iters = cluster_ref(R.cosine_similarity(x, x), np.arange(85), 3)
    assert size.tolist() == [29, 28, 28] and iters <= 3
    assert len({(a, b) for a, b in zip(label.tolist(), group.tolist())}) == 3


def test_interleave_ref_hand_worked():
    rows = np.array([[10, 11, 12, 13, 14, 15], [20, 21, 22, 23, 24, 25],
                     [30, 31, 32, 33, 34, 35]])
    scores = rows / 100.0
    # sizes (5, 3, 1), k = 6: quotients 5, 3, 2.5, 1.67, 1.5, 1.25 -> clusters 0 1 0 0 1 0
    r, s, cl, pos = interleave_ref([5, 3, 1], rows, scores, 6)
    assert cl.tolist() == [0, 1, 0, 0, 1, 0] and pos.tolist() == [0, 0, 1, 2, 1, 3]
    assert r.tolist() == [10, 20, 11, 12, 21, 13] and s.tolist() == [.1, .2, .11, .12, .21, .13]
    assert dhondt_seats([5, 3, 1], 6) == [4, 2, 0]
    assert r.dtype == np.int64 and cl.dtype == np.int32 and pos.dtype == np.int32
    # equal quotients go to the lower cluster: sizes (2, 2): 0 1 0 1
    assert interleave_ref([2, 2, 0], rows, scores, 6)[2].tolist() == [0, 1, 0, 1, 0, 1]
    # a duplicate row across lists is emitted once, by the list that reaches it first
    dup = rows.copy()
    dup[1, 0] = 10                       # cluster 1's best is cluster 0's best
    r, s, cl, pos = interleave_ref([5, 3, 1], dup, scores, 6)
    assert r.tolist() == [10, 21, 11, 12, 22, 13] and pos.tolist() == [0, 1, 1, 2, 2, 3]
    assert s[1] == scores[1, 1]
    # an exhausted list hands its slots on; everything exhausted: the tail is empty
    short = np.full((3, 6), -1)
    short[0, :2], short[1, :1], short[2, 3] = [10, 11], [20], 33
    r, s, cl, pos = interleave_ref([5, 3, 1], short, scores, 6)
    assert r.tolist() == [10, 20, 11, 33, -1, -1] and cl.tolist() == [0, 1, 0, 2, -1, -1]
    assert pos.tolist() == [0, 0, 1, 3, -1, -1] and np.isnan(s[4:]).all()
    # an empty cluster (size 0) is never asked, whatever its list holds
    assert interleave_ref([0, 3, 0], rows, scores, 3)[0].tolist() == [20, 21, 22]


# ------------------------------------------------- lib.get_user_recs_interests, on a stub ----
@pytest.fixture
def stub_lib(monkeypatch):
    from sqlalchemy import create_engine, insert
    from sqlalchemy.pool import StaticPool
    from robot_ebert_amd import interests, lib, tables
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

    def multi_interest_topk(c_, k, liked, c=3, exclude=None):
        calls["multi"] = (k, liked, c, exclude)
        # rows 5, 2, 8, 6 = ids "4", "100", "7", "55" from clusters 0, 1, 0, 1; medoids rows 0, 4
        n = min(k, 4)
        rows = torch.tensor([[5, 2, 8, 6][:n] + [-1] * (k - n)])
        scores = torch.tensor([[0.9, 0.95, 0.7, 0.6][:n] + [float("nan")] * (k - n)],
                              dtype=torch.float64)
        cluster = torch.tensor([[0, 1, 0, 1][:n] + [-1] * (k - n)], dtype=torch.int32)
        pos = torch.tensor([[0, 0, 1, 1][:n] + [-1] * (k - n)], dtype=torch.int32)
        size = torch.tensor([[2, 1] + [0] * (c - 2)], dtype=torch.int32)
        medoid_row = torch.tensor([[0, 4] + [-1] * (c - 2)])
        return interests.MultiInterest(rows, scores, cluster, pos, size, medoid_row)

    monkeypatch.setattr(interests, "multi_interest_topk", multi_interest_topk)
    monkeypatch.setattr(lib, "engine", engine)
    monkeypatch.setattr(lib, "movies_collab_catalog", cat)
    return lib, cat, calls


def test_get_user_recs_interests_order_and_id_pairing(stub_lib, monkeypatch):
    lib, cat, calls = stub_lib
    # get_movies answers ORDER BY tmdb_id, not in the order asked for
    monkeypatch.setattr(lib, "_get_movies_override", lambda ids: [_movie(t) for t in sorted(ids)])
    got = lib.get_user_recs_interests("u", k=6, interests=3)
    k, liked, c, exclude = calls["multi"]
    assert (k, c) == (6, 3)
    assert sorted(liked[0]) == sorted(cat.rows_of(["9", "10", "33"]))        # get_user_recs' sets
    assert sorted(exclude[0]) == sorted(cat.rows_of(["9", "10", "2", "33"]))
    # interleave order (not score order), each movie with ITS score, interest and anchor
    assert [(g.movie.tmdb_id, g.score, g.interest, g.anchor_tmdb_id) for g in got] == [
        ("4", 0.9, 0, "9"), ("100", 0.95, 1, "33"), ("7", 0.7, 0, "9"), ("55", 0.6, 1, "33")]
    lib.get_user_recs_interests("u")
    assert calls["multi"][0] == 10 and calls["multi"][2] == 3
    assert [g.movie.tmdb_id for g in lib.get_user_recs_interests("u", k=2, interests=2)] == \
        ["4", "100"]


def test_a_missing_movie_is_dropped_not_shifted(stub_lib, monkeypatch):
    """`movies` lacks "100" (SURVEY a-8): the others keep their own values and their order."""
    lib, cat, calls = stub_lib
    monkeypatch.setattr(lib, "_get_movies_override",
                        lambda ids: [_movie(t) for t in sorted(ids) if t != "100"])
    got = lib.get_user_recs_interests("u", k=4)
    assert [(g.movie.tmdb_id, g.score, g.interest) for g in got] == [
        ("4", 0.9, 0), ("7", 0.7, 0), ("55", 0.6, 1)]


def test_interests_errors_match_get_user_recs(stub_lib, monkeypatch):
    from robot_ebert_amd import EbertError
    lib, cat, calls = stub_lib
    monkeypatch.setattr(lib, "_get_movies_override", lambda ids: [_movie(t) for t in sorted(ids)])
    assert lib.get_user_recs_interests("nobody") == [] and lib.get_user_recs("nobody") == []
    with pytest.raises(ValueError, match="0 sample") as ei:               # no liked movie
        lib.get_user_recs_interests("cold")
    with pytest.raises(ValueError) as ei0:
        lib.get_user_recs("cold")
    assert str(ei.value) == str(ei0.value)
    for bad in (0, 9):
        with pytest.raises(EbertError, match=f"c={bad} clusters is outside"):
            lib.get_user_recs_interests("u", interests=bad)
    assert "multi" not in calls                                           # raised before the GPU


def test_route(monkeypatch):
    from fastapi.testclient import TestClient
    from robot_ebert_amd import api, lib
    from robot_ebert_amd.models import InterestRecommendation
    paths = {rt.path for rt in api.router.routes}
    assert "/users/{user_id}/recommendations/interests/" in paths
    assert "/users/{user_id}/recommendations/diverse/" in paths
    assert "/users/{user_id}/recommendations/" in paths
    calls = []

    def fake(user_id, k=10, interests=3):
        calls.append((user_id, k, interests))
        if user_id == "nolike":
            raise ValueError("Found array with 0 sample(s)")
        return [InterestRecommendation(movie=_movie(str(i)), score=1.0 - i / 10,
                                       interest=i % interests, anchor_tmdb_id=str(100 + i))
                for i in range(k)]
    monkeypatch.setattr(lib, "get_user_recs_interests", fake)
    c = TestClient(api.app(), raise_server_exceptions=False)
    url = "/users/u1/recommendations/interests/"
    got = c.get(url)
    assert got.status_code == 200 and len(got.json()) == 10 and calls[-1] == ("u1", 10, 3)
    got = c.get(url, params={"k": 3, "interests": 2}).json()
    assert calls[-1] == ("u1", 3, 2)
    assert [(x["movie"]["tmdb_id"], x["interest"], x["anchor_tmdb_id"]) for x in got] == [
        ("0", 0, "100"), ("1", 1, "101"), ("2", 0, "102")]
    assert c.get(url, params={"interests": 1}).status_code == 200
    assert c.get(url, params={"interests": 8}).status_code == 200
    n = len(calls)
    for bad in ({"interests": 0}, {"interests": 9}, {"interests": -1}, {"interests": "x"},
                {"k": "x"}):
        assert c.get(url, params=bad).status_code == 422, bad
    assert len(calls) == n                                   # rejected before the handler
    assert c.get("/users/nolike/recommendations/interests/").status_code == 500


# ----------------------------------------------------------- the kernels' register budget ----
def test_interest_kernels_have_no_scratch_and_no_spills(tmp_path):
    """Both kernels keep their per-lane state (the c x 8 accumulators, the 512 emitted rows) in
    registers: a private segment of 0 bytes and zero spill counts, read from the metadata notes
    of the built library (metadata only, no instruction text)."""
    from robot_ebert_amd import _lib
    from test_kernel_resources_host import READELF
    _lib.load()
    assert os.path.exists(READELF), READELF
    found = {}
    for i, image in enumerate(_gfx950_code_objects(_lib.LIB_PATH)):
        elf = tmp_path / f"co{i}.elf"
        elf.write_bytes(image)
        for name, k in _kernels(str(elf)).items():
            if "interest_cluster_kernel" in name or "interest_interleave_kernel" in name:
                found[name] = k
    assert sum("interest_cluster_kernel" in n for n in found) >= 1, sorted(found)
    assert sum("interest_interleave_kernel" in n for n in found) == 1, sorted(found)
    for name, k in sorted(found.items()):
        print(name, k)
        assert k["private_segment_fixed_size"] == 0, (name, k)
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (name, k)
