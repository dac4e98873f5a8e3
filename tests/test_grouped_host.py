"""CPU: grouped top-k (ebert.h 0.12.0) -- the new symbols and constants, every argument check of
the three entries (they run before any HIP call), ebt_grouped_pass_groups, the numpy restatement
(tests/grouped_ref.py) on a hand-worked case, lib.get_user_recs_by_group / its route on a stub,
and the kernel's register metadata in the built library.

The GPU paths (the kernel against numpy, the whole path bitwise against the masked path, the
certificates, the fallback, the invariances) are covered in test_gpu_grouped.py."""
import os

import numpy as np
import pytest
import torch

from grouped_ref import grouped_ref, select_ref
from test_explain_host import _StubCatalog, _movie
from test_kernel_resources_host import _gfx950_code_objects, _kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ebt_grouped_pass_groups", "ebt_select_topk_grouped", "ebt_cosine_topk_grouped_workspace",
       "ebt_cosine_topk_grouped_prepared")
EBT_EINVAL, EBT_ENOMEM, EBT_EUNSUPPORTED = -1, -3, -4
P = 1 << 30    # a fake device pointer: never dereferenced by a host check


def test_new_symbols_and_version():
    from robot_ebert_amd import _lib
    lib = _lib.load()
    for s in NEW:
        assert hasattr(lib, s), s
        assert s in _lib._SIGNATURES, s
    assert lib.ebt_version() >= 1200
    with open(os.path.join(ROOT, "include", "ebert.h")) as f:
        header = f.read()
    for s in NEW:
        assert s + "(" in header, s
    assert "0.12.0" in header and "lib.py:51-55" in header
    assert "#define EBT_NUM_STAGES 10" in header          # no new timer stage
    for name, v in (("EBT_GROUPS_MAX", 64), ("EBT_GROUPED_KPRIME_MAX", 512)):
        assert f"#define {name} {v}\n" in header, name
        assert getattr(_lib, name) == v
    import robot_ebert_amd as ebt
    assert ebt.score_topk_grouped is ebt.grouped.score_topk_grouped
    assert ebt.GroupedTopk._fields == ("scores", "rows", "group", "fallback")


def _err():
    from robot_ebert_amd import _lib
    return _lib.load().ebt_last_error().decode()


def test_select_argument_errors_without_a_gpu():
    """ebt_select_topk_grouped(vals, ld, B, n, col_begin, masks, words, n_masks, groups, G,
    kprime, segs, out_vals, out_idx, ld_out, stream)"""
    from robot_ebert_amd import _lib
    lib = _lib.load()
    who = "ebt_select_topk_grouped"
    good = [P, 1000, 4, 1000, 0, P, 32, 3, P, 5, 16, 1, P, P, 16, None]
    zero = list(good)
    zero[2] = 0
    assert lib.ebt_select_topk_grouped(*zero) == 0                      # B == 0
    for i in (0, 5, 8, 12, 13):
        a = list(good)
        a[i] = None
        assert lib.ebt_select_topk_grouped(*a) == EBT_EINVAL, i
        assert _err() == f"{who}: null pointer", (i, _err())
    for i, v, pat in ((9, 0, "G=0"), (9, 65, "G=65"), (9, -1, "G=-1"), (10, 0, "kprime=0"),
                      (10, 513, "kprime=513"), (1, 1002, "ld=1002"), (1, 996, "ld=996"),
                      (2, -1, "B=-1"), (3, -1, "n=-1"), (4, -4, "col_begin=-4"),
                      (11, 0, "segs=0"), (14, 15, "ld_out=15"), (0, P + 4, "16-byte aligned")):
        a = list(good)
        a[i] = v
        assert lib.ebt_select_topk_grouped(*a) == EBT_EINVAL, (i, v)
        assert _err().startswith(f"{who}: bad arguments") and pat in _err(), _err()
    # the table: words a multiple of 4 that reaches col_begin + n, n_masks >= 1
    for i, v in ((6, 30), (6, 28), (6, 0), (7, 0), (4, 32), (5, P + 8)):
        a = list(good)
        a[i] = v
        assert lib.ebt_select_topk_grouped(*a) == EBT_EINVAL, (i, v)
        assert _err().startswith(f"{who}: bad allow table"), _err()
    seg3 = list(good)
    seg3[11], seg3[14] = 3, 47                                          # ld_out < segs * kprime
    assert lib.ebt_select_topk_grouped(*seg3) == EBT_EINVAL


def _pipe_good(need=None):
    from robot_ebert_amd import _lib
    lib = _lib.load()
    if need is None:
        need = lib.ebt_cosine_topk_grouped_workspace(4, 128, 1000, 32, 128, 0, 5)
    #       q64 qimg qs eps B  B_pad cat dtype        ld  gn cimg cscale img_dtype    ld_img n
    return [P, P, P, P, 4, 128, P, _lib.EBT_F32, 64, P, P, None, _lib.EBT_F16, 64, 1000,
            # d d_pad off eo    er    k   k'  chunk flags groups G masks words n_masks
            64, 64, 0, None, None, 10, 32, 128, 0, P, 5, P, 32, 3,
            # ws ws_bytes out_s out_r cert timer stream
            P, need, P, P, P, None, None]


def test_pipeline_argument_errors_without_a_gpu():
    from robot_ebert_amd import _lib
    lib = _lib.load()
    who = "ebt_cosine_topk_grouped_prepared"
    f = lib.ebt_cosine_topk_grouped_prepared
    good = _pipe_good()
    assert good[30] > 0
    for i in (0, 1, 2, 3, 6, 9, 10, 24, 26, 29, 31, 32, 33):
        a = list(good)
        a[i] = None
        assert f(*a) == EBT_EINVAL, i
        assert _err() == f"{who}: null pointer", (i, _err())
    # EBT_EUNSUPPORTED: min(k, n) > 512 (the full-sort path among them), a row-sharded catalog
    for k, kp in ((513, 516), (5000, 5000)):
        a = list(good)
        a[20], a[21] = k, kp
        assert f(*a) == EBT_EUNSUPPORTED, k
        assert _err().startswith(who) and "not supported" in _err(), _err()
    a = list(good)
    a[17] = 37
    assert f(*a) == EBT_EUNSUPPORTED
    assert _err().startswith(who) and "row_offset=37" in _err(), _err()
    a = list(good)
    a[14], a[20], a[21] = 100, 600, 600                    # min(k, n) = 100: k' is the error
    assert f(*a) == EBT_EINVAL and "kprime=600" in _err()
    for i, v, pat in ((4, 0, "B=0"), (5, 100, "B_pad=100"), (14, 0, "n=0"), (20, 0, "k=0"),
                      (21, 8, "kprime=8"), (21, 34, "kprime=34"), (21, 516, "kprime=516"),
                      (22, 100, "chunk=100"), (25, 0, "G=0"), (25, 65, "G=65"),
                      (16, 65, "d_pad=65")):
        a = list(good)
        a[i] = v
        assert f(*a) == EBT_EINVAL, (i, v)
        assert _err().startswith(f"{who}: bad arguments") and pat in _err(), _err()
    a = list(good)
    a[18] = P                                              # exclusion offsets without rows
    assert f(*a) == EBT_EINVAL and _err().startswith(f"{who}: bad arguments")
    for i, v in ((27, 30), (27, 28), (28, 0), (26, P + 4)):
        a = list(good)
        a[i] = v
        assert f(*a) == EBT_EINVAL, (i, v)
        assert _err().startswith(f"{who}: bad allow table"), _err()
    for short in (0, good[30] - 1):
        a = list(good)
        a[30] = short
        assert f(*a) == EBT_ENOMEM
        assert _err() == (f"{who}: workspace {short} < {good[30]} bytes "
                          "(ebt_cosine_topk_grouped_workspace)")


def test_workspace_sizing():
    from robot_ebert_amd import _lib
    lib = _lib.load()
    w = lib.ebt_cosine_topk_grouped_workspace
    for bad in ((-1, 128, 1000, 32, 128, 0, 5), (4, 3, 1000, 32, 128, 0, 5),
                (4, 128, 0, 32, 128, 0, 5), (4, 128, 1000, 0, 128, 0, 5),
                (4, 128, 1000, 516, 128, 0, 5), (4, 128, 1000, 32, 0, 0, 5),
                (4, 128, 1000, 32, 128, 0, 0), (4, 128, 1000, 32, 128, 0, 65)):
        assert w(*bad) == 0, bad
    one, two, nine = (w(130, 256, 4099, 32, 1024, 0, g) for g in (1, 2, 9))
    assert 0 < one < two < nine and nine - one == 8 * (two - one)       # linear in G
    assert w(130, 256, 4099, 32, 1024, _lib.EBT_FLAG_EXACT, 2) > two    # the float64 screen's eps
    # one chunk and one segment: no per-chunk lists, the scores and the final lists only
    assert w(4, 128, 1000, 32, 1024, 0, 3) == 128 * 1000 * 4 + 3 * 4 * 32 * (4 + 8)
    # eight chunks: their lists too (every region rounded up to 256 bytes)
    assert w(4, 128, 1000, 32, 128, 0, 3) == 128 * 128 * 4 + 9 * 3 * 4 * 32 * (4 + 8)


def test_pass_groups():
    from robot_ebert_amd import _lib
    lib = _lib.load()
    got = [lib.ebt_grouped_pass_groups(kp) for kp in range(1, 513)]
    assert min(got) >= 1 and max(got) <= _lib.EBT_GROUPS_MAX
    assert all(a >= b for a, b in zip(got, got[1:]))                    # non-increasing
    assert got[-1] < 64                  # 64 groups at k' = 512 take more than one launch
    for kp in (0, -1, 513):
        assert lib.ebt_grouped_pass_groups(kp) == 0


# --------------------------------------------------------------- grouped_ref, hand-worked ----
def test_grouped_ref_hand_worked():
    """Eight rows, one query. Scores: rows 1 and 6 tie at 0.9 (the lower row first), row 3 is
    excluded, mask 2 is empty."""
    S = np.array([[0.1, 0.9, 0.5, 0.95, -0.2, 0.5, 0.9, 0.0]])
    flags = np.array([[1, 1, 1, 1, 0, 0, 1, 0],       # mask 0
                      [0, 0, 1, 1, 1, 1, 0, 1],       # mask 1
                      [0, 0, 0, 0, 0, 0, 0, 0]], bool)
    s, r = grouped_ref(S, flags, [0, 1, 2, 7, -1, 1], 3, exclude=[[3]])
    assert r.shape == (1, 6, 3) and s.shape == (1, 6, 3) and r.dtype == np.int64
    assert r[0, 0].tolist() == [1, 6, 2] and s[0, 0].tolist() == [0.9, 0.9, 0.5]   # the tie
    assert r[0, 1].tolist() == [2, 5, 7] and s[0, 1].tolist() == [0.5, 0.5, 0.0]
    for g in (2, 3):                                   # an empty mask, an id past the table
        assert r[0, g].tolist() == [-1] * 3 and np.isnan(s[0, g]).all()
    assert r[0, 4].tolist() == [1, 6, 2]               # unfiltered: still without row 3
    assert r[0, 5].tolist() == r[0, 1].tolist()        # the same id twice
    # fewer candidates than k; no exclusions: row 3 leads
    s, r = grouped_ref(S, flags, [1], 8)
    assert r[0, 0].tolist() == [3, 2, 5, 7, 4, -1, -1, -1] and np.isnan(s[0, 0, 5:]).all()


def test_select_ref_hand_worked():
    v = np.array([[0.5, np.nan, 0.7, 0.7, -np.inf, 0.9, 0.7, 0.1, 9.0, 9.0, 9.0, 9.0]],
                 dtype=np.float32)                      # n = 8 of ld = 12
    flags = np.zeros((2, 40), bool)
    flags[0, 32:40] = True
    flags[1, [34, 35, 38]] = True
    ov, oi = select_ref(v, 8, 32, flags, [0, 1, 5], 3, 1)
    assert oi[0, 0].tolist() == [37, 34, 35] and ov[0, 0].tolist() == [np.float32(0.9)] + \
        [np.float32(0.7)] * 2
    assert oi[1, 0].tolist() == [34, 35, 38]            # three equal values: by index
    assert oi[2, 0].tolist() == [-1] * 3 and np.isinf(ov[2, 0]).all()
    ov, oi = select_ref(v, 8, 32, flags, [0], 2, 2)     # two segments of four
    assert oi[0, 0].tolist() == [34, 35, 37, 38]


# ------------------------------------------------- lib.get_user_recs_by_group, on a stub ----
class _StubMasks:
    names = ["drama", "comedy", "docs"]
    n_masks = 3

    def index(self, g):
        from robot_ebert_amd import EbertError
        if isinstance(g, str):
            if g not in self.names:
                raise EbertError(f"unknown allow mask {g!r}")
            return self.names.index(g)
        return int(g)


@pytest.fixture
def stub_lib(monkeypatch):
    from sqlalchemy import create_engine, insert
    from sqlalchemy.pool import StaticPool
    from robot_ebert_amd import grouped, lib, tables
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
    # per mask id: rows and scores, score order; row 5 = id "4" sits on two shelves
    shelf = {0: ([5, 2, 8], [0.9, 0.8, 0.7]), 1: ([6, 5], [0.6, 0.5]), 2: ([], [])}

    def score_topk_grouped(c, k, masks, groups, liked=None, exclude=None, **kw):
        ids = grouped.resolve_groups(masks, groups)
        calls["grouped"] = (k, ids, liked, exclude)
        rows = torch.full((1, len(ids), k), -1, dtype=torch.int64)
        scores = torch.full((1, len(ids), k), float("nan"), dtype=torch.float64)
        for i, m in enumerate(ids):
            r, s = shelf.get(m, ([], []))
            n = min(k, len(r))
            rows[0, i, :n] = torch.tensor(r[:n], dtype=torch.int64)
            scores[0, i, :n] = torch.tensor(s[:n], dtype=torch.float64)
        return grouped.GroupedTopk(scores, rows, torch.tensor(ids, dtype=torch.int32), 0)

    monkeypatch.setattr(grouped, "score_topk_grouped", score_topk_grouped)
    monkeypatch.setattr(lib, "engine", engine)
    monkeypatch.setattr(lib, "movies_collab_catalog", cat)
    monkeypatch.setattr(lib, "allow_masks", _StubMasks())
    monkeypatch.setattr(lib, "_get_movies_override", lambda ids: [_movie(t) for t in sorted(ids)])
    return lib, cat, calls


def test_get_user_recs_by_group_shelves(stub_lib):
    lib, cat, calls = stub_lib
    got = lib.get_user_recs_by_group("u", k=3)
    k, ids, liked, exclude = calls["grouped"]
    assert (k, ids) == (3, [0, 1, 2])                                  # default: every mask
    assert sorted(liked[0]) == sorted(cat.rows_of(["9", "10", "33"]))  # get_user_recs' sets
    assert sorted(exclude[0]) == sorted(cat.rows_of(["9", "10", "2", "33"]))
    assert list(got) == ["drama", "comedy", "docs"]
    assert [(x.movie.tmdb_id, x.score) for x in got["drama"]] == [("4", 0.9), ("100", 0.8),
                                                                  ("7", 0.7)]
    assert [(x.movie.tmdb_id, x.score) for x in got["comedy"]] == [("55", 0.6), ("4", 0.5)]
    assert got["docs"] == []
    # names, indices, indices as strings (the route's form), a repeated group; the order asked
    got = lib.get_user_recs_by_group("u", k=2, groups=["comedy", 0, "2", "comedy"])
    assert calls["grouped"][:2] == (2, [1, 0, 2, 1])
    assert list(got) == ["comedy", "0", "2"]
    assert [x.movie.tmdb_id for x in got["0"]] == ["4", "100"]
    assert lib.get_user_recs_by_group("u")["drama"][0].score == 0.9 and calls["grouped"][0] == 10


def test_by_group_errors_match_get_user_recs(stub_lib, monkeypatch):
    from robot_ebert_amd import EbertError
    lib, cat, calls = stub_lib
    assert lib.get_user_recs_by_group("nobody") == {} and lib.get_user_recs("nobody") == []
    with pytest.raises(ValueError, match="0 sample") as ei:              # no liked movie
        lib.get_user_recs_by_group("cold")
    with pytest.raises(ValueError) as ei0:
        lib.get_user_recs("cold")
    assert str(ei.value) == str(ei0.value)
    with pytest.raises(EbertError, match="unknown allow mask 'horror'"):
        lib.get_user_recs_by_group("u", groups=["horror"])
    assert "grouped" not in calls                                        # raised before the GPU
    monkeypatch.setattr(lib, "allow_masks", None)
    with pytest.raises(EbertError, match="needs lib.configure"):
        lib.get_user_recs_by_group("u")


def test_python_argument_errors_before_any_device_work():
    from robot_ebert_amd import AllowMasks, EbertError, grouped

    class Shard:
        n, n_global, row_offset, device, d = 500, 1000, 500, "cpu", 8

    class Cat:
        n, n_global, row_offset, device, d, capacity = 1000, 1000, 0, "cpu", 8, 1000

    masks = AllowMasks(1000, 3, names=["a", "b", "c"], device="cpu")
    with pytest.raises(EbertError, match="row-sharded catalog is not supported"):
        grouped.score_topk_grouped(Shard(), 5, masks, [0], liked=[[501]])
    with pytest.raises(EbertError, match="k must be >= 1"):
        grouped.score_topk_grouped(Cat(), 0, masks, [0], liked=[[1]])
    with pytest.raises(EbertError, match="takes an AllowMasks"):
        grouped.score_topk_grouped(Cat(), 5, None, [0], liked=[[1]])
    with pytest.raises(EbertError, match="unknown allow mask 'z'"):
        grouped.score_topk_grouped(Cat(), 5, masks, ["a", "z"], liked=[[1]])
    with pytest.raises(EbertError, match="holds no group"):
        grouped.score_topk_grouped(Cat(), 5, masks, [], liked=[[1]])
    with pytest.raises(EbertError, match="k=600 over a 1000-row catalog"):
        grouped.score_topk_grouped(Cat(), 600, masks, [0], liked=[[1]])
    with pytest.raises(EbertError, match="kprime=1024 is more than 512"):
        grouped.score_topk_grouped(Cat(), 5, masks, [0], liked=[[1]], kprime=1024)
    with pytest.raises(EbertError, match="no CPU path"):                 # the last host check
        grouped.score_topk_grouped(Cat(), 5, masks, ["a", 7, -1], liked=[[1]])
    assert grouped.resolve_groups(masks, ["c", 0, 7, -1, "a"]) == [2, 0, 7, -1, 0]


def test_route(monkeypatch):
    from fastapi.testclient import TestClient
    from robot_ebert_amd import api, lib
    from robot_ebert_amd.models import Recommendation
    paths = {rt.path for rt in api.router.routes}
    assert "/users/{user_id}/recommendations/by-group/" in paths
    assert "/users/{user_id}/recommendations/interests/" in paths
    assert "/users/{user_id}/recommendations/" in paths
    calls = []

    def fake(user_id, k=10, groups=None):
        calls.append((user_id, k, groups))
        if user_id == "nolike":
            raise ValueError("Found array with 0 sample(s)")
        return {g: [Recommendation(movie=_movie(str(i)), score=1.0 - i / 10) for i in range(k)]
                for g in (groups or ["drama", "comedy"])}
    monkeypatch.setattr(lib, "get_user_recs_by_group", fake)
    c = TestClient(api.app(), raise_server_exceptions=False)
    url = "/users/u1/recommendations/by-group/"
    got = c.get(url)
    assert got.status_code == 200 and calls[-1] == ("u1", 10, None)
    assert list(got.json()) == ["drama", "comedy"] and len(got.json()["drama"]) == 10
    got = c.get(url, params={"k": 2, "groups": "comedy, 3,drama"}).json()
    assert calls[-1] == ("u1", 2, ["comedy", "3", "drama"])
    assert [x["movie"]["tmdb_id"] for x in got["3"]] == ["0", "1"]
    n = len(calls)
    assert c.get(url, params={"k": "x"}).status_code == 422
    assert len(calls) == n                                   # rejected before the handler
    assert c.get("/users/nolike/recommendations/by-group/").status_code == 500


# ------------------------------------------------------------- the kernel's register budget ----
def test_grouped_select_kernel_has_no_scratch(tmp_path):
    """The kernel keeps its two tiles of scores and its admission masks in registers: a private
    segment of 0 bytes and no vector register spilled, read from the metadata notes of the built
    library (metadata only, no instruction text)."""
    from robot_ebert_amd import _lib
    from test_kernel_resources_host import READELF
    _lib.load()
    assert os.path.exists(READELF), READELF
    found = {}
    for i, image in enumerate(_gfx950_code_objects(_lib.LIB_PATH)):
        elf = tmp_path / f"co{i}.elf"
        elf.write_bytes(image)
        for name, k in _kernels(str(elf)).items():
            if "grouped_select_kernel" in name:
                found[name] = k
    assert len(found) == 1, sorted(found)
    for name, k in found.items():
        print(name, k)
        assert k["private_segment_fixed_size"] == 0, (name, k)
        assert k["vgpr_spill_count"] == 0, (name, k)
