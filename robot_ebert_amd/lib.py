"""Drop-in GPU version of the reference's recommend call surface (src/backend/app/lib.py).

``get_user_recs(user_id, k)`` keeps ``lib.py:32-63``'s Python semantics -- the same SQL, the same
pandas filtering, the same ValueError for a user without liked movies, the same
``sort_index``/``zip``/``sorted`` hydration order -- and replaces only the scoring block
``lib.py:51-55`` (sklearn cosine_similarity + mean + pandas sort) by ``search.score_topk`` on the
HBM-resident catalog. ``user_movie_scores`` mirrors the re-weighting arithmetic of
``lib.py:94-121`` for ``run_search`` (whose LLM / Chroma retrieval is out of scope).

Module globals play the role of ``backend.app.constants`` (engine, catalog, thresholds) and are
set with ``configure``.
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import pandas as pd
import torch
from sqlalchemy import select

from . import tables
from .catalog import Catalog
from .models import (ExplainedRecommendation, InterestRecommendation, Movie, Reason,
                     Recommendation)
from .search import csr_from_lists, prepare_queries, rescore_rows, score_topk

LIKED_MOVIE_SCORE = 3.5   # constants.py:19
QUERY_SCORE_WEIGHT = 0.90  # constants.py:20
SIMILARITY_TOP_K = 10     # constants.py:21

engine = None                              # constants.py:26 (caller-supplied SQLAlchemy Engine)
movies_collab_catalog: Optional[Catalog] = None  # constants.py:55-56, resident in HBM
movies_content_catalog: Optional[Catalog] = None  # the movies-content collection (constants.py:29-53)
allow_masks = None                         # allow.AllowMasks over movies_collab_catalog (optional)
_get_movies_override: Optional[Callable[[List[str]], List[Movie]]] = None


def configure(engine=None, catalog: Optional[Catalog] = None,
              get_movies: Optional[Callable[[List[str]], List[Movie]]] = None,
              content_catalog: Optional[Catalog] = None, allow_masks=None) -> None:
    """Install the process-global resources (the reference builds them at import time).
    allow_masks: the allow.AllowMasks that ``get_user_recs(..., allow=)`` indexes."""
    g = globals()
    if allow_masks is not None:
        g["allow_masks"] = allow_masks
    if engine is not None:
        g["engine"] = engine
    if catalog is not None:
        g["movies_collab_catalog"] = catalog
    if content_catalog is not None:
        g["movies_content_catalog"] = content_catalog
    g["_get_movies_override"] = get_movies


def get_movies(tmdb_ids: List[str]) -> List[Movie]:
    """lib.py:23-29: Movie rows for the ids, ORDER BY tmdb_id."""
    if _get_movies_override is not None:
        return _get_movies_override(tmdb_ids)
    with engine.begin() as cnx:
        stmt = select(tables.movies).where(tables.movies.c.tmdb_id.in_(tmdb_ids)).order_by(
            tables.movies.c.tmdb_id)
        rows = cnx.execute(stmt).all()
    out = []
    for row in rows:
        d = row._asdict()
        d.pop("updated_at", None)
        out.append(Movie(**d))
    return out


def _user_ratings(user_id: str) -> pd.DataFrame:
    """lib.py:36-38 + 43-44: the user's ratings restricted to movies in the catalog."""
    with engine.begin() as cnx:
        rows = cnx.execute(select(tables.ratings).where(tables.ratings.c.user_id == user_id)).all()
    if not rows:  # pandas: an empty DataFrame has no "tmdb_id" column (lib.py:97)
        raise KeyError("tmdb_id")
    df = pd.DataFrame(rows)
    cat = movies_collab_catalog
    return df[cat.contains(df["tmdb_id"])]


def user_query_lists(user_ratings: pd.DataFrame, catalog: Catalog,
                     liked_threshold: float = LIKED_MOVIE_SCORE) -> Tuple[List[int], List[int]]:
    """lib.py:47-48 as row lists: (liked rows, rated rows). The reference's candidate set is
    catalog.index.difference(rated), i.e. every catalog row except the rated ones."""
    liked_ids = user_ratings[user_ratings["rating"] >= liked_threshold]["tmdb_id"]
    rated_ids = pd.unique(user_ratings["tmdb_id"])
    return catalog.rows_of(liked_ids), catalog.rows_of(rated_ids)


def order_recommendations(pairs: Sequence[Tuple[str, float]]) -> List[Tuple[str, float]]:
    """lib.py:55 ``.sort_index()`` (lexicographic on the string ids) -- the order in which
    lib.py:58-62 zips the movies with the scores -- then lib.py:63's stable sort by score."""
    by_id = sorted(pairs, key=lambda t: t[0])
    return sorted(by_id, key=lambda t: t[1], reverse=True)


def _user_request(user_id: str) -> Optional[Tuple[List[int], List[int]]]:
    """lib.py:36-48: (liked rows, rated rows) of a user, None when the user has no ratings;
    sklearn's ValueError when none of the ratings is a liked catalog movie."""
    cat = movies_collab_catalog
    with engine.begin() as cnx:  # lib.py:36-40
        statement = select(tables.ratings).where(tables.ratings.c.user_id == user_id)
        user_ratings = cnx.execute(statement).all()
        if not user_ratings:
            return None
    # lib.py:43-48 on the fetched rows in plain Python (the DataFrame construction and boolean
    # indexing cost ~2 ms of interpreter time per request, under FastAPI's 40 worker threads
    # all of it serialised on the GIL): keep the ratings of catalog movies (the isin of :44),
    # liked = ratings >= LIKED_MOVIE_SCORE in row order (:47), rated = their ids in first-seen
    # order (:48, pd.unique) -- the lists user_query_lists builds from the DataFrame.
    pos = cat.index_pos
    kept = [(r.tmdb_id, r.rating) for r in user_ratings if r.tmdb_id in pos]  # lib.py:44
    liked = cat.rows_of([t for t, rt in kept if rt >= LIKED_MOVIE_SCORE])     # lib.py:47
    rated = cat.rows_of(list(dict.fromkeys(t for t, _ in kept)))              # lib.py:48
    if not liked:  # sklearn check_pairwise_arrays on an empty X (lib.py:51)
        raise ValueError(f"Found array with 0 sample(s) (shape=(0, {cat.d})) while a minimum of 1 "
                         "is required by check_pairwise_arrays.")
    return liked, rated


def weight_by_rating(rating: float) -> float:
    """A ``weighting``: a liked movie counts by its rating, r if r >= LIKED_MOVIE_SCORE else 0
    (the reference's 0/1 vote of lib.py:47 with the rating kept; a 5.0 outweighs a 3.5)."""
    return float(rating) if rating >= LIKED_MOVIE_SCORE else 0.0


def weight_centered(rating: float) -> float:
    """A ``weighting``: r - LIKED_MOVIE_SCORE, so that a disliked movie pushes away (a 0.5 weighs
    -3.0, a 5.0 weighs +1.5, a 3.5 nothing)."""
    return float(rating) - LIKED_MOVIE_SCORE


def _user_request_weighted(user_id: str, weighting: Callable[[float], float]
                           ) -> Optional[Tuple[List[int], List[int], List[float]]]:
    """_user_request with ``weighting`` in place of lib.py:47's threshold: (rows, rated rows,
    weights), one term per rating of a catalog movie whose weight is not zero, in row order of
    the ratings; None when the user has no ratings; sklearn's ValueError when no term is left."""
    cat = movies_collab_catalog
    with engine.begin() as cnx:  # lib.py:36-40
        statement = select(tables.ratings).where(tables.ratings.c.user_id == user_id)
        user_ratings = cnx.execute(statement).all()
        if not user_ratings:
            return None
    pos = cat.index_pos
    kept = [(r.tmdb_id, r.rating) for r in user_ratings if r.tmdb_id in pos]  # lib.py:44
    terms = [(t, float(weighting(rt))) for t, rt in kept]
    terms = [(t, w) for t, w in terms if w != 0.0]
    rated = cat.rows_of(list(dict.fromkeys(t for t, _ in kept)))              # lib.py:48
    if not terms:  # sklearn check_pairwise_arrays on an empty X (lib.py:51)
        raise ValueError(f"Found array with 0 sample(s) (shape=(0, {cat.d})) while a minimum of 1 "
                         "is required by check_pairwise_arrays.")
    return cat.rows_of([t for t, _ in terms]), rated, [w for _, w in terms]


def _hydrate(s: np.ndarray, r: np.ndarray) -> List[Recommendation]:
    """lib.py:55-63 after the top-k: ids, sort_index, get_movies (ORDER BY id), zip, stable sort."""
    cat = movies_collab_catalog
    pairs = [(cat.id_of(int(rr)), float(ss)) for ss, rr in zip(s, r) if rr >= 0]
    ordered_by_id = sorted(pairs, key=lambda t: t[0])  # .sort_index()
    movies = get_movies(tmdb_ids=[t for t, _ in ordered_by_id])  # lib.py:58
    scores_by_id = [sc for _, sc in ordered_by_id]  # lib.py:59
    recommendations = [Recommendation(movie=m, score=sc) for m, sc in zip(movies, scores_by_id)]
    return sorted(recommendations, key=lambda x: x.score, reverse=True)  # lib.py:63


def _allow_of(allow):
    """(allow_masks, [mask index]) for one filtered request; EbertError on a bad name or index."""
    from ._lib import EbertError
    if allow_masks is None:
        raise EbertError("allow= needs lib.configure(allow_masks=...)")
    return allow_masks, [allow_masks.index(allow)]


def get_user_recs(user_id: str, k: int = 10, allow=None,
                  weighting: Optional[Callable[[float], float]] = None) -> List[Recommendation]:
    """GPU drop-in for lib.py:32-63 (same inputs, same outputs, same errors).

    Any k, as the reference's pandas `[:k]` (min(k, rows) > 4096 runs the full-sort path of
    csrc/large_k.hip). On a row-sharded catalog min(k, rows) <= 4096.

    allow: None (the reference's function), or the index or name of one of the configured
    ``allow_masks``: the recommendations come from the rows that mask allows (unrated ones, as
    always), min(k, rows) <= 4096.

    weighting: None (the reference's function: rating >= LIKED_MOVIE_SCORE is a 0/1 vote), or a
    callable rating -> weight applied to every rated catalog movie (``weight_by_rating``,
    ``weight_centered``): the score of a movie is sum_l w_l cos(x_l, x) / sum_l |w_l| over the
    rated movies with a non-zero weight; when none is left, sklearn's empty-array ValueError.
    Rated movies stay excluded either way."""
    if weighting is not None:
        wreq = _user_request_weighted(user_id, weighting)
        if wreq is None:
            return []
        liked, rated, w = wreq
        scores, rows = score_topk(movies_collab_catalog, k, liked=[liked], exclude=[rated],
                                  liked_weights=[w],
                                  allow=_allow_of(allow) if allow is not None else None)
        return _hydrate(scores[0].cpu().numpy(), rows[0].cpu().numpy())
    req = _user_request(user_id)
    if req is None:
        return []
    liked, rated = req
    if allow is not None:
        scores, rows = score_topk(movies_collab_catalog, k, liked=[liked], exclude=[rated],
                                  allow=_allow_of(allow))
        return _hydrate(scores[0].cpu().numpy(), rows[0].cpu().numpy())
    scores, rows = score_topk(movies_collab_catalog, k, liked=[liked], exclude=[rated])  # :51-55
    return _hydrate(scores[0].cpu().numpy(), rows[0].cpu().numpy())


get_user_recs_gpu = get_user_recs  # SURVEY §8b's name for the drop-in


def _user_terms(user_id: str, weighting: Optional[Callable[[float], float]]
                ) -> Optional[Tuple[List[int], List[int], Optional[List[float]], List[float]]]:
    """One fetch of what ``get_user_recs`` scores from, with the ratings kept: (liked rows, rated
    rows, weights or None, the rating behind each liked row). The lists are ``_user_request``'s
    (weighting None) or ``_user_request_weighted``'s, entry for entry; None when the user has no
    ratings; sklearn's ValueError when no liked row is left."""
    cat = movies_collab_catalog
    with engine.begin() as cnx:  # lib.py:36-40
        statement = select(tables.ratings).where(tables.ratings.c.user_id == user_id)
        user_ratings = cnx.execute(statement).all()
        if not user_ratings:
            return None
    pos = cat.index_pos
    kept = [(r.tmdb_id, r.rating) for r in user_ratings if r.tmdb_id in pos]  # lib.py:44
    if weighting is None:
        terms = [(t, None, rt) for t, rt in kept if rt >= LIKED_MOVIE_SCORE]  # lib.py:47
    else:
        terms = [(t, float(weighting(rt)), rt) for t, rt in kept]
        terms = [x for x in terms if x[1] != 0.0]
    rated = cat.rows_of(list(dict.fromkeys(t for t, _ in kept)))              # lib.py:48
    if not terms:  # sklearn check_pairwise_arrays on an empty X (lib.py:51)
        raise ValueError(f"Found array with 0 sample(s) (shape=(0, {cat.d})) while a minimum of 1 "
                         "is required by check_pairwise_arrays.")
    return (cat.rows_of([t for t, _, _ in terms]), rated,
            None if weighting is None else [w for _, w, _ in terms],
            [float(rt) for _, _, rt in terms])


def _hydrate_explained(s: np.ndarray, r: np.ndarray,
                       reasons_by_id) -> List[ExplainedRecommendation]:
    """``_hydrate`` with reasons. The reasons are keyed by the recommended movie's tmdb_id BEFORE
    the sort_index / get_movies / zip of lib.py:55-62 and attached by the id of the Movie that
    came back, never by zip position: when ``movies`` lacks a row (SURVEY a-8: 2269 collab ids,
    2264 movie rows) the reference's zip shifts the scores, and the reasons still follow their
    movie."""
    cat = movies_collab_catalog
    pairs = [(cat.id_of(int(rr)), float(ss)) for ss, rr in zip(s, r) if rr >= 0]
    ordered_by_id = sorted(pairs, key=lambda t: t[0])  # .sort_index()
    movies = get_movies(tmdb_ids=[t for t, _ in ordered_by_id])  # lib.py:58
    scores_by_id = [sc for _, sc in ordered_by_id]  # lib.py:59
    recs = [ExplainedRecommendation(movie=mv, score=sc, reasons=reasons_by_id.get(mv.tmdb_id, []))
            for mv, sc in zip(movies, scores_by_id)]
    return sorted(recs, key=lambda x: x.score, reverse=True)  # lib.py:63


def get_user_recs_explained(user_id: str, k: int = 10, m: int = 3,
                            weighting: Optional[Callable[[float], float]] = None,
                            allow=None) -> List[ExplainedRecommendation]:
    """``get_user_recs`` with the "because you liked" line: the same movies, scores, order and
    errors (``[]`` for a user without ratings, sklearn's ValueError for one without a liked
    movie), each item carrying up to ``m`` reasons -- the rated movies whose terms of the score
    (one per liked row, lib.py:51-52 before the ``.mean``) are largest, in that order, with the
    term and the user's rating. With a ``weighting`` that gives negative weights the terms of
    disliked movies are negative and rank last. ``explain.explain_topk`` computes them on the
    GPU for the k returned rows; a row-sharded catalog raises EbertError."""
    from .explain import explain_topk
    req = _user_terms(user_id, weighting)
    if req is None:
        return []
    liked, rated, w, ratings = req
    cat = movies_collab_catalog
    kw = {}
    if w is not None:
        kw["liked_weights"] = [w]
    if allow is not None:
        kw["allow"] = _allow_of(allow)
    scores, rows = score_topk(cat, k, liked=[liked], exclude=[rated], **kw)
    ex = explain_topk(cat, rows, [liked], liked_weights=[w] if w is not None else None, m=m)
    s, r = scores[0].cpu().numpy(), rows[0].cpu().numpy()
    val, pos = ex.contrib[0].cpu().numpy(), ex.pos[0].cpu().numpy()
    reasons_by_id = {}
    for j, rr in enumerate(r):
        if rr < 0:
            continue
        reasons_by_id[cat.id_of(int(rr))] = [
            Reason(tmdb_id=cat.id_of(liked[int(p)]), contribution=float(v),
                   rating=ratings[int(p)])
            for v, p in zip(val[j], pos[j]) if p >= 0]
    return _hydrate_explained(s, r, reasons_by_id)


def get_user_recs_diverse(user_id: str, k: int = 10, lam: float = 0.7,
                          pool: Optional[int] = None,
                          weighting: Optional[Callable[[float], float]] = None
                          ) -> List[Recommendation]:
    """``get_user_recs`` with variety: the same SQL, liked / rated sets and errors (``[]`` for a
    user without ratings, sklearn's ValueError for one without a liked movie), but the k movies
    are picked from the ``pool`` best (default min(10 k, 512, catalog rows)) greedily by maximal
    marginal relevance, each pick maximising lam * score - (1 - lam) * (largest cosine to a movie
    already picked) (``diversify.diversify_topk``; lam = 1 is the plain top k).

    Returns ``Recommendation(movie, score)`` with the relevance as the score, in SELECTION order.
    Movies are paired with their scores by tmdb_id; one that ``movies`` lacks is dropped (there is
    no reference order to mimic here, so lib.py:58-62's zip -- SURVEY a-8 -- is not reproduced).
    A row-sharded catalog raises EbertError."""
    from . import diversify
    from ._lib import EBT_MMR_POOL_MAX
    from .diversify import diversify_topk
    diversify._check_lam(lam)
    if pool is not None:
        diversify._check_pool(pool)
    req = _user_terms(user_id, weighting)
    if req is None:
        return []
    liked, rated, w, _ = req
    cat = movies_collab_catalog
    if pool is None:
        pool = min(10 * k, EBT_MMR_POOL_MAX, cat.n)
    kw = {"liked_weights": [w]} if w is not None else {}
    scores, rows = score_topk(cat, pool, liked=[liked], exclude=[rated], **kw)
    picked = diversify_topk(cat, scores, rows, min(k, int(rows.shape[1])), lam=lam)
    pairs = [(cat.id_of(int(rr)), float(ss))
             for ss, rr in zip(picked.scores[0].cpu().numpy(), picked.rows[0].cpu().numpy())
             if rr >= 0]
    movies = {m.tmdb_id: m for m in get_movies(tmdb_ids=sorted(t for t, _ in pairs))}
    return [Recommendation(movie=movies[t], score=sc) for t, sc in pairs if t in movies]


def get_user_recs_interests(user_id: str, k: int = 10,
                            interests: int = 3) -> List[InterestRecommendation]:
    """``get_user_recs`` for a user with several tastes: the same SQL, liked / rated sets and
    errors (``[]`` for a user without ratings, sklearn's ValueError for one without a liked
    movie), but the liked movies are grouped into up to ``interests`` clusters, each cluster is
    searched as a liked list of its own, and the k movies are drawn from the clusters' answers in
    proportion to their sizes (``interests.multi_interest_topk``; interests = 1 is the plain top
    k).

    Returns ``InterestRecommendation(movie, score, interest, anchor_tmdb_id)`` in INTERLEAVE
    order: the score is the mean cosine to the liked movies of the movie's interest, the anchor
    that interest's medoid ("more like X"). Movies are paired with their values by tmdb_id; one
    that ``movies`` lacks is dropped (there is no reference order to mimic here, so lib.py:58-62's
    zip -- SURVEY a-8 -- is not reproduced). A row-sharded catalog raises EbertError."""
    from . import interests as _interests
    _interests._check_c(interests)
    req = _user_request(user_id)
    if req is None:
        return []
    liked, rated = req
    cat = movies_collab_catalog
    got = _interests.multi_interest_topk(cat, k, liked=[liked], c=interests, exclude=[rated])
    anchor = [cat.id_of(int(r)) if r >= 0 else "" for r in got.medoid_row[0].cpu().numpy()]
    items = [(cat.id_of(int(rr)), float(ss), int(cc))
             for rr, ss, cc in zip(got.rows[0].cpu().numpy(), got.scores[0].cpu().numpy(),
                                   got.cluster[0].cpu().numpy()) if rr >= 0]
    movies = {m.tmdb_id: m for m in get_movies(tmdb_ids=sorted(t for t, _, _ in items))}
    return [InterestRecommendation(movie=movies[t], score=sc, interest=cl,
                                   anchor_tmdb_id=anchor[cl])
            for t, sc, cl in items if t in movies]


def _shelf_groups(masks, groups) -> List[Tuple[str, object]]:
    """(shelf key, group) of every requested shelf: every mask of the table when ``groups`` is
    None, keyed by its name (or its index as a string when the masks have no names). A string
    that is no mask name but reads as an integer is an index."""
    if groups is None:
        return [(str(masks.names[m]) if masks.names is not None else str(m), m)
                for m in range(masks.n_masks)]
    out = []
    for g in groups:
        if isinstance(g, str) and (masks.names is None or g not in masks.names) \
                and g.strip().lstrip("-").isdigit():
            out.append((g.strip(), int(g)))
        else:
            out.append((str(g), g))
    return out


def get_user_recs_by_group(user_id: str, k: int = 10, groups=None,
                           masks=None) -> Dict[str, List[Recommendation]]:
    """``get_user_recs`` once per shelf of a front page ("top drama for you", "top comedy for
    you"): the same SQL, liked / rated sets, errors (``{}`` for a user without ratings, sklearn's
    ValueError for one without a liked movie) and hydration (lib.py:55-63) per shelf, but all the
    shelves come from ONE scoring pass (``grouped.score_topk_grouped``). Shelf ``g`` holds what
    ``get_user_recs(user_id, k, allow=g)`` returns.

    groups: mask names or indices of ``masks`` (default: every mask); masks: an
    ``allow.AllowMasks`` over the catalog (default: the configured ``allow_masks``). The result
    is keyed by the group as it was asked for (a name, or the index as a string), in that order.
    A movie of several genres appears on each of its shelves. A row-sharded catalog raises
    EbertError."""
    from ._lib import EbertError
    from .grouped import resolve_groups, score_topk_grouped
    masks = masks if masks is not None else allow_masks
    if masks is None:
        raise EbertError("get_user_recs_by_group needs lib.configure(allow_masks=...) or masks=")
    shelves = _shelf_groups(masks, groups)
    resolve_groups(masks, [g for _, g in shelves])   # a bad name fails before the SQL
    req = _user_request(user_id)
    if req is None:
        return {}
    liked, rated = req
    got = score_topk_grouped(movies_collab_catalog, k, masks, [g for _, g in shelves],
                             liked=[liked], exclude=[rated])
    s, r = got.scores[0].cpu().numpy(), got.rows[0].cpu().numpy()
    return {key: _hydrate(s[i], r[i]) for i, (key, _) in enumerate(shelves)}


def get_user_recs_batched(batcher, user_id: str, k: int = 10, allow=None,
                          weighting: Optional[Callable[[float], float]] = None
                          ) -> List[Recommendation]:
    """``get_user_recs`` whose scoring step is coalesced with concurrent callers by a
    ``batcher.RecBatcher`` over ``movies_collab_catalog``: same SQL, same errors,
    same ordering; the GPU sees one batch for many request threads. allow: a mask index or name
    of the batcher's ``allow_masks`` (None: unfiltered). weighting: as ``get_user_recs``'s."""
    if weighting is not None:
        wreq = _user_request_weighted(user_id, weighting)
        if wreq is None:
            return []
        liked, rated, w = wreq
        kw = {"allow": allow} if allow is not None else {}
        s, r = batcher.submit(liked, rated, k, weights=w, **kw).result()
        return _hydrate(s, r)
    req = _user_request(user_id)
    if req is None:
        return []
    liked, rated = req
    if allow is not None:
        s, r = batcher.submit(liked, rated, k, allow=allow).result()
        return _hydrate(s, r)
    s, r = batcher.submit(liked, rated, k).result()
    return _hydrate(s, r)


def retrieve_content_matches(query_embedding, k: int = SIMILARITY_TOP_K) -> Tuple[List[str],
                                                                                   List[float]]:
    """the content retrieval of run_search (lib.py:71-73: the chat engine's
    ``similarity_top_k`` matches from the ``movies-content`` Chroma collection, hnsw:space=cosine,
    constants.py:29-53) as EXACT cosine top-k on the HBM content catalog. Returns (ids, cosine
    scores) in score order. HNSW is approximate; its result sets are not pinned."""
    cat = movies_content_catalog
    q = torch.as_tensor(np.asarray(query_embedding, dtype=np.float64).reshape(1, -1),
                        device=cat.device)
    scores, rows = score_topk(cat, k, queries=q)
    s, r = scores[0].cpu().numpy(), rows[0].cpu().numpy()
    keep = r >= 0
    return [cat.id_of(int(x)) for x in r[keep]], [float(x) for x in s[keep]]


def run_search_exact(query_embedding, user_id: Optional[str] = None,
                     k: int = SIMILARITY_TOP_K) -> List[Recommendation]:
    """lib.py:66-122 without the LLM: exact content retrieval of the query embedding, then the
    reference's re-ranking (user mean-cosine or popularity, 0.9 / 0.1 weights)."""
    ids, scores = retrieve_content_matches(query_embedding, k)
    return rerank_search_matches(ids, scores, user_id)


def user_movie_scores(user_id: str, match_ids: List[str]) -> pd.Series:
    """lib.py:94-106: mean cosine of the user's liked movies vs the query matches, float64,
    indexed by the match ids (in the given order). Raises ValueError when the user has no liked
    movie, exactly like the reference (its no-liked branch at :101-102 falls through into
    cosine_similarity with 0 rows)."""
    cat = movies_collab_catalog
    ur = _user_ratings(user_id)
    liked = cat.rows_of(ur[ur["rating"] >= LIKED_MOVIE_SCORE]["tmdb_id"])
    if not liked:
        raise ValueError(f"Found array with 0 sample(s) (shape=(0, {cat.d})) while a minimum of 1 "
                         "is required by check_pairwise_arrays.")
    qb = prepare_queries(cat, liked=csr_from_lists([liked], cat.device))
    match_rows = torch.tensor([cat.rows_of(match_ids)], dtype=torch.int64, device=cat.device)
    s, r = rescore_rows(cat, qb, match_rows)
    by_row = dict(zip(r[0].cpu().tolist(), s[0].cpu().tolist()))
    rows = cat.rows_of(match_ids)
    return pd.Series([by_row[x] for x in rows], index=list(match_ids))


def reweight(query_movie_scores: pd.Series, user_scores: pd.Series,
             weight: float = QUERY_SCORE_WEIGHT) -> pd.Series:
    """lib.py:117: weighted average of the query and user scores, sorted by id."""
    return (weight * query_movie_scores + (1 - weight) * user_scores).sort_index()


def popularity_scores(movies: List[Movie]) -> pd.Series:
    """lib.py:111-114: min-max scaled popularity of the query matches (no user given)."""
    s = pd.Series(data=[m.popularity for m in movies], index=[m.tmdb_id for m in movies])
    return (s - s.min()) / (s.max() - s.min())


def rerank_search_matches(match_ids: List[str], match_scores: List[float],
                          user_id: Optional[str] = None) -> List[Recommendation]:
    """lib.py:81-122 after the chat-engine retrieval: re-rank the query matches (sorted by id)
    with the user's mean-cosine scores (or popularity) and return them by descending score."""
    order = sorted(range(len(match_ids)), key=lambda i: match_ids[i])  # lib.py:75
    ids = [match_ids[i] for i in order]
    query_scores = pd.Series(data=[match_scores[i] for i in order], index=ids)
    query_movies = get_movies(tmdb_ids=ids)
    if user_id:
        user_scores = user_movie_scores(user_id, ids)
    else:
        user_scores = popularity_scores(query_movies)
    combined = reweight(query_scores, user_scores)
    recs = [Recommendation(movie=m, score=s) for m, s in zip(query_movies, combined)]
    return sorted(recs, key=lambda x: x.score, reverse=True)
