"""The recommend route, unchanged, over the GPU drop-in.

Mirrors /root/reference/src/backend/app/api/users.py:150-155 -- same path, same query
parameter, same response model, same behaviour on errors: ``get_user_recs`` raising (sklearn's
ValueError for a user without liked movies, lib.py:51) is not caught, so the server answers
HTTP 500 exactly as the reference's app does. The only difference is the import: the handler
calls ``robot_ebert_amd.lib.get_user_recs`` (HBM-resident catalog, HIP scoring) instead of
``backend.app.lib.get_user_recs`` (sklearn + pandas). ``app()`` assembles a FastAPI app the
way /root/reference/src/backend/app/main.py:11-12 does (users router, tag "Users"); the
reference's other routers (movies, search, login) are out of scope.
"""
from __future__ import annotations

from typing import Dict, List, Optional

from fastapi import APIRouter, FastAPI, Query

from . import lib
from .models import ExplainedRecommendation, InterestRecommendation, Recommendation

router = APIRouter()
# a batcher.RecBatcher installed by app(batcher=...): the handler's scoring step is then
# coalesced with the other worker threads' requests; None = one call per request
_batcher = None


@router.get("/users/{user_id}/recommendations/")
def get_user_recommendations(user_id: str, k: int = 10) -> List[Recommendation]:
    """get unconditional movie recommendations for an existing user by ID"""
    if _batcher is not None:
        return lib.get_user_recs_batched(_batcher, user_id=user_id, k=k)
    user_recommendations = lib.get_user_recs(user_id=user_id, k=k)
    return user_recommendations


@router.get("/users/{user_id}/recommendations/explained/")
def get_user_recommendations_explained(user_id: str, k: int = 10,
                                       m: int = 3) -> List[ExplainedRecommendation]:
    """the same recommendations, each with the m rated movies that contributed most to its score
    (no counterpart in the reference; never batched)"""
    return lib.get_user_recs_explained(user_id=user_id, k=k, m=m)


@router.get("/users/{user_id}/recommendations/diverse/")
def get_user_recommendations_diverse(user_id: str, k: int = 10,
                                     lam: float = Query(0.7, ge=0.0, le=1.0),
                                     pool: Optional[int] = Query(None, ge=1, le=512)
                                     ) -> List[Recommendation]:
    """k recommendations picked from the pool best by maximal marginal relevance, in selection
    order: lam = 1 is the plain top k, smaller values trade relevance for variety (no
    counterpart in the reference; never batched)"""
    return lib.get_user_recs_diverse(user_id=user_id, k=k, lam=lam, pool=pool)


@router.get("/users/{user_id}/recommendations/interests/")
def get_user_recommendations_interests(user_id: str, k: int = 10,
                                       interests: int = Query(3, ge=1, le=8)
                                       ) -> List[InterestRecommendation]:
    """k recommendations drawn from up to `interests` clusters of the user's liked movies in
    proportion to the clusters' sizes, each with the cluster's most central liked movie as its
    anchor (no counterpart in the reference; never batched)"""
    return lib.get_user_recs_interests(user_id=user_id, k=k, interests=interests)


@router.get("/users/{user_id}/recommendations/by-group/")
def get_user_recommendations_by_group(user_id: str, k: int = 10,
                                      groups: Optional[str] = None
                                      ) -> Dict[str, List[Recommendation]]:
    """one shelf of k recommendations per group ("top drama for you"): `groups` is a
    comma-separated list of mask names or indices of the configured allow masks (default: every
    mask), all shelves scored in one pass (no counterpart in the reference; never batched)"""
    names = [g.strip() for g in groups.split(",") if g.strip()] if groups is not None else None
    return lib.get_user_recs_by_group(user_id=user_id, k=k, groups=names)


def app(batcher=None) -> FastAPI:
    """FastAPI app with the users router (main.py:11-12); configure ``lib`` first. With a
    ``batcher.RecBatcher`` over ``lib.movies_collab_catalog`` the route's requests share GPU
    batches (same answers, same errors)."""
    global _batcher
    _batcher = batcher
    a = FastAPI()
    a.include_router(router, tags=["Users"])
    return a
