"""Response types of the recommend path (mirror of src/shared/models.py:33-49,73-75).

Only the types the hot path returns are mirrored; the reference's module also imports
llama_index message types for its chat endpoints, which are out of scope here.
"""
from __future__ import annotations

from datetime import date
from typing import List, Optional

from pydantic import BaseModel


class Movie(BaseModel):  # shared/models.py:33-49
    tmdb_id: str
    tmdb_homepage: str
    title: str
    language: str
    release_date: date
    runtime: int
    director: str
    actors: Optional[List[str]]
    genres: Optional[List[str]]
    keywords: Optional[List[str]]
    overview: str
    budget: int
    revenue: int
    popularity: float
    vote_average: float
    vote_count: int


class Recommendation(BaseModel):  # shared/models.py:73-75
    movie: Movie
    score: float


class Reason(BaseModel):  # (no counterpart in the reference: one term of lib.py:51-52's mean)
    tmdb_id: str          # a movie the user rated
    contribution: float   # its term of the recommendation's score
    rating: float         # the user's rating of it


class ExplainedRecommendation(BaseModel):
    movie: Movie
    score: float
    reasons: List[Reason]


class InterestRecommendation(BaseModel):  # (no counterpart in the reference)
    movie: Movie
    score: float          # the mean cosine to the liked movies of ITS interest (lib.py:51-52)
    interest: int         # which of the user's interests it came from, 0 = the largest
    anchor_tmdb_id: str   # that interest's most central liked movie: "more like X"
