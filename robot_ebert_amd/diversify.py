"""Diversified top-k: greedy maximal marginal relevance (MMR) over a candidate pool.

The reference sorts by score and cuts at k (``lib.py:51-55``), so the k best rows of a mean-cosine
recommender may be near copies of one another. ``diversify_topk`` re-ranks a pool of the p best
rows of each query (what ``score_topk(catalog, p, ...)`` returned): k picks, each maximising

    lam * relevance - (1 - lam) * (largest cosine to a row already picked),

with the cosine between two catalog rows -- ``lib.py:51``'s quantity -- taken among the results
(``ebt_mmr_topk``, include/ebert.h 0.10.0: a gathered float64 Gram matrix of p x d by d x p per
query on the float64 MFMA, then a sequential greedy selection, one wave per query). ``lam = 1``
returns the pool's own first k.

Out of scope: row-sharded catalogs (the pool rows must be on one device), ``RecBatcher``, the
``serving.py`` wire format, ``torch.ops.ebert.*`` and ``bench.py``.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional, Tuple

import torch

from . import _lib
from ._lib import EbertError, call, ptr, require_cuda, stream_of
from .catalog import Catalog, require_whole_catalog


class Diversified(NamedTuple):
    """``diversify_topk``'s result, all on the catalog's device, in selection order."""
    rows: torch.Tensor     # int64 [B, k]: the GLOBAL rows picked, -1 padded
    scores: torch.Tensor   # float64 [B, k]: their relevances (the input's bits), NaN padded
    mmr: torch.Tensor      # float64 [B, k]: the value each pick maximised, NaN padded
    pos: torch.Tensor      # int32 [B, k]: their positions in the pool, -1 padded


def _check_lam(lam) -> float:
    lam = float(lam)
    if not 0.0 <= lam <= 1.0:       # (a NaN fails both comparisons)
        raise EbertError(f"lam={lam} is outside [0, 1]")
    return lam


def _check_pool(p: int) -> None:
    if not 1 <= p <= _lib.EBT_MMR_POOL_MAX:
        raise EbertError(f"a pool of p={p} rows is outside [1, {_lib.EBT_MMR_POOL_MAX}]")


def _shape_of(rows, what: str) -> Tuple[int, int]:
    shape = tuple(getattr(rows, "shape", ()))
    if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
        raise EbertError(f"{what} must be [B, p] (what score_topk returned), got {shape}")
    return int(shape[0]), int(shape[1])


def _pool_rows(rows: torch.Tensor) -> torch.Tensor:
    require_cuda(rows, "rows")
    if rows.dtype != torch.int64:
        raise EbertError(f"rows must be int64 [B, p] (what score_topk returned), got {rows.dtype}")
    return rows.contiguous()


def _pool_scores(scores: torch.Tensor, B: int, p: int) -> torch.Tensor:
    require_cuda(scores, "scores")
    if scores.dtype != torch.float64 or tuple(scores.shape) != (B, p):
        raise EbertError(f"scores must be float64 [{B}, {p}] (what score_topk returned), got "
                         f"{scores.dtype} {tuple(scores.shape)}")
    return scores.contiguous()


def pool_gram(catalog: Catalog, rows: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``ebt_pool_gram``: (gram float64 [B, p, p], status int32 [B]); ``gram[b, i, j]`` is the
    cosine between pool slots i and j of query b, NaN where either is empty (-1). The status is
    left on the device (1, or -2 for a query with a row outside the catalog: all NaN)."""
    require_whole_catalog(catalog, "diversification needs the pool rows on one device")
    B, p = _shape_of(rows, "rows")
    _check_pool(p)
    rows = _pool_rows(rows)
    dev = catalog.device
    gram = torch.empty((B, p, p), dtype=torch.float64, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    call("ebt_pool_gram", ctypes.byref(catalog.cstruct), B, ptr(rows), p, ptr(gram), ptr(status),
         stream_of(dev))
    return gram, status


def mmr_select(gram: torch.Tensor, scores: torch.Tensor, rows: torch.Tensor, k: int, lam: float,
               status: Optional[torch.Tensor] = None) -> Diversified:
    """``ebt_mmr_select`` on a Gram matrix [B, p, p]: the greedy selection alone."""
    lam = _check_lam(lam)
    B, p = _shape_of(rows, "rows")
    _check_pool(p)
    if not 1 <= int(k) <= p:
        raise EbertError(f"k={k} is outside [1, p={p}]")
    rows = _pool_rows(rows)
    scores = _pool_scores(scores, B, p)
    require_cuda(gram, "gram")
    if gram.dtype != torch.float64 or tuple(gram.shape) != (B, p, p):
        raise EbertError(f"gram must be float64 [{B}, {p}, {p}], got {gram.dtype} "
                         f"{tuple(gram.shape)}")
    gram = gram.contiguous()
    dev = rows.device
    out = _outputs(B, int(k), dev)
    call("ebt_mmr_select", ptr(gram), ptr(scores), ptr(rows), B, p, int(k), lam, ptr(status),
         ptr(out.pos), ptr(out.rows), ptr(out.scores), ptr(out.mmr), stream_of(dev))
    return out


def _outputs(B: int, k: int, dev) -> Diversified:
    return Diversified(torch.empty((B, k), dtype=torch.int64, device=dev),
                       torch.empty((B, k), dtype=torch.float64, device=dev),
                       torch.empty((B, k), dtype=torch.float64, device=dev),
                       torch.empty((B, k), dtype=torch.int32, device=dev))


def diversify_topk(catalog: Catalog, scores: torch.Tensor, rows: torch.Tensor, k: int,
                   lam: float = 0.7, ws_budget: int = 1 << 30) -> Diversified:
    """k of the p pool rows of every query, picked greedily by maximal marginal relevance.

    scores, rows : float64 / int64 [B, p] on the catalog's device, what ``score_topk(catalog, p,
        ...)`` returned (-1 / NaN = an empty slot; results of masked and materialised-mask calls
        are parent rows and qualify). p <= 512.
    k : 1 .. p picks per query; slots past the candidates are -1 / NaN / NaN / -1.
    lam : 0 .. 1; 1 keeps the pool's order (its own first k, bit for bit), 0 ignores relevance
        after the first pick.
    ws_budget : bytes of workspace per call; the batch is split so that each call's Gram
        matrices (8 p^2 bytes per query) fit. One query always fits (2 MiB at p = 512).

    A pool row outside the catalog is never read and raises EbertError naming the query; a
    row-sharded catalog raises EbertError."""
    require_whole_catalog(catalog, "diversification needs the pool rows on one device")
    lam = _check_lam(lam)
    B, p = _shape_of(rows, "rows")
    _check_pool(p)
    if not 1 <= int(k) <= p:
        raise EbertError(f"k={k} is outside [1, p={p}]")
    k = int(k)
    rows = _pool_rows(rows)
    scores = _pool_scores(scores, B, p)
    dev = catalog.device
    lib = _lib.load()
    per = int(lib.ebt_mmr_workspace_bytes(1, p))
    chunk = max(1, min(B, int(ws_budget) // per))
    need = int(lib.ebt_mmr_workspace_bytes(chunk, p))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    out = _outputs(B, k, dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    for b0 in range(0, B, chunk):
        nb = min(chunk, B - b0)
        call("ebt_mmr_topk", ctypes.byref(catalog.cstruct), nb, ptr(scores[b0:]), ptr(rows[b0:]),
             p, k, lam, ptr(ws), need, ptr(out.pos[b0:]), ptr(out.rows[b0:]),
             ptr(out.scores[b0:]), ptr(out.mmr[b0:]), ptr(status[b0:]), stream_of(dev))
    bad = (status != 1).nonzero().flatten().tolist()
    if bad:
        lo, hi = catalog.row_offset, catalog.row_offset + catalog.n
        raise EbertError(f"query {bad[0]}: a pool row is outside the catalog rows [{lo}, {hi}) "
                         f"(status -2; queries {bad[:8]})")
    return out
