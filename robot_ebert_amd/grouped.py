"""Grouped top-k: the k best rows of every category from one scoring pass (ebert.h 0.12.0).

The reference keeps one list per user (``lib.py:51-55``); a front page shows a shelf per genre
("top drama for you", "top comedy for you"). ``score_topk(..., allow=(masks, [g] * B))`` answers
one shelf per call and repeats the whole B x N screening GEMM for query vectors that are the same
in every call. ``score_topk_grouped`` scores once: every score chunk is materialised as the
unfused path does, and one selection (``ebt_select_topk_grouped``) keeps a candidate list per
(query, group) while it streams each score row once; the exact float64 rescore and its
certificate then run per group.

``out[b, g]`` is, bit for bit, what ``score_topk(catalog, k, <the same queries / liked /
liked_weights / exclude>, allow=(masks, [groups[g]] * B))`` returns for query b.

Out of scope: row-sharded catalogs, ``RecBatcher``, the ``serving.py`` wire format,
``torch.ops.ebert.*``, ``bench.py`` and the fused screen (the grouped pass is the unfused path).
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from ._lib import EbertError, call, ptr, stream_of
from .allow import AllowMasks
from .catalog import Catalog
from .search import (DEFAULT_SCORE_BUDGET, _chunk_rows, _clamp_kprime, _liked_with_weights,
                     _pipe_operands, _round_up, _take, _take_weights, check_certificates,
                     exclusions_csr, pad_topk, prepare_queries, score_topk)


class GroupedTopk(NamedTuple):
    """``score_topk_grouped``'s result, on the catalog's device."""
    scores: torch.Tensor   # float64 [B, G, k]: NaN past a group's candidates
    rows: torch.Tensor     # int64 [B, G, k]: GLOBAL rows, -1 past a group's candidates
    group: torch.Tensor    # int32 [G]: the resolved mask ids
    fallback: int          # (b, g) pairs that were re-run through the masked path


def resolve_groups(masks: AllowMasks, groups) -> List[int]:
    """Mask ids of a list of groups: a name goes through ``AllowMasks.index``; an integer is
    taken as it is (an id >= n_masks is an empty shelf, a negative one the unfiltered list)."""
    if isinstance(groups, (str, int, np.integer)):
        groups = [groups]
    ids = []
    for g in groups:
        if isinstance(g, str):
            ids.append(masks.index(g))
            continue
        try:
            ids.append(int(g))
        except (TypeError, ValueError) as e:
            raise EbertError(f"malformed group {g!r}: {e}") from e
    if not ids:
        raise EbertError("groups holds no group")
    for m in ids:
        if not -2 ** 31 <= m < 2 ** 31:
            raise EbertError(f"group id {m} is not an int32")
    return ids


def score_topk_grouped(catalog: Catalog, k: int, masks: AllowMasks, groups,
                       queries: Optional[torch.Tensor] = None, liked=None, exclude=None,
                       liked_weights=None, kprime: Optional[int] = None,
                       chunk_rows: Optional[int] = None, timer: Optional[_lib.Timer] = None,
                       ws_budget: int = 1 << 30) -> GroupedTopk:
    """The top k of every query within each of G groups of rows, from one scoring pass.

    masks, groups : an ``AllowMasks`` over the catalog and a list of its masks, by name or index
        (``resolve_groups``). A row that belongs to several groups appears in each of them; the
        same group may be listed twice.
    queries / liked / liked_weights / exclude : as ``score_topk``'s; the query preparation is
        ``prepare_queries``, shared with it.
    kprime : the screening width (default ``default_kprime``), at most 512; chunk_rows: the rows
        of one score chunk (default: as the unfused path).
    ws_budget : bytes of candidate lists per call; when the lists of all G groups would exceed it,
        the groups -- never the batch -- are split over several calls. No output bit depends on
        it.

    A (query, group) pair whose certificate asks for a wider k' is re-run through the existing
    masked path (``score_topk(..., allow=)``, one call for all such pairs), which widens and falls
    back to the float64 screen on its own; ``fallback`` counts them. Materialised sub-catalogs
    are not used: the parent's bitmaps answer, so a stale copy cannot matter. min(k, rows) > 512
    and row-sharded catalogs raise EbertError; there is no CPU path."""
    k = int(k)
    if k < 1:
        raise EbertError("k must be >= 1")
    if not isinstance(masks, AllowMasks):
        raise EbertError("masks= takes an AllowMasks")
    if catalog.row_offset != 0 or catalog.n_global != catalog.n:
        raise EbertError("grouped top-k on a row-sharded catalog is not supported (this catalog "
                         f"holds {catalog.n} of {catalog.n_global} rows)")
    ids = resolve_groups(masks, groups)
    G = len(ids)
    k_eff = min(k, catalog.n)
    if k_eff > _lib.EBT_GROUPED_KPRIME_MAX:
        raise EbertError(f"k={k} over a {catalog.n}-row catalog is more than the "
                         f"{_lib.EBT_GROUPED_KPRIME_MAX} rows a grouped list holds")
    if kprime is not None and int(kprime) > _lib.EBT_GROUPED_KPRIME_MAX:
        raise EbertError(f"kprime={kprime} is more than {_lib.EBT_GROUPED_KPRIME_MAX}")
    if liked_weights is not None and liked is None:
        raise EbertError("liked_weights= weighs liked rows: pass liked= (dense queries take none)")
    dev = catalog.device
    if torch.device(dev).type != "cuda":
        raise EbertError("the catalog must be on a CUDA (HIP) device; libebert has no CPU path")
    a, b = masks.device, torch.device(dev)
    if a.type != b.type or (a.index is not None and b.index is not None and a.index != b.index):
        raise EbertError(f"the allow masks live on {masks.device}, the catalog on {dev}")
    if 32 * masks.words < catalog.n:
        raise EbertError(f"the allow masks cover {32 * masks.words} rows, the catalog has "
                         f"{catalog.n}")
    # the inputs as score_topk_stages prepares them
    lk, lw = _liked_with_weights(liked, liked_weights, dev) if liked is not None else (None, None)
    ex = exclusions_csr(exclude, dev)
    qb = prepare_queries(catalog, queries=queries, liked=lk, liked_weights=lw)
    B = qb.B
    if ex is not None and int(ex[0].numel()) != B + 1:
        raise EbertError(f"exclude holds {int(ex[0].numel()) - 1} lists for {B} queries")
    kp = min(_clamp_kprime(catalog, k_eff, kprime), _lib.EBT_GROUPED_KPRIME_MAX)
    kp = max(kp, _round_up(k_eff, 4))
    chunk = chunk_rows or _chunk_rows(catalog, qb.B_pad, DEFAULT_SCORE_BUDGET)
    lib = _lib.load()
    # G is split, not B: the candidate lists of one group (the call's other buffers do not grow
    # with G)
    base = int(lib.ebt_cosine_topk_grouped_workspace(B, qb.B_pad, catalog.n, kp, chunk, 0, 1))
    two = int(lib.ebt_cosine_topk_grouped_workspace(B, qb.B_pad, catalog.n, kp, chunk, 0,
                                                   min(2, _lib.EBT_GROUPS_MAX)))
    if base == 0:
        raise EbertError("invalid workspace request")
    per_group = max(two - base, 1)
    part = max(1, min(G, _lib.EBT_GROUPS_MAX, int(ws_budget) // per_group))
    out_s = torch.empty((G, B, k_eff), dtype=torch.float64, device=dev)
    out_r = torch.empty((G, B, k_eff), dtype=torch.int64, device=dev)
    cert = torch.empty((G, B), dtype=torch.int32, device=dev)
    gid = torch.tensor(ids, dtype=torch.int32, device=dev)
    ws = None
    for g0 in range(0, G, part):
        ng = min(part, G - g0)
        need = int(lib.ebt_cosine_topk_grouped_workspace(B, qb.B_pad, catalog.n, kp, chunk, 0, ng))
        if ws is None or ws.numel() < need:
            ws = torch.empty(need, dtype=torch.uint8, device=dev)
        call("ebt_cosine_topk_grouped_prepared",
             *_pipe_operands(catalog, qb, ex, k_eff, kp, chunk, 0),
             ptr(gid[g0:g0 + ng]), ng, ptr(masks.table), masks.words, masks.n_masks,
             ptr(ws), int(ws.numel()), ptr(out_s[g0:g0 + ng]), ptr(out_r[g0:g0 + ng]),
             ptr(cert[g0:g0 + ng]), timer.handle if timer is not None else None, stream_of(dev))
    flat = cert.cpu()
    check_certificates(flat)
    bad = torch.nonzero(flat != 1)   # [(g, b)]: the candidate set is not provably complete
    fallback = int(bad.shape[0])
    if fallback:
        gs, bs = bad[:, 0].tolist(), bad[:, 1].tolist()
        idx = torch.tensor(bs, dtype=torch.int64, device=dev)
        sub_ids = torch.tensor([ids[g] for g in gs], dtype=torch.int32, device=dev)
        s2, r2 = score_topk(
            catalog, k_eff,
            queries=queries.index_select(0, idx) if queries is not None else None,
            liked=_take(liked, bs, idx), exclude=_take(ex if isinstance(exclude, tuple)
                                                       else exclude, bs, idx),
            kprime=kprime, chunk_rows=chunk_rows, timer=timer, allow=(masks, sub_ids),
            liked_weights=_take_weights(liked, liked_weights, bs, idx))
        at = (torch.tensor(gs, dtype=torch.int64, device=dev), idx)
        out_s[at] = s2
        out_r[at] = r2
    out_s, out_r = pad_topk(out_s, out_r, k)
    return GroupedTopk(out_s.permute(1, 0, 2).contiguous(), out_r.permute(1, 0, 2).contiguous(),
                       gid, fallback)
