"""Multi-interest top-k: cluster a user's liked rows, search once per cluster, interleave.

The reference scores a user as the mean cosine to everything they liked (``lib.py:51-52``), and
the library folds that mean into one query vector: a user with two or three distinct tastes is
searched at the centroid of those tastes, and the top k sits between them. ``cluster_liked``
groups the liked rows of each query into up to c clusters (``ebt_liked_interests``, include/ebert.h
0.11.0: the float64 cosine matrix of the list, then seeding and reassignment passes in which a row
joins the cluster whose members' mean cosine to it -- the reference's own score of that row
against the cluster as a liked list -- is largest); ``multi_interest_topk`` scores every cluster's
member list with ``score_topk`` and merges the answers, each cluster taking output slots in
proportion to its size (``ebt_interest_interleave``, the highest-averages rule). ``c = 1`` is
``score_topk`` bit for bit.

Out of scope: ``liked_weights``, ``allow=``, row-sharded catalogs (the liked rows must be on one
device), ``RecBatcher``, the ``serving.py`` wire format, ``torch.ops.ebert.*`` and ``bench.py``.
"""
from __future__ import annotations

import ctypes
from typing import List, NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import EbertError, call, ptr, stream_of
from .catalog import Catalog, require_whole_catalog
from .search import score_topk

_SKLEARN_EMPTY = ("Found array with 0 sample(s) (shape=(0, {d})) while a minimum of 1 is required "
                  "by check_pairwise_arrays.")


class Interests(NamedTuple):
    """``cluster_liked``'s result, all on the catalog's device. P is the longest list's length;
    positions are those of ``rows`` (each list sorted ascending)."""
    label: torch.Tensor    # int32 [B, P]: the cluster of each liked row, -1 past the list
    size: torch.Tensor     # int32 [B, c]: members per cluster, descending; 0 = no such cluster
    medoid: torch.Tensor   # int32 [B, c]: the position of each cluster's medoid, -1 = none
    iters: torch.Tensor    # int32 [B]: reassignment passes run (EBT_INTEREST_ITERS = the cap)
    rows: torch.Tensor     # int64 [B, P]: the GLOBAL liked rows, sorted, -1 padded


class MultiInterest(NamedTuple):
    """``multi_interest_topk``'s result, all on the catalog's device, in interleave order."""
    rows: torch.Tensor        # int64 [B, k]: the GLOBAL rows, -1 padded
    scores: torch.Tensor      # float64 [B, k]: score_topk's score of the row for ITS cluster's list
    cluster: torch.Tensor     # int32 [B, k]: the cluster each row came from, -1 padded
    pos: torch.Tensor         # int32 [B, k]: its rank in that cluster's own top k, -1 padded
    size: torch.Tensor        # int32 [B, c]: members per cluster (cluster_liked's)
    medoid_row: torch.Tensor  # int64 [B, c]: the GLOBAL row of each cluster's medoid, -1 = none


def _check_c(c) -> int:
    if not 1 <= int(c) <= _lib.EBT_INTEREST_MAX:
        raise EbertError(f"c={c} clusters is outside [1, {_lib.EBT_INTEREST_MAX}]")
    return int(c)


def _host_lists(lists, what: str) -> List[np.ndarray]:
    """score_topk's list forms (host lists, or a device CSR of offsets and GLOBAL rows) as sorted
    int64 arrays, one per query."""
    if isinstance(lists, tuple):
        off, rows = (np.asarray(t.cpu().numpy(), dtype=np.int64) for t in lists[:2])
        lists = [rows[off[b]:off[b + 1]] for b in range(len(off) - 1)]
    out = [np.sort(np.asarray(l, dtype=np.int64).ravel()) for l in lists]
    if not out:
        raise EbertError(f"{what} holds no query")
    return out


def _bucket(length: int) -> int:
    p = 16
    while p < length:
        p *= 2
    return p


def cluster_liked(catalog: Catalog, liked, c: int = 3, ws_budget: int = 1 << 30) -> Interests:
    """Up to c clusters of every query's liked rows (include/ebert.h 0.11.0, ebt_liked_interests).

    liked : the list forms ``score_topk`` takes (host lists of GLOBAL rows, or a device CSR). Each
        list is sorted ascending, so positions follow row order and the result does not depend on
        the caller's order; at most 512 rows per query.
    c : 1 .. 8 clusters; a list of fewer rows has that many. Clusters are numbered by (size
        descending, lowest member ascending).
    ws_budget : bytes of workspace per call. Queries are grouped by length (padded with -1 to 16,
        32, ... 512 slots) and each group is split so that its matrices (8 p^2 bytes per query)
        fit; neither changes any output.

    A list longer than 512 rows or with a row outside the catalog raises EbertError naming the
    query (no such row is read); a row-sharded catalog raises EbertError; an empty list raises
    sklearn's ValueError, as ``score_topk`` does."""
    require_whole_catalog(catalog, "multi-interest search needs the liked rows on one device")
    c = _check_c(c)
    lists = _host_lists(liked, "liked")
    B = len(lists)
    lo, hi = catalog.row_offset, catalog.row_offset + catalog.n
    for b, l in enumerate(lists):
        if l.size == 0:
            raise ValueError(_SKLEARN_EMPTY.format(d=catalog.d))
        if l.size > _lib.EBT_MMR_POOL_MAX:
            raise EbertError(f"query {b}: {l.size} liked rows, more than the "
                             f"{_lib.EBT_MMR_POOL_MAX} a call can cluster")
        if l[0] < lo or l[-1] >= hi:
            raise EbertError(f"query {b}: a liked row is outside the catalog rows [{lo}, {hi})")
    dev = catalog.device
    if torch.device(dev).type != "cuda":     # the last host check
        raise EbertError("the catalog must be on a CUDA (HIP) device; libebert has no CPU path")
    lib = _lib.load()
    P = max(l.size for l in lists)
    rows_host = np.full((B, P), -1, dtype=np.int64)
    for b, l in enumerate(lists):
        rows_host[b, :l.size] = l
    out = Interests(torch.full((B, P), -1, dtype=torch.int32, device=dev),
                    torch.zeros((B, c), dtype=torch.int32, device=dev),
                    torch.full((B, c), -1, dtype=torch.int32, device=dev),
                    torch.zeros(B, dtype=torch.int32, device=dev),
                    torch.from_numpy(rows_host).to(dev))
    buckets = {}
    for b, l in enumerate(lists):
        buckets.setdefault(_bucket(l.size), []).append(b)
    bad: List[int] = []
    for p, members in sorted(buckets.items()):
        w = min(p, P)
        per = int(lib.ebt_interest_workspace_bytes(1, p))
        chunk = max(1, min(len(members), int(ws_budget) // per))
        need = int(lib.ebt_interest_workspace_bytes(chunk, p))
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        for m0 in range(0, len(members), chunk):
            idx = members[m0:m0 + chunk]
            nb = len(idx)
            padded = np.full((nb, p), -1, dtype=np.int64)
            padded[:, :w] = rows_host[idx, :w]
            rows = torch.from_numpy(padded).to(dev)
            label = torch.empty((nb, p), dtype=torch.int32, device=dev)
            size = torch.empty((nb, c), dtype=torch.int32, device=dev)
            medoid = torch.empty((nb, c), dtype=torch.int32, device=dev)
            iters = torch.empty(nb, dtype=torch.int32, device=dev)
            status = torch.empty(nb, dtype=torch.int32, device=dev)
            call("ebt_liked_interests", ctypes.byref(catalog.cstruct), nb, ptr(rows), p, c,
                 ptr(ws), need, ptr(label), ptr(size), ptr(medoid), ptr(iters), ptr(status),
                 stream_of(dev))
            it = torch.as_tensor(idx, dtype=torch.int64, device=dev)
            out.label[it, :w] = label[:, :w]
            out.size[it] = size
            out.medoid[it] = medoid
            out.iters[it] = iters
            bad += [idx[i] for i in (status != 1).nonzero().flatten().tolist()]
    if bad:
        bad.sort()
        raise EbertError(f"query {bad[0]}: a liked row is outside the catalog rows [{lo}, {hi}) "
                         f"(status -2; queries {bad[:8]})")
    return out


def interest_cluster(gram: torch.Tensor, rows: torch.Tensor, c: int,
                     status: Optional[torch.Tensor] = None):
    """``ebt_interest_cluster`` on cosine matrices [B, p, p] (``diversify.pool_gram``'s) of the
    lists rows [B, p] (-1 = an empty slot anywhere): the clustering alone, (label int32 [B, p],
    size int32 [B, c], medoid int32 [B, c], iters int32 [B])."""
    c = _check_c(c)
    _lib.require_cuda(rows, "rows")
    if rows.dim() != 2 or rows.dtype != torch.int64:
        raise EbertError(f"rows must be int64 [B, p], got {rows.dtype} {tuple(rows.shape)}")
    B, p = (int(x) for x in rows.shape)
    if not 1 <= p <= _lib.EBT_MMR_POOL_MAX:
        raise EbertError(f"a list of p={p} slots is outside [1, {_lib.EBT_MMR_POOL_MAX}]")
    if gram.dtype != torch.float64 or tuple(gram.shape) != (B, p, p):
        raise EbertError(f"gram must be float64 [{B}, {p}, {p}], got {gram.dtype} "
                         f"{tuple(gram.shape)}")
    dev = rows.device
    rows, gram = rows.contiguous(), gram.contiguous()
    label = torch.empty((B, p), dtype=torch.int32, device=dev)
    size = torch.empty((B, c), dtype=torch.int32, device=dev)
    medoid = torch.empty((B, c), dtype=torch.int32, device=dev)
    iters = torch.empty(B, dtype=torch.int32, device=dev)
    call("ebt_interest_cluster", ptr(gram), ptr(rows), B, p, c, ptr(status), ptr(label),
         ptr(size), ptr(medoid), ptr(iters), stream_of(dev))
    return label, size, medoid, iters


def interleave(size: torch.Tensor, list_rows: torch.Tensor,
               list_scores: torch.Tensor):
    """``ebt_interest_interleave`` on per-cluster lists [B, c, k] and sizes [B, c]: (rows int64,
    scores float64, cluster int32, pos int32), each [B, k]."""
    _lib.require_cuda(list_rows, "list_rows")
    if list_rows.dim() != 3 or list_rows.dtype != torch.int64:
        raise EbertError(f"list_rows must be int64 [B, c, k], got {list_rows.dtype} "
                         f"{tuple(list_rows.shape)}")
    B, c, k = (int(x) for x in list_rows.shape)
    _check_c(c)
    if not 1 <= k <= _lib.EBT_INTEREST_K_MAX:
        raise EbertError(f"k={k} is outside [1, {_lib.EBT_INTEREST_K_MAX}]")
    if list_scores.dtype != torch.float64 or tuple(list_scores.shape) != (B, c, k):
        raise EbertError(f"list_scores must be float64 [{B}, {c}, {k}], got {list_scores.dtype} "
                         f"{tuple(list_scores.shape)}")
    if size.dtype != torch.int32 or tuple(size.shape) != (B, c):
        raise EbertError(f"size must be int32 [{B}, {c}], got {size.dtype} {tuple(size.shape)}")
    dev = list_rows.device
    size, list_rows, list_scores = size.contiguous(), list_rows.contiguous(), list_scores.contiguous()
    rows = torch.empty((B, k), dtype=torch.int64, device=dev)
    scores = torch.empty((B, k), dtype=torch.float64, device=dev)
    cluster = torch.empty((B, k), dtype=torch.int32, device=dev)
    pos = torch.empty((B, k), dtype=torch.int32, device=dev)
    call("ebt_interest_interleave", ptr(size), ptr(list_rows), ptr(list_scores), B, c, k,
         ptr(rows), ptr(scores), ptr(cluster), ptr(pos), stream_of(dev))
    return rows, scores, cluster, pos


def multi_interest_topk(catalog: Catalog, k: int, liked, c: int = 3,
                        exclude: Optional[Sequence[Sequence[int]]] = None) -> MultiInterest:
    """The top k of every query, drawn from up to c interests of its liked rows.

    ``cluster_liked`` groups the liked rows; ONE ``score_topk(catalog, k, liked=<the member lists
    of all non-empty clusters>, exclude=<each query's exclusions, once per cluster>)`` call scores
    them; ``ebt_interest_interleave`` merges each query's lists: the cluster with the largest
    size / (slots taken + 1) emits its best row not yet emitted, ties to the lower cluster.
    ``scores[b, t]`` is, bit for bit, what ``score_topk`` returns for that cluster's member list;
    with c = 1 the whole result is ``score_topk(catalog, k, liked, exclude)``'s.

    k : 1 .. 512. liked, exclude : the list forms ``score_topk`` takes. Errors as
    ``cluster_liked``'s."""
    require_whole_catalog(catalog, "multi-interest search needs the liked rows on one device")
    c = _check_c(c)
    k = int(k)
    if not 1 <= k <= _lib.EBT_INTEREST_K_MAX:
        raise EbertError(f"k={k} is outside [1, {_lib.EBT_INTEREST_K_MAX}]")
    lists = _host_lists(liked, "liked")
    B = len(lists)
    excl = None
    if exclude is not None:
        excl = _host_lists(exclude, "exclude")
        if len(excl) != B:
            raise EbertError(f"exclude holds {len(excl)} lists for {B} queries")
    ints = cluster_liked(catalog, lists, c=c)
    dev = catalog.device
    label, size = ints.label.cpu().numpy(), ints.size.cpu().numpy()
    members, owner, member_excl = [], [], []
    for b, l in enumerate(lists):
        for m in range(c):
            if size[b, m] > 0:
                members.append(l[label[b, :l.size] == m])
                owner.append(b * c + m)
                if excl is not None:
                    member_excl.append(excl[b])
    s, r = score_topk(catalog, k, liked=members, exclude=member_excl if excl is not None else None)
    list_rows = torch.full((B * c, k), -1, dtype=torch.int64, device=dev)
    list_scores = torch.full((B * c, k), float("nan"), dtype=torch.float64, device=dev)
    at = torch.as_tensor(owner, dtype=torch.int64, device=dev)
    list_rows[at] = r
    list_scores[at] = s
    rows, scores, cluster, pos = interleave(ints.size, list_rows.view(B, c, k),
                                            list_scores.view(B, c, k))
    med = ints.medoid.long()
    medoid_row = torch.where(med >= 0, torch.gather(ints.rows, 1, med.clamp(min=0)),
                             torch.full_like(med, -1))
    return MultiInterest(rows, scores, cluster, pos, ints.size, medoid_row)
