"""Why a row was recommended: the per-liked-row contributions to each returned score.

The reference scores a user by ``cosine_similarity(catalog.loc[liked], catalog).mean(axis=0)``
(``lib.py:51-52``), so every returned score is a sum of one term per liked row,

    score_b(j) = sum_l  w_l cos(x_{r_l}, x_j) / W_b        (w_l = 1, W_b = L_b unweighted),

and ``score_topk`` folds the liked rows into one query vector before its GEMM: it returns the
sum and never holds the terms. ``explain_topk`` computes them afterwards for the rows a search
returned (``ebt_explain_topk``, include/ebert.h 0.9.0: a gathered float64 GEMM of k x d by
d x L_b per query on the float64 MFMA, then a top-m selection per result row) and returns the m
largest -- "because you liked X and Y" -- or, with ``largest=False``, the m smallest, which
with negative weights is "despite Z".

Out of scope: row-sharded catalogs (the liked rows and the result rows must be on one device),
``RecBatcher``, the ``serving.py`` wire format, ``torch.ops.ebert.*`` and ``bench.py``.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from ._lib import EbertError, call, ptr, require_cuda, stream_of
from .catalog import Catalog, require_whole_catalog
from .search import check_weights, device_liked_weights, parse_weight_lists


_ONE_DEVICE = "explanations need the liked rows and the result rows on one device"


class Explanation(NamedTuple):
    """``explain_topk``'s result, all on the catalog's device."""
    contrib: torch.Tensor     # float64 [B, k, m]: the m best contributions, NaN padded
    pos: torch.Tensor         # int32 [B, k, m]: their positions in the liked list, -1 padded
    liked_row: torch.Tensor   # int64 [B, k, m]: the GLOBAL liked rows there, -1 padded
    total: torch.Tensor       # float64 [B, k]: the sum of ALL L_b contributions (the row's score)


def _liked_csr(liked, liked_weights, dev) -> Tuple[torch.Tensor, torch.Tensor,
                                                    Optional[torch.Tensor], np.ndarray]:
    """(offsets, rows, weights or None) on the device and the offsets on the host, from the
    forms score_topk takes: host lists of lists (kept in the caller's order, so that ``pos``
    indexes the caller's list) or a device CSR pair. Weights go through ``check_weights``."""
    if isinstance(liked, tuple):
        off, rows = liked
        require_cuda(off, "liked offsets")
        require_cuda(rows, "liked rows")
        if off.dtype != torch.int64 or rows.dtype != torch.int64:
            raise EbertError("liked CSR must be int64 (offsets, rows)")
        off, rows = off.contiguous(), rows.contiguous()
        off_h = off.cpu().numpy()
        w = None
        if liked_weights is not None:
            w = device_liked_weights(liked_weights, int(rows.numel()))
            check_weights(off_h, w.cpu().numpy())
        return off, rows, w, off_h
    if isinstance(liked_weights, torch.Tensor):
        raise EbertError("with host liked lists, liked_weights must be host lists parallel to "
                         "them")
    segs = [np.asarray(l, dtype=np.int64).ravel() for l in liked]
    off_h = np.zeros(len(segs) + 1, dtype=np.int64)
    np.cumsum([s.size for s in segs], out=off_h[1:])
    flat = np.concatenate(segs) if segs and off_h[-1] else np.zeros(1, dtype=np.int64)
    w = None
    if liked_weights is not None:
        _, ws = parse_weight_lists(segs, liked_weights)
        wflat = np.concatenate(ws) if ws and off_h[-1] else np.zeros(1)
        check_weights(off_h, wflat)
        w = torch.from_numpy(wflat).to(dev)
    return torch.from_numpy(off_h).to(dev), torch.from_numpy(flat).to(dev), w, off_h


def _result_rows(catalog: Catalog, rows: torch.Tensor, B: int) -> torch.Tensor:
    require_cuda(rows, "rows")
    if rows.dtype != torch.int64 or rows.dim() != 2 or rows.shape[0] != B or rows.shape[1] < 1:
        raise EbertError(f"rows must be int64 [{B}, k] (what score_topk returned), got "
                         f"{rows.dtype} {tuple(rows.shape)}")
    return rows.contiguous()


def liked_contrib(catalog: Catalog, rows: torch.Tensor, liked,
                  liked_weights=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor,
                                               torch.Tensor]:
    """``ebt_liked_contrib``: the whole contribution matrix, CSR-shaped. Returns (out float64
    [k * nnz], status int32 [B], liked offsets, liked rows); query b's block is
    ``out[k * off[b] : k * off[b + 1]].view(k, L_b)``. The status is left on the device."""
    require_whole_catalog(catalog, _ONE_DEVICE)
    dev = catalog.device
    off, lrows, w, off_h = _liked_csr(liked, liked_weights, dev)
    B = int(off.numel()) - 1
    rows = _result_rows(catalog, rows, B)
    k = int(rows.shape[1])
    out = torch.empty(max(k * int(off_h[-1]), 1), dtype=torch.float64, device=dev)
    status = torch.empty(max(B, 1), dtype=torch.int32, device=dev)
    call("ebt_liked_contrib", ctypes.byref(catalog.cstruct), B, ptr(off), ptr(lrows), ptr(w),
         ptr(rows), k, ptr(out), ptr(status), stream_of(dev))
    return out, status[:B], off, lrows


def explain_select(contrib: torch.Tensor, off: torch.Tensor, lrows: torch.Tensor, k: int,
                   m: int = 3, largest: bool = True, total: bool = True):
    """``ebt_explain_select`` on a CSR-shaped matrix: (values [B, k, m], positions, liked rows,
    totals [B, k] or None)."""
    dev = contrib.device
    B = int(off.numel()) - 1
    val = torch.empty((B, k, m), dtype=torch.float64, device=dev)
    pos = torch.empty((B, k, m), dtype=torch.int32, device=dev)
    row = torch.empty((B, k, m), dtype=torch.int64, device=dev)
    tot = torch.empty((B, k), dtype=torch.float64, device=dev) if total else None
    call("ebt_explain_select", ptr(contrib), B, ptr(off), ptr(lrows), k, m, 1 if largest else 0,
         ptr(val), ptr(pos), ptr(row), ptr(tot), stream_of(dev))
    return val, pos, row, tot


def explain_topk(catalog: Catalog, rows: torch.Tensor,
                 liked: Union[Tuple[torch.Tensor, torch.Tensor], Sequence[Sequence[int]]],
                 liked_weights=None, m: int = 3, largest: bool = True) -> Explanation:
    """The m liked rows that contributed most (``largest=False``: least) to each returned row.

    rows : int64 [B, k] on the catalog's device, what ``score_topk`` returned (-1 = an empty
        slot; results of masked and materialised-mask calls are parent rows and qualify).
    liked, liked_weights : as ``score_topk`` takes them -- host lists of lists of GLOBAL rows
        (with parallel lists of weights), or a device CSR pair (with a device float64 [nnz]
        tensor). Host lists are used in the caller's order: ``pos`` indexes the caller's list.
    m : 1 .. 64 reasons per row; slots past the list's length are NaN / -1 / -1.

    ``total[b, j]`` is the sum of all of query b's contributions to row j: the score
    ``score_topk`` returned for it, to float64 round-off. A liked or result row outside the
    catalog is never read and raises EbertError naming the query; a query without a liked row
    raises sklearn's ValueError, as ``score_topk`` does. A row-sharded catalog raises EbertError.
    """
    require_whole_catalog(catalog, _ONE_DEVICE)
    if not 1 <= int(m) <= _lib.EBT_EXPLAIN_M_MAX:
        raise EbertError(f"m={m} is outside [1, {_lib.EBT_EXPLAIN_M_MAX}]")
    dev = catalog.device
    off, lrows, w, off_h = _liked_csr(liked, liked_weights, dev)
    B = int(off.numel()) - 1
    if B < 1:
        raise EbertError("empty query batch")
    if (off_h[1:] <= off_h[:-1]).any():
        raise ValueError(f"Found array with 0 sample(s) (shape=(0, {catalog.d})) while a minimum "
                         "of 1 is required by check_pairwise_arrays.")
    rows = _result_rows(catalog, rows, B)
    k, nnz = int(rows.shape[1]), int(off_h[-1])
    need = int(_lib.load().ebt_explain_workspace_bytes(nnz, k))
    if need == 0:
        raise EbertError(f"k={k} over {nnz} liked rows is not supported "
                         "(ebt_explain_workspace_bytes returned 0)")
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    val = torch.empty((B, k, m), dtype=torch.float64, device=dev)
    pos = torch.empty((B, k, m), dtype=torch.int32, device=dev)
    row = torch.empty((B, k, m), dtype=torch.int64, device=dev)
    tot = torch.empty((B, k), dtype=torch.float64, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    call("ebt_explain_topk", ctypes.byref(catalog.cstruct), B, ptr(off), ptr(lrows), ptr(w), nnz,
         ptr(rows), k, int(m), 1 if largest else 0, ptr(ws), need, ptr(val), ptr(pos), ptr(row),
         ptr(tot), ptr(status), stream_of(dev))
    bad = (status != 1).nonzero().flatten().tolist()
    if bad:
        lo, hi = catalog.row_offset, catalog.row_offset + catalog.n
        raise EbertError(f"query {bad[0]}: a liked or result row is outside the catalog rows "
                         f"[{lo}, {hi}) (status -2; queries {bad[:8]})")
    return Explanation(val, pos, row, tot)
