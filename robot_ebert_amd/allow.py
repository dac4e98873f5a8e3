"""Per-query allow masks: top-k within a subset of the catalog rows (include/ebert.h, 0.6.0).

The reference's candidate set is ``index.difference(rated)`` (lib.py:48,55); a filtered query
intersects it with the rows its mask allows ("within this genre", "only this tenant's items").
``AllowMasks`` owns the device table ``uint32 [n_masks, words]`` (held in an int32 tensor, the
same bits; bit r of mask m = GLOBAL row r is allowed in m) and is passed to
``score_topk(..., allow=(masks, mask_ids))``; its bits are written by the library's kernels
(ebt_allow_from_bool, ebt_allow_set_rows).

A sparse mask can be MATERIALISED (include/ebert.h, 0.7.0): ``materialize(mask)`` copies its
allowed rows once into a dense sub-catalog, and ``score_topk`` then scores the queries filtered by
that mask over those m rows -- through every existing path, the fused screen included -- instead of
over all n rows followed by the mask pass. Rows and float64 scores are the same, bit for bit; the
copy costs m / n of the catalog's matrix and image, and is rebuilt after the mask or the catalog
changes (a stale copy is never used: the mask pass answers).
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import EbertError, call, ptr, require_cuda, stream_of


def allow_words(n_rows: int) -> int:
    """ebt_allow_words: uint32 words of one mask row covering n_rows rows (a multiple of 4)."""
    return int(_lib.load().ebt_allow_words(int(n_rows)))


def _round_up(v: int, m: int) -> int:
    return (v + m - 1) // m * m


@dataclass
class SubCatalog:
    """One materialised mask: its allowed rows as a catalog of their own (Catalog.from_parts over
    the tensors ebt_catalog_gather_rows filled), the row list that maps its rows back to GLOBAL
    rows and the rank prefix that maps GLOBAL rows into it."""
    catalog: object            # the m-row Catalog
    rows: torch.Tensor         # int64 [m]: GLOBAL row of sub-catalog row i, ascending
    rank: torch.Tensor         # uint32 [words] (held as int32): allowed rows in all earlier words
    m: int
    n_rows: int                # the parent's n when it was built: bits at or above it are ignored
    edits: int                 # the parent's edit counter when it was built


class AllowMasks:
    """``n_masks`` allow masks over the rows of a catalog.

    catalog_or_n_rows : the Catalog the masks belong to (sized for its ``capacity``, so appended
        rows have a bit; ``n_global`` for a shard) or a row count (then ``device=`` says where).
    names : optional mask names, for ``index(name)`` and by-name lookups.

    All masks start empty: no row is allowed until ``set`` / ``from_bool`` says so, and a row
    appended to the catalog later is allowed in no mask until it is set. After
    ``Catalog.remove``, pass the moves it returned to ``apply_moves``.
    """

    def __init__(self, catalog_or_n_rows, n_masks: int, names: Optional[Sequence[str]] = None,
                 device=None) -> None:
        self.catalog = None
        if isinstance(catalog_or_n_rows, (int, np.integer)):
            n_rows = int(catalog_or_n_rows)
            dev = torch.device(device if device is not None else "cuda")
        else:
            self.catalog = catalog_or_n_rows
            cat = catalog_or_n_rows
            n_rows = max(int(cat.capacity), int(cat.n_global))
            dev = cat.device
        if n_rows < 1 or int(n_masks) < 1:
            raise EbertError(f"AllowMasks needs n_rows >= 1 and n_masks >= 1 (got {n_rows}, "
                             f"{n_masks})")
        if names is not None and len(names) != int(n_masks):
            raise EbertError(f"{len(names)} names for {n_masks} masks")
        self.n_rows = n_rows
        self.n_masks = int(n_masks)
        self.names = list(names) if names is not None else None
        self.words = allow_words(n_rows)
        self.device = dev
        self.table = torch.zeros((self.n_masks, self.words), dtype=torch.int32, device=dev)
        self._subs: Dict[int, SubCatalog] = {}   # materialised masks (materialize)

    # ---- lookups ------------------------------------------------------------------------------
    def index(self, name_or_index) -> int:
        """The index of a mask given its name (or a valid index, returned as it is)."""
        if isinstance(name_or_index, str):
            if self.names is None or name_or_index not in self.names:
                raise EbertError(f"unknown allow mask {name_or_index!r}")
            return self.names.index(name_or_index)
        try:
            m = int(name_or_index)
        except (TypeError, ValueError) as e:
            raise EbertError(f"malformed allow mask index: {e}") from e
        if m < 0 or m >= self.n_masks:
            raise EbertError(f"allow mask {m} is not in [0, {self.n_masks})")
        return m

    def _row(self, mask) -> torch.Tensor:
        return self.table[self.index(mask)]

    # ---- writers ------------------------------------------------------------------------------
    def set(self, mask, rows_or_ids, allowed: bool = True) -> None:
        """Allow (or disallow) a list of GLOBAL rows -- or string ids of the catalog -- in one
        mask (ebt_allow_set_rows). Rows outside the table are refused here."""
        row = self._row(mask)
        self._subs.pop(self.index(mask), None)   # its copy no longer matches the bits
        if isinstance(rows_or_ids, torch.Tensor):
            require_cuda(rows_or_ids, "rows")
            rows = rows_or_ids.to(torch.int64).contiguous().flatten()
        else:
            items = list(rows_or_ids)
            if any(isinstance(t, str) for t in items):
                if self.catalog is None:
                    raise EbertError("ids need the Catalog the masks were built for")
                try:
                    items = self.catalog.rows_of(items)
                except KeyError as e:
                    raise EbertError(f"unknown id {e}") from e
            try:
                host = np.asarray([int(r) for r in items], dtype=np.int64)
            except (TypeError, ValueError) as e:
                raise EbertError(f"malformed rows: {e}") from e
            if host.size and (host.min() < 0 or host.max() >= self.n_rows):
                raise EbertError(f"rows must be in [0, {self.n_rows})")
            rows = torch.from_numpy(host).to(self.device)
        if rows.numel() == 0:
            return
        call("ebt_allow_set_rows", ptr(row), self.words, ptr(rows), int(rows.numel()),
             1 if allowed else 0, stream_of(self.device))

    def from_bool(self, mask, flags: torch.Tensor) -> None:
        """Replace one mask by a boolean (or uint8) vector over rows [0, len(flags)): non-zero =
        allowed, rows past it not allowed (ebt_allow_from_bool)."""
        row = self._row(mask)
        self._subs.pop(self.index(mask), None)
        if not isinstance(flags, torch.Tensor):
            flags = torch.from_numpy(np.asarray(flags).astype(np.uint8)).to(self.device)
        require_cuda(flags, "flags")
        if flags.dim() != 1 or flags.numel() > 32 * self.words:
            raise EbertError(f"flags must be a vector of at most {32 * self.words} rows")
        if flags.dtype == torch.bool:
            flags = flags.to(torch.uint8)
        elif flags.dtype != torch.uint8:
            flags = (flags != 0).to(torch.uint8)
        flags = flags.contiguous()
        call("ebt_allow_from_bool", ptr(flags), int(flags.numel()), ptr(row), self.words,
             stream_of(self.device))

    def apply_moves(self, moves: Sequence[Tuple[int, int]], n_new: int) -> None:
        """Follow ``Catalog.remove``: for each (old, new) of its moves bit[new] = bit[old] in
        every mask, then the bits of rows >= n_new are cleared. (Sources are >= n_new and
        destinations < n_new, so the order of the moves does not matter.)"""
        n_new = int(n_new)
        if n_new < 0 or n_new > 32 * self.words:
            raise EbertError(f"n_new={n_new} is outside the table's rows")
        moves = [(int(s), int(t)) for s, t in moves]
        self._subs.clear()   # every mask is touched
        for s, t in moves:
            if not (0 <= t < n_new <= s < 32 * self.words):
                raise EbertError(f"move ({s}, {t}) is not one of a removal down to {n_new} rows")
        if moves:
            src = torch.tensor([s for s, _ in moves], dtype=torch.int64, device=self.device)
            dst = torch.tensor([t for _, t in moves], dtype=torch.int64, device=self.device)
            # torch reads of the words: bit[old] of every mask
            bits = (self.table[:, src >> 5] >> (src & 31).to(torch.int32)) & 1
            for m in range(self.n_masks):
                on = bits[m] != 0
                if bool(on.any()):
                    self.set(m, dst[on], True)
                if not bool(on.all()):
                    self.set(m, dst[~on], False)
        # clear [n_new, 32 words): whole words by a fill, the split word by the kernel
        w0 = (n_new + 31) // 32
        if w0 < self.words:
            self.table[:, w0:].zero_()
        if n_new % 32:
            tail = torch.arange(n_new, w0 * 32, dtype=torch.int64, device=self.device)
            for m in range(self.n_masks):
                self.set(m, tail, False)

    # ---- readers ------------------------------------------------------------------------------
    def count(self, mask) -> int:
        """Allowed rows of one mask (ebt_allow_count over all the table's rows)."""
        c = torch.empty(1, dtype=torch.int64, device=self.device)
        call("ebt_allow_count", ptr(self._row(mask)), self.words, 32 * self.words, ptr(c),
             stream_of(self.device))
        return int(c.item())

    def to_bool(self, mask, n: Optional[int] = None) -> torch.Tensor:
        """One mask as a bool vector over rows [0, n) (default: all the table's rows)."""
        n = self.n_rows if n is None else int(n)
        r = torch.arange(n, dtype=torch.int64, device=self.device)
        return ((self._row(mask)[r >> 5] >> (r & 31).to(torch.int32)) & 1) != 0

    # ---- materialised sub-catalogs (ebert.h 0.7.0) --------------------------------------------
    def materialize(self, mask) -> int:
        """Copy the allowed rows of one mask into a dense sub-catalog (ebt_allow_rows,
        ebt_catalog_gather_rows) and return their number m. From then on ``score_topk(...,
        allow=(masks, ids))`` with a HOST list of ids scores the queries of this mask over those
        m rows -- same rows, bitwise the same scores. The copy holds m / n of the catalog's
        matrix and image. It is a snapshot: ``set`` / ``from_bool`` / ``apply_moves`` on the mask
        drop it and an edit of the catalog makes it stale (never used again; the mask pass
        answers) until ``materialize`` is called again. m = 0 builds nothing (the mask stays on
        the mask pass). Waits for the stream once (m sizes the buffers)."""
        from .catalog import Catalog
        mi = self.index(mask)
        cat = self.catalog
        if cat is None:
            raise EbertError("materialize needs masks built for a Catalog, not for a row count")
        if cat.row_offset != 0 or cat.n_global != cat.n:
            raise EbertError("materialize on a row-sharded catalog is not supported")
        self._subs.pop(mi, None)
        dev, st = self.device, stream_of(self.device)
        row = self.table[mi]
        n_rows = min(int(cat.n), 32 * self.words)
        cnt = torch.empty(1, dtype=torch.int64, device=dev)
        call("ebt_allow_count", ptr(row), self.words, n_rows, ptr(cnt), st)
        m = int(cnt.item())
        if m == 0:
            return 0
        rows = torch.empty(m, dtype=torch.int64, device=dev)
        rank = torch.empty(self.words, dtype=torch.int32, device=dev)
        need = int(_lib.load().ebt_allow_rows_bytes(self.words))
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        call("ebt_allow_rows", ptr(row), self.words, n_rows, ptr(rows), m, ptr(rank), ptr(cnt),
             ptr(ws), need, st)
        # the copy's row stride: the parent's when its matrix is its own image (one ld_img for
        # the queries prepared on the parent), else d -- moved off 16-byte alignment when the
        # parent's rows are not aligned, so that the rescore takes the same form on both
        # (rescore.hip) and the scores stay bitwise equal
        es = cat.data.element_size()
        alias = int(cat.cstruct.image or 0) == int(cat.cstruct.data or 0)
        if alias:
            ld_out = cat.ld
        else:
            ld_out = cat.d
            parent_vec = cat.data.data_ptr() % 16 == 0 and (cat.ld * es) % 16 == 0
            if (cat.d * es) % 16 == 0 and not parent_vec:
                ld_out = cat.d + 1
        data = torch.empty((m, ld_out), dtype=cat.data.dtype, device=dev)
        if ld_out > cat.d:
            data.zero_()
        gnorm = torch.empty(m, dtype=torch.float64, device=dev)
        inv32 = torch.empty(_round_up(m, 128), dtype=torch.float32, device=dev)
        image = None if alias else torch.empty((m, cat.ld_img), dtype=cat.img_torch_dtype,
                                               device=dev)
        sub = _lib.EbtCatalog()
        call("ebt_catalog_gather_rows", ctypes.byref(cat.cstruct), ptr(rows), m, ptr(data), ld_out,
             ptr(gnorm), ptr(inv32), ptr(image), ctypes.byref(sub), st)
        view = Catalog.from_parts(data[:, :cat.d], gnorm, inv32, data if alias else image,
                                  u_cat=float(sub.u_cat))
        for f, _t in _lib.EbtCatalog._fields_:   # the library's struct and from_parts' agree
            if getattr(view.cstruct, f) != getattr(sub, f):
                raise EbertError(f"internal error: sub-catalog field {f} differs "
                                 f"({getattr(view.cstruct, f)} vs {getattr(sub, f)})")
        self._subs[mi] = SubCatalog(view, rows, rank, m, n_rows, int(cat.edits))
        return m

    def dematerialize(self, mask) -> None:
        """Free the sub-catalog of one mask (no-op when it has none)."""
        self._subs.pop(self.index(mask), None)

    def materialized(self) -> Dict[int, Tuple[int, bool]]:
        """mask index -> (rows of its sub-catalog, fresh): fresh = it matches the catalog's edit
        counter and is used; a stale one is kept until ``materialize`` / ``dematerialize``."""
        return {mi: (v.m, self._fresh(v)) for mi, v in sorted(self._subs.items())}

    def _fresh(self, v: SubCatalog) -> bool:
        return self.catalog is not None and v.edits == int(self.catalog.edits)

    def sub_for(self, catalog, mask: int) -> Optional[SubCatalog]:
        """The fresh sub-catalog of mask index `mask` for queries against `catalog`, or None."""
        v = self._subs.get(mask)
        if v is None or catalog is not self.catalog or not self._fresh(v):
            return None
        return v

    # ---- the C struct -------------------------------------------------------------------------
    def host_ids(self, ids, B: int) -> np.ndarray:
        """int32 [B] of per-query mask ids from a host list (None / -1 / a name / an index,
        range-checked here); -1 = unfiltered."""
        ids = list(ids)
        if len(ids) != B:
            raise EbertError(f"{len(ids)} mask ids for {B} queries")
        host = np.empty(B, dtype=np.int32)
        for b, m in enumerate(ids):
            if m is None or (not isinstance(m, str) and int(m) == -1):
                host[b] = -1
            else:
                host[b] = self.index(m)
        return host

    def mask_ids(self, ids, B: int) -> torch.Tensor:
        """Device int32 [B] of per-query mask ids from a host list (None / -1 / a name / an index,
        range-checked here) or a device int32 tensor (used as it is)."""
        if isinstance(ids, torch.Tensor):
            require_cuda(ids, "mask_ids")
            if ids.dtype != torch.int32 or ids.dim() != 1 or ids.numel() != B:
                raise EbertError(f"mask_ids must be int32 [{B}]")
            return ids.contiguous()
        return torch.from_numpy(self.host_ids(ids, B)).to(self.device)

    def cstruct(self, mask_id: torch.Tensor) -> "_lib.EbtAllow":
        return _lib.EbtAllow(masks=ptr(self.table), words=self.words, n_masks=self.n_masks,
                             mask_id=ptr(mask_id))

    def __repr__(self) -> str:
        return (f"AllowMasks(n_rows={self.n_rows}, n_masks={self.n_masks}, words={self.words}, "
                f"device={self.device})")


def resolve_allow(allow, B: int, device) -> Optional[Tuple["_lib.EbtAllow", tuple]]:
    """score_topk's ``allow=(AllowMasks, mask_ids)`` -> (ebt_allow, tensors to keep alive)."""
    if allow is None:
        return None
    try:
        masks, ids = allow
    except (TypeError, ValueError):
        raise EbertError("allow= takes (AllowMasks, mask_ids)") from None
    if not isinstance(masks, AllowMasks):
        raise EbertError("allow= takes (AllowMasks, mask_ids)")
    a, b = masks.device, torch.device(device)
    if a.type != b.type or (a.index is not None and b.index is not None and a.index != b.index):
        raise EbertError(f"the allow masks live on {masks.device}, the catalog on {device}")
    mid = masks.mask_ids(ids, B)
    return masks.cstruct(mid), (masks.table, mid)
