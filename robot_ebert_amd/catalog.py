"""HBM-resident catalog: the GPU replacement of ``movies_collab_embeddings``.

Reference: ``src/backend/app/constants.py:55-56`` loads every movie vector from Chroma into a
float64 ``DataFrame(index=tmdb_id)`` at import time, and ``lib.py:51`` then re-normalises the
WHOLE catalog on every request (sklearn ``metrics/pairwise.py:1730-1734``). Here the catalog is
uploaded once, its guarded float64 row norms are computed once (``ebt_row_norms``), and the
MFMA screening image is built once:

* float16 / bfloat16 catalogs with d % 64 == 0 are screened NATIVELY: the matrix itself is the
  MFMA operand (no copy) and 1/||c|| is applied in the GEMM epilogue, so screening products are
  exact and only float32 accumulation error remains;
* float32 / float64 catalogs (and 16-bit ones with ragged d) get a float16 image of the
  NORMALISED rows, zero-padded to a multiple of 64 columns (unit round-off 2^-11, all values in
  [-1, 1]).

Either way the exact float64 scores are recomputed from the original matrix for the screened
candidates, so the image precision never reaches the results ("certified
screening").
"""
from __future__ import annotations

import ctypes
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import DTYPE_CODE, EBT_BF16, EBT_F16, EbertError, call, ptr, require_cuda, stream_of  # noqa: F401

IMG_ALIGN = 64


def _round_up(v: int, m: int) -> int:
    return (v + m - 1) // m * m


def _al(v: int) -> int:
    """ebt_catalog_init's state-buffer alignment (256 bytes)."""
    return _round_up(v, 256)


class Catalog:
    """One (shard of a) catalog resident in HBM.

    Parameters
    ----------
    emb : CUDA tensor [n, d] of float32 / float64 / bfloat16 / float16, rows contiguous.
    ids : optional sequence of string ids (the DataFrame index of constants.py:56), one per row.
    row_offset : global row id of local row 0 when the catalog is row-sharded across ranks.
    n_global : total rows over all shards (defaults to n).
    capacity : optional row capacity >= n. The catalog then owns a ``[capacity, d]`` copy of
        ``emb`` and a state laid out for ``capacity`` rows, so that ``append`` can grow it in
        place; every attribute still describes the first n rows. Without it the catalog views
        ``emb`` itself (``update_rows`` then writes into that tensor) and cannot grow.
    """

    def __init__(self, emb: torch.Tensor, ids: Optional[Sequence[str]] = None,
                 row_offset: int = 0, n_global: Optional[int] = None,
                 capacity: Optional[int] = None) -> None:
        require_cuda(emb, "catalog embeddings")
        if emb.dim() != 2 or emb.shape[0] < 1 or emb.shape[1] < 1:
            raise EbertError(f"catalog must be a non-empty 2-D matrix, got {tuple(emb.shape)}")
        if emb.dtype not in DTYPE_CODE:
            raise EbertError(f"unsupported catalog dtype {emb.dtype}")
        if emb.stride(1) != 1:
            emb = emb.contiguous()
        self._store = emb   # the rows' storage: emb itself, or [capacity, d] owned here
        if capacity is not None:
            capacity = int(capacity)
            if capacity < emb.shape[0]:
                raise EbertError(f"capacity {capacity} < {emb.shape[0]} rows")
            self._store = torch.empty((capacity, emb.shape[1]), dtype=emb.dtype,
                                      device=emb.device)
            self._store[:emb.shape[0]].copy_(emb)
            emb = self._store[:emb.shape[0]]
        self.data = emb
        self.device = emb.device
        self.n, self.d = int(emb.shape[0]), int(emb.shape[1])
        self.ld = int(emb.stride(0))
        self.dtype_code = DTYPE_CODE[emb.dtype]
        self.row_offset = int(row_offset)
        self.n_global = int(n_global) if n_global is not None else self.n
        self.d_pad = _round_up(self.d, IMG_ALIGN)
        # the C ABI's catalog (ebt_catalog_init): guarded float64 norms, float32 inverse norms
        # and the screening image in one device state buffer owned here
        lib = _lib.load()
        self.capacity = capacity if capacity is not None else self.n
        need = lib.ebt_catalog_state_bytes(ptr(emb), self.dtype_code, self.capacity, self.d,
                                           self.ld)
        if need == 0:
            raise EbertError(f"bad catalog shape {tuple(emb.shape)} (ld {self.ld})")
        self.state = torch.empty(need, dtype=torch.uint8, device=self.device)
        self.cstruct = _lib.EbtCatalog()
        if capacity is None:
            call("ebt_catalog_init", ctypes.byref(self.cstruct), ptr(emb), self.dtype_code, self.n,
                 self.d, self.ld, self.row_offset, ptr(self.state), need, stream_of(self.device))
        else:
            call("ebt_catalog_init_reserved", ctypes.byref(self.cstruct), ptr(emb),
                 self.dtype_code, self.n, self.capacity, self.d, self.ld, self.row_offset,
                 ptr(self.state), need, stream_of(self.device))
        c = self.cstruct
        self.img_dtype = int(c.img_dtype)
        self.ld_img = int(c.ld_img)
        self.native = bool(c.native)
        self._views()
        self.ids: Optional[List[str]] = list(ids) if ids is not None else None
        if self.ids is not None and len(self.ids) != self.n:
            raise EbertError(f"{len(self.ids)} ids for {self.n} rows")
        self._pos: Optional[Dict[str, int]] = None
        # bumped by every edit (update_rows / append / remove): what was derived from the rows
        # (allow.AllowMasks' materialised sub-catalogs) is used only while it matches
        self.edits = 0

    def _views(self) -> None:
        """The tensors the scoring code reads, over the first n rows of a state laid out for
        ``capacity`` rows (ebt_catalog_init_reserved; capacity == n: ebt_catalog_init)."""
        c = self.cstruct
        self.n = int(c.n)
        self.data = self._store if self.n == self._store.shape[0] else self._store[:self.n]
        off_inv = _al(self.capacity * 8)
        off_img = off_inv + _al(_round_up(self.capacity, 128) * 4)
        n128 = _round_up(self.n, 128)
        self.gnorm = self.state[:self.n * 8].view(torch.float64)
        self.inv32 = self.state[off_inv:off_inv + n128 * 4].view(torch.float32)
        self.u_cat = float(c.u_cat)
        self.cscale = self.inv32 if self.native else None
        if c.image == self._store.data_ptr():
            self.image = self.data  # the matrix itself is the MFMA operand
        else:
            self.image = self.state[off_img:off_img + self.n * self.ld_img * 2].view(
                self.img_torch_dtype).view(self.n, self.ld_img)

    # ---- live updates (ebt_catalog_update_rows / _append_rows / _remove_rows) --------------
    def _vectors(self, vectors, m: Optional[int]) -> torch.Tensor:
        """The update's source rows as a device tensor [m, d] of a supported dtype, checked."""
        if self.state is None:
            raise EbertError("a from_parts catalog cannot be updated: its norms and image are "
                             "the caller's tensors, not a state this library laid out")
        if isinstance(vectors, np.ndarray):
            vectors = torch.from_numpy(np.ascontiguousarray(vectors))
        if not isinstance(vectors, torch.Tensor) or vectors.dim() != 2:
            raise EbertError("vectors must be a 2-D tensor or numpy array [m, d]")
        if vectors.dtype not in DTYPE_CODE:
            raise EbertError(f"unsupported vector dtype {vectors.dtype}")
        if int(vectors.shape[1]) != self.d:
            raise EbertError(f"vectors have d = {int(vectors.shape[1])}, the catalog {self.d}")
        if m is not None and int(vectors.shape[0]) != m:
            raise EbertError(f"{int(vectors.shape[0])} vectors for {m} rows")
        return vectors

    def update_rows(self, rows_or_ids, vectors) -> None:
        """Replace rows in place: ``rows_or_ids`` are GLOBAL rows or string ids, ``vectors`` a
        tensor or numpy array [m, d] of any supported dtype (converted as ``.to(dtype)``). One
        kernel rewrites the rows, their norms and image rows; the state afterwards equals that
        of a catalog built from the edited matrix, except that ``u_cat`` never decreases.
        Stream-ordered on the current stream; every batch submitted before it must have been
        finished (include/ebert.h, "Ordering"). Bad arguments raise EbertError before any GPU
        work and leave the catalog unchanged."""
        items = list(rows_or_ids)
        vectors = self._vectors(vectors, len(items))
        if any(isinstance(t, str) for t in items):
            try:
                rows = self.rows_of(items)
            except KeyError as e:
                raise EbertError(f"unknown id {e}") from e
        else:
            try:
                rows = [int(r) for r in items]
            except (TypeError, ValueError) as e:
                raise EbertError(f"malformed rows: {e}") from e
        lo, hi = self.row_offset, self.row_offset + self.n
        for r in rows:
            if r < lo or r >= hi:
                raise EbertError(f"row {r} is not in the catalog rows [{lo}, {hi})")
        if len(set(rows)) != len(rows):
            raise EbertError("duplicate rows in one update")
        m = len(rows)
        if m == 0:
            return
        order = sorted(range(m), key=rows.__getitem__)
        vectors = vectors.to(self.device)
        if order != list(range(m)):   # the library takes ascending rows: permute the vectors alike
            vectors = vectors[torch.tensor(order, dtype=torch.int64, device=self.device)]
        elif vectors.stride(1) != 1:
            vectors = vectors.contiguous()
        host_rows = np.asarray([rows[i] for i in order], dtype=np.int64)
        lib = _lib.load()
        ws = torch.empty(lib.ebt_catalog_update_bytes(m), dtype=torch.uint8, device=self.device)
        call("ebt_catalog_update_rows", ctypes.byref(self.cstruct), ptr(self.state),
             self.state.numel(), self.capacity, host_rows.ctypes.data, m, ptr(vectors),
             DTYPE_CODE[vectors.dtype], int(vectors.stride(0)), ptr(ws), ws.numel(),
             stream_of(self.device))
        self.u_cat = float(self.cstruct.u_cat)
        self.edits += 1

    def append(self, vectors, ids: Optional[Sequence[str]] = None) -> None:
        """Append rows in place, up to ``capacity``: n, n_global, the C struct, the ids and the
        id -> row map grow together. ``ids`` is required iff the catalog has ids. Refused on a
        row-sharded catalog. Ordering as for ``update_rows``."""
        vectors = self._vectors(vectors, None)
        if self.row_offset != 0 or self.n_global != self.n:
            raise EbertError("append on a row-sharded catalog is not supported")
        m = int(vectors.shape[0])
        if (ids is not None) != (self.ids is not None):
            raise EbertError("append needs ids exactly when the catalog has ids")
        if ids is not None:
            ids = list(ids)
            if len(ids) != m:
                raise EbertError(f"{len(ids)} ids for {m} rows")
            pos = self.index_pos
            if len(set(ids)) != m or any(t in pos for t in ids):
                raise EbertError("append: an id is already in the catalog (or given twice)")
        if self.n + m > self.capacity:
            raise EbertError(f"append of {m} rows to {self.n} exceeds the capacity "
                             f"{self.capacity} (construct the Catalog with capacity=)")
        if m == 0:
            return
        vectors = vectors.to(self.device)
        if vectors.stride(1) != 1:
            vectors = vectors.contiguous()
        first = self.n
        call("ebt_catalog_append_rows", ctypes.byref(self.cstruct), ptr(self.state),
             self.state.numel(), self.capacity, m, ptr(vectors), DTYPE_CODE[vectors.dtype],
             int(vectors.stride(0)), stream_of(self.device))
        self.edits += 1
        self._views()
        self.n_global = self.n
        if ids is not None:
            self.ids.extend(ids)
            for i, t in enumerate(ids):
                self._pos[t] = first + i

    def remove(self, rows_or_ids) -> List[Tuple[int, int]]:
        """Remove rows in place: ``rows_or_ids`` are GLOBAL rows or string ids, in any order.
        With n' = n - m, the removed rows below n' are filled, in ascending order, with the rows
        of [n', n) that are not removed, in ascending order (include/ebert.h, "removal"); every
        other row keeps its number. Returns those moves as ``(old_row, new_row)`` pairs, for a
        caller that holds row numbers to remap them. One kernel copies the moved rows with their
        norms and image rows; the state afterwards equals that of a catalog built from the edited
        matrix (``u_cat`` is kept). n, n_global, the ids and the id -> row map follow, and the
        freed rows are available to ``append``. Refused on a row-sharded catalog. Ordering as
        for ``update_rows``. Bad arguments raise EbertError before any GPU work and leave the
        catalog unchanged."""
        if self.state is None:
            raise EbertError("a from_parts catalog cannot be edited: its norms and image are "
                             "the caller's tensors, not a state this library laid out")
        if self.row_offset != 0 or self.n_global != self.n:
            raise EbertError("remove on a row-sharded catalog is not supported")
        items = list(rows_or_ids)
        if any(isinstance(t, str) for t in items):
            try:
                rows = self.rows_of(items)
            except KeyError as e:
                raise EbertError(f"unknown id {e}") from e
        else:
            try:
                rows = [int(r) for r in items]
            except (TypeError, ValueError) as e:
                raise EbertError(f"malformed rows: {e}") from e
        for r in rows:
            if r < 0 or r >= self.n:
                raise EbertError(f"row {r} is not in the catalog rows [0, {self.n})")
        if len(set(rows)) != len(rows):
            raise EbertError("duplicate rows in one removal")
        m = len(rows)
        if m >= self.n:
            raise EbertError(f"cannot remove every row ({m} of {self.n})")
        if m == 0:
            return []
        host_rows = np.asarray(sorted(rows), dtype=np.int64)
        src, dst = np.empty(m, dtype=np.int64), np.empty(m, dtype=np.int64)
        lib = _lib.load()
        p = lib.ebt_catalog_remove_plan(self.n, 0, host_rows.ctypes.data, m, src.ctypes.data,
                                        dst.ctypes.data)
        if p < 0:
            raise EbertError("ebt_catalog_remove_plan failed: " +
                             lib.ebt_last_error().decode(errors="replace"))
        moves = [(int(s), int(t)) for s, t in zip(src[:p], dst[:p])]
        ws = torch.empty(lib.ebt_catalog_remove_bytes(m), dtype=torch.uint8, device=self.device)
        call("ebt_catalog_remove_rows", ctypes.byref(self.cstruct), ptr(self.state),
             self.state.numel(), self.capacity, host_rows.ctypes.data, m, ptr(ws), ws.numel(),
             stream_of(self.device))
        self.edits += 1
        self._views()
        self.n_global = self.n
        if self.ids is not None:
            pos = self.index_pos
            for r in rows:
                del pos[self.ids[r]]
            for s, t in moves:
                self.ids[t] = self.ids[s]
                pos[self.ids[t]] = t
            del self.ids[self.n:]
        return moves

    # ---- constructors ---------------------------------------------------------------------
    @classmethod
    def from_matrix(cls, ids: Optional[Sequence[str]], emb, device="cuda", shard: bool = False,
                    **kw) -> "Catalog":
        """SURVEY §8b's ``Catalog.from_matrix(ids, emb, shard)``: upload a host or device matrix.
        With ``shard=True`` (an initialised torch.distributed group) this rank keeps only its
        row range ``shard_range(n, rank, world)`` (ids sliced alike); rows stay GLOBAL ids."""
        if isinstance(emb, np.ndarray):
            emb = torch.from_numpy(np.ascontiguousarray(emb))
        if shard:
            import torch.distributed as dist
            from .distributed import shard_range
            if not (dist.is_available() and dist.is_initialized()):
                raise EbertError("shard=True needs an initialised torch.distributed process group")
            n = int(emb.shape[0])
            a, b = shard_range(n, dist.get_rank(), dist.get_world_size())
            emb = emb[a:b]
            ids = list(ids)[a:b] if ids is not None else None
            kw = dict(kw, row_offset=a, n_global=n)
        return cls(emb.to(device), ids=ids, **kw)

    @classmethod
    def from_parts(cls, emb: torch.Tensor, gnorm: torch.Tensor, inv32: torch.Tensor,
                   image: torch.Tensor, row_offset: int = 0,
                   n_global: Optional[int] = None, u_cat: Optional[float] = None) -> "Catalog":
        """A catalog view over tensors already built by ``row_norms`` / ``screen_image`` (the
        torch ops of ``ops.py``): nothing is recomputed. ``image`` is the f16 normalised image,
        or the matrix itself for a native f16/bf16 catalog with d % 64 == 0. ``u_cat``: a bound
        on the image rows' error known to the caller (a sub-catalog carries its parent's measured
        value); default 0 for a 16-bit catalog, else the unit round-off 2^-11."""
        for t, what in ((emb, "catalog"), (gnorm, "gnorm"), (inv32, "inv"), (image, "image")):
            require_cuda(t, what)
        self = cls.__new__(cls)
        self.data = emb if emb.stride(1) == 1 else emb.contiguous()
        self.device = emb.device
        self.n, self.d = int(emb.shape[0]), int(emb.shape[1])
        self.ld = int(self.data.stride(0))
        self.dtype_code = DTYPE_CODE[emb.dtype]
        self.row_offset = int(row_offset)
        self.n_global = int(n_global) if n_global is not None else self.n
        self.d_pad = _round_up(self.d, IMG_ALIGN)
        if gnorm.dtype != torch.float64 or gnorm.numel() < self.n:
            raise EbertError("gnorm must be float64 [n]")
        if inv32.dtype != torch.float32 or inv32.numel() < _round_up(self.n, 128):
            raise EbertError("inv must be float32 [round_up(n, 128)]")
        self.gnorm, self.inv32 = gnorm, inv32
        native_16 = emb.dtype in (torch.float16, torch.bfloat16)
        if image.dtype not in (torch.float16, torch.bfloat16) or image.shape[0] != self.n or \
                image.stride(1) != 1 or image.stride(0) % IMG_ALIGN or image.shape[1] < self.d_pad:
            raise EbertError("image must be a 16-bit [n, >= round_up(d, 64)] matrix, "
                             "row stride a multiple of 64")
        self.image, self.ld_img = image, int(image.stride(0))
        self.img_dtype = EBT_F16 if image.dtype == torch.float16 else EBT_BF16
        self.native = native_16  # the image holds the raw rows, scaled by inv in the epilogue
        self.u_cat = float(u_cat) if u_cat is not None else (0.0 if native_16 else 2.0 ** -11)
        self.cscale = self.inv32 if native_16 else None
        self.ids, self._pos = None, None
        self.state = None   # no state of the library's layout: update_rows / append refuse
        self._store, self.capacity = self.data, self.n
        self.edits = 0
        self.cstruct = _lib.EbtCatalog(
            data=ptr(self.data), dtype=self.dtype_code, d=self.d, n=self.n, ld=self.ld,
            row_offset=self.row_offset, gnorm64=ptr(gnorm), inv32=ptr(inv32), image=ptr(image),
            cscale=ptr(self.cscale), img_dtype=self.img_dtype, ld_img=self.ld_img,
            d_pad=self.d_pad, native=1 if native_16 else 0, u_cat=self.u_cat)
        return self

    # ---- id helpers (the DataFrame index of constants.py:56) -----------------------------

    @property
    def index_pos(self) -> Dict[str, int]:
        if self.ids is None:
            raise EbertError("this catalog has no ids")
        if self._pos is None:
            self._pos = {t: i for i, t in enumerate(self.ids)}
        return self._pos

    def contains(self, tmdb_ids: Iterable[str]) -> List[bool]:
        pos = self.index_pos
        return [t in pos for t in tmdb_ids]

    def rows_of(self, tmdb_ids: Iterable[str]) -> List[int]:
        """Global row ids of the given string ids (KeyError for an unknown id)."""
        pos = self.index_pos
        return [pos[t] + self.row_offset for t in tmdb_ids]

    def id_of(self, global_row: int) -> str:
        return self.ids[global_row - self.row_offset]

    @property
    def img_torch_dtype(self) -> torch.dtype:
        return torch.float16 if self.img_dtype == EBT_F16 else torch.bfloat16

    def __repr__(self) -> str:
        return (f"Catalog(n={self.n}, d={self.d}, dtype={self.data.dtype}, row_offset="
                f"{self.row_offset}, image={'native' if self.native else 'f16-normalised'})")


def require_whole_catalog(catalog: Catalog, what: str) -> None:
    """EbertError for a shard of a row-sharded catalog; `what` says what needs one device."""
    if catalog.n_global != catalog.n:
        raise EbertError(f"{what}: this catalog is a shard ({catalog.n} of {catalog.n_global} "
                         "rows)")
