"""CPU: live catalog updates (ebert.h 0.4.0) -- the new symbols, the host-side argument checks of
ebt_catalog_update_rows / ebt_catalog_append_rows (they run before any GPU call, so fake device
pointers are never dereferenced), the RecBatcher update barrier with an injected score_fn, and
distributed.split_update."""
import ctypes
import threading

import numpy as np
import pytest

from robot_ebert_amd import _lib
from robot_ebert_amd.batcher import RecBatcher

EINVAL = -1
FAKE = 1 << 30          # "device" addresses, 256-byte aligned, never dereferenced
STATE = 1 << 32


def _al(v):
    return (v + 255) // 256 * 256


def _fake_catalog(n=1000, n_cap=1000, d=70, dtype=_lib.EBT_F32, row_offset=0):
    """An ebt_catalog whose pointers follow ebt_catalog_init_reserved's layout for n_cap rows
    (non-native: a separate f16 image)."""
    d_pad = (d + 63) // 64 * 64
    inv = STATE + _al(n_cap * 8)
    img = inv + _al((n_cap + 127) // 128 * 128 * 4)
    return _lib.EbtCatalog(data=FAKE, dtype=dtype, d=d, n=n, ld=d, row_offset=row_offset,
                           gnorm64=STATE, inv32=inv, image=img, cscale=None,
                           img_dtype=_lib.EBT_F16, ld_img=d_pad, d_pad=d_pad, native=0,
                           u_cat=2.0 ** -11)


def _rows(*r):
    return (ctypes.c_int64 * len(r))(*r)


def _update(lib, cat, rows, n_cap=1000, src_dtype=_lib.EBT_F32, ws_bytes=None, ld_src=70):
    m = len(rows)
    state_bytes = lib.ebt_catalog_state_bytes(FAKE, cat.dtype, n_cap, cat.d, cat.ld)
    if ws_bytes is None:
        ws_bytes = lib.ebt_catalog_update_bytes(m)
    return lib.ebt_catalog_update_rows(ctypes.byref(cat), STATE, state_bytes, n_cap,
                                       ctypes.cast(rows, ctypes.c_void_p), m, FAKE + (1 << 28),
                                       src_dtype, ld_src, FAKE + (1 << 29), ws_bytes, None)


def test_symbols_and_version():
    lib = _lib.load()
    for s in ("ebt_catalog_init_reserved", "ebt_catalog_update_bytes", "ebt_catalog_update_rows",
              "ebt_catalog_append_rows"):
        assert hasattr(lib, s), s
        assert s in _lib._SIGNATURES
    assert lib.ebt_version() >= 400


def test_update_bytes():
    lib = _lib.load()
    assert lib.ebt_catalog_update_bytes(0) == 0
    assert lib.ebt_catalog_update_bytes(-3) == 0
    for m in (1, 32, 33, 4096, 100_000):
        assert lib.ebt_catalog_update_bytes(m) == _al(8 * m)      # round_up(8 m, 256)


@pytest.mark.parametrize("rows, what", [
    ((5, 3, 9), b"ascending"),          # unsorted
    ((3, 5, 5), b"ascending"),          # duplicate
    ((3, 5, 1000), b"not in"),          # past the end
    ((-1, 5), b"not in"),
])
def test_update_rows_bad_rows(rows, what):
    lib = _lib.load()
    cat = _fake_catalog()
    before = bytes(cat)
    assert _update(lib, cat, _rows(*rows)) == EINVAL
    msg = lib.ebt_last_error()
    assert b"ebt_catalog_update_rows" in msg and what in msg, msg
    assert bytes(cat) == before                                   # *cat unchanged


def test_update_rows_range_follows_row_offset():
    lib = _lib.load()
    cat = _fake_catalog(row_offset=5000)
    assert _update(lib, cat, _rows(10, 20)) == EINVAL             # local ids, not global ones
    assert b"not in" in lib.ebt_last_error()
    assert _update(lib, cat, _rows(5010, 6000)) == EINVAL         # 6000 = row_offset + n
    assert b"not in" in lib.ebt_last_error()


def test_update_rows_bad_layout_dtype_workspace():
    lib = _lib.load()
    cat = _fake_catalog()
    # a capacity other than the one the state was laid out for
    assert _update(lib, cat, _rows(1, 2), n_cap=2000) == EINVAL
    assert b"n_cap" in lib.ebt_last_error()
    # n_cap below n
    assert _update(lib, cat, _rows(1, 2), n_cap=999) == EINVAL
    assert b"n_cap" in lib.ebt_last_error()
    # a hand-filled struct (the from_parts kind: pointers anywhere)
    loose = _fake_catalog()
    loose.gnorm64 = FAKE + 4096
    assert _update(lib, loose, _rows(1, 2)) == EINVAL
    assert b"laid out" in lib.ebt_last_error()
    # source dtype, source stride
    for bad in (-1, 4, 17):
        assert _update(lib, cat, _rows(1, 2), src_dtype=bad) == EINVAL
        assert b"src_dtype" in lib.ebt_last_error()
    assert _update(lib, cat, _rows(1, 2), ld_src=69) == EINVAL
    # workspace too small
    assert _update(lib, cat, _rows(1, 2), ws_bytes=8) == EINVAL
    assert b"workspace" in lib.ebt_last_error()
    # m == 0 passes the checks and does nothing (no GPU call: there is no GPU here)
    assert _update(lib, cat, _rows()) == 0
    assert lib.ebt_catalog_update_rows(None, STATE, 1 << 20, 1000, None, 0, None, 0, 70, None, 0,
                                       None) == EINVAL


def test_append_rows_checks():
    lib = _lib.load()
    cat = _fake_catalog(n=1000, n_cap=1400)
    state_bytes = lib.ebt_catalog_state_bytes(FAKE, cat.dtype, 1400, cat.d, cat.ld)
    before = bytes(cat)

    def append(m, n_cap=1400, src_dtype=_lib.EBT_F64):
        return lib.ebt_catalog_append_rows(ctypes.byref(cat), STATE, state_bytes, n_cap, m,
                                           FAKE + (1 << 28), src_dtype, 70, None)
    assert append(401) == EINVAL                                  # n + m > n_cap
    assert b"n_cap" in lib.ebt_last_error()
    assert append(10, n_cap=1500) == EINVAL                       # the state is too small for it
    assert b"n_cap" in lib.ebt_last_error()
    assert append(10, n_cap=1200) == EINVAL                       # mismatched capacity
    assert b"laid out" in lib.ebt_last_error()
    assert append(10, src_dtype=9) == EINVAL
    assert append(-1) == EINVAL
    assert append(0) == 0
    assert bytes(cat) == before and cat.n == 1000


# ---- the batcher's barrier -------------------------------------------------------------------
class _FakeCatalog:
    """Scores are the catalog's version: a request scored before the update answers 0."""
    def __init__(self, log):
        self.d, self.n, self.row_offset, self.n_global = 4, 100, 0, 100
        self.version = 0
        self.log = log
        self.busy = threading.Lock()       # held by every scoring call and by the update

    def update_rows(self, rows, vectors):
        assert self.busy.acquire(blocking=False), "the update overlaps a scoring call"
        try:
            self.log.append(("update", tuple(rows)))
            self.version += 1
        finally:
            self.busy.release()

    def append(self, vectors, ids=None):
        self.log.append(("append", len(vectors)))
        self.n += len(vectors)
        self.n_global = self.n


def _score(cat, k, liked, exclude):
    assert cat.busy.acquire(blocking=False), "a scoring call overlaps the update"
    try:
        cat.log.append(("score", len(liked)))
        B = len(liked)
        return (np.full((B, k), float(cat.version)), np.tile(np.arange(k, dtype=np.int64), (B, 1)))
    finally:
        cat.busy.release()


def test_batcher_update_is_a_barrier():
    log = []
    cat = _FakeCatalog(log)
    b = RecBatcher(cat, max_batch=8, max_wait_ms=2.0, score_fn=_score)
    before = [b.submit([i], [], 3) for i in range(20)]
    up = b.update_rows([1, 2], np.zeros((2, 4)))
    assert up.result(timeout=30) is None
    after = [b.submit([i], [], 3) for i in range(20)]
    for f in before:
        assert f.result(timeout=30)[0][0] == 0.0                  # the old catalog
    for f in after:
        assert f.result(timeout=30)[0][0] == 1.0                  # the new one
    b.close()
    kinds = [e[0] for e in log]
    u = kinds.index("update")
    assert kinds.count("update") == 1 and log[u] == ("update", (1, 2))
    assert sum(e[1] for e in log[:u]) == 20 and sum(e[1] for e in log[u + 1:]) == 20


def test_batcher_update_error_and_append_and_close_drains():
    log = []
    cat = _FakeCatalog(log)

    def bad_update(rows, vectors):
        raise ValueError("no such row")
    b = RecBatcher(cat, max_batch=4, max_wait_ms=1.0, score_fn=_score)
    assert isinstance(b.submit([100], [], 3).exception(timeout=5), ValueError)   # past n
    assert b.append(np.zeros((5, 4))).result(timeout=30) is None
    assert cat.n == 105
    ok = b.submit([100], [], 3)                                   # validated against the new n
    cat.update_rows = bad_update
    failed = b.update_rows([7], np.zeros((1, 4)))
    tail = [b.submit([i], [], 2) for i in range(10)]
    last = b.update_rows([8], np.zeros((1, 4)))
    b.close()                                                     # drains requests AND edits
    assert len(ok.result(timeout=30)[1]) == 3
    assert isinstance(failed.exception(timeout=30), ValueError)
    assert isinstance(last.exception(timeout=30), ValueError)
    for f in tail:
        assert len(f.result(timeout=30)[1]) == 2                  # an edit's error stops nothing
    assert isinstance(b.update_rows([1], np.zeros((1, 4))).exception(timeout=1), RuntimeError)
    assert isinstance(b.append(np.zeros((1, 4))).exception(timeout=1), RuntimeError)


# ---- distributed.split_update ----------------------------------------------------------------
class _Shard:
    def __init__(self, a, b):
        self.row_offset, self.n = a, b - a


@pytest.mark.parametrize("n, world", [(1000, 2), (1000, 3), (7, 8), (2269, 8)])
def test_split_update_tiles_the_update(n, world):
    from robot_ebert_amd.distributed import shard_range, split_update
    rng = np.random.default_rng(n + world)
    m = min(n, 40)
    rows = [int(r) for r in rng.choice(n, m, replace=False)]      # unsorted on purpose
    vec = rng.standard_normal((m, 6))
    got_rows, got_vec = [], []
    for r in range(world):
        a, b = shard_range(n, r, world)
        sr, sv = split_update(rows, vec, _Shard(a, b))
        assert all(a <= x < b for x in sr) and len(sr) == len(sv)
        got_rows += sr
        got_vec += list(sv)
    assert sorted(got_rows) == sorted(rows) and len(got_rows) == m    # nothing lost or doubled
    by_row = dict(zip(rows, vec))
    for x, v in zip(got_rows, got_vec):
        np.testing.assert_array_equal(v, by_row[x])
    import torch
    sr, sv = split_update(rows, torch.from_numpy(vec), _Shard(0, n))
    assert sr == rows and torch.equal(sv, torch.from_numpy(vec))
