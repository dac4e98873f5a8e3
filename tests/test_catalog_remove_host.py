"""CPU: removing catalog rows in place (ebert.h 0.5.0) -- the new symbols, ebt_catalog_remove_plan
against a numpy restatement of the rule, the host-side argument checks of ebt_catalog_remove_rows
(they run before any GPU call, so fake device pointers are never dereferenced) and the RecBatcher
barrier with an injected score_fn."""
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


def _rows(r):
    return (ctypes.c_int64 * len(r))(*r)


def _remove(lib, cat, rows, n_cap=1000, ws_bytes=None, null_rows=False, m=None):
    m = len(rows) if m is None else m
    state_bytes = lib.ebt_catalog_state_bytes(FAKE, cat.dtype, n_cap, cat.d, cat.ld)
    if ws_bytes is None:
        ws_bytes = lib.ebt_catalog_remove_bytes(m)
    arr = _rows(rows)
    return lib.ebt_catalog_remove_rows(ctypes.byref(cat), STATE, state_bytes, n_cap,
                                       None if null_rows else ctypes.cast(arr, ctypes.c_void_p),
                                       m, FAKE + (1 << 29), ws_bytes, None)


def _plan(lib, n, row_offset, rows, with_out=True):
    m = len(rows)
    arr = _rows(rows)
    src, dst = (ctypes.c_int64 * max(m, 1))(), (ctypes.c_int64 * max(m, 1))()
    p = lib.ebt_catalog_remove_plan(n, row_offset, ctypes.cast(arr, ctypes.c_void_p), m,
                                    ctypes.cast(src, ctypes.c_void_p) if with_out else None,
                                    ctypes.cast(dst, ctypes.c_void_p) if with_out else None)
    return p, list(src[:max(p, 0)]), list(dst[:max(p, 0)])


def _rule(n, row_offset, rows):
    """The rule, restated: holes = removed rows below n', survivors = kept rows of [n', n)."""
    local = np.asarray(rows, dtype=np.int64) - row_offset
    n_new = n - len(local)
    holes = np.sort(local[local < n_new])
    tail = np.arange(n_new, n)
    surv = tail[~np.isin(tail, local)]
    assert len(holes) == len(surv)
    return [int(s) + row_offset for s in surv], [int(h) + row_offset for h in holes]


def test_symbols_and_version():
    lib = _lib.load()
    for s in ("ebt_catalog_remove_bytes", "ebt_catalog_remove_plan", "ebt_catalog_remove_rows"):
        assert hasattr(lib, s), s
        assert s in _lib._SIGNATURES
    assert lib.ebt_version() >= 500


def test_remove_bytes():
    lib = _lib.load()
    assert lib.ebt_catalog_remove_bytes(0) == 0
    assert lib.ebt_catalog_remove_bytes(-3) == 0
    for m in (1, 16, 17, 4096):
        assert lib.ebt_catalog_remove_bytes(m) == _al(16 * m)     # round_up(16 m, 256)


def _mixed(n, seed=3):
    rng = np.random.default_rng(seed)
    rows = set(int(r) for r in rng.choice(n, 37, replace=False))
    return sorted(rows | {0, n - 1, n - 2})


@pytest.mark.parametrize("n, off, rows", [
    (1000, 0, [0, 3, 17, 500, 899]),                 # head only: the last five rows move
    (1000, 0, list(range(990, 1000))),               # tail only: p = 0
    (1000, 0, [995]),                                # one tail row that is not the last
    (1000, 0, _mixed(1000)),                         # mixed
    (1000, 0, list(range(600))),                     # m > n / 2: every survivor moves
    (1000, 0, list(range(999))),                     # m = n - 1: row 999 becomes row 0
    (1000, 0, list(range(1, 1000))),                 # m = n - 1, p = 0
    (1000, 5000, [r + 5000 for r in _mixed(1000, 4)]),   # row_offset > 0
    (1000, 5000, [5000, 5999]),
], ids=["head", "tail", "tail-inner", "mixed", "most", "all-but-last", "all-but-first",
        "offset-mixed", "offset-ends"])
def test_remove_plan_is_the_rule(n, off, rows):
    lib = _lib.load()
    want_from, want_to = _rule(n, off, rows)
    p, src, dst = _plan(lib, n, off, rows)
    assert p == len(want_from)
    assert src == want_from and dst == want_to
    assert _plan(lib, n, off, rows, with_out=False)[0] == p      # from / to may both be NULL
    # applied to a matrix: the edit of the issue's numpy line
    c = np.arange(n)
    c2 = c.copy()
    c2[np.asarray(dst, dtype=np.int64) - off] = c[np.asarray(src, dtype=np.int64) - off]
    c2 = c2[:n - len(rows)]
    assert sorted(c2) == sorted(set(range(n)) - {r - off for r in rows})


def test_remove_plan_expected_values():
    lib = _lib.load()
    assert _plan(lib, 1000, 0, list(range(990, 1000))) == (0, [], [])
    assert _plan(lib, 1000, 0, [3, 998]) == (1, [999], [3])
    assert _plan(lib, 1000, 0, list(range(999))) == (1, [999], [0])
    p, src, dst = _plan(lib, 1000, 0, list(range(600)))
    assert (p, src, dst) == (400, list(range(600, 1000)), list(range(400)))
    assert _plan(lib, 10, 0, []) == (0, [], [])


@pytest.mark.parametrize("rows, what", [
    ((5, 3, 9), b"ascending"),          # unsorted
    ((3, 5, 5), b"ascending"),          # duplicate
    ((3, 5, 1000), b"not in"),          # past the end
    ((-1, 5), b"not in"),
    (tuple(range(1000)), b"every row"),  # m = n
])
def test_remove_plan_bad_rows(rows, what):
    lib = _lib.load()
    assert _plan(lib, 1000, 0, list(rows))[0] == -1
    msg = lib.ebt_last_error()
    assert b"ebt_catalog_remove_plan" in msg and what in msg, msg


def test_remove_plan_range_follows_row_offset():
    lib = _lib.load()
    assert _plan(lib, 1000, 5000, [10, 20])[0] == -1              # local ids, not global ones
    assert b"not in" in lib.ebt_last_error()
    assert _plan(lib, 1000, 5000, [5010, 6000])[0] == -1          # 6000 = row_offset + n
    assert b"not in" in lib.ebt_last_error()
    assert _plan(lib, 4, 0, [0, 1, 2, 3, 4])[0] == -1             # m > n
    assert lib.ebt_catalog_remove_plan(1000, 0, None, 2, None, None) == -1   # NULL rows


@pytest.mark.parametrize("kw, rows, what", [
    (dict(n_cap=2000), (1, 2), b"n_cap"),                         # another capacity
    (dict(n_cap=999), (1, 2), b"n_cap"),                          # n_cap below n
    (dict(ws_bytes=16), (1, 2), b"workspace"),                    # 32 bytes are not 256
    (dict(ws_bytes=0), (1, 2), b"workspace"),
    (dict(null_rows=True, m=2), (), b"rows is NULL"),
    (dict(), tuple(range(1000)), b"every row"),                   # m = n
    (dict(), (5, 3), b"ascending"),
    (dict(), (3, 3), b"ascending"),
    (dict(), (3, 1000), b"not in"),
    (dict(m=-1), (), b"m ="),
])
def test_remove_rows_bad_arguments(kw, rows, what):
    lib = _lib.load()
    cat = _fake_catalog()
    before = bytes(cat)
    assert _remove(lib, cat, rows, **kw) == EINVAL
    msg = lib.ebt_last_error()
    assert b"ebt_catalog_remove_rows" in msg and what in msg, msg
    assert bytes(cat) == before and cat.n == 1000                 # *cat unchanged


def test_remove_rows_layout_and_empty():
    lib = _lib.load()
    loose = _fake_catalog()                 # a hand-filled struct (the from_parts kind)
    loose.gnorm64 = FAKE + 4096
    before = bytes(loose)
    assert _remove(lib, loose, (1, 2)) == EINVAL
    assert b"laid out" in lib.ebt_last_error()
    assert bytes(loose) == before
    cat = _fake_catalog(row_offset=5000)
    assert _remove(lib, cat, (10, 20)) == EINVAL                  # local ids, not global ones
    assert b"not in" in lib.ebt_last_error()
    # m == 0 passes the checks and does nothing (no GPU call: there is no GPU here)
    before = bytes(cat)
    assert _remove(lib, cat, ()) == 0
    assert bytes(cat) == before
    assert lib.ebt_catalog_remove_rows(None, STATE, 1 << 20, 1000, None, 0, None, 0,
                                       None) == EINVAL


# ---- the batcher's barrier -------------------------------------------------------------------
class _FakeCatalog:
    """Scores are the catalog's version: a request scored before the removal answers 0."""
    def __init__(self, log):
        self.d, self.n, self.row_offset, self.n_global = 4, 100, 0, 100
        self.version = 0
        self.log = log
        self.busy = threading.Lock()       # held by every scoring call and by the edit

    def remove(self, rows):
        assert self.busy.acquire(blocking=False), "the removal overlaps a scoring call"
        try:
            rows = sorted(rows)
            self.log.append(("remove", tuple(rows)))
            n_new = self.n - len(rows)
            holes = [r for r in rows if r < n_new]
            surv = [r for r in range(n_new, self.n) if r not in rows]
            self.n = self.n_global = n_new
            self.version += 1
            return list(zip(surv, holes))
        finally:
            self.busy.release()


def _score(cat, k, liked, exclude):
    assert cat.busy.acquire(blocking=False), "a scoring call overlaps the removal"
    try:
        cat.log.append(("score", len(liked)))
        B = len(liked)
        return (np.full((B, k), float(cat.version)), np.tile(np.arange(k, dtype=np.int64), (B, 1)))
    finally:
        cat.busy.release()


def test_batcher_remove_is_a_barrier():
    log = []
    cat = _FakeCatalog(log)
    b = RecBatcher(cat, max_batch=8, max_wait_ms=2.0, score_fn=_score)
    before = [b.submit([80 + i], [], 3) for i in range(20)]      # rows 80 .. 99: valid until then
    rm = b.remove([2, 97, 5])
    assert rm.result(timeout=30) == [(98, 2), (99, 5)]            # the Future holds the moves
    assert cat.n == 97
    after = [b.submit([i], [], 3) for i in range(20)]
    gone = b.submit([97], [], 3)                                  # validated against the new n
    for f in before:
        assert f.result(timeout=30)[0][0] == 0.0                  # the old catalog
    for f in after:
        assert f.result(timeout=30)[0][0] == 1.0                  # the new one
    assert isinstance(gone.exception(timeout=30), ValueError)
    b.close()
    kinds = [e[0] for e in log]
    u = kinds.index("remove")
    assert kinds.count("remove") == 1 and log[u] == ("remove", (2, 5, 97))
    assert sum(e[1] for e in log[:u]) == 20 and sum(e[1] for e in log[u + 1:]) == 20


def test_batcher_remove_error_fails_only_its_future():
    log = []
    cat = _FakeCatalog(log)
    good = cat.remove

    def bad_remove(rows):
        raise ValueError("no such row")
    b = RecBatcher(cat, max_batch=4, max_wait_ms=1.0, score_fn=_score)
    cat.remove = bad_remove
    head = [b.submit([i], [], 2) for i in range(6)]
    failed = b.remove([7])
    tail = [b.submit([i], [], 2) for i in range(10)]
    assert isinstance(failed.exception(timeout=30), ValueError)
    cat.remove = good
    last = b.remove([99])
    b.close()                                                     # drains requests AND edits
    assert last.result(timeout=30) == []                          # a tail row: nothing moves
    for f in head + tail:
        assert len(f.result(timeout=30)[1]) == 2                  # an edit's error stops nothing
    assert cat.n == 99
    assert isinstance(b.remove([1]).exception(timeout=1), RuntimeError)   # closed
