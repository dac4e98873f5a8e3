"""CPU: per-query allow masks (ebert.h 0.6.0) -- the new symbols, ebt_allow_words, the host-side
argument checks of every new entry (they run before any GPU call, so fake device pointers are
never dereferenced) and the RecBatcher's handling of filtered requests with an injected
score_fn."""
import ctypes

import numpy as np
import pytest

import robot_ebert_amd
from oracle import restatement as R
from robot_ebert_amd import _lib
from robot_ebert_amd.batcher import RecBatcher

EINVAL, ENOMEM, EUNSUPPORTED = -1, -3, -4
FAKE = 1 << 30          # "device" addresses, 256-byte aligned, never dereferenced
STATE = 1 << 32
NEW = ("ebt_allow_words", "ebt_allow_from_bool", "ebt_allow_set_rows", "ebt_mask_allowed",
       "ebt_cosine_topk_prepared_allowed", "ebt_cosine_topk_allowed",
       "ebt_cosine_topk_allowed_submit", "ebt_cosine_topk_allowed_finish")


def _al(v):
    return (v + 255) // 256 * 256


def _fake_catalog(n=1000, d=70, row_offset=0):
    d_pad = (d + 63) // 64 * 64
    inv = STATE + _al(n * 8)
    img = inv + _al((n + 127) // 128 * 128 * 4)
    return _lib.EbtCatalog(data=FAKE, dtype=_lib.EBT_F32, d=d, n=n, ld=d, row_offset=row_offset,
                           gnorm64=STATE, inv32=inv, image=img, cscale=None,
                           img_dtype=_lib.EBT_F16, ld_img=d_pad, d_pad=d_pad, native=0,
                           u_cat=2.0 ** -11)


def _allow(masks=FAKE, words=32, n_masks=2, mask_id=FAKE + 4096):
    return _lib.EbtAllow(masks=masks, words=words, n_masks=n_masks, mask_id=mask_id)


def _err(lib):
    return lib.ebt_last_error().decode()


# every way an ebt_allow can be wrong for rows [0, 1000): (struct, a word of the message)
BAD_ALLOW = [
    (dict(masks=None), "null"),
    (dict(mask_id=None), "null"),
    (dict(words=0), "words"),
    (dict(words=-4), "words"),
    (dict(words=30), "words"),          # not a multiple of 4
    (dict(n_masks=0), "n_masks"),
    (dict(n_masks=-1), "n_masks"),
    (dict(words=28), "words"),          # 896 rows < 1000
]
BAD_IDS = ["null-masks", "null-ids", "words-0", "words-neg", "words-odd", "n-masks-0",
           "n-masks-neg", "words-short"]


def test_symbols_and_version():
    lib = _lib.load()
    for s in NEW:
        assert hasattr(lib, s), s
        assert s in _lib._SIGNATURES, s
    assert lib.ebt_version() >= 600
    assert hasattr(robot_ebert_amd, "AllowMasks")
    assert hasattr(_lib, "EbtAllow")


def test_allow_words_values():
    lib = _lib.load()
    for n, w in ((1, 4), (32, 4), (128, 4), (129, 8), (1_000_000, 31252)):
        assert lib.ebt_allow_words(n) == w, n
    for n in (1, 31, 33, 127, 129, 4097, 999_999):
        w = lib.ebt_allow_words(n)
        assert w % 4 == 0 and 32 * w >= n and 32 * (w - 4) < n
    assert lib.ebt_allow_words(0) == 0 and lib.ebt_allow_words(-5) == 0


@pytest.mark.parametrize("kw, word", BAD_ALLOW, ids=BAD_IDS)
def test_mask_allowed_rejects_bad_allow(kw, word):
    lib = _lib.load()
    a = _allow(**kw)
    rc = lib.ebt_mask_allowed(FAKE + (1 << 20), 1000, 4, 0, 1000, ctypes.byref(a), None)
    assert rc == EINVAL and word in _err(lib).lower(), _err(lib)


def test_mask_allowed_rejects_bad_scores():
    lib = _lib.load()
    a = _allow()
    S = FAKE + (1 << 20)
    for args in ((None, 1000, 4, 0, 1000),      # NULL scores
                 (S, 1000, 4, 0, 1000, None),   # NULL allow
                 (S, 1000, -1, 0, 1000),        # B < 0
                 (S, 1000, 4, 10, 5),           # col_end < col_begin
                 (S, 1000, 4, -4, 100),         # col_begin < 0
                 (S, 96, 4, 0, 100),            # ld < columns
                 (S, 1002, 4, 0, 1000),         # ld % 4
                 (S + 4, 1000, 4, 0, 1000),     # scores not 16-byte aligned
                 (S, 1000, 4, 1000, 1100)):     # 32 words = 1024 < col_end
        al = ctypes.byref(a) if len(args) == 5 else None
        assert lib.ebt_mask_allowed(*args[:5], al, None) == EINVAL, args
        assert _err(lib)


def test_builders_reject_bad_arguments():
    lib = _lib.load()
    row, src = FAKE, FAKE + (1 << 20)
    for args in ((None, 10, row, 4), (src, 10, None, 4), (src, -1, row, 4), (src, 10, row, 0),
                 (src, 10, row, 6), (src, 200, row, 4), (src, 10, row + 4, 4)):
        assert lib.ebt_allow_from_bool(*args, None) == EINVAL, args
        assert _err(lib)
    for args in ((None, 4, src, 3, 1), (row, 4, None, 3, 1), (row, 0, src, 3, 1),
                 (row, 4, src, -1, 0)):
        assert lib.ebt_allow_set_rows(*args, None) == EINVAL, args
        assert _err(lib)


def _prepared(lib, allow, B=5, n=1000, d=70, k=10, kprime=32, chunk=1024, flags=0,
              ws_bytes=None, row_offset=0):
    cat = _fake_catalog(n, d, row_offset)
    B_pad = 128
    if ws_bytes is None:
        ws_bytes = lib.ebt_cosine_topk_workspace(B, B_pad, n, kprime, chunk,
                                                 flags | _lib.EBT_FLAG_NO_FUSE)
    P = FAKE + (1 << 24)
    return lib.ebt_cosine_topk_prepared_allowed(
        P, P + 4096, P + 8192, P + 12288, B, B_pad, cat.data, cat.dtype, cat.ld, cat.gnorm64,
        cat.image, None, cat.img_dtype, cat.ld_img, n, d, cat.d_pad, row_offset, None, None, k,
        kprime, chunk, flags, FAKE + (1 << 26), ws_bytes, P + (1 << 20), P + (2 << 20),
        P + (3 << 20), None, None, ctypes.byref(allow) if allow is not None else None)


@pytest.mark.parametrize("kw, word", BAD_ALLOW, ids=BAD_IDS)
def test_prepared_allowed_rejects_bad_allow(kw, word):
    lib = _lib.load()
    assert _prepared(lib, _allow(**kw)) == EINVAL
    assert word in _err(lib).lower(), _err(lib)


def test_prepared_allowed_words_follow_row_offset_and_workspace():
    lib = _lib.load()
    # 32 words cover rows [0, 1024): enough for a shard at row_offset 0, not at row_offset 37
    assert _prepared(lib, _allow(words=32), row_offset=37) == EINVAL
    assert "words" in _err(lib)
    # the unfused workspace is what the caller sizes: one byte less is EBT_ENOMEM
    need = lib.ebt_cosine_topk_workspace(5, 128, 1000, 32, 1024, _lib.EBT_FLAG_NO_FUSE)
    assert _prepared(lib, _allow(), ws_bytes=need - 1) == ENOMEM


def _submit(lib, allow, cat=None, B=5, k=10, ws_bytes=None, sync=False):
    cat = cat if cat is not None else _fake_catalog()
    opt = _lib.EbtOptions(kprime=0, flags=_lib.EBT_FLAG_NO_FUSE, chunk_rows=0)
    if ws_bytes is None:
        ws_bytes = lib.ebt_workspace_bytes(ctypes.byref(cat), B, k, ctypes.byref(opt))
    P = FAKE + (1 << 24)
    cert = (ctypes.c_int32 * (B + 1))()
    pend = _lib.EbtPending()
    al = ctypes.byref(allow) if allow is not None else None
    if sync:
        return lib.ebt_cosine_topk_allowed(ctypes.byref(cat), P, _lib.EBT_F32, B, cat.d, None,
                                           None, k, None, None, ctypes.byref(opt),
                                           FAKE + (1 << 26), ws_bytes, P + (1 << 20),
                                           P + (2 << 20), None, None, al)
    return lib.ebt_cosine_topk_allowed_submit(
        ctypes.byref(cat), P, _lib.EBT_F32, B, cat.d, None, None, k, None, None,
        ctypes.byref(opt), FAKE + (1 << 26), ws_bytes, P + (1 << 20), P + (2 << 20),
        ctypes.cast(cert, ctypes.c_void_p), ctypes.byref(pend), None, None, al)


@pytest.mark.parametrize("sync", [False, True], ids=["submit", "one-call"])
@pytest.mark.parametrize("kw, word", BAD_ALLOW, ids=BAD_IDS)
def test_topk_allowed_rejects_bad_allow(kw, word, sync):
    lib = _lib.load()
    assert _submit(lib, _allow(**kw), sync=sync) == EINVAL
    assert word in _err(lib).lower(), _err(lib)


def test_topk_allowed_workspace_and_large_k():
    lib = _lib.load()
    cat = _fake_catalog()
    opt = _lib.EbtOptions(kprime=0, flags=_lib.EBT_FLAG_NO_FUSE, chunk_rows=0)
    need = lib.ebt_workspace_bytes(ctypes.byref(cat), 5, 10, ctypes.byref(opt))
    assert _submit(lib, _allow(), ws_bytes=need - 1) == ENOMEM
    # min(k, n) > 4096 is the full-sort path: no masks there
    big = _fake_catalog(n=10000)
    assert _submit(lib, _allow(words=316), cat=big, k=5000) == EUNSUPPORTED
    assert "4096" in _err(lib)


@pytest.mark.parametrize("kw, word", BAD_ALLOW, ids=BAD_IDS)
def test_finish_allowed_rejects_bad_allow(kw, word):
    lib = _lib.load()
    cat = _fake_catalog()
    pend = _lib.EbtPending()
    pend.cat = ctypes.cast(ctypes.pointer(cat), ctypes.c_void_p)
    pend.event = FAKE      # "submitted": the allow check comes before the event is waited for
    a = _allow(**kw)
    assert lib.ebt_cosine_topk_allowed_finish(ctypes.byref(pend), ctypes.byref(a)) == EINVAL
    assert word in _err(lib).lower(), _err(lib)
    assert lib.ebt_cosine_topk_allowed_finish(None, ctypes.byref(a)) == EINVAL


# ---- RecBatcher with an injected score_fn -----------------------------------------------------
class _Cat:
    def __init__(self, x):
        self.x, self.d, self.n = x, x.shape[1], x.shape[0]


class _Masks:
    """What RecBatcher needs of allow.AllowMasks: index() of a name or an index."""

    def __init__(self, sets, names):
        self.sets, self.names, self.n_masks = sets, names, len(sets)

    def index(self, m):
        if isinstance(m, str):
            if m not in self.names:
                raise _lib.EbertError(f"unknown allow mask {m!r}")
            return self.names.index(m)
        m = int(m)
        if m < 0 or m >= self.n_masks:
            raise _lib.EbertError(f"allow mask {m} is not in [0, {self.n_masks})")
        return m


def _score_fn(calls):
    def score(cat, k, liked, exclude, **kw):
        calls.append(dict(kw))
        qs = np.stack([R.mean_cosine_query(cat.x[l]) for l in liked])
        if "allow" in kw:
            masks, ids = kw["allow"]
            everything = set(range(cat.n))
            exclude = [sorted(set(e) | (everything - masks.sets[m])) if m >= 0 else e
                       for e, m in zip(exclude, ids)]
        return R.cosine_topk(qs, cat.x, k, exclude)
    return score


def _direct(cat, liked, excl, k, allowed=None):
    if allowed is not None:
        excl = sorted(set(excl) | (set(range(cat.n)) - allowed))
    s, r = R.cosine_topk(R.mean_cosine_query(cat.x[liked])[None, :], cat.x, k, [excl])
    keep = r[0] >= 0
    return s[0][keep], r[0][keep]


def test_batcher_unfiltered_batch_never_passes_allow():
    cat = _Cat(np.random.default_rng(0).standard_normal((200, 8)))
    masks = _Masks([set(range(0, 200, 2))], ["even"])
    calls = []
    b = RecBatcher(cat, max_batch=16, max_wait_ms=20.0, score_fn=_score_fn(calls),
                   allow_masks=masks)
    futs = [b.submit([i], [i + 1], 4) for i in range(12)]
    res = [f.result(timeout=30) for f in futs]
    b.close()
    assert calls and all("allow" not in c for c in calls)
    for i, (s, r) in enumerate(res):
        ws, wr = _direct(cat, [i], [i + 1], 4)
        np.testing.assert_array_equal(r, wr)


def test_batcher_bad_mask_fails_only_its_request_and_mixed_batch_is_one_call():
    cat = _Cat(np.random.default_rng(1).standard_normal((200, 8)))
    sets = [set(range(0, 200, 2)), {3, 5, 8}]
    masks = _Masks(sets, ["even", "tiny"])
    calls = []
    b = RecBatcher(cat, max_batch=16, max_wait_ms=200.0, score_fn=_score_fn(calls),
                   allow_masks=masks)
    reqs = [([1], [2], 5, None), ([4], [], 5, "even"), ([7], [8], 5, 1), ([9], [], 5, 0),
            ([11], [12], 5, None)]
    futs = [b.submit(l, e, k, allow=a) for l, e, k, a in reqs[:2]]
    bad = [b.submit([1], [], 5, allow=2), b.submit([1], [], 5, allow="nope"),
           b.submit([1], [], 5, allow=-7)]
    futs += [b.submit(l, e, k, allow=a) for l, e, k, a in reqs[2:]]
    res = [f.result(timeout=30) for f in futs]
    for f in bad:
        assert isinstance(f.exception(timeout=5), ValueError)
    b.close()
    filtered = [c for c in calls if "allow" in c]
    assert filtered, "no call carried allow="
    for c in filtered:     # unfiltered members of a filtered batch carry -1
        assert c["allow"][0] is masks and all(m in (-1, 0, 1) for m in c["allow"][1])
    assert any(-1 in c["allow"][1] for c in filtered) or len(calls) > 1
    for (l, e, k, a), (s, r) in zip(reqs, res):
        allowed = None if a is None else sets[masks.index(a)]
        ws, wr = _direct(cat, l, e, k, allowed)
        np.testing.assert_array_equal(r, wr)
        np.testing.assert_allclose(s, ws, atol=1e-15)
    assert len(res[2][1]) == 2          # mask "tiny" minus the rated row 8: rows 3 and 5


def test_batcher_without_masks_refuses_allow():
    cat = _Cat(np.random.default_rng(2).standard_normal((20, 4)))
    b = RecBatcher(cat, max_batch=4, max_wait_ms=5.0, score_fn=_score_fn([]))
    assert isinstance(b.submit([1], [], 3, allow=0).exception(timeout=5), ValueError)
    assert len(b.submit([1], [], 3).result(timeout=10)[1]) == 3
    b.close()
