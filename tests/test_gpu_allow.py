"""GPU: per-query allow masks (ebert.h 0.6.0: ebt_mask_allowed, ebt_allow_from_bool,
ebt_allow_set_rows, the _allowed entries, AllowMasks, score_topk(allow=), RecBatcher).

A filtered query's answer is the top k of (allowed rows minus excluded rows). The end-to-end
reference is the engine as it stood before the feature: the complement of the mask written as an
exclusion list, on the unfused path -- the same -inf entries in the same score chunks, so rows
must be identical and float64 scores bitwise identical. A second reference is the float64 oracle
with the same exclusion lists."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from inputs import gaussian
from oracle import restatement as R

pytestmark = pytest.mark.gpu
TDT = {"f32": torch.float32, "bf16": torch.bfloat16}
ATOL = 1e-10            # tests/test_gpu_catalog_remove.py
SENTINEL = np.float32(1234.5)
KINDS = {"f32": ("f32", 77), "bf16": ("bf16", 128)}   # image catalog / native catalog


def _t(x, dt, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev).to(TDT[dt])


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _pack(flags, words):
    """A bool vector as a mask row: numpy.packbits, little bit order, zero up to `words`."""
    by = np.packbits(np.asarray(flags, dtype=np.uint8), bitorder="little")
    out = np.zeros(words * 4, dtype=np.uint8)
    out[:by.size] = by
    return out.view("<u4")


# ---- 1. the kernel contract of ebt_mask_allowed -------------------------------------------------
def _ref_mask(S, nc, c0, table, ids):
    """numpy restatement: entry (b, j), j < nc, of a filtered query becomes -inf unless bit
    c0 + j of its mask is set; an id past the table masks everything."""
    out = S.copy()
    M, words = table.shape
    r = c0 + np.arange(nc)
    for b, m in enumerate(ids):
        if m < 0:
            continue
        ok = np.zeros(nc, dtype=bool)
        if m < M:
            inside = (r >> 5) < words
            w = table[m, np.minimum(r >> 5, words - 1)]
            ok = inside & (((w >> (r & 31).astype(np.uint32)) & 1) != 0)
        out[b, :nc][~ok] = -np.inf
    return out


def _contract_masks(c0, nc, n_rows, words):
    rng = np.random.default_rng(1000 * c0 + nc)
    rows = [np.ones(n_rows, bool), np.zeros(n_rows, bool)]
    edge = (c0 // 32 + 1) * 32                      # the first word boundary inside / past c0
    for p in [c0 + q for q in (0, 31, 32, 63, 64)] + [edge - 1, edge, 0, 31, 32, 63, 64]:
        f = np.zeros(n_rows, bool)
        f[p] = True
        rows.append(f)
    rows.append(rng.random(n_rows) < 0.5)
    rows.append(rng.random(n_rows) < 0.02)
    return np.stack([_pack(f, words) for f in rows])


@pytest.mark.parametrize("c0", [0, 37, 4096 - 5])
@pytest.mark.parametrize("nc", [1, 31, 64, 333])
@pytest.mark.parametrize("B", [1, 5])
def test_mask_allowed_contract(cuda_device, B, nc, c0):
    from robot_ebert_amd import _lib
    lib = _lib.load()
    dev = cuda_device
    ld = (nc + 3) // 4 * 4 + 8
    n_rows = 4096 + 333 + 200
    words = lib.ebt_allow_words(n_rows)
    table = _contract_masks(c0, nc, n_rows, words)
    M = table.shape[0]
    d_table = torch.from_numpy(table.view(np.int32)).to(dev)
    S0 = gaussian(7, B, ld, "f32").astype(np.float32)
    S0[:, nc:] = SENTINEL
    for m in range(M):
        # -1, valid ids and one id past the table in one launch
        ids = np.array([m] if B == 1 else [m, -1, M + 3, (m + 1) % M, m], dtype=np.int32)
        for id_set in ([ids] if B > 1 else [ids, np.array([-1], np.int32),
                                            np.array([M], np.int32)]):
            S = torch.from_numpy(S0).to(dev)
            d_ids = torch.from_numpy(id_set).to(dev)
            a = _lib.EbtAllow(masks=d_table.data_ptr(), words=words, n_masks=M,
                              mask_id=d_ids.data_ptr())
            _lib.call("ebt_mask_allowed", S.data_ptr(), ld, B, c0, c0 + nc, ctypes.byref(a),
                      _lib.stream_of(dev))
            want = _ref_mask(S0, nc, c0, table, id_set)
            got = S.cpu().numpy()
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (m, id_set)
            assert np.all(got[:, nc:] == SENTINEL)


def test_mask_allowed_last_rows_of_the_table(cuda_device):
    """The last word of a mask row: a table of exactly 128 rows against columns [100, 128) (a
    table that does not reach col_end is refused on the host, tests/test_allow_host.py)."""
    from robot_ebert_amd import _lib
    dev = cuda_device
    table = np.full((1, 4), 0xFFFFFFFF, dtype=np.uint32)
    S0 = gaussian(8, 3, 28, "f32").astype(np.float32)
    S = torch.from_numpy(S0).to(dev)
    d_table = torch.from_numpy(table.view(np.int32)).to(dev)
    d_ids = torch.tensor([0, -1, 0], dtype=torch.int32, device=dev)
    a = _lib.EbtAllow(masks=d_table.data_ptr(), words=4, n_masks=1, mask_id=d_ids.data_ptr())
    _lib.call("ebt_mask_allowed", S.data_ptr(), 28, 3, 100, 128, ctypes.byref(a),
              _lib.stream_of(dev))
    assert np.array_equal(S.cpu().numpy().view(np.uint32), S0.view(np.uint32))   # all allowed


# ---- 2. the builders ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_allow_from_bool_is_packbits(cuda_device, n):
    from robot_ebert_amd import _lib
    lib = _lib.load()
    dev = cuda_device
    rng = np.random.default_rng(n)
    for extra in (0, 8):                       # the exact row, and one with a tail of whole words
        words = lib.ebt_allow_words(n) + extra
        for flags in (rng.random(n) < 0.5, np.ones(n, bool), rng.integers(0, 256, n) * (
                rng.random(n) < 0.3)):
            f8 = np.asarray(flags).astype(np.uint8)
            row = torch.full((words,), -1, dtype=torch.int32, device=dev)   # stale bits
            d_f = torch.from_numpy(f8).to(dev)
            _lib.call("ebt_allow_from_bool", d_f.data_ptr(), n, row.data_ptr(), words,
                      _lib.stream_of(dev))
            assert np.array_equal(_u32(row), _pack(f8 != 0, words))


def test_allow_set_rows(cuda_device):
    from robot_ebert_amd import _lib
    dev = cuda_device
    words = 8                                          # rows [0, 256)
    row = torch.zeros(words, dtype=torch.int32, device=dev)

    def run(rows, allowed):
        d = torch.tensor(rows, dtype=torch.int64, device=dev)
        _lib.call("ebt_allow_set_rows", row.data_ptr(), words, d.data_ptr(), len(rows),
                  1 if allowed else 0, _lib.stream_of(dev))

    want = np.zeros(256, bool)
    # duplicates, rows outside [0, 256) ignored, every bit of word 1, both ends
    rows = [0, 255, 5, 5, 5, 200, -1, 256, 10 ** 12, -(10 ** 12)] + list(range(32, 64)) * 3
    run(rows, True)
    want[[r for r in rows if 0 <= r < 256]] = True
    assert np.array_equal(_u32(row), _pack(want, words))
    clear = [5, 5, 33, 40, 40, 63, 255, 256, -3, 100]   # 100 was never set
    run(clear, False)
    want[[r for r in clear if 0 <= r < 256]] = False
    assert np.array_equal(_u32(row), _pack(want, words))
    run(list(range(256)), False)
    assert not _u32(row).any()


def test_allow_masks_class(cuda_device):
    import robot_ebert_amd as ebt
    dev = cuda_device
    m = ebt.AllowMasks(1000, 3, names=["a", "b", "c"], device=dev)
    assert m.words == 32 and tuple(m.table.shape) == (3, 32) and not _u32(m.table).any()
    flags = np.random.default_rng(5).random(1000) < 0.3
    m.from_bool("b", torch.from_numpy(flags).to(dev))
    m.set(2, np.nonzero(flags)[0].tolist())             # the same set, by the other builder
    assert np.array_equal(_u32(m.table[1]), _u32(m.table[2]))
    assert m.count("b") == int(flags.sum()) == m.count(2) and m.count(0) == 0
    assert np.array_equal(m.to_bool(1).cpu().numpy(), flags)
    assert m.index("c") == 2
    for bad in ("zz", 3, -1):
        with pytest.raises(ebt.EbertError):
            m.index(bad)
    with pytest.raises(ebt.EbertError):
        m.set(0, [1000])


# ---- 3. end to end ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _host_catalog(n, kind):
    dt, d = KINDS[kind]
    return gaussian(1, n, d, dt)


_CATS = {}


def _catalog(n, kind, dev):
    import robot_ebert_amd as ebt
    key = (n, kind)
    if key not in _CATS:
        _CATS[key] = ebt.Catalog(_t(_host_catalog(n, kind), KINDS[kind][0], dev))
    return _CATS[key]


def _mask_flags(n, seed=4):
    """densities 1.0, 0.3, 3 / n (fewer than k allowed rows) and 0 (an all-zero mask)."""
    rng = np.random.default_rng(seed)
    three = np.zeros(n, bool)
    three[rng.choice(n, 3, replace=False)] = True
    return [np.ones(n, bool), rng.random(n) < 0.3, three, np.zeros(n, bool)]


def _masks(cat_or_n, flags, dev, by_rows=False):
    import robot_ebert_amd as ebt
    m = (ebt.AllowMasks(cat_or_n, len(flags), device=dev) if isinstance(cat_or_n, int)
         else ebt.AllowMasks(cat_or_n, len(flags)))
    for i, f in enumerate(flags):
        if by_rows:
            m.set(i, np.nonzero(f)[0].tolist())
        else:
            m.from_bool(i, torch.from_numpy(np.asarray(f)).to(dev))
    return m


def _ids(B, n_masks):
    """Every mask and -1, mixed in one batch."""
    return [(b % (n_masks + 1)) - 1 for b in range(B)]


def _rated(B, n, lo=0, liked=None):
    """Rated rows; a user's liked rows are among them, as in lib.py:47-48 (and two liked rows a, b
    of one user tie exactly, (1 + cos(a, b)) / 2 each, so they must not be candidates of a test
    that compares an order)."""
    out = [list(range(lo + b % 50, lo + n, 97)) for b in range(B)]
    if liked is not None:
        out = [sorted(set(e) | set(l)) for e, l in zip(out, liked)]
    return out


def _complement(rated, flags, ids, lo=0, n=None):
    """rated[b] united with the catalog rows [lo, lo + n) that query b's mask does not allow."""
    out = []
    for e, m in zip(rated, ids):
        if m < 0:
            out.append(sorted(e))
            continue
        f = flags[m]
        hi = lo + (n if n is not None else len(f))
        rows = np.arange(lo, hi)
        out.append(sorted(set(e) | set(rows[~f[lo:hi]].tolist())))
    return out


def _queries(B, kind, n, qkind):
    dt, d = KINDS[kind]
    if qkind == "dense":
        return dict(q=gaussian(2, B, d, "f32")), None
    rng = np.random.default_rng(6)
    liked = [sorted(rng.choice(n, 1 + b % 4, replace=False).tolist()) for b in range(B)]
    return None, liked


def _same(a, b):
    (s, r), (s2, r2) = a, b
    r, r2 = r.cpu().numpy(), r2.cpu().numpy()
    np.testing.assert_array_equal(r, r2)
    s, s2 = s.cpu().numpy(), s2.cpu().numpy()
    assert np.array_equal(s.view(np.uint64), s2.view(np.uint64)), "scores differ bitwise"


@pytest.mark.parametrize("qkind", ["dense", "liked"])
@pytest.mark.parametrize("k", [1, 10, 100])
@pytest.mark.parametrize("B", [5, 130])
@pytest.mark.parametrize("kind", ["f32", "bf16"])
@pytest.mark.parametrize("n", [333, 1000])
def test_equals_complement_exclusion(cuda_device, n, kind, B, k, qkind):
    """Masks of density 1.0, 0.3, 3 / n and 0 mixed with unfiltered queries in one batch, eight
    chunks at n = 1000: equal to the exclusion of the complement on the unfused path."""
    import robot_ebert_amd as ebt
    dev = cuda_device
    cat = _catalog(n, kind, dev)
    flags = _mask_flags(n)
    masks = _masks(cat, flags, dev, by_rows=(k == 10))     # either builder, the same sets
    ids = _ids(B, len(flags))
    dense, liked = _queries(B, kind, n, qkind)
    rated = _rated(B, n, liked=liked)
    kw = dict(liked=liked) if liked is not None else dict(
        queries=torch.from_numpy(dense["q"].astype(np.float32)).to(dev))
    got = ebt.score_topk(cat, k, exclude=rated, chunk_rows=128, allow=(masks, ids), **kw)
    want = ebt.score_topk(cat, k, exclude=_complement(rated, flags, ids), chunk_rows=128,
                          fuse=False, **kw)
    _same(got, want)
    r = got[1].cpu().numpy()
    for b, m in enumerate(ids):                             # the NaN / -1 slots
        if m == 3:
            assert (r[b] == -1).all() and np.isnan(got[0][b].cpu().numpy()).all()
        if m == 2:
            assert (r[b] >= 0).sum() == min(k, len(set(np.nonzero(flags[2])[0]) - set(rated[b])))
    # a device int32 id tensor and the default chunking give the same answer
    if k == 10 and B == 5:
        d_ids = torch.tensor(ids, dtype=torch.int32, device=dev)
        _same(ebt.score_topk(cat, k, exclude=rated, allow=(masks, d_ids), **kw), want)


@pytest.mark.parametrize("flagset", ["mfma", "exact"])
@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_prepared_entry_with_row_offset(cuda_device, kind, flagset):
    """A shard whose first GLOBAL row is 37 through the prepared-level entry: col_begin of every
    chunk is unaligned against the mask words."""
    import robot_ebert_amd as ebt
    from robot_ebert_amd import _lib, search
    dev = cuda_device
    n, off, n_glob, B, k = 1000, 37, 1100, 130, 10
    dt, d = KINDS[kind]
    cat = ebt.Catalog(_t(_host_catalog(n, kind), dt, dev), row_offset=off, n_global=n_glob)
    flags = _mask_flags(n_glob, seed=9)
    masks = _masks(cat, flags, dev)
    assert masks.n_rows == n_glob
    ids = _ids(B, len(flags))
    rated = _rated(B, n, lo=off)
    q = torch.from_numpy(gaussian(2, B, d, "f32").astype(np.float32)).to(dev)
    qb = search.prepare_queries(cat, queries=q)
    kp = 64
    fl = _lib.EBT_FLAG_EXACT if flagset == "exact" else 0
    s, r, c = search.run_pipeline(cat, qb, k, kp, search.csr_from_lists(rated, dev),
                                  chunk_rows=128, flags=fl, allow=(masks, ids))
    ex = search.csr_from_lists(_complement(rated, flags, ids, lo=off, n=n), dev)
    s2, r2, c2 = search.run_pipeline(cat, qb, k, kp, ex, chunk_rows=128,
                                     flags=fl or _lib.EBT_FLAG_NO_FUSE)
    _same((s, r), (s2, r2))
    assert torch.equal(c, c2)
    rr = r.cpu().numpy()
    assert rr[rr >= 0].min() >= off and rr.max() < off + n


@pytest.mark.parametrize("qkind", ["dense", "liked"])
@pytest.mark.parametrize("k", [10, 100])
@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_equals_float64_oracle(cuda_device, kind, k, qkind):
    import robot_ebert_amd as ebt
    dev = cuda_device
    n, B = 1000, 130
    cat = _catalog(n, kind, dev)
    c = _host_catalog(n, kind)
    flags = _mask_flags(n)
    masks = _masks(cat, flags, dev)
    ids = _ids(B, len(flags))
    dense, liked = _queries(B, kind, n, qkind)
    rated = _rated(B, n, liked=liked)
    excl = _complement(rated, flags, ids)
    if liked is not None:
        got = ebt.score_topk(cat, k, liked=liked, exclude=rated, allow=(masks, ids))
        s1, r1 = R.liked_topk(c, liked, k + 1, excl)
    else:
        q = dense["q"].astype(np.float32)
        got = ebt.score_topk(cat, k, queries=torch.from_numpy(q).to(dev), exclude=rated,
                             allow=(masks, ids))
        s1, r1 = R.cosine_topk(q.astype(np.float64), c, k + 1, excl)
    # the oracle's k-th and (k+1)-th scores differ for every query: no query is left out
    both = r1[:, k] >= 0
    assert (s1[both, k - 1] > s1[both, k]).all()
    s_ref, r_ref = s1[:, :k], r1[:, :k]
    np.testing.assert_array_equal(got[1].cpu().numpy(), r_ref)
    m = r_ref >= 0
    np.testing.assert_allclose(got[0].cpu().numpy()[m], s_ref[m], rtol=0, atol=ATOL)
    assert np.isnan(got[0].cpu().numpy()[~m]).all()


# ---- 4. retries under a mask --------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_widen_rounds_keep_each_query_its_mask(cuda_device, kind):
    """kprime = k never certifies a query with more than k candidates at the first pass: the
    widen rounds of ebt_cosine_topk_allowed_finish regroup the queries, and every retried query
    must keep its own mask."""
    import robot_ebert_amd as ebt
    dev = cuda_device
    n, B, k = 1000, 130, 12
    cat = _catalog(n, kind, dev)
    flags = _mask_flags(n)
    masks = _masks(cat, flags, dev)
    ids = _ids(B, len(flags))
    rated = _rated(B, n)
    q = torch.from_numpy(gaussian(2, B, KINDS[kind][1], "f32").astype(np.float32)).to(dev)
    timer = ebt.Timer()
    forced = ebt.score_topk(cat, k, queries=q, exclude=rated, kprime=k, timer=timer,
                            allow=(masks, ids))
    assert timer.query("rescore")[1] >= 2, "no retry was exercised"
    _same(forced, ebt.score_topk(cat, k, queries=q, exclude=rated, allow=(masks, ids)))
    _same(forced, ebt.score_topk(cat, k, queries=q, fuse=False,
                                 exclude=_complement(rated, flags, ids)))


@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_exact_screen_is_filtered(cuda_device, kind):
    """EBT_FLAG_EXACT goes through the same chunks: equal to the MFMA-screened answer."""
    import robot_ebert_amd as ebt
    from robot_ebert_amd import _lib, search
    dev = cuda_device
    n, B, k = 1000, 130, 10
    cat = _catalog(n, kind, dev)
    flags = _mask_flags(n)
    masks = _masks(cat, flags, dev)
    ids = _ids(B, len(flags))
    rated = _rated(B, n)
    q = torch.from_numpy(gaussian(2, B, KINDS[kind][1], "f32").astype(np.float32)).to(dev)
    qb = search.prepare_queries(cat, queries=q)
    s, r, c = search.run_pipeline(cat, qb, k, 64, search.csr_from_lists(rated, dev),
                                  chunk_rows=128, flags=_lib.EBT_FLAG_EXACT, allow=(masks, ids))
    assert bool((c == 1).all())
    _same((s, r), ebt.score_topk(cat, k, queries=q, exclude=rated, allow=(masks, ids)))


# ---- 5. allow = NULL, the submit / finish pair --------------------------------------------------
def _c_pair(cat, q, k, excl, allow_struct, flags, pinned):
    """ebt_cosine_topk_allowed_submit + _finish called directly."""
    from robot_ebert_amd import _lib
    lib = _lib.load()
    dev = cat.device
    B = q.shape[0]
    opt = _lib.EbtOptions(kprime=0, flags=flags, chunk_rows=0)
    need = lib.ebt_workspace_bytes(ctypes.byref(cat.cstruct), B, k, ctypes.byref(opt))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    s = torch.empty((B, k), dtype=torch.float64, device=dev)
    r = torch.empty((B, k), dtype=torch.int64, device=dev)
    if pinned:
        cert_t = torch.full((B + 1,), 9, dtype=torch.int32, pin_memory=True)
        cert_p = ctypes.c_void_p(cert_t.data_ptr())
    else:
        cert_t = np.full(B + 1, 9, dtype=np.int32)
        cert_p = cert_t.ctypes.data_as(ctypes.c_void_p)
    pend = _lib.EbtPending()
    al = ctypes.byref(allow_struct) if allow_struct is not None else None
    eo, er = excl if excl is not None else (None, None)
    _lib.call("ebt_cosine_topk_allowed_submit", ctypes.byref(cat.cstruct), q.data_ptr(),
              _lib.DTYPE_CODE[q.dtype], B, int(q.stride(0)), None, None, k, _lib.ptr(eo),
              _lib.ptr(er), ctypes.byref(opt), ws.data_ptr(), need, s.data_ptr(), r.data_ptr(),
              cert_p, ctypes.byref(pend), None, _lib.stream_of(dev), al)
    _lib.call("ebt_cosine_topk_allowed_finish", ctypes.byref(pend), al)
    torch.cuda.synchronize(dev)
    return s, r


def test_null_allow_is_the_unfiltered_call(cuda_device):
    """allow = NULL / None on the default (fused) path: bitwise the unfiltered call."""
    import robot_ebert_amd as ebt
    from robot_ebert_amd import search
    dev = cuda_device
    n, d, B, k = 6000, 64, 130, 10
    cat = ebt.Catalog(_t(gaussian(1, n, d, "f32"), "f32", dev))
    assert search.plan(cat, B, k)["fused"]
    q = torch.from_numpy(gaussian(2, B, d, "f32").astype(np.float32)).to(dev)
    rated = _rated(B, n)
    want = ebt.score_topk(cat, k, queries=q, exclude=rated)
    _same(ebt.score_topk(cat, k, queries=q, exclude=rated, allow=None), want)
    _same(_c_pair(cat, q, k, search.csr_from_lists(rated, dev), None, 0, True), want)
    lib = ebt.load()
    s = torch.empty((B, k), dtype=torch.float64, device=dev)
    r = torch.empty((B, k), dtype=torch.int64, device=dev)
    need = lib.ebt_workspace_bytes(ctypes.byref(cat.cstruct), B, k, None)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    eo, er = search.csr_from_lists(rated, dev)
    from robot_ebert_amd import _lib
    _lib.call("ebt_cosine_topk_allowed", ctypes.byref(cat.cstruct), q.data_ptr(), _lib.EBT_F32, B,
              d, None, None, k, eo.data_ptr(), er.data_ptr(), None, ws.data_ptr(), need,
              s.data_ptr(), r.data_ptr(), None, _lib.stream_of(dev), None)
    _same((s, r), want)


@pytest.mark.parametrize("pinned", [True, False], ids=["pinned", "pageable"])
def test_submit_finish_pair(cuda_device, pinned):
    import robot_ebert_amd as ebt
    from robot_ebert_amd import _lib, search
    dev = cuda_device
    n, B, k = 1000, 130, 10
    cat = _catalog(n, "f32", dev)
    flags = _mask_flags(n)
    masks = _masks(cat, flags, dev)
    ids = _ids(B, len(flags))
    rated = _rated(B, n)
    q = torch.from_numpy(gaussian(2, B, 77, "f32").astype(np.float32)).to(dev)
    d_ids = masks.mask_ids(ids, B)
    got = _c_pair(cat, q, k, search.csr_from_lists(rated, dev), masks.cstruct(d_ids),
                  _lib.EBT_FLAG_NO_FUSE, pinned)
    _same(got, ebt.score_topk(cat, k, queries=q, fuse=False,
                              exclude=_complement(rated, flags, ids)))


def test_hooks_are_refused(cuda_device):
    import robot_ebert_amd as ebt
    dev = cuda_device
    cat = _catalog(333, "f32", dev)
    masks = _masks(cat, _mask_flags(333), dev)
    q = torch.from_numpy(gaussian(2, 5, 77, "f32").astype(np.float32)).to(dev)
    for kw in (dict(t_floor_hook=lambda v, e: None), dict(liked_sum_hook=lambda x: x)):
        with pytest.raises(ebt.EbertError, match="allow"):
            ebt.score_topk(cat, 5, queries=q, allow=(masks, [0] * 5), **kw)
    with pytest.raises(ebt.EbertError):
        ebt.score_topk(cat, 5, queries=q, allow=(masks, [0, 1, 2, 3, 4]))   # mask 4 of 4
    with pytest.raises(ebt.EbertError):
        ebt.score_topk(cat, 5, queries=q, allow=(masks, [0]))              # one id for five


# ---- 6. live edits -----------------------------------------------------------------------------
def test_masks_follow_remove_and_append(cuda_device):
    """Catalog.remove -> AllowMasks.apply_moves -> append (new rows in no mask until set): equal
    to a fresh catalog and fresh masks built from the edited matrix and id -> genre map."""
    import robot_ebert_amd as ebt
    dev = cuda_device
    n, cap, d, G, B, k = 1000, 1100, 77, 3, 64, 10
    c = gaussian(1, n, d, "f32")
    ids = [f"m{i}" for i in range(n)]
    rng = np.random.default_rng(12)
    genre = {t: int(g) for t, g in zip(ids, rng.integers(0, G, n))}
    cat = ebt.Catalog(_t(c, "f32", dev), ids=list(ids), capacity=cap)
    masks = ebt.AllowMasks(cat, G, names=[f"g{g}" for g in range(G)])
    assert masks.words == ebt.load().ebt_allow_words(cap)
    for g in range(G):
        masks.set(g, [t for t in ids if genre[t] == g])               # by string id
    gone = [int(x) for x in rng.choice(n, 37, replace=False)] + [n - 1, 0]
    gone = sorted(set(gone))
    moves = cat.remove(gone)
    assert moves
    masks.apply_moves(moves, cat.n)
    extra = gaussian(13, 20, d, "f32")
    new_ids = [f"x{i}" for i in range(20)]
    cat.append(_t(extra, "f32", dev), ids=new_ids)
    for t in new_ids[:10]:                                            # ten of them get a genre
        genre[t] = 1
    q = torch.from_numpy(gaussian(2, B, d, "f32").astype(np.float32)).to(dev)
    qids = [b % (G + 1) - 1 for b in range(B)]
    rated = _rated(B, cat.n)
    before_set = ebt.score_topk(cat, k, queries=q, exclude=rated, allow=(masks, qids))
    filtered = torch.tensor([m >= 0 for m in qids], device=dev)
    assert before_set[1][filtered].max().item() < cat.n - 20          # appended: in no mask yet
    masks.set("g1", new_ids[:10])
    # fresh objects from the edited matrix and map
    host = cat.data.cpu().numpy()
    fresh = ebt.Catalog(_t(host, "f32", dev), ids=list(cat.ids), capacity=cap)
    fresh_masks = ebt.AllowMasks(fresh, G)
    for g in range(G):
        fresh_masks.from_bool(g, torch.tensor([genre.get(t, -1) == g for t in fresh.ids],
                                              device=dev))
    assert np.array_equal(_u32(masks.table), _u32(fresh_masks.table))
    got = ebt.score_topk(cat, k, queries=q, exclude=rated, allow=(masks, qids))
    _same(got, ebt.score_topk(fresh, k, queries=q, exclude=rated, allow=(fresh_masks, qids)))
    # and the oracle on the edited matrix
    flags = [np.array([genre.get(t, -1) == g for t in fresh.ids]) for g in range(G)]
    s_ref, r_ref = R.cosine_topk(q.cpu().numpy().astype(np.float64), host.astype(np.float64), k,
                                 _complement(rated, flags, qids))
    np.testing.assert_array_equal(got[1].cpu().numpy(), r_ref)
    np.testing.assert_allclose(got[0].cpu().numpy(), s_ref, rtol=0, atol=ATOL)


# ---- 7. RecBatcher -----------------------------------------------------------------------------
def test_batcher_mixed_requests(cuda_device):
    import robot_ebert_amd as ebt
    from robot_ebert_amd.batcher import RecBatcher
    dev = cuda_device
    n, k = 1000, 10
    cat = _catalog(n, "f32", dev)
    flags = _mask_flags(n)
    masks = _masks(cat, flags, dev)
    masks.names = ["all", "third", "three", "none"]
    rng = np.random.default_rng(21)
    reqs = []
    for i in range(40):
        liked = sorted(rng.choice(n, 1 + i % 3, replace=False).tolist())
        rated = sorted(set(rng.choice(n, 20, replace=False).tolist()) | set(liked))
        allow = [None, 0, "third", 2, "none"][i % 5]
        reqs.append((liked, rated, k, allow))
    b = RecBatcher(cat, max_batch=64, max_wait_ms=50.0, allow_masks=masks)
    try:
        futs = [b.submit(l, e, kk, allow=a) for l, e, kk, a in reqs]
        bad = b.submit([1], [], k, allow=9)
        res = [f.result(timeout=60) for f in futs]
        assert isinstance(bad.exception(timeout=5), ValueError)
        plain = [b.submit(l, e, kk).result(timeout=60) for l, e, kk, _ in reqs[:3]]
    finally:
        b.close()
    for (l, e, kk, a), (s, r) in zip(reqs, res):
        mid = -1 if a is None else masks.index(a)
        ws, wr = ebt.score_topk(cat, kk, liked=[l], exclude=[e], allow=(masks, [mid]))
        wr, ws = wr[0].cpu().numpy(), ws[0].cpu().numpy()
        keep = wr >= 0
        np.testing.assert_array_equal(r, wr[keep])
        np.testing.assert_allclose(s, ws[keep], rtol=0, atol=ATOL)
        if a == "none":
            assert len(r) == 0
    for (l, e, kk, _), (s, r) in zip(reqs[:3], plain):
        ws, wr = ebt.score_topk(cat, kk, liked=[l], exclude=[e])
        np.testing.assert_array_equal(r, wr[0].cpu().numpy())
