"""GPU: materialised sub-catalogs (ebert.h 0.7.0: ebt_allow_count, ebt_allow_rows,
ebt_catalog_gather_rows, ebt_sub_exclusions, ebt_sub_rows_to_global; AllowMasks.materialize and
the routing of score_topk(allow=) over them).

The answer of a filtered query must not depend on whether its mask was materialised: the same
rows and bitwise the same float64 scores as the mask pass gives (the engine as it stood before the
feature), and equal to the float64 oracle over (allowed rows minus excluded rows)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from inputs import gaussian
from oracle import restatement as R

pytestmark = pytest.mark.gpu
TDT = {"f32": torch.float32, "bf16": torch.bfloat16}
ATOL = 1e-10            # tests/test_gpu_allow.py
KINDS = {"f32": ("f32", 72), "bf16": ("bf16", 64)}   # image catalog, d % 64 != 0 / native catalog
SIZES = [333, 1000]
M_ONE, M_37, M_THIRD, M_HALF = 0, 1, 2, 3            # the masks of _flags, by index
MATERIALISED = (M_ONE, M_37, M_THIRD)                # M_HALF stays on the mask pass


def _t(x, dt, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev).to(TDT[dt])


def _words(n):
    return ((n + 31) // 32 + 3) // 4 * 4


@functools.lru_cache(maxsize=None)
def _flags(n):
    """Four masks over the 32 * words rows of the table: 1 row, 37 rows (on both sides of 32-bit
    word and 128-row boundaries, the last row included), about n / 3 rows, about n / 2 rows. Every
    mask also has bits set at or above n (from_bool can set them; they must be ignored)."""
    rng = np.random.default_rng(40 + n)
    total = 32 * _words(n)
    out = []
    one = np.zeros(total, bool)
    one[127] = True
    out.append(one)
    edge = [0, 31, 32, 33, 63, 64, 127, 128, 129, 255, 256, 257, n - 1, n - 2]
    more = rng.choice(np.setdiff1d(np.arange(n), edge), 37 - len(edge), replace=False)
    m37 = np.zeros(total, bool)
    m37[edge] = True
    m37[more] = True
    out.append(m37)
    for p in (1 / 3, 1 / 2):
        f = np.zeros(total, bool)
        f[:n] = rng.random(n) < p
        f[[127, 128]] = True
        out.append(f)
    for f in out:
        f[[n, n + 5, total - 1]] = True
    assert [int(f[:n].sum()) for f in out[:2]] == [1, 37]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _host_catalog(n, kind):
    dt, d = KINDS[kind]
    return gaussian(1, n, d, dt)


_CATS = {}


def _setup(n, kind, dev):
    """(catalog, masks with MATERIALISED materialised, the same masks never materialised)."""
    import robot_ebert_amd as ebt
    key = (n, kind)
    if key not in _CATS:
        cat = ebt.Catalog(_t(_host_catalog(n, kind), KINDS[kind][0], dev))
        both = []
        for _ in range(2):
            m = ebt.AllowMasks(cat, 4)
            for i, f in enumerate(_flags(n)):
                m.from_bool(i, torch.from_numpy(f).to(dev))
            both.append(m)
        for i in MATERIALISED:
            assert both[0].materialize(i) == int(_flags(n)[i][:n].sum())
        _CATS[key] = (cat, both[0], both[1])
    return _CATS[key]


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _same(a, b):
    (s, r), (s2, r2) = a, b
    r, r2 = r.cpu().numpy(), r2.cpu().numpy()
    np.testing.assert_array_equal(r, r2)
    s, s2 = s.cpu().numpy(), s2.cpu().numpy()
    assert np.array_equal(s.view(np.uint64), s2.view(np.uint64)), "scores differ bitwise"


# ---- 1. the compaction ----------------------------------------------------------------------------
@pytest.mark.parametrize("mask", [M_ONE, M_37, M_THIRD, M_HALF])
@pytest.mark.parametrize("n", SIZES)
def test_allow_rows_and_count(cuda_device, n, mask):
    from robot_ebert_amd import _lib
    lib = _lib.load()
    dev = cuda_device
    _, _, masks = _setup(n, "f32", dev)
    flags = _flags(n)[mask]
    row, words = masks.table[mask], masks.words
    want = torch.nonzero(masks.to_bool(mask, n)).flatten().cpu().numpy()
    assert np.array_equal(want, np.nonzero(flags[:n])[0])
    m = len(want)
    # the rank prefix from numpy: popcounts of the words with the bits >= n cleared
    live = flags.copy()
    live[n:] = False
    pop = live.reshape(words, 32).sum(1)
    want_rank = np.concatenate([[0], np.cumsum(pop)[:-1]]).astype(np.uint32)
    need = lib.ebt_allow_rows_bytes(words)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    for cap in (m, m + 7, max(m - 5, 0), 0):
        rows = torch.full((cap + 3,), -7, dtype=torch.int64, device=dev)
        rank = torch.full((words,), -1, dtype=torch.int32, device=dev)
        cnt = torch.full((1,), -1, dtype=torch.int64, device=dev)
        _lib.call("ebt_allow_rows", row.data_ptr(), words, n, rows.data_ptr(), cap,
                  rank.data_ptr(), cnt.data_ptr(), ws.data_ptr(), need, _lib.stream_of(dev))
        got = rows.cpu().numpy()
        assert int(cnt.item()) == m                        # counted even when not written
        assert np.array_equal(got[:min(cap, m)], want[:min(cap, m)])
        assert (got[min(cap, m):] == -7).all()             # nothing past cap, nothing past count
        assert np.array_equal(_u32(rank), want_rank)
    cnt = torch.full((1,), -1, dtype=torch.int64, device=dev)
    _lib.call("ebt_allow_count", row.data_ptr(), words, n, cnt.data_ptr(), _lib.stream_of(dev))
    assert int(cnt.item()) == m
    # AllowMasks.count keeps its value: every bit of the row, those at or above n included
    assert masks.count(mask) == int(flags.sum()) == m + 3


def test_allow_rows_many_workgroups(cuda_device):
    """600 words: three workgroups, the last one partial; n_rows inside a word."""
    from robot_ebert_amd import _lib
    lib = _lib.load()
    dev = cuda_device
    words, n = 600, 600 * 32 - 13
    flags = np.random.default_rng(3).random(words * 32) < 0.4
    row = torch.from_numpy(np.packbits(flags, bitorder="little").view(np.int32)).to(dev)
    want = np.nonzero(flags[:n])[0]
    live = flags.copy()
    live[n:] = False
    pop = live.reshape(words, 32).sum(1)
    need = lib.ebt_allow_rows_bytes(words)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    rows = torch.full((len(want) + 3,), -7, dtype=torch.int64, device=dev)
    rank = torch.empty(words, dtype=torch.int32, device=dev)
    cnt = torch.empty(1, dtype=torch.int64, device=dev)
    _lib.call("ebt_allow_rows", row.data_ptr(), words, n, rows.data_ptr(), len(want),
              rank.data_ptr(), cnt.data_ptr(), ws.data_ptr(), need, _lib.stream_of(dev))
    assert int(cnt.item()) == len(want)
    assert np.array_equal(rows.cpu().numpy()[:-3], want) and (rows.cpu().numpy()[-3:] == -7).all()
    assert np.array_equal(_u32(rank), np.concatenate([[0], np.cumsum(pop)[:-1]]).astype(np.uint32))


# ---- 2. the gather --------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", MATERIALISED)
@pytest.mark.parametrize("kind", ["f32", "bf16"])
@pytest.mark.parametrize("n", SIZES)
def test_gather_equals_fresh_catalog(cuda_device, n, kind, mask):
    """The sub-catalog of materialize: data, gnorm, inv32 (with its 1.0f tail) and image bitwise
    those of a catalog built from the same rows."""
    import robot_ebert_amd as ebt
    dev = cuda_device
    cat, masks, _ = _setup(n, kind, dev)
    sub = masks._subs[mask]
    rows = np.nonzero(_flags(n)[mask][:n])[0]
    assert np.array_equal(sub.rows.cpu().numpy(), rows) and sub.m == len(rows)
    view = sub.catalog
    fresh = ebt.Catalog(cat.data[torch.from_numpy(rows).to(dev)].contiguous())
    m = len(rows)
    assert (view.n, view.d, view.native, view.img_dtype, view.ld_img, view.d_pad) == \
        (fresh.n, fresh.d, fresh.native, fresh.img_dtype, fresh.ld_img, fresh.d_pad)
    assert view.u_cat == cat.u_cat and view.row_offset == 0
    bits = {2: torch.int16, 4: torch.int32, 8: torch.int64}
    assert torch.equal(view.data.contiguous().view(bits[view.data.element_size()]),
                       fresh.data.view(bits[fresh.data.element_size()]))
    assert torch.equal(view.gnorm[:m].view(torch.int64), fresh.gnorm[:m].view(torch.int64))
    assert torch.equal(view.inv32[:m].view(torch.int32), fresh.inv32[:m].view(torch.int32))
    m128 = (m + 127) // 128 * 128
    assert view.inv32.numel() == m128 and bool((view.inv32[m:] == 1.0).all())
    assert torch.equal(view.image[:m].contiguous().view(torch.int16),
                       fresh.image[:m].contiguous().view(torch.int16))
    assert (view.image.data_ptr() == view.data.data_ptr()) == (kind == "bf16")


@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_gather_out_of_range_rows(cuda_device, kind):
    """The C entry with a list that is neither sorted nor all inside the parent: a row outside
    [0, n) gives a zero row with gnorm 1 and inv32 1; the others are the parent's rows."""
    from robot_ebert_amd import _lib
    dev = cuda_device
    n = 333
    cat, _, _ = _setup(n, kind, dev)
    d = cat.d
    lst = [5, n + 3, -1, 7, n, 332, 5, 2 ** 40]
    m = len(lst)
    rows = torch.tensor(lst, dtype=torch.int64, device=dev)
    data = torch.full((m, d), 3.0, dtype=cat.data.dtype, device=dev)
    gnorm = torch.full((m,), 9.0, dtype=torch.float64, device=dev)
    inv32 = torch.full((128,), 9.0, dtype=torch.float32, device=dev)
    alias = cat.image.data_ptr() == cat.data.data_ptr()
    image = None if alias else torch.full((m, cat.ld_img), 3.0, dtype=cat.img_torch_dtype,
                                          device=dev)
    sub = _lib.EbtCatalog()
    _lib.call("ebt_catalog_gather_rows", ctypes.byref(cat.cstruct), rows.data_ptr(), m,
              data.data_ptr(), d, gnorm.data_ptr(), inv32.data_ptr(), _lib.ptr(image),
              ctypes.byref(sub), _lib.stream_of(dev))
    assert (sub.n, sub.row_offset, sub.d, sub.ld, sub.native) == (m, 0, d, d, int(cat.native))
    assert sub.image == (data.data_ptr() if alias else image.data_ptr())
    assert bool((inv32[m:] == 1.0).all())
    for i, r in enumerate(lst):
        if 0 <= r < n:
            assert torch.equal(data[i], cat.data[r]) and gnorm[i] == cat.gnorm[r]
            assert inv32[i] == cat.inv32[r]
            if image is not None:
                assert torch.equal(image[i], cat.image[r])
        else:
            assert not bool(data[i].any()) and gnorm[i] == 1.0 and inv32[i] == 1.0
            if image is not None:
                assert not bool(image[i].any())


# ---- 3. exclusions and rows back ------------------------------------------------------------------
@pytest.mark.parametrize("mask", [M_ONE, M_37, M_THIRD])
@pytest.mark.parametrize("n", SIZES)
def test_sub_exclusions_equal_searchsorted(cuda_device, n, mask):
    from robot_ebert_amd import _lib
    lib = _lib.load()
    dev = cuda_device
    _, masks, _ = _setup(n, "f32", dev)
    sub = masks._subs[mask]
    flags = _flags(n)[mask]
    allowed = np.nonzero(flags[:n])[0]
    disallowed = np.nonzero(~flags[:n])[0]
    rng = np.random.default_rng(n + mask)
    segs = [np.array([], np.int64),                                    # empty
            np.sort(rng.choice(disallowed, 40, replace=False)),        # entirely disallowed
            np.arange(n + 40),                                         # every row and rows >= n
            allowed.copy(),                                            # entirely allowed
            np.array([], np.int64),
            np.array([n, n + 5, 32 * masks.words - 1, 2 ** 40])]       # set bits at or above n
    segs += [np.sort(rng.choice(n, 70, replace=False)) for _ in range(67)]   # > 64: two ballots
    B = len(segs)
    pad = 11                                                           # off[0] > 0
    lens = np.array([len(s) for s in segs])
    off = pad + np.concatenate([[0], np.cumsum(lens)])
    flat = np.concatenate([np.full(pad, 127)] + segs + [np.full(5, 127)]).astype(np.int64)
    d_off = torch.from_numpy(off.astype(np.int64)).to(dev)
    d_rows = torch.from_numpy(flat).to(dev)
    nnz = len(flat)
    need = lib.ebt_sub_exclusions_bytes(B, nnz)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    off_out = torch.full((B + 1,), -1, dtype=torch.int64, device=dev)
    rows_out = torch.full((nnz,), -7, dtype=torch.int64, device=dev)
    _lib.call("ebt_sub_exclusions", masks.table[mask].data_ptr(), masks.words,
              sub.rank.data_ptr(), n, d_off.data_ptr(), d_rows.data_ptr(), B, nnz,
              off_out.data_ptr(), rows_out.data_ptr(), ws.data_ptr(), need, _lib.stream_of(dev))
    want = []
    for s in segs:
        keep = s[np.isin(s, allowed)]
        want.append(np.searchsorted(allowed, keep))
    want_off = np.concatenate([[0], np.cumsum([len(w) for w in want])])
    assert np.array_equal(off_out.cpu().numpy(), want_off)
    total = int(want_off[-1])
    got = rows_out.cpu().numpy()
    assert np.array_equal(got[:total], np.concatenate(want))
    assert (got[total:] == -7).all()


def test_sub_rows_to_global(cuda_device):
    from robot_ebert_amd import _lib
    dev = cuda_device
    m = 37
    lst = torch.arange(1000, 1000 + 3 * m, 3, dtype=torch.int64, device=dev)
    src = [-1, 0, m - 1, m, -5, m + 100, 2 ** 40, 1]
    rows = torch.tensor(src * 70, dtype=torch.int64, device=dev)       # more than one workgroup
    _lib.call("ebt_sub_rows_to_global", rows.data_ptr(), rows.numel(), lst.data_ptr(), m,
              _lib.stream_of(dev))
    want = [-1, 1000, 1000 + 3 * (m - 1), -1, -1, -1, -1, 1003] * 70
    assert rows.cpu().tolist() == want


# ---- 4. end to end --------------------------------------------------------------------------------
def _ids(B):
    """The three materialised masks, the one that is not, and None, mixed in one batch."""
    return [[M_ONE, M_37, None, M_THIRD, M_HALF][b % 5] for b in range(B)]


def _liked(B, n):
    rng = np.random.default_rng(6)
    return [sorted(rng.choice(n, 1 + b % 4, replace=False).tolist()) for b in range(B)]


def _rated(B, n, liked):
    """Rated rows; a user's liked rows are among them, as in lib.py:47-48 (two liked rows of one
    user tie exactly, so they must not be candidates of a test that compares an order)."""
    out = [list(range(b % 50, n, 97)) for b in range(B)]
    if liked is not None:
        out = [sorted(set(e) | set(l)) for e, l in zip(out, liked)]
    return out


def _complement(rated, n, ids):
    out = []
    for e, m in zip(rated, ids):
        if m is None:
            out.append(sorted(e))
        else:
            out.append(sorted(set(e) | set(np.nonzero(~_flags(n)[m][:n])[0].tolist())))
    return out


def _check_routes(routes, ids, n):
    """Every materialised mask of the batch answered its own queries from its sub-catalog."""
    want = {m: [b for b, i in enumerate(ids) if i == m] for m in MATERIALISED}
    want = {m: q for m, q in want.items() if q}
    assert {m: q for m, q, _ in routes} == want
    for m, _, rows in routes:
        assert rows == int(_flags(n)[m][:n].sum())


@pytest.mark.parametrize("excl", [False, True], ids=["noexcl", "excl"])
@pytest.mark.parametrize("qkind", ["dense", "liked"])
@pytest.mark.parametrize("k", [1, 10, 100])
@pytest.mark.parametrize("B", [5, 130])
@pytest.mark.parametrize("kind", ["f32", "bf16"])
@pytest.mark.parametrize("n", SIZES)
def test_materialised_equals_mask_pass_and_oracle(cuda_device, n, kind, B, k, qkind, excl):
    import robot_ebert_amd as ebt
    dev = cuda_device
    cat, masks, plain = _setup(n, kind, dev)
    c = _host_catalog(n, kind)
    ids = _ids(B)
    d = KINDS[kind][1]
    liked = _liked(B, n) if qkind == "liked" else None
    if excl:
        rated = _rated(B, n, liked)
    else:   # bare for dense queries; a liked user's own rows tie exactly, so they stay excluded
        rated = [sorted(l) for l in liked] if liked is not None else None
    q = gaussian(2, B, d, "f32").astype(np.float32)
    kw = dict(liked=liked) if liked is not None else dict(queries=torch.from_numpy(q).to(dev))
    p = ebt.score_topk_submit(cat, k, exclude=rated, allow=(masks, ids), **kw)
    _check_routes(p.routes, ids, n)
    got = ebt.score_topk_finish(p)
    p0 = ebt.score_topk_submit(cat, k, exclude=rated, allow=(plain, ids), **kw)
    assert tuple(p0.routes) == ()
    _same(got, ebt.score_topk_finish(p0))
    # the float64 oracle over (allowed minus excluded), as tests/test_gpu_allow.py compares
    ex = _complement(rated if rated is not None else [[]] * B, n, ids)
    if liked is not None:
        s1, r1 = R.liked_topk(c, liked, k + 1, ex)
    else:
        s1, r1 = R.cosine_topk(q.astype(np.float64), c, k + 1, ex)
    both = r1[:, k] >= 0
    assert (s1[both, k - 1] > s1[both, k]).all()
    s_ref, r_ref = s1[:, :k], r1[:, :k]
    np.testing.assert_array_equal(got[1].cpu().numpy(), r_ref)
    ok = r_ref >= 0
    np.testing.assert_allclose(got[0].cpu().numpy()[ok], s_ref[ok], rtol=0, atol=ATOL)
    assert np.isnan(got[0].cpu().numpy()[~ok]).all()
    if k > 1:                                   # k > m: the one-row mask pads with NaN / -1
        r = got[1].cpu().numpy()
        for b, m in enumerate(ids):
            if m == M_ONE:
                assert (r[b, 1:] == -1).all()


@pytest.mark.parametrize("qkind", ["dense", "liked"])
def test_sub_catalog_takes_the_fused_screen(cuda_device, qkind):
    """A sub-catalog large enough for the fused screen (the parents above give copies of at most
    a few hundred rows, which run unfused): the copy is scored by the path an unfiltered catalog
    of its size takes, and the answer is still the mask pass's, bit for bit, and the oracle's."""
    import robot_ebert_amd as ebt
    from robot_ebert_amd import search
    dev = cuda_device
    n, d, B, k = 20000, 64, 130, 10
    c = gaussian(1, n, d, "f32")
    cat = ebt.Catalog(_t(c, "f32", dev))
    f = np.random.default_rng(8).random(n) < 0.3
    masks, plain = ebt.AllowMasks(cat, 1), ebt.AllowMasks(cat, 1)
    for m in (masks, plain):
        m.from_bool(0, torch.from_numpy(f).to(dev))
    assert masks.materialize(0) == int(f.sum())
    assert search.plan(masks._subs[0].catalog, 65, k)["fused"]
    ids = [0 if b % 2 == 0 else None for b in range(B)]
    liked = _liked(B, n) if qkind == "liked" else None
    rated = _rated(B, n, liked)
    q = gaussian(2, B, d, "f32").astype(np.float32)
    kw = dict(liked=liked) if liked is not None else dict(queries=torch.from_numpy(q).to(dev))
    p = ebt.score_topk_submit(cat, k, exclude=rated, allow=(masks, ids), **kw)
    assert p.routes == ((0, list(range(0, B, 2)), int(f.sum())),)
    got = ebt.score_topk_finish(p)
    _same(got, ebt.score_topk(cat, k, exclude=rated, allow=(plain, ids), **kw))
    gone = np.nonzero(~f)[0].tolist()
    ex = [sorted(set(e) | set(gone)) if i == 0 else sorted(e) for e, i in zip(rated, ids)]
    if liked is not None:
        s_ref, r_ref = R.liked_topk(c, liked, k, ex)
    else:
        s_ref, r_ref = R.cosine_topk(q.astype(np.float64), c, k, ex)
    np.testing.assert_array_equal(got[1].cpu().numpy(), r_ref)
    np.testing.assert_allclose(got[0].cpu().numpy(), s_ref, rtol=0, atol=ATOL)


def test_device_csr_inputs(cuda_device):
    """liked and exclude as device CSRs (what RecBatcher's stager passes) take the same routes."""
    import robot_ebert_amd as ebt
    from robot_ebert_amd import search
    dev = cuda_device
    n, B, k = 1000, 130, 10
    cat, masks, plain = _setup(n, "f32", dev)
    ids = _ids(B)
    liked = _liked(B, n)
    rated = _rated(B, n, liked)
    lc, ec = search.csr_from_lists(liked, dev), search.csr_from_lists(rated, dev)
    p = ebt.score_topk_submit(cat, k, liked=lc, exclude=ec, allow=(masks, ids))
    _check_routes(p.routes, ids, n)
    _same(ebt.score_topk_finish(p),
          ebt.score_topk(cat, k, liked=liked, exclude=rated, allow=(plain, ids)))
    # an unsorted caller's CSR of exclusions is sorted first, as on the usual path
    raw = (ec[0].clone(), torch.cat([torch.flip(ec[1][:int(ec[0][1])], [0]),
                                     ec[1][int(ec[0][1]):]]))
    q = torch.from_numpy(gaussian(2, B, 72, "f32").astype(np.float32)).to(dev)
    _same(ebt.score_topk(cat, k, queries=q, exclude=raw, allow=(masks, ids)),
          ebt.score_topk(cat, k, queries=q, exclude=rated, allow=(plain, ids)))


# ---- 5. edge cases --------------------------------------------------------------------------------
def test_empty_mask_device_ids_and_refusals(cuda_device):
    import robot_ebert_amd as ebt
    dev = cuda_device
    n, B, k = 333, 5, 10
    cat, masks, plain = _setup(n, "f32", dev)
    q = torch.from_numpy(gaussian(2, B, 72, "f32").astype(np.float32)).to(dev)
    # m = 0: nothing is built, the mask pass answers with NaN / -1 (bits at or above n only)
    empty = ebt.AllowMasks(cat, 2)
    f = np.zeros(32 * empty.words, bool)
    f[[n, n + 5]] = True
    empty.from_bool(0, torch.from_numpy(f).to(dev))
    assert empty.materialize(0) == 0 and empty.materialize(1) == 0 and empty.materialized() == {}
    p = ebt.score_topk_submit(cat, k, queries=q, allow=(empty, [0] * B))
    assert tuple(p.routes) == ()
    s, r = ebt.score_topk_finish(p)
    assert bool((r == -1).all()) and bool(torch.isnan(s).all())
    # a device tensor of ids keeps the mask pass: no routes, the same answer
    ids = _ids(B)
    d_ids = torch.tensor([-1 if i is None else i for i in ids], dtype=torch.int32, device=dev)
    p = ebt.score_topk_submit(cat, k, queries=q, allow=(masks, d_ids))
    assert tuple(p.routes) == ()
    _same(ebt.score_topk_finish(p), ebt.score_topk(cat, k, queries=q, allow=(masks, ids)))
    # refusals: masks of a bare row count, a row-sharded catalog
    with pytest.raises(ebt.EbertError, match="Catalog"):
        ebt.AllowMasks(n, 1, device=dev).materialize(0)
    shard = ebt.Catalog(_t(_host_catalog(n, "f32"), "f32", dev), row_offset=37, n_global=n + 100)
    sm = ebt.AllowMasks(shard, 1)
    sm.set(0, [40, 50])
    with pytest.raises(ebt.EbertError, match="shard"):
        sm.materialize(0)
    with pytest.raises(ebt.EbertError):
        masks.materialize(4)                                  # mask 4 of 4
    # dematerialize: back on the mask pass
    one = ebt.AllowMasks(cat, 1)
    one.from_bool(0, torch.from_numpy(_flags(n)[M_37]).to(dev))
    assert one.materialize(0) == 37 and one.materialized() == {0: (37, True)}
    assert ebt.score_topk_submit(cat, k, queries=q, allow=(one, [0] * B)).routes == (
        (0, list(range(B)), 37),)
    one.dematerialize(0)
    assert one.materialized() == {}
    assert tuple(ebt.score_topk_submit(cat, k, queries=q, allow=(one, [0] * B)).routes) == ()


@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_stale_views_are_never_used(cuda_device, kind):
    """set / update_rows / remove + apply_moves: each leaves the view gone or stale, the mask pass
    answers (equal to masks that were never materialised), and a renewed materialize is used."""
    import robot_ebert_amd as ebt
    dev = cuda_device
    n, B, k = 333, 130, 10
    dt, d = KINDS[kind]
    cat = ebt.Catalog(_t(_host_catalog(n, kind), dt, dev), capacity=n + 16)
    masks, plain = ebt.AllowMasks(cat, 2), ebt.AllowMasks(cat, 2)
    f = _flags(n)[M_THIRD][:n]
    for m in (masks, plain):
        m.from_bool(0, torch.from_numpy(f).to(dev))
        m.from_bool(1, torch.from_numpy(_flags(n)[M_37][:n]).to(dev))
    q = torch.from_numpy(gaussian(2, B, d, "f32").astype(np.float32)).to(dev)
    ids = [[0, 1, None][b % 3] for b in range(B)]
    rated = _rated(B, n, None)

    def run(ms):
        p = ebt.score_topk_submit(cat, k, queries=q, exclude=rated, allow=(ms, ids))
        return {m for m, _, _ in p.routes}, ebt.score_topk_finish(p)

    def both(expect):
        routes, got = run(masks)
        assert routes == expect
        _same(got, run(plain)[1])
        return got

    m0 = masks.materialize(0)
    masks.materialize(1)
    first = both({0, 1})
    # 1. set on mask 0: its view is gone, mask 1's is kept
    row = int(np.nonzero(f)[0][3])
    for m in (masks, plain):
        m.set(0, [row], False)
    assert masks.materialized() == {1: (37, True)}
    second = both({1})
    q0 = torch.tensor([b for b, i in enumerate(ids) if i == 0], device=dev)
    assert bool((first[1] >= 0).all()) and not bool((second[1][q0] == row).any())
    assert masks.materialize(0) == m0 - 1
    both({0, 1})
    # 2. update_rows on an allowed row: both views stale (kept, not used)
    row = int(np.nonzero(f)[0][5])
    cat.update_rows([row], _t(gaussian(77, 1, d, dt), dt, dev))
    assert masks.materialized() == {0: (m0 - 1, False), 1: (37, False)}
    both(set())
    masks.materialize(0)
    assert masks.materialized() == {0: (m0 - 1, True), 1: (37, False)}
    both({0})
    masks.materialize(1)
    # 3. remove + apply_moves: the views are dropped
    gone = sorted({0, 31, 32, 127, 128, n - 1, int(np.nonzero(f)[0][7])})
    moves = cat.remove(gone)
    assert moves
    for m in (masks, plain):
        m.apply_moves(moves, cat.n)
    assert masks.materialized() == {}
    rated = _rated(B, cat.n, None)
    both(set())
    masks.materialize(0)
    masks.materialize(1)
    got = both({0, 1})
    # and the oracle on the edited matrix and masks
    host = cat.data.float().cpu().numpy().astype(np.float64)
    allowed = [plain.to_bool(i, cat.n).cpu().numpy() for i in range(2)]
    ex = [sorted(set(e) | (set() if i is None else set(np.nonzero(~allowed[i])[0].tolist())))
          for e, i in zip(rated, ids)]
    s_ref, r_ref = R.cosine_topk(q.cpu().numpy().astype(np.float64), host, k, ex)
    np.testing.assert_array_equal(got[1].cpu().numpy(), r_ref)
    np.testing.assert_allclose(got[0].cpu().numpy(), s_ref, rtol=0, atol=ATOL)


def test_batcher_over_a_materialised_mask(cuda_device):
    """RecBatcher passes a host list of ids: its filtered requests are routed without a change,
    with the answers of masks that were never materialised."""
    import robot_ebert_amd as ebt
    from robot_ebert_amd.batcher import RecBatcher
    dev = cuda_device
    n, k = 1000, 10
    cat, masks, plain = _setup(n, "f32", dev)
    rng = np.random.default_rng(21)
    reqs = []
    for i in range(40):
        liked = sorted(rng.choice(n, 1 + i % 3, replace=False).tolist())
        rated = sorted(set(rng.choice(n, 20, replace=False).tolist()) | set(liked))
        reqs.append((liked, rated, k, [None, M_ONE, M_37, M_THIRD, M_HALF][i % 5]))
    seen = []

    def submit(*a, **kw):
        p = ebt.score_topk_submit(*a, **kw)
        seen.append(p.routes)
        return p

    b = RecBatcher(cat, max_batch=64, max_wait_ms=50.0, allow_masks=masks, submit_fn=submit)
    try:
        res = [f.result(timeout=60) for f in [b.submit(l, e, kk, allow=a)
                                              for l, e, kk, a in reqs]]
    finally:
        b.close()
    assert any(len(r) for r in seen), "no batch was answered from a sub-catalog"
    for (l, e, kk, a), (s, r) in zip(reqs, res):
        ws, wr = ebt.score_topk(cat, kk, liked=[l], exclude=[e],
                                allow=(plain, [-1 if a is None else a]))
        wr, ws = wr[0].cpu().numpy(), ws[0].cpu().numpy()
        keep = wr >= 0
        np.testing.assert_array_equal(r, wr[keep])
        assert np.array_equal(s.view(np.uint64), ws[keep].view(np.uint64))
        if a == M_ONE:
            assert len(r) <= 1
