"""GPU: explanations (include/ebert.h 0.9.0) -- the per-liked-row contributions to each score.

    contrib(b, j, l) = ( w_l * ( (x_{r_l} . x_j) / (g_{r_l} * g_j) ) ) * (1 / W_b)

The oracle is oracle.restatement: R.cosine_similarity(cat[liked], cat[rows]) times w / W (the
reference's pairwise_similarities restricted to the returned columns, lib.py:51-52 before the
.mean), on the catalog's values as stored (rounded to its dtype). Values are compared within the
project's SCORE_ATOL = 1e-12 (tests/test_gpu_weighted.py); the selection kernel and the
invariants are compared BITWISE. The top-m checks are tolerance-aware and need no gap condition:
the returned values are ordered, each equals the oracle at its position within SCORE_ATOL, and no
position left out is more than SCORE_ATOL better than the m-th returned.

Shapes: catalogs of 2,000 rows, batches of at most 8 queries; L crosses the 16-wide MFMA tiles and
the 96-row staging block (1, 15, 16, 17, 33, 300), k crosses the tiles (1, 10, 17, 100)."""
import ctypes

import numpy as np
import pytest
import torch

from inputs import c1_catalog, gaussian
from oracle import restatement as R

pytestmark = pytest.mark.gpu
SCORE_ATOL = 1e-12
N = 2000
ZERO_ROW = 3
LENS = (1, 15, 16, 17, 33, 300, 85, 2)
TORCH_DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16,
            "f64": torch.float64}


def _ebt():
    import robot_ebert_amd as ebt
    from robot_ebert_amd import _lib, explain
    return ebt, _lib, explain


def _t(x, dt, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev).to(TORCH_DT[dt])


def mixed_weights(rng, n):
    """n finite weights of both signs, none zero, magnitudes in [0.5, 5]."""
    w = rng.uniform(0.5, 5.0, n) * rng.choice([-1.0, 1.0], n)
    if n > 1:
        w[0], w[1] = abs(w[0]), -abs(w[1])
    return w


def make_batch(seed, k, n=N, lens=LENS, row_offset=0):
    """(liked lists, weights, rows [B, k]) as GLOBAL rows: lists with duplicates, the zero-norm
    row as a liked row (query 2) and as a result row (query 1), -1 result slots (queries 0, 3)."""
    rng = np.random.default_rng(seed)
    liked = [rng.integers(0, n, size=L) for L in lens]        # with replacement: duplicates
    liked[2][0] = ZERO_ROW
    if len(lens) > 4:
        liked[4][:3] = liked[4][3]                            # one row four times
    rows = np.stack([rng.choice(n, size=k, replace=False) for _ in lens]).astype(np.int64)
    rows[1, 0] = ZERO_ROW
    rows += row_offset
    if k >= 2:
        rows[0, k // 2] = -1
        rows[3, k - 1] = -1
    w = [mixed_weights(rng, L) for L in lens]
    return [(l + row_offset).tolist() for l in liked], [x.tolist() for x in w], rows


def oracle_contrib(cat64, liked, w, rows, row_offset=0):
    """[k, L] float64: R.cosine_similarity(cat[liked], cat[rows]) times w / W; NaN rows for -1."""
    liked = np.asarray(liked, dtype=np.int64) - row_offset
    rows = np.asarray(rows, dtype=np.int64)
    w = np.ones(len(liked)) if w is None else np.asarray(w, dtype=np.float64)
    C = np.full((len(rows), len(liked)), np.nan)
    ok = rows >= 0
    S = R.cosine_similarity(cat64[liked], cat64[rows[ok] - row_offset])   # [L, k_valid]
    C[ok] = ((w[:, None] * S) / np.abs(w).sum()).T
    return C


def device_blocks(out, off, k):
    """The CSR-shaped matrix as one [k, L_b] numpy array per query."""
    o, off = out.cpu().numpy(), off.cpu().numpy()
    return [o[k * off[b]:k * off[b + 1]].reshape(k, off[b + 1] - off[b])
            for b in range(len(off) - 1)]


def check_matrix(explain, cat, cat64, liked, w, rows, dev, row_offset=0):
    out, status, off, _ = explain.liked_contrib(cat, torch.from_numpy(rows).to(dev), liked, w)
    assert status.cpu().tolist() == [1] * len(liked)
    k = rows.shape[1]
    for b, got in enumerate(device_blocks(out, off, k)):
        want = oracle_contrib(cat64, liked[b], None if w is None else w[b], rows[b], row_offset)
        empty = rows[b] < 0
        assert np.isnan(got[empty]).all(), b
        err = np.abs(got[~empty] - want[~empty])
        print(f"query {b}: L={len(liked[b])} k={k} max |err| = {err.max() if err.size else 0:.3e}")
        np.testing.assert_allclose(got[~empty], want[~empty], rtol=0, atol=SCORE_ATOL)
        # a zero-norm row contributes exactly 0, as a liked row and as a result row
        lz = np.asarray(liked[b]) - row_offset == ZERO_ROW
        rz = rows[b] - row_offset == ZERO_ROW
        assert (got[~empty][:, lz] == 0.0).all() and (got[rz & ~empty] == 0.0).all(), b
    return out, off


def check_topm(val, pos, C, m, largest=True):
    """The tolerance-aware top-m rule for one (b, j) segment: val / pos [m], C [L] the oracle."""
    L = len(C)
    n = min(m, L)
    assert (pos[:n] >= 0).all() and (pos[n:] == -1).all() and np.isnan(val[n:]).all()
    assert len(set(pos[:n].tolist())) == n
    sgn = 1.0 if largest else -1.0
    for t in range(1, n):   # ordered by (value, position)
        a, b = sgn * val[t - 1], sgn * val[t]
        assert a > b or (a == b and pos[t - 1] < pos[t]), (val, pos)
    np.testing.assert_allclose(val[:n], C[pos[:n]], rtol=0, atol=SCORE_ATOL)
    if n < L:
        rest = np.ones(L, dtype=bool)
        rest[pos[:n]] = False
        assert (sgn * C[rest]).max() <= sgn * val[n - 1] + SCORE_ATOL, (val, pos)


@pytest.fixture(scope="module")
def catalogs(cuda_device):
    """One 2,000-row catalog per (dtype, d), row 3 zero; built on first use."""
    ebt, _, _ = _ebt()
    made = {}

    def get(dt, d):
        if (dt, d) not in made:
            x = gaussian(91, N, d, dt)
            x[ZERO_ROW] = 0.0
            xt = _t(x, dt, cuda_device)
            made[dt, d] = (ebt.Catalog(xt), xt.to(torch.float64).cpu().numpy())
        return made[dt, d]
    return get


# ----------------------------------------------------------- 1. the matrix against the oracle ----
@pytest.mark.parametrize("dt", ["f32", "bf16", "f16", "f64"])
@pytest.mark.parametrize("d", [32, 77, 768, 1536])
def test_contrib_matrix_matches_oracle(cuda_device, catalogs, dt, d):
    """Every dtype and d (77: the element path, no row is 16-byte aligned), L in 1 .. 300, k in
    1 .. 100, duplicates, mixed-sign weights, the zero-norm row on both sides, -1 slots."""
    _, _, explain = _ebt()
    cat, cat64 = catalogs(dt, d)
    for k in (1, 10, 17, 100):
        liked, w, rows = make_batch(100 + k, k)
        check_matrix(explain, cat, cat64, liked, w, rows, cuda_device)
    liked, _, rows = make_batch(7, 17)
    check_matrix(explain, cat, cat64, liked, None, rows, cuda_device)      # unweighted


@pytest.mark.parametrize("dt,d,ld", [("f32", 768, 772), ("f32", 768, 771), ("bf16", 77, 80),
                                     ("f64", 32, 33)])
def test_contrib_matrix_padded_rows_and_row_offset(cuda_device, dt, d, ld):
    """A padded ld > d (772 floats: 16-byte rows, the chunk path; 771: the element path) whose
    padding holds NaN (never read into a product), on a catalog with row_offset = 5000: the same
    oracle, and -- given the same norms -- bitwise the matrix of the same values stored densely
    at row_offset 0."""
    ebt, _, explain = _ebt()
    dev = cuda_device
    x = gaussian(92, N, d, dt)
    x[ZERO_ROW] = 0.0
    dense = _t(x, dt, dev)
    big = torch.full((N, ld), float("nan"), dtype=dense.dtype, device=dev)
    big[:, :d] = dense
    cat = ebt.Catalog(big[:, :d], row_offset=5000)
    assert cat.ld == ld and cat.row_offset == 5000
    cat64 = dense.to(torch.float64).cpu().numpy()
    liked, w, rows = make_batch(11, 17, row_offset=5000)
    out, off = check_matrix(explain, cat, cat64, liked, w, rows, dev, row_offset=5000)
    cat0 = ebt.Catalog(dense)
    liked0 = [[r - 5000 for r in l] for l in liked]
    rows0 = np.where(rows >= 0, rows - 5000, -1)
    out0, _, _, _ = explain.liked_contrib(cat0, torch.from_numpy(rows0).to(dev), liked0, w)
    # (ebt_row_norms adds a row's squares in another order when its rows are not 16-byte
    # aligned, so the two catalogs' norms may differ in the last bit: with the dense catalog's
    # norms in place, the element path stages the same values and gives the same bits)
    cat.gnorm.copy_(cat0.gnorm)
    out, _, _, _ = explain.liked_contrib(cat, torch.from_numpy(rows).to(dev), liked, w)
    assert out.cpu().numpy().tobytes() == out0.cpu().numpy().tobytes()


# ------------------------------------------------------------------------------ 2. sum rule ----
@pytest.fixture(scope="module")
def wide(cuda_device):
    """2,000 x 768 f32, 8 users with 1 .. 300 liked rows (duplicates), weights, exclusions."""
    ebt, _, _ = _ebt()
    c = gaussian(71, N, 768, "f32")
    cat = ebt.Catalog(_t(c, "f32", cuda_device))
    rng = np.random.default_rng(72)
    liked = [rng.integers(0, N, size=m).tolist() for m in LENS]
    w = [mixed_weights(rng, m).tolist() for m in LENS]
    excl = [sorted(set(rng.choice(N, 25, replace=False).tolist())) for _ in LENS]
    return cat, c.astype(np.float64), liked, w, excl


@pytest.mark.parametrize("case", ["unweighted", "weighted", "excluded", "materialised"])
def test_totals_equal_the_scores(cuda_device, wide, case):
    """total[b, j] = the sum of all L_b contributions = the score score_topk returned for that
    row, within SCORE_ATOL; empty slots (k beyond the allowed rows) are NaN on both sides."""
    ebt, _, _ = _ebt()
    cat, _, liked, w, excl = wide
    k = 17
    kw = {}
    if case != "unweighted":
        kw["liked_weights"] = w
    if case in ("excluded", "materialised"):
        kw["exclude"] = excl
    if case == "materialised":
        masks = ebt.AllowMasks(cat, 1)
        masks.set(0, [r for r in range(N) if r % 150 == 1])      # 14 rows: some slots stay empty
        assert masks.materialize(0) == 14
        p = ebt.score_topk_submit(cat, k, liked=liked, allow=(masks, [0] * 7 + [-1]), **kw)
        assert [rt[0] for rt in p.routes] == [0]
        scores, rows = ebt.score_topk_finish(p)
        assert bool((rows[:7, 14:] == -1).all())
    else:
        scores, rows = ebt.score_topk(cat, k, liked=liked, **kw)
    ex = ebt.explain_topk(cat, rows, liked, liked_weights=kw.get("liked_weights"), m=3)
    assert tuple(ex.total.shape) == (8, k) and tuple(ex.contrib.shape) == (8, k, 3)
    s, t, r = scores.cpu().numpy(), ex.total.cpu().numpy(), rows.cpu().numpy()
    assert np.isnan(t[r < 0]).all() and np.isnan(s[r < 0]).all()
    print(case, "max |total - score| =", np.abs(t[r >= 0] - s[r >= 0]).max())
    np.testing.assert_allclose(t[r >= 0], s[r >= 0], rtol=0, atol=SCORE_ATOL)


# ------------------------------------------------------------------- 3. selection, bitwise ----
def _numpy_select(block, lrows, m, largest):
    """(val [k, m], pos, row, total [k]) of one query's [k, L] block: numpy lexsort by (value,
    position) and a sequential Python sum in list order."""
    k, L = block.shape
    val = np.full((k, m), np.nan)
    pos = np.full((k, m), -1, dtype=np.int32)
    row = np.full((k, m), -1, dtype=np.int64)
    tot = np.zeros(k)
    for j in range(k):
        v = block[j]
        keep = np.flatnonzero(~np.isnan(v))                 # a NaN is never selected
        order = keep[np.lexsort((keep, -v[keep] if largest else v[keep]))][:m]
        n = len(order)
        val[j, :n], pos[j, :n], row[j, :n] = v[order], order, lrows[order]
        acc = 0.0
        for x in v.tolist():
            acc += x
        tot[j] = acc
    return val, pos, row, tot


@pytest.mark.parametrize("m", [1, 3, 64])
@pytest.mark.parametrize("largest", [True, False])
def test_select_bitwise_on_a_hand_made_matrix(cuda_device, m, largest):
    """ebt_explain_select against numpy: exact ties (values on a 0.25 grid), -0.0 beside +0.0,
    negative values, L_b < m, L_b = 1, L_b = 300, a NaN segment and NaN entries."""
    _, _, explain = _ebt()
    dev = cuda_device
    rng = np.random.default_rng(31)
    lens, k = [1, 2, 300, 17, 64, 65], 5
    off = np.zeros(len(lens) + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    lrows = rng.integers(0, 10 ** 12, size=off[-1])
    blocks = []
    for L in lens:
        b = np.round(rng.standard_normal((k, L)) * 4) / 4      # many exact ties
        b[1] = np.round(rng.standard_normal(L), 3) * 1e-3      # few ties, tiny values
        b[2] = -np.abs(b[2]) - 0.25                            # all negative
        b[3, ::2] = 0.0
        b[3, 1::2] = -0.0                                      # one value: position decides
        blocks.append(b)
    blocks[2][4, :] = np.nan                                   # an empty result slot
    blocks[3][0, 5] = np.nan                                   # a stray NaN is skipped
    flat = np.concatenate([b.ravel() for b in blocks])
    val, pos, row, tot = explain.explain_select(
        torch.from_numpy(flat).to(dev), torch.from_numpy(off).to(dev),
        torch.from_numpy(lrows).to(dev), k, m=m, largest=largest)
    for b, blk in enumerate(blocks):
        wv, wp, wr, wt = _numpy_select(blk, lrows[off[b]:off[b + 1]], m, largest)
        assert val[b].cpu().numpy().tobytes() == wv.tobytes(), b
        assert np.array_equal(pos[b].cpu().numpy(), wp), b
        assert np.array_equal(row[b].cpu().numpy(), wr), b
        assert tot[b].cpu().numpy().tobytes() == wt.tobytes(), b
    assert pos.dtype == torch.int32 and row.dtype == torch.int64
    # out_total == NULL: the same selection
    v2, p2, _, t2 = explain.explain_select(
        torch.from_numpy(flat).to(dev), torch.from_numpy(off).to(dev),
        torch.from_numpy(lrows).to(dev), k, m=m, largest=largest, total=False)
    assert t2 is None and torch.equal(p2, pos)


# ------------------------------------------------------- 4. top-m end to end, tolerance-aware ----
@pytest.mark.parametrize("dt,d", [("f32", 768), ("bf16", 77), ("f64", 1536)])
@pytest.mark.parametrize("weighted", [False, True])
def test_explain_topk_end_to_end(cuda_device, catalogs, dt, d, weighted):
    ebt, _, _ = _ebt()
    cat, cat64 = catalogs(dt, d)
    for k, m in ((10, 3), (100, 1), (17, 64)):
        liked, w, rows = make_batch(200 + k, k)
        w = w if weighted else None
        rt = torch.from_numpy(rows).to(cuda_device)
        for largest in (True, False):
            ex = ebt.explain_topk(cat, rt, liked, liked_weights=w, m=m, largest=largest)
            val, pos, lr = (x.cpu().numpy() for x in (ex.contrib, ex.pos, ex.liked_row))
            tot = ex.total.cpu().numpy()
            for b in range(len(liked)):
                C = oracle_contrib(cat64, liked[b], None if w is None else w[b], rows[b])
                for j in range(k):
                    if rows[b, j] < 0:
                        assert np.isnan(val[b, j]).all() and (pos[b, j] == -1).all()
                        assert (lr[b, j] == -1).all() and np.isnan(tot[b, j])
                        continue
                    check_topm(val[b, j], pos[b, j], C[j], m, largest)
                    n = min(m, len(liked[b]))
                    assert lr[b, j, :n].tolist() == [liked[b][p] for p in pos[b, j, :n]]
                    assert abs(tot[b, j] - C[j].sum()) <= SCORE_ATOL


# ------------------------------------------------------------------- 5. invariants, bitwise ----
def _bits(ex):
    return tuple(x.cpu().numpy().tobytes() for x in ex)


def test_invariants_bitwise(cuda_device, catalogs):
    ebt, _, explain = _ebt()
    dev = cuda_device
    cat, _ = catalogs("f32", 768)
    k, m = 17, 3
    liked, w, rows = make_batch(301, k)
    rt = torch.from_numpy(rows).to(dev)
    base = ebt.explain_topk(cat, rt, liked, liked_weights=w, m=m)
    # the same call twice
    assert _bits(ebt.explain_topk(cat, rt, liked, liked_weights=w, m=m)) == _bits(base)
    # query b alone == query b inside the batch of 8 (matrix and selection)
    out, _, off, _ = explain.liked_contrib(cat, rt, liked, w)
    blocks = device_blocks(out, off, k)
    for b in range(len(liked)):
        one = ebt.explain_topk(cat, rt[b:b + 1], [liked[b]], liked_weights=[w[b]], m=m)
        assert _bits(one) == tuple(x[b:b + 1].cpu().numpy().tobytes() for x in base), b
        o1, _, off1, _ = explain.liked_contrib(cat, rt[b:b + 1], [liked[b]], [w[b]])
        assert device_blocks(o1, off1, k)[0].tobytes() == blocks[b].tobytes(), b
    # weights of 1.0 == liked_w NULL
    ones = [[1.0] * len(l) for l in liked]
    assert _bits(ebt.explain_topk(cat, rt, liked, liked_weights=ones, m=m)) == \
        _bits(ebt.explain_topk(cat, rt, liked, m=m))
    o_1, _, _, _ = explain.liked_contrib(cat, rt, liked, ones)
    o_n, _, _, _ = explain.liked_contrib(cat, rt, liked, None)
    assert o_1.cpu().numpy().tobytes() == o_n.cpu().numpy().tobytes()
    # weights x 4 == weights
    w4 = [[4.0 * x for x in l] for l in w]
    assert _bits(ebt.explain_topk(cat, rt, liked, liked_weights=w4, m=m)) == _bits(base)
    # a device CSR with device weights == host lists
    off_t = torch.from_numpy(np.cumsum([0] + [len(l) for l in liked])).to(dev)
    lr_t = torch.tensor(sum(liked, []), dtype=torch.int64, device=dev)
    w_t = torch.tensor(sum(w, []), dtype=torch.float64, device=dev)
    assert _bits(ebt.explain_topk(cat, rt, (off_t, lr_t), liked_weights=w_t, m=m)) == _bits(base)
    # largest = 0: the other end of the SAME matrix
    small = ebt.explain_topk(cat, rt, liked, liked_weights=w, m=m, largest=False)
    assert small.total.cpu().numpy().tobytes() == base.total.cpu().numpy().tobytes()
    for b, blk in enumerate(blocks):
        lr = np.asarray(liked[b], dtype=np.int64)
        for largest, ex in ((True, base), (False, small)):
            wv, wp, wr, _ = _numpy_select(blk, lr, m, largest)
            assert ex.contrib[b].cpu().numpy().tobytes() == wv.tobytes(), (b, largest)
            assert np.array_equal(ex.pos[b].cpu().numpy(), wp)
            assert np.array_equal(ex.liked_row[b].cpu().numpy(), wr)


# -------------------------------------------------------------------------- 6. corrupt input ----
def _raw_topk(L, cat, rows, liked, w, m, dev):
    """ebt_explain_topk through _lib.call with NaN / -9 pre-filled outputs: (val, pos, row, total,
    status) as numpy, whatever the status says."""
    off = torch.from_numpy(np.cumsum([0] + [len(l) for l in liked])).to(dev)
    lr = torch.tensor(sum(liked, []), dtype=torch.int64, device=dev)
    wt = torch.tensor(sum(w, []), dtype=torch.float64, device=dev)
    B, k = rows.shape
    nnz = int(lr.numel())
    need = L.load().ebt_explain_workspace_bytes(nnz, k)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    val = torch.full((B, k, m), 7.0, dtype=torch.float64, device=dev)
    pos = torch.full((B, k, m), -9, dtype=torch.int32, device=dev)
    row = torch.full((B, k, m), -9, dtype=torch.int64, device=dev)
    tot = torch.full((B, k), 7.0, dtype=torch.float64, device=dev)
    status = torch.full((B,), -9, dtype=torch.int32, device=dev)
    rt = torch.from_numpy(rows).to(dev)
    L.call("ebt_explain_topk", ctypes.byref(cat.cstruct), B, L.ptr(off), L.ptr(lr), L.ptr(wt), nnz,
           L.ptr(rt), k, m, 1, L.ptr(ws), need, L.ptr(val), L.ptr(pos), L.ptr(row), L.ptr(tot),
           L.ptr(status), L.stream_of(dev))
    return tuple(x.cpu().numpy() for x in (val, pos, row, tot, status))


@pytest.mark.parametrize("where", ["liked_high", "liked_negative", "result_high", "result_low"])
def test_row_outside_the_catalog(cuda_device, where):
    """A liked or result row outside [row_offset, row_offset + n) gives status -2 and NaN / -1 for
    that query only; its neighbours are bit-equal to a clean batch; explain_topk raises naming the
    query. (That nothing out of range is read is a property of the kernel's guards -- the rows of a
    query are range-checked before any is followed, csrc/explain.hip -- not something a test can
    show; the catalog here sits at row_offset 1000 so that "below" is a non-negative row.)"""
    ebt, L, _ = _ebt()
    dev = cuda_device
    x = gaussian(93, N, 96, "f32")
    cat = ebt.Catalog(_t(x, "f32", dev), row_offset=1000)
    k, m, q = 10, 3, 2
    liked, w, rows = make_batch(401, k, lens=(5, 33, 17, 100), row_offset=1000)
    clean = _raw_topk(L, cat, rows, liked, w, m, dev)
    assert clean[4].tolist() == [1, 1, 1, 1]
    bad_liked, bad_rows = [list(l) for l in liked], rows.copy()
    if where == "liked_high":
        bad_liked[q][7] = 1000 + N
    elif where == "liked_negative":
        bad_liked[q][0] = -7
    elif where == "result_high":
        bad_rows[q, 4] = 1000 + N + 123456789
    else:
        bad_rows[q, 0] = 999            # a row of another shard: below row_offset
    got = _raw_topk(L, cat, bad_rows, bad_liked, w, m, dev)
    assert got[4].tolist() == [1, 1, -2, 1]
    assert np.isnan(got[0][q]).all() and (got[1][q] == -1).all() and (got[2][q] == -1).all()
    assert np.isnan(got[3][q]).all()
    for b in (0, 1, 3):
        for a, c in zip(got[:4], clean[:4]):
            assert a[b].tobytes() == c[b].tobytes(), b
    with pytest.raises(ebt.EbertError, match=f"query {q}"):
        ebt.explain_topk(cat, torch.from_numpy(bad_rows).to(dev), bad_liked, liked_weights=w, m=m)
    ex = ebt.explain_topk(cat, torch.from_numpy(rows).to(dev), liked, liked_weights=w, m=m)
    assert ex.contrib.cpu().numpy().tobytes() == clean[0].tobytes()       # and it still works


# ------------------------------------------------- 7. lib.get_user_recs_explained on C1 inputs ----
def test_get_user_recs_explained_c1(cuda_device):
    """The C1 catalog and users (inputs.c1_catalog, the ratings of c1_users as the golden file
    holds them): movies and scores identical to get_user_recs, each item's reasons the oracle's
    top 3 under the tolerance-aware rule, [] without ratings, sklearn's ValueError without a liked
    movie."""
    from test_gpu_parity import _collab_setup
    lib, gold = _collab_setup(cuda_device)
    ids, cat_np = c1_catalog()
    pos = {t: i for i, t in enumerate(ids)}
    k, m = 10, 3
    seen = 0
    for uid, rec in gold["users"].items():
        want = rec[f"k{k}"]
        if isinstance(want, dict):
            with pytest.raises(ValueError) as ei:
                lib.get_user_recs_explained(uid, k, m)
            assert str(ei.value) == want["message"]
            continue
        got = lib.get_user_recs_explained(uid, k, m)
        plain = lib.get_user_recs(uid, k)
        assert [(g.movie.tmdb_id, g.score) for g in got] == \
            [(p.movie.tmdb_id, p.score) for p in plain], uid
        assert [g.movie.tmdb_id for g in got] == [x[0] for x in want], uid
        if not rec["ratings"]:
            assert got == []
            continue
        rating = {t: r for t, r in rec["ratings"] if t in pos}
        liked_ids = [t for t, r in rating.items() if r >= lib.LIKED_MOVIE_SCORE]
        S = R.cosine_similarity(cat_np[[pos[t] for t in liked_ids]],
                                cat_np[[pos[g.movie.tmdb_id] for g in got]]) / len(liked_ids)
        for j, g in enumerate(got):
            C = dict(zip(liked_ids, S[:, j]))
            n = min(m, len(liked_ids))
            assert len(g.reasons) == n and len({r.tmdb_id for r in g.reasons}) == n
            vals = [r.contribution for r in g.reasons]
            assert all(a >= b for a, b in zip(vals, vals[1:]))
            for r in g.reasons:
                assert abs(r.contribution - C[r.tmdb_id]) <= SCORE_ATOL
                assert r.rating == rating[r.tmdb_id] and r.rating >= lib.LIKED_MOVIE_SCORE
            left = [v for t, v in C.items() if t not in {r.tmdb_id for r in g.reasons}]
            assert not left or max(left) <= vals[-1] + SCORE_ATOL
            assert abs(sum(C.values()) - g.score) <= SCORE_ATOL
        seen += 1
    assert seen >= 15
    # a weighting: the same movies and scores as get_user_recs(weighting=), reasons in order
    got = lib.get_user_recs_explained("u05", k, m, weighting=lib.weight_centered)
    plain = lib.get_user_recs("u05", k, weighting=lib.weight_centered)
    assert [(g.movie.tmdb_id, g.score) for g in got] == [(p.movie.tmdb_id, p.score) for p in plain]
    rating = dict(gold["users"]["u05"]["ratings"])
    for g in got:
        vals = [r.contribution for r in g.reasons]
        assert len(vals) == m and all(a >= b for a, b in zip(vals, vals[1:]))
        assert all(r.rating == rating[r.tmdb_id] for r in g.reasons)
