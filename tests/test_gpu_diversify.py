"""GPU: diversified top-k (include/ebert.h 0.10.0) -- greedy MMR re-ranking of a candidate pool.

    S(b, i, j) = (x_i . x_j) / (g_i * g_j)
    v_i = (lam * rel_i) - ((1 - lam) * max over the picks so far of S(b, s, i))

The oracle for S and rel is oracle.restatement.cosine_similarity on the catalog's values as stored
(rounded to its dtype); the greedy restatement is tests/mmr_ref.py. Values are compared within the
project's SCORE_ATOL = 1e-12 (tests/test_gpu_weighted.py); the selection kernel and the invariants
of the matrix are compared BITWISE. The end-to-end checks are tolerance-aware and need no gap
condition: |dv| <= lam |d rel| + (1 - lam) |d pen| <= 1e-12 per value, and two values are
compared, so no unpicked candidate's oracle value may exceed the chosen one's by more than 2e-12.
Equality with the oracle's own greedy is asserted where the oracle's gaps decide it (> 1e-9).

Shapes: catalogs of 2,000 rows, batches of 8 queries; p crosses the 16-wide MFMA tile, the 64-lane
wave of the selection and the 128-slot workgroup tile (1, 15, 16, 17, 63, 64, 65, 100, 129, 512)."""
import ctypes

import numpy as np
import pytest
import torch

from inputs import c1_catalog, gaussian
from mmr_ref import mmr_ref
from oracle import restatement as R

pytestmark = pytest.mark.gpu
SCORE_ATOL = 1e-12
N = 2000
ZERO_ROW = 3
LENS = (1, 15, 16, 17, 33, 300, 85, 2)
POOLS = (1, 15, 16, 17, 63, 64, 65, 100, 129, 512)
TORCH_DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16,
            "f64": torch.float64}


def _ebt():
    import robot_ebert_amd as ebt
    from robot_ebert_amd import _lib, diversify
    return ebt, _lib, diversify


def _t(x, dt, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev).to(TORCH_DT[dt])


def liked_lists(n=N):
    rng = np.random.default_rng(7)
    return [rng.choice(n, size=L, replace=False).tolist() for L in LENS]


def bits(x):
    return (x.cpu().numpy() if isinstance(x, torch.Tensor) else np.ascontiguousarray(x)).tobytes()


@pytest.fixture(scope="module")
def catalogs(cuda_device):
    """One 2,000-row catalog per (dtype, d), row 3 zero, with the oracle's whole similarity matrix
    (R.cosine_similarity of the stored values, computed once) and the GPU's top 512 of the eight
    liked lists; built on first use, the last three kept."""
    ebt, _, _ = _ebt()
    made = {}

    def get(dt, d):
        if (dt, d) not in made:
            while len(made) >= 3:
                made.pop(next(iter(made)))
            x = gaussian(91, N, d, dt)
            x[ZERO_ROW] = 0.0
            xt = _t(x, dt, cuda_device)
            cat = ebt.Catalog(xt)
            cat64 = xt.to(torch.float64).cpu().numpy()
            S = R.cosine_similarity(cat64, cat64)
            scores, rows = ebt.score_topk(cat, max(POOLS), liked=liked_lists())
            made[dt, d] = (cat, S, scores, rows)
        return made[dt, d]
    return get


def oracle_rel(S, liked, rows):
    """The oracle's relevance of the pool rows: the mean cosine to the liked rows (lib.py:51-52);
    NaN for an empty slot."""
    rel = np.full(len(rows), np.nan)
    ok = rows >= 0
    rel[ok] = S[np.asarray(liked)][:, rows[ok]].mean(axis=0)
    return rel


def oracle_gram(S, rows):
    G = np.full((len(rows), len(rows)), np.nan)
    ok = rows >= 0
    G[np.ix_(ok, ok)] = S[np.ix_(rows[ok], rows[ok])]
    return G


def make_pool(scores, rows, p):
    """The first p of a score_topk result (its own top p) with one -1 slot (query 0) and the
    zero-norm row forced in (query 1)."""
    r = rows[:, :p].cpu().numpy().copy()
    s = scores[:, :p].cpu().numpy().copy()
    r[0, p // 2], s[0, p // 2] = -1, np.nan
    if ZERO_ROW not in r[1]:
        r[1, 0], s[1, 0] = ZERO_ROW, 0.0
    return s, r


def check_gram(got, S, rows, row_offset=0):
    """One query's [p, p] matrix against the oracle; returns the largest error."""
    empty = rows < 0
    local = np.where(empty, -1, rows - row_offset)
    want = oracle_gram(S, local)
    nan = empty[:, None] | empty[None, :]
    assert np.array_equal(np.isnan(got), nan)
    err = np.abs(got[~nan] - want[~nan])
    np.testing.assert_allclose(got[~nan], want[~nan], rtol=0, atol=SCORE_ATOL)
    z = local == ZERO_ROW
    assert (got[z][:, ~empty] == 0.0).all() and (got[:, z][~empty] == 0.0).all()
    assert got.tobytes() == np.ascontiguousarray(got.T).tobytes()          # bitwise symmetric
    return err.max() if err.size else 0.0


# -------------------------------------------------------------- 1. the matrix against the oracle ----
@pytest.mark.parametrize("dt", ["f32", "bf16", "f16", "f64"])
@pytest.mark.parametrize("d", [32, 77, 768, 1536])
def test_gram_matches_oracle(cuda_device, catalogs, dt, d):
    """Every dtype and d (77: the element path, no row is 16-byte aligned) at every pool size:
    within SCORE_ATOL of the oracle, NaN exactly on empty slots, exactly 0 on the zero-norm row,
    bitwise symmetric, bitwise the same alone as in the batch, bitwise permuted by a permutation
    of the pool."""
    _, _, dv = _ebt()
    dev = cuda_device
    cat, S, scores, rows = catalogs(dt, d)
    rng = np.random.default_rng(5)
    worst = 0.0
    for p in POOLS:
        _, r = make_pool(scores, rows, p)
        rt = torch.from_numpy(r).to(dev)
        gram, status = dv.pool_gram(cat, rt)
        assert status.cpu().tolist() == [1] * len(LENS) and tuple(gram.shape) == (len(LENS), p, p)
        g = gram.cpu().numpy()
        for b in range(len(LENS)):
            worst = max(worst, check_gram(g[b], S, r[b]))
        for b in (0, 1, 5):
            one, st = dv.pool_gram(cat, rt[b:b + 1])
            assert st.cpu().tolist() == [1] and bits(one[0]) == g[b].tobytes(), (p, b)
        perm = rng.permutation(p)
        permuted, _ = dv.pool_gram(cat, torch.from_numpy(np.ascontiguousarray(r[:, perm])).to(dev))
        assert bits(permuted) == np.ascontiguousarray(g[:, perm][:, :, perm]).tobytes(), p
    print(f"{dt} d={d}: max |S - oracle| = {worst:.3e} over p in {POOLS}")


@pytest.mark.parametrize("dt,d,ld", [("f32", 768, 772), ("f32", 768, 771), ("bf16", 77, 80)])
def test_gram_row_offset_padded_rows_and_rows_outside(cuda_device, dt, d, ld):
    """A catalog at row_offset 5000 with a padded ld > d whose padding holds NaN (772 floats: the
    chunk path, 771: the element path): the oracle's matrix, and -- given the same norms --
    bitwise the matrix of the same values stored densely at row_offset 0. A pool row outside
    [row_offset, row_offset + n) gives status -2 and NaN for that query only."""
    ebt, L, dv = _ebt()
    dev = cuda_device
    x = gaussian(92, N, d, dt)
    x[ZERO_ROW] = 0.0
    dense = _t(x, dt, dev)
    big = torch.full((N, ld), float("nan"), dtype=dense.dtype, device=dev)
    big[:, :d] = dense
    cat = ebt.Catalog(big[:, :d], row_offset=5000)
    cat0 = ebt.Catalog(dense)
    assert cat.ld == ld and cat.row_offset == 5000
    cat.gnorm.copy_(cat0.gnorm)       # (ebt_row_norms may differ in the last bit on unaligned rows)
    cat64 = dense.to(torch.float64).cpu().numpy()
    S = R.cosine_similarity(cat64, cat64)
    rng = np.random.default_rng(11)
    p = 100
    r0 = np.stack([rng.choice(N, size=p, replace=False) for _ in range(4)]).astype(np.int64)
    r0[1, 0], r0[0, 7] = ZERO_ROW, -1
    r = np.where(r0 >= 0, r0 + 5000, -1)
    gram, status = dv.pool_gram(cat, torch.from_numpy(r).to(dev))
    assert status.cpu().tolist() == [1, 1, 1, 1]
    g = gram.cpu().numpy()
    for b in range(4):
        check_gram(g[b], S, r[b], row_offset=5000)
    gram0, _ = dv.pool_gram(cat0, torch.from_numpy(r0).to(dev))
    assert bits(gram0) == g.tobytes()
    rel = torch.from_numpy(rng.standard_normal((4, p))).to(dev)
    clean = dv.diversify_topk(cat, rel, torch.from_numpy(r).to(dev), 10, lam=0.5)
    for q, where, bad_row in ((2, 4, 5000 + N), (1, 0, 4999), (3, p - 1, -7),
                              (0, 50, 5000 + N + 123456789)):
        bad = r.copy()
        bad[q, where] = bad_row
        bt = torch.from_numpy(bad).to(dev)
        gram, status = dv.pool_gram(cat, bt)
        want = [1, 1, 1, 1]
        want[q] = -2
        assert status.cpu().tolist() == want
        gb = gram.cpu().numpy()
        assert np.isnan(gb[q]).all()
        for b in range(4):
            assert b == q or gb[b].tobytes() == g[b].tobytes(), (q, b)
        # ebt_mmr_topk: the bad query's outputs are all empty, its neighbours' untouched
        need = L.load().ebt_mmr_workspace_bytes(4, p)
        ws = torch.zeros(need, dtype=torch.uint8, device=dev)
        pos = torch.full((4, 10), -9, dtype=torch.int32, device=dev)
        orow = torch.full((4, 10), -9, dtype=torch.int64, device=dev)
        orel = torch.full((4, 10), 7.0, dtype=torch.float64, device=dev)
        ommr = torch.full((4, 10), 7.0, dtype=torch.float64, device=dev)
        st = torch.full((4,), -9, dtype=torch.int32, device=dev)
        L.call("ebt_mmr_topk", ctypes.byref(cat.cstruct), 4, L.ptr(rel), L.ptr(bt), p, 10, 0.5,
               L.ptr(ws), need, L.ptr(pos), L.ptr(orow), L.ptr(orel), L.ptr(ommr), L.ptr(st),
               L.stream_of(dev))
        assert st.cpu().tolist() == want
        assert (pos[q] == -1).all() and (orow[q] == -1).all()
        assert torch.isnan(orel[q]).all() and torch.isnan(ommr[q]).all()
        for b in range(4):
            if b != q:
                assert (bits(pos[b]), bits(orow[b]), bits(orel[b]), bits(ommr[b])) == \
                    (bits(clean.pos[b]), bits(clean.rows[b]), bits(clean.scores[b]),
                     bits(clean.mmr[b])), (q, b)
        with pytest.raises(ebt.EbertError, match=f"query {q}"):
            dv.diversify_topk(cat, rel, bt, 10, lam=0.5)


# ------------------------------------------------------------------------ 2. selection, bitwise ----
def check_select(out, G, rel, rows, k, lam):
    """ebt_mmr_select's outputs against mmr_ref on the same matrix and relevances, bit for bit."""
    pos, orow, orel, ommr = (x.cpu().numpy() for x in (out.pos, out.rows, out.scores, out.mmr))
    assert pos.dtype == np.int32 and orow.dtype == np.int64
    for b in range(len(rows)):
        wp, wr, ws, wv = mmr_ref(G[b], rel[b], rows[b], k, lam)
        assert np.array_equal(pos[b], wp), (b, k, lam, pos[b], wp)
        assert np.array_equal(orow[b], wr), (b, k, lam)
        assert orel[b].tobytes() == ws.tobytes(), (b, k, lam)
        assert ommr[b].tobytes() == wv.tobytes(), (b, k, lam)


@pytest.mark.parametrize("p", POOLS)
def test_select_bitwise_on_the_device_matrix(cuda_device, catalogs, p):
    """mmr_ref fed the GPU's own matrix and relevances: out_pos equal, out_mmr / out_rel equal as
    bit patterns, for lam in {0, 0.3, 0.7, 1} and k in {1, 10, p}; the relevances hold a NaN and
    two equal values (the position tie-break), the pool a -1 slot and the zero-norm row."""
    _, _, dv = _ebt()
    dev = cuda_device
    cat, _, scores, rows = catalogs("f32", 768)
    s, r = make_pool(scores, rows, p)
    if p > 3:
        s[:, 3] = np.nan
    if p > 5:
        s[:, 5] = s[:, 4]
    if p > 20:
        s[2, 9] = s[2, 8] = s[2, 1]           # three equal values
    rt, st = torch.from_numpy(r).to(dev), torch.from_numpy(s).to(dev)
    gram, status = dv.pool_gram(cat, rt)
    G = gram.cpu().numpy()
    for lam in (0.0, 0.3, 0.7, 1.0):
        for k in sorted({1, min(10, p), p}):
            check_select(dv.mmr_select(gram, st, rt, k, lam, status=status), G, s, r, k, lam)
    # status NULL: the same selection
    k = min(10, p)
    a, b = dv.mmr_select(gram, st, rt, k, 0.7), dv.mmr_select(gram, st, rt, k, 0.7, status=status)
    assert all(bits(x) == bits(y) for x, y in zip(a, b))


@pytest.mark.parametrize("p", [5, 64, 130])
def test_select_bitwise_on_a_hand_made_matrix(cuda_device, p):
    """Exact ties everywhere (similarities and relevances on a 0.25 grid), -0.0 beside +0.0,
    infinite and NaN relevances, a query with no candidate, a query whose status is -2."""
    _, _, dv = _ebt()
    dev = cuda_device
    rng = np.random.default_rng(31)
    B = 6
    G = np.round(rng.uniform(-1, 1, (B, p, p)) * 4) / 4
    G = np.maximum(G, G.transpose(0, 2, 1))
    G[1][G[1] == 0.0] = -0.0
    rel = np.round(rng.standard_normal((B, p)) * 2) / 4
    rel[1, ::2], rel[1, 1::2] = 0.0, -0.0
    rel[2, 0], rel[2, 1], rel[2, 2] = np.inf, -np.inf, np.nan
    rows = rng.integers(0, 10 ** 12, size=(B, p))
    rows[3] = -1                                                  # no candidate at all
    rows[4, 1] = -1
    status = np.array([1, 1, 1, 1, 1, -2], dtype=np.int32)
    gt, st, rt = (torch.from_numpy(x).to(dev) for x in (G, rel, rows))
    for lam in (0.0, 0.5, 1.0):
        for k in (1, min(p, 7), p):
            out = dv.mmr_select(gt, st, rt, k, lam, status=torch.from_numpy(status).to(dev))
            want_rows = rows.copy()
            want_rows[5] = -1                                     # status -2: all-empty outputs
            check_select(out, G, rel, want_rows, k, lam)
            assert (out.pos[3] == -1).all() and (out.pos[5] == -1).all()
            assert torch.isnan(out.mmr[5]).all() and (out.rows[5] == -1).all()


# ------------------------------------------------------- 3. end to end, tolerance-aware ----
@pytest.mark.parametrize("lam", [0.0, 0.3, 0.7, 1.0])
@pytest.mark.parametrize("dt,d", [("f32", 768), ("bf16", 77), ("f16", 32), ("f64", 1536)])
def test_diversify_topk_end_to_end(cuda_device, catalogs, dt, d, lam):
    """At each step t, on the GPU's own prefix: the oracle value of the chosen slot is within
    SCORE_ATOL of out_mmr, and no unpicked candidate's oracle value exceeds it by more than
    2 SCORE_ATOL. Every pool size, no case skipped."""
    ebt, _, _ = _ebt()
    dev = cuda_device
    cat, S, scores, rows = catalogs(dt, d)
    liked = liked_lists()
    oml = 1.0 - lam
    worst = 0.0
    for p in POOLS:
        s, r = make_pool(scores, rows, p)
        k = min(p, 10)
        out = ebt.diversify_topk(cat, torch.from_numpy(s).to(dev), torch.from_numpy(r).to(dev), k,
                                 lam=lam)
        pos, orow, orel, ommr = (x.cpu().numpy() for x in (out.pos, out.rows, out.scores, out.mmr))
        for b in range(len(LENS)):
            cand = r[b] >= 0
            # (the forced zero-norm row's relevance is the oracle's too: exactly 0)
            rel = oracle_rel(S, liked[b], r[b])
            np.testing.assert_allclose(s[b][cand], rel[cand], rtol=0, atol=SCORE_ATOL)
            G = oracle_gram(S, r[b])
            n = min(k, int(cand.sum()))
            assert (pos[b, :n] >= 0).all() and len(set(pos[b, :n].tolist())) == n
            assert (pos[b, n:] == -1).all() and (orow[b, n:] == -1).all()
            assert np.isnan(orel[b, n:]).all() and np.isnan(ommr[b, n:]).all()
            pen = np.zeros(p)
            left = cand.copy()
            for t in range(n):
                c = pos[b, t]
                assert left[c] and orow[b, t] == r[b, c]
                assert orel[b, t].tobytes() == s[b, c].tobytes()
                v = lam * rel - oml * pen
                worst = max(worst, abs(v[c] - ommr[b, t]))
                assert abs(v[c] - ommr[b, t]) <= SCORE_ATOL, (p, b, t)
                left[c] = False
                if left.any():
                    assert v[left].max() <= v[c] + 2 * SCORE_ATOL, (p, b, t)
                pen = G[c].copy() if t == 0 else np.fmax(pen, G[c])
    print(f"{dt} d={d} lam={lam}: max |oracle v - out_mmr| = {worst:.3e}")


# ------------------------------------- 4. equality with the oracle's greedy where it is decidable ----
def oracle_greedy_with_gaps(G, rel, rows, k, lam):
    """mmr_ref's picks on the oracle's values and the smallest gap between the best and the
    runner-up over the k rounds."""
    pos, orow, _, _ = mmr_ref(G, rel, rows, k, lam)
    oml = 1.0 - lam
    pen = np.zeros(len(rel))
    left = (rows >= 0) & ~np.isnan(rel)
    gap = np.inf
    for t, c in enumerate(pos):
        v = lam * rel - oml * pen
        top = np.sort(v[left])[::-1]
        assert top[0] == v[c]
        if len(top) > 1:
            gap = min(gap, top[0] - top[1])
        left[c] = False
        pen = G[c].copy() if t == 0 else np.fmax(pen, G[c])
    return pos, orow, gap


@pytest.mark.parametrize("lam", [0.3, 0.7])
@pytest.mark.parametrize("p", [17, 100, 512])
@pytest.mark.parametrize("d", [32, 77, 1536])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_rows_equal_the_oracles_greedy(cuda_device, catalogs, dt, d, p, lam):
    """pool = the top p minus the liked rows, k = min(p, 20). The oracle's smallest gap between
    the best and the runner-up is ASSERTED to exceed 1e-9 (1,000 times the tolerance: the choice
    is decidable), then the GPU's rows equal the oracle's greedy."""
    ebt, _, _ = _ebt()
    cat, S, _, _ = catalogs(dt, d)
    liked = liked_lists()
    k = min(p, 20)
    scores, rows = ebt.score_topk(cat, p, liked=liked, exclude=[sorted(l) for l in liked])
    out = ebt.diversify_topk(cat, scores, rows, k, lam=lam)
    got = out.rows.cpu().numpy()
    moved, gap = 0, np.inf
    for b in range(len(LENS)):
        full = S[np.asarray(liked[b])].mean(axis=0)
        osc, orows = R.topk_from_scores(full, p, exclude=liked[b])
        opos, want, g = oracle_greedy_with_gaps(S[np.ix_(orows, orows)], osc, orows, k, lam)
        gap = min(gap, g)
        moved += int((opos != np.arange(k)).sum())
        assert g > 1e-9, (b, g)
        assert np.array_equal(got[b], want), (b, got[b], want)
    print(f"{dt} d={d} p={p} lam={lam}: smallest oracle gap {gap:.3e}, "
          f"{moved} of {len(LENS) * k} positions moved by the selection")
    assert moved > 0


# ------------------------------------------------------------------------------ 5. behaviour ----
def test_lam_one_is_the_plain_topk(cuda_device, catalogs):
    ebt, _, _ = _ebt()
    cat, _, scores, rows = catalogs("f32", 768)
    for p, k in ((512, 10), (100, 100), (17, 1), (65, 64)):
        s, r = scores[:, :p].contiguous(), rows[:, :p].contiguous()
        out = ebt.diversify_topk(cat, s, r, k, lam=1.0)
        assert torch.equal(out.rows, r[:, :k]) and bits(out.scores) == bits(s[:, :k].contiguous())
        assert bits(out.mmr) == bits(s[:, :k].contiguous())
        assert torch.equal(out.pos.long(), torch.arange(k, device=r.device).expand(len(LENS), k))


def test_copies_of_a_row_are_kept_apart(cuda_device):
    """Row 9 is the direction of the liked rows' mean query (the best row there can be), rows 10
    and 11 are copies of it, so the liked list ranks the three first: the plain top 3 holds all of
    them; at lam = 0.5 the oracle's greedy keeps exactly one in its top 10 (asserted of the
    oracle first), and so does the GPU, the same one."""
    ebt, _, _ = _ebt()
    dev = cuda_device
    x = gaussian(91, N, 768, "f32")
    liked = [20, 21, 22, 23, 24]
    x[9] = R.mean_cosine_query(x[liked]).astype(np.float32)
    x[10] = x[11] = x[9]
    cat = ebt.Catalog(_t(x, "f32", dev))
    S = R.cosine_similarity(x, x)
    scores, rows = ebt.score_topk(cat, 100, liked=[liked])
    r = rows[0].cpu().numpy()
    assert r[:3].tolist() == [9, 10, 11]
    _, want, _, _ = mmr_ref(S[np.ix_(r, r)], S[liked].mean(axis=0)[r], r, 10, 0.5)
    assert len({9, 10, 11} & set(want.tolist())) == 1
    out = ebt.diversify_topk(cat, scores, rows, 10, lam=0.5)
    got = out.rows[0].cpu().numpy()
    assert {9, 10, 11} & set(got.tolist()) == {9, 10, 11} & set(want.tolist())
    assert np.array_equal(got, want)


def test_chunked_by_ws_budget_equals_unchunked(cuda_device, catalogs):
    ebt, L, _ = _ebt()
    cat, _, scores, rows = catalogs("f32", 768)
    p = 100
    s, r = scores[:, :p].contiguous(), rows[:, :p].contiguous()
    whole = ebt.diversify_topk(cat, s, r, 10, lam=0.7)
    per = L.load().ebt_mmr_workspace_bytes(1, p)
    for budget in (3 * per, 3 * per + per // 2, 1, 0):      # 3 + 3 + 2 queries; one at a time
        part = ebt.diversify_topk(cat, s, r, 10, lam=0.7, ws_budget=budget)
        assert all(bits(a) == bits(b) for a, b in zip(whole, part)), budget


@pytest.mark.parametrize("materialised", [False, True])
def test_pools_of_masked_searches(cuda_device, catalogs, materialised):
    """Results of masked and materialised-mask searches are parent rows: the pool of a mask with
    14 allowed rows has three empty slots at p = 17, and the picks come from the allowed rows."""
    ebt, _, dv = _ebt()
    cat, _, _, _ = catalogs("f32", 768)
    liked = liked_lists()
    allowed = [r for r in range(N) if r % 150 == 1]
    masks = ebt.AllowMasks(cat, 1)
    masks.set(0, allowed)
    if materialised:
        assert masks.materialize(0) == 14
    scores, rows = ebt.score_topk(cat, 17, liked=liked, allow=(masks, [0] * 7 + [-1]))
    assert bool((rows[:7, 14:] == -1).all()) and bool((rows[7] >= 0).all())
    out = ebt.diversify_topk(cat, scores, rows, 17, lam=0.5)
    gram, status = dv.pool_gram(cat, rows)
    check_select(out, gram.cpu().numpy(), scores.cpu().numpy(), rows.cpu().numpy(), 17, 0.5)
    got = out.rows.cpu().numpy()
    for b in range(7):
        assert sorted(got[b, :14].tolist()) == allowed and (got[b, 14:] == -1).all()


def test_get_user_recs_diverse_c1(cuda_device):
    """The C1 catalog and users (inputs.c1_catalog, the ratings of c1_users as the golden file
    holds them): the movies of mmr_ref over the oracle's scores and similarities, in selection
    order, with the oracle's relevances; the pool defaults to min(10 k, 512, rows); [] without
    ratings, sklearn's ValueError without a liked movie."""
    from test_gpu_parity import _collab_setup
    lib, gold = _collab_setup(cuda_device)
    ids, cat_np = c1_catalog()
    index = {t: i for i, t in enumerate(ids)}
    S = R.cosine_similarity(cat_np, cat_np)
    k = 10

    def oracle(rec, k, lam, pool):
        rating = {}
        for t, rt in rec["ratings"]:
            if t in index:
                rating.setdefault(t, []).append(rt)
        liked = [index[t] for t, rs in rating.items() for rt in rs if rt >= lib.LIKED_MOVIE_SCORE]
        full = S[liked].mean(axis=0)
        sc, rows = R.topk_from_scores(full, pool, exclude=[index[t] for t in rating])
        _, prow, prel, _ = mmr_ref(S[np.ix_(rows, rows)], sc, rows, min(k, len(rows)), lam)
        return [(ids[r], s) for r, s in zip(prow, prel) if r >= 0]

    seen = 0
    for uid, rec in gold["users"].items():
        want = rec[f"k{k}"]
        if isinstance(want, dict):
            with pytest.raises(ValueError) as ei:
                lib.get_user_recs_diverse(uid, k)
            assert str(ei.value) == want["message"]
            continue
        if not rec["ratings"]:
            assert lib.get_user_recs_diverse(uid, k) == []
            continue
        for lam, pool in ((0.7, None), (0.3, 30)):
            got = lib.get_user_recs_diverse(uid, k, lam=lam, pool=pool)
            ref = oracle(rec, k, lam, 100 if pool is None else pool)
            assert [g.movie.tmdb_id for g in got] == [t for t, _ in ref], (uid, lam, pool)
            assert all(abs(g.score - s) <= SCORE_ATOL for g, (_, s) in zip(got, ref))
        plain = lib.get_user_recs(uid, k)
        same = lib.get_user_recs_diverse(uid, k, lam=1.0)
        assert [(p.movie.tmdb_id, p.score) for p in plain] == \
            [(g.movie.tmdb_id, g.score) for g in same], uid
        assert lib.get_user_recs_diverse(uid, k, pool=100) == lib.get_user_recs_diverse(uid, k)
        seen += 1
    assert seen >= 15
    from robot_ebert_amd import EbertError
    with pytest.raises(EbertError, match="outside"):
        lib.get_user_recs_diverse("u05", k, lam=1.5)
    with pytest.raises(EbertError, match="p=600"):
        lib.get_user_recs_diverse("u05", k, pool=600)
