"""GPU: per-row weights on liked-row queries (include/ebert.h 0.8.0).

    score_b(j) = ( sum_l w_l cos(x_{r_l}, x_j) ) / W_b,    W_b = sum_l |w_l|

The oracle is built here from oracle.restatement: S = cosine_similarity(cat[liked], cat),
scores = (w[:, None] * S).sum(0) / abs(w).sum(), topk_from_scores(scores, k, exclude). Rows must
be equal, scores within SCORE_ATOL = 1e-12. Every oracle comparison first asserts on the CPU that
the oracle's top k + 1 scores have no adjacent gap below 1e-9 other than exact ties, so that a
row swap cannot hide behind round-off.

The prep kernels and the invariants (weights 1.0 == no weights, weights x 4 == weights, a 0.0
weight == the entry removed, device weights == host weights, checked == unchecked, mask pass ==
materialised mask, fused == unfused) are compared BITWISE: the operation order is fixed
(w * (x / g) rounded, added in CSR order; W_b a sequential sum; the scale 1.0 / W_b).
"""
import ctypes
import threading

import numpy as np
import pytest
import torch

from inputs import c1_catalog, gaussian
from oracle import restatement as R

pytestmark = pytest.mark.gpu
SCORE_ATOL = 1e-12
GAP = 1e-9
TORCH_DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16,
            "f64": torch.float64}
VP, I32, I64, SZ = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_size_t
EBT_EINVAL = -1
EBT_FLAG_LIKED_CHECKED = 8


def _ebt():
    import robot_ebert_amd as ebt
    from robot_ebert_amd import _lib
    return ebt, _lib


def _t(x, dt, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev).to(TORCH_DT[dt])


def weighted_oracle(cat_np, liked, weights, k, excl=None):
    """(scores [B, k], rows [B, k]) of the weighted mean cosine, NaN / -1 padded; asserts the
    gap condition on every query's top k + 1."""
    B = len(liked)
    out_s = np.full((B, k), np.nan)
    out_r = np.full((B, k), -1, dtype=np.int64)
    for b in range(B):
        w = np.asarray(weights[b], dtype=np.float64)
        S = R.cosine_similarity(cat_np[np.asarray(liked[b], dtype=np.int64)], cat_np)
        scores = (w[:, None] * S).sum(0) / np.abs(w).sum()
        e = excl[b] if excl is not None else None
        s1, _ = R.topk_from_scores(scores, k + 1, e)
        gaps = -np.diff(s1[~np.isnan(s1)])
        assert ((gaps == 0.0) | (gaps >= GAP)).all(), (b, gaps.min())
        s, r = R.topk_from_scores(scores, k, e)
        out_s[b, :len(s)], out_r[b, :len(r)] = s, r
    return out_s, out_r


def assert_topk_equal(s, r, s_ref, r_ref):
    s, r = s.cpu().numpy(), r.cpu().numpy()
    np.testing.assert_array_equal(r, r_ref)
    m = r_ref >= 0
    np.testing.assert_allclose(s[m], s_ref[m], rtol=0, atol=SCORE_ATOL)
    assert np.all(np.isnan(s[~m]))


def assert_bitwise(a, b):
    assert torch.equal(a[1], b[1])
    torch.testing.assert_close(a[0], b[0], rtol=0, atol=0, equal_nan=True)


def mixed_weights(rng, n):
    """n finite weights of both signs, none zero, magnitudes in [0.5, 5]."""
    w = rng.uniform(0.5, 5.0, n) * rng.choice([-1.0, 1.0], n)
    if n > 1:
        w[0], w[1] = abs(w[0]), -abs(w[1])
    return w


# ------------------------------------------------------------------- 1. the prep kernels ----
LENS = (1, 7, 8, 9, 256, 257, 300)   # across QL_UL = 8 and QL_STAGE = 256


def _wsum(L, xt, d, ld, g, off, rows, w, dev):
    B = off.numel() - 1
    q64 = torch.full((B, d), float("nan"), dtype=torch.float64, device=dev)
    L.call("ebt_query_liked_wsum", L.ptr(xt), L.DTYPE_CODE[xt.dtype], d, ld, L.ptr(g), B,
           L.ptr(off), L.ptr(rows), L.ptr(w), L.ptr(q64), L.stream_of(dev))
    return q64


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16", "f64"])
@pytest.mark.parametrize("d", [77, 768, 1536])
def test_query_liked_wsum_bitwise(cuda_device, dt, d):
    """ebt_query_liked_wsum against a float64 numpy loop in the same order (term = w * (x / g),
    added in CSR order; numpy multiplies, divides and adds in IEEE float64 without fusing):
    d = 77 runs the element form, 768 and 1536 the 16-byte-chunk form; lists with duplicates,
    mixed-sign weights. On the aligned input the element form (the same values at a row stride
    that is no multiple of 16 bytes) gives the chunk form's bits."""
    ebt, L = _ebt()
    dev = cuda_device
    n = 2000
    x = gaussian(61, n, d, dt)
    x[3] = 0.0                                    # a zero-norm row (norm guard 1.0)
    xt = _t(x, dt, dev)
    g = torch.empty(n, dtype=torch.float64, device=dev)
    L.call("ebt_row_norms", L.ptr(xt), L.DTYPE_CODE[xt.dtype], n, d, d, L.ptr(g), None,
           L.stream_of(dev))
    rng = np.random.default_rng(62)
    lists = [rng.integers(0, n, size=m) for m in LENS]      # with replacement: duplicates
    lists[1][0] = 3
    ws = [mixed_weights(rng, m) for m in LENS]
    off_np = np.zeros(len(LENS) + 1, dtype=np.int64)
    off_np[1:] = np.cumsum(LENS)
    off = torch.from_numpy(off_np).to(dev)
    rows = torch.from_numpy(np.concatenate(lists)).to(dev)
    w = torch.from_numpy(np.concatenate(ws)).to(dev)
    got = _wsum(L, xt, d, d, g, off, rows, w, dev).cpu().numpy()
    g_np = g.cpu().numpy()
    x64 = xt.to(torch.float64).cpu().numpy()
    want = np.zeros((len(LENS), d))
    for b, (rl, wl) in enumerate(zip(lists, ws)):
        acc = np.zeros(d)
        for r, wv in zip(rl, wl):
            acc = acc + wv * (x64[r] / g_np[r])
        want[b] = acc
    assert got.tobytes() == want.tobytes()
    # weights of 1.0: the unweighted kernels' bits
    one = torch.ones_like(w)
    q1 = _wsum(L, xt, d, d, g, off, rows, one, dev)
    q0 = torch.empty_like(q1)
    L.call("ebt_query_liked_sum", L.ptr(xt), L.DTYPE_CODE[xt.dtype], d, d, L.ptr(g), len(LENS),
           L.ptr(off), L.ptr(rows), L.ptr(q0), L.stream_of(dev))
    assert torch.equal(q1, q0)
    if d != 77:
        # the same values at row stride d + 1 elements: not 16-byte rows, the element form
        es = xt.element_size()
        assert (d * es) % 16 == 0 and ((d + 1) * es) % 16 != 0
        xp = torch.zeros((n, d + 1), dtype=xt.dtype, device=dev)
        xp[:, :d] = xt
        got_s = _wsum(L, xp, d, d + 1, g, off, rows, w, dev).cpu().numpy()
        assert got_s.tobytes() == got.tobytes()


def _sum(L, xt, d, ld, g, off, rows, dev):
    B = off.numel() - 1
    q64 = torch.full((B, d), float("nan"), dtype=torch.float64, device=dev)
    L.call("ebt_query_liked_sum", L.ptr(xt), L.DTYPE_CODE[xt.dtype], d, ld, L.ptr(g), B,
           L.ptr(off), L.ptr(rows), L.ptr(q64), L.stream_of(dev))
    return q64


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16", "f64"])
@pytest.mark.parametrize("d", [77, 768])
def test_query_liked_sum_bitwise(cuda_device, dt, d):
    """ebt_query_liked_sum itself (above it is pinned only through "weights of 1.0 give its
    bits") against a float64 numpy loop in the same order, acc = acc + x / g in CSR order:
    d = 77 runs the element form, 768 the 16-byte-chunk form; lists with duplicates, a
    zero-norm row. On the aligned input the element form (the same values at row stride d + 1)
    gives the chunk form's bits."""
    ebt, L = _ebt()
    dev = cuda_device
    n = 2000
    x = gaussian(63, n, d, dt)
    x[3] = 0.0                                    # a zero-norm row (norm guard 1.0)
    xt = _t(x, dt, dev)
    g = torch.empty(n, dtype=torch.float64, device=dev)
    L.call("ebt_row_norms", L.ptr(xt), L.DTYPE_CODE[xt.dtype], n, d, d, L.ptr(g), None,
           L.stream_of(dev))
    rng = np.random.default_rng(64)
    lists = [rng.integers(0, n, size=m) for m in LENS]      # with replacement: duplicates
    lists[1][0] = 3
    lists[6][:2] = lists[6][2]                               # and a certain one
    off_np = np.zeros(len(LENS) + 1, dtype=np.int64)
    off_np[1:] = np.cumsum(LENS)
    off = torch.from_numpy(off_np).to(dev)
    rows = torch.from_numpy(np.concatenate(lists)).to(dev)
    got = _sum(L, xt, d, d, g, off, rows, dev).cpu().numpy()
    g_np = g.cpu().numpy()
    assert g_np[3] == 1.0
    x64 = xt.to(torch.float64).cpu().numpy()
    want = np.zeros((len(LENS), d))
    for b, rl in enumerate(lists):
        acc = np.zeros(d)
        for r in rl:
            acc = acc + x64[r] / g_np[r]
        want[b] = acc
    assert got.tobytes() == want.tobytes()
    if d != 77:
        # the same values at row stride d + 1 elements: not 16-byte rows, the element form
        es = xt.element_size()
        assert (d * es) % 16 == 0 and ((d + 1) * es) % 16 != 0
        xp = torch.zeros((n, d + 1), dtype=xt.dtype, device=dev)
        xp[:, :d] = xt
        got_s = _sum(L, xp, d, d + 1, g, off, rows, dev).cpu().numpy()
        assert got_s.tobytes() == got.tobytes()


# ------------------------------------------------------------ 2. invariants of score_topk ----
@pytest.fixture(scope="module")
def c1(cuda_device):
    ebt, _ = _ebt()
    ids, cat_np = c1_catalog()
    cat = ebt.Catalog(_t(cat_np, "f64", cuda_device), ids=ids)
    rng = np.random.default_rng(7)      # test_liked_queries_match_oracle's lists and exclusions
    liked = [sorted(rng.choice(len(ids), size=int(rng.integers(1, 90)), replace=False).tolist())
             for _ in range(20)]
    liked[0] = [7]  # only the zero-norm row
    excl = [sorted(set(l) | set(rng.choice(len(ids), 30, replace=False).tolist()))
            for l in liked]
    return cat, cat_np, liked, excl


@pytest.fixture(scope="module")
def wide(cuda_device):
    """2,000 x 768 f32 (the chunk form of the prep kernel), 12 users with 1..300 liked rows
    (duplicates included), mixed-sign weights."""
    ebt, _ = _ebt()
    c = gaussian(71, 2000, 768, "f32")
    cat = ebt.Catalog(_t(c, "f32", cuda_device))
    rng = np.random.default_rng(72)
    lens = [1, 2, 7, 8, 9, 40, 64, 100, 255, 256, 257, 300]
    liked = [rng.integers(0, 2000, size=m).tolist() for m in lens]
    w = [mixed_weights(rng, m).tolist() for m in lens]
    excl = [sorted(set(rng.choice(2000, 25, replace=False).tolist())) for _ in lens]
    return cat, c, liked, w, excl


@pytest.mark.parametrize("which", ["c1", "wide"])
def test_score_topk_weight_invariants(cuda_device, c1, wide, which):
    ebt, _ = _ebt()
    if which == "c1":
        cat, _, liked, excl = c1
        rng = np.random.default_rng(8)
        w = [mixed_weights(rng, len(l)).tolist() for l in liked]
    else:
        cat, _, liked, w, excl = wide
    k = 10
    base = ebt.score_topk(cat, k, liked=liked, exclude=excl, liked_weights=w)
    # weights all 1.0 == no weights
    ones = [[1.0] * len(l) for l in liked]
    assert_bitwise(ebt.score_topk(cat, k, liked=liked, exclude=excl, liked_weights=ones),
                   ebt.score_topk(cat, k, liked=liked, exclude=excl))
    # weights x 4.0 == weights
    w4 = [[4.0 * x for x in l] for l in w]
    assert_bitwise(ebt.score_topk(cat, k, liked=liked, exclude=excl, liked_weights=w4), base)
    # an entry with weight 0.0 == that entry removed (every list with >= 2 entries loses one)
    liked_z, w_z, liked_r, w_r = [], [], [], []
    for b, (l, x) in enumerate(zip(liked, w)):
        if len(l) < 2:
            liked_z.append(l), w_z.append(x), liked_r.append(l), w_r.append(x)
            continue
        j = b % len(l)
        liked_z.append(l), w_z.append(x[:j] + [0.0] + x[j + 1:])
        liked_r.append(l[:j] + l[j + 1:]), w_r.append(x[:j] + x[j + 1:])
    assert_bitwise(ebt.score_topk(cat, k, liked=liked_z, exclude=excl, liked_weights=w_z),
                   ebt.score_topk(cat, k, liked=liked_r, exclude=excl, liked_weights=w_r))
    # device-tensor weights (a CSR pair: the C entry checks on the host) == host-list weights
    # (checked while the CSR is built: EBT_FLAG_LIKED_CHECKED, 1 / W_b on the device)
    csr, wt = ebt.search.csr_from_weighted_lists(liked, w, cuda_device)
    assert wt.dtype == torch.float64 and wt.is_cuda and wt.numel() == sum(map(len, liked))
    assert_bitwise(ebt.score_topk(cat, k, liked=(csr[0], csr[1]), exclude=excl,
                                  liked_weights=wt), base)


def test_python_weight_errors(cuda_device, c1):
    ebt, _ = _ebt()
    cat, _, liked, excl = c1
    liked = liked[:3]
    ok = [[1.0] * len(l) for l in liked]
    for bad, pat in (([ok[0], ok[1] + [1.0], ok[2]], "query 1"),
                     ([ok[0], ok[1], [float("nan")] + ok[2][1:]], "query 2"),
                     ([[0.0], ok[1], ok[2]], "query 0"),
                     (ok[:2], "weight lists")):
        with pytest.raises(ebt.EbertError, match=pat):
            ebt.score_topk(cat, 5, liked=liked, liked_weights=bad)
    with pytest.raises(ebt.EbertError):
        ebt.score_topk(cat, 5, queries=torch.zeros((1, cat.d), device=cuda_device),
                       liked_weights=[[1.0]])
    # a device tensor of the wrong length, and device weights the C entry rejects (query named)
    csr, wt = ebt.search.csr_from_weighted_lists(liked, ok, cuda_device)
    with pytest.raises(ebt.EbertError):
        ebt.score_topk(cat, 5, liked=(csr[0], csr[1]), liked_weights=wt[:-1].clone())
    bad = wt.clone()
    bad[len(liked[0])] = float("inf")
    with pytest.raises(ebt.EbertError, match="query 1"):
        ebt.score_topk(cat, 5, liked=(csr[0], csr[1]), liked_weights=bad)
    with pytest.raises(ValueError, match="0 sample"):
        ebt.score_topk(cat, 5, liked=[[1], []], liked_weights=[[1.0], []])
    s, r = ebt.score_topk(cat, 5, liked=liked, liked_weights=ok)     # and it still works
    assert r.shape == (3, 5)


# ----------------------------------------------------------------------- 3. oracle parity ----
@pytest.mark.parametrize("signs", ["positive", "mixed"])
def test_weighted_matches_oracle_c1(cuda_device, c1, signs):
    """20 users, 1-90 liked rows, exclusions and k = 10, as test_liked_queries_match_oracle."""
    ebt, _ = _ebt()
    cat, cat_np, liked, excl = c1
    rng = np.random.default_rng(11)
    if signs == "positive":
        w = [rng.uniform(0.5, 5.0, len(l)).tolist() for l in liked]
    else:
        w = [mixed_weights(rng, len(l)).tolist() for l in liked]
    s_ref, r_ref = weighted_oracle(cat_np, liked, w, 10, excl)
    s, r = ebt.score_topk(cat, 10, liked=liked, exclude=excl, liked_weights=w)
    assert_topk_equal(s, r, s_ref, r_ref)
    assert tuple(r.shape) == (20, 10)


def test_weighted_wide_matches_oracle(cuda_device, wide):
    """The chunk-form prep (d = 768 f32), duplicates in the lists, lists of up to 300 rows."""
    ebt, _ = _ebt()
    cat, c, liked, w, excl = wide
    s_ref, r_ref = weighted_oracle(c.astype(np.float64), liked, w, 10, excl)
    s, r = ebt.score_topk(cat, 10, liked=liked, exclude=excl, liked_weights=w)
    assert_topk_equal(s, r, s_ref, r_ref)


def test_weighted_speculative_fused_equals_unfused(cuda_device):
    """The smallest shape at which test_gpu_parity.py runs the speculative fused screen
    (98,304 x 96 f32, 300 queries, k = 20): a weighted liked batch through it is bitwise the
    same call with fuse=False, and equals the oracle on sampled queries."""
    ebt, _ = _ebt()
    n, d, B, k = 98_304, 96, 300, 20
    c = gaussian(21, n, d, "f32")
    cat = ebt.Catalog(_t(c, "f32", cuda_device))
    rng = np.random.default_rng(24)
    liked = [rng.choice(n, size=int(rng.integers(1, 21)), replace=False).tolist()
             for _ in range(B)]
    w = [mixed_weights(rng, len(l)).tolist() for l in liked]
    excl = [sorted(set(l) | set(rng.choice(n, 40, replace=False).tolist())) for l in liked]
    pl = ebt.search.plan(cat, B, k)
    assert pl["fused"] and pl["spec"] is not None, pl
    timer = ebt.Timer()
    fused = ebt.score_topk(cat, k, liked=liked, exclude=excl, liked_weights=w, timer=timer)
    assert timer.query("gemm_filter")[1] >= 1, "fused path not taken"
    unfused = ebt.score_topk(cat, k, liked=liked, exclude=excl, liked_weights=w, fuse=False)
    assert_bitwise(fused, unfused)
    sample = [0, 150, 299]
    s_ref, r_ref = weighted_oracle(c.astype(np.float64), [liked[i] for i in sample],
                                   [w[i] for i in sample], k, [excl[i] for i in sample])
    assert_topk_equal(fused[0][sample], fused[1][sample], s_ref, r_ref)


# ------------------------------------------------------------------------------- 4. masks ----
def test_weighted_mask_pass_equals_materialised(cuda_device, c1):
    """A weighted batch under an allow mask, and the same mask materialised (the query prepared
    against the parent, scored over the sub-catalog): the same rows, bitwise the same scores,
    equal to the oracle with the disallowed rows excluded. No liked row is in the mask."""
    ebt, _ = _ebt()
    cat, cat_np, _, _ = c1
    n = cat.n
    allowed = [r for r in range(n) if r % 3 == 0]
    rng = np.random.default_rng(12)
    pool = np.array([r for r in range(n) if r % 3 != 0])
    liked = [sorted(rng.choice(pool, size=int(rng.integers(1, 60)), replace=False).tolist())
             for _ in range(9)]
    w = [mixed_weights(rng, len(l)).tolist() for l in liked]
    excl = [sorted(rng.choice(n, 20, replace=False).tolist()) for _ in liked]
    ids = [0] * 8 + [-1]            # the last query is unfiltered
    masks = ebt.AllowMasks(cat, 1)
    masks.set(0, allowed)
    by_mask = ebt.score_topk(cat, 10, liked=liked, exclude=excl, liked_weights=w,
                             allow=(masks, ids))
    assert masks.materialize(0) == len(allowed)
    p = ebt.score_topk_submit(cat, 10, liked=liked, exclude=excl, liked_weights=w,
                              allow=(masks, ids))
    assert [rt[0] for rt in p.routes] == [0] and p.routes[0][1] == list(range(8))
    by_sub = ebt.score_topk_finish(p)
    assert_bitwise(by_sub, by_mask)
    blocked = set(range(n)) - set(allowed)
    excl_ref = [sorted(set(e) | blocked) for e in excl[:8]] + [excl[8]]
    s_ref, r_ref = weighted_oracle(cat_np, liked, w, 10, excl_ref)
    assert_topk_equal(by_mask[0], by_mask[1], s_ref, r_ref)
    # a device CSR with device weights takes the same route
    csr, wt = ebt.search.csr_from_weighted_lists(liked, w, cuda_device)
    by_dev = ebt.score_topk(cat, 10, liked=(csr[0], csr[1]), exclude=excl, liked_weights=wt,
                            allow=(masks, ids))
    assert_bitwise(by_dev, by_mask)


# --------------------------------------------------------- 5. the C ABI through bare ctypes ----
class Options(ctypes.Structure):   # struct ebt_options
    _fields_ = [("kprime", I32), ("flags", I32), ("chunk_rows", I64)]


class Pending(ctypes.Structure):   # struct ebt_pending
    _fields_ = [("cat", VP), ("opt", Options), ("B", I64), ("B_pad", I64), ("chunk", I64),
                ("k", I32), ("k_eff", I32), ("kprime", I32), ("flags", I32), ("excl_off", VP),
                ("excl_rows", VP), ("ws", VP), ("ws_bytes", SZ), ("out_scores", VP),
                ("out_rows", VP), ("cert_host", VP), ("event", VP), ("timer", VP),
                ("stream", VP)]


@pytest.fixture(scope="module")
def capi():
    from test_gpu_capi import LIB, Catalog
    h = ctypes.CDLL(LIB)
    PC = ctypes.POINTER(Catalog)
    h.ebt_last_error.restype = ctypes.c_char_p
    h.ebt_catalog_state_bytes.argtypes = [VP, ctypes.c_int, I64, I32, I64]
    h.ebt_catalog_state_bytes.restype = SZ
    h.ebt_catalog_init.argtypes = [PC, VP, ctypes.c_int, I64, I32, I64, I64, VP, SZ, VP]
    h.ebt_workspace_bytes.argtypes = [PC, I64, I32, VP]
    h.ebt_workspace_bytes.restype = SZ
    h.ebt_cosine_topk.argtypes = [PC, VP, ctypes.c_int, I64, I64, VP, VP, I32, VP, VP, VP, VP,
                                  SZ, VP, VP, VP, VP]
    h.ebt_cosine_topk_weighted.argtypes = [PC, VP, ctypes.c_int, I64, I64, VP, VP, I32, VP, VP,
                                           VP, VP, SZ, VP, VP, VP, VP, VP, VP]
    h.ebt_cosine_topk_weighted_submit.argtypes = [PC, VP, ctypes.c_int, I64, I64, VP, VP, I32,
                                                  VP, VP, VP, VP, SZ, VP, VP, VP,
                                                  ctypes.POINTER(Pending), VP, VP, VP, VP]
    h.ebt_cosine_topk_allowed_finish.argtypes = [ctypes.POINTER(Pending), VP]
    return h


def _c_weighted(h, cat, k, dev, liked, w, excl=None, q=None, opt=None):
    """One ebt_cosine_topk_weighted call (allow = NULL); (rc, message, scores, rows)."""
    from test_gpu_capi import CODE, P
    B = q.shape[0] if q is not None else liked[0].numel() - 1
    optp = ctypes.byref(opt) if opt is not None else None
    need = h.ebt_workspace_bytes(ctypes.byref(cat), B, k, optp)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    s = torch.empty((B, k), dtype=torch.float64, device=dev)
    r = torch.empty((B, k), dtype=torch.int64, device=dev)
    lo, lr = liked if liked is not None else (None, None)
    eo, er = excl if excl is not None else (None, None)
    rc = h.ebt_cosine_topk_weighted(
        ctypes.byref(cat), P(q), CODE[q.dtype] if q is not None else 0, B,
        q.stride(0) if q is not None else 0, P(lo), P(lr), k, P(eo), P(er), optp, P(ws), need,
        P(s), P(r), None, torch.cuda.current_stream(dev).cuda_stream, None, P(w))
    return rc, (h.ebt_last_error().decode() if rc else ""), s, r


def test_capi_weighted(cuda_device, capi, c1):
    from test_gpu_capi import P, csr, make_catalog, topk
    ebt, _ = _ebt()
    dev = cuda_device
    cat_py, cat_np, liked, excl = c1
    rng = np.random.default_rng(13)
    w_l = [mixed_weights(rng, len(l)).tolist() for l in liked]
    want = ebt.score_topk(cat_py, 10, liked=liked, exclude=excl, liked_weights=w_l)
    emb = torch.from_numpy(cat_np).to(dev)
    cat, state = make_catalog(capi, emb)
    lcsr, ecsr = csr(liked, dev), csr(excl, dev)      # (the lists are sorted already)
    w = torch.from_numpy(np.concatenate([np.asarray(x) for x in w_l])).to(dev)
    B, k = len(liked), 10
    # the blocking entry == the Python result
    rc, msg, s, r = _c_weighted(capi, cat, k, dev, lcsr, w, ecsr)
    assert rc == 0, msg
    assert_bitwise((s, r), want)
    # EBT_FLAG_LIKED_CHECKED (1 / W_b on the device, nothing read back) == the checked path
    rc, msg, s2, r2 = _c_weighted(capi, cat, k, dev, lcsr, w, ecsr,
                                  opt=Options(0, EBT_FLAG_LIKED_CHECKED, 0))
    assert rc == 0, msg
    assert_bitwise((s2, r2), (s, r))
    # _weighted_submit, finished with ebt_cosine_topk_allowed_finish
    need = capi.ebt_workspace_bytes(ctypes.byref(cat), B, k, None)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    s3 = torch.empty((B, k), dtype=torch.float64, device=dev)
    r3 = torch.empty((B, k), dtype=torch.int64, device=dev)
    cert = torch.empty(B + 1, dtype=torch.int32, pin_memory=True)
    pend = Pending()
    st = torch.cuda.current_stream(dev).cuda_stream
    rc = capi.ebt_cosine_topk_weighted_submit(
        ctypes.byref(cat), None, 0, B, 0, P(lcsr[0]), P(lcsr[1]), k, P(ecsr[0]), P(ecsr[1]), None,
        P(ws), need, P(s3), P(r3), P(cert), ctypes.byref(pend), None, st, None, P(w))
    assert rc == 0, capi.ebt_last_error()
    assert capi.ebt_cosine_topk_allowed_finish(ctypes.byref(pend), None) == 0, \
        capi.ebt_last_error()
    torch.cuda.synchronize(dev)
    assert_bitwise((s3, r3), (s, r))
    # liked_w == NULL is the unweighted entry
    rc, msg, s4, r4 = _c_weighted(capi, cat, k, dev, lcsr, None, ecsr)
    assert rc == 0, msg
    rc0, s0, r0 = topk(capi, cat, k, dev, liked=lcsr, excl=ecsr)
    assert rc0 == 0
    assert s4.cpu().numpy().tobytes() == s0.tobytes() and np.array_equal(r4.cpu().numpy(), r0)

    def still_works():
        rc, s5, r5 = topk(capi, cat, k, dev, liked=lcsr, excl=ecsr)
        assert rc == 0, capi.ebt_last_error()
        assert np.array_equal(r5, r0) and s5.tobytes() == s0.tobytes()
    # EBT_EINVAL with a message: a NaN weight, W = 0, liked_w with dense q
    off = lcsr[0].cpu().numpy()
    bad = w.clone()
    bad[int(off[3])] = float("nan")
    rc, msg, _, _ = _c_weighted(capi, cat, k, dev, lcsr, bad, ecsr)
    assert rc == EBT_EINVAL and "query 3" in msg, (rc, msg)
    still_works()
    bad = w.clone()
    bad[int(off[5]):int(off[6])] = 0.0
    rc, msg, _, _ = _c_weighted(capi, cat, k, dev, lcsr, bad, ecsr)
    assert rc == EBT_EINVAL and "query 5" in msg, (rc, msg)
    still_works()
    q = emb[:B].contiguous()
    rc, msg, _, _ = _c_weighted(capi, cat, k, dev, None, w, None, q=q)
    assert rc == EBT_EINVAL and "liked_w" in msg, (rc, msg)
    still_works()


# ----------------------------------------------------------------------------- 6. sharded ----
def _run_ranks_weighted(h, hip, full, world, k, liked, w, excl, allreduce):
    """ebt_cosine_topk_sharded_weighted on `world` thread ranks (the harness of
    test_gpu_capi_sharded.py with the weighted entry); per-rank (rc, message, s, r)."""
    from test_gpu_capi import P, make_catalog
    from test_gpu_capi_sharded import GATHER, REDUCE, Comm, shard_cuts
    dev = full.device
    n = full.shape[0]
    cuts = shard_cuts(n, world)
    shared = {"slots": [None] * world, "barrier": threading.Barrier(world, timeout=120),
              "rslots": [None] * world, "reduces": [0] * world}
    cats = []
    for r in range(world):
        cat, state = make_catalog(h, full[cuts[r]:cuts[r + 1]])
        cat.row_offset = cuts[r]
        cats.append((cat, state))
    out = [None] * world

    def body(rank):
        def gather(ctx, send, recv, nbytes, stream):
            try:
                hip.hipStreamSynchronize(stream)
                shared["slots"][rank] = send
                shared["barrier"].wait()
                for src in range(world):
                    if hip.hipMemcpy(recv + src * nbytes, shared["slots"][src], nbytes, 3):
                        return -1
                shared["barrier"].wait()
                return 0
            except threading.BrokenBarrierError:
                return -9

        def reduce(ctx, buf, count, stream):
            try:
                shared["reduces"][rank] += 1
                hip.hipStreamSynchronize(stream)
                mine = torch.empty(count, dtype=torch.float64, device=dev)
                if hip.hipMemcpy(mine.data_ptr(), buf, count * 8, 3):
                    return -1
                shared["rslots"][rank] = mine
                shared["barrier"].wait()
                acc = shared["rslots"][0].clone()
                for src in range(1, world):
                    acc += shared["rslots"][src]
                torch.cuda.synchronize(dev)
                if hip.hipMemcpy(buf, acc.data_ptr(), count * 8, 3):
                    return -1
                shared["barrier"].wait()
                return 0
            except threading.BrokenBarrierError:
                return -9
        try:
            cb, rcb = GATHER(gather), REDUCE(reduce)
            comm = Comm(rank, world, n, cb, None, ctypes.cast(rcb, VP) if allreduce else None)
            cat = cats[rank][0]
            B = liked[0].numel() - 1
            need = h.ebt_sharded_workspace_bytes(ctypes.byref(cat), ctypes.byref(comm), B, k, None)
            assert need > 0
            ws = torch.empty(need, dtype=torch.uint8, device=dev)
            s = torch.full((B, k), float("nan"), dtype=torch.float64, device=dev)
            rr = torch.full((B, k), -2, dtype=torch.int64, device=dev)
            rc = h.ebt_cosine_topk_sharded_weighted(
                ctypes.byref(cat), ctypes.byref(comm), None, 0, B, 0, P(liked[0]), P(liked[1]), k,
                P(excl[0]), P(excl[1]), None, P(ws), need, P(s), P(rr), None,
                torch.cuda.current_stream(dev).cuda_stream, P(w))
            out[rank] = (rc, h.ebt_last_error().decode() if rc else "", s, rr)
        except BaseException:  # noqa: BLE001
            shared["barrier"].abort()
            raise
    ts = [threading.Thread(target=body, args=(r,)) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(300)
    assert all(o is not None for o in out), "a rank did not finish"
    return out, shared["reduces"]


@pytest.fixture(scope="module")
def sharded_case(cuda_device):
    """3,000 x 64 f32; 6 users whose liked lists straddle the shard boundaries of world 2
    (1500) and 3 (1000, 2000), one wholly on the last shard, mixed-sign weights."""
    ebt, _ = _ebt()
    n, d = 3000, 64
    c = gaussian(81, n, d, "f32")
    rng = np.random.default_rng(82)
    liked = [[999, 1000, 1499, 1500, 1999, 2000], [0, 2999], [1499, 1500],
             sorted(rng.choice(n, 70, replace=False).tolist()), [2500, 2600, 2700],
             sorted(rng.choice(n, 300, replace=False).tolist())]
    w = [mixed_weights(rng, len(l)).tolist() for l in liked]
    excl = [sorted(set(l) | set(rng.choice(n, 15, replace=False).tolist())) for l in liked]
    full = _t(c, "f32", cuda_device)
    single = ebt.score_topk(ebt.Catalog(full), 10, liked=liked, exclude=excl, liked_weights=w)
    s_ref, r_ref = weighted_oracle(c.astype(np.float64), liked, w, 10, excl)
    assert_topk_equal(single[0], single[1], s_ref, r_ref)
    return full, liked, w, excl, single


@pytest.mark.parametrize("allreduce", [False, True])
@pytest.mark.parametrize("world", [2, 3])
def test_capi_sharded_weighted(cuda_device, sharded_case, world, allreduce):
    from test_gpu_capi import LIB, Catalog, csr
    from test_gpu_capi_sharded import Comm
    full, liked, w_l, excl, single = sharded_case
    h = ctypes.CDLL(LIB)
    PC, PM = ctypes.POINTER(Catalog), ctypes.POINTER(Comm)
    h.ebt_last_error.restype = ctypes.c_char_p
    h.ebt_catalog_state_bytes.argtypes = [VP, ctypes.c_int, I64, I32, I64]
    h.ebt_catalog_state_bytes.restype = SZ
    h.ebt_catalog_init.argtypes = [PC, VP, ctypes.c_int, I64, I32, I64, I64, VP, SZ, VP]
    h.ebt_sharded_workspace_bytes.argtypes = [PC, PM, I64, I32, VP]
    h.ebt_sharded_workspace_bytes.restype = SZ
    h.ebt_cosine_topk_sharded_weighted.argtypes = [PC, PM, VP, ctypes.c_int, I64, I64, VP, VP,
                                                   I32, VP, VP, VP, VP, SZ, VP, VP, VP, VP, VP]
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [VP, VP, SZ, ctypes.c_int]
    hip.hipStreamSynchronize.argtypes = [VP]
    dev = cuda_device
    w = torch.from_numpy(np.concatenate([np.asarray(x) for x in w_l])).to(dev)
    res, reduces = _run_ranks_weighted(h, hip, full, world, 10, csr(liked, dev), w,
                                       csr(excl, dev), allreduce)
    assert all(n == (1 if allreduce else 0) for n in reduces), reduces
    for rc, msg, s, r in res:
        assert rc == 0, msg
        assert torch.equal(r, single[1])
        torch.testing.assert_close(s, single[0], rtol=0, atol=SCORE_ATOL)


@pytest.mark.parametrize("world", [2, 3])
def test_python_sharded_weighted(cuda_device, sharded_case, world):
    """distributed.score_topk_sharded (split_liked's local weights and W_b, the all-reduce of
    the weighted partial sums) and the per-shard path score_topk_sharded_local."""
    from robot_ebert_amd.distributed import score_topk_sharded, score_topk_sharded_local
    from test_gpu_sharded import _run_sharded
    full, liked, w, excl, single = sharded_case
    for fn in (score_topk_sharded, score_topk_sharded_local):
        res = _run_sharded(full, world, lambda r, cat, coll: fn(
            cat, 10, liked=liked, exclude=excl, liked_weights=w, collectives=coll))
        for s, r in res:
            assert torch.equal(r, single[1]), fn.__name__
            torch.testing.assert_close(s, single[0], rtol=0, atol=SCORE_ATOL)


# --------------------------------------------------------------------- 7. batcher and lib ----
def test_batcher_mixes_weighted_and_unweighted(cuda_device, c1):
    """One batch of weighted and unweighted requests: each equals its own single call; a request
    with bad weights fails alone."""
    ebt, _ = _ebt()
    from robot_ebert_amd.batcher import RecBatcher
    cat, _, liked, excl = c1
    rng = np.random.default_rng(14)
    w = [mixed_weights(rng, len(l)).tolist() if b % 2 == 0 else None
         for b, l in enumerate(liked)]
    b = RecBatcher(cat, max_batch=64, max_wait_ms=300.0)
    try:
        futs = [b.submit(l, e, 10, weights=x) for l, e, x in zip(liked, excl, w)]
        bad = [b.submit(liked[1], excl[1], 10, weights=[1.0]),
               b.submit(liked[1], excl[1], 10, weights=[float("nan")] * len(liked[1])),
               b.submit(liked[1], excl[1], 10, weights=[0.0] * len(liked[1]))]
        got = [f.result(timeout=60) for f in futs]
        for f in bad:
            assert isinstance(f.exception(timeout=60), ValueError)
    finally:
        b.close()
    assert max(b.batches) > 1, "nothing was coalesced"
    for (s, r), l, e, x in zip(got, liked, excl, w):
        kw = {"liked_weights": [x]} if x is not None else {}
        s1, r1 = ebt.score_topk(cat, 10, liked=[l], exclude=[e], **kw)
        assert np.array_equal(r, r1[0].cpu().numpy())
        assert s.tobytes() == s1[0].cpu().numpy().tobytes()


def _weighted_user_recs(ratings, ids, cat_np, k, weighting):
    """get_user_recs(weighting=) restated in numpy float64: every rated catalog movie with a
    non-zero weight is a term; rated movies are excluded; ordered as lib.py:55-63."""
    pos = {t: i for i, t in enumerate(ids)}
    kept = [(t, r) for t, r in ratings if t in pos]
    terms = [(pos[t], weighting(r)) for t, r in kept if weighting(r) != 0.0]
    rated = sorted({pos[t] for t, _ in kept})
    rows = np.array([t[0] for t in terms], dtype=np.int64)
    w = np.array([t[1] for t in terms], dtype=np.float64)
    S = R.cosine_similarity(cat_np[rows], cat_np)
    scores = (w[:, None] * S).sum(0) / np.abs(w).sum()
    s1, _ = R.topk_from_scores(scores, k + 1, rated)
    gaps = -np.diff(s1[~np.isnan(s1)])
    assert ((gaps == 0.0) | (gaps >= GAP)).all()
    s, r = R.topk_from_scores(scores, k, rated)
    pairs = sorted(((ids[int(rr)], float(ss)) for ss, rr in zip(s, r)), key=lambda t: t[0])
    return sorted(pairs, key=lambda t: t[1], reverse=True)


def test_get_user_recs_weighting(cuda_device):
    """weighting=weight_centered against numpy float64 on the C1 fixtures of
    test_get_user_recs_matches_reference; weighting=None still returns the golden."""
    from test_gpu_parity import _collab_setup
    lib, gold = _collab_setup(cuda_device)
    ids, cat_np = c1_catalog()
    k = 10
    seen = 0
    for uid, rec in gold["users"].items():
        want_plain = rec[f"k{k}"]
        if isinstance(want_plain, dict):            # no liked movie: sklearn's ValueError
            with pytest.raises(ValueError) as ei:
                lib.get_user_recs(uid, k, weighting=None)
            assert str(ei.value) == want_plain["message"]
        else:
            got = lib.get_user_recs(uid, k, weighting=None)
            assert [g.movie.tmdb_id for g in got] == [x[0] for x in want_plain], uid
            np.testing.assert_allclose([g.score for g in got], [x[1] for x in want_plain],
                                       rtol=0, atol=SCORE_ATOL)
        if not rec["ratings"]:
            assert lib.get_user_recs(uid, k, weighting=lib.weight_centered) == []
            continue
        want = _weighted_user_recs(rec["ratings"], ids, cat_np, k, lib.weight_centered)
        got = lib.get_user_recs(uid, k, weighting=lib.weight_centered)
        assert [g.movie.tmdb_id for g in got] == [x[0] for x in want], uid
        np.testing.assert_allclose([g.score for g in got], [x[1] for x in want], rtol=0,
                                   atol=SCORE_ATOL)
        rated = {t for t, _ in rec["ratings"]}
        assert not rated & {g.movie.tmdb_id for g in got}
        seen += 1
    assert seen >= 15
    # a user whose every weight is zero: sklearn's empty-array error, as lib.py:51
    uid = next(u for u, rec in gold["users"].items() if rec["ratings"])
    with pytest.raises(ValueError, match="0 sample"):
        lib.get_user_recs(uid, k, weighting=lambda r: 0.0)
    # weight_by_rating: the reference's liked set, each movie by its rating
    want = _weighted_user_recs(gold["users"]["u05"]["ratings"], ids, cat_np, k,
                               lib.weight_by_rating)
    got = lib.get_user_recs("u05", k, weighting=lib.weight_by_rating)
    assert [g.movie.tmdb_id for g in got] == [x[0] for x in want]
    np.testing.assert_allclose([g.score for g in got], [x[1] for x in want], rtol=0,
                               atol=SCORE_ATOL)
