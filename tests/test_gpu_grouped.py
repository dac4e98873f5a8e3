"""GPU: grouped top-k (ebert.h 0.12.0: ebt_select_topk_grouped, ebt_cosine_topk_grouped_prepared,
score_topk_grouped).

The contract: out[b][g] is bit for bit what score_topk(..., allow=(masks, [groups[g]] * B))
returns for query b. So the end-to-end reference is the masked path as it stood before the
feature, compared bitwise; a second one is the float64 oracle per group (tests/grouped_ref.py).
The select kernel alone is compared with numpy exactly, values and indices. The first-pass
certificates are compared with the masked pipeline's, element for element, so that nothing hides
behind the fallback; the fallback itself is forced by a tie cluster wider than k'."""
import functools

import numpy as np
import pytest
import torch

from grouped_ref import grouped_ref, scores64, select_ref
from inputs import gaussian

pytestmark = pytest.mark.gpu
ATOL = 1e-10            # tests/test_gpu_allow.py's tolerance against the oracle
TDT = {"f64": torch.float64, "f32": torch.float32, "bf16": torch.bfloat16}
CATS = {"f64": (2269, 32), "f32": (4099, 64), "bf16": (1500, 100)}
ZERO_ROW = 7            # a zero-norm catalog row (score 0), allowed in masks 0 and 1
N_MASKS = 9


def _pack(flags, words):
    by = np.packbits(np.asarray(flags, dtype=np.uint8), bitorder="little")
    out = np.zeros(words * 4, dtype=np.uint8)
    out[:by.size] = by
    return out.view("<u4")


# ---- 1. the kernel alone ------------------------------------------------------------------------
def _kernel_flags(n, col_begin, rows, rng):
    """empty, full, a single row, the last row only, two identical masks, density 0.5"""
    single = np.zeros(rows, bool)
    single[col_begin + n // 2] = True
    last = np.zeros(rows, bool)
    last[col_begin + n - 1] = True
    twin = rng.random(rows) < 0.3
    return np.stack([np.zeros(rows, bool), np.ones(rows, bool), single, last, twin, twin.copy(),
                     rng.random(rows) < 0.5])


def _kernel_scores(B, n, ld, rng):
    """Random f32 with -inf, NaN and runs of 40 equal values that cross the boundary between
    the segments of segs = 3 (and, at n = 4100, the 4096-entry tile); the padding up to ld holds
    a value larger than every score, which must never be selected."""
    v = rng.standard_normal((B, ld)).astype(np.float32)
    v[:, n:] = np.float32(1e9)
    if n >= 63:
        v[:, rng.choice(n, n // 16, replace=False)] = -np.inf
        v[:, rng.choice(n, n // 16, replace=False)] = np.nan
    if n >= 1000:
        seg_len = (-(-n // 3) + 3) // 4 * 4
        for b in range(B):
            v[b, seg_len - 20 - b:seg_len + 20 - b] = np.float32(2.5)        # above everything
            v[b, 2 * seg_len - 20:2 * seg_len + 20] = np.float32(0.25 * b)   # in the middle
    if n > 4096:
        v[:, n - 40:n] = np.float32(3.0)
    return v


@pytest.mark.parametrize("col_begin", [0, 96, 1028])
@pytest.mark.parametrize("n", [1, 63, 1000, 4100])
def test_select_kernel_equals_numpy(cuda_device, n, col_begin):
    from robot_ebert_amd import _lib
    lib = _lib.load()
    dev = cuda_device
    B = 3
    ld = (n + 3) // 4 * 4
    rng = np.random.default_rng(100 * n + col_begin)
    words = int(lib.ebt_allow_words(col_begin + n))
    flags = _kernel_flags(n, col_begin, 32 * words, rng)
    M = flags.shape[0]
    table = torch.from_numpy(np.stack([_pack(f, words) for f in flags]).view(np.int32)).to(dev)
    v = _kernel_scores(B, n, ld, rng)
    d_v = torch.from_numpy(v).to(dev)
    cycle = [6, 1, 0, 2, 3, 4, 5, -1, M, 6, M + 100, -7]      # a repeat, ids outside the table
    assert lib.ebt_grouped_pass_groups(512) < 64               # G = 64: more than one launch
    for G in (1, 5, 64):
        groups = [cycle[i % len(cycle)] for i in range(G)]
        d_g = torch.tensor(groups, dtype=torch.int32, device=dev)
        for kprime in (1, 8, 512):
            for segs in (1, 3):
                ld_out = segs * kprime
                ov = torch.full((G, B, ld_out), 77.0, dtype=torch.float32, device=dev)
                oi = torch.full((G, B, ld_out), -77, dtype=torch.int64, device=dev)
                _lib.call("ebt_select_topk_grouped", d_v.data_ptr(), ld, B, n, col_begin,
                          table.data_ptr(), words, M, d_g.data_ptr(), G, kprime, segs,
                          ov.data_ptr(), oi.data_ptr(), ld_out, _lib.stream_of(dev))
                wv, wi = select_ref(v, n, col_begin, flags, groups, kprime, segs)
                what = (G, kprime, segs)
                np.testing.assert_array_equal(oi.cpu().numpy(), wi, err_msg=str(what))
                assert np.array_equal(ov.cpu().numpy().view(np.uint32), wv.view(np.uint32)), what


# ---- 2. the whole path --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _host_catalog(kind):
    n, d = CATS[kind]
    c = gaussian(1, n, d, kind)
    c[ZERO_ROW] = 0.0
    return c


_CACHE = {}


def _catalog(kind, dev):
    import robot_ebert_amd as ebt
    if ("cat", kind) not in _CACHE:
        c = torch.from_numpy(np.ascontiguousarray(_host_catalog(kind))).to(dev).to(TDT[kind])
        _CACHE[("cat", kind)] = ebt.Catalog(c)
    return _CACHE[("cat", kind)]


@functools.lru_cache(maxsize=None)
def _flags(kind):
    """Nine overlapping masks: densities 0.4, 0.3, 0.1; an empty one (3); five rows (4: fewer
    than k = 10); the rest 0.2. The zero-norm row is in masks 0 and 1."""
    n = CATS[kind][0]
    rng = np.random.default_rng(11)
    f = [rng.random(n) < p for p in (0.4, 0.3, 0.1)]
    f.append(np.zeros(n, bool))
    five = np.zeros(n, bool)
    five[rng.choice(n, 5, replace=False)] = True
    f.append(five)
    f += [rng.random(n) < 0.2 for _ in range(N_MASKS - 5)]
    f[0][ZERO_ROW] = f[1][ZERO_ROW] = True
    return np.stack(f)


def _masks(kind, dev):
    import robot_ebert_amd as ebt
    if ("masks", kind) not in _CACHE:
        m = ebt.AllowMasks(_catalog(kind, dev), N_MASKS, names=[f"g{i}" for i in range(N_MASKS)])
        for i, f in enumerate(_flags(kind)):
            m.from_bool(i, torch.from_numpy(f).to(dev))
        _CACHE[("masks", kind)] = m
    return _CACHE[("masks", kind)]


def _groups(G):
    """Overlapping masks, the empty one, the five-row one, an id >= n_masks, a negative id and a
    repeated id (G >= 7); by name and by index."""
    base = ["g0", 1, 3, 4, N_MASKS + 2, -1, 1, 2, 5, "g6", 7, 8]
    return [base[i % len(base)] for i in range(G)]


def _request(kind, B, qkind, dev):
    """(score_topk keyword arguments, oracle scores [B, n], exclusion lists that overlap the
    groups and hold every liked row: two liked rows of one user tie exactly)."""
    n, d = CATS[kind]
    c = _host_catalog(kind)
    rng = np.random.default_rng(1000 + B)
    if qkind == "dense":
        q = gaussian(2, B, d, "f32").astype(np.float32)
        kw = dict(queries=torch.from_numpy(q).to(dev))
        S = scores64(c, queries=q)
        liked = [[] for _ in range(B)]
    else:
        liked = [sorted(rng.choice(n, 2 + b % 4, replace=False).tolist()) for b in range(B)]
        kw = dict(liked=liked)
        w = None
        if qkind == "weighted":
            w = [[(-0.5 if i == 1 else 1.0 + 0.25 * i) for i in range(len(l))] for l in liked]
            kw["liked_weights"] = w
        S = scores64(c, liked=liked, liked_weights=w)
    excl = [sorted(set(range(b % 50, n, 97)) | set(l)) for b, l in enumerate(liked)]
    kw["exclude"] = excl
    return kw, S, excl


def _masked_path(cat, masks, ids, k, B, dev, **kw):
    """The existing code, one call per distinct mask id: ([B, G, k] scores, rows)."""
    import robot_ebert_amd as ebt
    per = {}
    for m in set(ids):
        per[m] = ebt.score_topk(cat, k, allow=(masks, torch.full((B,), m, dtype=torch.int32,
                                                                 device=dev)), **kw)
    return (torch.stack([per[m][0] for m in ids], 1), torch.stack([per[m][1] for m in ids], 1))


def _bitwise(got, want):
    assert torch.equal(got.rows, want[1]), "rows differ"
    assert torch.equal(got.scores.view(torch.int64), want[0].view(torch.int64)), \
        "scores differ bitwise"


# one combination of (queries, k, chunk_rows, G) per line; together they cover every value
COMBOS = [("dense", 10, None, 7), ("liked", 1, 1024, 1), ("weighted", 10, 1024, 33),
          ("liked", 40, None, 7), ("dense", 1, 1024, 7)]


@pytest.mark.parametrize("B", [1, 3, 130])
@pytest.mark.parametrize("kind", ["f64", "f32", "bf16"])
def test_equals_masked_path_and_oracle(cuda_device, kind, B):
    import robot_ebert_amd as ebt
    from robot_ebert_amd.grouped import resolve_groups
    dev = cuda_device
    cat, masks, flags = _catalog(kind, dev), _masks(kind, dev), _flags(kind)
    for qkind, k, chunk_rows, G in COMBOS:
        what = (qkind, k, chunk_rows, G)
        kw, S, excl = _request(kind, B, qkind, dev)
        groups = _groups(G)
        ids = resolve_groups(masks, groups)
        got = ebt.score_topk_grouped(cat, k, masks, groups, chunk_rows=chunk_rows, **kw)
        assert got.scores.shape == (B, G, k) and got.rows.shape == (B, G, k), what
        assert got.scores.dtype == torch.float64 and got.rows.dtype == torch.int64
        assert got.group.tolist() == ids and got.group.dtype == torch.int32
        _bitwise(got, _masked_path(cat, masks, ids, k, B, dev, chunk_rows=chunk_rows, **kw))
        s_ref, r_ref = grouped_ref(S, flags, ids, k, excl)
        r, s = got.rows.cpu().numpy(), got.scores.cpu().numpy()
        np.testing.assert_array_equal(r, r_ref, err_msg=str(what))
        m = r_ref >= 0
        np.testing.assert_allclose(s[m], s_ref[m], rtol=0, atol=ATOL, err_msg=str(what))
        assert np.isnan(s[~m]).all(), what
        if G >= 7:      # the empty mask, the id past the table; the five-row group is short
            assert (r[:, 2] == -1).all() and (r[:, 4] == -1).all()
            assert ((r[:, 3] >= 0).sum(axis=1) <= min(k, 5)).all()
            assert (r[:, 1] == r[:, 6]).all()                       # the repeated id


def test_zero_norm_row_inside_a_group(cuda_device):
    """A group of three rows, one of them zero-norm: it is returned with score exactly 0, in
    (score descending, row ascending) order among the others."""
    import robot_ebert_amd as ebt
    dev = cuda_device
    cat = _catalog("f32", dev)
    masks = ebt.AllowMasks(cat, 1)
    masks.set(0, [ZERO_ROW, 100, 200])
    kw, S, _ = _request("f32", 3, "dense", dev)
    got = ebt.score_topk_grouped(cat, 3, masks, [0], queries=kw["queries"])
    r, s = got.rows[:, 0].cpu().numpy(), got.scores[:, 0].cpu().numpy()
    assert (np.sort(r, axis=1) == [ZERO_ROW, 100, 200]).all()
    assert (s[r == ZERO_ROW] == 0.0).all() and (np.diff(s, axis=1) <= 0).all()
    _bitwise(got, _masked_path(cat, masks, [0], 3, 3, dev, queries=kw["queries"]))


# ---- 3. nothing hides behind the fallback -------------------------------------------------------
def _first_pass(cat, masks, qb, ids, k, kp, chunk, excl, dev, timer=None):
    """ebt_cosine_topk_grouped_prepared alone: (scores, rows, certified), each [G, B, ...]."""
    from robot_ebert_amd import _lib, search
    lib = _lib.load()
    G, B = len(ids), qb.B
    need = int(lib.ebt_cosine_topk_grouped_workspace(B, qb.B_pad, cat.n, kp, chunk, 0, G))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    s = torch.empty((G, B, k), dtype=torch.float64, device=dev)
    r = torch.empty((G, B, k), dtype=torch.int64, device=dev)
    c = torch.full((G, B), 99, dtype=torch.int32, device=dev)
    gid = torch.tensor(ids, dtype=torch.int32, device=dev)
    _lib.call("ebt_cosine_topk_grouped_prepared",
              *search._pipe_operands(cat, qb, excl, k, kp, chunk, 0), gid.data_ptr(), G,
              masks.table.data_ptr(), masks.words, masks.n_masks, ws.data_ptr(), need,
              s.data_ptr(), r.data_ptr(), c.data_ptr(),
              timer.handle if timer is not None else None, _lib.stream_of(dev))
    return s, r, c


@pytest.mark.parametrize("chunk", [1024, 4224])
@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_first_pass_certificates_equal_the_masked_pipeline(cuda_device, kind, chunk):
    """Same chunk_rows and k': certified[g][b] -- and the rows and scores with it -- equal what
    run_pipeline(flags=EBT_FLAG_NO_FUSE, allow=(masks, [g] * B)) returns. k' = 12 leaves two
    rows of slack beside k = 10: wherever the masked pipeline cannot certify, the certificate
    must be 0 here too (the tie-cluster test below forces such a pair)."""
    from robot_ebert_amd import _lib, search
    dev = cuda_device
    cat, masks = _catalog(kind, dev), _masks(kind, dev)
    B, k, kp = 130, 10, 12
    kw, _, excl = _request(kind, B, "dense", dev)
    qb = search.prepare_queries(cat, queries=kw["queries"])
    ex = search.csr_from_lists(excl, dev)
    ids = [0, 1, 3, 4, N_MASKS + 2, -1, 1, 2]
    s, r, c = _first_pass(cat, masks, qb, ids, k, kp, chunk, ex, dev)
    seen = set()
    for g, m in enumerate(ids):
        d_ids = torch.full((B,), m, dtype=torch.int32, device=dev)
        s2, r2, c2 = search.run_pipeline(cat, qb, k, kp, ex, chunk_rows=chunk,
                                         flags=_lib.EBT_FLAG_NO_FUSE, allow=(masks, d_ids))
        assert torch.equal(c[g], c2), (m, c[g].tolist(), c2.tolist())
        assert torch.equal(r[g], r2) and torch.equal(s[g].view(torch.int64), s2.view(torch.int64))
        seen |= set(c2.tolist())
    assert seen <= {0, 1} and 1 in seen


@pytest.mark.parametrize("chunk,launches", [
    (128, {"gemm": 8, "mask": 8, "select": 8, "merge_select": 1, "rescore": 1}),
    (1024, {"gemm": 1, "mask": 1, "select": 1, "merge_select": 0, "rescore": 1})])
def test_timer_records_one_stage_per_launch_group(cuda_device, chunk, launches):
    """A Timer on one grouped call, 1000 rows in eight chunks of 128 or in one: every chunk is
    one record each of the screening GEMM, the exclusion mask and the grouped select (G = 3 fits
    one launch), the per-chunk lists are merged once (not at all when there is one list), and the
    G rescores are one record. The timer changes no output bit."""
    import robot_ebert_amd as ebt
    from robot_ebert_amd import _lib, search
    dev = cuda_device
    n, d, B, k, kp = 1000, 64, 4, 10, 32
    cat = ebt.Catalog(torch.from_numpy(gaussian(41, n, d, "f32").astype(np.float32)).to(dev))
    rng = np.random.default_rng(42)
    masks = ebt.AllowMasks(cat, 3)
    for i, p in enumerate((0.5, 0.2, 0.05)):
        masks.from_bool(i, torch.from_numpy(rng.random(n) < p).to(dev))
    q = torch.from_numpy(gaussian(43, B, d, "f32").astype(np.float32)).to(dev)
    qb = search.prepare_queries(cat, queries=q)
    ex = search.csr_from_lists([list(range(b, n, 97)) for b in range(B)], dev)
    plain = _first_pass(cat, masks, qb, [0, 1, 2], k, kp, chunk, ex, dev)
    timer = _lib.Timer()
    timed = _first_pass(cat, masks, qb, [0, 1, 2], k, kp, chunk, ex, dev, timer=timer)
    torch.cuda.synchronize(dev)
    got = {}
    for stage in launches:
        ms, got[stage] = timer.query(stage)
        assert np.isfinite(ms) and ms >= 0.0, (stage, ms)
    assert got == launches
    for stage in set(_lib.STAGES) - set(launches):
        assert timer.query(stage)[1] == 0, stage
    assert torch.equal(timed[0].view(torch.int64), plain[0].view(torch.int64))
    assert torch.equal(timed[1], plain[1]) and torch.equal(timed[2], plain[2])
    assert (plain[2] != 99).all() and (plain[1][:, :, 0] >= 0).all()


# ---- 4. the fallback itself ---------------------------------------------------------------------
def test_tie_cluster_wider_than_kprime_takes_the_fallback(cuda_device):
    """40 identical rows straddle the 1024-row chunk boundary inside one group; the query is that
    vector and k' = 16: the first pass cannot certify (more than k' rows tie with the k-th), the
    pair is re-run through the masked path and the answer is rows 1000..1009 in row order."""
    import robot_ebert_amd as ebt
    dev = cuda_device
    c = _host_catalog("f32").copy()
    c[1000:1040] = c[1000]
    cat = ebt.Catalog(torch.from_numpy(c).to(dev))
    n = c.shape[0]
    rng = np.random.default_rng(5)
    f = rng.random(n) < 0.3
    f[1000:1040] = True
    masks = ebt.AllowMasks(cat, 3)
    masks.from_bool(0, torch.from_numpy(f).to(dev))
    masks.from_bool(1, torch.from_numpy(rng.random(n) < 0.3).to(dev))     # mask 2 stays empty
    q = torch.from_numpy(np.stack([c[1000], c[5]]).astype(np.float32)).to(dev)
    got = ebt.score_topk_grouped(cat, 10, masks, [0, 1, 2], queries=q, kprime=16, chunk_rows=1024)
    assert got.fallback >= 1
    assert got.rows[0, 0].tolist() == list(range(1000, 1010))
    _bitwise(got, _masked_path(cat, masks, [0, 1, 2], 10, 2, dev, queries=q, kprime=16,
                               chunk_rows=1024))
    empty = ebt.score_topk_grouped(cat, 10, masks, [2, 7, 2], queries=q, kprime=16,
                                   chunk_rows=1024)
    assert empty.fallback == 0 and (empty.rows == -1).all() and torch.isnan(empty.scores).all()


# ---- 5. invariances -----------------------------------------------------------------------------
def test_permuting_and_splitting_the_groups_changes_no_bit(cuda_device):
    import robot_ebert_amd as ebt
    dev = cuda_device
    cat, masks = _catalog("f32", dev), _masks("f32", dev)
    kw, _, _ = _request("f32", 3, "liked", dev)
    groups = _groups(12)
    base = ebt.score_topk_grouped(cat, 10, masks, groups, chunk_rows=1024, **kw)
    perm = np.random.default_rng(3).permutation(len(groups)).tolist()
    got = ebt.score_topk_grouped(cat, 10, masks, [groups[i] for i in perm], chunk_rows=1024, **kw)
    assert torch.equal(got.rows, base.rows[:, perm])
    assert torch.equal(got.scores.view(torch.int64), base.scores[:, perm].view(torch.int64))
    assert got.group.tolist() == [base.group.tolist()[i] for i in perm]
    for budget in (1, 40000):                       # one group per call, a few groups per call
        split = ebt.score_topk_grouped(cat, 10, masks, groups, chunk_rows=1024, ws_budget=budget,
                                       **kw)
        _bitwise(split, (base.scores, base.rows))


def test_catalog_and_mask_edits_are_seen(cuda_device):
    import robot_ebert_amd as ebt
    dev = cuda_device
    c = _host_catalog("f32").copy()
    cat = ebt.Catalog(torch.from_numpy(c).to(dev))
    masks = ebt.AllowMasks(cat, 2)
    masks.set(0, list(range(0, 4099, 3)))
    masks.set(1, list(range(1, 4099, 3)))
    q = torch.from_numpy(gaussian(9, 2, 64, "f32").astype(np.float32)).to(dev)
    before = ebt.score_topk_grouped(cat, 5, masks, [0, 1], queries=q)
    _bitwise(before, _masked_path(cat, masks, [0, 1], 5, 2, dev, queries=q))
    # row 301 (mask 1: 301 % 3 == 1) becomes query 0's vector; row 302 joins mask 0
    cat.update_rows([301], q[:1])
    masks.set(0, [302])
    after = ebt.score_topk_grouped(cat, 5, masks, [0, 1], queries=q)
    assert after.rows[0, 1, 0].item() == 301 and abs(after.scores[0, 1, 0].item() - 1.0) < 1e-6
    _bitwise(after, _masked_path(cat, masks, [0, 1], 5, 2, dev, queries=q))
    c[301] = q[0].cpu().numpy()
    f = np.zeros((2, 4099), bool)
    f[0, 0::3] = f[1, 1::3] = True
    f[0, 302] = True
    s_ref, r_ref = grouped_ref(scores64(c, queries=q.cpu().numpy()), f, [0, 1], 5)
    np.testing.assert_array_equal(after.rows.cpu().numpy(), r_ref)
    np.testing.assert_allclose(after.scores.cpu().numpy(), s_ref, rtol=0, atol=ATOL)
