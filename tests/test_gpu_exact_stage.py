"""Contract tests for the exact stage: rescore, certificate, two-phase and cut kernels.

Every exactness claim rests on the screening bound |approx - exact| <= eps (tested in
test_gpu_certificate.py) and on the decision logic that turns approx scores, eps and t_floor into
a gather set and a certificate. The pipeline heals a conservative mistake end to end (a wrong 0 or
-1 is retried, a rescore that gathers too much still returns the right rows), so the decision
logic is pinned here at kernel level against a float64 numpy model written from the text of
include/ebert.h (ebt_rescore, ebt_rescore_owned, ebt_finalize_topk, ebt_certify_cut), not from
the kernels:

  valid     0 <= row < n_rows; any row >= n_rows gives certified = -2
  cut       max(cv[k-1] - 2 eps, t_floor - eps)
  kept      valid and not (cv < cut)
  cut2      max(cut, s_min - eps) if eps > 0 and the first k positions are all kept
            (s_min = their smallest exact score), else cut
  gathered  kept at positions < k, plus kept at positions >= k with not (cv < cut2)
  output    the k best of the gathered set by (exact desc, row asc), rows + row_offset, NaN / -1
  cert      1 if nvalid < k' or n_rows <= k', else 1 iff cv[k'-1] < cut2

`cut` is the same float64 expression on both sides (bit-identical); only s_min can differ from
numpy's by float64 round-off, so a generated case with some cv within CUT_GUARD of a raised cut2
(or of cut) is reseeded on the host; the explicit boundary cases sit exactly on `cut`.
Catalog tensors carry GUARD_ROWS extra rows (and the padding columns) filled with 1e30: a wrongly
read row >= n_rows shows in the output instead of reading outside an allocation.
"""
import numpy as np
import pytest
import torch

from inputs import gaussian
from oracle import restatement as R

gpu = pytest.mark.gpu
TORCH_DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "f64": torch.float64}
SCORE_ATOL = 1e-12   # float64 rescore vs float64 reference (tests/test_gpu_workloads.py)
CUT_GUARD = 1e-6     # no generated cv this close to cut / cut2 (GPU s_min: float64 round-off only)
TIE_GUARD = 1e-9     # no two gathered exact scores this close, declared duplicates apart
GUARD_ROWS = 8
GUARD_FILL = 1e30
N_CAT = 2048


# ------------------------------------------------------------------------------ the model ----
class Verdict:
    """The contract's answer for one query."""

    def __init__(self, out_s, out_r, cert, gathered, cut, cut2, kept):
        self.out_s, self.out_r, self.cert = out_s, out_r, cert
        self.gathered, self.cut, self.cut2, self.kept = gathered, cut, cut2, kept

    @property
    def n_gathered(self):
        return int(self.gathered.sum())

    @property
    def n_kept(self):
        return int(self.kept.sum())


def contract_model(cv, rows, exact, k, n_rows, eps, t_floor=None, row_offset=0, rise=True):
    """One query. cv: float32 [k'] approx scores; rows: int64 [k'] (LOCAL, -1 empty); exact:
    float64 [k'] exact score of each position's row (ignored where the row is not valid)."""
    cv = np.asarray(cv, dtype=np.float32).astype(np.float64)
    rows = np.asarray(rows, dtype=np.int64)
    exact = np.asarray(exact, dtype=np.float64)
    kp = cv.shape[0]
    eps = float(np.float32(eps))
    valid = (rows >= 0) & (rows < n_rows)
    corrupt = bool(np.any(rows >= n_rows))
    cut = cv[k - 1] - 2.0 * eps
    if t_floor is not None and float(t_floor) - eps > cut:
        cut = float(t_floor) - eps
    kept = valid & ~(cv < cut)
    cut2 = cut
    if rise and eps > 0 and bool(kept[:k].all()):
        s_min = float(exact[:k].min())
        if s_min - eps > cut2:
            cut2 = s_min - eps
    pos = np.arange(kp)
    gathered = kept & ((pos < k) | ~(cv < cut2))
    g = np.flatnonzero(gathered)
    o = g[np.lexsort((rows[g], -exact[g]))][:k]
    out_s = np.full(k, np.nan)
    out_r = np.full(k, -1, dtype=np.int64)
    out_s[:o.size] = exact[o]
    out_r[:o.size] = rows[o] + row_offset
    if corrupt:
        cert = -2
    elif int(valid.sum()) < kp or n_rows <= kp:
        cert = 1
    else:
        cert = 1 if cv[kp - 1] < cut2 else 0
    return Verdict(out_s, out_r, cert, gathered, cut, cut2, kept)


def well_separated(v, cv, exact, eps, dup_ok=False, boundary=False):
    """No valid cv within CUT_GUARD of cut2 (nor of cut when eps > 0; eps = 0 puts cv[k-1] on
    the cut by definition, an explicit boundary) and no near-tie among the gathered scores
    (cv, exact: the k' positions of the list)."""
    c = np.asarray(cv, dtype=np.float32).astype(np.float64)
    c = c[np.isfinite(c)]
    if float(np.float32(eps)) > 0 and not boundary:
        if np.any(np.abs(c - v.cut) < CUT_GUARD) or np.any(np.abs(c - v.cut2) < CUT_GUARD):
            return False
    if not dup_ok:
        e = np.sort(np.asarray(exact, dtype=np.float64)[v.gathered])
        if e.size > 1 and np.min(np.diff(e)) < TIE_GUARD:
            return False
    return True


def test_contract_model_is_sound():
    """The soundness argument as executable code (no GPU): with |approx - exact| <= eps and the
    list = the k' best approx of the whole catalog, whenever the model certifies, its output is
    the brute-force top k of the whole catalog; and the grid holds uncertified queries (k' = k
    can never certify on a catalog larger than k')."""
    n, d, B = 2000, 32, 32
    rng = np.random.default_rng(11)
    cat = rng.standard_normal((n, d))
    q = rng.standard_normal((B, d))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    exact = (q @ cat.T) / np.linalg.norm(cat, axis=1)
    n_cert = n_not = 0
    not_at_k = {}
    for eps in (np.float32(0.004), np.float32(0.03)):
        # |approx32 - exact| <= eps: noise within eps - 1e-6, float32 rounding of |s| <= 1 is 6e-8
        noise = rng.uniform(-1.0, 1.0, exact.shape) * (float(eps) - 1e-6)
        approx = (exact + noise).astype(np.float32)
        assert np.all(np.abs(approx.astype(np.float64) - exact) <= float(eps))
        order = np.lexsort((np.broadcast_to(np.arange(n), exact.shape),
                            -approx.astype(np.float64)), axis=1)
        for k in (1, 20):
            for kp in (k, 64, 300):
                for with_floor in (False, True):
                    for b in range(B):
                        rows = order[b, :kp]
                        cv = approx[b, rows]
                        # a valid floor: k rows have exact >= approx - eps >= cv[k-1] - eps
                        tf = float(cv[k - 1]) - float(eps) if with_floor else None
                        v = contract_model(cv, rows, exact[b, rows], k, n, eps, t_floor=tf)
                        if v.cert == 1:
                            n_cert += 1
                            top = np.lexsort((np.arange(n), -exact[b]))[:k]
                            np.testing.assert_array_equal(v.out_r, top)
                            np.testing.assert_array_equal(v.out_s, exact[b, top])
                        else:
                            assert v.cert == 0
                            n_not += 1
                            not_at_k[(k, kp)] = not_at_k.get((k, kp), 0) + 1
    assert n_cert > 0 and n_not > 0
    for k in (1, 20):
        assert not_at_k.get((k, k), 0) == 4 * B   # k' = k: every query, both eps, both floors


# ---------------------------------------------------------------------------- GPU helpers ----
def _L():
    from robot_ebert_amd import _lib
    return _lib


class DevCatalog:
    """n rows of d elements of `dt`, row stride ld, plus GUARD_ROWS rows; padding columns and
    guard rows hold 1e30. Host side: the float64 values and their float64 norms."""

    def __init__(self, dev, dt, d, ld=None, n=N_CAT, seed=1, dup=()):
        self.dt, self.d, self.ld, self.n, self.dev = dt, d, ld or d, n, dev
        self.host = gaussian(seed, n, d, dt)
        for dst, src in dup:
            self.host[dst] = self.host[src]
        self.gnorm = np.linalg.norm(self.host, axis=1)
        full = np.full((n + GUARD_ROWS, self.ld), GUARD_FILL, dtype=np.float64)
        full[:n, :d] = self.host
        self.t = torch.from_numpy(full).to(dev).to(TORCH_DT[dt]).contiguous()
        g = np.concatenate([self.gnorm, np.ones(GUARD_ROWS)])
        self.g = torch.from_numpy(g).to(dev)

    def exact(self, q64, dup=()):
        e = (q64 @ self.host.T) / self.gnorm
        for dst, src in dup:
            e[:, dst] = e[:, src]   # bit-identical rows score bit-identically
        return e

    def shard(self, lo, hi):
        """Rows [lo, hi) as a catalog of their own (with its own guard rows)."""
        s = object.__new__(DevCatalog)
        s.dt, s.d, s.ld, s.n, s.dev = self.dt, self.d, self.ld, hi - lo, self.dev
        s.host, s.gnorm = self.host[lo:hi], self.gnorm[lo:hi]
        full = np.full((s.n + GUARD_ROWS, s.ld), GUARD_FILL, dtype=np.float64)
        full[:s.n, :s.d] = s.host
        s.t = torch.from_numpy(full).to(self.dev).to(TORCH_DT[self.dt]).contiguous()
        s.g = torch.from_numpy(np.concatenate([s.gnorm, np.ones(GUARD_ROWS)])).to(self.dev)
        return s


def unit_queries(seed, B, d):
    q = np.random.default_rng(seed).standard_normal((B, d))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


_TIMER = {}


def _timer():
    if "t" not in _TIMER:
        t = _L().Timer()
        t.count_rows(True)
        _TIMER["t"] = t
    return _TIMER["t"]


def run_rescore(cat, q64, cv, rows, k, eps, t_floor=None, row_offset=0, n_rows=None):
    """ebt_rescore on a batch -> (scores, rows, cert, rows gathered by the kernel). No row
    passed here may lie outside the allocation of n + GUARD_ROWS rows."""
    L = _L()
    dev = cat.dev
    B, kp = cv.shape
    n_rows = cat.n if n_rows is None else n_rows
    assert rows.max() < cat.n + GUARD_ROWS and n_rows <= cat.n
    qt = torch.from_numpy(np.ascontiguousarray(q64)).to(dev)
    cvt = torch.from_numpy(np.ascontiguousarray(cv, dtype=np.float32)).to(dev)
    rt = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int64)).to(dev)
    et = torch.from_numpy(np.ascontiguousarray(eps, dtype=np.float32)).to(dev)
    tf = None if t_floor is None else torch.from_numpy(
        np.ascontiguousarray(t_floor, dtype=np.float64)).to(dev)
    out_s = torch.full((B, k), 777.0, dtype=torch.float64, device=dev)
    out_r = torch.full((B, k), -7, dtype=torch.int64, device=dev)
    cert = torch.full((B,), 99, dtype=torch.int32, device=dev)
    t = _timer()
    torch.cuda.synchronize(dev)
    t.reset()
    L.call("ebt_rescore", L.ptr(qt), B, cat.d, L.ptr(cat.t), L.DTYPE_CODE[TORCH_DT[cat.dt]],
           cat.ld, L.ptr(cat.g), row_offset, L.ptr(cvt), L.ptr(rt), kp, k, n_rows, L.ptr(et),
           L.ptr(tf), L.ptr(out_s), L.ptr(out_r), L.ptr(cert), t.handle, L.stream_of(dev))
    torch.cuda.synchronize(dev)
    return out_s.cpu().numpy(), out_r.cpu().numpy(), cert.cpu().numpy(), t.rows()


def model_batch(cv, rows, exact_all, k, n_rows, eps, t_floor=None, row_offset=0, rise=True):
    out = []
    for b in range(cv.shape[0]):
        r = rows[b]
        ex = np.where((r >= 0) & (r < n_rows), exact_all[b, np.clip(r, 0, n_rows - 1)], np.nan)
        out.append(contract_model(cv[b], r, ex, k, n_rows, eps[b],
                                  None if t_floor is None else t_floor[b], row_offset, rise))
    return out


def assert_matches(vs, s, r, cert, counted):
    """Rows and certificate equal, scores within SCORE_ATOL (NaN slots alike), gathered count
    equal. Figures are printed before the count is asserted (pytest -s shows them)."""
    for b, v in enumerate(vs):
        np.testing.assert_array_equal(r[b], v.out_r, err_msg=f"rows of query {b}")
        np.testing.assert_allclose(s[b], v.out_s, rtol=0, atol=SCORE_ATOL, equal_nan=True,
                                   err_msg=f"scores of query {b}")
        assert int(cert[b]) == v.cert, (b, int(cert[b]), v.cert, v.cut, v.cut2)
    want = sum(v.n_gathered for v in vs)
    print(f"gathered: kernel {counted}, model {want}; kept {[v.n_kept for v in vs]}")
    assert counted == want, (counted, want, [v.n_gathered for v in vs])


def screened_lists(exact_all, k, kp, eps, seed, noise=1.5, dup_ok=False):
    """Lists as a screen would leave them, sorted by approx desc: approx = exact + noise * eps *
    U(-1, 1) (noise > 1: the contract does not need the screen's bound), the k' best approx.
    Reseeded until every query is well separated from its cuts."""
    B, n = exact_all.shape
    eps = np.asarray(eps, dtype=np.float32)
    for attempt in range(50):
        rng = np.random.default_rng(seed + 1000 * attempt)
        approx = (exact_all + noise * eps[:, None].astype(np.float64) *
                  rng.uniform(-1.0, 1.0, exact_all.shape)).astype(np.float32)
        rows = np.lexsort((np.broadcast_to(np.arange(n), approx.shape),
                           -approx.astype(np.float64)), axis=1)[:, :kp].astype(np.int64)
        cv = np.take_along_axis(approx, rows, 1)
        vs = model_batch(cv, rows, exact_all, k, n, eps)
        if all(well_separated(v, cv[b], exact_all[b, rows[b]], eps[b], dup_ok)
               for b, v in enumerate(vs)):
            return cv, rows
    raise AssertionError("no well-separated case in 50 seeds")


_SHARED = {}


def shared_case(dev, dt, d, ld=None):
    """One catalog, query batch and float64 exact matrix per (dtype, d, ld): built once."""
    key = (dt, d, ld)
    if key not in _SHARED:
        cat = DevCatalog(dev, dt, d, ld, seed=100 + d)
        q64 = unit_queries(200 + d, 5, d)
        _SHARED[key] = (cat, q64, cat.exact(q64))
    return _SHARED[key]


EPS5 = np.array([0.002, 0.01, 0.02, 0.05, 0.1], dtype=np.float32)


# ------------------------------------------------------------- 2. ebt_rescore vs the model ----
@gpu
@pytest.mark.parametrize("dt,d,ld", [("f32", 64, 64), ("bf16", 64, 64), ("f16", 64, 64),
                                     ("f64", 64, 64), ("f32", 64, 96), ("bf16", 64, 96),
                                     ("f32", 77, 77), ("bf16", 100, 100)])
def test_rescore_dtype_layout(cuda_device, dt, d, ld):
    """Every element type on the 16-byte path (ld = d and ld > d) and the element-wise path
    (rows that are no 16-byte multiple), with and without a row offset."""
    cat, q64, exact = shared_case(cuda_device, dt, d, ld)
    k, kp = 20, 64
    cv, rows = screened_lists(exact, k, kp, EPS5, seed=d + ld)
    for off in (0, 123457):
        vs = model_batch(cv, rows, exact, k, cat.n, EPS5, row_offset=off)
        assert_matches(vs, *run_rescore(cat, q64, cv, rows, k, EPS5, row_offset=off))
    assert {v.cert for v in vs} == {0, 1}   # the five eps reach both answers


@gpu
@pytest.mark.parametrize("k,kp,eps,lo,hi", [
    (20, 64, EPS5, 1, 128),                                   # nk <= 128: two threads per row
    (1, 64, EPS5, 1, 128),
    (20, 20, EPS5, 1, 128),                                   # k' = k
    (1, 1, EPS5, 1, 128),
    (20, 300, EPS5 * 2, 129, 512),                            # 128 < nk <= 512: one per row
    (100, 512, EPS5 * 2, 129, 512),
])
def test_rescore_ordering_paths(cuda_device, k, kp, eps, lo, hi):
    """The ordering paths by kept count nk, on screened lists; the widest query's nk must lie in
    [lo, hi] (a check of the construction)."""
    cat, q64, exact = shared_case(cuda_device, "f32", 64)
    cv, rows = screened_lists(exact, k, kp, eps, seed=7 * k + kp)
    vs = model_batch(cv, rows, exact, k, cat.n, eps)
    assert lo <= max(v.n_kept for v in vs) <= hi
    assert_matches(vs, *run_rescore(cat, q64, cv, rows, k, eps))


@gpu
@pytest.mark.parametrize("k,kp", [(20, 128), (20, 129), (100, 512), (100, 513), (600, 1024)])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_rescore_every_candidate(cuda_device, dt, k, kp):
    """eps = 0 with equal cand_vals rescores every candidate: nk = k' on both sides of each
    ordering threshold (128 / 129, 512 / 513) and on the bitonic path (k' = 1024, k = 600).
    Random rows in random order; one query has a -1 tail (nvalid < k')."""
    cat, q64, exact = shared_case(cuda_device, dt, 64)
    B = q64.shape[0]
    rng = np.random.default_rng(kp)
    rows = np.stack([rng.permutation(cat.n)[:kp] for _ in range(B)]).astype(np.int64)
    cv = np.full((B, kp), 0.25, dtype=np.float32)
    rows[1, kp - 5:] = -1
    cv[1, kp - 5:] = -np.inf
    eps = np.zeros(B, dtype=np.float32)
    vs = model_batch(cv, rows, exact, k, cat.n, eps)
    assert [v.n_kept for v in vs] == [kp, kp - 5, kp, kp, kp]
    assert [v.cert for v in vs] == [0, 1, 0, 0, 0]
    assert all(well_separated(v, cv[b], exact[b, np.clip(rows[b], 0, None)], 0.0)
               for b, v in enumerate(vs))
    assert_matches(vs, *run_rescore(cat, q64, cv, rows, k, eps))


@gpu
@pytest.mark.parametrize("dt,k,kp", [("f32", 20, 64), ("bf16", 20, 300), ("f64", 100, 1024)])
def test_rescore_query_forms_bitwise(cuda_device, dt, k, kp):
    """ebt_rescore_form(1) (query in registers) and (0) (query in LDS): outputs, certificates
    and gathered counts bitwise equal, and equal to the model."""
    L = _L()
    cat, q64, exact = shared_case(cuda_device, dt, 64)
    cv, rows = screened_lists(exact, k, kp, EPS5, seed=kp)
    vs = model_batch(cv, rows, exact, k, cat.n, EPS5)
    prev = L.load().ebt_rescore_form(-1)
    outs = {}
    try:
        for form in (1, 0):
            L.load().ebt_rescore_form(form)
            outs[form] = run_rescore(cat, q64, cv, rows, k, EPS5)
    finally:
        L.load().ebt_rescore_form(prev)
    for form in (1, 0):
        assert_matches(vs, *outs[form])
    assert np.array_equal(outs[0][0].view(np.int64), outs[1][0].view(np.int64))
    assert np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][2], outs[1][2])
    assert outs[0][3] == outs[1][3]


@gpu
@pytest.mark.parametrize("k,kp,ntail", [(20, 64, 0), (20, 300, 7), (1, 64, 0), (100, 512, 0)])
def test_rescore_partitioned_list(cuda_device, k, kp, ntail):
    """A list partitioned at k as ebt_merge_hits leaves it ([0, k-1) and [k, n-1) in any order,
    [n, k') empty) gives the outputs of the sorted list, bit for bit."""
    cat, q64, exact = shared_case(cuda_device, "f32", 64)
    cv, rows = screened_lists(exact, k, kp, EPS5, seed=3 * kp + k)
    if ntail:
        rows[:, kp - ntail:] = -1
        cv[:, kp - ntail:] = -np.inf
    n_ent = kp - ntail
    vs = model_batch(cv, rows, exact, k, cat.n, EPS5)
    a = run_rescore(cat, q64, cv, rows, k, EPS5)
    assert_matches(vs, *a)
    rng = np.random.default_rng(5)
    cv2, rows2 = cv.copy(), rows.copy()
    for b in range(cv.shape[0]):
        perm = np.arange(kp)
        perm[:k - 1] = rng.permutation(k - 1)
        perm[k:n_ent - 1] = k + rng.permutation(n_ent - 1 - k)
        cv2[b], rows2[b] = cv[b, perm], rows[b, perm]
    assert not np.array_equal(rows2, rows) or kp <= 2
    vs2 = model_batch(cv2, rows2, exact, k, cat.n, EPS5)
    b_ = run_rescore(cat, q64, cv2, rows2, k, EPS5)
    assert_matches(vs2, *b_)
    assert np.array_equal(a[0].view(np.int64), b_[0].view(np.int64))
    assert np.array_equal(a[1], b_[1]) and np.array_equal(a[2], b_[2]) and a[3] == b_[3]


def _one(cat, q64, exact, cv, rows, k, eps, t_floor=None, n_rows=None, boundary=False,
         dup_ok=False):
    """One constructed query through the kernel and the model, compared -> (verdict, s, r, cert,
    count). boundary: a cv sits on `cut` on purpose (bit-identical on both sides)."""
    n_rows = cat.n if n_rows is None else n_rows
    cv = np.asarray(cv, dtype=np.float32)[None]
    rows = np.asarray(rows, dtype=np.int64)[None]
    e = np.array([eps], dtype=np.float32)
    tf = None if t_floor is None else np.array([t_floor], dtype=np.float64)
    v = model_batch(cv, rows, exact[:1], k, n_rows, e, tf)[0]
    assert well_separated(v, cv[0], exact[0, np.clip(rows[0], 0, n_rows - 1)], eps, dup_ok,
                          boundary)
    s, r, c, cnt = run_rescore(cat, q64[:1], cv, rows, k, e, tf, n_rows=n_rows)
    assert_matches([v], s, r, c, cnt)
    return v, s[0], r[0], int(c[0]), cnt


@gpu
def test_rescore_certificate_truth_table(cuda_device):
    """One constructed query per clause of the certificate, each asserting the exact value."""
    cat, q64, exact = shared_case(cuda_device, "f32", 64)
    k, kp = 8, 32
    by_exact = np.argsort(-exact[0], kind="stable")          # query 0's rows, best first
    near0 = np.argsort(np.abs(exact[0]), kind="stable")      # rows scoring nearest 0
    assert np.abs(exact[0, near0[:kp]]).max() < 0.01
    flat = np.full(kp, 0.3, dtype=np.float32)

    # k' >= n_rows: 1 whatever the values (the same list against one more row: 0)
    low = np.random.default_rng(1).permutation(kp).astype(np.int64)
    assert _one(cat, q64, exact, flat, low, k, 0.01, n_rows=kp)[3] == 1
    assert _one(cat, q64, exact, flat, low, k, 0.01, n_rows=kp + 1)[3] == 0

    # a tail of -1 rows (nvalid < k'): 1; the full list: 0
    rows = by_exact[100:100 + kp].copy()
    assert _one(cat, q64, exact, flat, rows, k, 0.01)[3] == 0
    cv_t, rows_t = flat.copy(), rows.copy()
    cv_t[-3:], rows_t[-3:] = -np.inf, -1
    assert _one(cat, q64, exact, cv_t, rows_t, k, 0.01)[3] == 1

    # a full list with cv[k'-1] well below / well above cut2
    v, *_, c, _ = _one(cat, q64, exact, np.linspace(0.9, 0.1, kp), rows, k, 0.01)
    assert c == 1 and v.cut2 - 0.1 > 0.1
    v, *_, c, _ = _one(cat, q64, exact, np.linspace(0.9, 0.89, kp), rows, k, 0.05)
    assert c == 0 and 0.89 - v.cut2 > 0.05

    # the strict boundary: cv[k-1] = 0.5, eps = 0.125, first-k exact near 0 (no rise): cut =
    # 0.25 exactly; cv[k'-1] = 0.25 is not below it (0, and the row is gathered), the next
    # float32 towards 0 is (1, and it is not)
    rows_b = near0[:kp].copy()
    cv_b = np.concatenate([np.linspace(0.9, 0.5, k), np.linspace(0.45, 0.3, kp - k)]).astype(np.float32)
    cv_b[-1] = 0.25
    v0, _, _, c0, n0 = _one(cat, q64, exact, cv_b, rows_b, k, 0.125, boundary=True)
    assert v0.cut == 0.25 and v0.cut2 == 0.25 and c0 == 0 and n0 == kp
    cv_b[-1] = np.nextafter(np.float32(0.25), np.float32(0))
    v1, _, _, c1, n1 = _one(cat, q64, exact, cv_b, rows_b, k, 0.125, boundary=True)
    assert v1.cut2 == 0.25 and c1 == 1 and n1 == kp - 1

    # the t_floor clause alone: t_floor - eps = 0.70 above cv[k-1] - 2 eps = 0.50 turns a 0 into
    # a 1, and the top-k slots that cut empties read NaN / -1
    cv_f = np.concatenate([np.linspace(0.9, 0.6, k), np.linspace(0.59, 0.55, kp - k)])
    v, s, r, c, _ = _one(cat, q64, exact, cv_f, rows, k, 0.05)
    assert c == 0 and abs(v.cut - 0.5) < 1e-6 and np.all(r >= 0)
    v, s, r, c, cnt = _one(cat, q64, exact, cv_f, rows, k, 0.05, t_floor=0.75)
    n_above = int(np.sum(cv_f.astype(np.float32).astype(np.float64) >= v.cut))
    assert c == 1 and abs(v.cut - 0.70) < 1e-6 and v.cut2 == v.cut and 0 < n_above < k
    assert cnt == n_above and np.all(r[n_above:] == -1) and np.all(np.isnan(s[n_above:]))
    assert np.all(r[:n_above] >= 0)

    # the rise alone: s_min - eps above cut turns a 0 into a 1 and removes rows from the
    # gathered count
    rows_r = by_exact[:kp].copy()                     # the first k are the query's k best rows
    eps_r = float(np.float32(0.05))
    s_min = float(exact[0, rows_r[:k]].min())
    c2 = s_min - eps_r
    # cut = c2 - 0.05; 12 candidates above c2 (gathered), 12 between cut and c2 (kept, skipped)
    cv_r = np.concatenate([np.linspace(0.6, c2 + 0.05, k),
                           np.linspace(c2 + 0.03, c2 + 0.01, 12),
                           np.linspace(c2 - 0.01, c2 - 0.04, kp - k - 12)])
    assert np.all(np.diff(cv_r) < 0)
    no_rise = model_batch(cv_r[None].astype(np.float32), rows_r[None], exact[:1], k, cat.n,
                          np.array([eps_r], np.float32), rise=False)[0]
    v, _, _, c, cnt = _one(cat, q64, exact, cv_r, rows_r, k, eps_r)
    assert no_rise.cert == 0 and no_rise.n_gathered == kp
    assert c == 1 and abs(v.cut - (c2 - 0.05)) < 1e-6 and abs(v.cut2 - c2) < 1e-12
    assert v.n_kept == kp and cnt == k + 12
    # ... and with eps = 0 there is no rise: equal cand_vals below s_min, every row gathered, 0
    v, _, _, c, cnt = _one(cat, q64, exact, np.full(kp, 0.1), rows_r, k, 0.0)
    assert s_min > 0.1 and v.cut2 == v.cut and c == 0 and cnt == kp

    # a row equal to n_rows (the first guard row, inside the allocation): -2, never read
    for bad in (cat.n, cat.n + GUARD_ROWS - 1):
        rows_c = rows.copy()
        rows_c[2] = bad
        v, s, r, c, _ = _one(cat, q64, exact, np.linspace(0.9, 0.1, kp), rows_c, k, 0.01)
        assert c == -2 and not np.any(r == bad)
        assert np.all(np.abs(s[~np.isnan(s)]) <= 1.0 + 1e-9)


@gpu
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("eps", [0.0, 0.05])
def test_rescore_ties_row_ascending(cuda_device, dt, eps):
    """Bit-identical duplicate catalog rows come out row-ascending: a pair inside the top k and
    a pair straddling position k, in the list (k-1 and k: scored by different passes) and in
    the order of exact scores, listed with the higher row first."""
    d, k, kp = 64, 8, 32
    base = DevCatalog(cuda_device, dt, d, seed=100 + d)
    q64 = unit_queries(200 + d, 5, d)[:1]
    order = np.argsort(-base.exact(q64)[0], kind="stable")
    # rows ranked 2 and k-2 (0-based) get a bit-identical copy at another row id
    src_in, src_cut = int(order[2]), int(order[k - 2])
    dst_in, dst_cut = int(order[900]), int(order[901])
    dup = ((dst_in, src_in), (dst_cut, src_cut))
    cat = DevCatalog(cuda_device, dt, d, seed=100 + d, dup=dup)
    exact = cat.exact(q64, dup)
    # exact order of the list: order[0 .. k-2] with src_in's copy -> k ranks 0 .. k-1 hold
    # order[0], order[1], {src_in, dst_in}, order[3 .. k-3], and {src_cut, dst_cut} at k-1, k
    head = [int(x) for x in order[:k - 2] if x != src_in]
    hi_cut, lo_cut = max(src_cut, dst_cut), min(src_cut, dst_cut)
    first_k = head + [max(src_in, dst_in), min(src_in, dst_in), hi_cut]   # higher rows first
    assert len(first_k) == k
    rest = [lo_cut] + [int(x) for x in order[k:k + kp - k - 1] if x not in (dst_in, dst_cut)]
    rows = np.array(first_k + rest, dtype=np.int64)[:kp]
    assert rows.size == kp and np.unique(rows).size == kp
    assert rows[k - 1] == hi_cut and rows[k] == lo_cut
    cv = (np.linspace(0.6, 0.5, kp) if eps > 0 else np.full(kp, 0.5)).astype(np.float32)
    v, s, r, c, _ = _one(cat, q64, exact, cv, rows, k, eps, dup_ok=True)
    assert v.gathered[k]                                 # the copy at position k is scored
    assert r[k - 1] == lo_cut and hi_cut not in r          # the lower row takes the last slot
    i = int(np.flatnonzero(r == min(src_in, dst_in))[0])
    assert r[i + 1] == max(src_in, dst_in) and s[i] == s[i + 1]


@gpu
def test_rescore_shortfall(cuda_device):
    """Fewer than k valid candidates: the valid ones in order, then NaN / -1; certified 1."""
    cat, q64, exact = shared_case(cuda_device, "f32", 64)
    k, kp, nv = 20, 64, 7
    rows = np.full(kp, -1, dtype=np.int64)
    rows[:nv] = np.random.default_rng(3).permutation(cat.n)[:nv]
    cv = np.full(kp, -np.inf, dtype=np.float32)
    cv[:nv] = np.linspace(0.5, 0.4, nv)
    v, s, r, c, cnt = _one(cat, q64, exact, cv, rows, k, 0.01)
    assert c == 1 and cnt == nv and np.all(r[:nv] >= 0)
    assert np.all(r[nv:] == -1) and np.all(np.isnan(s[nv:]))


# ------------------------------------------ 3. ebt_rescore_owned + ebt_finalize_topk ----------
def run_owned(shard, row_offset, q64, cv, rows, k, eps):
    L = _L()
    dev = shard.dev
    B, kp = cv.shape
    qt = torch.from_numpy(np.ascontiguousarray(q64)).to(dev)
    cvt = torch.from_numpy(np.ascontiguousarray(cv, dtype=np.float32)).to(dev)
    rt = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int64)).to(dev)
    et = torch.from_numpy(np.ascontiguousarray(eps, dtype=np.float32)).to(dev)
    ex = torch.full((B, kp), 555.0, dtype=torch.float64, device=dev)
    L.call("ebt_rescore_owned", L.ptr(qt), B, shard.d, L.ptr(shard.t),
           L.DTYPE_CODE[TORCH_DT[shard.dt]], shard.ld, L.ptr(shard.g), row_offset, shard.n,
           L.ptr(cvt), L.ptr(rt), kp, k, L.ptr(et), L.ptr(ex), L.stream_of(dev))
    torch.cuda.synchronize(dev)
    return ex


def run_finalize(dev, cv, rows, exact_t, k, n_global, eps, ovf="null"):
    L = _L()
    B, kp = cv.shape
    cvt = torch.from_numpy(np.ascontiguousarray(cv, dtype=np.float32)).to(dev)
    rt = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int64)).to(dev)
    et = torch.from_numpy(np.ascontiguousarray(eps, dtype=np.float32)).to(dev)
    ot = None if isinstance(ovf, str) else torch.from_numpy(
        np.ascontiguousarray(ovf, dtype=np.int32)).to(dev)
    out_s = torch.full((B, k), 777.0, dtype=torch.float64, device=dev)
    out_r = torch.full((B, k), -7, dtype=torch.int64, device=dev)
    cert = torch.full((B,), 99, dtype=torch.int32, device=dev)
    L.call("ebt_finalize_topk", L.ptr(cvt), L.ptr(rt), L.ptr(exact_t), B, kp, k, n_global,
           L.ptr(et), L.ptr(ot), L.ptr(out_s), L.ptr(out_r), L.ptr(cert), L.stream_of(dev))
    torch.cuda.synchronize(dev)
    return out_s.cpu().numpy(), out_r.cpu().numpy(), cert.cpu().numpy()


SHARD_BOUNDS = {1: [0, N_CAT], 3: [0, 1000, 1300, N_CAT]}


@gpu
@pytest.mark.parametrize("R_", [1, 3])
@pytest.mark.parametrize("dt,d", [("f32", 64), ("bf16", 64), ("f32", 77), ("bf16", 77)])
def test_two_phase_owned_and_finalize(cuda_device, dt, d, R_):
    """One catalog in R uneven shards, one merged sorted list of GLOBAL rows. Per shard,
    ebt_rescore_owned writes the float64 score of the rows it owns above the cut and exactly 0.0
    elsewhere; every kept candidate is non-zero on exactly one shard; after the sum,
    ebt_finalize_topk equals the model without rise and t_floor; ovf != 0 gives -1, ovf = NULL
    is accepted, a row >= n_rows_global gives -2 (which wins over -1)."""
    dev = cuda_device
    cat, q64, exact = shared_case(dev, dt, d)
    B = q64.shape[0]
    bounds = SHARD_BOUNDS[R_]
    key = ("shards", dt, d, R_)
    if key not in _SHARED:
        _SHARED[key] = [cat.shard(bounds[i], bounds[i + 1]) for i in range(R_)]
    shards = _SHARED[key]
    for k in (1, 20):
        for kp in (64, 300):
            cv, rows = screened_lists(exact, k, kp, EPS5, seed=11 * kp + k + d)
            rows[4, kp - 6:] = -1            # one query with an empty tail
            cv[4, kp - 6:] = -np.inf
            valid = rows >= 0
            ex_pos = np.where(valid, np.take_along_axis(exact, np.clip(rows, 0, None), 1), 0.0)
            cut = cv[:, k - 1].astype(np.float64) - 2.0 * EPS5.astype(np.float64)
            kept = valid & ~(cv.astype(np.float64) < cut[:, None])
            assert kept.sum() < valid.sum()   # the cut removes something somewhere
            total = torch.zeros((B, kp), dtype=torch.float64, device=dev)
            nonzero = np.zeros((B, kp), dtype=np.int64)
            for i, sh in enumerate(shards):
                lo, hi = bounds[i], bounds[i + 1]
                ex = run_owned(sh, lo, q64, cv, rows, k, EPS5)
                e = ex.cpu().numpy()
                mine = kept & (rows >= lo) & (rows < hi)
                assert np.all(e[~mine] == 0.0) and not np.any(np.signbit(e[~mine]))
                np.testing.assert_allclose(e[mine], ex_pos[mine], rtol=0, atol=SCORE_ATOL)
                nonzero += (e != 0.0)
                total += ex
            assert np.array_equal(nonzero, kept.astype(np.int64))
            vs = [contract_model(cv[b], rows[b], ex_pos[b], k, N_CAT, EPS5[b], rise=False)
                  for b in range(B)]
            ovf = np.array([0, 1, 0, 2, 0], dtype=np.int32)
            for o in ("null", np.zeros(B, np.int32), ovf):
                s, r, c = run_finalize(dev, cv, rows, total, k, N_CAT, EPS5, o)
                for b, v in enumerate(vs):
                    np.testing.assert_array_equal(r[b], v.out_r)
                    np.testing.assert_allclose(s[b], v.out_s, rtol=0, atol=SCORE_ATOL,
                                               equal_nan=True)
                    want = -1 if (not isinstance(o, str) and o[b] != 0) else v.cert
                    assert int(c[b]) == want, (k, kp, b, int(c[b]), want)
            # the corrupt-list clause: a valid row >= n_rows_global, in queries 0 and 1 (ovf set)
            rows_c = rows.copy()
            rows_c[0, 0] = N_CAT
            rows_c[1, kp // 2] = N_CAT + 5
            vc = [contract_model(cv[b], rows_c[b], ex_pos[b], k, N_CAT, EPS5[b], rise=False)
                  for b in range(B)]
            assert [v.cert for v in vc[:2]] == [-2, -2]
            s, r, c = run_finalize(dev, cv, rows_c, total, k, N_CAT, EPS5, ovf)
            for b, v in enumerate(vc):
                np.testing.assert_array_equal(r[b], v.out_r)
                np.testing.assert_allclose(s[b], v.out_s, rtol=0, atol=SCORE_ATOL, equal_nan=True)
                want = v.cert if v.cert == -2 else (-1 if ovf[b] else v.cert)
                assert int(c[b]) == want, (k, kp, b, int(c[b]), want)


# -------------------------- 4. ebt_certify_cut, ebt_mask_excluded, ebt_scale_rows_f64 ---------
@gpu
def test_certify_cut_cross_product(cuda_device):
    """B = 300 (two blocks and a tail): incoming cert x ovf x theta against t_floor - eps. -2
    stays; -1 where ovf != 0 or not (theta <= t_floor - eps) (NaN gives -1); else unchanged."""
    L = _L()
    dev = cuda_device
    B = 300
    pairs = [(0.5, 0.125), (1.0, 0.25), (-0.25, 0.0625), (0.75, 0.5), (0.0, 0.0)]
    cert, ovf, theta, tfl, eps = [], [], [], [], []
    for tf, e in pairs:
        edge = np.float32(tf - e)
        assert float(edge) == tf - e          # t_floor - eps is a float32: "equal" is exact
        for c in (1, 0, -1, -2):
            for o in (0, 1, 2):
                for th, tfv in ((edge - np.float32(0.1), tf), (edge, tf),
                                (np.nextafter(edge, np.float32(np.inf)), tf),
                                (np.float32(np.nan), tf), (edge - np.float32(0.1), np.nan)):
                    cert.append(c); ovf.append(o); theta.append(th); tfl.append(tfv); eps.append(e)
    assert len(cert) == B
    cert = np.array(cert, np.int32); ovf = np.array(ovf, np.int32)
    theta = np.array(theta, np.float32); tfl = np.array(tfl, np.float64)
    eps = np.array(eps, np.float32)
    T = lambda a: torch.from_numpy(a.copy()).to(dev)
    for use_theta in (True, False):
        ok = theta.astype(np.float64) <= tfl - eps.astype(np.float64)   # NaN: False
        drop = (ovf != 0) | (~ok if use_theta else False)
        want = np.where(cert == -2, -2, np.where(drop, -1, cert)).astype(np.int32)
        ct, ot, tt, ft, et = T(cert), T(ovf), T(theta), T(tfl), T(eps)
        if use_theta:
            L.call("ebt_certify_cut", L.ptr(ct), L.ptr(ot), L.ptr(tt), L.ptr(ft), L.ptr(et), B,
                   L.stream_of(dev))
        else:
            L.call("ebt_certify_cut", L.ptr(ct), L.ptr(ot), None, None, None, B, L.stream_of(dev))
        torch.cuda.synchronize(dev)
        np.testing.assert_array_equal(ct.cpu().numpy(), want)
        assert set(want.tolist()) == {1, 0, -1, -2}
        # the inputs are read-only
        assert torch.equal(ot, T(ovf)) and torch.equal(ft.view(torch.int64), T(tfl).view(torch.int64))


@gpu
def test_mask_excluded_cells(cuda_device):
    """B = 7, ld = 40, window [100, 132): exactly the model's cells become -inf, every other
    cell (padding columns, rows outside every segment included) is bit-unchanged."""
    L = _L()
    dev = cuda_device
    B, ld, c0, c1 = 7, 40, 100, 132
    segs = [[99, 100, 131, 132, 500], [], [110, 110, 110], [0, 5], list(range(100, 132)), [131],
            [200, 105, 101, -3]]
    junk_head, junk_tail = [100, 101, 120], [131, 115]   # outside every segment: not applied
    rows = np.array(junk_head + sum(segs, []) + junk_tail, dtype=np.int64)
    off = np.concatenate([[len(junk_head)], len(junk_head) + np.cumsum([len(s) for s in segs])])
    assert off[0] > 0 and off[-1] + len(junk_tail) == rows.size
    rng = np.random.default_rng(9)
    sc = rng.standard_normal((B, ld)).astype(np.float32)
    sc[0, 3] = np.nan
    sc[5, 39] = np.inf
    want = sc.copy()
    for b, s in enumerate(segs):
        for g in s:
            if c0 <= g < c1:
                want[b, g - c0] = -np.inf
    assert np.isneginf(want).sum() == 2 + 1 + 32 + 1 + 2
    st = torch.from_numpy(sc.copy()).to(dev)
    ot = torch.from_numpy(off.astype(np.int64)).to(dev)
    rt = torch.from_numpy(rows).to(dev)
    L.call("ebt_mask_excluded", L.ptr(st), ld, B, c0, c1, L.ptr(ot), L.ptr(rt), L.stream_of(dev))
    torch.cuda.synchronize(dev)
    assert np.array_equal(st.cpu().numpy().view(np.int32), want.view(np.int32))


@gpu
@pytest.mark.parametrize("d", [1, 77])
def test_scale_rows_bit_equal(cuda_device, d):
    L = _L()
    dev = cuda_device
    B = 5
    rng = np.random.default_rng(d)
    q = rng.standard_normal((B, d)) * np.exp2(rng.integers(-30, 30, (B, d)))
    scale = 1.0 / rng.integers(1, 200, B).astype(np.float64)
    qt = torch.from_numpy(q.copy()).to(dev)
    stt = torch.from_numpy(scale).to(dev)
    L.call("ebt_scale_rows_f64", L.ptr(qt), B, d, L.ptr(stt), L.stream_of(dev))
    torch.cuda.synchronize(dev)
    assert np.array_equal(qt.cpu().numpy().view(np.int64), (q * scale[:, None]).view(np.int64))


# --------------------------------- 5. the first pass certifies where it provably can ----------
@gpu
@pytest.mark.parametrize("dt,d", [("f32", 64), ("bf16", 256), ("f16", 256)])
def test_first_pass_certifies_benign(cuda_device, dt, d):
    """The k'-th best approx is at most the k'-th best exact + eps and the k-th best approx at
    least the k-th best exact - eps, so exact_(k') < exact_(k) - 4 eps_b implies approx_(k') <
    approx_(k) - 2 eps_b: the first pass MUST certify such a query (unfused: 1; the fused screen
    may also answer -1, never 0). Every query of these Gaussian inputs satisfies the inequality
    with the library's own eps -- a condition of the test, asserted, not skipped."""
    import robot_ebert_amd as ebt
    from robot_ebert_amd import search
    L = _L()
    dev = cuda_device
    n, B, k, kp = 8192, 64, 10, 128
    c = gaussian(41, n, d, dt)
    q = gaussian(42, B, d, dt)
    cat = ebt.Catalog(torch.from_numpy(np.ascontiguousarray(c)).to(dev).to(TORCH_DT[dt]))
    qb = ebt.prepare_queries(cat, queries=torch.from_numpy(np.ascontiguousarray(q)).to(dev)
                             .to(TORCH_DT[dt]))
    torch.cuda.synchronize(dev)
    eps = qb.eps[:B].cpu().numpy().astype(np.float64)
    q64 = q / np.linalg.norm(q, axis=1, keepdims=True)
    exact = (q64 @ c.T) / np.linalg.norm(c, axis=1)
    srt = -np.sort(-exact, axis=1)
    gap = srt[:, k - 1] - srt[:, kp - 1]
    print(f"{dt} d={d}: min gap {gap.min():.4f}, max 4 eps {4 * eps.max():.5f}")
    assert np.all(eps > 0) and np.all(srt[:, kp - 1] < srt[:, k - 1] - 4.0 * eps)
    s_ref, r_ref = R.cosine_topk(q, c, k)
    for flags, allowed in ((L.EBT_FLAG_NO_FUSE, {1}), (0, {1, -1})):
        s, r, cert = search.run_pipeline(cat, qb, k, kp, None, None, None, flags=flags)
        torch.cuda.synchronize(dev)
        cert = cert.cpu().numpy()
        assert set(cert.tolist()) <= allowed, (flags, np.unique(cert, return_counts=True))
        ok = cert == 1
        np.testing.assert_array_equal(r.cpu().numpy()[ok], r_ref[ok])
        np.testing.assert_allclose(s.cpu().numpy()[ok], s_ref[ok], rtol=0, atol=SCORE_ATOL)
