"""GPU: multi-interest top-k (include/ebert.h 0.11.0) -- cluster the liked rows, interleave.

The two kernels are compared BITWISE with tests/interest_ref.py: the clustering on the device's
own pool_gram matrix (labels, sizes, medoids, iters: no tolerance, no gap condition), the
interleave on synthetic lists. Against the oracle (oracle.restatement.cosine_similarity of the
stored values) the labels are equal for every query whose oracle decisions all have a gap above
1e-9 -- the device matrix is within SCORE_ATOL = 1e-12 of the oracle's, so such gaps decide --
and that every query of these shapes has such gaps is ASSERTED, not filtered.

Shapes: catalogs of 2,000 rows with one zero-norm row, batches of 8 queries; p crosses the 16-wide
MFMA tile, the 64-lane wave, the kernel's 1 / 2 / 4 / 8 slots per lane and the 128-slot workgroup
tile of the matrix (1, 2, 15, 16, 17, 63, 64, 65, 129, 300, 512)."""
import ctypes

import numpy as np
import pytest
import torch

from inputs import gaussian, round_to
from interest_ref import cluster_ref, dhondt_seats, interleave_ref, planted
from oracle import restatement as R

pytestmark = pytest.mark.gpu
N = 2000
ZERO_ROW = 3
PS = (1, 2, 15, 16, 17, 63, 64, 65, 129, 300, 512)
CS = (1, 2, 3, 8)
TORCH_DT = {"f32": torch.float32, "bf16": torch.bfloat16}
# (kind, dtype, d): planted data (g = 3) with the noise in the name, or iid Gaussian rows
KERNEL_CASES = [("planted1.0", "f32", 32), ("iid", "f32", 32), ("planted1.0", "bf16", 768),
                ("iid", "bf16", 768)]
# the eight L = 300 lists of test_the_cap_and_an_earlier_stop (iid, d = 32): rng seeds picked on
# the CPU with interest_ref over the oracle's matrix (smallest gap 3.8e-6): 1, 3, 4 and 6 stop at
# the cap
CAP_SEEDS = (0, 1, 2, 3, 4, 5, 6, 7)


def _ebt():
    import robot_ebert_amd as ebt
    from robot_ebert_amd import _lib, diversify, interests
    return ebt, _lib, diversify, interests


def bits(x):
    return (x.cpu().numpy() if isinstance(x, torch.Tensor) else np.ascontiguousarray(x)).tobytes()


def catalog_values(kind, dt, d):
    """The stored values of a catalog as float64 (rounded to dt), row 3 zero. Row i of a planted
    catalog belongs to group i % 3."""
    if kind == "iid":
        x = gaussian(91, N, d, dt)
    else:
        x = round_to(planted(92, 3, d, N, float(kind[len("planted"):]))[0], dt)
    x[ZERO_ROW] = 0.0
    return x


@pytest.fixture(scope="module")
def catalogs(cuda_device):
    """(Catalog, its stored values as float64) per (kind, dtype, d); the last three are kept."""
    ebt = _ebt()[0]
    made = {}

    def get(kind, dt, d):
        if (kind, dt, d) not in made:
            while len(made) >= 3:
                made.pop(next(iter(made)))
            x = catalog_values(kind, dt, d)
            xt = torch.from_numpy(x).to(cuda_device).to(TORCH_DT[dt])
            made[kind, dt, d] = (ebt.Catalog(xt), x)
        return made[kind, dt, d]
    return get


def kernel_lists(p, seed=5):
    """Eight lists of p slots: full, a -1 mid-list, the zero row, a duplicated row, L < c (two
    rows), all empty, every third slot empty, full."""
    rng = np.random.default_rng(seed + p)
    r = np.stack([rng.choice(np.arange(4, N), size=p, replace=False) for _ in range(8)])
    r = r.astype(np.int64)
    r[1, p // 2] = -1
    r[2, 0] = ZERO_ROW
    if p > 1:
        r[3, p - 1] = r[3, 0]
    r[4, 2:] = -1
    r[5] = -1
    r[6, 1::3] = -1
    return r


def check_cluster(got, G, rows, c, status=None):
    """ebt_interest_cluster's outputs against cluster_ref on the same matrix: all equal."""
    label, size, medoid, iters = (x.cpu().numpy() for x in got)
    assert label.dtype == np.int32 and size.dtype == np.int32 and medoid.dtype == np.int32
    assert label.shape == rows.shape and size.shape == (len(rows), c) == medoid.shape
    for b in range(len(rows)):
        r = rows[b] if status is None or status[b] >= 0 else np.full_like(rows[b], -1)
        wl, ws, wm, wi = cluster_ref(G[b], r, c)
        assert np.array_equal(label[b], wl), (b, c, label[b], wl)
        assert np.array_equal(size[b], ws), (b, c, size[b], ws)
        assert np.array_equal(medoid[b], wm), (b, c, medoid[b], wm)
        assert iters[b] == wi, (b, c, iters[b], wi)
    return iters


# ------------------------------------------------------------------ 1. the cluster kernel, bitwise ----
@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("kind,dt,d", KERNEL_CASES)
def test_cluster_bitwise_on_the_device_matrix(cuda_device, catalogs, kind, dt, d, p):
    """cluster_ref fed the GPU's own pool_gram matrix: labels, sizes, medoids and iters equal for
    every c, on lists with a -1 mid-list, the zero row, a duplicated row, L < c and no row."""
    _, _, dv, it = _ebt()
    cat, _ = catalogs(kind, dt, d)
    r = kernel_lists(p)
    rt = torch.from_numpy(r).to(cuda_device)
    gram, status = dv.pool_gram(cat, rt)
    assert status.cpu().tolist() == [1] * 8
    G = gram.cpu().numpy()
    for c in CS:
        iters = check_cluster(it.interest_cluster(gram, rt, c, status=status), G, r, c)
        assert np.array_equal(iters == 0, (r >= 0).sum(axis=1) == 0) and iters[5] == 0
    # status NULL: the same clustering
    a, b = it.interest_cluster(gram, rt, 3), it.interest_cluster(gram, rt, 3, status=status)
    assert all(bits(x) == bits(y) for x, y in zip(a, b))


def cap_lists():
    return np.stack([np.sort(np.random.default_rng(1000 + s).choice(np.arange(4, N), size=300,
                                                                     replace=False))
                     for s in CAP_SEEDS]).astype(np.int64)


def test_the_cap_and_an_earlier_stop(cuda_device, catalogs):
    """iid d = 32, L = 300, c = 3: of these eight lists at least one runs to the cap of 16 passes
    (and takes the final pass after it) and at least one converges earlier; all bitwise."""
    _, L, dv, it = _ebt()
    cat, _ = catalogs("iid", "f32", 32)
    r = cap_lists()
    rt = torch.from_numpy(r).to(cuda_device)
    gram, status = dv.pool_gram(cat, rt)
    iters = check_cluster(it.interest_cluster(gram, rt, 3, status=status), gram.cpu().numpy(), r, 3)
    print("iters", iters.tolist())
    assert (iters == L.EBT_INTEREST_ITERS).any() and (iters < L.EBT_INTEREST_ITERS).any()


def test_hand_made_matrix_with_exact_ties(cuda_device):
    """Similarities on a 0.25 grid (exact ties everywhere: every arg max falls to the position or
    to m), -0.0 beside +0.0, a query whose status is -2, a query with no row."""
    _, _, _, it = _ebt()
    rng = np.random.default_rng(31)
    for p in (5, 64, 130):
        B = 6
        G = np.round(rng.uniform(-1, 1, (B, p, p)) * 4) / 4
        G = np.maximum(G, G.transpose(0, 2, 1))
        G[1][G[1] == 0.0] = -0.0
        G[2][:] = 0.5
        rows = rng.integers(0, 10 ** 12, size=(B, p))
        rows[3] = -1
        rows[4, 1] = -1
        G[4][1, :] = G[4][:, 1] = np.nan
        G[3][:] = np.nan
        status = np.array([1, 1, 1, 1, 1, -2], dtype=np.int32)
        gt, rt = torch.from_numpy(G).to(cuda_device), torch.from_numpy(rows).to(cuda_device)
        for c in CS:
            got = it.interest_cluster(gt, rt, c, status=torch.from_numpy(status).to(cuda_device))
            check_cluster(got, G, rows, c, status=status)
            assert (got[0][5] == -1).all() and (got[1][5] == 0).all() and (got[2][5] == -1).all()


# ----------------------------------------------------------------------------- 2. invariance ----
def test_padding_batch_and_slot_positions_do_not_matter(cuda_device, catalogs):
    _, _, dv, it = _ebt()
    dev = cuda_device
    cat, _ = catalogs("planted1.0", "f32", 32)
    base = kernel_lists(17)
    c = 3

    def run(rows):
        rt = torch.from_numpy(np.ascontiguousarray(rows)).to(dev)
        gram, status = dv.pool_gram(cat, rt)
        return [x.cpu().numpy() for x in it.interest_cluster(gram, rt, c, status=status)]

    label, size, medoid, iters = run(base)
    # padded to 512 (another instantiation of the kernel, another tiling of the matrix)
    for p in (64, 100, 512):
        wide = np.full((8, p), -1, dtype=np.int64)
        wide[:, :17] = base
        l2, s2, m2, i2 = run(wide)
        assert np.array_equal(l2[:, :17], label) and (l2[:, 17:] == -1).all(), p
        assert np.array_equal(s2, size) and np.array_equal(m2, medoid), p
        assert np.array_equal(i2, iters), p
    # alone
    for b in (0, 1, 3, 6):
        one = run(base[b:b + 1])
        assert all(np.array_equal(x[0], y[b]) for x, y in zip(one, (label, size, medoid, iters)))
    # the -1 slots moved: the rows keep their order, the outputs follow the rows
    rng = np.random.default_rng(9)
    for p in (40, 130):
        slots = np.stack([np.sort(rng.choice(p, size=17, replace=False)) for _ in range(8)])
        moved = np.full((8, p), -1, dtype=np.int64)
        for b in range(8):
            moved[b, slots[b]] = base[b]
        l2, s2, m2, i2 = run(moved)
        for b in range(8):
            assert np.array_equal(l2[b, slots[b]], label[b]), (p, b)
            assert (np.delete(l2[b], slots[b]) == -1).all()
            assert np.array_equal(m2[b], np.where(medoid[b] >= 0,
                                                  slots[b][np.maximum(medoid[b], 0)], -1)), (p, b)
        assert np.array_equal(s2, size) and np.array_equal(i2, iters), p


def test_cluster_liked_order_and_ws_budget_do_not_matter(cuda_device, catalogs):
    ebt, L, _, _ = _ebt()
    cat, _ = catalogs("planted1.0", "f32", 32)
    rng = np.random.default_rng(13)
    lens = (1, 15, 16, 17, 33, 300, 85, 2)
    lists = [rng.choice(N, size=n, replace=False).tolist() for n in lens]
    whole = ebt.cluster_liked(cat, lists, c=3)
    assert tuple(whole.label.shape) == (8, 300) and tuple(whole.size.shape) == (8, 3)
    for b, n in enumerate(lens):
        assert whole.rows[b, :n].cpu().tolist() == sorted(lists[b])
        assert (whole.rows[b, n:] == -1).all() and (whole.label[b, n:] == -1).all()
        assert (whole.label[b, :n] >= 0).all() and int(whole.size[b].sum()) == n
    shuffled = [rng.permutation(l).tolist() for l in lists]
    again = ebt.cluster_liked(cat, shuffled, c=3)
    assert all(bits(a) == bits(b) for a, b in zip(whole, again))
    per = L.load().ebt_interest_workspace_bytes(1, 16)
    for budget in (2 * per, 2 * per + per // 2, 1, 0):        # the 16-slot group split; one at a time
        part = ebt.cluster_liked(cat, lists, c=3, ws_budget=budget)
        assert all(bits(a) == bits(b) for a, b in zip(whole, part)), budget
    # the device CSR form of score_topk's liked=
    from robot_ebert_amd.search import csr_from_lists
    csr = csr_from_lists(lists, cuda_device)
    again = ebt.cluster_liked(cat, (csr[0], csr[1]), c=3)
    assert all(bits(a) == bits(b) for a, b in zip(whole, again))


# ----------------------------------------------------------------------- 3. against the oracle ----
# A cluster of exactly two rows has no decidable medoid: both means are (1 + S_ij) / 2 up to the
# rounding of the diagonal, a structural tie. The lengths avoid the smallest such lists (L = 2
# always, L = 3 at c = 2) and the seeds -- the first from 21 on -- were picked on the CPU with
# interest_ref over the oracle's matrix so that every decision of every list has a gap above 1e-9
# (the smallest is 2.6e-6); the test asserts it again.
ORACLE_LENS = {2: (1, 15, 17, 33, 64, 85, 129, 300), 3: (1, 3, 15, 17, 64, 85, 129, 300),
               8: (1, 3, 33, 64, 85, 129, 200, 300)}
ORACLE_SEED = {("planted1.0", "f32", 32, 8): 26, ("iid", "f32", 32, 8): 25,
               ("planted1.0", "bf16", 768, 8): 25, ("iid", "bf16", 768, 3): 22,
               ("iid", "bf16", 768, 8): 25}


def oracle_lists(seed, lens=ORACLE_LENS[3]):
    rng = np.random.default_rng(seed)
    return [np.sort(rng.choice(np.arange(4, N), size=n, replace=False)) for n in lens]


@pytest.mark.parametrize("c", [2, 3, 8])
@pytest.mark.parametrize("kind,dt,d", KERNEL_CASES)
def test_labels_equal_the_oracles(cuda_device, catalogs, kind, dt, d, c):
    """cluster_liked against cluster_ref on the oracle's cosine matrix of the stored values. The
    oracle's smallest gap over every decision (seeds, every assignment of every pass, medoids) is
    ASSERTED to exceed 1e-9 for every query, then everything is equal."""
    ebt = _ebt()[0]
    cat, x = catalogs(kind, dt, d)
    lists = oracle_lists(ORACLE_SEED.get((kind, dt, d, c), 21), ORACLE_LENS[c])
    got = ebt.cluster_liked(cat, [l.tolist() for l in lists], c=c)
    label, size, medoid, iters = (t.cpu().numpy() for t in got[:4])
    worst = np.inf
    for b, l in enumerate(lists):
        S = R.cosine_similarity(x[l], x[l])
        wl, ws, wm, wi, gap = cluster_ref(S, l, c, with_gap=True)
        worst = min(worst, gap)
        assert gap > 1e-9, (b, gap)
        assert np.array_equal(label[b, :len(l)], wl), b
        assert np.array_equal(size[b], ws) and np.array_equal(medoid[b], wm) and iters[b] == wi, b
    print(f"{kind} {dt} d={d} c={c}: smallest oracle gap {worst:.3e}")


@pytest.mark.parametrize("dt,d", [("f32", 32), ("bf16", 768)])
def test_planted_groups_are_recovered(cuda_device, catalogs, dt, d):
    """Noise 0.7: the three planted groups (row % 3) are the three clusters, exactly."""
    ebt = _ebt()[0]
    cat, x = catalogs("planted0.7", dt, d)
    lists = [l for l in oracle_lists(22) if len(l) >= 15]
    got = ebt.cluster_liked(cat, [l.tolist() for l in lists], c=3)
    label = got.label.cpu().numpy()
    for b, l in enumerate(lists):
        pairs = {(int(a), int(g)) for a, g in zip(label[b, :len(l)], l % 3)}
        assert len(pairs) == 3 and len({a for a, _ in pairs}) == 3, (b, sorted(pairs))
        counts = np.bincount(l % 3, minlength=3)
        assert sorted(got.size[b].cpu().tolist(), reverse=True) == sorted(counts, reverse=True)


# --------------------------------------------------------------------- 4. the interleave, bitwise ----
@pytest.mark.parametrize("c", [1, 3, 8])
@pytest.mark.parametrize("k", [1, 10, 63, 64, 65, 512])
def test_interleave_bitwise(cuda_device, k, c):
    """Synthetic lists: rows drawn from a small range (duplicates within and across lists), -1
    holes, short lists, empty clusters (size 0 with a full list), everything exhausted before k,
    scores with -0.0 and NaN payloads kept as bits."""
    _, _, _, it = _ebt()
    rng = np.random.default_rng(100 * k + c)
    B = 8
    rows = rng.integers(0, max(2 * k, 4), size=(B, c, k)).astype(np.int64)
    rows[0] = rng.integers(0, 10 ** 12, size=(c, k))                 # no duplicates: all k emitted
    rows[1][rng.random((c, k)) < 0.3] = -1                           # holes
    for m in range(c):
        rows[2, m, rng.integers(0, k + 1):] = -1                     # short lists
    rows[3, :, (k + 3) // 4:] = -1                                   # exhausted before k
    rows[3, :, :(k + 3) // 4] = rng.integers(0, max(k // 8, 2), size=(c, (k + 3) // 4))
    rows[4] = -1                                                     # nothing at all
    rows[5] = rows[5, 0]                                             # every list the same
    size = rng.integers(1, 200, size=(B, c)).astype(np.int32)
    size[6, ::2] = 0                                                 # empty clusters
    size[7] = 1                                                      # equal sizes: ties to the lower m
    if c > 1:
        size[1, 1] = 0
    scores = rng.standard_normal((B, c, k))
    scores[0, 0, 0] = -0.0
    sb = scores.view(np.int64)
    sb[1, 0, :] = 0x7ff8000000000123                                 # a NaN with a payload
    dev = cuda_device
    got = it.interleave(torch.from_numpy(size).to(dev), torch.from_numpy(rows).to(dev),
                        torch.from_numpy(scores).to(dev))
    g_rows, g_scores, g_cluster, g_pos = (x.cpu().numpy() for x in got)
    assert g_rows.dtype == np.int64 and g_cluster.dtype == np.int32 and g_pos.dtype == np.int32
    for b in range(B):
        wr, ws, wc, wp = interleave_ref(size[b], rows[b], scores[b], k)
        assert np.array_equal(g_rows[b], wr), (b, g_rows[b], wr)
        assert np.array_equal(g_cluster[b], wc) and np.array_equal(g_pos[b], wp), b
        emitted = wr >= 0
        assert g_scores[b][emitted].tobytes() == ws[emitted].tobytes(), b
        assert np.isnan(g_scores[b][~emitted]).all()
    assert (g_rows[0] >= 0).all() and (g_rows[4] == -1).all() and (g_rows[3, -1] == -1 or k < 4)


# ------------------------------------------------------------------------------- 5. end to end ----
def e2e_lists():
    rng = np.random.default_rng(17)
    liked = [rng.choice(np.arange(4, N), size=n, replace=False).tolist()
             for n in (1, 2, 15, 17, 64, 85, 129, 300)]
    liked[2][0] = ZERO_ROW
    exclude = [sorted(set(l) | set(rng.choice(N, size=40, replace=False).tolist())) for l in liked]
    return liked, exclude


@pytest.mark.parametrize("kind,dt,d", [("planted1.0", "f32", 32), ("iid", "bf16", 768)])
def test_one_interest_is_score_topk(cuda_device, catalogs, kind, dt, d):
    ebt = _ebt()[0]
    cat, _ = catalogs(kind, dt, d)
    liked, exclude = e2e_lists()
    for k in (1, 10, 100):
        for ex in (exclude, None):
            s, r = ebt.score_topk(cat, k, liked=liked, exclude=ex)
            got = ebt.multi_interest_topk(cat, k, liked, c=1, exclude=ex)
            assert torch.equal(got.rows, r) and bits(got.scores) == bits(s), (k, ex is None)
            assert (got.cluster == 0).all()
            assert torch.equal(got.pos.long(), torch.arange(k, device=r.device).expand(8, k))
            assert got.size[:, 0].cpu().tolist() == [len(l) for l in liked]


@pytest.mark.parametrize("kind,dt,d", [("planted1.0", "f32", 32), ("planted1.0", "bf16", 768)])
def test_three_interests_end_to_end(cuda_device, catalogs, kind, dt, d):
    """No row twice, no excluded row; every emitted score is score_topk's for that cluster's
    member list, bit for bit; each cluster's rows come in its list's order; the seats taken are
    the D'Hondt seats computed independently when no list ran out."""
    ebt = _ebt()[0]
    cat, _ = catalogs(kind, dt, d)
    liked, exclude = e2e_lists()
    c, k = 3, 10
    got = ebt.multi_interest_topk(cat, k, liked, c=c, exclude=exclude)
    ints = ebt.cluster_liked(cat, liked, c=c)
    assert bits(ints.size) == bits(got.size)
    label, size = ints.label.cpu().numpy(), ints.size.cpu().numpy()
    srows = ints.rows.cpu().numpy()
    med = ints.medoid.cpu().numpy()
    rows, scores, cluster, pos = (x.cpu().numpy() for x in got[:4])
    medoid_row = got.medoid_row.cpu().numpy()
    members, owner = [], []
    for b in range(8):
        for m in range(c):
            if size[b, m] > 0:
                members.append(srows[b][label[b] == m].tolist())
                owner.append((b, m))
            assert medoid_row[b, m] == (srows[b, med[b, m]] if size[b, m] > 0 else -1)
    s, r = ebt.score_topk(cat, k, liked=members, exclude=[exclude[b] for b, _ in owner])
    s, r = s.cpu().numpy(), r.cpu().numpy()
    at = {bm: i for i, bm in enumerate(owner)}
    seats_checked = 0
    for b in range(8):
        out = rows[b]
        n_out = int((out >= 0).sum())
        assert n_out == k and len(set(out.tolist())) == k                 # 2,000 rows: k are found
        assert not set(out.tolist()) & set(exclude[b])
        last = [-1] * c
        for t in range(k):
            m, q = int(cluster[b, t]), int(pos[b, t])
            assert size[b, m] > 0 and q > last[m]                         # its list's order
            last[m] = q
            i = at[b, m]
            assert out[t] == r[i, q] and scores[b, t].tobytes() == s[i, q].tobytes(), (b, t)
        taken = [int((cluster[b] == m).sum()) for m in range(c)]
        if all(last[m] < k - 1 for m in range(c)):                        # nothing ran out
            assert taken == dhondt_seats(size[b].tolist(), k), (b, taken, size[b])
            seats_checked += 1
    assert seats_checked >= 6
    # more than one interest is served where there is more than one
    assert (np.array([len(set(cluster[b].tolist())) for b in range(3, 8)]) == 3).all()


def test_rows_outside_the_catalog_and_shards(cuda_device, catalogs):
    ebt, L, _, _ = _ebt()
    dev = cuda_device
    cat, x = catalogs("planted1.0", "f32", 32)
    liked, _ = e2e_lists()
    for q, bad in ((5, N), (0, -7), (7, N + 123456789)):
        lists = [list(l) for l in liked]
        lists[q][0] = bad
        with pytest.raises(ebt.EbertError, match=f"query {q}"):
            ebt.cluster_liked(cat, lists)
        with pytest.raises(ebt.EbertError, match=f"query {q}"):
            ebt.multi_interest_topk(cat, 10, lists)
    # the C entry itself: the bad query is never read (status -2, all-empty outputs), its
    # neighbours are untouched
    p, c = 17, 3
    r = kernel_lists(p)
    rt = torch.from_numpy(r).to(dev)
    need = L.load().ebt_interest_workspace_bytes(8, p)

    def run(rows_t):
        ws = torch.zeros(need, dtype=torch.uint8, device=dev)
        label = torch.full((8, p), -9, dtype=torch.int32, device=dev)
        size = torch.full((8, c), -9, dtype=torch.int32, device=dev)
        medoid = torch.full((8, c), -9, dtype=torch.int32, device=dev)
        iters = torch.full((8,), -9, dtype=torch.int32, device=dev)
        status = torch.full((8,), -9, dtype=torch.int32, device=dev)
        L.call("ebt_liked_interests", ctypes.byref(cat.cstruct), 8, L.ptr(rows_t), p, c, L.ptr(ws),
               need, L.ptr(label), L.ptr(size), L.ptr(medoid), L.ptr(iters), L.ptr(status),
               L.stream_of(dev))
        return [t.cpu().numpy() for t in (label, size, medoid, iters, status)]

    clean = run(rt)
    assert clean[4].tolist() == [1] * 8
    for q, where, bad_row in ((2, 4, N), (0, 0, -7), (7, p - 1, N + 123456789)):
        bad = r.copy()
        bad[q, where] = bad_row
        got = run(torch.from_numpy(bad).to(dev))
        want = [1] * 8
        want[q] = -2
        assert got[4].tolist() == want
        assert (got[0][q] == -1).all() and (got[1][q] == 0).all() and (got[2][q] == -1).all()
        assert got[3][q] == 0
        for b in range(8):
            if b != q:
                assert all(np.array_equal(g[b], w[b]) for g, w in zip(got[:4], clean[:4])), (q, b)
    shard = ebt.Catalog(torch.from_numpy(x[:1000]).to(dev).float(), row_offset=0, n_global=N)
    with pytest.raises(ebt.EbertError, match="on one device"):
        ebt.cluster_liked(shard, liked)
    with pytest.raises(ebt.EbertError, match="on one device"):
        ebt.multi_interest_topk(shard, 10, liked)


def test_get_user_recs_interests_c1(cuda_device):
    """The C1 catalog and users: one interest is get_user_recs; three interests return k movies,
    none rated, each with its interest's anchor among the user's liked movies."""
    from test_gpu_parity import _collab_setup
    lib, gold = _collab_setup(cuda_device)
    k = 10
    seen = 0
    for uid, rec in gold["users"].items():
        want = rec[f"k{k}"]
        if isinstance(want, dict):
            with pytest.raises(ValueError) as ei:
                lib.get_user_recs_interests(uid, k)
            assert str(ei.value) == want["message"]
            continue
        if not rec["ratings"]:
            assert lib.get_user_recs_interests(uid, k) == []
            continue
        plain = lib.get_user_recs(uid, k)
        one = lib.get_user_recs_interests(uid, k, interests=1)
        assert [(p.movie.tmdb_id, p.score) for p in plain] == \
            [(g.movie.tmdb_id, g.score) for g in one], uid
        assert len({g.anchor_tmdb_id for g in one}) == 1 and {g.interest for g in one} == {0}
        three = lib.get_user_recs_interests(uid, k, interests=3)
        rated = {t for t, _ in rec["ratings"]}
        liked = {t for t, rt in rec["ratings"] if rt >= lib.LIKED_MOVIE_SCORE}
        assert len(three) == len(plain) and len({g.movie.tmdb_id for g in three}) == len(three)
        assert not {g.movie.tmdb_id for g in three} & rated
        assert {g.anchor_tmdb_id for g in three} <= liked
        assert len({(g.interest, g.anchor_tmdb_id) for g in three}) == len({g.interest
                                                                            for g in three})
        seen += 1
    assert seen >= 15
