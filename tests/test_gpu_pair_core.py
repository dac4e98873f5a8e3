"""GPU: the two float64 MFMA pair-product kernels give the same dot-product bits (csrc/pair_f64.h).

    contrib(b, j, l) = (w_l * ((x_l . x_j) / (g_l * g_j))) * (1 / W_b)      liked_contrib_kernel
    gram(b, i, j)    = (x_i . x_j) / (g_i * g_j)                            pool_gram_kernel

With no weights w_l = 1 and W_b = L_b, and with L_b a power of two 1 / W_b is an exact power of
two, so contrib(b, j, l) * L_b is dot / (g * g'), rounded once, times exact factors: it must equal
gram(b, slot(j), slot(l)) BIT FOR BIT, slot(r) the index of row r in pool b. The two kernels stage
and accumulate through the same code with different workgroup shapes, pipelines and operand roles
(a liked row is a B operand there, an A or B operand here), so equality pins the header's claim
that the order of a dot product depends on d and the dtype only.

Shapes: a catalog of 2,000 rows, 4 queries; (p, L) = (17, 1) crosses the 16-wide MFMA tile and
needs no scaling, (17, 16), and (129, 128): two workgroup tiles per side of the Gram matrix
(off-diagonal and mirrored tiles) and two liked panels (96 + 32) of the contribution kernel.
d = 77 is the element path. A pool is p slots: p - 1 distinct rows and one -1; the liked list is
L of the pool's rows in another order than the pool's."""
import numpy as np
import pytest
import torch

from inputs import gaussian

pytestmark = pytest.mark.gpu
N = 2000
B = 4
ZERO_ROW = 3
TORCH_DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16,
            "f64": torch.float64}
POS_ZERO = np.float64(0.0).tobytes()


@pytest.fixture(scope="module")
def catalogs(cuda_device):
    """One 2,000-row catalog per (dtype, d), row 3 zero; the last one is kept."""
    import robot_ebert_amd as ebt
    made = {}

    def get(dt, d):
        if (dt, d) not in made:
            made.clear()
            x = gaussian(91, N, d, dt)
            x[ZERO_ROW] = 0.0
            xt = torch.from_numpy(np.ascontiguousarray(x)).to(cuda_device).to(TORCH_DT[dt])
            made[dt, d] = ebt.Catalog(xt)
        return made[dt, d]
    return get


def make_pools(p, L):
    """(pool [B, p] with one -1 slot per query, liked lists of L pool rows in another order); the
    zero-norm row is in every pool and, where L > 1, in every liked list."""
    rng = np.random.default_rng(1000 * p + L)
    pool = np.empty((B, p), dtype=np.int64)
    liked = []
    for b in range(B):
        others = rng.choice(np.setdiff1d(np.arange(N), [ZERO_ROW]), size=p - 2, replace=False)
        rows = rng.permutation(np.concatenate([others, [ZERO_ROW]]))
        pool[b] = np.insert(rows, (5 * b + p // 2) % p, -1)
        order = rng.permutation(rows)
        while L > 1 and np.array_equal(order, rows):
            order = rng.permutation(rows)
        if L > 1 and ZERO_ROW not in order[:L]:
            at = np.flatnonzero(order == ZERO_ROW)[0]
            order[0], order[at] = order[at], order[0]
        liked.append(order[:L].tolist())
    return pool, liked


@pytest.mark.parametrize("p,L", [(17, 1), (17, 16), (129, 128)])   # (varies fastest)
@pytest.mark.parametrize("d", [32, 77, 768])
@pytest.mark.parametrize("dt", ["f32", "bf16", "f16", "f64"])
def test_contrib_times_L_has_the_gram_entry_bits(cuda_device, catalogs, dt, d, p, L):
    from robot_ebert_amd import diversify, explain
    cat = catalogs(dt, d)
    pool, liked = make_pools(p, L)
    rows = torch.from_numpy(pool).to(cuda_device)
    gram, gstatus = diversify.pool_gram(cat, rows)
    out, cstatus, off, _ = explain.liked_contrib(cat, rows, liked)
    assert gstatus.cpu().tolist() == [1] * B and cstatus.cpu().tolist() == [1] * B
    assert off.cpu().tolist() == [L * b for b in range(B + 1)]
    gram = gram.cpu().numpy()
    contrib = out.cpu().numpy().reshape(B, p, L)       # every query has L liked rows: [k = p, L]
    for b in range(B):
        empty = pool[b] < 0
        slot = {int(r): i for i, r in enumerate(pool[b]) if r >= 0}
        cols = np.array([slot[r] for r in liked[b]])
        assert L == 1 or not np.array_equal(pool[b][~empty][:L], np.asarray(liked[b]))
        # NaN exactly on the empty slot, in both
        assert np.array_equal(np.isnan(gram[b]), empty[:, None] | empty[None, :]), b
        assert np.array_equal(np.isnan(contrib[b]), np.repeat(empty[:, None], L, axis=1)), b
        scaled = contrib[b][~empty] * float(L)         # exact: L is a power of two
        want = gram[b][~empty][:, cols]
        assert scaled.tobytes() == np.ascontiguousarray(want).tobytes(), (b, np.argwhere(
            scaled.view(np.uint64) != np.ascontiguousarray(want).view(np.uint64))[:5].tolist())
        # +0.0 on the zero-norm row, as a result row and as a liked row, in both
        z = slot[ZERO_ROW]
        assert gram[b][z][~empty].tobytes() == POS_ZERO * (p - 1), b
        assert gram[b][~empty][:, z].tobytes() == POS_ZERO * (p - 1), b
        assert contrib[b][z].tobytes() == POS_ZERO * L, b
        if ZERO_ROW in liked[b]:
            col = contrib[b][~empty][:, liked[b].index(ZERO_ROW)]
            assert np.ascontiguousarray(col).tobytes() == POS_ZERO * (p - 1), b
