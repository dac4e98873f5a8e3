"""The exact screen (screen_exact_kernel) and the full-sort path (exact_keys_kernel, min(k, n) >
4096) run ONE float64 FMA tile (csrc/exact_tile_f64.h), so they hold the same float64 value per
(query, row): the full sort's score, rounded once to float32, IS the exact screen's entry -- no
tolerance. Shapes: the smallest at which every edge of the 64 x 64 x 16 tile is ragged and the
full-sort path is reached (n = 4200 = 65 * 64 + 40 > 4096, d = 100 = 6 * 16 + 4, B = 70 = 64 + 6),
with an all-zero row (the guarded norm) and a row holding a NaN.

The queries are +-1 on 64 of the 100 positions and 0 elsewhere: their norm is exactly 8 and the
normalised query exactly +-0.125 in float64 whichever prep kernel made it, so ebt_screen_exact
may take a host-built q64 while score_topk prepares its own."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, D, B = 4200, 100, 70
ZERO_ROW, NAN_ROW = 70, 4180
TORCH_DT = {"f32": torch.float32, "bf16": torch.bfloat16}


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_exact_screen_and_full_sort_share_bits(cuda_device, dt):
    import robot_ebert_amd as ebt
    from robot_ebert_amd import _lib as L
    rng = np.random.default_rng(19)
    c = rng.standard_normal((N, D)).astype(np.float32)
    c[ZERO_ROW] = 0.0
    c[NAN_ROW, 37] = np.nan
    q = np.zeros((B, D), dtype=np.float32)
    for b in range(B):
        q[b, rng.choice(D, 64, replace=False)] = rng.choice([-1.0, 1.0], 64)
    ct = torch.from_numpy(c).to(cuda_device).to(TORCH_DT[dt])
    qt = torch.from_numpy(q).to(cuda_device).to(TORCH_DT[dt])   # +-1 and 0: exact in bf16

    # the full sort: k = n, every row but the NaN one
    cat = ebt.Catalog(ct)
    s, r = ebt.score_topk(cat, N, queries=qt)
    s, r = s.cpu().numpy(), r.cpu().numpy()

    # the exact screen on the same rows and norms, q64 built on the host
    g = torch.empty(N, dtype=torch.float64, device=cuda_device)
    L.call("ebt_row_norms", L.ptr(ct), L.DTYPE_CODE[ct.dtype], N, D, D, L.ptr(g), None,
           L.stream_of(cuda_device))
    q64 = torch.from_numpy(q.astype(np.float64) / 8.0).to(cuda_device)
    ld_s = N + 3
    S = torch.full((B, ld_s), float("nan"), device=cuda_device)
    L.call("ebt_screen_exact", L.ptr(q64), B, D, L.ptr(ct), L.DTYPE_CODE[ct.dtype], D, L.ptr(g), N,
           L.ptr(S), ld_s, L.stream_of(cuda_device))
    S = S.cpu().numpy()

    assert g[ZERO_ROW].item() == 1.0
    assert s.shape == (B, N) and r.shape == (B, N)
    # the NaN row: in no list (the last slot is empty), -inf in the screen
    assert not (r == NAN_ROW).any()
    assert (r[:, :N - 1] >= 0).all()
    assert (r[:, N - 1] == -1).all() and np.isnan(s[:, N - 1]).all()
    assert np.all(S[:, NAN_ROW] == -np.inf)
    # the padding columns are untouched
    assert np.isnan(S[:, N:]).all()
    # every valid slot: the same float64 value, rounded once
    rows = r[:, :N - 1]
    assert all(np.array_equal(np.sort(rows[b]), np.delete(np.arange(N), NAN_ROW)) for b in range(B))
    got = s[:, :N - 1].astype(np.float32)
    want = np.take_along_axis(S, rows, axis=1)
    bad = np.nonzero(got != want)
    assert bad[0].size == 0, (bad[0][:5], bad[1][:5], got[bad][:5], want[bad][:5])
    assert np.all(S[:, ZERO_ROW] == 0.0)
