"""The filter screening GEMM's zero-C instantiation (screen_gemm.hip, ZC: a tile's first K-tile
pair runs ahead of the K-loop with MFMAs whose C operand is the constant 0, and the accumulators
are never cleared) against the store epilogue of the same kernel, which never takes that path.

A stale accumulator can show only from a workgroup's SECOND tile on, so the catalog has
256 * 520 + 77 rows: 521 catalog tiles on one query tile, two or three tiles for every workgroup
of a 256-workgroup grid, the last tile ragged. d walks the K-tile counts at which the tile's
K-loop changes shape: 2 K-tiles (the clearing instantiation, the boundary pair is the whole tile),
3 -> 4 and 4 (peeled pair + boundary pair, loop empty), 5 -> 6 and 6 (loop runs once), 8 (twice),
each for an f16 and a bf16 image, with and without row scales.

Per (query, 256-row group) whose hits fit the 32 slots the hit set must be EXACTLY
{(f2key(s) << 32) | ~row : s >= thr} of the stored scores, the counts equal, and the overflow flag
set exactly for the queries with a group over its slots. The threshold is each query's 0.998
quantile of its first 8192 stored scores: a 256-row group then holds 0.5 hits on average, and at
most 1 % of the cells may overflow (asserted). Everything is compared on the device (the score
matrix is 136 MB).

The second test drives the whole path: score_topk over a 300 000 x 256 f16 catalog (1172 catalog
tiles, four or five per workgroup of the fused speculative screen) against the float64 oracle."""
import numpy as np
import pytest
import torch

from inputs import gaussian
from oracle import restatement as R

pytestmark = pytest.mark.gpu

B, N, BASE, SLOTS = 256, 256 * 520 + 77, 11, 32
DENSITY = 0.002
I64_MIN = -(1 << 63)


def _composite(s, rows):
    """(f2key(s) << 32) | ~row as int64 with the top bit flipped, so that signed order is the
    composite's unsigned order and I64_MIN stands for 'no hit'."""
    v = s + 0.0                                               # -0.0 -> +0.0
    u = v.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    k = torch.where((u & 0x80000000) != 0, (~u) & 0xFFFFFFFF, u | 0x80000000)
    k = torch.where(torch.isnan(v) | (v == float("-inf")), torch.zeros_like(k), k)
    return ((k << 32) | ((~rows) & 0xFFFFFFFF)[None, :]) ^ I64_MIN


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("d", [128, 192, 256, 320, 384, 512])
def test_filter_matches_store_many_tiles(cuda_device, d, dt, scaled):
    from robot_ebert_amd import _lib as L
    dev = cuda_device
    g = torch.Generator(device=dev).manual_seed(29 + d)
    q = torch.randn((B, d), generator=g, device=dev).to(dt)
    c = torch.randn((N, d), generator=g, device=dev).to(dt)
    qs = (torch.rand(B, generator=g, device=dev) + 0.5).contiguous()
    cs = ((torch.rand((N + 255) // 256 * 256, generator=g, device=dev) + 0.5).contiguous()
          if scaled else None)
    st = L.stream_of(dev)
    code = L.DTYPE_CODE[dt]
    ld = (N + 3) // 4 * 4
    S = torch.full((B, ld), float("nan"), device=dev)
    L.call("ebt_screen_scores", L.ptr(q), B, L.ptr(c), N, d, d, code, L.ptr(qs), L.ptr(cs),
           L.ptr(S), ld, st)
    S = S[:, :N]
    thr = torch.quantile(S[:, :8192], 1.0 - DENSITY, dim=1).contiguous()
    G = int(L.load().ebt_filter_group_rows(B))
    assert G == 256
    groups = (N + G - 1) // G
    assert groups == 521
    cand = torch.zeros((B, groups * SLOTS), dtype=torch.int64, device=dev)
    counts = torch.zeros((B, groups), dtype=torch.uint8, device=dev)
    ovf = torch.zeros(B, dtype=torch.int32, device=dev)
    L.call("ebt_screen_filter", L.ptr(q), B, L.ptr(c), N, d, d, code, L.ptr(qs), L.ptr(cs),
           L.ptr(thr), L.ptr(cand), groups * SLOTS, SLOTS, L.ptr(counts), groups, L.ptr(ovf),
           BASE, st)
    torch.cuda.synchronize(dev)

    hit = S >= thr[:, None]
    pad = groups * G - N
    want_cnt = torch.nn.functional.pad(hit, (0, pad)).view(B, groups, G).sum(-1)
    rows = torch.arange(N, dtype=torch.int64, device=dev) + BASE
    comp = torch.where(hit, _composite(S, rows), torch.full_like(rows, I64_MIN)[None, :])
    comp = torch.nn.functional.pad(comp, (0, pad), value=I64_MIN).view(B, groups, G)
    want_sorted = comp.sort(dim=-1, descending=True).values[:, :, :SLOTS]

    got_cnt = counts.to(torch.int64)
    live = (torch.arange(SLOTS, device=dev)[None, None, :]
            < torch.clamp(got_cnt, max=SLOTS)[:, :, None])
    got = torch.where(live, cand.view(B, groups, SLOTS) ^ I64_MIN,
                      torch.full_like(live, I64_MIN, dtype=torch.int64))
    got_sorted = got.sort(dim=-1, descending=True).values

    fits = want_cnt <= SLOTS
    over = int((~fits).sum())
    print(f"d={d} {dt} scaled={scaled}: {float(want_cnt.sum()) / B:.0f} hits per query, "
          f"{over} of {B * groups} cells over their slots")
    assert over <= 0.01 * B * groups
    assert torch.equal(got_cnt[fits], want_cnt[fits])
    assert torch.equal(got_cnt[~fits], torch.clamp(want_cnt[~fits], max=255))
    assert torch.equal(got_sorted[fits], want_sorted[fits]), "hit sets differ"
    assert torch.equal(ovf != 0, (~fits).any(dim=1))


def test_score_topk_many_tiles_per_workgroup(cuda_device):
    import robot_ebert_amd as ebt
    dev = cuda_device
    n, d, b, k = 300_000, 256, 256, 10
    c = gaussian(51, n, d, "f16")
    q = gaussian(52, b, d, "f16")
    cat = ebt.Catalog(torch.from_numpy(np.ascontiguousarray(c)).to(dev).half())
    s, r = ebt.score_topk(cat, k, queries=torch.from_numpy(np.ascontiguousarray(q)).to(dev).half())
    s_ref, r_ref = R.cosine_topk(q, c, k)
    np.testing.assert_array_equal(r.cpu().numpy(), r_ref)
    err = float(np.max(np.abs(s.cpu().numpy() - s_ref)))
    print(f"max |score - oracle| = {err:.3g}")
    assert err <= 1e-5
