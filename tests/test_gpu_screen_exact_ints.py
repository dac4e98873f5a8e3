"""Every instantiation of the screening GEMM (screen_gemm.hip) against a float64 matmul, bit for
bit.

The operands are integers in [-4, 4] (exact in f16 and bf16) and the query / row scales are in
{0.5, 1, 2}. With the accumulation rounding of v_mfma_f32_16x16x32 (a product
is truncated to the f32 grid of its 8-group's largest product, C is added with round-to-nearest)
every product, every partial sum in any order (|sum| <= d * 16 <= 2^16 at d = 4096) and both
epilogue multiplications fl(fl(a * qs) * cs) are then exact, so the kernel's scores equal the
float64 reference exactly: a dropped, doubled, stale or misplaced K-slice, row or column is a
failed equality. No comparison here has a tolerance.

Images have the row pitch ld_img = d_pad + 64 (one parameter set per section keeps ld_img == d_pad)
and the 64 pad columns of every catalog and query row hold NaN, as do the row scales past the
catalog's end: whatever reads them turns its scores into NaN. That includes the ODD instantiations,
whose extra all-zero K-tile lies exactly on that pad. Score buffers are pre-filled with NaN and
their columns [N, ld_scores) must still be NaN afterwards.

1. store epilogue of the persistent 256 x 256 kernel: K-tile counts 1, 2, 3, 4, 5, 6, 8, 24 and 64,
   one to three query tiles (three: the walk's division path), two or three tiles per workgroup
   with a ragged last tile group (n_ctiles % 4 = 1, 2, 3) and a ragged last tile (N % 256 = 77).
2. filter epilogue against the reference (not against the store epilogue): thresholds are attained
   integers, so many scores tie with them (>= against >); exact hit sets, counts and overflow
   flags, a starved run with one slot per cell, and queries with thr = +inf.
3. pool epilogue (ebt_cosine_sample / ebt_cosine_sample_lead): the 64-row subgroup maxima over
   the strided / lead tile addressing and the lead tiles' stored scores; the catalog rows between
   the sampled tiles are NaN.
4. the 128 x 128 kernel (B_pad = 128 and 384): the same store and filter checks.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
NAN, INF = float("nan"), float("inf")
BASE, SLOTS, DENSITY = 11, 32, 0.002
I64_MIN = -(1 << 63)
SENTINEL = 0x5A5A5A5A5A5A5A5A     # candidate slots before the launch
COUNT_FILL = 77                   # counts before the launch


def _id(v):
    return {F16: "f16", BF16: "bf16"}.get(v, str(v))


def _scales(g, n, dev):
    table = torch.tensor([0.5, 1.0, 2.0], device=dev)
    return table[torch.randint(0, 3, (n,), generator=g, device=dev)].contiguous()


def _image(g, rows, d, pad, dt, dev):
    """[rows][d + pad] image of integers in [-4, 4], the pad columns NaN."""
    x = torch.full((rows, d + pad), NAN, dtype=dt, device=dev)
    x[:, :d] = torch.randint(-4, 5, (rows, d), generator=g, device=dev).to(dt)
    return x


class _Case:
    """Inputs of one launch and its float64 reference (held as f32: checked to be exact)."""

    def __init__(self, dev, seed, B, N, d, dt, pad, scaled):
        g = torch.Generator(device=dev).manual_seed(seed)
        self.dev, self.B, self.N, self.d, self.ld, self.dt = dev, B, N, d, d + pad, dt
        self.q = _image(g, B, d, pad, dt, dev)
        self.c = _image(g, N, d, pad, dt, dev)
        self.qs = _scales(g, B, dev)
        self.cs = None
        ref = (self.q[:, :d].double() @ self.c[:, :d].double().T) * self.qs.double()[:, None]
        if scaled:
            self.cs = torch.full(((N + 255) // 256 * 256,), NAN, device=dev)
            self.cs[:N] = _scales(g, N, dev)
            ref *= self.cs[:N].double()[None, :]
        self.ref = ref.float()
        assert torch.equal(self.ref.double(), ref)


def _cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _rows_for(dev, nqt, rem):
    """Catalog rows for which every workgroup of the persistent grid walks two or three tiles:
    n_ctiles * nqt in (2 CUs, 3 CUs), n_ctiles % 4 == rem, the last tile 77 rows."""
    cus = _cus(dev)
    n_ctiles = -(-(2 * cus + 8) // nqt)
    while n_ctiles % 4 != rem:
        n_ctiles += 1
    assert 2 * cus < n_ctiles * nqt < 3 * cus
    return 256 * (n_ctiles - 1) + 77


def _check_store(case):
    from robot_ebert_amd import _lib as L
    B, N = case.B, case.N
    ld_s = (N + 3) // 4 * 4 + 4
    S = torch.full((B, ld_s), NAN, device=case.dev)
    L.call("ebt_screen_scores", L.ptr(case.q), B, L.ptr(case.c), N, case.d, case.ld,
           L.DTYPE_CODE[case.dt], L.ptr(case.qs), L.ptr(case.cs), L.ptr(S), ld_s,
           L.stream_of(case.dev))
    torch.cuda.synchronize(case.dev)
    assert torch.isnan(S[:, N:]).all(), "score columns past N were written"
    bad = S[:, :N] != case.ref
    assert not bad.any(), (f"{int(bad.sum())} scores differ, first at (query, row) "
                           f"{bad.nonzero()[0].tolist()}")
    assert torch.equal(S[:, :N], case.ref)


def _composite(s, rows):
    """(f2key(s) << 32) | ~row as int64 with the top bit flipped, so that signed order is the
    composite's unsigned order and I64_MIN stands for 'no hit'."""
    v = s + 0.0                                               # -0.0 -> +0.0
    u = v.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    k = torch.where((u & 0x80000000) != 0, (~u) & 0xFFFFFFFF, u | 0x80000000)
    k = torch.where(torch.isnan(v) | (v == -INF), torch.zeros_like(k), k)
    return ((k << 32) | ((~rows) & 0xFFFFFFFF)[None, :]) ^ I64_MIN


def _thresholds(case):
    """Per query the ceiling of the 0.998 quantile of its first 8192 reference scores, and +inf
    for three queries."""
    n8 = min(8192, case.N)
    thr = torch.ceil(torch.quantile(case.ref[:, :n8].double(), 1.0 - DENSITY, dim=1)).float()
    for b in (3, case.B // 2 + 1, case.B - 1):
        thr[b] = INF
    return thr.contiguous()


def _check_filter(case, thr, G, slots, capped):
    """One ebt_screen_filter launch against the reference. Counts and overflow flags are exact
    for every cell; a cell that fits its slots holds exactly its hit set and leaves the other
    slots untouched; every live slot of any cell, overflowing ones too, holds the composite of a
    distinct true hit of that cell."""
    from robot_ebert_amd import _lib as L
    dev, B, N, ref = case.dev, case.B, case.N, case.ref
    assert int(L.load().ebt_filter_group_rows(B)) == G
    groups = (N + G - 1) // G
    ld_counts = groups + 5
    cand = torch.full((B, groups * slots), SENTINEL, dtype=torch.int64, device=dev)
    counts = torch.full((B, ld_counts), COUNT_FILL, dtype=torch.uint8, device=dev)
    ovf = torch.zeros(B, dtype=torch.int32, device=dev)
    L.call("ebt_screen_filter", L.ptr(case.q), B, L.ptr(case.c), N, case.d, case.ld,
           L.DTYPE_CODE[case.dt], L.ptr(case.qs), L.ptr(case.cs), L.ptr(thr), L.ptr(cand),
           groups * slots, slots, L.ptr(counts), ld_counts, L.ptr(ovf), BASE, L.stream_of(dev))
    torch.cuda.synchronize(dev)

    hit = ref >= thr[:, None]
    pad = groups * G - N
    want_cnt = torch.nn.functional.pad(hit, (0, pad)).view(B, groups, G).sum(-1)
    fits = want_cnt <= slots
    over = int((~fits).sum())
    ties = int((ref == thr[:, None]).sum())
    print(f"B={B} N={N} d={case.d} {case.dt} slots={slots}: {float(want_cnt.sum()) / B:.1f} hits "
          f"per query, largest cell {int(want_cnt.max())}, {over} of {B * groups} cells over "
          f"their slots, {ties} scores equal to their threshold")
    if capped:
        assert over <= 0.01 * B * groups
    else:
        assert over > 0, "the starved run does not overflow"

    assert (counts[:, groups:] == COUNT_FILL).all(), "counts past the groups were written"
    got_cnt = counts[:, :groups].to(torch.int64)
    assert torch.equal(got_cnt, torch.clamp(want_cnt, max=255)), "hit counts differ"
    assert torch.equal(ovf != 0, (~fits).any(dim=1)), "overflow flags differ"

    rows = torch.arange(N, dtype=torch.int64, device=dev)
    comp_all = _composite(ref, rows + BASE)
    comp = torch.where(hit, comp_all, torch.full_like(comp_all, I64_MIN))
    comp = torch.nn.functional.pad(comp, (0, pad), value=I64_MIN).view(B, groups, G)
    want_sorted = comp.sort(dim=-1, descending=True).values[:, :, :slots]
    cand3 = cand.view(B, groups, slots)
    live = (torch.arange(slots, device=dev)[None, None, :]
            < torch.clamp(got_cnt, max=slots)[:, :, None])
    assert (cand3[~live] == SENTINEL).all(), "a slot past the cell's count was written"
    got = torch.where(live, cand3 ^ I64_MIN, torch.full_like(cand3, I64_MIN))
    got_sorted = got.sort(dim=-1, descending=True).values
    assert torch.equal(got_sorted[fits], want_sorted[fits]), "hit sets differ"

    # every live slot: the composite of a true hit inside its own group, no hit twice
    low = cand3 & 0xFFFFFFFF
    row = ((~low) & 0xFFFFFFFF) - BASE
    first = torch.arange(groups, dtype=torch.int64, device=dev)[None, :, None] * G
    inside = (row >= first) & (row < torch.clamp(first + G, max=N))
    at = row.clamp(0, N - 1).view(B, groups * slots)
    same = (cand3 ^ I64_MIN) == comp_all.gather(1, at).view(B, groups, slots)
    true_hit = hit.gather(1, at).view(B, groups, slots)
    assert (inside & same & true_hit)[live].all(), "a slot holds something that is no hit"
    twice = (got_sorted[:, :, 1:] == got_sorted[:, :, :-1]) & (got_sorted[:, :, 1:] != I64_MIN)
    assert not twice.any(), "a hit was stored twice"

    inf_q = torch.isinf(thr)
    assert int(inf_q.sum()) == 3
    assert (got_cnt[inf_q] == 0).all() and (cand[inf_q] == SENTINEL).all()
    return ties


def _check_filter_both(case, G):
    thr = _thresholds(case)
    ties = _check_filter(case, thr, G, SLOTS, capped=True)
    _check_filter(case, thr, G, 1, capped=False)
    return ties


# ---- 1. store epilogue, persistent kernel ---------------------------------------------------
# (d_pad, type, query tiles, n_ctiles % 4 of a catalog of two or three tiles per workgroup -- or
# the catalog's rows when above 3 --, pad columns, row scales)
STORE_CASES = [
    (64, F16, 1, 1, 64, True),
    (64, BF16, 3, 3, 64, True),
    (128, BF16, 2, 2, 64, True),
    (128, F16, 1, 3, 0, False),
    (192, F16, 3, 3, 64, True),
    (192, BF16, 2, 1, 64, False),
    (256, BF16, 1, 2, 64, True),
    (256, F16, 3, 1, 64, True),
    (320, BF16, 3, 1, 64, True),
    (320, F16, 2, 2, 64, True),
    (384, F16, 2, 3, 64, True),
    (384, BF16, 1, 1, 64, False),
    (512, F16, 3, 2, 64, True),
    (512, BF16, 1, 3, 0, True),
    (1536, F16, 1, 256 * 3 + 77, 64, True),
    (1536, BF16, 3, 256 * 3 + 77, 64, True),
    (1536, F16, 2, 256 * 2 + 77, 0, False),
    (4096, F16, 2, 256 + 77, 64, True),
    (4096, BF16, 1, 256 + 77, 64, True),
]


@pytest.mark.parametrize("d,dt,nqt,rows,pad,scaled", STORE_CASES, ids=_id)
def test_store_exact(cuda_device, d, dt, nqt, rows, pad, scaled):
    N = rows if rows > 3 else _rows_for(cuda_device, nqt, rows)
    _check_store(_Case(cuda_device, 1000 + d + nqt, 256 * nqt, N, d, dt, pad, scaled))


# ---- 2. filter epilogue, persistent kernel --------------------------------------------------
# K-tiles after the odd pad: 2 (the clearing instantiation) or >= 4 (ZC); ODD and even
FILTER_CASES = [
    (64, F16, 1, 1, 64, True),      # f16  ODD  clearing
    (64, BF16, 2, 3, 64, False),    # bf16 ODD  clearing
    (128, F16, 2, 2, 64, False),    # f16  even clearing
    (128, BF16, 1, 3, 64, True),    # bf16 even clearing
    (192, F16, 2, 1, 64, True),     # f16  ODD  ZC, K-loop empty
    (320, BF16, 1, 2, 64, False),   # bf16 ODD  ZC, K-loop once
    (256, BF16, 2, 3, 64, True),    # bf16 even ZC, K-loop empty
    (512, F16, 1, 1, 64, False),    # f16  even ZC, K-loop twice
    (384, F16, 1, 2, 0, True),      # ld_img == d_pad
]


@pytest.mark.parametrize("d,dt,nqt,rem,pad,scaled", FILTER_CASES, ids=_id)
def test_filter_exact(cuda_device, d, dt, nqt, rem, pad, scaled):
    N = _rows_for(cuda_device, nqt, rem)
    case = _Case(cuda_device, 2000 + d + nqt, 256 * nqt, N, d, dt, pad, scaled)
    assert _check_filter_both(case, 256) > 0, "no score ties with its threshold"


# ---- 3. pool epilogue -----------------------------------------------------------------------
# (d_pad, type, query tiles, tile stride, lead tiles, pad columns, row scales)
POOL_CASES = [
    (64, F16, 2, 1, 0, 64, True),       # f16  ODD
    (192, BF16, 2, 3, 5, 64, True),     # bf16 ODD
    (128, BF16, 1, 3, 0, 64, True),     # bf16 even
    (256, F16, 2, 1, 5, 64, True),      # f16  even
    (320, F16, 3, 3, 5, 0, False),      # three query tiles, ld_img == d_pad, no row scales
]


@pytest.mark.parametrize("d,dt,nqt,stride,lead,pad,scaled", POOL_CASES, ids=_id)
def test_pool_exact(cuda_device, d, dt, nqt, stride, lead, pad, scaled):
    from robot_ebert_amd import _lib as L
    dev = cuda_device
    B = 256 * nqt
    tiles = -(-(_cus(dev) * 5 // 4) // nqt)     # tiles * nqt > CUs: a second tile for some
    assert tiles * nqt > _cus(dev) and tiles > lead
    g = torch.Generator(device=dev).manual_seed(3000 + d + stride + lead)
    t = torch.arange(tiles, dtype=torch.int64, device=dev)
    row0 = 256 * torch.where(t < lead, t, lead + (t - lead) * stride)
    n_rows = int(row0[-1]) + 256
    idx = (row0[:, None] + torch.arange(256, device=dev)[None, :]).reshape(-1)  # image rows
    ns = tiles * 256                                                           # sample rows

    q = _image(g, B, d, pad, dt, dev)
    qs = _scales(g, B, dev)
    ci = torch.randint(-4, 5, (ns, d), generator=g, device=dev).to(dt)
    cs_s = _scales(g, ns, dev)
    # subgroup sg: row pos(sg) of its 64 is a copy of query sg % B with the largest row scale, so
    # that query's maximum sits there; pos walks all 64 places (accumulator i = pos // 16, 16-lane
    # group (pos % 16) // 4, element pos % 4)
    sg = torch.arange(tiles * 4, dtype=torch.int64, device=dev)
    place = sg * 64 + (sg * 21 + 5) % 64
    assert len(set(((sg * 21 + 5) % 64).tolist())) == 64
    ci[place] = q[sg % B, :d]
    cs_s[place] = 2.0
    # everything outside the sample is NaN: the rows between the tiles, their scales, the pad
    c = torch.full((n_rows, d + pad), NAN, dtype=dt, device=dev)
    c[idx, :d] = ci
    cs = None
    if scaled:
        cs = torch.full((n_rows,), NAN, device=dev)
        cs[idx] = cs_s
        if stride > 1:   # a tile's logical rows 256 t .. carry other scales than its image rows
            assert (cs[:ns] != cs_s).any()
    else:
        cs_s = torch.ones_like(cs_s)
    ref64 = (q[:, :d].double() @ ci.double().T) * qs.double()[:, None] * cs_s.double()[None, :]
    ref = ref64.float()
    assert torch.equal(ref.double(), ref64)
    want = ref.view(B, tiles * 4, 64).max(dim=-1).values
    assert torch.equal(want[sg % B, sg], ref[sg % B, place]), "a placed row is no maximum"

    ld_p = tiles * 4 + 4
    pooled = torch.full((B, ld_p), NAN, device=dev)
    st = L.stream_of(dev)
    code = L.DTYPE_CODE[dt]
    if lead == 0:
        L.call("ebt_cosine_sample", L.ptr(q), L.ptr(qs), B, L.ptr(c), L.ptr(cs), code, d + pad,
               n_rows, d, tiles, stride, L.ptr(pooled), ld_p, None, st)
    else:
        ld_l = 256 * lead + 4
        lead_s = torch.full((B, ld_l), NAN, device=dev)
        L.call("ebt_cosine_sample_lead", L.ptr(q), L.ptr(qs), B, L.ptr(c), L.ptr(cs), code,
               d + pad, n_rows, d, tiles, stride, L.ptr(pooled), ld_p, lead, L.ptr(lead_s), ld_l,
               None, st)
    torch.cuda.synchronize(dev)
    assert torch.isnan(pooled[:, tiles * 4:]).all(), "pooled columns past the sample were written"
    bad = pooled[:, :tiles * 4] != want
    assert not bad.any(), (f"{int(bad.sum())} subgroup maxima differ, first at (query, subgroup) "
                           f"{bad.nonzero()[0].tolist()}")
    assert torch.equal(pooled[:, :tiles * 4], want)
    if lead:
        assert torch.isnan(lead_s[:, 256 * lead:]).all(), "lead columns past the lead were written"
        assert torch.equal(lead_s[:, :256 * lead], ref[:, :256 * lead]), "lead scores differ"


# ---- 4. the 128 x 128 kernel ----------------------------------------------------------------
@pytest.fixture(scope="module", params=[(B, N, d, dt) for B in (128, 384)
                                        for N in (128 * 5 + 77, 128 * 17 + 1)
                                        for d in (64, 192, 1536) for dt in (F16, BF16)],
                ids=lambda p: f"B{p[0]}-N{p[1]}-d{p[2]}-{_id(p[3])}")
def small_case(request, cuda_device):
    B, N, d, dt = request.param
    # ld_img == d_pad at B = 384, d = 192; no row scales at d = 64 in f16 and d = 192 in bf16
    pad = 0 if (B, d) == (384, 192) else 64
    scaled = (d, dt) not in ((64, F16), (192, BF16))
    return _Case(cuda_device, 4000 + B + N + d, B, N, d, dt, pad, scaled)


def test_small_store_exact(small_case):
    _check_store(small_case)


def test_small_filter_exact(small_case):
    _check_filter_both(small_case, 128)
