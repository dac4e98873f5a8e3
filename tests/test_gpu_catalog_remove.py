"""GPU: removing catalog rows in place (Catalog.remove, ebt_catalog_remove_rows /
ebt_catalog_remove_plan, RecBatcher.remove).

With n' = n - m, the removed rows below n' (the holes, ascending) receive the rows of [n', n) that
are not removed (the survivors, ascending). The state afterwards must be BITWISE the state of a
catalog built afresh from the edited matrix (data, guarded float64 norms, float32 inverse norms,
image), u_cat is kept, and every result must equal the float64 oracle on the host matrix with the
same edit applied."""
import ctypes
import os

import numpy as np
import pytest
import torch

from inputs import gaussian
from oracle import restatement as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TDT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "f64": torch.float64}
N, M, B = 1000, 37, 64
ATOL = 1e-10


def _t(x, dt, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev).to(TDT[dt])


def _bits(t):
    return t.contiguous().view(torch.uint8)


def _up(v, m):
    return (v + m - 1) // m * m


def _excl(n):
    return [list(range(b, n, 97)) for b in range(B)]


def _rule(n, rows):
    """The rule restated on the host: (holes, survivors, n')."""
    rows = np.asarray(sorted(rows), dtype=np.int64)
    n_new = n - len(rows)
    holes = rows[rows < n_new]
    tail = np.arange(n_new, n)
    surv = tail[~np.isin(tail, rows)]
    assert len(holes) == len(surv)
    return holes, surv, n_new


def _edited(c, rows):
    """c2 = c.copy(); c2[H] = c[S]; c2 = c2[:n'] -- on a matrix or a list of ids."""
    holes, surv, n_new = _rule(len(c), rows)
    if isinstance(c, list):
        c2 = list(c)
        for h, s in zip(holes, surv):
            c2[h] = c[s]
        return c2[:n_new]
    c2 = c.copy()
    c2[holes] = c[surv]
    return c2[:n_new]


def _moves(n, rows):
    holes, surv, _ = _rule(n, rows)
    return [(int(s), int(h)) for s, h in zip(surv, holes)]


def _removal(seed, n, m=M):
    """m distinct rows in no order, row 0, row n-1 and row n-2 among them, row n-3 not."""
    rng = np.random.default_rng(seed)
    rest = [int(r) for r in rng.permutation(np.arange(1, n - 3))]
    rows = [n - 1, 0, n - 2] + rest[:m - 3]
    return [rows[i] for i in rng.permutation(m)]


def _catalog(seed, n, d, dt):
    """Gaussian rows with an all-zero row (guarded norm 1.0) at n-3: one of the moved survivors."""
    c = gaussian(seed, n, d, dt)
    c[n - 3] = 0.0
    return c


def assert_state_equal(cat, fresh):
    n = fresh.n
    assert cat.n == n == cat.cstruct.n and cat.ld_img == fresh.ld_img
    assert cat.native == fresh.native
    assert torch.equal(_bits(cat.data), _bits(fresh.data)), "data"
    assert torch.equal(_bits(cat.gnorm), _bits(fresh.gnorm)), "gnorm"
    assert cat.inv32.numel() == _up(n, 128) == fresh.inv32.numel()
    assert torch.equal(_bits(cat.inv32), _bits(fresh.inv32)), "inv32"
    assert torch.equal(_bits(cat.image), _bits(fresh.image)), "image"
    if fresh.native:
        assert cat.u_cat == 0.0 and cat.cstruct.u_cat == 0.0
    else:
        assert fresh.u_cat <= cat.u_cat <= 2.0 ** -11, (fresh.u_cat, cat.u_cat)
        assert cat.cstruct.u_cat == np.float32(cat.u_cat)


def assert_topk(s, r, s_ref, r_ref):
    s = s.cpu().numpy() if torch.is_tensor(s) else s
    r = r.cpu().numpy() if torch.is_tensor(r) else r
    np.testing.assert_array_equal(r, r_ref)
    m = r_ref >= 0
    np.testing.assert_allclose(s[m], s_ref[m], rtol=0, atol=ATOL)


def _inv32_all(cat):
    """inv32 over the whole capacity (the view cat.inv32 stops at round_up(n, 128))."""
    off = _up(cat.capacity * 8, 256)
    return cat.state[off:off + _up(cat.capacity, 128) * 4].view(torch.float32)


# ---- 1. the state equals a fresh build ---------------------------------------------------------
# d = 64: the 16-bit catalogs' matrix is their image; 70: ragged (an element tail after the 16-byte
# chunks, a separate raw image for 16-bit); 1536: more than one chunk per lane for f32 / f64;
# 2100: more chunks per lane than the kernel keeps in flight, and a tail
@pytest.mark.parametrize("dt, d", [(dt, d) for d in (64, 70, 1536)
                                   for dt in ("f32", "f64", "f16", "bf16")] + [("f32", 2100)])
def test_state_equals_fresh_build(cuda_device, dt, d):
    import robot_ebert_amd as ebt
    c = _catalog(1, N, d, dt)
    rows = _removal(11, N)
    assert 0 in rows and N - 1 in rows and N - 2 in rows and N - 3 not in rows
    cat = ebt.Catalog(_t(c, dt, cuda_device))
    moves = cat.remove(rows)
    assert moves == _moves(N, rows) and N - 3 in [s for s, _ in moves]
    want = _edited(c, rows)
    assert len(want) == N - M
    assert_state_equal(cat, ebt.Catalog(_t(want, dt, cuda_device)))
    assert bool((_inv32_all(cat)[N - M:] == 1.0).all())


# ---- 2. ld > d: a column slice of a wider tensor -----------------------------------------------
# f32 70 / 96: aligned rows with a tail; f64 70 / 75: unaligned rows (the element loop); bf16
# 64 / 128: the slice itself is the image; f16 64 / 72: aligned rows, a separate image
@pytest.mark.parametrize("dt, d, ld", [("f32", 70, 96), ("f64", 70, 75), ("bf16", 64, 128),
                                       ("f16", 64, 72)])
def test_state_equals_fresh_build_strided(cuda_device, dt, d, ld):
    import robot_ebert_amd as ebt
    c = _catalog(3, N, ld, dt)
    rows = _removal(13, N)
    wide = _t(c, dt, cuda_device)
    cat = ebt.Catalog(wide[:, :d])
    assert cat.ld == ld
    cat.remove(rows)
    n_new = N - M
    want = c[:n_new].copy()                       # the columns past d stay where they are
    want[:, :d] = _edited(c, rows)[:, :d]
    assert torch.equal(_bits(wide[:n_new]), _bits(_t(want, dt, cuda_device))), \
        "columns past d touched (or a row not moved)"
    assert_state_equal(cat, ebt.Catalog(_t(want, dt, cuda_device)[:, :d]))


# ---- 3. boundaries of n -------------------------------------------------------------------------
def _boundary_rows(n, m):
    if m == 2:
        return [3, n - 1]
    rng = np.random.default_rng(n)
    return [int(r) for r in rng.choice(n, m, replace=False)]


# 1025 -> 1023: the last 128-row pad and 256-row tile disappear; 1000 -> 890: across the 128-row
# boundary at 896; 257 -> 255: below one 256-row tile
@pytest.mark.parametrize("n, m", [(1025, 2), (1000, 110), (257, 2)])
@pytest.mark.parametrize("dt, d", [("f32", 70), ("bf16", 64)])
def test_boundaries_of_n(cuda_device, dt, d, n, m):
    import robot_ebert_amd as ebt
    c = _catalog(1, n, d, dt)
    q = gaussian(2, B, d, dt)
    rows = _boundary_rows(n, m)
    cat = ebt.Catalog(_t(c, dt, cuda_device))
    cat.remove(rows)
    want = _edited(c, rows)
    assert cat.n == n - m == len(want)
    assert_state_equal(cat, ebt.Catalog(_t(want, dt, cuda_device)))
    assert bool((_inv32_all(cat)[n - m:] == 1.0).all())
    excl = _excl(n - m)
    qt = _t(q, dt, cuda_device)
    for k in (10, 100):
        s, r = ebt.score_topk(cat, k, queries=qt, exclude=excl)
        assert_topk(s, r, *R.cosine_topk(q, want, k, excl))


# ---- 4. only tail rows removed: no move ---------------------------------------------------------
@pytest.mark.parametrize("dt, d", [("f32", 70), ("f16", 64)])
def test_tail_only_moves_nothing(cuda_device, dt, d):
    import robot_ebert_amd as ebt
    c = _catalog(1, N, d, dt)
    cat = ebt.Catalog(_t(c, dt, cuda_device))
    n_new = N - M
    before = [x[:n_new].clone() for x in (cat.data, cat.gnorm, cat.image)]
    assert cat.remove(list(range(N - 1, n_new - 1, -1))) == []
    assert cat.n == n_new
    for x, b in zip((cat.data, cat.gnorm, cat.image), before):
        assert torch.equal(_bits(x), _bits(b))
    assert bool((_inv32_all(cat)[n_new:_up(N, 128)] == 1.0).all())
    assert_state_equal(cat, ebt.Catalog(_t(c[:n_new], dt, cuda_device)))


# ---- 5. every survivor moves ---------------------------------------------------------------------
@pytest.mark.parametrize("dt, d", [("f32", 70), ("f64", 64), ("bf16", 64), ("f16", 70)])
def test_every_survivor_moves(cuda_device, dt, d):
    import robot_ebert_amd as ebt
    c = _catalog(1, N, d, dt)
    cat = ebt.Catalog(_t(c, dt, cuda_device))
    moves = cat.remove(range(600))
    assert moves == [(600 + i, i) for i in range(400)]
    assert_state_equal(cat, ebt.Catalog(_t(c[600:], dt, cuda_device)))


# ---- 6. results -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dt, d", [("f32", 70), ("bf16", 64), ("f64", 1536)])
def test_results_after_removal(cuda_device, dt, d):
    import robot_ebert_amd as ebt
    c = _catalog(1, N, d, dt)
    q = gaussian(2, B, d, dt)
    rows = _removal(31, N)
    # query 3's top-1 is removed as well: it must stop being recommended
    _, r0 = R.cosine_topk(q, c, 10, _excl(N))
    top = int(r0[3, 0])
    if top not in rows and top != N - 3:
        rows[rows.index(next(r for r in rows if r not in (0, N - 1, N - 2)))] = top
    ids = [f"m{i}" for i in range(N)]
    cat = ebt.Catalog(_t(c, dt, cuda_device), ids=ids)
    moves = cat.remove([ids[r] for r in rows])                   # by id
    assert moves == _moves(N, rows)
    want, want_ids = _edited(c, rows), _edited(ids, rows)
    n_new = N - M
    assert cat.ids == want_ids and cat.n == cat.n_global == n_new
    gone = {ids[r] for r in rows}
    assert cat.contains([ids[r] for r in rows]) == [False] * M
    assert cat.rows_of([ids[s] for s, _ in moves]) == [t for _, t in moves]
    assert cat.rows_of(want_ids) == list(range(n_new))
    # dense queries with exclusions
    qt = _t(q, dt, cuda_device)
    excl = _excl(n_new)
    for k in (10, 100):
        s, r = ebt.score_topk(cat, k, queries=qt, exclude=excl)
        assert_topk(s, r, *R.cosine_topk(q, want, k, excl))
        for x in r.cpu().numpy().ravel():
            assert cat.id_of(int(x)) == want_ids[int(x)] and want_ids[int(x)] not in gone
    # liked lists held as OLD rows, moved rows among them, translated through the returned moves
    new_of = dict(moves)
    moved = [s for s, _ in moves]
    f = [r for r in range(1, n_new) if r not in rows][:4]        # rows that keep their number
    old = [[moved[0], f[0]], [N - 3, f[1]], [moved[1], moved[2], f[1]], [f[2], f[3]],
           [moved[-1], moved[0]]]
    assert all(r not in rows for l in old for r in l)
    liked = [sorted(new_of.get(r, r) for r in l) for l in old]
    rated = [sorted(set(l + [8, 9])) for l in liked]
    for k in (10, 100):
        s, r = ebt.score_topk(cat, k, liked=liked, exclude=rated)
        assert_topk(s, r, *R.liked_topk(want, liked, k, rated))


# ---- 7. remove, then append into the freed rows -------------------------------------------------
@pytest.mark.parametrize("dt, d", [("f32", 70), ("bf16", 64)])
def test_remove_then_append(cuda_device, dt, d):
    import robot_ebert_amd as ebt
    c = _catalog(1, N, d, dt)
    more = gaussian(5, 51, d, dt)
    rows = _removal(41, N)
    ids = [f"m{i}" for i in range(N)]
    new_ids = [f"x{i}" for i in range(51)]
    cat = ebt.Catalog(_t(c, dt, cuda_device), ids=ids, capacity=N + 13)
    cat.remove(rows)
    mt = _t(more, dt, cuda_device)
    cat.append(mt[:50], ids=new_ids[:50])                        # 963 + 50 = N + 13
    want = np.concatenate([_edited(c, rows), more[:50]])
    want_ids = _edited(ids, rows) + new_ids[:50]
    assert cat.n == cat.n_global == N + 13 == cat.capacity
    assert_state_equal(cat, ebt.Catalog(_t(want, dt, cuda_device)))
    assert cat.ids == want_ids
    assert cat.rows_of(want_ids) == list(range(N + 13))
    assert cat.contains([ids[r] for r in rows]) == [False] * M
    assert all(cat.contains(want_ids))
    with pytest.raises(ebt.EbertError):
        cat.append(mt[50:51], ids=new_ids[50:51])                # past the capacity
    assert cat.n == N + 13
    q = gaussian(2, B, d, dt)
    excl = _excl(N + 13)
    s, r = ebt.score_topk(cat, 10, queries=_t(q, dt, cuda_device), exclude=excl)
    assert_topk(s, r, *R.cosine_topk(q, want, 10, excl))


# ---- 8. refusals change nothing ------------------------------------------------------------------
def _snapshot(cat):
    out = {}
    for k, v in vars(cat).items():
        if torch.is_tensor(v):
            out[k] = (v.data_ptr(), tuple(v.shape), tuple(v.stride()), v.dtype)
        elif isinstance(v, ctypes.Structure):
            out[k] = bytes(v)
        elif isinstance(v, (list, dict)):
            out[k] = type(v)(v)
        else:
            out[k] = v
    dev = [cat._store.clone()] + ([cat.state.clone()] if cat.state is not None else
                                  [cat.gnorm.clone(), cat.inv32.clone(), cat.image.clone()])
    return out, dev


def test_refusals_change_nothing(cuda_device):
    import robot_ebert_amd as ebt
    dt, d = "f32", 70
    c = _catalog(1, N, d, dt)
    ids = [f"m{i}" for i in range(N)]
    cat = ebt.Catalog(_t(c, dt, cuda_device), ids=ids, capacity=N + 10)
    assert cat.rows_of(["m5"]) == [5]            # the id -> row map is built on first use
    plain = ebt.Catalog(_t(c, dt, cuda_device))
    parts = ebt.Catalog.from_parts(plain.data, plain.gnorm, plain.inv32, plain.image)
    shard = ebt.Catalog(_t(c[:500], dt, cuda_device), row_offset=0, n_global=N)
    later = ebt.Catalog(_t(c[500:], dt, cuda_device), row_offset=500, n_global=N)
    for target, bad in ((cat, lambda: cat.remove(["m4", "nope"])),          # unknown id
                        (cat, lambda: cat.remove(["m4", "m9", "m4"])),      # duplicate id
                        (cat, lambda: cat.remove([4, 9, 4])),               # duplicate row
                        (cat, lambda: cat.remove([4, N])),                  # past the end
                        (cat, lambda: cat.remove([-1, 5])),
                        (cat, lambda: cat.remove(range(N))),                # every row
                        (cat, lambda: cat.remove(ids)),
                        (plain, lambda: plain.remove(["m4"])),              # no ids
                        (parts, lambda: parts.remove([4, 5])),
                        (shard, lambda: shard.remove([4, 5])),
                        (later, lambda: later.remove([504, 505]))):
        before, dev_before = _snapshot(target)
        with pytest.raises(ebt.EbertError):
            bad()
        after, dev_after = _snapshot(target)
        assert after == before
        for x, y in zip(dev_before, dev_after):
            assert torch.equal(_bits(x), _bits(y))
    assert cat.remove([]) == [] and cat.n == N                    # m == 0: nothing happens
    q = gaussian(2, B, d, dt)
    s, r = ebt.score_topk(cat, 10, queries=_t(q, dt, cuda_device), exclude=_excl(N))
    assert_topk(s, r, *R.cosine_topk(q, c, 10, _excl(N)))


# ---- 9. bare ctypes, the way a non-Python caller binds the library ------------------------------
VP, I32, I64, SZ, F32 = (ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_size_t,
                         ctypes.c_float)
CODE = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2, torch.float64: 3}


class CCatalog(ctypes.Structure):   # struct ebt_catalog
    _fields_ = [("data", VP), ("dtype", I32), ("d", I32), ("n", I64), ("ld", I64),
                ("row_offset", I64), ("gnorm64", VP), ("inv32", VP), ("image", VP),
                ("cscale", VP), ("img_dtype", I32), ("ld_img", I32), ("d_pad", I32),
                ("native", I32), ("u_cat", F32)]


@pytest.fixture(scope="module")
def clib():
    h = ctypes.CDLL(os.path.join(ROOT, "robot_ebert_amd", "libebert.so"))
    PC = ctypes.POINTER(CCatalog)
    PI = ctypes.POINTER(I64)
    h.ebt_last_error.restype = ctypes.c_char_p
    h.ebt_catalog_state_bytes.argtypes = [VP, ctypes.c_int, I64, I32, I64]
    h.ebt_catalog_state_bytes.restype = SZ
    h.ebt_catalog_init_reserved.argtypes = [PC, VP, ctypes.c_int, I64, I64, I32, I64, I64, VP, SZ,
                                            VP]
    h.ebt_catalog_remove_bytes.argtypes = [I64]
    h.ebt_catalog_remove_bytes.restype = SZ
    h.ebt_catalog_remove_plan.argtypes = [I64, I64, PI, I64, PI, PI]
    h.ebt_catalog_remove_plan.restype = I64
    h.ebt_catalog_remove_rows.argtypes = [PC, VP, SZ, I64, PI, I64, VP, SZ, VP]
    return h


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


@pytest.mark.parametrize("dt, d", [("f32", 70), ("f16", 64)])
def test_bare_ctypes_second_stream(cuda_device, clib, dt, d):
    h, dev = clib, cuda_device
    # GLOBAL rows: a shard whose row 0 is row 5000. A capacity whose layout differs from that of
    # n_cap = N (the norms' 256-byte pad moves), so that the wrong capacity below is detected
    off, n_cap = 5000, N + 40
    c = _catalog(1, N, d, dt)
    rows = sorted(_removal(51, N))
    side = torch.cuda.Stream(dev)
    st = side.cuda_stream
    emb = torch.zeros((n_cap, d), dtype=TDT[dt], device=dev)
    emb[:N] = _t(c, dt, dev)
    need = h.ebt_catalog_state_bytes(P(emb), CODE[emb.dtype], n_cap, d, d)
    state = torch.empty(need, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)                  # emb is ready before the side stream reads it
    cat = CCatalog()
    assert h.ebt_catalog_init_reserved(ctypes.byref(cat), P(emb), CODE[emb.dtype], N, n_cap, d, d,
                                       off, P(state), need, st) == 0, h.ebt_last_error()
    side.synchronize()
    emb0, state0 = emb.clone(), state.clone()
    hrows = (I64 * M)(*[r + off for r in rows])
    src, dst = (I64 * M)(), (I64 * M)()
    p = h.ebt_catalog_remove_plan(N, off, hrows, M, src, dst)
    assert p == len(_moves(N, rows))
    assert [(src[i] - off, dst[i] - off) for i in range(p)] == _moves(N, rows)
    ws = torch.empty(h.ebt_catalog_remove_bytes(M), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    # refused calls first: unsorted rows, every row, a short workspace, another capacity
    before = bytes(cat)
    every = (I64 * N)(*range(off, off + N))
    unsorted = (I64 * 2)(off + 5, off + 3)
    assert h.ebt_catalog_remove_rows(ctypes.byref(cat), P(state), need, n_cap, unsorted, 2, P(ws),
                                     ws.numel(), st) == -1
    assert h.ebt_catalog_remove_rows(ctypes.byref(cat), P(state), need, n_cap, every, N, P(ws),
                                     1 << 20, st) == -1
    assert b"every row" in h.ebt_last_error()
    assert h.ebt_catalog_remove_rows(ctypes.byref(cat), P(state), need, n_cap, hrows, M, P(ws),
                                     16 * M - 1, st) == -1
    assert h.ebt_catalog_remove_rows(ctypes.byref(cat), P(state), need, N, hrows, M, P(ws),
                                     ws.numel(), st) == -1
    side.synchronize()
    assert bytes(cat) == before and cat.n == N
    assert torch.equal(state, state0) and torch.equal(_bits(emb), _bits(emb0))
    # the removal, on the side stream
    assert h.ebt_catalog_remove_rows(ctypes.byref(cat), P(state), need, n_cap, hrows, M, P(ws),
                                     ws.numel(), st) == 0, h.ebt_last_error()
    side.synchronize()
    n_new = N - M
    assert cat.n == n_new and cat.row_offset == off
    # exactly the plan's moves: every destination holds its source's row, norm and inverse norm,
    # and every other row below n' is what it was
    frm = torch.tensor([src[i] - off for i in range(p)], device=dev)
    to = torch.tensor([dst[i] - off for i in range(p)], device=dev)
    keep = torch.ones(n_new, dtype=torch.bool, device=dev)
    keep[to] = False
    gn0, gn = state0[:n_cap * 8].view(torch.float64), state[:n_cap * 8].view(torch.float64)
    o = _up(n_cap * 8, 256)
    iv0 = state0[o:o + _up(n_cap, 128) * 4].view(torch.float32)
    iv = state[o:o + _up(n_cap, 128) * 4].view(torch.float32)
    assert torch.equal(_bits(emb[to]), _bits(emb0[frm]))
    assert torch.equal(_bits(emb[:n_new][keep]), _bits(emb0[:n_new][keep]))
    assert torch.equal(_bits(gn[to]), _bits(gn0[frm]))
    assert torch.equal(_bits(gn[:n_new][keep]), _bits(gn0[:n_new][keep]))
    assert torch.equal(_bits(iv[to]), _bits(iv0[frm]))
    assert torch.equal(_bits(iv[:n_new][keep]), _bits(iv0[:n_new][keep]))
    assert bool((iv[n_new:] == 1.0).all())
    # and the whole state is that of the library's own build of the edited matrix
    import robot_ebert_amd as ebt
    fresh = ebt.Catalog(_t(_edited(c, rows), dt, dev))
    assert torch.equal(_bits(emb[:n_new]), _bits(fresh.data))
    assert torch.equal(_bits(gn[:n_new]), _bits(fresh.gnorm))
    assert torch.equal(_bits(iv[:_up(n_new, 128)]), _bits(fresh.inv32))
    if not fresh.native or fresh.image.data_ptr() != fresh.data.data_ptr():
        o2 = o + _up(_up(n_cap, 128) * 4, 256)
        img = state[o2:o2 + n_new * fresh.ld_img * 2].view(fresh.image.dtype).view(
            n_new, fresh.ld_img)
        assert torch.equal(_bits(img), _bits(fresh.image))


# ---- 10. the batcher's barrier on the GPU --------------------------------------------------------
def test_batcher_remove_between_requests(cuda_device):
    import robot_ebert_amd as ebt
    from robot_ebert_amd.batcher import RecBatcher
    dt, d, k = "f32", 70, 10
    c = _catalog(1, N, d, dt)
    rows = _removal(71, N)
    cat = ebt.Catalog(_t(c, dt, cuda_device))
    want = _edited(c, rows)
    n_new = N - M
    rng = np.random.default_rng(72)

    def requests(n, count):
        out = []
        for _ in range(count):
            liked = sorted(int(r) for r in rng.choice(n, 3, replace=False))
            out.append((liked, liked + [int(r) for r in rng.choice(n, 5, replace=False)]))
        return out
    old, new = requests(N, 200), requests(n_new, 200)
    going = sorted({rows[0], N - 1})                              # rows that are about to go
    old[0] = (going, going)
    b = RecBatcher(cat, max_batch=16, max_wait_ms=1.0, max_inflight=2)
    try:
        first = [b.submit(l, e, k) for l, e in old]
        rm = b.remove(rows)
        assert rm.result(timeout=60) == _moves(N, rows)
        assert cat.n == n_new
        assert isinstance(b.submit([n_new], [], k).exception(timeout=5), ValueError)
        last = [b.submit(l, e, k) for l, e in new]
        got = [f.result(timeout=60) for f in first + last]        # raises if a request failed
    finally:
        b.close()
    for lo, mat, part in ((0, c, old), (200, want, new)):
        s_ref, r_ref = R.liked_topk(mat, [l for l, _ in part], k, [e for _, e in part])
        for i, (s, r) in enumerate(got[lo:lo + 200]):
            np.testing.assert_array_equal(r, r_ref[i])
            np.testing.assert_allclose(s, s_ref[i], rtol=0, atol=ATOL)
    assert b.stats()["requests"] == 400
