"""GPU: live catalog updates (Catalog.update_rows / append, ebt_catalog_update_rows /
ebt_catalog_append_rows, RecBatcher.update_rows, distributed.split_update).

The state after an update must be BITWISE the state of a catalog built afresh from the edited
matrix (data, guarded float64 norms, float32 inverse norms, image), u_cat a running maximum, and
every result must equal the float64 oracle on the host matrix with the same edits applied."""
import ctypes
import os
import threading

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


def _edit(seed, n, d, dt, zero_row=5):
    """The catalog (row `zero_row` all zeros), M distinct rows in no order -- row 0, row n-1, the
    formerly-zero row (set non-zero) and one row set to zeros among them -- and their vectors."""
    c = gaussian(1, n, d, dt)
    c[zero_row] = 0.0
    rng = np.random.default_rng(seed)
    rest = [int(r) for r in rng.permutation(np.arange(1, n - 1)) if r not in (zero_row, 17)]
    rows = [n - 1, 17, 0, zero_row] + rest[:M - 4]
    order = rng.permutation(M)
    rows = [rows[i] for i in order]
    v = gaussian(seed + 1, M, d, dt)
    v[rows.index(17)] = 0.0
    return c, rows, v


def assert_state_equal(cat, fresh):
    n = fresh.n
    assert cat.n == n and cat.ld_img == fresh.ld_img and cat.native == fresh.native
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


# ---- 1. the state equals a fresh build ---------------------------------------------------------
# d = 64: the 16-bit catalogs' matrix is their image; 70: ragged (element-form norms for f32, a
# separate raw image for 16-bit); 1536; 2048: the last d the kernel stages in LDS; 2100 / 2112: past it
@pytest.mark.parametrize("dt, d", [(dt, d) for d in (64, 70, 1536)
                                   for dt in ("f32", "f64", "f16", "bf16")] +
                         [("f32", 2048), ("f32", 2100), ("f64", 2100), ("f16", 2112)])
def test_state_equals_fresh_build(cuda_device, dt, d):
    import robot_ebert_amd as ebt
    c, rows, v = _edit(11, N, d, dt)
    cat = ebt.Catalog(_t(c, dt, cuda_device))
    cat.update_rows(rows, _t(v, dt, cuda_device))
    c[rows] = v
    assert_state_equal(cat, ebt.Catalog(_t(c, dt, cuda_device)))


# ld > d: a column slice of a wider tensor. f32 70 / 96: aligned rows, element-form norms;
# f64 70 / 75: unaligned rows; bf16 64 / 128: the slice itself is the image; f16 64 / 72: it is not
@pytest.mark.parametrize("dt, d, ld", [("f32", 70, 96), ("f64", 70, 75), ("bf16", 64, 128),
                                       ("f16", 64, 72)])
def test_state_equals_fresh_build_strided(cuda_device, dt, d, ld):
    import robot_ebert_amd as ebt
    c, rows, v = _edit(13, N, ld, dt)
    wide = _t(c, dt, cuda_device)
    cat = ebt.Catalog(wide[:, :d])
    assert cat.ld == ld
    cat.update_rows(rows, _t(v, dt, cuda_device)[:, :d])          # a strided source as well
    want = c.copy()
    want[rows, :d] = v[:, :d]
    assert torch.equal(_bits(wide), _bits(_t(want, dt, cuda_device))), "columns past d touched"
    assert_state_equal(cat, ebt.Catalog(_t(want, dt, cuda_device)[:, :d]))


# ---- 2. source conversion ----------------------------------------------------------------------
def _rounding_values(bits, rng, count):
    """float64 values that need rounding to a format of `bits` significand bits: exact ties (to
    even and to odd), just above / below a tie (by one float64 ulp and by less than a float32
    ulp: the latter is a tie only after a first rounding to float), and ordinary values."""
    ulp = 2.0 ** -(bits - 1)
    j = np.arange(count // 4)
    tie = 1.0 + (j + 0.5) * ulp
    v = np.concatenate([tie, -tie, tie + 2.0 ** -52, tie - 2.0 ** -52, tie + 2.0 ** -30,
                        tie - 2.0 ** -30, rng.standard_normal(count) * 3.0])
    return v


@pytest.mark.parametrize("src, dst", [("f64", "f32"), ("f64", "f16"), ("f64", "bf16"),
                                      ("f32", "f16"), ("f32", "bf16"), ("f16", "bf16"),
                                      ("bf16", "f64")])
def test_source_conversion_is_torch_to(cuda_device, src, dst):
    import robot_ebert_amd as ebt
    n, d, m = 200, 70, 16
    rng = np.random.default_rng(21)
    sig = {"f32": 24, "f16": 11, "bf16": 8, "f64": 53}[dst]
    vals = _rounding_values(sig, rng, 160)
    extra = np.array([0.0, -0.0, 65504.0, 65520.0, 70000.0, -1e6, 6e-8, 2.9e-8, 3.1e-8, 1e-40,
                      -1e-41, 3.3e38, np.inf, -np.inf, 0.1, 1.0 / 3.0])
    flat = np.resize(np.concatenate([vals, extra]), m * d)
    host = torch.from_numpy(flat.reshape(m, d)).to(TDT[src])      # the source as its own dtype
    source = host.to(cuda_device)
    cat = ebt.Catalog(_t(gaussian(1, n, d, dst), dst, cuda_device))
    rows = [int(r) for r in rng.choice(n, m, replace=False)]
    cat.update_rows(rows, source)
    want = source.to(TDT[dst])
    got = cat.data[torch.tensor(rows, device=cuda_device)]
    assert torch.equal(_bits(got), _bits(want))
    # a numpy source takes the same path
    if src in ("f64", "f32"):
        cat.update_rows(rows[::-1], host.numpy()[::-1])
        assert torch.equal(_bits(cat.data[torch.tensor(rows, device=cuda_device)]), _bits(want))


# ---- 3. results ---------------------------------------------------------------------------------
def _planted(c, q, excl):
    """Edits with known consequences: A, query 3's top-1, overwritten with its negation; Bq, a row
    query 5 may be recommended, overwritten with query 5's own vector."""
    _, r0 = R.cosine_topk(q, c, 10, excl)
    A = int(r0[3, 0])
    Bq = next(r for r in range(500, N) if r != A and r not in excl[5])
    return A, Bq


def _results_case(dt, d):
    c, rows, v = _edit(31, N, d, dt)
    q = gaussian(2, B, d, dt)
    excl = _excl(N)
    A, Bq = _planted(c, q, excl)
    keep = [i for i, r in enumerate(rows) if r not in (A, Bq)]
    rows = [rows[i] for i in keep] + [A, Bq]
    v = np.concatenate([v[keep], -c[A][None, :], q[5][None, :]])
    edited = c.copy()
    edited[rows] = v
    return c, q, excl, rows, v, edited, A, Bq


def _check_planted(r10, A, Bq):
    assert r10[5, 0] == Bq, "the row overwritten with query 5's vector is its top-1"
    assert A not in r10[3], "the negated former top-1 still appears"


@pytest.mark.parametrize("dt, d", [("f32", 70), ("bf16", 64), ("f64", 1536)])
def test_results_after_update(cuda_device, dt, d):
    import robot_ebert_amd as ebt
    c, q, excl, rows, v, edited, A, Bq = _results_case(dt, d)
    cat = ebt.Catalog(_t(c, dt, cuda_device))
    qt = _t(q, dt, cuda_device)
    s, r = ebt.score_topk(cat, 10, queries=qt, exclude=excl)
    assert_topk(s, r, *R.cosine_topk(q, c, 10, excl))
    assert int(r[3, 0]) == A
    cat.update_rows(rows, _t(v, dt, cuda_device))
    for k in (10, 100):
        s, r = ebt.score_topk(cat, k, queries=qt, exclude=excl)
        assert_topk(s, r, *R.cosine_topk(q, edited, k, excl))
        if k == 10:
            _check_planted(r.cpu().numpy(), A, Bq)
    # liked rows that are themselves updated rows (A, Bq) and untouched ones
    liked = [sorted({A, 7}), [Bq], sorted({rows[0], rows[1], 21}), [3, 4]]
    rated = [sorted(set(l + [8, 9])) for l in liked]
    for k in (10, 100):
        s, r = ebt.score_topk(cat, k, liked=liked, exclude=rated)
        assert_topk(s, r, *R.liked_topk(edited, liked, k, rated))


# bare ctypes, the way a non-Python caller binds the library (no robot_ebert_amd import)
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
    h.ebt_last_error.restype = ctypes.c_char_p
    h.ebt_catalog_state_bytes.argtypes = [VP, ctypes.c_int, I64, I32, I64]
    h.ebt_catalog_state_bytes.restype = SZ
    h.ebt_catalog_init.argtypes = [PC, VP, ctypes.c_int, I64, I32, I64, I64, VP, SZ, VP]
    h.ebt_catalog_init_reserved.argtypes = [PC, VP, ctypes.c_int, I64, I64, I32, I64, I64, VP, SZ,
                                            VP]
    h.ebt_catalog_update_bytes.argtypes = [I64]
    h.ebt_catalog_update_bytes.restype = SZ
    h.ebt_catalog_update_rows.argtypes = [PC, VP, SZ, I64, ctypes.POINTER(I64), I64, VP,
                                          ctypes.c_int, I64, VP, SZ, VP]
    h.ebt_catalog_append_rows.argtypes = [PC, VP, SZ, I64, I64, VP, ctypes.c_int, I64, VP]
    h.ebt_workspace_bytes.argtypes = [PC, I64, I32, VP]
    h.ebt_workspace_bytes.restype = SZ
    h.ebt_cosine_topk.argtypes = [PC, VP, ctypes.c_int, I64, I64, VP, VP, I32, VP, VP, VP, VP, SZ,
                                  VP, VP, VP, VP]
    return h


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _csr(lists, dev):
    off = np.zeros(len(lists) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(x) for x in lists])
    flat = np.concatenate([np.sort(np.asarray(x, dtype=np.int64)) for x in lists])
    return torch.from_numpy(off).to(dev), torch.from_numpy(flat).to(dev)


def _c_topk(h, cat, k, dev, qt, excl):
    ws_bytes = h.ebt_workspace_bytes(ctypes.byref(cat), B, k, None)
    assert ws_bytes > 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    s = torch.empty((B, k), dtype=torch.float64, device=dev)
    r = torch.empty((B, k), dtype=torch.int64, device=dev)
    eo, er = _csr(excl, dev)
    rc = h.ebt_cosine_topk(ctypes.byref(cat), P(qt), CODE[qt.dtype], B, qt.stride(0), None, None,
                           k, P(eo), P(er), None, P(ws), ws_bytes, P(s), P(r), None,
                           torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, h.ebt_last_error()
    return s.cpu().numpy(), r.cpu().numpy()


def test_results_after_update_bare_ctypes(cuda_device, clib):
    h, dev, dt, d = clib, cuda_device, "f32", 70
    c, q, excl, rows, v, edited, A, Bq = _results_case(dt, d)
    st = torch.cuda.current_stream(dev).cuda_stream
    n_cap = N + 8
    emb = torch.zeros((n_cap, d), dtype=TDT[dt], device=dev)
    emb[:N] = _t(c, dt, dev)
    need = h.ebt_catalog_state_bytes(P(emb), CODE[emb.dtype], n_cap, d, d)
    state = torch.empty(need, dtype=torch.uint8, device=dev)
    cat = CCatalog()
    assert h.ebt_catalog_init_reserved(ctypes.byref(cat), P(emb), CODE[emb.dtype], N, n_cap, d, d,
                                       0, P(state), need, st) == 0, h.ebt_last_error()
    qt = _t(q, dt, dev)
    assert_topk(*_c_topk(h, cat, 10, dev, qt, excl), *R.cosine_topk(q, c, 10, excl))
    # the update: ascending rows on the host, a float64 source converted by the kernel
    order = np.argsort(rows)
    hrows = (I64 * len(rows))(*[rows[i] for i in order])
    src = torch.from_numpy(np.ascontiguousarray(v[order])).to(dev)
    ws = torch.empty(h.ebt_catalog_update_bytes(len(rows)), dtype=torch.uint8, device=dev)
    u0 = cat.u_cat
    assert h.ebt_catalog_update_rows(ctypes.byref(cat), P(state), need, n_cap, hrows, len(rows),
                                     P(src), CODE[src.dtype], d, P(ws), ws.numel(), st) == 0, \
        h.ebt_last_error()
    assert u0 <= cat.u_cat <= 2.0 ** -11 and cat.n == N
    for k in (10, 100):
        s, r = _c_topk(h, cat, k, dev, qt, excl)
        assert_topk(s, r, *R.cosine_topk(q, edited, k, excl))
        if k == 10:
            _check_planted(r, A, Bq)
    # append through the C entry: 8 rows, the first of them query 9's vector
    more = gaussian(41, 8, d, dt)
    more[0] = q[9]
    assert h.ebt_catalog_append_rows(ctypes.byref(cat), P(state), need, n_cap, 8,
                                     P(_t(more, dt, dev)), CODE[TDT[dt]], d, st) == 0, \
        h.ebt_last_error()
    assert cat.n == N + 8
    grown = np.concatenate([edited, more])
    s, r = _c_topk(h, cat, 10, dev, qt, excl)
    assert_topk(s, r, *R.cosine_topk(q, grown, 10, excl))
    assert r[9, 0] == N
    # a refused call changes nothing: unsorted rows, then one row too many
    before = bytes(cat)
    bad = (I64 * 2)(5, 3)
    assert h.ebt_catalog_update_rows(ctypes.byref(cat), P(state), need, n_cap, bad, 2, P(src),
                                     CODE[src.dtype], d, P(ws), ws.numel(), st) == -1
    assert h.ebt_catalog_append_rows(ctypes.byref(cat), P(state), need, n_cap, 1, P(src),
                                     CODE[src.dtype], d, st) == -1
    assert bytes(cat) == before
    assert_topk(*_c_topk(h, cat, 10, dev, qt, excl), *R.cosine_topk(q, grown, 10, excl))


# ---- 4. append ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dt, d", [("f32", 70), ("bf16", 64), ("f16", 70), ("f64", 64)])
def test_append_grows_in_place(cuda_device, dt, d):
    import robot_ebert_amd as ebt
    cap = 1400
    c = gaussian(1, cap, d, dt)
    q = gaussian(2, B, d, dt)
    c[1010] = q[2]          # in the first append
    c[1290] = q[6]          # in the second
    c[1020] = 0.0
    ids = [f"m{i}" for i in range(cap)]
    full = _t(c, dt, cuda_device)
    qt = _t(q, dt, cuda_device)
    cat = ebt.Catalog(full[:N], ids=ids[:N], capacity=cap)
    assert cat.n == N and cat.capacity == cap
    assert_state_equal(cat, ebt.Catalog(full[:N]))               # construction with room
    n = N
    for m in (30, 270):     # the second crosses the 128-row pad (1152) and the 256-row tile (1280)
        cat.append(full[n:n + m], ids=ids[n:n + m])
        n += m
        assert cat.n == n == cat.n_global == cat.cstruct.n and len(cat.ids) == n
        assert_state_equal(cat, ebt.Catalog(full[:n].clone()))
        assert bool((cat.inv32[n:] == 1.0).all())
        excl = _excl(n)
        for k in (10, 100):
            s, r = ebt.score_topk(cat, k, queries=qt, exclude=excl)
            assert_topk(s, r, *R.cosine_topk(q, c[:n], k, excl))
        assert int(r[2, 0]) == 1010
        assert cat.rows_of([ids[n - 1], ids[0]]) == [n - 1, 0] and cat.id_of(n - 1) == ids[n - 1]
    assert int(r[6, 0]) == 1290
    for bad in (lambda: cat.append(full[:101], ids=[f"x{i}" for i in range(101)]),   # past capacity
                lambda: cat.append(full[:1], ids=["m3"]),                            # id present
                lambda: cat.append(full[:1])):                                       # ids missing
        with pytest.raises(ebt.EbertError):
            bad()
    assert cat.n == n and len(cat.ids) == n
    s, r = ebt.score_topk(cat, 10, queries=qt, exclude=excl)
    assert_topk(s, r, *R.cosine_topk(q, c[:n], 10, excl))
    # replace an appended row, then fill the capacity exactly
    cat.update_rows(["m1290"], -full[1290:1291])
    cat.append(full[n:cap], ids=ids[n:cap])
    c[1290] = -c[1290]
    assert_state_equal(cat, ebt.Catalog(_t(c, dt, cuda_device)))
    s, r = ebt.score_topk(cat, 10, queries=qt, exclude=_excl(cap))
    assert_topk(s, r, *R.cosine_topk(q, c, 10, _excl(cap)))


# ---- 5. errors leave the catalog usable ---------------------------------------------------------
def test_errors_leave_the_catalog_usable(cuda_device):
    import robot_ebert_amd as ebt
    dt, d = "f32", 70
    c = gaussian(1, N, d, dt)
    q = gaussian(2, B, d, dt)
    excl = _excl(N)
    want = R.cosine_topk(q, c, 10, excl)
    qt = _t(q, dt, cuda_device)
    cat = ebt.Catalog(_t(c, dt, cuda_device), capacity=N + 10)
    v = _t(gaussian(5, 3, d, dt), dt, cuda_device)
    parts = ebt.Catalog.from_parts(cat.data, cat.gnorm, cat.inv32, cat.image)
    shard = ebt.Catalog(_t(c[:500], dt, cuda_device), row_offset=0, n_global=N, capacity=600)
    later = ebt.Catalog(_t(c[500:], dt, cuda_device), row_offset=500, n_global=N, capacity=600)
    for target, bad in ((cat, lambda: cat.update_rows([4, 9, 4], v)),                 # duplicate
                        (cat, lambda: cat.update_rows([4, N, 9], v)),                 # past the end
                        (cat, lambda: cat.update_rows([-1, 5, 9], v)),
                        (cat, lambda: cat.update_rows([4, 5, 9], v[:, :d - 1])),      # wrong d
                        (cat, lambda: cat.update_rows([4, 5], v)),                    # 3 vectors
                        (cat, lambda: cat.update_rows([4, 5, 9], v.to(torch.int32))),
                        (cat, lambda: cat.update_rows(["a", "b", "c"], v)),           # no ids
                        (cat, lambda: cat.append(_t(c[:11], dt, cuda_device))),       # capacity
                        (parts, lambda: parts.update_rows([4, 5, 9], v)),
                        (parts, lambda: parts.append(v)),
                        (later, lambda: later.update_rows([4, 5, 9], v)),             # not its rows
                        (shard, lambda: shard.append(v)),
                        (later, lambda: later.append(v))):
        with pytest.raises(ebt.EbertError):
            bad()
        if target is shard or target is later:
            lo = target.row_offset
            own = [[r for r in x if lo <= r < lo + 500] for x in excl]   # global ids it holds
            s_ref, r_ref = R.cosine_topk(q, c[lo:lo + 500], 10,
                                         [[r - lo for r in x] for x in own])
            s, r = ebt.score_topk(target, 10, queries=qt, exclude=own)
            assert_topk(s, r, s_ref, np.where(r_ref >= 0, r_ref + lo, r_ref))
        else:
            assert_topk(*ebt.score_topk(target, 10, queries=qt, exclude=excl), *want)
    assert cat.n == N and shard.n == 500
    cat.update_rows([], v[:0])                                    # m == 0: nothing happens
    assert_topk(*ebt.score_topk(cat, 10, queries=qt, exclude=excl), *want)


# ---- 6. row-sharded: one global update handed to every rank -------------------------------------
def test_row_sharded_update(cuda_device):
    import robot_ebert_amd as ebt
    from robot_ebert_amd.distributed import score_topk_sharded, shard_range, split_update
    from test_gpu_sharded import ThreadCollectives
    dt, d, world, k = "f32", 128, 2, 10
    c, rows, v = _edit(61, N, d, dt)
    q = gaussian(2, B, d, dt)
    excl = _excl(N)
    full, qt, vt = _t(c, dt, cuda_device), _t(q, dt, cuda_device), _t(v, dt, cuda_device)
    cats = []
    for r in range(world):
        a, b = shard_range(N, r, world)
        cats.append(ebt.Catalog(full[a:b].clone(), row_offset=a, n_global=N))
    counts = []
    for cat in cats:
        sr, sv = split_update(rows, vt, cat)
        counts.append(len(sr))
        cat.update_rows(sr, sv)
    assert sum(counts) == M and min(counts) > 0                   # rows of both shards
    c[rows] = v
    shared = {"world": world, "slots": [None] * world, "barrier": threading.Barrier(world)}
    out, errs = [None] * world, []

    def body(r):
        try:
            torch.cuda.set_device(cuda_device)
            out[r] = score_topk_sharded(cats[r], k, queries=qt, exclude=excl,
                                        collectives=ThreadCollectives(r, shared))
        except BaseException as e:  # noqa: BLE001
            errs.append(e)
            shared["barrier"].abort()
    ts = [threading.Thread(target=body, args=(r,)) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(120)
    if errs:
        raise errs[0]
    s_ref, r_ref = R.cosine_topk(q, c, k, excl)
    for s, r in out:
        assert_topk(s, r, s_ref, r_ref)


# ---- 7. the batcher's barrier on the GPU --------------------------------------------------------
def test_batcher_update_between_requests(cuda_device):
    import robot_ebert_amd as ebt
    from robot_ebert_amd.batcher import RecBatcher
    dt, d, k = "f32", 70, 10
    c, rows, v = _edit(71, N, d, dt)
    cat = ebt.Catalog(_t(c, dt, cuda_device))
    rng = np.random.default_rng(72)
    reqs = []
    for i in range(400):
        liked = [int(r) for r in rng.choice(N, 3, replace=False)]
        if i % 4 == 0:
            liked[0] = rows[i % M]                                # a liked row that is replaced
            liked = sorted(set(liked))
        reqs.append((liked, liked + [int(r) for r in rng.choice(N, 5, replace=False)]))
    b = RecBatcher(cat, max_batch=16, max_wait_ms=1.0, max_inflight=2)
    try:
        first = [b.submit(l, e, k) for l, e in reqs[:200]]
        up = b.update_rows(rows, _t(v, dt, cuda_device))
        assert up.result(timeout=60) is None
        last = [b.submit(l, e, k) for l, e in reqs[200:]]
        got = [f.result(timeout=60) for f in first + last]        # raises if a request failed
    finally:
        b.close()
    edited = c.copy()
    edited[rows] = v
    for lo, mat in ((0, c), (200, edited)):
        part = reqs[lo:lo + 200]
        s_ref, r_ref = R.liked_topk(mat, [l for l, _ in part], k, [e for _, e in part])
        for i, (s, r) in enumerate(got[lo:lo + 200]):
            np.testing.assert_array_equal(r, r_ref[i])
            np.testing.assert_allclose(s, s_ref[i], rtol=0, atol=ATOL)
    assert b.stats()["requests"] == 400
