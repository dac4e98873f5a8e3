"""CPU: materialised sub-catalogs (ebert.h 0.7.0) -- the new symbols, the sizing functions and the
host-side argument checks of every new entry (they run before any GPU call, so the fake device
pointers are never dereferenced)."""
import ctypes

import pytest

import robot_ebert_amd
from robot_ebert_amd import _lib

EINVAL = -1
FAKE = 1 << 30          # "device" addresses, 256-byte aligned, never dereferenced
STATE = 1 << 32
NEW = ("ebt_allow_count", "ebt_allow_rows_bytes", "ebt_allow_rows", "ebt_catalog_gather_rows",
       "ebt_sub_exclusions_bytes", "ebt_sub_exclusions", "ebt_sub_rows_to_global")


def _al(v):
    return (v + 255) // 256 * 256


def _fake_catalog(n=1000, d=72, native=False):
    """A hand-filled ebt_catalog: f32 with an image of its own, or bf16 whose matrix is its image."""
    d_pad = (d + 63) // 64 * 64
    inv = STATE + _al(n * 8)
    img = inv + _al((n + 127) // 128 * 128 * 4)
    if native:
        return _lib.EbtCatalog(data=FAKE, dtype=_lib.EBT_BF16, d=d, n=n, ld=d, row_offset=0,
                               gnorm64=STATE, inv32=inv, image=FAKE, cscale=inv,
                               img_dtype=_lib.EBT_BF16, ld_img=d, d_pad=d_pad, native=1, u_cat=0.0)
    return _lib.EbtCatalog(data=FAKE, dtype=_lib.EBT_F32, d=d, n=n, ld=d, row_offset=0,
                           gnorm64=STATE, inv32=inv, image=img, cscale=None,
                           img_dtype=_lib.EBT_F16, ld_img=d_pad, d_pad=d_pad, native=0,
                           u_cat=2.0 ** -11)


def _err(lib):
    return lib.ebt_last_error().decode()


def test_symbols_and_version():
    lib = _lib.load()
    for s in NEW:
        assert hasattr(lib, s), s
        assert s in _lib._SIGNATURES, s
    assert lib.ebt_version() >= 700
    for name in ("materialize", "dematerialize", "materialized"):
        assert hasattr(robot_ebert_amd.AllowMasks, name), name


def test_bytes_functions():
    lib = _lib.load()
    for bad in (0, -4, 3, 6, 1 << 40):
        assert lib.ebt_allow_rows_bytes(bad) == 0, bad
    prev = 0
    for words in (4, 8, 256, 260, 1024, 31252, 1 << 20):
        b = lib.ebt_allow_rows_bytes(words)
        assert b >= 4 * ((words + 255) // 256) and b >= prev, words     # one u32 per workgroup
        prev = b
    for B, nnz in ((0, 10), (-1, 10), (5, -1), (1 << 40, 10), (5, 1 << 40)):
        assert lib.ebt_sub_exclusions_bytes(B, nnz) == 0, (B, nnz)
    prev = 0
    for B in (1, 5, 64, 65, 4096, 100000):
        for nnz in (0, 1, 10 ** 6):
            b = lib.ebt_sub_exclusions_bytes(B, nnz)
            assert b >= 4 * B and b >= prev, (B, nnz)                  # one u32 count per query
            prev = b


# (words, n_rows): words not a positive multiple of 4, n_rows outside the mask row
BAD_ROW = [(0, 0), (-4, 0), (6, 10), (30, 10), (4, 129), (32, 1025), (4, -1)]


@pytest.mark.parametrize("words, n_rows", BAD_ROW)
def test_mask_row_checks(words, n_rows):
    lib = _lib.load()
    M, R, K, C, W = FAKE, FAKE + (1 << 20), FAKE + (2 << 20), FAKE + (3 << 20), FAKE + (4 << 20)
    assert lib.ebt_allow_count(M, words, n_rows, C, None) == EINVAL
    assert _err(lib)
    assert lib.ebt_allow_rows(M, words, n_rows, R, 100, K, C, W, 1 << 20, None) == EINVAL
    assert _err(lib)
    assert lib.ebt_sub_exclusions(M, words, K, n_rows, R, R + 4096, 5, 10, C, C + 4096, W,
                                  1 << 20, None) == EINVAL
    assert _err(lib)


def test_allow_count_and_rows_reject_null_and_workspace():
    lib = _lib.load()
    M, R, K, C, W = FAKE, FAKE + (1 << 20), FAKE + (2 << 20), FAKE + (3 << 20), FAKE + (4 << 20)
    for args in ((None, 32, 1000, C), (M, 32, 1000, None)):
        assert lib.ebt_allow_count(*args, None) == EINVAL and "null" in _err(lib)
    need = lib.ebt_allow_rows_bytes(32)
    good = [M, 32, 1000, R, 100, K, C, W, need]
    for i in (0, 3, 5, 6, 7):                       # mask_row, rows_out, rank_out, count_out, ws
        a = list(good)
        a[i] = None
        assert lib.ebt_allow_rows(*a, None) == EINVAL and "null" in _err(lib), i
    a = list(good)
    a[4] = -1                                       # cap < 0
    assert lib.ebt_allow_rows(*a, None) == EINVAL
    a = list(good)
    a[8] = need - 1                                 # workspace too small
    assert lib.ebt_allow_rows(*a, None) == EINVAL and "workspace" in _err(lib)


def _gather(lib, cat, rows=FAKE + (5 << 20), m=10, data_out=FAKE + (6 << 20), ld_out=None,
            gnorm_out=FAKE + (7 << 20), inv32_out=FAKE + (8 << 20), image_out=FAKE + (9 << 20),
            sub=True, parent=True):
    out = _lib.EbtCatalog()
    ld_out = cat.d if ld_out is None else ld_out
    return lib.ebt_catalog_gather_rows(ctypes.byref(cat) if parent else None, rows, m, data_out,
                                       ld_out, gnorm_out, inv32_out, image_out,
                                       ctypes.byref(out) if sub else None, None)


def test_gather_rows_rejects_bad_arguments():
    lib = _lib.load()
    cat = _fake_catalog()
    for kw in (dict(parent=False), dict(rows=None), dict(data_out=None), dict(gnorm_out=None),
               dict(inv32_out=None), dict(sub=False)):
        assert _gather(lib, cat, **kw) == EINVAL and "null" in _err(lib), kw
    for m in (0, -3):
        assert _gather(lib, cat, m=m) == EINVAL and "m=" in _err(lib)
    assert _gather(lib, cat, ld_out=cat.d - 1) == EINVAL and "ld_out" in _err(lib)
    # a parent with an image of its own needs room for the image rows
    assert _gather(lib, cat, image_out=None) == EINVAL and "image_out" in _err(lib)
    # a parent whose matrix is its own image: the copy is one too, so ld_out % 64 == 0
    nat = _fake_catalog(d=128, native=True)
    assert _gather(lib, nat, ld_out=130, image_out=None) == EINVAL and "64" in _err(lib)
    assert _gather(lib, nat, ld_out=127, image_out=None) == EINVAL


def test_sub_exclusions_and_rows_to_global_reject_bad_arguments():
    lib = _lib.load()
    M, K, O, R, OO, RO, W = (FAKE + (i << 20) for i in range(7))
    need = lib.ebt_sub_exclusions_bytes(5, 10)
    good = [M, 32, K, 1000, O, R, 5, 10, OO, RO, W, need]
    for i in (0, 2, 4, 5, 8, 9, 10):
        a = list(good)
        a[i] = None
        assert lib.ebt_sub_exclusions(*a, None) == EINVAL and "null" in _err(lib), i
    for i, v in ((6, 0), (7, -1), (11, need - 1)):  # B < 1, nnz < 0, workspace too small
        a = list(good)
        a[i] = v
        assert lib.ebt_sub_exclusions(*a, None) == EINVAL, (i, v)
        assert _err(lib)
    assert lib.ebt_sub_rows_to_global(None, 5, R, 10, None) == EINVAL
    assert lib.ebt_sub_rows_to_global(O, 5, None, 10, None) == EINVAL
    assert lib.ebt_sub_rows_to_global(O, -1, R, 10, None) == EINVAL
    assert lib.ebt_sub_rows_to_global(O, 5, R, -1, None) == EINVAL
    assert lib.ebt_sub_rows_to_global(None, 0, None, 0, None) == 0     # nothing to do
