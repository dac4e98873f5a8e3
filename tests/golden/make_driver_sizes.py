"""Record the self-contained path's sizing entries over a grid that hits every conditional region.

    python tests/golden/make_driver_sizes.py

Writes tests/golden/driver_sizes.json: what the BUILT library returns from
ebt_catalog_state_bytes, ebt_workspace_bytes and ebt_sharded_workspace_bytes (host arithmetic: no
GPU, the catalog's device pointers are never read). tests/test_driver_sizes_host.py then holds
every later build to these integers, zeros (refused inputs) included. Regenerate only when a
layout is changed on purpose.
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from robot_ebert_amd import _lib  # noqa: E402

F32, BF16, F16, F64 = _lib.EBT_F32, _lib.EBT_BF16, _lib.EBT_F16, _lib.EBT_F64
FAKE = 1 << 30                      # a 16-byte aligned "device pointer", never dereferenced
NO_FUSE, LIKED_CHECKED, UNKNOWN_FLAG = _lib.EBT_FLAG_NO_FUSE, _lib.EBT_FLAG_LIKED_CHECKED, 64

STATE_COLS = ["data", "dtype", "n", "d", "ld"]
DRIVER_COLS = ["dtype", "n", "B", "k", "kprime", "flags", "chunk_rows"]
SHARDED_COLS = ["case", "dtype", "n_global", "n", "row_offset", "world", "all_reduce", "B", "k",
                "kprime", "flags", "chunk_rows"]


def catalog(dtype, n, row_offset=0):
    """What ebt_catalog_init leaves: f32 rows of d = 100 behind an f16 image of 128 columns; a
    native (16-bit) matrix of d = ld = 64 that is its own image."""
    native = dtype in (F16, BF16)
    d = 64 if native else 100
    d_pad = 64 if native else 128
    return _lib.EbtCatalog(data=FAKE, dtype=dtype, d=d, n=n, ld=d, row_offset=row_offset,
                           gnorm64=FAKE, inv32=FAKE, image=FAKE, cscale=FAKE if native else None,
                           img_dtype=dtype if native else F16, ld_img=d_pad, d_pad=d_pad,
                           native=int(native), u_cat=0.0 if native else 2.0 ** -11)


def options(kprime, flags, chunk_rows):
    if not (kprime or flags or chunk_rows):
        return None
    return ctypes.byref(_lib.EbtOptions(kprime=kprime, flags=flags, chunk_rows=chunk_rows))


def state_bytes(lib, data, dtype, n, d, ld):
    return lib.ebt_catalog_state_bytes(data, dtype, n, d, ld)


def driver_bytes(lib, dtype, n, B, k, kprime, flags, chunk_rows):
    cat = catalog(dtype, n)
    return lib.ebt_workspace_bytes(ctypes.byref(cat), B, k, options(kprime, flags, chunk_rows))


def sharded_bytes(lib, case, dtype, n_global, n, row_offset, world, all_reduce, B, k, kprime,
                  flags, chunk_rows):
    cat = catalog(dtype, n, row_offset)
    gather = _lib.ALLGATHER_FN(lambda *a: 0)
    reduce_ = _lib.ALLREDUCE_F64_FN(lambda *a: 0) if all_reduce else _lib.ALLREDUCE_F64_FN()
    comm = _lib.EbtComm(rank=0, world=world, n_global=n_global, all_gather=gather,
                        all_reduce_f64=reduce_)
    return lib.ebt_sharded_workspace_bytes(ctypes.byref(cat), ctypes.byref(comm), B, k,
                                           options(kprime, flags, chunk_rows))


def state_grid():
    rows = []
    for dtype in (F32, BF16, F16, F64):
        for d, ld in ((64, 64), (64, 65), (100, 100), (1536, 1536)):
            for data in (FAKE, FAKE + 8):
                for n in (1, 127, 128, 129, 5000):
                    rows.append([data, dtype, n, d, ld])
        rows.append([FAKE, dtype, 0, 64, 64])       # n = 0 -> 0
        rows.append([FAKE, dtype, 128, 64, 63])     # ld < d -> 0
    return rows


OPTION_SETS = [(8, 0, 0), (600, 0, 0), (4096, 0, 0), (0, 0, 128), (0, 0, 100), (0, 0, 262144),
               (0, NO_FUSE, 0), (0, LIKED_CHECKED, 0), (0, UNKNOWN_FLAG, 0)]


def driver_grid():
    rows = []
    for dtype in (F16, F32):
        for n in (50, 5000, 1_000_000):
            for B in (1, 128, 129, 300, 4096):
                for k in (1, 100, 512, 4096, 5000):
                    rows.append([dtype, n, B, k, 0, 0, 0])
            for B, k in ((1, 1), (129, 100), (300, 512), (4096, 100), (4096, 5000)):
                for kprime, flags, chunk in OPTION_SETS:
                    rows.append([dtype, n, B, k, kprime, flags, chunk])
    return rows


def sharded_grid():
    """(case, dtype, n_global, shard rows or None = ceil(n_global / world), B, k, options)"""
    cases = [("c3", F32, 1_000_000, None, 4096, 100, (0, 0, 0)),
             ("c3_native", F16, 1_000_000, None, 4096, 100, (0, 0, 0)),
             ("ten_million", BF16, 10_000_000, None, 4096, 100, (0, 0, 0)),
             ("short_shard", F32, 1_000_000, 1000, 4096, 100, (0, 0, 0)),
             ("padded", F32, 1_000_000, 50, 300, 100, (0, 0, 0)),
             ("small_batch", F32, 2_000_000, None, 129, 10, (0, 0, 0)),
             ("wide_k", F32, 1_000_000, None, 16, 2000, (0, 0, 0)),
             ("no_fuse", F32, 1_000_000, None, 4096, 100, (0, NO_FUSE, 0)),
             ("kprime_600", F32, 1_000_000, None, 4096, 100, (600, 0, 0)),
             ("chunk_128", F32, 1_000_000, None, 4096, 100, (0, 0, 128)),
             ("k_4097", F32, 1_000_000, None, 4096, 4097, (0, 0, 0)),
             ("k_4096", F32, 1_000_000, None, 16, 4096, (0, 0, 0))]
    rows = []
    for name, dtype, n_global, n, B, k, opt in cases:
        for world in (1, 2, 8):
            for all_reduce in (1, 0):
                shard = n if n is not None else -(-n_global // world)
                rows.append([name, dtype, n_global, shard, 0, world, all_reduce, B, k, *opt])
    # a shard that is not the first: n_global must cover row_offset + n
    rows.append(["offset_ok", F32, 1_000_000, 125_000, 875_000, 8, 1, 4096, 100, 0, 0, 0])
    rows.append(["offset_past_end", F32, 1_000_000, 125_000, 875_001, 8, 1, 4096, 100, 0, 0, 0])
    return rows


PARTS = (("state", STATE_COLS, state_grid, state_bytes),
         ("driver", DRIVER_COLS, driver_grid, driver_bytes),
         ("sharded", SHARDED_COLS, sharded_grid, sharded_bytes))


def main():
    lib = _lib.load()
    out = {}
    for name, cols, grid, fn in PARTS:
        out[name] = {"columns": cols + ["bytes"],
                     "rows": [row + [int(fn(lib, *row))] for row in grid()]}
    path = os.path.join(HERE, "driver_sizes.json")
    with open(path, "w") as f:
        for i, (name, _, _, _) in enumerate(PARTS):
            f.write('%s "%s": {"columns": %s, "rows": [\n  '
                    % (",\n" if i else "{\n", name, json.dumps(out[name]["columns"])))
            f.write(",\n  ".join(json.dumps(r) for r in out[name]["rows"]))
            f.write("\n ]}")
        f.write("\n}\n")
    print("wrote", path, {name: len(out[name]["rows"]) for name, _, _, _ in PARTS})


if __name__ == "__main__":
    main()
