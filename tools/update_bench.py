"""Live catalog updates against a rebuild (ebt_catalog_update_rows, catalog_update.hip): at C3's
shape (1M x 1536 f32) and C2's (100K x 768 bf16), for m in {1, 64, 4096} replaced rows,

  * us per ``Catalog.update_rows`` call (host clock around calls that end in a device
    synchronise; the Python wrapper's sorting and argument checks included),
  * us per bare ``ebt_catalog_update_rows`` call on prepared arguments (the C entry: row-list
    copy, ONE kernel, and for a non-native catalog the error slot's read-back),
  * us per full ``Catalog(emb)`` rebuild, the only way to change a row before 0.4.0, in the same
    process on the same matrix,
  * the update's achieved bytes/s over the C call: m x (source row + stored row + image row)
    bytes, and its share of the 8 TB/s HBM figure of MI355X_MICROARCH.md.

    bash tools/gpu.sh py OUT tools/update_bench.py [--shapes C3,C2] [--trials 3]

With ``--ops remove`` (default: both) the same for ``Catalog.remove`` / ``ebt_catalog_remove_rows``
(0.5.0, catalog_move_kernel): the m removed rows are drawn below n - m, so every removal causes a
move (p = m). A removal shrinks the catalog, so each timed call is followed by putting n back
(``cstruct.n = n`` on the host; the tail rows are still in place, only their inv32 is 1.0f, which
the next call's moves copy as they would any value). ``Catalog.remove`` also needs its views
refreshed; that restore is timed alone as ``restore_us`` and is included in ``remove_us``. Counted
bytes per move: 2 x (d x elem + separate-image bytes + 12), read plus written.

One JSON line per (shape, op, m). Every timed window is preceded by a warm-up of the same call and
lasts at least --window seconds; the median of --trials windows is reported with their range.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import robot_ebert_amd as ebt  # noqa: E402
from robot_ebert_amd import _lib  # noqa: E402

SHAPES = {"C3": (1_000_000, 1536, torch.float32), "C2": (100_000, 768, torch.bfloat16)}
HBM_BYTES_PER_S = 8e12


def make_matrix(n, d, dtype, dev):
    g = torch.Generator(device=dev).manual_seed(1)
    out = torch.empty((n, d), dtype=dtype, device=dev)
    for a in range(0, n, 65536):      # in blocks: no float32 temporary of the whole matrix
        b = min(n, a + 65536)
        out[a:b] = torch.randn((b - a, d), generator=g, device=dev, dtype=torch.float32).to(dtype)
    return out


def window_us(fn, dev, window, trials):
    """Median (and range) of us per call over `trials` windows of >= `window` seconds each."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(5):
        fn()
    torch.cuda.synchronize(dev)
    est = max((time.perf_counter() - t0) / 5, 1e-6)
    iters = int(min(max(window / est, 10), 20000))
    out = []
    for _ in range(trials):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize(dev)
        out.append((time.perf_counter() - t0) / iters * 1e6)
    return statistics.median(out), min(out), max(out), iters


def remove_op(name, n, d, dtype, cat, m, rebuild, dev, a, lib):
    """One JSON line for removing m rows that all cause a move."""
    es = cat.data.element_size()
    img_row = 0 if cat.image.data_ptr() == cat.data.data_ptr() else cat.ld_img * 2
    rng = np.random.default_rng(3)
    rows = np.sort(rng.choice(n - m, m, replace=False)).astype(np.int64)
    assert lib.ebt_catalog_remove_plan(n, 0, rows.ctypes.data, m, None, None) == m
    row_list = rows.tolist()

    def restore():
        cat.cstruct.n = n
        cat._views()
        cat.n_global = n

    def py_call():
        cat.remove(row_list)
        restore()
    py = window_us(py_call, dev, a.window, a.trials)
    rs = window_us(restore, dev, a.window, a.trials)
    ws = torch.empty(lib.ebt_catalog_remove_bytes(m), dtype=torch.uint8, device=dev)
    args = (ctypes.byref(cat.cstruct), _lib.ptr(cat.state), cat.state.numel(), cat.capacity,
            rows.ctypes.data, m, _lib.ptr(ws), ws.numel(), _lib.stream_of(dev))

    def c_call():
        _lib.call("ebt_catalog_remove_rows", *args)
        cat.cstruct.n = n
    c = window_us(c_call, dev, a.window, a.trials)
    restore()
    nbytes = 2 * m * (d * es + img_row + 12)
    print(json.dumps({
        "shape": name, "op": "remove", "n": n, "d": d, "dtype": str(dtype).split(".")[-1], "m": m,
        "moves": m, "native": cat.native, "remove_us": round(py[0], 2),
        "remove_us_range": [round(py[1], 2), round(py[2], 2)], "restore_us": round(rs[0], 2),
        "c_call_us": round(c[0], 2), "c_call_us_range": [round(c[1], 2), round(c[2], 2)],
        "rebuild_us": round(rebuild[0], 1),
        "rebuild_us_range": [round(rebuild[1], 1), round(rebuild[2], 1)],
        "iters": {"remove": py[3], "c_call": c[3], "rebuild": rebuild[3]},
        "move_bytes": nbytes, "c_call_bytes_per_s": round(nbytes / (c[0] * 1e-6), 1),
        "share_of_8TBps": round(nbytes / (c[0] * 1e-6) / HBM_BYTES_PER_S, 6),
        "trials": a.trials, "window_s": a.window}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="C3,C2")
    ap.add_argument("--ops", default="update,remove")
    ap.add_argument("--m", default="1,64,4096")
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--trials", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = ebt.load()
    for name in a.shapes.split(","):
        n, d, dtype = SHAPES[name]
        emb = make_matrix(n, d, dtype, dev)
        cat = ebt.Catalog(emb)
        es = emb.element_size()
        img_row = 0 if cat.image.data_ptr() == emb.data_ptr() else cat.ld_img * 2
        rebuild = window_us(lambda: ebt.Catalog(emb), dev, a.window, a.trials)
        rng = np.random.default_rng(2)
        ops = a.ops.split(",")
        for m in (int(x) for x in a.m.split(",") if "update" in ops):
            rows = np.sort(rng.choice(n, m, replace=False)).astype(np.int64)
            vec = make_matrix(m, d, dtype, dev)
            row_list = rows.tolist()
            py = window_us(lambda: cat.update_rows(row_list, vec), dev, a.window, a.trials)
            ws = torch.empty(lib.ebt_catalog_update_bytes(m), dtype=torch.uint8, device=dev)
            st = _lib.stream_of(dev)
            args = (ctypes.byref(cat.cstruct), _lib.ptr(cat.state), cat.state.numel(),
                    cat.capacity, rows.ctypes.data, m, _lib.ptr(vec), _lib.DTYPE_CODE[dtype], d,
                    _lib.ptr(ws), ws.numel(), st)
            c = window_us(lambda: _lib.call("ebt_catalog_update_rows", *args), dev, a.window,
                          a.trials)
            nbytes = m * (d * es + d * es + img_row)
            print(json.dumps({
                "shape": name, "op": "update", "n": n, "d": d,
                "dtype": str(dtype).split(".")[-1], "m": m,
                "native": cat.native, "update_rows_us": round(py[0], 2),
                "update_rows_us_range": [round(py[1], 2), round(py[2], 2)],
                "c_call_us": round(c[0], 2), "c_call_us_range": [round(c[1], 2), round(c[2], 2)],
                "rebuild_us": round(rebuild[0], 1),
                "rebuild_us_range": [round(rebuild[1], 1), round(rebuild[2], 1)],
                "iters": {"update_rows": py[3], "c_call": c[3], "rebuild": rebuild[3]},
                "update_bytes": nbytes, "c_call_bytes_per_s": round(nbytes / (c[0] * 1e-6), 1),
                "share_of_8TBps": round(nbytes / (c[0] * 1e-6) / HBM_BYTES_PER_S, 6),
                "trials": a.trials, "window_s": a.window}), flush=True)
        # last: the removals leave inv32 of the tail rows at 1.0f
        for m in (int(x) for x in a.m.split(",") if "remove" in ops):
            remove_op(name, n, d, dtype, cat, m, rebuild, dev, a, lib)
        del cat, emb
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
