"""Query prep for liked-movie users (lib.py:52: the mean of the liked rows' cosine rows, folded
into one query per user) at the C3 catalog: B users with L liked rows each, hipEvent-timed,
against the dense-query prep of the same batch.

    python tools/liked_bench.py [--b 4096] [--liked 20] [--iters 20]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import robot_ebert_amd as ebt  # noqa: E402
from robot_ebert_amd import search  # noqa: E402


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def weighted_pair(config, liked_per_user, iters, rounds, baseline_lib=None):
    """ebt_query_liked_sum and ebt_query_liked_wsum (ebert.h 0.8.0) over the same CSR at one
    config's shape, interleaved in one process: `rounds` alternating windows of `iters` calls
    each, hipEvent-timed; one JSON line with each form's median, min and max ms per call and
    the achieved bytes/s at the median (the liked rows read once, the [B][d] float64 sums
    written, the CSR; the weighted call counted at the same bytes plus 8 per liked row).
    baseline_lib: another build of libebert.so (the parent commit's) whose ebt_query_liked_sum
    takes a window in every round too, on the same buffers ("baseline_unweighted")."""
    import ctypes
    from robot_ebert_amd._lib import call, ptr, stream_of
    cfg = bench.CONFIGS[config]
    dev = torch.device("cuda:0")
    emb = bench.make_catalog_shard(cfg, 0, cfg["n"], dev)
    cat = ebt.Catalog(emb)
    B, d = cfg["b"], cfg["d"]
    rng = np.random.default_rng(0)
    liked = [sorted(rng.choice(cfg["n"], liked_per_user, replace=False).tolist())
             for _ in range(B)]
    w = [(rng.uniform(0.5, 5.0, liked_per_user) * rng.choice([-1.0, 1.0], liked_per_user)).tolist()
         for _ in range(B)]
    (off, rows), wt = search.csr_from_weighted_lists(liked, w, dev)
    q64 = torch.empty((B, d), dtype=torch.float64, device=dev)
    st = stream_of(dev)
    head = (ptr(cat.data), cat.dtype_code, d, cat.ld, ptr(cat.gnorm), B, ptr(off), ptr(rows))

    def plain():
        call("ebt_query_liked_sum", *head, ptr(q64), st)

    def weighted():
        call("ebt_query_liked_wsum", *head, ptr(wt), ptr(q64), st)
    ms = {"unweighted": [], "weighted": []}
    base = None
    if baseline_lib:
        fn = ctypes.CDLL(os.path.abspath(baseline_lib)).ebt_query_liked_sum
        vp, i64 = ctypes.c_void_p, ctypes.c_int64
        fn.argtypes = [vp, ctypes.c_int, ctypes.c_int32, i64, vp, i64, vp, vp, vp, vp]

        def base():
            if fn(*head, ptr(q64), st) != 0:
                raise RuntimeError("the baseline library's ebt_query_liked_sum failed")
        ms["baseline_unweighted"] = []
    for _ in range(rounds):
        if base is not None:
            ms["baseline_unweighted"].append(timed(base, iters))
        ms["unweighted"].append(timed(plain, iters))
        ms["weighted"].append(timed(weighted, iters))
    nnz = B * liked_per_user
    nbytes = nnz * d * emb.element_size() + nnz * 16 + B * d * 8 + (B + 1) * 8
    out = {"config": config, "users": B, "liked_per_user": liked_per_user, "d": d,
           "dtype": cfg["dtype"], "iters": iters, "rounds": rounds}
    for name, extra in (("baseline_unweighted", 0), ("unweighted", 0), ("weighted", 8 * nnz)):
        if name not in ms:
            continue
        v = sorted(ms[name])
        med = v[len(v) // 2]
        out[name] = {"ms_median": round(med, 4), "ms_min": round(v[0], 4),
                     "ms_max": round(v[-1], 4), "bytes": nbytes + extra,
                     "GBps_at_median": round((nbytes + extra) / med / 1e6, 1)}
    out["weighted_over_unweighted"] = round(out["weighted"]["ms_median"] /
                                            out["unweighted"]["ms_median"], 4)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3", choices=sorted(bench.CONFIGS))
    ap.add_argument("--b", type=int, default=4096)
    ap.add_argument("--liked", type=int, default=20)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--unaligned", action="store_true",
                    help="catalog rows at stride d + 1 (the element form of ebt_query_liked_sum)")
    ap.add_argument("--weighted", action="store_true",
                    help="the weighted and the unweighted liked-row sums interleaved, at C3's and "
                         "C2's shapes with 50 liked rows per user (one JSON line each)")
    ap.add_argument("--rounds", type=int, default=7, help="--weighted: alternating windows")
    ap.add_argument("--baseline-lib", default=None,
                    help="--weighted: a second libebert.so whose unweighted sum is timed too")
    a = ap.parse_args()
    if a.weighted:
        ebt.load()
        for config in ("C3", "C2"):
            weighted_pair(config, 50, a.iters, a.rounds, a.baseline_lib)
        return
    cfg = bench.CONFIGS[a.config]
    dev = torch.device("cuda:0")
    ebt.load()
    emb = bench.make_catalog_shard(cfg, 0, cfg["n"], dev)
    if a.unaligned:
        wide = torch.empty((cfg["n"], cfg["d"] + 1), dtype=emb.dtype, device=dev)
        wide[:, :cfg["d"]] = emb
        emb = wide[:, :cfg["d"]]
    cat = ebt.Catalog(emb)
    rng = np.random.default_rng(0)
    liked = [sorted(rng.choice(cfg["n"], a.liked, replace=False).tolist()) for _ in range(a.b)]
    lk = search.csr_from_lists(liked, dev)
    q = bench.make_queries(cfg, dev)[:a.b].contiguous()
    ms_liked = timed(lambda: search.prepare_queries(cat, liked=lk), a.iters)
    ms_dense = timed(lambda: search.prepare_queries(cat, queries=q), a.iters)
    rows_read = a.b * a.liked
    print(json.dumps({"config": a.config, "users": a.b, "liked_per_user": a.liked,
                      "form": "element (ld = d + 1)" if a.unaligned else "vector",
                      "liked_prep_ms": round(ms_liked, 4), "dense_prep_ms": round(ms_dense, 4),
                      "liked_rows_GBps": round(rows_read * cfg["d"] * 4 / ms_liked / 1e6, 1)}),
          flush=True)


if __name__ == "__main__":
    main()
