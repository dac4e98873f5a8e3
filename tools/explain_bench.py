"""ebt_explain_topk (include/ebert.h 0.9.0) at a C3-like and a C2-like request, against a torch
baseline interleaved in the same process, and beside the score_topk step that produced the rows.

    C3-like: 1M x 1536 f32, B = 4096, k = 100;  C2-like: 100K x 768 bf16, B = 1024, k = 100;
    both with L = 85 liked rows per query (SURVEY section 8d's mean user) and m = 3.

One JSON line per shape: ms per ebt_explain_topk call (median / min / max over the rounds), the
achieved float64 FLOP/s (2 B k L d per call) against the 79 TFLOP/s float64 matrix peak of
SURVEY, the ms of the torch baseline (gather both panels, convert them to float64, torch.bmm,
scale, topk) and the ms of the score_topk call. hipEvent-timed windows of `iters` calls,
`rounds` alternating windows of each.

    python tools/explain_bench.py [--shapes C3,C2] [--iters 5] [--rounds 3] [--liked 85] [--m 3]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import robot_ebert_amd as ebt  # noqa: E402
from robot_ebert_amd import _lib, search  # noqa: E402
from robot_ebert_amd._lib import call, ptr, stream_of  # noqa: E402

PEAK_F64_TFLOPS = 79.0   # MI355X float64 matrix


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


def stats(v):
    v = sorted(v)
    return {"ms_median": round(v[len(v) // 2], 4), "ms_min": round(v[0], 4),
            "ms_max": round(v[-1], 4)}


def run(config, L, m, iters, rounds):
    cfg = bench.CONFIGS[config]
    dev = torch.device("cuda:0")
    cat = ebt.Catalog(bench.make_catalog_shard(cfg, 0, cfg["n"], dev))
    B, d, k, n = cfg["b"], cfg["d"], cfg["k"], cfg["n"]
    rng = np.random.default_rng(0)
    # L distinct rows per query: a random start and a random stride below n / L
    liked_np = (rng.integers(0, n, size=(B, 1)) +
                np.arange(L)[None, :] * rng.integers(1, n // L, size=(B, 1))) % n
    liked = liked_np.tolist()
    off = torch.arange(0, (B + 1) * L, L, dtype=torch.int64, device=dev)
    lrows = torch.from_numpy(liked_np.reshape(-1)).to(dev)
    # (the CSR is built once: the timed call is the GPU step, not the host's list handling)
    csr = search.csr_from_lists(liked, dev)
    score_ms = timed(lambda: ebt.score_topk(cat, k, liked=csr, exclude=csr), 3)
    _, rows = ebt.score_topk(cat, k, liked=csr, exclude=csr)
    rows = rows.contiguous()
    nnz = B * L
    need = _lib.load().ebt_explain_workspace_bytes(nnz, k)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    val = torch.empty((B, k, m), dtype=torch.float64, device=dev)
    pos = torch.empty((B, k, m), dtype=torch.int32, device=dev)
    lrow = torch.empty((B, k, m), dtype=torch.int64, device=dev)
    tot = torch.empty((B, k), dtype=torch.float64, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    st = stream_of(dev)

    def ours():
        call("ebt_explain_topk", ctypes.byref(cat.cstruct), B, ptr(off), ptr(lrows), None, nnz,
             ptr(rows), k, m, 1, ptr(ws), need, ptr(val), ptr(pos), ptr(lrow), ptr(tot),
             ptr(status), st)

    def contrib_only():
        call("ebt_liked_contrib", ctypes.byref(cat.cstruct), B, ptr(off), ptr(lrows), None,
             ptr(rows), k, ptr(ws), ptr(status), st)

    g = cat.gnorm
    keep = {}

    def torch_baseline():
        a = cat.data.index_select(0, rows.reshape(-1)).to(torch.float64).view(B, k, d)
        b = cat.data.index_select(0, lrows).to(torch.float64).view(B, L, d)
        s = torch.bmm(a, b.transpose(1, 2))
        s = s / (g[rows].unsqueeze(2) * g[lrows].view(B, 1, L)) * (1.0 / L)
        keep["top"] = s.topk(m, dim=2)
        keep["total"] = s.sum(dim=2)

    ms = {"explain_topk": [], "liked_contrib": [], "torch": []}
    for _ in range(rounds):
        ms["explain_topk"].append(timed(ours, iters))
        ms["liked_contrib"].append(timed(contrib_only, iters))
        ms["torch"].append(timed(torch_baseline, iters))
    assert bool((status == 1).all().item())
    # the two paths agree (values within 1e-12; the baseline's topk has no tie rule)
    ours()
    torch_baseline()
    torch.cuda.synchronize()
    err = float((val - keep["top"][0]).abs().max().item())
    flops = 2.0 * B * k * L * d
    out = {"shape": f"{config}-like", "n": n, "d": d, "dtype": cfg["dtype"], "B": B, "k": k,
           "L": L, "m": m, "iters": iters, "rounds": rounds, "flops_per_call": flops,
           "workspace_bytes": int(need)}
    for name, v in ms.items():
        out[name] = stats(v)
    med = out["explain_topk"]["ms_median"]
    out["explain_topk"]["f64_TFLOPs"] = round(flops / med / 1e9, 2)
    out["explain_topk"]["frac_of_79_TFLOPs"] = round(flops / med / 1e9 / PEAK_F64_TFLOPS, 4)
    out["liked_contrib"]["f64_TFLOPs"] = round(flops / out["liked_contrib"]["ms_median"] / 1e9, 2)
    out["torch_over_explain_topk"] = round(out["torch"]["ms_median"] / med, 3)
    out["score_topk_ms"] = round(score_ms, 4)
    out["max_abs_diff_vs_torch"] = err
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="C3,C2")
    ap.add_argument("--liked", type=int, default=85)
    ap.add_argument("--m", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    ebt.load()
    for config in a.shapes.split(","):
        run(config, a.liked, a.m, a.iters, a.rounds)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
