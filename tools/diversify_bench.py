"""ebt_mmr_topk (include/ebert.h 0.10.0) at a C3-like and a C2-like request, against a torch
baseline interleaved in the same process, and beside the score_topk(p) step that produced the pool.

    C3-like: 1M x 1536 f32, B = 4096;  C2-like: 100K x 768 bf16, B = 1024;
    both with a pool of p = 100, k = 10 picks and lam = 0.7.

One JSON line per shape: ms per ebt_mmr_topk call (median / min / max over the rounds), ms of
ebt_pool_gram alone with its float64 FLOP/s (2 B p^2 d useful flops per call) against the 79
TFLOP/s float64 matrix peak of SURVEY, the ms of the torch baseline (index_select gather, float64
copies, torch.bmm, norm scaling, then k rounds of batched argmax / maximum on the device) and the
ms of the score_topk call. Before anything is timed the baseline's selections must equal the
library's. hipEvent-timed windows of `iters` calls, `rounds` alternating windows of each.

    python tools/diversify_bench.py [--shapes C3,C2] [--iters 5] [--rounds 3] [--pool 100]
                                    [--k 10] [--lam 0.7] [--liked 85]
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


def run(config, L, p, k, lam, iters, rounds):
    cfg = bench.CONFIGS[config]
    dev = torch.device("cuda:0")
    cat = ebt.Catalog(bench.make_catalog_shard(cfg, 0, cfg["n"], dev))
    B, d, n = cfg["b"], cfg["d"], cfg["n"]
    rng = np.random.default_rng(0)
    # L distinct liked rows per query: a random start and a random stride below n / L
    liked_np = (rng.integers(0, n, size=(B, 1)) +
                np.arange(L)[None, :] * rng.integers(1, n // L, size=(B, 1))) % n
    csr = search.csr_from_lists(liked_np.tolist(), dev)
    score_ms = timed(lambda: ebt.score_topk(cat, p, liked=csr, exclude=csr), 3)
    rel, rows = ebt.score_topk(cat, p, liked=csr, exclude=csr)
    rel, rows = rel.contiguous(), rows.contiguous()
    need = _lib.load().ebt_mmr_workspace_bytes(B, p)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    pos = torch.empty((B, k), dtype=torch.int32, device=dev)
    orow = torch.empty((B, k), dtype=torch.int64, device=dev)
    orel = torch.empty((B, k), dtype=torch.float64, device=dev)
    ommr = torch.empty((B, k), dtype=torch.float64, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    st = stream_of(dev)

    def ours():
        call("ebt_mmr_topk", ctypes.byref(cat.cstruct), B, ptr(rel), ptr(rows), p, k, lam, ptr(ws),
             need, ptr(pos), ptr(orow), ptr(orel), ptr(ommr), ptr(status), st)

    def gram_only():
        call("ebt_pool_gram", ctypes.byref(cat.cstruct), B, ptr(rows), p, ptr(ws), ptr(status), st)

    g = cat.gnorm
    keep = {}
    ar = torch.arange(B, device=dev)

    def torch_baseline():
        x = cat.data.index_select(0, rows.reshape(-1)).to(torch.float64).view(B, p, d)
        s = torch.bmm(x, x.transpose(1, 2))
        gr = g[rows]
        s = s / (gr.unsqueeze(2) * gr.unsqueeze(1))
        pen = torch.zeros_like(rel)
        alive = torch.ones_like(rel, dtype=torch.bool)
        picks = []
        for t in range(k):
            v = (lam * rel - (1.0 - lam) * pen).masked_fill(~alive, float("-inf"))
            c = v.argmax(dim=1)
            picks.append(c)
            alive[ar, c] = False
            row = s[ar, c]
            pen = row if t == 0 else torch.maximum(pen, row)
        keep["pos"] = torch.stack(picks, dim=1)

    # the two paths pick the same slots (the pool of a search has no empty slot and no NaN here)
    ours()
    torch_baseline()
    torch.cuda.synchronize()
    assert bool((status == 1).all().item())
    same = bool(torch.equal(keep["pos"], pos.long()))
    if not same:
        raise SystemExit(f"{config}: the torch baseline's selections differ from the library's in "
                         f"{int((keep['pos'] != pos.long()).any(dim=1).sum())} of {B} queries")
    ms = {"mmr_topk": [], "pool_gram": [], "torch": []}
    for _ in range(rounds):
        ms["mmr_topk"].append(timed(ours, iters))
        ms["pool_gram"].append(timed(gram_only, iters))
        ms["torch"].append(timed(torch_baseline, iters))
    flops = 2.0 * B * p * p * d
    out = {"shape": f"{config}-like", "n": n, "d": d, "dtype": cfg["dtype"], "B": B, "p": p,
           "k": k, "lam": lam, "L": L, "iters": iters, "rounds": rounds, "flops_per_call": flops,
           "workspace_bytes": int(need), "selections_equal_torch": same}
    for name, v in ms.items():
        out[name] = stats(v)
    med = out["mmr_topk"]["ms_median"]
    gmed = out["pool_gram"]["ms_median"]
    out["pool_gram"]["f64_TFLOPs"] = round(flops / gmed / 1e9, 2)
    out["pool_gram"]["frac_of_79_TFLOPs"] = round(flops / gmed / 1e9 / PEAK_F64_TFLOPS, 4)
    out["torch_over_mmr_topk"] = round(out["torch"]["ms_median"] / med, 3)
    out["score_topk_ms"] = round(score_ms, 4)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="C3,C2")
    ap.add_argument("--liked", type=int, default=85)
    ap.add_argument("--pool", type=int, default=100)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--lam", type=float, default=0.7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    ebt.load()
    for config in a.shapes.split(","):
        run(config, a.liked, a.pool, a.k, a.lam, a.iters, a.rounds)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
