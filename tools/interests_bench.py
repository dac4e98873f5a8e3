"""Multi-interest top-k (include/ebert.h 0.11.0) at a C3-like and a C2-like request, against a
torch baseline interleaved in the same process, and beside the scoring steps around it.

    C3-like: 1M x 1536 f32, B = 4096;  C2-like: 100K x 768 bf16, B = 1024;
    both with L = 85 liked rows per query, c = 3 clusters and k = 10. Rows of that many iid
    dimensions are nearly orthogonal, so the first pass already confirms the seeding there; a
    third shape makes the passes count:
    D32: 100K x 32 f32, B = 4096, L = 300 (eight slots per lane; most lists run 8 to 16 passes).

One JSON line per shape: ms per ebt_liked_interests call (median / min / max over the rounds), ms
of ebt_pool_gram alone, ms per ebt_interest_interleave call, ms of the B c-query score_topk step
over the clusters' member lists and of the plain B-query step, and the ms of the torch baseline
(index_select gather, float64 copies, torch.bmm, norm scaling, the seeding, then 16 reassignment
passes with index_add_ and the renumbering, batched over the queries on the device). Before
anything is timed the baseline's labels must equal the library's. hipEvent-timed windows of
`iters` calls, `rounds` alternating windows of each.

    python tools/interests_bench.py [--shapes C3,C2,D32] [--iters 5] [--rounds 3] [--liked 85]
                                    [--c 3] [--k 10]
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
from robot_ebert_amd import _lib, interests, search  # noqa: E402
from robot_ebert_amd._lib import call, ptr, stream_of  # noqa: E402


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


SHAPES = dict(bench.CONFIGS, D32=dict(n=100_000, d=32, dtype="f32", b=4096))
D32_LIKED = 300


def run(config, L, c, k, iters, rounds):
    cfg = SHAPES[config]
    dev = torch.device("cuda:0")
    cat = ebt.Catalog(bench.make_catalog_shard(cfg, 0, cfg["n"], dev))
    B, d, n = cfg["b"], cfg["d"], cfg["n"]
    rng = np.random.default_rng(0)
    # L distinct liked rows per query, ascending: a random start and a random stride below n / L
    start = rng.integers(0, n // 2, size=(B, 1))
    liked_np = start + np.arange(L)[None, :] * rng.integers(1, n // (2 * L), size=(B, 1))
    rows = torch.from_numpy(liked_np.astype(np.int64)).to(dev)
    need = _lib.load().ebt_interest_workspace_bytes(B, L)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    label = torch.empty((B, L), dtype=torch.int32, device=dev)
    size = torch.empty((B, c), dtype=torch.int32, device=dev)
    medoid = torch.empty((B, c), dtype=torch.int32, device=dev)
    n_it = torch.empty(B, dtype=torch.int32, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    st = stream_of(dev)

    def ours():
        call("ebt_liked_interests", ctypes.byref(cat.cstruct), B, ptr(rows), L, c, ptr(ws), need,
             ptr(label), ptr(size), ptr(medoid), ptr(n_it), ptr(status), st)

    def gram_only():
        call("ebt_pool_gram", ctypes.byref(cat.cstruct), B, ptr(rows), L, ptr(ws), ptr(status), st)

    g = cat.gnorm
    keep = {}
    ar = torch.arange(B, device=dev)
    base = (ar * c)[:, None]
    ones = torch.ones(B * L, dtype=torch.float64, device=dev)

    def torch_baseline():
        x = cat.data.index_select(0, rows.reshape(-1)).to(torch.float64).view(B, L, d)
        s = torch.bmm(x, x.transpose(1, 2))
        gr = g[rows]
        s = s / (gr.unsqueeze(2) * gr.unsqueeze(1))
        seed = [s.sum(dim=2).argmax(dim=1)]
        near = s[ar, seed[0]]
        taken = torch.zeros((B, L), dtype=torch.bool, device=dev)
        taken[ar, seed[0]] = True
        for m in range(1, c):
            seed.append(near.masked_fill(taken, float("inf")).argmin(dim=1))
            near = torch.maximum(near, s[ar, seed[m]])
            taken[ar, seed[m]] = True
        lab = torch.stack([s[ar, sm] for sm in seed], dim=2).argmax(dim=2)
        for m in range(c):
            lab[ar, seed[m]] = m
        flat = s.view(B * L, L)
        for _ in range(_lib.EBT_INTEREST_ITERS):
            idx = (base + lab).view(-1)
            acc = torch.zeros((B * c, L), dtype=torch.float64, device=dev).index_add_(0, idx, flat)
            cnt = torch.zeros(B * c, dtype=torch.float64, device=dev).index_add_(0, idx, ones)
            mean = (acc / cnt[:, None]).view(B, c, L)
            mean = mean.masked_fill((cnt == 0).view(B, c, 1), float("-inf"))
            lab = mean.argmax(dim=1)
        cnt = torch.zeros(B * c, dtype=torch.int64, device=dev).index_add_(
            0, (base + lab).view(-1), torch.ones(B * L, dtype=torch.int64, device=dev)).view(B, c)
        low = torch.full((B, c), L, dtype=torch.int64, device=dev).scatter_reduce_(
            1, lab, torch.arange(L, device=dev).expand(B, L), "amin")
        order = torch.argsort(-cnt * (L + 1) + low, dim=1)      # (n desc, lowest member asc)
        rank = torch.empty_like(order).scatter_(1, order, torch.arange(c, device=dev).expand(B, c))
        keep["label"] = rank.gather(1, lab)

    ours()
    torch_baseline()
    torch.cuda.synchronize()
    assert bool((status == 1).all().item())
    same = bool(torch.equal(keep["label"], label.long()))
    if not same:
        raise SystemExit(f"{config}: the torch baseline's labels differ from the library's in "
                         f"{int((keep['label'] != label.long()).any(dim=1).sum())} of {B} queries")
    # the scoring steps: B c member lists (the clusters), and the plain B lists beside them
    lab_np, size_np = label.cpu().numpy(), size.cpu().numpy()
    members = [liked_np[b][lab_np[b] == m] for b in range(B) for m in range(c) if size_np[b, m] > 0]
    owner = torch.as_tensor([b * c + m for b in range(B) for m in range(c) if size_np[b, m] > 0],
                            dtype=torch.int64, device=dev)
    excl = search.csr_from_lists([liked_np[int(o) // c] for o in owner.cpu().tolist()], dev)
    mem_csr = search.csr_from_lists(members, dev)
    all_csr = search.csr_from_lists(liked_np, dev)
    sc, rw = ebt.score_topk(cat, k, liked=mem_csr, exclude=excl)
    list_rows = torch.full((B * c, k), -1, dtype=torch.int64, device=dev)
    list_scores = torch.full((B * c, k), float("nan"), dtype=torch.float64, device=dev)
    list_rows[owner], list_scores[owner] = rw, sc
    list_rows, list_scores = list_rows.view(B, c, k), list_scores.view(B, c, k)
    ms = {"liked_interests": [], "pool_gram": [], "interleave": [], "torch": [],
          "score_topk_clusters": [], "score_topk_plain": []}
    for _ in range(rounds):
        ms["liked_interests"].append(timed(ours, iters))
        ms["pool_gram"].append(timed(gram_only, iters))
        ms["torch"].append(timed(torch_baseline, iters))
        ms["interleave"].append(timed(lambda: interests.interleave(size, list_rows, list_scores),
                                      iters))
        ms["score_topk_clusters"].append(
            timed(lambda: ebt.score_topk(cat, k, liked=mem_csr, exclude=excl), 2))
        ms["score_topk_plain"].append(
            timed(lambda: ebt.score_topk(cat, k, liked=all_csr, exclude=all_csr), 2))
    it = n_it.cpu().numpy()
    out = {"shape": f"{config}-like", "n": n, "d": d, "dtype": cfg["dtype"], "B": B, "L": L, "c": c,
           "k": k, "iters": iters, "rounds": rounds, "workspace_bytes": int(need),
           "labels_equal_torch": same, "cluster_queries": len(members),
           "passes_mean": round(float(it.mean()), 2),
           "passes_at_cap": int((it == _lib.EBT_INTEREST_ITERS).sum())}
    for name, v in ms.items():
        out[name] = stats(v)
    out["cluster_only_ms"] = round(out["liked_interests"]["ms_median"] -
                                   out["pool_gram"]["ms_median"], 4)
    out["torch_over_liked_interests"] = round(out["torch"]["ms_median"] /
                                              out["liked_interests"]["ms_median"], 3)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="C3,C2,D32")
    ap.add_argument("--liked", type=int, default=85)
    ap.add_argument("--c", type=int, default=3)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    ebt.load()
    for config in a.shapes.split(","):
        run(config, D32_LIKED if config == "D32" else a.liked, a.c, a.k, a.iters, a.rounds)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
