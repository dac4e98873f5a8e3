"""What a front page of G shelves costs (grouped top-k, ebert.h 0.12.0): at a C3-like request
(1M x 1536 f32, B = 4096) and a C2-like one (100K x 768 bf16, B = 1024), k = 10, G in {4, 16}
random masks of density 0.1 (independent, so they overlap), in ONE process and interleaved round
by round, ms per call of

  * score_topk_grouped(cat, k, masks, groups) -- one scoring pass, one list per (query, group),
  * the baseline, the code as it stood: G calls of score_topk(..., allow=(masks, [g] * B)).

The two results must be bitwise equal before anything is timed. A second interleaved pass records
the grouped call's EBT_STAGE_SELECT time (the grouped select's launches, one stage record per score
chunk) and its bytes/s against B n 4 bytes per launch -- each launch reads the score chunk once --
and the 8 TB/s HBM figure of MI355X_MICROARCH.md, and its GEMM, mask, merge and rescore stages.

    bash tools/gpu.sh py OUT tools/grouped_bench.py [--shapes C3,C2] [--steps 3] [--rounds 3]

One JSON line per (shape, G). Both sides are warmed up before the first timed round; a call is
followed by a device synchronise, host clock; medians over the rounds.
"""
import argparse
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

SHAPES = {"C3": (1_000_000, 1536, torch.float32, 4096),
          "C2": (100_000, 768, torch.bfloat16, 1024)}
GS = (4, 16)
K = 10
DENSITY = 0.1
HBM_BYTES_PER_S = 8e12
STAGES = ("gemm", "mask", "select", "merge_select", "rescore")


def make_matrix(n, d, dtype, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    out = torch.empty((n, d), dtype=dtype, device=dev)
    for a in range(0, n, 65536):      # in blocks: no float32 temporary of the whole matrix
        b = min(n, a + 65536)
        out[a:b] = torch.randn((b - a, d), generator=g, device=dev, dtype=torch.float32).to(dtype)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="C3,C2")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.load()
    for name in a.shapes.split(","):
        n, d, dtype, B = SHAPES[name]
        cat = ebt.Catalog(make_matrix(n, d, dtype, dev, 1))
        q = make_matrix(B, d, dtype, dev, 2)
        masks = ebt.AllowMasks(cat, max(GS))
        rng = np.random.default_rng(5)
        for m in range(max(GS)):
            masks.from_bool(m, torch.from_numpy(rng.random(n) < DENSITY).to(dev))
        ids = [torch.full((B,), m, dtype=torch.int32, device=dev) for m in range(max(GS))]
        for G in GS:
            groups = list(range(G))

            def grouped(timer=None):
                out = ebt.score_topk_grouped(cat, K, masks, groups, queries=q, timer=timer)
                torch.cuda.synchronize(dev)
                return out

            def baseline():
                out = [ebt.score_topk(cat, K, queries=q, allow=(masks, ids[g])) for g in groups]
                torch.cuda.synchronize(dev)
                return out

            got, want = grouped(), baseline()
            for g in groups:      # bitwise equal before anything is timed
                assert torch.equal(got.rows[:, g], want[g][1]), (name, G, g, "rows")
                assert torch.equal(got.scores[:, g].view(torch.int64),
                                   want[g][0].view(torch.int64)), (name, G, g, "scores")
            for _ in range(a.warmup):
                grouped()
                baseline()
            ms = {"grouped": [], "baseline": []}
            for _ in range(a.rounds):
                for side, f in (("grouped", grouped), ("baseline", baseline)):
                    t0 = time.perf_counter()
                    for _ in range(a.steps):
                        f()
                    ms[side].append((time.perf_counter() - t0) / a.steps * 1e3)
            timer = ebt.Timer()
            timer.only(*STAGES)
            stage = {s: [] for s in STAGES}
            records = 0
            for _ in range(a.rounds):
                timer.reset()
                for _ in range(a.steps):
                    grouped(timer)
                for s in STAGES:
                    tot, cnt = timer.query(s)
                    stage[s].append(tot / a.steps)
                    if s == "select":
                        records = cnt // a.steps
            kp = min(ebt.search.default_kprime(cat, K), _lib.EBT_GROUPED_KPRIME_MAX)
            passes = -(-G // int(lib.ebt_grouped_pass_groups(kp)))
            sel = statistics.median(stage["select"])
            read = 4 * B * n * passes                    # every launch reads its chunk once
            med = {side: statistics.median(x) for side, x in ms.items()}
            out = {"shape": name, "n": n, "d": d, "dtype": str(dtype).split(".")[-1], "B": B,
                   "k": K, "G": G, "density": DENSITY, "kprime": kp, "fallback": got.fallback,
                   "steps": a.steps, "rounds": a.rounds,
                   "ms_per_call": {s: round(v, 3) for s, v in med.items()},
                   "ms_per_call_range": {s: [round(min(x), 3), round(max(x), 3)]
                                         for s, x in ms.items()},
                   "grouped_over_baseline": round(med["grouped"] / med["baseline"], 4),
                   "stage_ms_per_call": {s: round(statistics.median(x), 3)
                                         for s, x in stage.items()},
                   "select": {"ms_per_call": round(sel, 3), "chunks_per_call": records,
                              "launches_per_chunk": passes, "score_bytes_read": read,
                              "bytes_per_s": round(read / (sel * 1e-3), 1) if sel > 0 else 0.0,
                              "share_of_8TBps": round(read / (sel * 1e-3) / HBM_BYTES_PER_S, 4)
                              if sel > 0 else 0.0}}
            print(json.dumps(out), flush=True)
            del got, want
        del cat, q, masks, ids
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
