"""What a filtered batch costs (per-query allow masks, ebert.h 0.6.0): at C3's shape (1M x 1536
f32, B = 4096, k = 100) and C2's (100K x 768 bf16, B = 1024, k = 100), in ONE process and
interleaved round by round, ms per step of

  * the default step (fused screen),
  * the unfiltered step with fuse=False (the path a filtered batch is forced onto),
  * the filtered step, every query under one mask of density 1.0, 0.1 and 0.01 (random rows).

The cost of the feature is filtered minus unfiltered-unfused; the fused step is there to show what
forcing the unfused path costs. A second interleaved pass records the EBT_STAGE_MASK time of the
filtered steps (no exclusions here, so the stage is mask_allowed_kernel alone, one launch per score
chunk) and its achieved bytes/s against the 8 TB/s HBM figure of MI355X_MICROARCH.md. Bytes
counted: 4 B n (1 - density) stored plus 16 B per mixed group of 4 columns read (a mixed group is
also stored whole: `bytes_with_mixed_stores` counts that too).

    bash tools/gpu.sh py OUT tools/allow_bench.py [--shapes C3,C2] [--steps 5] [--rounds 3]

One JSON line per shape. Every variant is warmed up (--warmup steps) before the first timed round;
a step is score_topk_submit + score_topk_finish followed by a device synchronise, host clock.
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

SHAPES = {"C3": (1_000_000, 1536, torch.float32, 4096, 100),
          "C2": (100_000, 768, torch.bfloat16, 1024, 100)}
DENSITIES = (1.0, 0.1, 0.01)
HBM_BYTES_PER_S = 8e12


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
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for name in a.shapes.split(","):
        n, d, dtype, B, k = SHAPES[name]
        cat = ebt.Catalog(make_matrix(n, d, dtype, dev, 1))
        q = make_matrix(B, d, dtype, dev, 2)
        masks = ebt.AllowMasks(cat, len(DENSITIES))
        rng = np.random.default_rng(5)
        facts = {}
        for m, p in enumerate(DENSITIES):
            f = np.ones(n, bool) if p >= 1.0 else rng.random(n) < p
            masks.from_bool(m, torch.from_numpy(f).to(dev))
            g = np.pad(f, (0, -n % 4)).reshape(-1, 4).sum(1)
            facts[p] = dict(allowed=int(f.sum()), mixed_groups=int(((g > 0) & (g < 4)).sum()),
                            empty_groups=int((g == 0).sum()))
        ids = [torch.full((B,), m, dtype=torch.int32, device=dev) for m in range(len(DENSITIES))]
        variants = [("fused", dict()), ("unfused", dict(fuse=False))]
        variants += [(f"allow_{p}", dict(allow=(masks, ids[m]))) for m, p in enumerate(DENSITIES)]

        def step(kw, timer=None):
            ebt.score_topk_finish(ebt.score_topk_submit(cat, k, queries=q, timer=timer, **kw))
            torch.cuda.synchronize(dev)

        for _, kw in variants:
            for _ in range(a.warmup):
                step(kw)
        ms = {v: [] for v, _ in variants}
        for _ in range(a.rounds):
            for v, kw in variants:
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    step(kw)
                ms[v].append((time.perf_counter() - t0) / a.steps * 1e3)
        # the mask stage alone, by the library's stage timer (events around each launch)
        timer = ebt.Timer()
        timer.only("mask")
        stage = {}
        for _ in range(a.rounds):
            for (v, kw), p in zip(variants[2:], DENSITIES):
                timer.reset()
                for _ in range(a.steps):
                    step(kw, timer)
                tot, launches = timer.query("mask")
                stage.setdefault(p, []).append((tot / a.steps, launches // a.steps))
        out = {"shape": name, "n": n, "d": d, "dtype": str(dtype).split(".")[-1], "B": B, "k": k,
               "steps": a.steps, "rounds": a.rounds,
               "ms_per_step": {v: round(statistics.median(x), 3) for v, x in ms.items()},
               "ms_per_step_range": {v: [round(min(x), 3), round(max(x), 3)]
                                     for v, x in ms.items()}}
        base = out["ms_per_step"]["unfused"]
        out["filtered_minus_unfused_ms"] = {str(p): round(out["ms_per_step"][f"allow_{p}"] - base, 3)
                                            for p in DENSITIES}
        out["mask_stage"] = {}
        for p in DENSITIES:
            t = statistics.median(x[0] for x in stage[p])
            fa = facts[p]
            stored = 4 * B * (n - fa["allowed"])
            reads = 16 * B * fa["mixed_groups"]
            moved = 16 * B * (fa["empty_groups"] + 2 * fa["mixed_groups"])
            bps = (stored + reads) / (t * 1e-3) if t > 0 else 0.0
            out["mask_stage"][str(p)] = {
                "ms_per_step": round(t, 4), "launches_per_step": stage[p][0][1],
                "allowed_rows": fa["allowed"], "mixed_groups": fa["mixed_groups"],
                "stored_bytes": stored, "mixed_read_bytes": reads,
                "bytes_with_mixed_stores": moved, "bytes_per_s": round(bps, 1),
                "share_of_8TBps": round(bps / HBM_BYTES_PER_S, 4),
                "share_of_8TBps_with_mixed_stores": round(
                    moved / (t * 1e-3) / HBM_BYTES_PER_S, 4) if t > 0 else 0.0}
        print(json.dumps(out), flush=True)
        del cat, q, masks
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
