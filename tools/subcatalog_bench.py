"""What a sparse filtered batch costs with and without a materialised sub-catalog (ebert.h 0.7.0):
at C3's shape (1M x 1536 f32, B = 4096, k = 100) and C2's (100K x 768 bf16, B = 1024, k = 100),
every query under one mask of density 0.1 or 0.01 (random rows), in ONE process and interleaved
round by round, ms per step of

  * the default unfiltered step (fused screen), for scale,
  * the mask pass: the filtered step over masks that were never materialised (the path as it was
    before the feature: every row scored, then ebt_mask_allowed),
  * the materialised path: the same ids over masks with a sub-catalog (AllowMasks.materialize).

The two filtered variants are checked to give the same rows and bitwise the same scores before
anything is timed. Also: ms per AllowMasks.materialize call (the count and its read-back, the
compaction, the gather, the host work) and the bytes it moves per second -- per copied row
2 * (d * elem + separate-image bytes + 12), read and written -- against the 8 TB/s HBM figure.

    python tools/subcatalog_bench.py [--shapes C3,C2] [--steps 5] [--rounds 3]

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
DENSITIES = (0.1, 0.01)
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
        plain = ebt.AllowMasks(cat, len(DENSITIES))
        mat = ebt.AllowMasks(cat, len(DENSITIES))
        rng = np.random.default_rng(5)
        rows = {}
        for m, p in enumerate(DENSITIES):
            f = torch.from_numpy(rng.random(n) < p).to(dev)
            plain.from_bool(m, f)
            mat.from_bool(m, f)
        # materialize itself: warm once, then timed (each call rebuilds the copy)
        build_ms = {}
        for m, p in enumerate(DENSITIES):
            mat.materialize(m)
            torch.cuda.synchronize(dev)
            t = []
            for _ in range(a.rounds):
                t0 = time.perf_counter()
                rows[p] = mat.materialize(m)
                torch.cuda.synchronize(dev)
                t.append((time.perf_counter() - t0) * 1e3)
            build_ms[p] = t
        variants = [("fused_unfiltered", dict())]
        for m, p in enumerate(DENSITIES):
            variants.append((f"mask_pass_{p}", dict(allow=(plain, [m] * B))))
            variants.append((f"materialised_{p}", dict(allow=(mat, [m] * B))))

        def step(kw):
            out = ebt.score_topk_finish(ebt.score_topk_submit(cat, k, queries=q, **kw))
            torch.cuda.synchronize(dev)
            return out

        same = {}
        for m, p in enumerate(DENSITIES):
            s0, r0 = step(dict(allow=(plain, [m] * B)))
            pend = ebt.score_topk_submit(cat, k, queries=q, allow=(mat, [m] * B))
            assert [x[0] for x in pend.routes] == [m], "the sub-catalog did not answer"
            s1, r1 = ebt.score_topk_finish(pend)
            same[str(p)] = bool(torch.equal(r0, r1) and
                                torch.equal(s0.view(torch.int64), s1.view(torch.int64)))
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
        elem = cat.data.element_size()
        img = 0 if cat.image.data_ptr() == cat.data.data_ptr() else cat.ld_img * 2
        out = {"shape": name, "n": n, "d": d, "dtype": str(dtype).split(".")[-1], "B": B, "k": k,
               "steps": a.steps, "rounds": a.rounds, "bitwise_equal": same,
               "ms_per_step": {v: round(statistics.median(x), 3) for v, x in ms.items()},
               "ms_per_step_range": {v: [round(min(x), 3), round(max(x), 3)]
                                     for v, x in ms.items()},
               "materialize": {}}
        for p in DENSITIES:
            t = statistics.median(build_ms[p])
            moved = 2 * rows[p] * (d * elem + img + 12)
            out["materialize"][str(p)] = {
                "rows": rows[p], "ms_per_call": round(t, 3),
                "ms_range": [round(min(build_ms[p]), 3), round(max(build_ms[p]), 3)],
                "copy_bytes": rows[p] * (d * elem + img + 12), "moved_bytes": moved,
                "bytes_per_s": round(moved / (t * 1e-3), 1),
                "share_of_8TBps": round(moved / (t * 1e-3) / HBM_BYTES_PER_S, 4)}
        print(json.dumps(out), flush=True)
        del cat, q, plain, mat
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
