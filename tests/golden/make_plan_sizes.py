"""Record the unfused plan's sizing entries over a grid that crosses every branch of the plan.

    python tests/golden/make_plan_sizes.py

Writes tests/golden/plan_sizes.json: what the BUILT library returns from ebt_cosine_topk_plan and
ebt_cosine_topk_workspace at the flags EBT_FLAG_NO_FUSE and EBT_FLAG_EXACT, and from
ebt_cosine_topk_grouped_workspace at the flags 0 and EBT_FLAG_EXACT (host arithmetic: no GPU).
Only the unfused flags are recorded: the fused layout depends on the device's CU count. The file
was written from the library at ABI 0.12.0, before the prepared pipeline and the grouped pipeline
shared one chunk plan; tests/test_plan_sizes_host.py holds every later build to these integers.
Regenerate only when the plan is changed on purpose.
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from robot_ebert_amd import _lib  # noqa: E402

NO_FUSE, EXACT = _lib.EBT_FLAG_NO_FUSE, _lib.EBT_FLAG_EXACT
BS = (1, 4, 130, 512, 600)
NS = (1, 1000, 4099, 8192, 70000)
CHUNKS = (128, 1024, 4224, 16384)
KPRIMES = (32, 512)
GS = (1, 5, 64)

PREPARED_COLS = ["B", "n", "chunk_rows", "kprime", "flags"]
GROUPED_COLS = PREPARED_COLS + ["G"]


def pad_batch(B):
    """search.pad_batch"""
    return 128 if B <= 128 else (B + 255) // 256 * 256


def prepared(lib, B, n, chunk_rows, kprime, flags):
    """[rc, head_rows, cap, chunk, fused] of ebt_cosine_topk_plan, then the workspace bytes"""
    h, cap, ch = ctypes.c_int64(-1), ctypes.c_int64(-1), ctypes.c_int64(-1)
    fused = ctypes.c_int32(-1)
    rc = lib.ebt_cosine_topk_plan(B, pad_batch(B), n, kprime, chunk_rows, flags, ctypes.byref(h),
                                  ctypes.byref(cap), ctypes.byref(ch), ctypes.byref(fused))
    ws = lib.ebt_cosine_topk_workspace(B, pad_batch(B), n, kprime, chunk_rows, flags)
    return [int(rc), h.value, cap.value, ch.value, fused.value, int(ws)]


def grouped(lib, B, n, chunk_rows, kprime, flags, G):
    return [int(lib.ebt_cosine_topk_grouped_workspace(B, pad_batch(B), n, kprime, chunk_rows,
                                                      flags, G))]


def _grid(flagset, extra=((),)):
    return [[B, n, c, kp, fl, *x] for B in BS for n in NS for c in CHUNKS for kp in KPRIMES
            for fl in flagset for x in extra]


def prepared_grid():
    return _grid((NO_FUSE, EXACT))


def grouped_grid():
    return _grid((0, EXACT), [(G,) for G in GS])


PARTS = (("prepared", PREPARED_COLS, ["rc", "head_rows", "cap", "chunk", "fused", "bytes"],
          prepared_grid, prepared),
         ("grouped", GROUPED_COLS, ["bytes"], grouped_grid, grouped))


def main():
    lib = _lib.load()
    path = os.path.join(HERE, "plan_sizes.json")
    with open(path, "w") as f:
        for i, (name, cols, outs, grid, fn) in enumerate(PARTS):
            f.write('%s "%s": {"columns": %s, "rows": [\n  '
                    % (",\n" if i else "{\n", name, json.dumps(cols + outs)))
            f.write(",\n  ".join(json.dumps(row + fn(lib, *row)) for row in grid()))
            f.write("\n ]}")
        f.write("\n}\n")
    print("wrote", path, {name: len(grid()) for name, _, _, grid, _ in PARTS})


if __name__ == "__main__":
    main()
