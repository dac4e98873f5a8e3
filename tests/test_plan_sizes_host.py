"""CPU: the unfused plan's sizing entries return, bit for bit, the values recorded in
tests/golden/plan_sizes.json (tests/golden/make_plan_sizes.py wrote them from the library at ABI
0.12.0, when the prepared pipeline and the grouped pipeline each computed the chunk plan on their
own). Both now take it from one function (api.hip chunk_plan), so a change to the chunk, pitch or
segment rule moves both layouts or neither. Host arithmetic only; the fused flags are left out
because that layout depends on the device's CU count.

Which rows cover which branch of the plan
-----------------------------------------
  * the pitch: chunk 128 (and n = 1, 1000 at any chunk_rows) keeps ld_s = chunk rounded to 4 below
    1024; chunk 1024, 4224, 16384 (and n = 4099, 8192 cut to the catalog) take the
    "64 past a multiple of 64" pitch, 1024 exactly at its threshold;
  * the segments: B = 1, 4 want 512 and 128 of them and are capped by chunk / 8192 (1 below
    16384 rows, 2 at chunk 16384 of n = 70000, 1 at n = 8192: the chunk is cut to the catalog
    first); B = 130 wants 4 (capped at 2), B = 512 and 600 want 1;
  * one chunk (n <= chunk_rows, n = 1 included) against many (n = 70000: 547 chunks of 128, 5 of
    16384 with a short last one; n = 4099 over 1024: a last chunk of 3 rows);
  * EBT_FLAG_EXACT: the eps block behind the lists; grouped: G = 1, 5, 64 lists per query, and
    lists = n_chunks * segs = 1 (no per-chunk lists) against more.
"""
import json
import os

import pytest

import make_plan_sizes as gen

with open(os.path.join(os.path.dirname(os.path.abspath(gen.__file__)), "plan_sizes.json")) as f:
    GOLDEN = json.load(f)


@pytest.mark.parametrize("name,cols,outs,grid,fn", gen.PARTS, ids=[p[0] for p in gen.PARTS])
def test_sizes_match_the_recorded_ones(name, cols, outs, grid, fn):
    from robot_ebert_amd import _lib
    lib = _lib.load()
    part = GOLDEN[name]
    n_in = len(cols)
    assert part["columns"] == cols + outs
    assert [r[:n_in] for r in part["rows"]] == grid(), "the grid changed: regenerate on purpose only"
    got = [r[:n_in] + fn(lib, *r[:n_in]) for r in part["rows"]]
    wrong = [(g, r) for g, r in zip(got, part["rows"]) if g != r]
    assert not wrong, f"{len(wrong)} of {len(got)} rows differ, first (got, recorded): {wrong[:5]}"
    assert all(r[-1] > 0 for r in part["rows"])


def test_the_grid_crosses_every_branch_of_the_plan():
    """From the recorded plan outputs themselves: chunks below and from the pitch threshold on,
    segment counts capped by the chunk and by B, one chunk and many. This shows what the grid
    covers; the library is checked by the comparison above, where the segment count enters
    through the sizes of the lists (it is not an output of the plan entry)."""
    col = {c: i for i, c in enumerate(GOLDEN["prepared"]["columns"])}
    rows = GOLDEN["prepared"]["rows"]
    assert all(r[col["rc"]] == 0 and r[col["fused"]] == 0 and r[col["head_rows"]] == r[col["n"]]
               and r[col["chunk"]] == min(r[col["chunk_rows"]], r[col["n"]]) for r in rows)
    chunks = {r[col["chunk"]] for r in rows}
    assert {1, 128, 1000, 1024, 4099, 4224, 8192, 16384} <= chunks      # both sides of 1024
    many = {-(-r[col["n"]] // r[col["chunk"]]) for r in rows}
    assert {1, 2, 5, 547} <= many
    want = {(r[col["B"]], min(-(-512 // r[col["B"]]), max(r[col["chunk"]] // 8192, 1)))
            for r in rows}
    assert {(1, 1), (1, 2), (130, 1), (130, 2), (512, 1), (600, 1)} <= want
