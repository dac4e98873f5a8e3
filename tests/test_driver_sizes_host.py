"""CPU: the sizing entries of the self-contained path return, bit for bit, the values recorded in
tests/golden/driver_sizes.json (tests/golden/make_driver_sizes.py wrote them from the library at
ABI 0.6.0, so that the driver's layouts can be single-sourced later against fixed numbers). Host
arithmetic only: the catalog's device pointers are fakes that are never read. Zeros are refused
inputs and are pinned too.

Which rows cover which branch
-----------------------------
state (ebt_catalog_state_bytes):
  * dtype 1, 2 with (d, ld) = (64, 64) or (1536, 1536) and the aligned pointer: the matrix is its
    own image (no image region); the same with the pointer + 8, or (64, 65), or (100, 100): an
    image copy; dtype 0, 3: image + the 4-byte error slot;
  * n = 127 / 128 / 129: the inverse norms' padding to 128 rows; n = 0 and ld < d: 0.
driver (ebt_workspace_bytes):
  * n = 50, k = 100 / 512 / 4096 / 5000: k_eff < k, the padded results regions;
  * n >= 5000, k = 5000: the full-sort layout (min(k, n) > 4096); n = 5000, k = 4096: the widest
    screened k';
  * B = 1 / 128 / 129 / 300 / 4096: both batch paddings, retry groups smaller than and equal to
    256 queries;
  * kprime 8 (clamped up to k), 600, 4096 (clamped to the catalog at n = 50); chunk_rows 128 and
    262144 (given) and 100 (not a multiple of 128 -> 0); flags NO_FUSE, LIKED_CHECKED (sizes as
    without it) and an unknown bit (-> 0).
sharded (ebt_sharded_workspace_bytes), every case at world 1, 2, 8 with and without
all_reduce_f64 (without it: the gathered partial sums of the liked path):
  * c3 / c3_native at world 8 (125 000-row shards, B = 4096): sample tiles > 0, the lead's room,
    packed results (cap > 0); at world 2 (500 000-row shards) and ten_million: tiles = 0;
    world 1: tiles = 0 and cap = 0 (the full exchange);
  * short_shard at world 8: a 1000-row shard of a 1M-row catalog, where the screen at the shared
    threshold needs more than the retries' pass region (its own region is carved);
  * padded: k_eff < k on a 50-row shard; small_batch: B_pad = 256;
  * wide_k: k = 2000, no shared threshold (k' > 512), cap = 0 at world 8 (world * k > 8192);
  * no_fuse, kprime_600: the shared threshold switched off by options; chunk_128: a given chunk;
  * k_4096: the largest k; k_4097: 0; offset_ok / offset_past_end: n_global against
    row_offset + n (the latter 0).
"""
import json
import os

import pytest

import make_driver_sizes as gen

with open(os.path.join(os.path.dirname(os.path.abspath(gen.__file__)), "driver_sizes.json")) as f:
    GOLDEN = json.load(f)


@pytest.mark.parametrize("name,cols,grid,fn", gen.PARTS, ids=[p[0] for p in gen.PARTS])
def test_sizes_match_the_recorded_ones(name, cols, grid, fn):
    from robot_ebert_amd import _lib
    lib = _lib.load()
    part = GOLDEN[name]
    assert part["columns"] == cols + ["bytes"]
    assert [r[:-1] for r in part["rows"]] == grid(), "the grid changed: regenerate on purpose only"
    got = [[*r[:-1], int(fn(lib, *r[:-1]))] for r in part["rows"]]
    wrong = [(g, r[-1]) for g, r in zip(got, part["rows"]) if g != r]
    assert not wrong, f"{len(wrong)} of {len(got)} sizes differ, first: {wrong[:5]}"
    assert any(r[-1] == 0 for r in part["rows"]) and any(r[-1] > 0 for r in part["rows"])
