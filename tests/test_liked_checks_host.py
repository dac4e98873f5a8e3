"""CPU: the shared Python checks of liked weights and of whole catalogs, message by message.

search.parse_weight_lists and search.device_liked_weights serve search._liked_with_weights,
csr_from_weighted_lists and explain._liked_csr; catalog.require_whole_catalog serves explain,
diversify and interests. Callers match on these texts, so each is pinned whole, through the
helper and through the public functions that raise it."""
import numpy as np
import pytest
import torch


def _raises(fn, *a):
    from robot_ebert_amd import EbertError
    with pytest.raises(EbertError) as ei:
        fn(*a)
    return str(ei.value)


def test_parse_weight_lists_messages_and_order():
    from robot_ebert_amd import search
    f = search.parse_weight_lists
    segs, ws = f([[5, 2], [], [7]], [[1.5, -2.0], [], [0.0]])
    assert [s.tolist() for s in segs] == [[5, 2], [], [7]]          # the caller's order
    assert [w.tolist() for w in ws] == [[1.5, -2.0], [], [0.0]]
    assert all(s.dtype == np.int64 for s in segs) and all(w.dtype == np.float64 for w in ws)
    assert _raises(f, [[1], [2, 3]], [[1.0]]) == "1 weight lists for 2 liked lists"
    assert _raises(f, [[1], [2, 3]], [[1.0], [1.0]]) == "query 1 has 1 weights for 2 liked rows"
    msg = _raises(f, [[1], [2]], [[1.0], ["x"]])
    assert msg.startswith("liked weights of query 1: ") and "x" in msg
    # the first bad query wins, and a length is checked before a later query is parsed
    assert _raises(f, [[1], [2]], [[], ["x"]]) == "query 0 has 0 weights for 1 liked rows"


def test_parse_weight_lists_is_what_both_callers_raise():
    from robot_ebert_amd import explain, search
    lists, bad = [[1], [2, 3]], [[1.0], [1.0]]
    want = "query 1 has 1 weights for 2 liked rows"
    assert _raises(search.csr_from_weighted_lists, lists, bad, "cpu") == want
    assert _raises(explain._liked_csr, lists, bad, "cpu") == want
    assert _raises(search._liked_with_weights, lists, bad, "cpu") == want


def test_device_liked_weights_messages():
    from robot_ebert_amd import explain, search
    not_tensor = "with a device CSR, liked_weights must be a device float64 [nnz] tensor"
    assert _raises(search.device_liked_weights, [1.0, 2.0], 2) == not_tensor
    csr = (torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int64))
    assert _raises(search._liked_with_weights, csr, [1.0, 2.0], "cpu") == not_tensor
    no_cpu = "liked_weights must be a CUDA (HIP) tensor; libebert has no CPU path"
    assert _raises(search.device_liked_weights, torch.ones(2, dtype=torch.float64), 2) == no_cpu
    assert _raises(search._liked_with_weights, csr, torch.ones(2, dtype=torch.float64),
                   "cpu") == no_cpu
    # (explain._liked_csr asks for a device CSR first)
    assert _raises(explain._liked_csr, csr, [1.0, 2.0], "cpu") == \
        "liked offsets must be a CUDA (HIP) tensor; libebert has no CPU path"


def test_device_liked_weights_shape_message(monkeypatch):
    """The dtype / shape text, with the device check stubbed out (no GPU here)."""
    from robot_ebert_amd import search
    monkeypatch.setattr(search, "require_cuda", lambda t, what: None)
    for t in (torch.ones(3, dtype=torch.float32), torch.ones(2, dtype=torch.float64),
              torch.ones((3, 1), dtype=torch.float64)):
        assert _raises(search.device_liked_weights, t, 3) == (
            f"liked_weights must be float64 [3] (one per liked row), got {t.dtype} "
            f"{tuple(t.shape)}")
    ok = torch.ones(6, dtype=torch.float64)[::2]
    got = search.device_liked_weights(ok, 3)
    assert got.is_contiguous() and got.tolist() == [1.0, 1.0, 1.0]


def test_require_whole_catalog_messages():
    from robot_ebert_amd import diversify, explain, interests
    from robot_ebert_amd.catalog import require_whole_catalog

    class Shard:
        n, n_global, row_offset, device = 500, 1000, 500, None

    class Whole:
        n, n_global = 1000, 1000

    require_whole_catalog(Whole(), "anything")
    tail = ": this catalog is a shard (500 of 1000 rows)"
    assert _raises(require_whole_catalog, Shard(), "x needs y") == "x needs y" + tail
    assert _raises(explain.explain_topk, Shard(), None, [[1]]) == \
        "explanations need the liked rows and the result rows on one device" + tail
    assert _raises(explain.liked_contrib, Shard(), None, [[1]]) == \
        "explanations need the liked rows and the result rows on one device" + tail
    assert _raises(diversify.diversify_topk, Shard(), None, None, 5) == \
        "diversification needs the pool rows on one device" + tail
    assert _raises(interests.cluster_liked, Shard(), [[1]]) == \
        "multi-interest search needs the liked rows on one device" + tail


@pytest.mark.parametrize("weighted", [False, True])
def test_liked_batch_on_a_catalog_of_unknown_dtype_is_einval(weighted):
    """An ebt_catalog is caller-filled and the drivers' own checks never look at its dtype: a
    liked batch on dtype 7 must stop at the liked sum's operand check, EBT_EINVAL under the
    sum's entry name, before anything is launched (no dtype means no kernel that could read the
    rows at their width). EBT_FLAG_LIKED_CHECKED keeps the host checks, which copy from the
    device, out of the way; the fake pointers are never dereferenced."""
    import ctypes
    from robot_ebert_amd import _lib
    lib = _lib.load()
    fake = 1 << 30
    d = 64
    cat = _lib.EbtCatalog(data=fake, dtype=_lib.EBT_F32, d=d, n=1000, ld=d, row_offset=0,
                          gnorm64=fake, inv32=fake, image=fake, cscale=None,
                          img_dtype=_lib.EBT_F16, ld_img=d, d_pad=d, native=0, u_cat=2.0 ** -11)
    opt = _lib.EbtOptions(kprime=0, flags=8, chunk_rows=0)        # EBT_FLAG_LIKED_CHECKED
    B, k = 2, 5
    need = lib.ebt_workspace_bytes(ctypes.byref(cat), B, k, ctypes.byref(opt))
    assert need > 0
    cat.dtype = 7
    rc = lib.ebt_cosine_topk_weighted(ctypes.byref(cat), None, 0, B, 0, fake, fake, k, None, None,
                                      ctypes.byref(opt), fake, need, fake, fake, None, None, None,
                                      fake if weighted else None)
    assert rc == -1
    name = "ebt_query_liked_wsum" if weighted else "ebt_query_liked_sum"
    assert lib.ebt_last_error().decode() == f"{name}: bad arguments"
