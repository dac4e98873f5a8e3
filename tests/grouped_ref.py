"""numpy restatements for the grouped top-k (ebert.h 0.12.0), test infrastructure only.

``grouped_ref``: per group, the float64 scores of oracle/restatement.py restricted to the rows the
group's mask allows minus the query's excluded rows, stable-sorted by (score descending, row
ascending). ``select_ref``: the contract of ebt_select_topk_grouped on one f32 score row.
"""
import numpy as np

from oracle import restatement as R


def scores64(catalog, queries=None, liked=None, liked_weights=None):
    """float64 [B, n]: cosine of dense queries, the mean cosine over liked rows (lib.py:51-52),
    or sum_l w_l cos(x_l, .) / sum_l |w_l| with liked_weights."""
    c = np.asarray(catalog, dtype=np.float64)
    if queries is not None:
        return R.cosine_similarity(np.asarray(queries, dtype=np.float64), c)
    out = np.empty((len(liked), c.shape[0]))
    for b, rows in enumerate(liked):
        S = R.cosine_similarity(c[np.asarray(rows, dtype=np.int64)], c)
        if liked_weights is None:
            out[b] = S.mean(axis=0)
        else:
            w = np.asarray(liked_weights[b], dtype=np.float64)
            out[b] = (w[:, None] * S).sum(axis=0) / np.abs(w).sum()
    return out


def grouped_ref(S, flags, groups, k, exclude=None):
    """(scores f64 [B, G, k] NaN-padded, rows i64 [B, G, k] -1-padded).

    S: float64 [B, n]; flags: bool [n_masks, n]; groups: mask ids (an id >= n_masks is an empty
    group, a negative one every row); exclude: per-query row lists or None."""
    S = np.asarray(S, dtype=np.float64)
    B, n = S.shape
    G = len(groups)
    out_s = np.full((B, G, k), np.nan)
    out_r = np.full((B, G, k), -1, dtype=np.int64)
    for b in range(B):
        ok_b = np.ones(n, dtype=bool)
        if exclude is not None and len(exclude[b]):
            ok_b[np.asarray(list(exclude[b]), dtype=np.int64)] = False
        for gi, g in enumerate(groups):
            if g >= len(flags):
                continue
            ok = ok_b if g < 0 else ok_b & np.asarray(flags[g], dtype=bool)[:n]
            rows = np.nonzero(ok)[0]                       # ascending
            order = np.argsort(-S[b, rows], kind="stable")[:k]   # ties keep the lower row
            out_s[b, gi, :order.size] = S[b, rows][order]
            out_r[b, gi, :order.size] = rows[order]
    return out_s, out_r


def select_ref(vals, n, col_begin, flags, groups, kprime, segs):
    """ebt_select_topk_grouped on vals f32 [B, ld]: (out_vals f32, out_idx i64), both
    [G, B, segs * kprime]; flags: bool [n_masks, rows] over GLOBAL rows."""
    B = vals.shape[0]
    G = len(groups)
    seg_len = (-(-max(n, 1) // segs) + 3) // 4 * 4
    out_v = np.full((G, B, segs * kprime), -np.inf, dtype=np.float32)
    out_i = np.full((G, B, segs * kprime), -1, dtype=np.int64)
    for gi, g in enumerate(groups):
        if g >= len(flags):
            continue
        allow = np.ones(n, bool) if g < 0 else np.asarray(flags[g][col_begin:col_begin + n], bool)
        for b in range(B):
            v = vals[b, :n]
            ok = allow & ~np.isnan(v) & (v != -np.inf)
            for s in range(segs):
                lo, hi = s * seg_len, min((s + 1) * seg_len, n)
                if lo >= hi:
                    continue
                idx = lo + np.nonzero(ok[lo:hi])[0]
                order = np.argsort(-v[idx].astype(np.float64), kind="stable")[:kprime]
                out_v[gi, b, s * kprime:s * kprime + order.size] = v[idx][order]
                out_i[gi, b, s * kprime:s * kprime + order.size] = col_begin + idx[order]
    return out_v, out_i
