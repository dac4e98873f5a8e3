"""Test-side numpy form of the greedy MMR selection (include/ebert.h 0.10.0, ebt_mmr_select):
the header's pseudo-code, one float64 operation at a time. S is one query's [p, p] similarity
matrix (the oracle's, or the device's own), rel / rows its [p] pool."""
import numpy as np


def mmr_ref(S, rel, rows, k, lam):
    """(pos int32 [k], rows int64 [k], rel float64 [k], mmr float64 [k]); -1 / -1 / NaN / NaN
    past the candidates."""
    S, rel, rows = np.asarray(S, np.float64), np.asarray(rel, np.float64), np.asarray(rows)
    lam = np.float64(lam)
    oml = np.float64(1.0) - lam
    alive = (rows >= 0) & ~np.isnan(rel)
    pen = np.zeros(len(rel))
    pos = np.full(k, -1, dtype=np.int32)
    out_rows = np.full(k, -1, dtype=np.int64)
    out_rel, out_mmr = np.full(k, np.nan), np.full(k, np.nan)
    for t in range(k):
        with np.errstate(invalid="ignore"):
            v = (lam * rel) - (oml * pen)
        ok = alive & ~np.isnan(v)
        if not ok.any():
            break
        s = int(np.flatnonzero(ok & (v == v[ok].max()))[0])      # (v desc, position asc)
        pos[t], out_rows[t], out_rel[t], out_mmr[t] = s, rows[s], rel[s], v[s]
        alive[s] = False
        with np.errstate(invalid="ignore"):
            pen = S[s].copy() if t == 0 else np.where(S[s] > pen, S[s], pen)
    return pos, out_rows, out_rel, out_mmr
