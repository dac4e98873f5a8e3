"""Test-side numpy forms of the two multi-interest pseudo-codes (include/ebert.h 0.11.0,
ebt_interest_cluster and ebt_interest_interleave), one float64 operation at a time: the j loops
are Python loops, vectorised over i. S is one query's [p, p] similarity matrix (the oracle's, or
the device's own: bitwise symmetric), rows its [p] list with -1 on empty slots.

`planted` draws liked lists with known groups."""
import numpy as np

ITERS = 16    # EBT_INTEREST_ITERS


def _arg_best(vals, cand, smallest=False):
    """The candidate position with the largest (smallest) value, the lowest position among equal
    values (-0 equals +0); a NaN ranks last; (position, gap to the runner-up or inf)."""
    pos = np.flatnonzero(cand)
    v = vals[pos]
    v = -v if smallest else v
    ok = ~np.isnan(v)
    if not ok.any():
        return int(pos[0]), np.inf
    top = v[ok].max()
    at = int(pos[np.flatnonzero(ok & (v == top))[0]])
    rest = np.sort(v[ok])[::-1]
    return at, (rest[0] - rest[1] if len(rest) > 1 else np.inf)


def _pass(S, label, valid, c):
    """PASS(label): (n [c], mean [p, c]; columns of empty clusters are NaN)."""
    p = len(label)
    n = np.array([int((label == m).sum()) for m in range(c)])
    acc = np.zeros((p, c))
    for j in np.flatnonzero(valid):
        acc[:, label[j]] = acc[:, label[j]] + S[:, j]
    mean = np.full((p, c), np.nan)
    for m in range(c):
        if n[m] > 0:
            mean[:, m] = acc[:, m] / np.float64(n[m])
    return n, mean


def _assign(vals, live):
    """Per row: the arg max over the live columns by (value desc, column asc), and the gap between
    the two largest live values (inf with one live column)."""
    best = np.full(vals.shape[0], -1)
    bv = np.zeros(vals.shape[0])
    for m in np.flatnonzero(live):
        with np.errstate(invalid="ignore"):
            take = (best < 0) | (vals[:, m] > bv)
        bv = np.where(take, vals[:, m], bv)
        best = np.where(take, m, best)
    lv = np.sort(vals[:, live], axis=1)
    gap = lv[:, -1] - lv[:, -2] if lv.shape[1] > 1 else np.full(vals.shape[0], np.inf)
    return best, gap


def cluster_ref(S, rows, c, with_gap=False):
    """(label int32 [p], size int32 [c], medoid int32 [c], iters); with_gap: also the smallest
    gap between the winner and the runner-up over every decision taken (the seed choices, every
    assignment of every pass, the medoids)."""
    S, rows = np.asarray(S, np.float64), np.asarray(rows)
    p = len(rows)
    valid = rows >= 0
    L = int(valid.sum())
    label = np.full(p, -1, dtype=np.int32)
    size, medoid = np.zeros(c, dtype=np.int32), np.full(c, -1, dtype=np.int32)
    gap = np.inf
    if L == 0:
        return (label, size, medoid, 0, gap) if with_gap else (label, size, medoid, 0)
    c_eff = min(c, L)
    idx = np.flatnonzero(valid)
    with np.errstate(invalid="ignore"):
        tot = np.zeros(p)
        for j in idx:
            tot = tot + S[:, j]
        seeds = []
        s0, g = _arg_best(tot, valid)
        gap = min(gap, g)
        seeds.append(s0)
        near = S[s0].copy()
        for m in range(1, c_eff):
            cand = valid.copy()
            cand[seeds] = False
            sm, g = _arg_best(near, cand, smallest=True)
            gap = min(gap, g)
            seeds.append(sm)
            near = np.where(S[sm] > near, S[sm], near)
        first, g = _assign(S[seeds].T, np.ones(c_eff, dtype=bool))
        free = valid.copy()
        free[seeds] = False
        if free.any():
            gap = min(gap, g[free].min())
        lab = np.where(valid, first, -1)
        for m, sm in enumerate(seeds):
            lab[sm] = m
        iters = 0
        capped = True
        for it in range(1, ITERS + 1):
            n, mean = _pass(S, lab, valid, c_eff)
            new, g = _assign(mean, n > 0)
            gap = min(gap, g[valid].min())
            new = np.where(valid, new, -1)
            iters = it
            if np.array_equal(new, lab):
                capped = False
                break
            lab = new
        if capped:
            n, mean = _pass(S, lab, valid, c_eff)
        med = np.full(c_eff, -1)
        low = np.full(c_eff, p)
        for m in range(c_eff):
            if n[m] > 0:
                members = lab == m
                med[m], g = _arg_best(mean[:, m], members)
                gap = min(gap, g)
                low[m] = np.flatnonzero(members)[0]
    order = sorted((m for m in range(c_eff) if n[m] > 0), key=lambda m: (-n[m], low[m]))
    for new_m, m in enumerate(order):
        label[lab == m] = new_m
        size[new_m] = n[m]
        medoid[new_m] = med[m]
    return (label, size, medoid, iters, gap) if with_gap else (label, size, medoid, iters)


def interleave_ref(size, list_rows, list_scores, k):
    """(rows int64 [k], scores float64 [k], cluster int32 [k], pos int32 [k]) of one query:
    size [c], list_rows / list_scores [c, k]; -1 / NaN / -1 / -1 past the stop."""
    size, list_rows = np.asarray(size), np.asarray(list_rows)
    list_scores = np.asarray(list_scores, np.float64)
    c = len(size)
    out_rows = np.full(k, -1, dtype=np.int64)
    out_scores = np.full(k, np.nan)
    out_cluster, out_pos = np.full(k, -1, dtype=np.int32), np.full(k, -1, dtype=np.int32)
    taken, nxt = [0] * c, [0] * c
    emitted = set()
    for t in range(k):
        for m in range(c):
            while nxt[m] < k and (list_rows[m, nxt[m]] < 0 or int(list_rows[m, nxt[m]]) in emitted):
                nxt[m] += 1
        best = -1
        for m in range(c):
            if size[m] <= 0 or nxt[m] >= k:
                continue
            if best < 0 or int(size[m]) * (taken[best] + 1) > int(size[best]) * (taken[m] + 1):
                best = m
        if best < 0:
            break
        q = nxt[best]
        out_rows[t], out_scores[t] = list_rows[best, q], list_scores[best, q]
        out_cluster[t], out_pos[t] = best, q
        emitted.add(int(list_rows[best, q]))
        taken[best] += 1
        nxt[best] += 1
    return out_rows, out_scores, out_cluster, out_pos


def dhondt_seats(size, k):
    """Seats per cluster after k rounds of the highest-averages rule when no list runs out."""
    taken = [0] * len(size)
    for _ in range(k):
        live = [m for m in range(len(size)) if size[m] > 0]
        if not live:
            break
        best = live[0]
        for m in live[1:]:
            if int(size[m]) * (taken[best] + 1) > int(size[best]) * (taken[m] + 1):
                best = m
        taken[best] += 1
    return taken


def planted(seed, g, d, L, noise):
    """(x float64 [L, d], group [L]): g Gaussian centres plus noise * N(0, 1); row i belongs to
    group i % g."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((g, d))
    group = np.arange(L) % g
    return centres[group] + noise * rng.standard_normal((L, d)), group
