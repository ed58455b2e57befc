"""numpy f32 restatement of the best-improvement 2-opt that ``co_tsp_two_opt`` reproduces
(written from the semantics in include/co_env.h): per sweep every move (i, j),
1 <= i < j <= n-1, is scored in f32 left to right,

    change = ((D[t[i-1], t[j]] + D[t[i], t[(j+1) % n]]) - D[t[i-1], t[i]]) - D[t[j], t[(j+1) % n]]

the smallest change wins (equal values: the lexicographically first (i, j), from a strict
``<`` against delta = 0), t[i..j] is reversed when it is below -1e-6 (compared in double),
and the search ends with the first sweep that does not improve or after max_iterations.

``two_opt`` is the per-sweep vectorised form (row-major flattening + ``np.argmin``, which
returns the first minimum); ``two_opt_scalar`` is the plain double loop; both return
``(tour, sweeps, n_tied_sweeps)`` where a tied sweep is an applied sweep whose minimum was
reached by more than one move."""
import numpy as np


def dist_from_locs(locs):
    """f32 ``sqrt(dx*dx + dy*dy)`` between all pairs of ``locs [n, 2]`` (each step rounded
    to f32, no fused multiply-add)."""
    locs = np.asarray(locs, dtype=np.float32)
    dx = locs[None, :, 0] - locs[:, None, 0]
    dy = locs[None, :, 1] - locs[:, None, 1]
    return np.sqrt(dx * dx + dy * dy, dtype=np.float32)


def two_opt_scalar(D, tour, max_iterations):
    D = np.asarray(D, dtype=np.float32)
    tour = [int(v) for v in tour]
    n = len(tour)
    min_change, it, tied = -1.0, 0, 0
    while min_change < -1e-6 and it < max_iterations:
        p = q = 0
        delta = np.float32(0.0)
        hits = 0
        for i in range(1, n - 1):
            for j in range(i + 1, n):
                prev, nxt = tour[i - 1], tour[(j + 1) % n]
                if prev == tour[j] or nxt == tour[i]:
                    continue
                change = np.float32(np.float32(np.float32(D[prev, tour[j]] + D[tour[i], nxt])
                                               - D[prev, tour[i]]) - D[tour[j], nxt])
                if change < delta:
                    p, q, delta, hits = i, j, change, 1
                elif change == delta:
                    hits += 1
        if float(delta) < -1e-6:
            tour[p:q + 1] = tour[p:q + 1][::-1]
            min_change = float(delta)
            tied += hits > 1
        else:
            min_change = 0.0
        it += 1
    return np.asarray(tour, dtype=np.int64), it, tied


def two_opt(D, tour, max_iterations):
    D = np.asarray(D, dtype=np.float32)
    tour = np.array(tour, dtype=np.int64)
    n = len(tour)
    if n < 3:
        return tour, (1 if max_iterations > 0 else 0), 0
    ii, jj = np.triu_indices(n, 1)  # every i < j, row-major: i ascending, then j
    ii, jj = ii[ii >= 1], jj[ii >= 1]
    jn = (jj + 1) % n
    min_change, it, tied = -1.0, 0, 0
    while min_change < -1e-6 and it < max_iterations:
        prev, nxt, ti, tj = tour[ii - 1], tour[jn], tour[ii], tour[jj]
        change = ((D[prev, tj] + D[ti, nxt]) - D[prev, ti]) - D[tj, nxt]
        assert change.dtype == np.float32
        skip = (prev == tj) | (nxt == ti)
        change = np.where(skip | ~(change < 0), np.float32(0.0), change)
        k = int(np.argmin(change))
        delta = change[k]
        if float(delta) < -1e-6:
            tied += int((change == delta).sum()) > 1
            p, q = int(ii[k]), int(jj[k])
            tour[p:q + 1] = tour[p:q + 1][::-1].copy()
            min_change = float(delta)
        else:
            min_change = 0.0
        it += 1
    return tour, it, tied
