"""numpy restatement of the CVRP giant-tour local search that ``co_cvrp_local_search``
reproduces, written from the semantics in include/co_env.h.

The row becomes a cyclic giant tour g (g[0] = 0 fixed, routes separated by zeros, length m
fixed).  A sweep scores, in f32 and left to right as bracketed,

  2-opt (i, j), 1 <= i < j <= m-1 (reverse g[i..j]), p, x, y, n = g[i-1], g[i], g[j], g[j+1]:
      change = ((D[p,y] + D[x,n]) - D[p,x]) - D[y,n]
  relocate (i, j), g[i] != 0, j != i, j != i-1 (c = g[i] goes between positions j and j+1),
  p, n, a, b = g[i-1], g[i+1], g[j], g[j+1]:
      change = ((D[a,c] + D[c,b]) - D[a,b]) + ((D[p,n] - D[p,c]) - D[c,n])

keeps the admissible ones (integer loads q(x) = rint(x * 2^40) against q(capacity) + 2^20),
takes the smallest change < 0 (ties: 2-opt first, then the smaller i, then the smaller j),
applies it when it is below -1e-6 in double, and stops with the first sweep that applies
nothing or after max_iterations sweeps.

``local_search_scalar`` is the plain double loop with the loads summed directly along the
tour; ``local_search`` is the per-sweep vectorised form (prefix loads, candidates flattened
in tie order, ``np.argmin`` = first minimum).  Both return ``(row, sweeps, tied_sweeps)``
with ``row`` None for a row that fails the row check (the entry then copies its input)."""
import numpy as np

SCALE = float(2 ** 40)
SLACK = 2 ** 20
LIMIT = 4096.0


def dist_from_locs(locs):
    """f32 ``sqrt(dx*dx + dy*dy)`` between all pairs of ``locs [n, 2]`` (no FMA)."""
    locs = np.asarray(locs, dtype=np.float32)
    dx = locs[None, :, 0] - locs[:, None, 0]
    dy = locs[None, :, 1] - locs[:, None, 1]
    return np.sqrt(dx * dx + dy * dy, dtype=np.float32)


def quantise(x):
    return np.rint(np.asarray(x, dtype=np.float32).astype(np.float64) * SCALE).astype(np.int64)


def giant_tour(row, n, demand, capacity):
    """The row check and the giant tour; None for an invalid row."""
    row = [int(v) for v in row]
    demand = np.asarray(demand, dtype=np.float32)
    capacity = np.float32(capacity)
    if any(v < 0 or v > n for v in row):
        return None
    if sorted(v for v in row if v) != list(range(1, n + 1)):
        return None
    vals = np.append(demand, capacity)
    if not (np.isfinite(vals).all() and (vals >= 0).all() and (vals <= LIMIT).all()):
        return None
    g = [0]
    for v in row:
        if v or g[-1]:
            g.append(v)
    if len(g) > 1 and g[-1] == 0:
        g.pop()
    return g


def emit(g, width):
    out = []
    for v in g[1:]:
        if v or (out and out[-1]):
            out.append(v)
    if out and out[-1] == 0:
        out.pop()
    assert len(out) <= width
    return np.asarray(out + [0] * (width - len(out)), dtype=np.int64)


def _apply(g, kind, i, j):
    if kind == 0:
        g[i:j + 1] = g[i:j + 1][::-1]
    else:
        c = g[i]
        if j > i:
            g[i:j] = g[i + 1:j + 1]
            g[j] = c
        else:
            g[j + 2:i + 1] = g[j + 1:i]
            g[j + 1] = c


def local_search_scalar(D, demand, capacity, row, max_iterations):
    D = np.asarray(D, dtype=np.float32)
    n = len(demand)
    g = giant_tour(row, n, demand, capacity)
    if g is None:
        return None, 0, 0
    q = [0] + [int(v) for v in quantise(demand)]
    cap_q = int(quantise(capacity)) + SLACK
    m = len(g)
    f32 = np.float32

    def back(k):  # customers of k's route at positions <= k
        s = 0
        while g[k] != 0:
            s += q[g[k]]
            k -= 1
        return s

    def fwd(k):  # customers from position k to the end of that route
        s = 0
        while k < m and g[k] != 0:
            s += q[g[k]]
            k += 1
        return s

    it = tied = 0
    while it < min(max_iterations, 2 ** 31 - 1):
        it += 1
        best, move, hits = f32(0.0), None, 0

        def offer(change, mv):
            nonlocal best, move, hits
            if change < best:
                best, move, hits = change, mv, 1
            elif change == best:
                hits += 1

        for i in range(1, m - 1):
            for j in range(i + 1, m):
                p, x, y, nx = g[i - 1], g[i], g[j], g[(j + 1) % m]
                change = f32(f32(f32(D[p, y] + D[x, nx]) - D[p, x]) - D[y, nx])
                if 0 in g[i:j + 1]:
                    zeros = [k for k in range(i, j + 1) if g[k] == 0]
                    left = back(i - 1) + sum(q[g[k]] for k in range(zeros[-1] + 1, j + 1))
                    right = sum(q[g[k]] for k in range(i, zeros[0])) + fwd(j + 1)
                    if left > cap_q or right > cap_q:
                        continue
                offer(change, (0, i, j))
        for i in range(1, m):
            c = g[i]
            if c == 0:
                continue
            for j in range(m):
                if j == i or j == i - 1:
                    continue
                p, nx, a, b = g[i - 1], g[(i + 1) % m], g[j], g[(j + 1) % m]
                change = f32(f32(f32(D[a, c] + D[c, b]) - D[a, b])
                             + f32(f32(D[p, nx] - D[p, c]) - D[c, nx]))
                if g[:j + 1].count(0) != g[:i + 1].count(0):
                    if back(j) + fwd(j + 1) + q[c] > cap_q:
                        continue
                offer(change, (1, i, j))
        if move is None or not float(best) < -1e-6:
            break
        tied += hits > 1
        _apply(g, *move)
    return emit(g, len(row)), it, tied


def local_search(D, demand, capacity, row, max_iterations):
    D = np.asarray(D, dtype=np.float32)
    n = len(demand)
    g = giant_tour(row, n, demand, capacity)
    if g is None:
        return None, 0, 0
    g = np.asarray(g, dtype=np.int64)
    q = np.concatenate([[0], quantise(demand)]).astype(np.int64)
    cap_q = int(quantise(capacity)) + SLACK
    m = len(g)
    pos = np.arange(m)
    ii, jj = np.triu_indices(m, 1)
    ii, jj = ii[ii >= 1], jj[ii >= 1]
    ri, rj = np.meshgrid(np.arange(1, m), pos, indexing="ij")
    ri, rj = ri.ravel(), rj.ravel()
    zero = np.float32(0.0)
    it = tied = 0
    while it < min(max_iterations, 2 ** 31 - 1):
        it += 1
        ge = np.append(g, 0)  # position m is position 0
        isz = ge == 0
        W = np.cumsum(q[ge])  # prefix loads, W[m] = W[m-1]
        Z = np.cumsum(g == 0)
        pz = np.maximum.accumulate(np.where(isz, np.arange(m + 1), 0))  # last zero <= k
        nz = np.minimum.accumulate(np.where(isz, np.arange(m + 1), m)[::-1])[::-1]  # first >= k
        # 2-opt
        p, x, y, nx = g[ii - 1], g[ii], g[jj], ge[jj + 1]
        ch2 = ((D[p, y] + D[x, nx]) - D[p, x]) - D[y, nx]
        left = (W[ii - 1] - W[pz[ii - 1]]) + (W[jj] - W[pz[jj]])
        right = (W[nz[ii]] - W[ii - 1]) + (W[nz[jj + 1]] - W[jj])
        ok2 = (Z[jj] == Z[ii - 1]) | ((left <= cap_q) & (right <= cap_q))
        # relocate
        c, p, nx, a, b = g[ri], g[ri - 1], ge[ri + 1], g[rj], ge[rj + 1]
        chr_ = ((D[a, c] + D[c, b]) - D[a, b]) + ((D[p, nx] - D[p, c]) - D[c, nx])
        target = (W[nz[rj + 1]] - W[pz[rj]]) + q[c]
        okr = (c != 0) & (rj != ri) & (rj != ri - 1) & ((Z[rj] == Z[ri]) | (target <= cap_q))
        change = np.concatenate([np.where(ok2 & (ch2 < 0), ch2, zero),
                                 np.where(okr & (chr_ < 0), chr_, zero)])
        assert change.dtype == np.float32
        if change.size == 0:
            break
        k = int(np.argmin(change))
        delta = change[k]
        if not float(delta) < -1e-6:
            break
        tied += int((change == delta).sum()) > 1
        gl = [int(v) for v in g]
        if k < len(ii):
            _apply(gl, 0, int(ii[k]), int(jj[k]))
        else:
            _apply(gl, 1, int(ri[k - len(ii)]), int(rj[k - len(ii)]))
        g = np.asarray(gl, dtype=np.int64)
    return emit([int(v) for v in g], len(row)), it, tied
