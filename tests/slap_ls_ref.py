"""A numpy restatement of co_slap_local_search (include/co_env.h states it), in two forms:
``local_search_brute`` evaluates every candidate as F(s') - F(s) on the whole objective,
``local_search`` uses the QAP table.  Everything is int64, so both are exact."""
import numpy as np

SCALE = float(1 << 20)


def dist_from_locs(locs):
    """The f32 matrix co_distance_matrix writes: sqrt(dx*dx + dy*dy), no FMA."""
    locs = np.asarray(locs, dtype=np.float32)
    d = locs[None, :, :] - locs[:, None, :]
    return np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1], dtype=np.float32)


def quantise(D):
    return np.rint(np.asarray(D, dtype=np.float32).astype(np.float64) * SCALE).astype(np.int64)


def flows(picklist, p):
    """W[a][c]: how often product a is followed (cyclically, within an order) by c != a."""
    pl = np.asarray(picklist, dtype=np.int64)
    nxt = np.roll(pl, -1, axis=1)
    w = np.zeros((p, p), dtype=np.int64)
    keep = pl != nxt
    np.add.at(w, (pl[keep], nxt[keep]), 1)
    return w


def objective(w, q, s):
    return int((w * q[np.ix_(s, s)]).sum())


def check(D, picklist, s, locs=None):
    """The row check: None when the row is searched, else the status bits it sets."""
    s = np.asarray(s, dtype=np.int64)
    L = len(D)
    bits = 0
    if ((s < 0) | (s >= L)).any() or len(set(s.tolist())) != len(s):
        bits |= 1
    if locs is not None:
        if not (np.abs(np.asarray(locs, dtype=np.float32)) <= 2.0 ** 18).all():
            bits |= 1
    elif not ((np.asarray(D) >= 0) & (np.asarray(D) <= 2.0 ** 20)).all():
        bits |= 1
    pl = np.asarray(picklist)
    if ((pl < 0) | (pl >= len(s))).any():
        bits |= 8
    return bits or None


def _pick(cands):
    """cands: (change, kind, p, x).  The applied one and whether its change is shared."""
    best = min(cands, default=None)
    if best is None or best[0] >= 0:
        return None, False
    return best, sum(c[0] == best[0] for c in cands) > 1


def local_search_brute(D, picklist, s, max_iterations=1000, locs=None):
    """(row, sweeps, cost, tied sweeps), or (None, 0, -1, 0) for a row that fails its check."""
    s = np.array(s, dtype=np.int64)
    if check(D, picklist, s, locs) is not None:
        return None, 0, -1, 0
    p, L = len(s), len(D)
    w, q = flows(picklist, p), quantise(D)
    it = tied = 0
    while it < max_iterations:
        it += 1
        f0 = objective(w, q, s)
        used = set(s.tolist())
        cands = []
        for a in range(p):
            for x in range(1, L):
                if x not in used:
                    t = s.copy()
                    t[a] = x
                    cands.append((objective(w, q, t) - f0, 0, a, x))
        for a in range(p):
            for c in range(a + 1, p):
                t = s.copy()
                t[a], t[c] = s[c], s[a]
                cands.append((objective(w, q, t) - f0, 1, a, c))
        best, shared = _pick(cands)
        if best is None:
            break
        tied += shared
        _, kind, a, x = best
        if kind:
            s[a], s[x] = s[x], s[a]
        else:
            s[a] = x
    return s, it, objective(w, q, s), tied


def local_search(D, picklist, s, max_iterations=1000, locs=None):
    """The table form: C[p][l] = sum_r W[p][r] Q[l][s_r] + W[r][p] Q[s_r][l]; a move changes
    F by C[p][x] - C[p][s_p], a swap by two such differences and the pair's own term."""
    s = np.array(s, dtype=np.int64)
    if check(D, picklist, s, locs) is not None:
        return None, 0, -1, 0
    p, L = len(s), len(D)
    w, q = flows(picklist, p), quantise(D)
    ws = w + w.T
    diag = np.diagonal(q)
    it = tied = 0
    while it < max_iterations:
        it += 1
        C = w @ q[:, s].T + w.T @ q[s, :]  # [P, L]
        own = C[np.arange(p), s]
        free = np.ones(L, dtype=bool)
        free[s] = False
        free[0] = False
        mv = np.where(free[None, :], C - own[:, None], 1)  # 1: not a candidate
        cs = C[:, s]  # cs[a, c] = C[a][s_c]
        qs = q[np.ix_(s, s)]
        sw = (cs - own[:, None]) + (cs.T - own[None, :]) \
            + ws * (qs + qs.T - diag[s][:, None] - diag[s][None, :])
        sw = np.where(np.triu(np.ones((p, p), dtype=bool), 1), sw, 1)
        m0, m1 = int(mv.min()), int(sw.min())
        best = min(m0, m1)
        if best >= 0:
            break
        tied += int((mv == best).sum() + (sw == best).sum()) > 1
        if m0 <= m1:
            a, x = np.unravel_index(np.argmax(mv == best), mv.shape)  # first in (p, x) order
            s[a] = x
        else:
            a, c = np.unravel_index(np.argmax(sw == best), sw.shape)
            s[a], s[c] = s[c], s[a]
    return s, it, objective(w, q, s), tied
