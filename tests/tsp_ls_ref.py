"""numpy f32 restatement of the 2-opt + Or-opt descent of ``co_tsp_local_search`` (written
from the semantics in include/co_env.h).

Or-opt move (L, i, k, rev): the segment t[i..i+L-1], L in {1, 2, 3}, 1 <= i, i+L-1 <= n-1,
is taken out and reinserted (reversed if rev; L = 1: rev = 0 only) directly after c = t[k],
0 <= k <= n-1, k not in [i-1, i+L-1].  With a = t[i-1], s1 = t[i], s2 = t[i+L-1],
b = t[(i+L) % n], d = t[(k+1) % n], (x, y) = (s1, s2) or, reversed, (s2, s1):

    change = ((((D[a,b] + D[c,x]) + D[y,d]) - D[a,s1]) - D[s2,b]) - D[c,d]

in f32, left to right.  A sweep: with TWO_OPT the best 2-opt move (two_opt_ref's sweep) is
applied if below -1e-6; if none was applied and OR_OPT is enabled the best Or-opt move --
equal values: the first in the order L, i, k, rev, a strict ``<`` from 0 -- is applied if
below -1e-6 (compared in double).  The search ends with the first sweep that applies
nothing or after max_iterations sweeps.

``local_search_scalar`` is the plain-loop form (the readable definition), ``local_search``
the per-sweep vectorised form (candidates flattened in enumeration order + ``np.argmin``,
which returns the first minimum).  Both return ``(tour, sweeps, (n2opt, noropt),
tied_sweeps)``: a tied sweep is an applied move whose minimum more than one candidate of
its neighbourhood reached."""
import functools

import numpy as np

from two_opt_ref import two_opt, two_opt_scalar

TWO_OPT, OR_OPT = 1, 2
F = np.float32


def or_change(D, t, L, i, k, rev):
    """The header's expression for one candidate of tour ``t`` (a list of ints)."""
    n = len(t)
    a, s1, s2, b = t[i - 1], t[i], t[i + L - 1], t[(i + L) % n]
    c, d = t[k], t[(k + 1) % n]
    x, y = (s2, s1) if rev else (s1, s2)
    v = F(D[a, b] + D[c, x])
    v = F(v + D[y, d])
    v = F(v - D[a, s1])
    v = F(v - D[s2, b])
    return F(v - D[c, d])


def or_candidates(n):
    """Every (L, i, k, rev) of an n-position tour, in the enumeration order."""
    out = []
    for L in (1, 2, 3):
        if n - L - 1 < 1:
            continue
        for i in range(1, n - L + 1):
            for k in range(n):
                if i - 1 <= k <= i + L - 1:
                    continue
                for rev in ((0, 1) if L > 1 else (0,)):
                    out.append((L, i, k, rev))
    return out


def or_scan_scalar(D, t):
    """(best change f32, its (L, i, k, rev) or None, number of candidates equal to it)."""
    best, move, hits = F(0.0), None, 0
    for L, i, k, rev in or_candidates(len(t)):
        ch = or_change(D, t, L, i, k, rev)
        if ch < best:
            best, move, hits = ch, (L, i, k, rev), 1
        elif ch == best:
            hits += 1
    return best, move, hits


def apply_or(t, L, i, k, rev):
    """Remove t[i..i+L-1] and reinsert it (reversed if rev) directly after node t[k]."""
    t = list(t)
    c = t[k]
    seg = t[i:i + L]
    if rev:
        seg = seg[::-1]
    rest = t[:i] + t[i + L:]
    at = rest.index(c)
    return rest[:at + 1] + seg + rest[at + 1:]


def _two_opt_step(fn, D, t):
    """One 2-opt sweep through two_opt_ref: (tour, applied, tied)."""
    r, _, tied = fn(D, t, 1)
    r = [int(v) for v in r]
    return r, r != list(t), tied


def local_search_scalar(D, tour, operators=TWO_OPT | OR_OPT, max_iterations=1000):
    D = np.asarray(D, dtype=F)
    t = [int(v) for v in tour]
    it = n2 = nor = tied = 0
    while it < max_iterations:
        it += 1
        if operators & TWO_OPT:
            r, applied, k = _two_opt_step(two_opt_scalar, D, t)
            if applied:
                t, n2, tied = r, n2 + 1, tied + k
                continue
        if not operators & OR_OPT:
            break
        best, move, hits = or_scan_scalar(D, t)
        if not float(best) < -1e-6:
            break
        t = apply_or(t, *move)
        nor += 1
        tied += hits > 1
    return np.asarray(t, dtype=np.int64), it, (n2, nor), tied


def _or_index(n, L):
    """The candidates of one L in the enumeration order (i, then k, then rev), as int32
    arrays: (i, e = i+L-1, position of b, k, position of d, rev)."""
    i, k = np.meshgrid(np.arange(1, n - L + 1, dtype=np.int32), np.arange(n, dtype=np.int32),
                       indexing="ij")
    keep = (k < i - 1) | (k > i + L - 1)
    i, k = i[keep], k[keep]
    nrev = 2 if L > 1 else 1
    i, k = np.repeat(i, nrev), np.repeat(k, nrev)
    rev = np.tile(np.arange(nrev, dtype=np.int32), len(i) // nrev).astype(bool)
    e = i + (L - 1)
    return i, e, (e + 1) % n, k, (k + 1) % n, rev


_or_index_cached = functools.lru_cache(maxsize=None)(_or_index)


def or_scan(D, t):
    """``or_scan_scalar`` on arrays: per L the first minimum (``np.argmin``), the Ls joined
    by the same strict ``<``."""
    t = np.asarray(t, dtype=np.int64)
    n = len(t)
    best, move, hits = F(0.0), None, 0
    for L in (1, 2, 3):
        if n - L - 1 < 1:
            continue
        i, e, bpos, k, dpos, rev = (_or_index_cached if n <= 256 else _or_index)(n, L)
        a, s1, s2, b, cc, d = t[i - 1], t[i], t[e], t[bpos], t[k], t[dpos]
        x, y = np.where(rev, s2, s1), np.where(rev, s1, s2)
        ch = ((((D[a, b] + D[cc, x]) + D[y, d]) - D[a, s1]) - D[s2, b]) - D[cc, d]
        assert ch.dtype == F
        m = int(np.argmin(ch))
        if ch[m] < best:
            best, move = ch[m], (L, int(i[m]), int(k[m]), int(rev[m]))
            hits = int((ch == best).sum())
        elif ch[m] == best and move is not None:
            hits += int((ch == best).sum())
    return best, move, hits


def local_search(D, tour, operators=TWO_OPT | OR_OPT, max_iterations=1000):
    D = np.asarray(D, dtype=F)
    t = [int(v) for v in tour]
    it = n2 = nor = tied = 0
    while it < max_iterations:
        it += 1
        if operators & TWO_OPT:
            r, applied, k = _two_opt_step(two_opt, D, t)
            if applied:
                t, n2, tied = r, n2 + 1, tied + k
                continue
        if not operators & OR_OPT:
            break
        best, move, hits = or_scan(D, t)
        if not float(best) < -1e-6:
            break
        t = apply_or(t, *move)
        nor += 1
        tied += hits > 1
    return np.asarray(t, dtype=np.int64), it, (n2, nor), tied
