"""Inputs and restatement results shared by the CVRP local-search tests
(tests/test_host_cvrp_ls.py on the host build, tests/test_gpu_cvrp_ls.py on the device):
each case is built and solved by tests/cvrp_ls_ref.py once per session and handed out
read-only.  Demands are the generator's k / capacity (k in 1..9, rounded f32), the vehicle
capacity is 1; even rows start from a random permutation cut where the f32 running load
would pass 1.0, odd rows from the nearest-feasible greedy tour; every row is padded with 3
trailing zeros (and up to the widest row of its batch)."""
import functools

import numpy as np

from ls_cases_common import frozen, to_device, to_numpy
from cvrp_ls_ref import dist_from_locs, local_search

PAD = 3


def demands(rng, b, n, cap):
    return (rng.integers(1, 10, size=(b, n)).astype(np.float32) / np.float32(cap)).astype(np.float32)


def split_tour(perm, demand):
    """Visit ``perm`` (customers 1..n) in order, returning to the depot whenever the f32
    running load would pass 1.0 (the env's ``used + demand > capacity`` mask)."""
    out, used = [], np.float32(0.0)
    for c in perm:
        d = demand[c - 1]
        if np.float32(used + d) > np.float32(1.0):
            out.append(0)
            used = np.float32(0.0)
        out.append(int(c))
        used = np.float32(used + d)
    return out


def greedy_tour(D, demand):
    """From the current node go to the nearest unvisited customer that still fits (lowest
    index on ties), to the depot when none fits."""
    n = len(demand)
    left = set(range(1, n + 1))
    out, cur, used = [], 0, np.float32(0.0)
    while left:
        fit = [c for c in sorted(left) if not np.float32(used + demand[c - 1]) > np.float32(1.0)]
        if not fit:
            out.append(0)
            cur, used = 0, np.float32(0.0)
            continue
        c = min(fit, key=lambda v: (D[cur, v], v))
        out.append(c)
        left.discard(c)
        cur, used = c, np.float32(used + demand[c - 1])
    return out


def pad_rows(rows, pad=PAD):
    t = max(len(r) for r in rows) + pad
    return np.asarray([r + [0] * (t - len(r)) for r in rows], dtype=np.int64)


def solve(D, demand, tours, max_iterations=1000, capacity=None):
    """The restatement on every row; row ``e`` uses instance ``e % len(D)``.  Returns
    (rows int64 [B, T], sweeps int32 [B], tied sweeps in total); an invalid row comes back
    unchanged with 0 sweeps."""
    out, sweeps, tied = [], [], 0
    lb = len(D)
    for e, t in enumerate(tours):
        cap = 1.0 if capacity is None else capacity[e % lb]
        r, s, k = local_search(D[e % lb], demand[e % lb], cap, t, max_iterations)
        out.append(np.asarray(t, dtype=np.int64) if r is None else r)
        sweeps.append(s)
        tied += k
    return np.stack(out), np.asarray(sweeps, dtype=np.int32), tied


def start_tours(D, demand, b, seed, kind="mixed"):
    rng = np.random.default_rng(seed)
    lb, n = demand.shape
    rows = []
    for e in range(b):
        greedy = kind == "greedy" or (kind == "mixed" and e % 2 == 1)
        if greedy:
            rows.append(greedy_tour(D[e % lb], demand[e % lb]))
        else:
            rows.append(split_tour(rng.permutation(n) + 1, demand[e % lb]))
    return pad_rows(rows)


@functools.lru_cache(maxsize=None)
def uniform_case(b, n, cap=30, max_iterations=1000, lb=None):
    """Uniform coordinates [lb or b, n+1, 2] (depot first), demands [lb or b, n], start
    tours [b, T] and the restatement's (rows, sweeps, tied) on ``dist_from_locs``."""
    rng = np.random.default_rng(b * 4099 + n * 17 + cap)
    locs = rng.random((lb or b, n + 1, 2), dtype=np.float32)
    demand = demands(rng, lb or b, n, cap)
    D = [dist_from_locs(l) for l in locs]
    tours = start_tours(D, demand, b, seed=b * 7 + n)
    ref, sweeps, tied = solve(D, demand, tours, max_iterations)
    return frozen(locs, demand, tours, ref, sweeps) + (tied,)


@functools.lru_cache(maxsize=None)
def grid_case():
    """Depot at a corner of the 4 x 4 integer grid, the 15 other points as customers: many
    moves share a change bit for bit."""
    pts = np.array([(x, y) for x in range(4) for y in range(4)], dtype=np.float32)
    b = 32
    rng = np.random.default_rng(5)
    locs = np.repeat(pts[None], b, 0)
    demand = demands(rng, b, 15, 20)
    D = [dist_from_locs(pts)] * b
    tours = start_tours(D, demand, b, seed=6)
    ref, sweeps, tied = solve(D, demand, tours)
    return frozen(locs, demand, tours, ref, sweeps) + (tied,)


@functools.lru_cache(maxsize=None)
def int_matrix_case(b, n, symmetric, max_iterations=1000):
    """Explicit [n+1, n+1] matrices with entries in {1, 2, 3} (symmetric or not; an
    asymmetric search may cycle until max_iterations)."""
    rng = np.random.default_rng(n * 31 + symmetric)
    D = rng.integers(1, 4, size=(b, n + 1, n + 1)).astype(np.float32)
    if symmetric:
        D = (np.triu(D, 1) + np.transpose(np.triu(D, 1), (0, 2, 1))
             + np.eye(n + 1, dtype=np.float32))
    D = np.ascontiguousarray(D)
    demand = demands(rng, b, n, 30)
    tours = start_tours(D, demand, b, seed=n + 77)
    ref, sweeps, tied = solve(D, demand, tours, max_iterations)
    return frozen(D, demand, tours, ref, sweeps) + (tied,)


_LINE = np.array([(0, 0), (1, 0), (2, 0)], dtype=np.float32)
_H = np.float32(25) / np.float32(50)
# (name, locs [n+1, 2], demand [n], row, expected row, expected sweeps); capacity 1
KNOWN = [
    # sweep 1: 2-opt (1,2) and (2,3) tie at -2, (1,2) wins -> g = 0 0 1 2; sweep 2: nothing
    ("merge two routes", _LINE, [.4, .4], [1, 0, 2], [1, 2, 0], 2),
    # .6 + .6 > 1: every improving move is inadmissible
    ("merge refused", _LINE, [.6, .6], [1, 0, 2], [1, 0, 2], 1),
    # f32(25/50) twice fills the vehicle exactly
    ("exact fill", _LINE, [_H, _H], [1, 0, 2], [1, 2, 0], 2),
    ("zeros collapse", _LINE, [.4, .4], [0, 0, 2, 0, 0, 1, 0], [2, 1, 0, 0, 0, 0, 0], 2),
    # customer 3 = (4,0) leaves route 1-3 for the end of route 2-4: a relocate
    ("relocate", np.array([(0, 0), (0, 1), (1, 1), (4, 0), (4, 1)], dtype=np.float32),
     [.3, .3, .3, .3], [1, 3, 0, 2, 4], [1, 0, 2, 4, 3], 2),
]


def run(fn, tours, demand, locs=None, distances=None, capacity=None, device="cpu", **kw):
    """Call ``ops.cvrp_local_search`` on numpy inputs moved to ``device``; numpy
    (rows, sweeps)."""
    def dev(a, dt):
        return to_device(a, dt, device)

    return to_numpy(fn(dev(tours, np.int64), dev(demand, np.float32),
                       locs=dev(locs, np.float32), distances=dev(distances, np.float32),
                       capacity=dev(capacity, np.float32), return_sweeps=True, **kw))
