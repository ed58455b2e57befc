"""Inputs and restatement results shared by the SLAP local-search tests
(tests/test_host_slap_ls.py on the host build, tests/test_gpu_slap_ls.py on the device):
each case is built and solved by tests/slap_ls_ref.py once per session and handed out
read-only.  Picklists are uniform draws from 0..P-1 (repeats within an order included, as
the generator's).  Start rows cycle through three kinds: distinct random slots from
1..L-1, distinct random slots from 0..L-1 (a product may sit on the depot slot) and the
P slots closest to slot 0 in product order."""
import functools

import numpy as np
import torch

from ls_cases_common import frozen, to_device, to_numpy
from slap_ls_ref import dist_from_locs, local_search
from rl4co_slap_amd import TensorDict
from rl4co_slap_amd._native import ST_INDEX_RANGE, ST_INVALID_TOUR

# (B, P, L, O, K, max_iterations): the smallest shapes at which the kernel can go wrong
SHAPES = [(37, 1, 2, 1, 1, 1000), (37, 2, 3, 2, 2, 1000), (64, 5, 8, 4, 3, 1000),
          (16, 20, 100, 20, 5, 1000), (8, 63, 64, 20, 5, 1000), (8, 64, 130, 30, 5, 1000),
          (8, 65, 130, 30, 5, 1000), (2, 128, 256, 40, 5, 5), (2, 20, 1024, 20, 5, 3)]


# (P, L) on either side of the device's table / direct cut (CO_SLAP_LS_TABLE_FITS)
CUT_SHAPES = [(32, 239), (32, 240), (50, 147), (50, 148)]


def grid_locs(n_aisles=10, n_locs=10, inter_aisle=2.4, inter_loc=1.0):
    """The coordinates SLAPGenerator.grid() gives (f64 products rounded to f32)."""
    i = np.arange(n_aisles * n_locs)
    return np.stack([(i // n_locs) * inter_aisle, (i % n_locs) * inter_loc], -1).astype(np.float32)


def start_rows(rng, D, b, p):
    """[b, p] int32 start assignments; D [lb, L, L] orders the closest-to-depot rows."""
    lb, L = len(D), len(D[0])
    rows = []
    for e in range(b):
        kind = e % 3
        if kind == 0 or p > L - 1:
            lo = 0 if p > L - 1 else 1
            rows.append(lo + rng.permutation(L - lo)[:p])
        elif kind == 1:
            rows.append(rng.permutation(L)[:p])
        else:
            order = np.argsort(D[e % lb][0][1:], kind="stable") + 1
            rows.append(order[:p])
    return np.asarray(rows, dtype=np.int32)


def solve(D, picklist, rows, max_iterations=1000, locs=None):
    """The restatement on every row; row ``e`` uses instance ``e % len(D)``.  Returns (rows
    int32 [B, P], sweeps int32 [B], cost int64 [B], tied sweeps in total); a row that fails
    its check comes back unchanged with 0 sweeps and cost -1."""
    out, sweeps, cost, tied = [], [], [], 0
    lb = len(D)
    for e, s in enumerate(rows):
        r, n, f, k = local_search(D[e % lb], picklist[e % lb], s, max_iterations,
                                  None if locs is None else locs[e % lb])
        out.append(np.asarray(s) if r is None else r)
        sweeps.append(n)
        cost.append(f)
        tied += k
    return (np.stack(out).astype(np.int32), np.asarray(sweeps, dtype=np.int32),
            np.asarray(cost, dtype=np.int64), tied)


@functools.lru_cache(maxsize=None)
def coords_case(b, p, L, o, k, max_iterations=1000, lb=None, grid=False):
    """Coordinates [lb or b, L, 2] (uniform in [0, 10)^2, or the generator's grid),
    picklists [lb or b, o, k], start rows [b, p] and the restatement's (rows, sweeps, cost,
    tied) on ``dist_from_locs``."""
    n = lb or b
    rng = np.random.default_rng(b * 4099 + p * 17 + L)
    if grid:
        locs = np.repeat(grid_locs()[None], n, 0)
        assert L == locs.shape[1]
    else:
        locs = (rng.random((n, L, 2), dtype=np.float32) * np.float32(10)).astype(np.float32)
    picklist = rng.integers(0, p, size=(n, o, k)).astype(np.int64)
    D = [dist_from_locs(l) for l in locs]
    rows = start_rows(rng, D, b, p)
    ref, sweeps, cost, tied = solve(D, picklist, rows, max_iterations, locs)
    return frozen(locs, picklist, rows, ref, sweeps, cost) + (tied,)


@functools.lru_cache(maxsize=None)
def int_matrix_case(b, symmetric, p=12, L=14, o=10, k=4, max_iterations=1000):
    """Explicit [L, L] matrices with entries in {0, 1, 2}, the diagonal included (symmetric
    or not): many candidates share a change bit for bit."""
    rng = np.random.default_rng(L * 31 + p + symmetric)
    D = rng.integers(0, 3, size=(b, L, L)).astype(np.float32)
    if symmetric:
        up = np.triu(D, 1)
        D = up + np.transpose(up, (0, 2, 1)) + D * np.eye(L, dtype=np.float32)
    D = np.ascontiguousarray(D)
    picklist = rng.integers(0, p, size=(b, o, k)).astype(np.int64)
    rows = start_rows(rng, D, b, p)
    ref, sweeps, cost, tied = solve(D, picklist, rows, max_iterations)
    return frozen(D, picklist, rows, ref, sweeps, cost) + (tied,)


@functools.lru_cache(maxsize=None)
def matrix_case(b, p, L, o, k, max_iterations=1000):
    """An explicit asymmetric matrix: Euclidean distances plus a one-way surcharge."""
    rng = np.random.default_rng(b * 131 + p * 7 + L)
    locs = (rng.random((b, L, 2), dtype=np.float32) * np.float32(10)).astype(np.float32)
    D = np.stack([dist_from_locs(l) for l in locs])
    D = np.ascontiguousarray(D + np.triu(rng.random((b, L, L), dtype=np.float32), 1))
    picklist = rng.integers(0, p, size=(b, o, k)).astype(np.int64)
    rows = start_rows(rng, D, b, p)
    ref, sweeps, cost, tied = solve(D, picklist, rows, max_iterations)
    return frozen(D, picklist, rows, ref, sweeps, cost) + (tied,)


_LINE4 = np.array([(0, 0), (1, 0), (2, 0), (3, 0)], dtype=np.float32)
_LINE5 = np.array([(0, 0), (1, 0), (2, 0), (3, 0), (4, 0)], dtype=np.float32)
_U = 1 << 20
# (name, locs [L, 2], picklist [O, K], row, expected row, expected sweeps, expected cost)
KNOWN = [
    # F = 2 d(1,3) = 4.  Moves (0 -> 2) and (1 -> 2) tie at -2, the smaller p wins; then the
    # only free target is slot 1 (slot 0 is never one) and nothing improves
    ("two moves tie", _LINE4, [[0, 1]], [1, 3], [2, 3], 2, 2 * _U),
    ("already optimal", _LINE4, [[0, 1]], [1, 2], [1, 2], 1, 2 * _U),
    # no free slot: swaps (0,1) and (1,2) tie at -2, (0,2) changes nothing; (0,1) wins
    ("two swaps tie", _LINE4, [[0, 2]], [1, 2, 3], [2, 1, 3], 2, 2 * _U),
    # product 2 has no flow.  Move (0 -> 4) and swaps (0,2), (1,2) tie at -2: the move wins
    ("move before swap", _LINE5, [[0, 1]], [1, 3, 2], [4, 3, 2], 2, 2 * _U),
    # F = 6.  (0 -> 2) and (1 -> 1) tie at -4: the product on the depot slot leaves it
    ("slot 0 is left", _LINE4, [[0, 1]], [0, 3], [2, 3], 2, 2 * _U),
    # an order that repeats a product: [0, 0, 1] has the pairs (0,1), (1,0) only
    ("equal neighbours", _LINE4, [[0, 0, 1]], [1, 3], [2, 3], 2, 2 * _U),
    # one product, nowhere to gain: one sweep, cost 0
    ("one product", _LINE4[:2], [[0]], [1], [1], 1, 0),
]


def run(fn, rows, picklist, locs=None, distances=None, device="cpu", dtype=np.int32, **kw):
    """Call ``ops.slap_local_search`` on numpy inputs moved to ``device``; numpy
    (rows, sweeps, cost)."""
    def dev(a, dt):
        return to_device(a, dt, device)

    return to_numpy(fn(dev(rows, dtype), dev(picklist, np.int64), locs=dev(locs, np.float32),
                       distances=dev(distances, np.float32), return_sweeps=True,
                       return_cost=True, **kw))


def slap_td(locs, pl, rows, dev="cpu", dist=None):
    n = len(locs)
    d = {"locs": torch.as_tensor(locs.copy()).to(dev),
         "picklist": torch.as_tensor(pl.copy()).to(dev),
         "assignment": torch.as_tensor(rows[:n].copy()).to(dev),
         "freq": torch.ones(n, rows.shape[1], 1, device=dev)}
    if dist is not None:
        d["dist_mat"] = torch.as_tensor(dist.copy()).to(dev)
    return TensorDict(d, [n])


ERRORS = ["duplicate", "minus_one", "slot_L", "picklist_P", "nan_coord", "matrix_above"]


def error_inputs(kind):
    """The (64, 5, 8, 4, 3) case with row / instance 3 broken; (rows, pl, locs, D, bit)."""
    locs, pl, rows, ref, sweeps, cost, _ = coords_case(64, 5, 8, 4, 3)
    rows, pl, locs = rows.copy(), pl.copy(), locs.copy()
    D = None
    bit = ST_INVALID_TOUR
    if kind == "duplicate":
        rows[3, 1] = rows[3, 0]
    elif kind == "minus_one":
        rows[3, 2] = -1
    elif kind == "slot_L":
        rows[3, 4] = 8
    elif kind == "picklist_P":
        pl[3, 1, 2] = 5
        bit = ST_INDEX_RANGE
    elif kind == "nan_coord":
        locs[3, 7, 1] = np.nan
    else:
        D = np.stack([dist_from_locs(l) for l in locs])
        D[3, 2, 5] = np.float32(2 ** 20 + 1)
    return rows, pl, locs, D, bit


def bound(reward, o, k):
    return 1e-5 * reward.abs().double() + o * k * 2.0 ** -20
