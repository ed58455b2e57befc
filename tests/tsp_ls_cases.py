"""Inputs and restatement results shared by the TSP local-search tests (co_tsp_local_search:
tests/test_host_tsp_ls.py on the host build, tests/test_gpu_tsp_ls.py on the device;
co_tsp_two_opt takes the TWO_OPT cases through the view in tests/two_opt_cases.py): each case
is built and solved by tests/tsp_ls_ref.py once per session and handed out read-only.

A case meant to exercise Or-opt after 2-opt must apply at least one Or-opt move in a
quarter of its rows (``min_or_rows``, asserted when the case is built; the seeds are
fixed).  After 2-opt has converged that holds from about n = 20 on; the small shapes run
with OR_OPT alone from random tours, where Or-opt moves are plentiful."""
import functools

import numpy as np
import torch

from ls_cases_common import frozen, to_device, to_numpy
from tsp_ls_ref import OR_OPT, TWO_OPT, local_search
from two_opt_ref import dist_from_locs

BOTH = TWO_OPT | OR_OPT
NAMES = {TWO_OPT: ("two_opt",), OR_OPT: ("or_opt",), BOTH: ("two_opt", "or_opt")}


def perms(b, n, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(n) for _ in range(b)]).astype(np.int64).reshape(b, n)


def uniform_locs(b, n, seed):
    return np.random.default_rng(seed + 1000).random((b, n, 2), dtype=np.float32)


def solve(D, tours, operators=BOTH, max_iterations=1000, min_or_rows=0.0):
    """The restatement on every row; row ``e`` uses matrix ``e % len(D)``.  Returns (tours
    int64 [B, n], sweeps int32 [B], moves int32 [B, 2], tied sweeps in total)."""
    out, sweeps, moves, tied = [], [], [], 0
    for e, t in enumerate(tours):
        r, s, m, k = local_search(D[e % len(D)], t, operators, max_iterations)
        out.append(r)
        sweeps.append(s)
        moves.append(m)
        tied += k
    moves = np.asarray(moves, dtype=np.int32).reshape(len(tours), 2)
    assert (moves[:, 1] > 0).mean() >= min_or_rows, ("too few rows apply an Or-opt move",
                                                     moves[:, 1])
    return (np.stack(out).reshape(len(tours), -1), np.asarray(sweeps, dtype=np.int32), moves,
            tied)


@functools.lru_cache(maxsize=None)
def uniform_case(b, n, operators=BOTH, max_iterations=1000, lb=None, min_or_rows=0.25):
    """Random uniform coordinates [lb or b, n, 2], random tours [b, n] and the restatement's
    (tours, sweeps, moves) on ``dist_from_locs``."""
    locs = uniform_locs(lb or b, n, seed=b * 4099 + n)
    tours = perms(b, n, seed=b * 7 + n)
    D = [dist_from_locs(l) for l in locs]
    ref, sweeps, moves, _ = solve(D, tours, operators, max_iterations, min_or_rows)
    return frozen(locs, tours, ref, sweeps, moves)


@functools.lru_cache(maxsize=None)
def matrix_case(b, n, operators=BOTH, max_iterations=1000, min_or_rows=0.25):
    """``uniform_case`` handed over as explicit f32 matrices [b, n, n]."""
    locs, tours, ref, sweeps, moves = uniform_case(b, n, operators, max_iterations, None,
                                                   min_or_rows)
    D = np.stack([dist_from_locs(l) for l in locs])
    return frozen(D, tours, ref, sweeps, moves)


@functools.lru_cache(maxsize=None)
def grid_case(operators=BOTH):
    """32 random tours of the 4 x 4 integer grid: many moves share a change bit for bit."""
    pts = np.array([(x, y) for x in range(4) for y in range(4)], dtype=np.float32)
    locs = np.repeat(pts[None], 32, 0)
    tours = perms(32, 16, seed=5)
    ref, sweeps, moves, tied = solve([dist_from_locs(pts)], tours, operators)
    return frozen(locs, tours, ref, sweeps, moves) + (tied,)


@functools.lru_cache(maxsize=None)
def int_matrix_case(b, n, symmetric, operators=BOTH, max_iterations=1000):
    """Explicit matrices with entries in {1, 2, 3} (symmetric or not; an asymmetric search
    may cycle until max_iterations: always pass a small cap there)."""
    rng = np.random.default_rng(n * 31 + symmetric)
    D = rng.integers(1, 4, size=(b, n, n)).astype(np.float32)
    if symmetric:
        D = np.triu(D, 1) + np.transpose(np.triu(D, 1), (0, 2, 1)) + np.eye(n, dtype=np.float32)
    tours = perms(b, n, seed=n + 77)
    ref, sweeps, moves, tied = solve(D, tours, operators, max_iterations)
    return frozen(np.ascontiguousarray(D), tours, ref, sweeps, moves) + (tied,)


def _line(xs):
    return np.array([(x, 0.0) for x in xs], dtype=np.float32)


def _ones5(eps_units):
    """All distances 1 except D[1,3] = D[3,1] = 1 - eps_units * 2^-23: moving city 2 of the
    tour 0 1 2 3 4 elsewhere gains exactly that much (2-opt is disabled in these cases)."""
    D = np.ones((5, 5), dtype=np.float32)
    D[1, 3] = D[3, 1] = np.float32(1.0 - eps_units * 2.0 ** -23)
    return D


# (name, locs [n, 2] or None, distances [n, n] or None, operators, tour, expected tour,
#  expected sweeps, expected (2-opt, Or-opt) moves)
KNOWN = [
    # cities on a line at 0 1 2 3 4 (+ one far above closing the loop); city 2 is parked
    # between 4 and 5: one L = 1 move puts it back between 1 and 3
    ("parked city", np.array([(0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (2, 3)], dtype=np.float32),
     None, OR_OPT, [0, 1, 3, 4, 2, 5], [0, 1, 2, 3, 4, 5], 2, (0, 1)),
    # the pair (3, 2) sits after 5 in the wrong order: it goes back between 1 and 4 reversed
    ("reversed pair", np.array([(0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (5, 0), (2.5, 4)],
                               dtype=np.float32),
     None, OR_OPT, [0, 1, 4, 5, 3, 2, 6], [0, 1, 2, 3, 4, 5, 6], 2, (0, 1)),
    # the best change is -4.77e-7, above the -1e-6 threshold: nothing is applied
    ("below threshold", None, _ones5(4), OR_OPT, [0, 1, 2, 3, 4], [0, 1, 2, 3, 4], 1, (0, 0)),
    # -1.9e-6 is applied; of the 11 tied candidates the first, (L = 1, i = 1, k = 2), wins
    ("above threshold", None, _ones5(16), OR_OPT, [0, 1, 2, 3, 4], [0, 2, 1, 3, 4], 2, (0, 1)),
    # n = 3: only L = 1 has a move (one per i); n = 4: L = 1 and L = 2, never L = 3
    ("n = 3", _line([0, 1, 2]), None, BOTH, [0, 2, 1], [0, 2, 1], 1, (0, 0)),
    ("n = 4", np.array([(0, 0), (1, 0), (1, 1), (0, 1)], dtype=np.float32), None, OR_OPT,
     [0, 2, 1, 3], [0, 1, 2, 3], 2, (0, 1)),
]


# ``ops.tsp_local_search(..., operators=("two_opt",))`` with both counts asked for: on the
# device the kernel instance without the Or-opt half, which co_tsp_two_opt runs with a null
# moves_out.  (b, n): the sizes around 3 (nothing to move below), one and several windows of
# 64, and on the distances path both sides of the LDS staging cut (126).
TWO_OPT_ONLY_COORDS = [(9, 1), (9, 2), (9, 3), (37, 5), (16, 20), (8, 63), (8, 64), (8, 65)]
TWO_OPT_ONLY_MATRICES = [(8, 12), (2, 126), (2, 127)]


def check_two_opt_only(ops, case, device, max_iterations=1000, **src):
    """``case`` = (tours, restatement tours, sweeps, moves) of the TWO_OPT restatement: the
    tours and sweeps are ``ops.two_opt``'s and the restatement's, no Or-opt move is counted
    and the 2-opt count is the restatement's.  Returns the restatement's (sweeps, moves)."""
    tours, ref, sweeps, moves = case
    got = run(ops.tsp_local_search, tours, device=device, operators=TWO_OPT,
              max_iterations=max_iterations, **src)
    old = to_numpy(ops.two_opt(to_device(tours, np.int64, device), return_sweeps=True,
                               max_iterations=max_iterations,
                               **{k: to_device(v, np.float32, device) for k, v in src.items()}))
    assert np.array_equal(got[0], old[0]) and np.array_equal(got[0], ref), "tours differ"
    assert np.array_equal(got[1], old[1]) and np.array_equal(got[1], sweeps), (got[1], sweeps)
    assert (got[2][:, 1] == 0).all() and (moves[:, 1] == 0).all()
    assert np.array_equal(got[2][:, 0], moves[:, 0]), ("moves differ", got[2][:, 0], moves[:, 0])
    return sweeps, moves


def check_two_opt_only_invalid_rows(ops, device, status_bit):
    """One duplicate and one out-of-range row at (16, 20): the status bit is set, both rows
    are copied with 0 sweeps and 0 moves, every other row is the restatement's."""
    locs, tours, ref, sweeps, moves = uniform_case(16, 20, TWO_OPT, 1000, None, 0.0)
    bad = tours.copy()
    bad[3, 7] = bad[3, 8]
    bad[5, 0] = 20
    status = torch.zeros(1, dtype=torch.int32, device=device)
    out, sw, mv = to_numpy(ops.tsp_local_search(
        to_device(bad, np.int64, device), locs=to_device(locs, np.float32, device),
        operators=("two_opt",), return_sweeps=True, return_moves=True, status=status))
    assert int(status.item()) == status_bit
    keep = ~np.isin(np.arange(16), [3, 5])
    assert np.array_equal(out[keep], ref[keep]) and np.array_equal(sw[keep], sweeps[keep])
    assert np.array_equal(mv[keep], moves[keep])
    assert np.array_equal(out[~keep], bad[~keep])
    assert (sw[~keep] == 0).all() and (mv[~keep] == 0).all()


def check_two_opt_only_null_outputs(ops, device):
    """moves_out null with sweeps_out given, and the reverse: what is given is still right."""
    locs, tours, ref, sweeps, moves = uniform_case(16, 20, TWO_OPT, 1000, None, 0.0)
    t, l = to_device(tours, np.int64, device), to_device(locs, np.float32, device)
    out, sw = to_numpy(ops.tsp_local_search(t, locs=l, operators=("two_opt",),
                                            return_sweeps=True))
    assert np.array_equal(out, ref) and np.array_equal(sw, sweeps)
    out, mv = to_numpy(ops.tsp_local_search(t, locs=l, operators=("two_opt",),
                                            return_moves=True))
    assert np.array_equal(out, ref) and np.array_equal(mv, moves)


def run(fn, tours, locs=None, distances=None, device="cpu", operators=BOTH, **kw):
    """Call ``ops.tsp_local_search`` on numpy inputs moved to ``device``; numpy (tours,
    sweeps, moves)."""
    return to_numpy(fn(to_device(tours, np.int64, device),
                       locs=to_device(locs, np.float32, device),
                       distances=to_device(distances, np.float32, device),
                       operators=NAMES[operators], return_sweeps=True, return_moves=True, **kw))
