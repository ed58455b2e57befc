"""Inputs and restatement results shared by the 2-opt tests (tests/test_host_two_opt.py on
the host build, tests/test_gpu_two_opt.py on the device): each case is built and solved by
tests/two_opt_ref.py once per session and handed out read-only."""
import functools

import numpy as np

from ls_cases_common import frozen, to_device, to_numpy
from two_opt_ref import dist_from_locs, two_opt

E23 = 2.0 ** -23


def perms(b, n, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(n) for _ in range(b)]).astype(np.int64).reshape(b, n)


def uniform_locs(b, n, seed):
    return np.random.default_rng(seed + 1000).random((b, n, 2), dtype=np.float32)


def solve(D, tours, max_iterations=1000):
    """The restatement on every row; row ``e`` uses matrix ``e % len(D)``.  Returns
    (tours int64 [B, n], sweeps int32 [B], tied sweeps in total)."""
    out, sweeps, tied = [], [], 0
    for e, t in enumerate(tours):
        r, s, k = two_opt(D[e % len(D)], t, max_iterations)
        out.append(r)
        sweeps.append(s)
        tied += k
    return (np.stack(out).reshape(len(tours), -1), np.asarray(sweeps, dtype=np.int32), tied)


@functools.lru_cache(maxsize=None)
def uniform_case(b, n, max_iterations=1000, lb=None):
    """Random uniform coordinates [lb or b, n, 2], random tours [b, n] and the restatement's
    (tours, sweeps) on ``dist_from_locs``."""
    locs = uniform_locs(lb or b, n, seed=b * 4099 + n)
    tours = perms(b, n, seed=b * 7 + n)
    D = [dist_from_locs(l) for l in locs]
    ref, sweeps, _ = solve(D, tours, max_iterations)
    return frozen(locs, tours, ref, sweeps)


@functools.lru_cache(maxsize=None)
def grid_case():
    """32 random tours of the 4 x 4 integer grid: many moves share a change bit for bit."""
    pts = np.array([(x, y) for x in range(4) for y in range(4)], dtype=np.float32)
    locs = np.repeat(pts[None], 32, 0)
    tours = perms(32, 16, seed=5)
    ref, sweeps, tied = solve([dist_from_locs(pts)], tours)
    return frozen(locs, tours, ref, sweeps) + (tied,)


@functools.lru_cache(maxsize=None)
def int_matrix_case(b, n, symmetric, max_iterations=1000):
    """Explicit matrices with entries in {1, 2, 3} (symmetric or not; an asymmetric search
    may cycle until max_iterations)."""
    rng = np.random.default_rng(n * 31 + symmetric)
    D = rng.integers(1, 4, size=(b, n, n)).astype(np.float32)
    if symmetric:
        D = np.triu(D, 1) + np.transpose(np.triu(D, 1), (0, 2, 1)) + np.eye(n, dtype=np.float32)
    tours = perms(b, n, seed=n + 77)
    ref, sweeps, tied = solve(D, tours, max_iterations)
    return frozen(np.ascontiguousarray(D), tours, ref, sweeps) + (tied,)


def _ones4(eps_units):
    D = np.ones((4, 4), dtype=np.float32)
    D[0, 2] = D[2, 0] = np.float32(1.0 - eps_units * E23)
    return D


# (name, locs [n, 2] or None, distances [n, n] or None, tour, expected tour, expected sweeps)
KNOWN = [
    ("unit square", np.array([(0, 0), (1, 0), (1, 1), (0, 1)], dtype=np.float32), None,
     [0, 2, 1, 3], [0, 1, 2, 3], 2),
    # the best change is -4.77e-7, above the -1e-6 threshold: nothing is applied
    ("below threshold", None, _ones4(4), [0, 1, 2, 3], [0, 1, 2, 3], 1),
    # two moves tie at -1.9e-6: the earlier (1, 2) wins
    ("tied pair", None, _ones4(16), [0, 1, 2, 3], [0, 2, 1, 3], 2),
]


def run(two_opt_fn, tours, locs=None, distances=None, device="cpu", **kw):
    """Call ``ops.two_opt`` on numpy inputs moved to ``device``; numpy (tours, sweeps)."""
    return to_numpy(two_opt_fn(to_device(tours, np.int64, device),
                               locs=to_device(locs, np.float32, device),
                               distances=to_device(distances, np.float32, device),
                               return_sweeps=True, **kw))
