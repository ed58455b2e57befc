"""The 2-opt tests' view of tests/tsp_ls_cases.py (tests/test_host_two_opt.py on the host
build, tests/test_gpu_two_opt.py on the device): the TWO_OPT cases without their moves
column, and the hand cases of ``co_tsp_two_opt``."""
import numpy as np

import tsp_ls_cases as lc
from ls_cases_common import to_device, to_numpy
from tsp_ls_cases import perms, uniform_locs  # noqa: F401  (the tests build inputs with them)
from tsp_ls_ref import TWO_OPT

E23 = 2.0 ** -23


def solve(D, tours, max_iterations=1000):
    """(tours int64 [B, n], sweeps int32 [B], tied sweeps in total)."""
    out, sweeps, _, tied = lc.solve(D, tours, TWO_OPT, max_iterations)
    return out, sweeps, tied


def uniform_case(b, n, max_iterations=1000, lb=None):
    """(locs, tours, restatement tours, restatement sweeps)."""
    return lc.uniform_case(b, n, TWO_OPT, max_iterations, lb, 0.0)[:4]


def grid_case():
    """(locs, tours, restatement tours, restatement sweeps, tied sweeps)."""
    case = lc.grid_case(TWO_OPT)
    return case[:4] + case[5:]


def int_matrix_case(b, n, symmetric, max_iterations=1000):
    """(matrices, tours, restatement tours, restatement sweeps, tied sweeps)."""
    case = lc.int_matrix_case(b, n, symmetric, TWO_OPT, max_iterations)
    return case[:4] + case[5:]


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
