"""co_tsp_two_opt (TSPEnv.local_search) on uniform TSP-100 at B = 8,192 and TSP-20 at
B = 65,536, from random permutations and from nearest-neighbour tours (measurement tool,
not part of the product).  Per case: ms per call (median of 5 calls after a warm-up, by
device events around the call), the total sweeps (sweeps_out) and candidate evaluations
per second, counted as sum(sweeps) * (N-1)(N-2)/2.  The host build is timed in the same
run on the first 256 rows (wall clock, one thread: the host library is single-threaded).
Usage: python tools/bench_two_opt.py [--quick] -> one JSON line."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from rl4co_slap_amd import _native as nat  # noqa: E402
from rl4co_slap_amd.utils.ops import get_distance_matrix, two_opt  # noqa: E402
from ls_bench import HOST_THREADS, host_leg, same_rows, timed  # noqa: E402


def nearest_neighbour_tours(locs):
    """Start at node 0, always move to the nearest unvisited node (lowest index on ties)."""
    b, n, _ = locs.shape
    dist = get_distance_matrix(locs)
    rows = torch.arange(b, device=locs.device)
    visited = torch.zeros(b, n, dtype=torch.bool, device=locs.device)
    cur = torch.zeros(b, dtype=torch.int64, device=locs.device)
    tour = [cur]
    visited[rows, cur] = True
    for _ in range(n - 1):
        cur = dist[rows, cur].masked_fill(visited, float("inf")).argmin(1)
        visited[rows, cur] = True
        tour.append(cur)
    return torch.stack(tour, 1)


def measure(locs, tours, dev):
    n = tours.shape[1]
    ms, (out, sweeps) = timed(lambda: two_opt(tours, locs=locs, return_sweeps=True), dev)
    total = int(sweeps.sum().item())
    evals = total * (n - 1) * (n - 2) // 2
    (ht, hl), host_ms, (hout, hsw) = host_leg(
        lambda t, l: two_opt(t, locs=l, return_sweeps=True), tours, locs)
    host_evals = int(hsw.sum().item()) * (n - 1) * (n - 2) // 2
    same = same_rows((hout, hsw), (out, sweeps))
    return {"ms_per_call_events": round(ms, 4), "sweeps_total": total,
            "sweeps_mean": round(total / tours.shape[0], 2), "sweeps_max": int(sweeps.max().item()),
            "candidate_evals_per_s": round(evals / (ms * 1e-3), 1),
            "host_rows": hl.shape[0], "host_threads": HOST_THREADS,
            "host_ms_wall": round(host_ms, 2),
            "host_candidate_evals_per_s": round(host_evals / (host_ms * 1e-3), 1),
            "host_equals_device": same}


def main():
    quick = "--quick" in sys.argv
    dev = torch.device("cuda:0")
    nat.load()
    nat.load_host()
    res = {"device": torch.cuda.get_device_name(0)}
    for n, b in ((100, 8192), (20, 65536)):
        if quick:
            b //= 16
        g = torch.Generator().manual_seed(n)
        locs = torch.rand(b, n, 2, generator=g).to(dev)
        rand = torch.rand(b, n, generator=g).argsort(1).to(dev)
        res[f"tsp{n}_b{b}_random"] = measure(locs, rand, dev)
        res[f"tsp{n}_b{b}_nearest"] = measure(locs, nearest_neighbour_tours(locs), dev)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
