"""co_slap_local_search (SLAPEnv.improve) on the default SLAP instance (P = 20 products,
L = 100 grid slots, O = 20 orders of K = 5) at B = 8,192, from a seeded random assignment
(distinct slots from 1..L-1) and from the assignment the closest-free-slot policy's rollout
ends with (product i on the i-th closest slot to the depot, lowest index on ties)
(measurement tool, not part of the product).  Per case and evaluation scheme (table, direct):
ms per ``ops.slap_local_search`` call (median of 5 calls after a warm-up, by device events
around the call), the sweeps per row and candidate evaluations per second, counted as sum
over rows of sweeps * (P (L-1-P) + P (P-1) / 2), and the mean reward before and after.  The
host build is timed in the same run on the first 256 rows (wall clock, one thread: the host
library is single-threaded) and its results are compared with the device's.  Further cases:
the Manhattan ``dist_mat`` of the same instances, and larger shapes (P = 32 and 50, uniform
coordinates, B / 4 rows) under both schemes up to the table / direct cut and the first direct
shape beyond it, two of them on an explicit matrix as well.
Usage: python tools/bench_slap_ls.py [--quick] -> one JSON line."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from rl4co_slap_amd import TensorDict  # noqa: E402
from rl4co_slap_amd import _native as nat  # noqa: E402
from rl4co_slap_amd.envs import SLAPEnv  # noqa: E402
from rl4co_slap_amd.envs.slap import SLAPGenerator  # noqa: E402
from rl4co_slap_amd.utils.ops import get_distance_matrix, slap_local_search  # noqa: E402
from ls_bench import HOST_THREADS, host_leg, same_rows, timed  # noqa: E402

SCHEMES = {"table": nat.SLAP_LS_TABLE, "direct": nat.SLAP_LS_DIRECT}


def measure(assign, picklist, dev, schemes, locs=None, distances=None, host=True):
    b, p = assign.shape
    src = locs if locs is not None else distances
    n_slots = src.shape[1]
    per_sweep = p * (n_slots - 1 - p) + p * (p - 1) // 2
    res = {"batch": b, "products": p, "slots": n_slots, "candidates_per_sweep": per_sweep}
    first = None
    for name in schemes:
        ms, (out, sweeps, cost) = timed(lambda: slap_local_search(
            assign, picklist, locs=locs, distances=distances, return_sweeps=True,
            return_cost=True, scheme=SCHEMES[name]), dev)
        total = int(sweeps.sum().item())
        res[name] = {"ms_per_call_events": round(ms, 4),
                     "candidate_evals_per_s": round(total * per_sweep / (ms * 1e-3), 1)}
        if first is None:
            first = (out, sweeps, cost)
            res.update({"sweeps_mean": round(total / b, 2), "sweeps_max": int(sweeps.max().item()),
                        "cost_after_over_before": None})
        else:
            res["schemes_equal"] = bool(torch.equal(out, first[0]) and torch.equal(sweeps, first[1])
                                        and torch.equal(cost, first[2]))
    out, sweeps, cost = first
    _, cost0 = slap_local_search(assign, picklist, locs=locs, distances=distances,
                                 max_iterations=0, return_cost=True)
    res["cost_after_over_before"] = round(float((cost.double() / cost0.double()).mean().item()), 4)
    if locs is not None:
        env = SLAPEnv(device=dev)
        for key, a in (("reward_mean_before", assign), ("reward_mean_after", out)):
            td = TensorDict({"assignment": a, "picklist": picklist, "locs": locs}, [b])
            res[key] = round(float(env.get_reward(td, None).mean().item()), 3)
    if host:
        h, host_ms, (hout, hsw, hcost) = host_leg(
            lambda a, pl, xy, d: slap_local_search(a, pl, locs=xy, distances=d, return_sweeps=True,
                                                   return_cost=True),
            assign, picklist, locs, distances)
        res.update({"host_rows": h[0].shape[0], "host_threads": HOST_THREADS,
                    "host_ms_wall": round(host_ms, 2),
                    "host_candidate_evals_per_s": round(
                        int(hsw.sum().item()) * per_sweep / (host_ms * 1e-3), 1),
                    "host_equals_device": same_rows((hout, hsw, hcost), (out, sweeps, cost))})
    return res


def random_rows(b, p, n_slots, gen, dev):
    return (torch.rand(b, n_slots - 1, generator=gen).argsort(1)[:, :p] + 1).to(torch.int32).to(dev)


def main():
    quick = "--quick" in sys.argv
    dev = torch.device("cuda:0")
    nat.load()
    nat.load_host()
    res = {"device": torch.cuda.get_device_name(0)}
    b = 8192 // (16 if quick else 1)
    g = torch.Generator().manual_seed(20)
    gen = SLAPGenerator()
    p, o, k = gen.n_products, gen.max_orders, gen.max_products_in_order
    grid = gen.grid()
    n_slots = grid.shape[0]
    locs = grid.expand(b, n_slots, 2).contiguous().to(dev)
    picklist = torch.randint(0, p, (b, o, k), generator=g).to(dev)
    rand = random_rows(b, p, n_slots, g, dev)
    depot = SLAPGenerator._get_distance_matrix(grid)[0]  # Manhattan, as depot_loc_dist
    closest = (torch.argsort(depot[1:], stable=True)[:p] + 1).to(torch.int32)
    closest = closest.expand(b, p).contiguous().to(dev)
    both = ("table", "direct")
    res["default_random"] = measure(rand, picklist, dev, both, locs=locs)
    res["default_closest_free"] = measure(closest, picklist, dev, both, locs=locs)
    manhattan = SLAPGenerator._get_distance_matrix(grid).expand(b, n_slots, n_slots)
    res["default_random_dist_mat"] = measure(rand, picklist, dev, both,
                                             distances=manhattan.contiguous().to(dev))
    # larger tables (fewer rows resident per CU) under both schemes, up to the cut at P = 32
    # and P = 50, and the first direct shape beyond each
    bc = b // 4
    for pp, ll in ((32, 128), (32, 239), (32, 240), (50, 100), (50, 147), (50, 148)):
        schemes = both if nat.slap_ls_table_fits(pp, ll) else ("direct",)
        xy = (torch.rand(bc, ll, 2, generator=g) * 10).to(dev)
        pl = torch.randint(0, pp, (bc, o, k), generator=g).to(dev)
        rows = random_rows(bc, pp, ll, g, dev)
        res[f"p{pp}_l{ll}_locs"] = measure(rows, pl, dev, schemes, locs=xy, host=False)
        if ll in (100, 239):
            res[f"p{pp}_l{ll}_dist_mat"] = measure(rows, pl, dev, schemes,
                                                   distances=get_distance_matrix(xy), host=False)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
