"""co_tsp_local_search (TSPEnv.local_search with operators=...) on uniform TSP-100 at
B = 8,192 and TSP-20 at B = 65,536, from random permutations and from nearest-neighbour
tours (measurement tool, not part of the product).  Per case, ms per call (tools/ls_bench.py:
the median of 5 calls after a warm-up, by device events around the call) of
co_tsp_two_opt, of co_tsp_local_search with TWO_OPT only and of co_tsp_two_opt again (the two
entries run the same kernel instance: the spread of the two co_tsp_two_opt runs is what
any figure of this tool is read against), then of co_tsp_local_search with both operators;
the mean tour length after each, the sweeps and the applied moves.  The host build runs
both operators on the first 256 rows and is compared.
Usage: python tools/bench_tsp_ls.py [--quick] -> one JSON line."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from rl4co_slap_amd import _native as nat  # noqa: E402
from rl4co_slap_amd.utils.ops import gather_by_index, tsp_local_search, two_opt  # noqa: E402
from bench_two_opt import nearest_neighbour_tours  # noqa: E402
from ls_bench import HOST_THREADS, host_leg, same_rows, timed  # noqa: E402


def mean_length(locs, tours):
    p = gather_by_index(locs, tours)
    return round(float((p - p.roll(-1, 1)).norm(dim=-1).sum(1).double().mean().item()), 5)


def measure(locs, tours, dev):
    def new(operators):
        return lambda: tsp_local_search(tours, locs=locs, operators=operators,
                                        return_sweeps=True, return_moves=True)

    def old():
        return two_opt(tours, locs=locs, return_sweeps=True)

    old_a, (o_out, o_sw) = timed(old, dev)
    new_2, (t_out, t_sw, _) = timed(new(("two_opt",)), dev)
    old_b, _ = timed(old, dev)
    both, (b_out, b_sw, b_mv) = timed(new(("two_opt", "or_opt")), dev)
    _, host_ms, hres = host_leg(lambda t, l: tsp_local_search(
        t, locs=l, return_sweeps=True, return_moves=True), tours, locs)
    return {"ms_two_opt_entry": [round(old_a, 4), round(old_b, 4)],
            "ms_new_entry_two_opt_only": round(new_2, 4),
            "ms_new_entry_both": round(both, 4),
            "two_opt_only_equals_two_opt_entry": bool(torch.equal(o_out, t_out)
                                                      and torch.equal(o_sw, t_sw)),
            "mean_length_start": mean_length(locs, tours),
            "mean_length_two_opt": mean_length(locs, o_out),
            "mean_length_both": mean_length(locs, b_out),
            "sweeps_mean_two_opt": round(float(o_sw.double().mean().item()), 2),
            "sweeps_mean_both": round(float(b_sw.double().mean().item()), 2),
            "moves_mean_both": [round(v, 2) for v in b_mv.double().mean(0).tolist()],
            "rows_with_or_opt_move": round(float((b_mv[:, 1] > 0).double().mean().item()), 4),
            "host_rows": hres[0].shape[0], "host_threads": HOST_THREADS,
            "host_ms_wall_both": round(host_ms, 2),
            "host_equals_device": same_rows(hres, (b_out, b_sw, b_mv))}


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
