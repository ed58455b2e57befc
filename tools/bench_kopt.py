"""Env-steps/s of the k-opt improvement MDP at TSP-100 for k_max 2 and 4: the fused
``co_tsp_kopt_steps`` launch (``TSPkoptEnv.improve_steps``), T single ``co_tsp_kopt_step``
launches (``TSPkoptEnv.step``) and the torch restatement tests/kopt_ref.py, which issues the
reference's O(N) gather / scatter launches per step, all on the same device.  Prints one
JSON line.  Usage: ``python tools/bench_kopt.py [--batch B] [--steps T] [--reps R]
[--device cuda]``."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import kopt_cases as kc  # noqa: E402
import kopt_ref  # noqa: E402


def timed(fn, reps, device):
    best = float("inf")
    for _ in range(reps + 1):  # the first run warms up
        if device != "cpu":
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        if device != "cpu":
            torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--num-loc", type=int, default=100)
    ap.add_argument("--device", default="cuda" if torch.cuda.is_available() else "cpu")
    a = ap.parse_args()
    b, t, n, dev = a.batch, a.steps, a.num_loc, a.device
    out = {"bench": "tsp_kopt", "num_loc": n, "batch": b, "steps": t, "device": dev}
    for k in (2, 4):
        locs, rec, g = kc.instance(b, n, 17 + k)
        # valid actions need the evolving tour: generated on a slice of the batch and tiled
        small = min(b, 64)
        acts = kc.actions_for(g, rec[:small], k, t)
        acts = acts.repeat(1, -(-b // small), 1)[:, :b].contiguous()
        rec = rec[:small].repeat(-(-b // small), 1)[:b].contiguous()
        env = kc.product_env(n, k, dev)
        dacts, dlocs, drec = acts.to(dev), locs.to(dev), rec.to(dev)

        def fused():
            env.improve_steps(kc.product_state(dlocs, drec, dev), dacts)

        def single():
            td = kc.product_state(dlocs, drec, dev)
            for x in dacts:
                td["action"] = x
                td = env.step(td)["next"]

        def restated():
            kopt_ref.steps(kopt_ref.reset(dlocs, drec.clone()), dacts, k)

        for name, fn in (("fused", fused), ("single", single), ("torch", restated)):
            out[f"k{k}_{name}_steps_per_s"] = round(b * t / timed(fn, a.reps, dev), 1)
        out[f"k{k}_fused_over_torch"] = round(
            out[f"k{k}_fused_steps_per_s"] / out[f"k{k}_torch_steps_per_s"], 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
