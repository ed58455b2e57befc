"""Recorder of tests/golden/kopt/ref_kopt.npz (a folder of its own: tests/test_golden.py pins
the ``ref_*.npz`` set beside this file): what the reference's own ``TSPkoptEnv``
(``rl4co/envs/routing/tsp/env.py``) returns over seeded episodes whose actions come from its
own ``_random_action``.  Runs in a process of its own (``python tests/golden/record_kopt.py
[--out DIR]``): ``oracle.reference.load()`` imports the reference's modules from a checkout
through stand-ins; nothing of the reference is copied -- only arrays and key names are
stored, node indices as uint8.

Keys are ``kopt/<case>/<name>``; per-step arrays are stacked ``[T, ...]``.  A case starts
with ``torch.manual_seed(seed)``, draws ``locs = torch.rand(B, N, 2)`` and resets (the
initial solution is the generator's draw from the same stream).

Condition on the inputs (not a tolerance of the tests): a row-step is *clear* when the step
left ``rec_current`` unchanged or the new cost differs from the best-so-far cost by at least
``1e-4 * cost_bsf``, so that a 1e-5 relative difference in the summation cannot flip an
improvement test; ``step_margin`` stores the figure per row-step (inf for a no-op).  For the
cases not in TIES the seed is re-drawn (at most MAX_REDRAWS times) until every row-step is
clear.  The cases in TIES never met that: a move that only turns the tour round (2-opt with
second == pred(first): one pair in N - 1) or that returns to the best tour changes rec and
leaves the cost equal up to summation order, and on small tours such moves are frequent (3
to 25 % of the row-steps).  They are recorded under their first seed with the margins as
they are; the tests compare what does not depend on the improvement test (``rec_current``,
``visited_time``, ``cost_current``, ``i``) on every row-step and the best-so-far keys
(``cost_bsf``, ``reward``, ``rec_best``) on each row up to its first row-step that is not
clear.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import reference  # noqa: E402
from oracle.record_reference import write_npz  # noqa: E402

MARGIN = 1e-4
MAX_REDRAWS = 400
B, T = 16, 12
CASES = [(k, n, "random") for k in (2, 3, 4) for n in (5, 20, 65)] + \
        [(k, 20, "greedy") for k in (2, 3, 4)]
TIES = ((2, 5, "random"), (3, 5, "random"), (4, 5, "random"), (2, 20, "random"))
STEP_KEYS = ("rec_current", "visited_time", "cost_current", "cost_bsf", "reward", "rec_best", "i")
RESET_KEYS = ("cost_current", "cost_bsf", "rec_current", "rec_best", "visited_time", "i", "done",
              "terminated")


def case_name(k, n, init):
    return f"k{k}n{n}_{init}"


def small(t):
    """Node indices and visiting times fit a byte (N <= 65)."""
    if t.dtype == torch.int64 and t.numel() and 0 <= int(t.min()) and int(t.max()) < 256:
        return t.to(torch.uint8)
    return t


def run_case(mods, k, n, init, seed, ties=False):
    TD = reference.TensorDict
    Env = mods["rl4co.envs.routing.tsp.env"].TSPkoptEnv
    env = Env(generator_params=dict(num_loc=n, init_sol_type=init), k_max=k)
    torch.manual_seed(seed)
    locs = torch.rand(B, n, 2)
    td = env.reset(TD({"locs": locs}, batch_size=[B]), batch_size=[B])
    out = {"locs": locs, "seed": seed, "k_max": k}
    for key in RESET_KEYS:
        out["reset_" + key] = td[key].clone()
    steps = {key: [] for key in STEP_KEYS + ("action", "margin")}
    for _ in range(T):
        before_rec, before_bsf = td["rec_current"].clone(), td["cost_bsf"].clone()
        action = env._random_action(td).clone()
        td = env._step(td)
        same = (td["rec_current"] == before_rec).all(1)
        margin = (td["cost_current"] - before_bsf).abs() / before_bsf
        margin = torch.where(same, torch.full_like(margin, float("inf")), margin)
        if not ties and bool((margin < MARGIN).any()):
            return None
        steps["action"].append(action)
        steps["margin"].append(margin.clamp(max=1e30))
        for key in STEP_KEYS:
            steps[key].append(td[key].clone())
    for key, rows in steps.items():
        out["step_" + key] = torch.stack(rows)
    out["best_solution"] = env.get_best_solution(td)
    out["current_solution"] = env.get_current_solution(td)
    out["costs_best"] = env.get_costs(locs, td["rec_best"])
    tour = torch.rand(B, n).argsort(1)
    out["tour"] = tour
    out["linked_list"] = env._get_linked_list_solution(tour)
    td = env.step_to_solution(td, out["linked_list"])
    for key in STEP_KEYS:
        out["to_solution_" + key] = td[key].clone()
    if k == 2:
        out["mask"] = env.get_mask(td)
    else:
        try:
            env.get_mask(td)
            raise RuntimeError("the reference returned a mask in k-opt mode")
        except AssertionError as exc:
            out["mask_error"] = str(exc)
    try:
        env._get_reward(td, None)
        raise RuntimeError("the reference computed an episode reward")
    except NotImplementedError as exc:
        out["get_reward_error"] = str(exc)
    return out


def record(mods):
    rec = {}
    for k, n, init in CASES:
        seed = 1000 * k + n + (500 if init == "greedy" else 0)
        out = None
        for _ in range(MAX_REDRAWS):
            out = run_case(mods, k, n, init, seed, ties=(k, n, init) in TIES)
            if out is not None:
                break
            seed += 100000
        if out is None:
            raise RuntimeError(f"{case_name(k, n, init)}: no seed among {MAX_REDRAWS} is clear")
        for name, value in out.items():
            if isinstance(value, torch.Tensor):
                value = small(value.detach().cpu().contiguous()).numpy().copy()
            rec[f"kopt/{case_name(k, n, init)}/{name}"] = np.asarray(value)
    return rec


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    out_dir = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(
        os.path.dirname(os.path.abspath(__file__)), "kopt")
    os.makedirs(out_dir, exist_ok=True)
    mods = reference.load()
    torch.set_num_threads(1)
    rec = record(mods)
    path = os.path.join(out_dir, "ref_kopt.npz")
    write_npz(path, rec)
    print(path, os.path.getsize(path), "bytes,", len(rec), "arrays")


if __name__ == "__main__":
    main()
