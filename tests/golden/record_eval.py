"""Recorder of tests/golden/eval/ref_eval.npz (a folder of its own: the ``ref_*.npz``
beside this file are the groups of ``oracle.record_reference``, whose set
tests/test_golden.py pins): what the reference's own evaluators
(``rl4co/tasks/eval.py``) return, driven by a scripted policy that hands back seeded action
rows.  Runs in a process of its own (``python tests/golden/record_eval.py [--out DIR]``):
``oracle.reference.load()`` imports the reference's modules from a checkout through
stand-ins, ``rl4co.tasks`` is added as a package path, and nothing of the reference is
copied -- only what its functions return is stored.

Keys are ``<function>/<case>/<name>``.  Action rows are stored as uint8 (node indices below
256) to keep the archive small.  In every recorded instance the reference's best reward
exceeds its second best by more than ``1e-4 * |best|`` (checked here; the seed is re-drawn
otherwise and stored with the margins), so that a 1e-5 relative reward difference cannot
flip a winner: a condition on the inputs, not a tolerance of the tests.
"""
import importlib
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import reference  # noqa: E402
from oracle.record_reference import write_npz  # noqa: E402

MARGIN = 1e-4
BATCH_SIZE_CASES = ((10, None, None), (20, None, None), (100, None, None), (100, 8, None),
                    (None, 8, None), (None, None, 1280), (50, 8, None), (1000, 8, None),
                    (None, None, 16), (19, 3, None))


class ScriptedPolicy:
    """Returns the preset ``[K*B, T]`` action rows of the batches in order."""

    def __init__(self, rows):
        self.rows = list(rows)
        self.calls = 0
        self._p = torch.zeros(1)

    def parameters(self):
        return iter([self._p])

    def __call__(self, td, **kwargs):
        rows = self.rows[self.calls]
        self.calls += 1
        return {"actions": rows, "reward": torch.zeros(rows.shape[0])}


def tsp_rows(g, e, n):
    return torch.rand(e, n, generator=g).argsort(1)


def cvrp_rows(g, demand_int, cap, k):
    """Feasible rows [k*B, T]: customers in seeded order, back to the depot when the next
    demand would exceed the capacity; zero-padded to the longest row."""
    b, n = demand_int.shape
    rows = []
    for e in range(k * b):
        d = demand_int[e % b]
        order = (torch.rand(n, generator=g).argsort() + 1).tolist()
        row, used = [], 0
        for c in order:
            if used + int(d[c - 1]) > cap:
                row.append(0)
                used = 0
            row.append(c)
            used += int(d[c - 1])
        rows.append(row)
    t = max(len(r) for r in rows)
    return torch.tensor([r + [0] * (t - len(r)) for r in rows], dtype=torch.int64)


def margins(env, td_init, rows, k, batchify, unbatchify):
    """Per instance: (best - second best) / |best| of the reference's rewards (inf for
    k = 1)."""
    rew = env.get_reward(batchify(td_init, k) if k > 1 else td_init, rows)
    r = unbatchify(rew, k) if k > 1 else rew[:, None]
    if k == 1:
        return torch.full((r.shape[0],), float("inf"))
    top = r.topk(2, dim=1).values
    return (top[:, 0] - top[:, 1]) / top[:, 0].abs()


def record(mods, ev):
    ops = mods["rl4co.utils.ops"]
    TD = reference.TensorDict
    TSPEnv = mods["rl4co.envs.routing.tsp.env"].TSPEnv
    CVRPEnv = mods["rl4co.envs.routing.cvrp.env"].CVRPEnv
    rec = {}

    def put(fn, case, **arrays):
        for name, value in arrays.items():
            if isinstance(value, torch.Tensor):
                value = value.detach().cpu().contiguous().numpy().copy()
            rec[f"{fn}/{case}/{name}"] = np.asarray(value)

    def inner_case(env, make_inputs, make_rows, evaluator, k, case, seed):
        """Run ``evaluator._inner`` on seeded inputs whose winners are clear."""
        while True:
            g = torch.Generator().manual_seed(seed)
            inp = make_inputs(g)
            b = next(iter(inp.values())).shape[0]
            td = env.reset(TD(dict(inp), batch_size=[b]), batch_size=[b])
            rows = make_rows(g, inp, k * b)
            m = margins(env, td.clone(), rows, k, ops.batchify, ops.unbatchify)
            if bool((m > MARGIN).all()):
                break
            seed += 1000
        torch.manual_seed(seed)  # the symmetric augmentation's draw (its output is unused)
        actions, rewards = evaluator._inner(ScriptedPolicy([rows]), td)
        put(type(evaluator).__name__ + "._inner", case, **inp, rows=rows.to(torch.uint8),
            candidates=k, out_actions=actions.to(torch.uint8), out_rewards=rewards,
            margins=m.clamp(max=1e30), seed=seed)

    # -- TSP ---------------------------------------------------------------------------
    def tsp_inputs(b, n):
        return lambda g: {"locs": torch.rand(b, n, 2, generator=g)}

    def tsp_make(n):
        return lambda g, inp, e: tsp_rows(g, e, n)

    env = TSPEnv(generator_params=dict(num_loc=7), seed=0)
    inner_case(env, tsp_inputs(3, 7), tsp_make(7), ev.GreedyEval(env, progress=False), 1,
               "tsp_b3n7", 11)
    inner_case(env, tsp_inputs(3, 7), tsp_make(7),
               ev.AugmentationEval(env, num_augment=8, progress=False), 8, "tsp_b3n7", 12)
    inner_case(env, tsp_inputs(3, 7), tsp_make(7),
               ev.GreedyMultiStartEval(env, num_starts=7, progress=False), 7, "tsp_b3n7", 13)
    inner_case(env, tsp_inputs(3, 7), tsp_make(7),
               ev.GreedyMultiStartAugmentEval(env, num_starts=7, num_augment=8, progress=False),
               56, "tsp_b3n7", 14)
    env = TSPEnv(generator_params=dict(num_loc=20), seed=0)
    inner_case(env, tsp_inputs(4, 20), tsp_make(20),
               ev.GreedyMultiStartAugmentEval(env, num_starts=20, num_augment=8, progress=False),
               160, "tsp_b4n20", 15)

    # -- CVRP --------------------------------------------------------------------------
    env = CVRPEnv(generator_params=dict(num_loc=10), seed=0)
    cap = int(env.generator.capacity)
    state = {}

    def cvrp_inputs(g):
        state["demand_int"] = torch.randint(1, 10, (3, 10), generator=g)
        return {"locs": torch.rand(3, 10, 2, generator=g), "depot": torch.rand(3, 2, generator=g),
                "demand": state["demand_int"].float() / cap}

    def cvrp_make(g, inp, e):
        return cvrp_rows(g, state["demand_int"], cap, e // 3)

    inner_case(env, cvrp_inputs, cvrp_make,
               ev.AugmentationEval(env, num_augment=8, progress=False), 8, "cvrp_b3n10", 21)
    inner_case(env, cvrp_inputs, cvrp_make,
               ev.GreedyMultiStartAugmentEval(env, num_starts=10, num_augment=8, progress=False),
               80, "cvrp_b3n10", 22)

    # -- one whole __call__: 5 instances at batch size 2 -----------------------------------
    env = TSPEnv(generator_params=dict(num_loc=7), seed=0)
    seed = 31
    while True:
        g = torch.Generator().manual_seed(seed)
        locs = torch.rand(5, 7, 2, generator=g)
        batches = [locs[0:2], locs[2:4], locs[4:5]]
        rows = [tsp_rows(g, 7 * x.shape[0], 7) for x in batches]
        ms = []
        for x, r in zip(batches, rows):
            td = env.reset(TD({"locs": x}, batch_size=[x.shape[0]]), batch_size=[x.shape[0]])
            ms.append(margins(env, td, r, 7, ops.batchify, ops.unbatchify))
        if bool((torch.cat(ms) > MARGIN).all()):
            break
        seed += 1000
    loader = [TD({"locs": x.clone()}, batch_size=[x.shape[0]]) for x in batches]
    out = ev.GreedyMultiStartEval(env, num_starts=7, progress=False)(ScriptedPolicy(rows), loader)
    put("EvalBase.__call__", "tsp_d5n7_bs2", locs=locs, rows=torch.cat(rows).to(torch.uint8),
        candidates=7, batch_size=2, out_rewards=out["rewards"], out_avg_reward=out["avg_reward"],
        margins=torch.cat(ms), seed=seed)

    # -- get_automatic_batch_size ----------------------------------------------------------
    for starts, augment, samples in BATCH_SIZE_CASES:
        fn = types.SimpleNamespace(**{k: v for k, v in (("num_starts", starts),
                                                        ("num_augment", augment),
                                                        ("samples", samples)) if v is not None})
        put("get_automatic_batch_size", f"s{starts}_a{augment}_n{samples}",
            num_starts=-1 if starts is None else starts,
            num_augment=-1 if augment is None else augment,
            samples=-1 if samples is None else samples, out=ev.get_automatic_batch_size(fn))
    return rec


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    out_dir = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(
        os.path.dirname(os.path.abspath(__file__)), "eval")
    mods = reference.load()
    reference._module("rl4co.tasks").__path__ = [os.path.join(reference.reference_path(),
                                                              "rl4co", "tasks")]
    ev = importlib.import_module("rl4co.tasks.eval")
    torch.set_num_threads(1)
    rec = record(mods, ev)
    path = os.path.join(out_dir, "ref_eval.npz")
    write_npz(path, rec)
    print(path, os.path.getsize(path), "bytes,", len(rec), "arrays")


if __name__ == "__main__":
    main()
