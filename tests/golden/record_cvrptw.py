"""Recorder of tests/golden/cvrptw/ref_cvrptw.npz (a folder of its own: tests/test_golden.py
pins the ``ref_*.npz`` set beside this file): what the reference's own ``CVRPTWEnv`` and
``CVRPTWGenerator`` (``rl4co/envs/routing/cvrptw/``) return over seeded episodes.  Runs in a
process of its own (``python tests/golden/record_cvrptw.py [--out DIR]``):
``oracle.reference.load()`` imports the reference's modules from a checkout through
stand-ins, and this file adds the three that loader lacks for CVRPTW (the Solomon loaders as
unavailable stubs, a package path for ``rl4co.envs.routing.cvrptw`` and a stand-in for its
``render``).  Nothing of the reference is copied -- only arrays and key names are stored,
node indices as uint8, masks and visited sets bit-packed.

Keys are ``cvrptw/<case>/<name>`` for what a case's policies share (the generator's output
from its seed, the reset state) and ``cvrptw/<case>/<policy>/<name>`` per policy; per-step
arrays are stacked ``[T, ...]``.  Per-step ``distances`` are kept for N <= 20 only; the
larger cases keep them at reset and at the last step.

Policies, drawn here and stored: ``random`` = ``torch.multinomial`` on the mask, seeded;
``nearest`` = argmin of the reference's own ``distances`` over the mask.

Condition on the inputs (not a tolerance of the tests): every compare ``current_time +
distances[k]`` against ``time_windows[k, 1]`` of a recorded episode (every column k of every
mask call, both policies) keeps ``|gap| >= 1e-2`` time units (``1e-2 / max_time`` with
``scale``).  The product's leg differs from torch's by at most 2 ulp of a value below 256
(3e-5) and each addition into a time below 512 rounds by at most 1.5e-5 on either side, so
the two sides drift apart by at most about 6e-5 per leg, 1.2e-3 over the ~20 legs of a route
before the depot resets the clock; the margin keeps an eightfold reserve.  The seed is
re-drawn (at most MAX_REDRAWS times) until a case is clear; a seed with a row that has no
feasible action is rejected too.  The seed and the smallest gap are stored.

One tampered row per case and policy: in row TAMPER_ROW the deadline of one visited customer
is lowered to 2 time units below the (truncated) arrival of the reference's own validity
scan -- the first customer of the row's route for which the window stays open -- and the
``AssertionError`` text the reference raises is stored.  With ``scale`` the scan's truncated
times are all 0, so its deadline test cannot fail; there the deadline is lowered to 2 units
below the window's start (which lies before any arrival) and the reference reports an
unfeasible window.  The reset ``locs`` are not stored: they are ``cat(depot, locs)``.
"""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import reference  # noqa: E402
from oracle.record_reference import write_npz  # noqa: E402

MARGIN = 1e-2
MAX_REDRAWS = 400
MAX_TIME = 480
TAMPER_ROW = 1
CASES = [(5, 16, False), (20, 16, False), (50, 16, False), (70, 8, False), (20, 16, True)]
POLICIES = ("random", "nearest")
STEP_KEYS = ("action_mask", "visited", "current_node", "done", "reward", "used_capacity",
             "current_loc", "current_time")
GEN_KEYS = ("locs", "depot", "demand", "capacity", "durations", "time_windows")


def case_name(n, b, scale):
    return f"n{n}b{b}" + ("_scale" if scale else "")


def load_env_module():
    mods = reference.load()

    def unavailable(*args, **kwargs):
        raise RuntimeError("not available in the reference loader")

    utils = sys.modules["rl4co.data.utils"]
    utils.load_solomon_instance = unavailable
    utils.load_solomon_solution = unavailable
    pkg = "rl4co.envs.routing.cvrptw"
    reference._module(pkg).__path__ = [os.path.join(reference.reference_path(), *pkg.split("."))]
    reference._module(pkg + ".render", render=unavailable)
    mods[pkg + ".env"] = importlib.import_module(pkg + ".env")
    return mods


def pack(t):
    """A 0/1 tensor bit-packed along its last axis."""
    return np.packbits(t.to(torch.uint8).numpy(), axis=-1)


def small(t):
    if t.dtype == torch.int64 and t.numel() and 0 <= int(t.min()) and int(t.max()) < 256:
        return t.to(torch.uint8)
    return t


def gap_of(td):
    """The smallest |current_time + distances - deadline| of the td's last mask call."""
    return float((td["current_time"] + td["distances"] - td["time_windows"][..., 1]).abs().min())


def run_policy(env, td, policy, n, margin, seed):
    """One episode from the reset td; None when a compare comes closer than the margin or
    a row has no feasible action."""
    b = td["locs"].shape[0]
    gen = torch.Generator().manual_seed(seed + 7)
    keep_dist = n <= 20
    steps = {key: [] for key in STEP_KEYS + ("action",) + (("distances",) if keep_dist else ())}
    min_gap = gap_of(td)
    while not bool(td["done"].all()):
        mask = td["action_mask"]
        if min_gap < margin or not bool(mask.any(-1).all()):
            return None
        if policy == "random":
            action = torch.multinomial(mask.float(), 1, generator=gen).squeeze(-1)
        else:
            action = td["distances"].masked_fill(~mask, float("inf")).argmin(-1)
        td["action"] = action
        td = env._step(td)
        min_gap = min(min_gap, gap_of(td))
        steps["action"].append(action.clone())
        for key in steps:
            if key != "action":
                steps[key].append(td[key].clone())
    if min_gap < margin:
        return None
    out = {"min_gap": min_gap}
    for key, rows in steps.items():
        stacked = torch.stack(rows)
        out["step_" + key] = pack(stacked) if key in ("action_mask", "visited") else stacked
    out["last_distances"] = td["distances"].clone()
    actions = torch.stack(steps["action"], 1)
    assert actions.shape == (b, len(steps["action"]))
    out["get_reward"] = env.get_reward(td, actions)  # runs the reference's validity check
    out.update(tamper(env, td, actions))
    return out


def tamper(env, td, actions):
    """Lower one deadline of row TAMPER_ROW below the validity scan's arrival there."""
    get_distance = sys.modules["rl4co.utils.ops"].get_distance
    r = TAMPER_ROW
    locs, tw, dur = td["locs"][r], td["time_windows"][r], td["durations"][r]
    scaled = tw.dtype.is_floating_point
    t, prev, pick = torch.zeros(()), 0, None
    first = None
    for a in actions[r].tolist():
        arrival = (t + get_distance(locs[prev], locs[a])).int()
        if a != 0:
            # with scale the scan's truncated times are all 0 and its deadline test cannot
            # fail: there the deadline goes 2 units below the window's start, not above it
            end = arrival - 2 if not scaled else ((tw[a, 0] * MAX_TIME).round() - 2) / MAX_TIME
            first = first if first is not None else (a, end)
            if bool(end > tw[a, 0] if not scaled else end >= 0) and pick is None:
                pick = (a, end)
        t = torch.max(arrival, tw[a, 0]) + dur[a]
        if a == 0:
            t = torch.zeros(())
        prev = a
    node, end = pick if pick is not None else first
    bad = td.clone()
    bad["time_windows"][r, node, 1] = end.to(tw.dtype)
    try:
        env.check_solution_validity(bad, actions)
        raise RuntimeError("the reference accepted the tampered row")
    except AssertionError as exc:
        message = str(exc)
    return {"tamper_node": node, "tamper_end": bad["time_windows"][r, node, 1].clone(),
            "tamper_message": message}


def run_case(mods, n, b, scale, seed):
    env_mod = mods["rl4co.envs.routing.cvrptw.env"]
    env = env_mod.CVRPTWEnv(generator_params=dict(num_loc=n, scale=scale))
    torch.manual_seed(seed)
    inst = env.generator(b)
    out = {"seed": seed}
    for key in GEN_KEYS:
        out["gen_" + key] = inst[key].clone()
    margin = MARGIN / MAX_TIME if scale else MARGIN
    gaps = []
    for policy in POLICIES:
        td = env.reset(inst.clone(), batch_size=[b])
        if policy == POLICIES[0]:
            for key in ("current_node", "current_time", "used_capacity",
                        "vehicle_capacity", "current_loc", "distances", "done"):
                out["reset_" + key] = td[key].clone()
            out["reset_action_mask"] = pack(td["action_mask"])
            out["reset_visited"] = pack(td["visited"])
        res = run_policy(env, td, policy, n, margin, seed)
        if res is None:
            return None
        gaps.append(res.pop("min_gap"))
        for key, value in res.items():
            out[f"{policy}/{key}"] = value
    out["min_gap"] = min(gaps)
    return out


def record(mods):
    rec = {}
    for n, b, scale in CASES:
        seed = 1000 + n + (500 if scale else 0)
        out = None
        for _ in range(MAX_REDRAWS):
            out = run_case(mods, n, b, scale, seed)
            if out is not None:
                break
            seed += 100000
        if out is None:
            raise RuntimeError(f"{case_name(n, b, scale)}: no seed among {MAX_REDRAWS} is clear")
        for name, value in out.items():
            if isinstance(value, torch.Tensor):
                value = small(value.detach().cpu().contiguous()).numpy().copy()
            rec[f"cvrptw/{case_name(n, b, scale)}/{name}"] = np.asarray(value)
    return rec


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    out_dir = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(
        os.path.dirname(os.path.abspath(__file__)), "cvrptw")
    os.makedirs(out_dir, exist_ok=True)
    mods = load_env_module()
    torch.set_num_threads(1)
    rec = record(mods)
    path = os.path.join(out_dir, "ref_cvrptw.npz")
    write_npz(path, rec)
    print(path, os.path.getsize(path), "bytes,", len(rec), "arrays")


if __name__ == "__main__":
    main()
