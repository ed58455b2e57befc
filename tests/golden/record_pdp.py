"""Recorder of tests/golden/pdp/ref_pdp.npz (a folder of its own: tests/test_golden.py pins
the ``ref_*.npz`` set beside this file): what the reference's own ``PDPEnv`` and
``PDPGenerator`` (``rl4co/envs/routing/pdp/``) return over seeded episodes.  Runs in a
process of its own (``python tests/golden/record_pdp.py [--out DIR]``):
``oracle.reference.load()`` imports the reference's modules from a checkout through
stand-ins, and this file adds the two that loader lacks for PDP (a package path for
``rl4co.envs.routing.pdp`` and a stand-in for its ``render`` module).  Nothing of the
reference is copied -- only arrays and key names are stored, node indices as uint8, masks and
the two sets bit-packed.

Keys are ``pdp/<case>/<name>`` for what a case's policies share (the generator's output from
its seed, the reset state) and ``pdp/<case>/<policy>/<name>`` per policy; per-step arrays are
stacked ``[T, ...]``.  The reset ``locs`` are not stored: they are ``cat(depot, locs)``.

Policies, drawn here and stored: ``random`` = ``torch.multinomial`` on the mask, seeded;
``nearest`` = argmin of the distance from the current node over the mask.  The case
``n20b4_multistart`` is one POMO episode: the reset td batchified ``get_num_starts`` times, the
first action ``select_start_nodes``'s (a pickup, from the reset state whose mask holds the
depot only), then ``random``.

The step compares no floats, so there is no margin condition on the inputs; only
``get_reward`` is float.  Two tampered action rows per case and policy, with the
``AssertionError`` text the reference raises: in row TAMPER_ROW the first pickup of the tour
swapped with its delivery, and one node written over its neighbour (a duplicate).
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

TAMPER_ROW = 1
CASES = [(2, 16), (4, 16), (20, 16), (50, 16), (70, 8)]
MULTISTART = (20, 4)
POLICIES = ("random", "nearest")
STEP_KEYS = ("action_mask", "available", "to_deliver", "current_node", "i", "done", "reward")
PACKED = ("action_mask", "available", "to_deliver")
GEN_KEYS = ("locs", "depot")


def case_name(n, b):
    return f"n{n}b{b}"


def load_env_module():
    mods = reference.load()

    def unavailable(*args, **kwargs):
        raise RuntimeError("not available in the reference loader")

    pkg = "rl4co.envs.routing.pdp"
    reference._module(pkg).__path__ = [os.path.join(reference.reference_path(), *pkg.split("."))]
    reference._module(pkg + ".render", render=unavailable, render_improvement=unavailable)
    mods[pkg + ".env"] = importlib.import_module(pkg + ".env")
    return mods


def pack(t):
    """A 0/1 tensor bit-packed along its last axis."""
    return np.packbits(t.to(torch.uint8).numpy(), axis=-1)


def small(t):
    if t.dtype == torch.int64 and t.numel() and 0 <= int(t.min()) and int(t.max()) < 256:
        return t.to(torch.uint8)
    return t


def choose(td, policy, gen):
    mask = td["action_mask"]
    assert bool(mask.any(-1).all())
    if policy == "random":
        return torch.multinomial(mask.float(), 1, generator=gen).squeeze(-1)
    locs = td["locs"]
    cur = locs.gather(1, td["current_node"][..., None].expand(-1, 1, 2))
    dist = (locs - cur).norm(p=2, dim=-1)
    return dist.masked_fill(~mask, float("inf")).argmin(-1)


def run_policy(env, td, policy, seed, first=None):
    """One episode from the reset td -> the per-step states, the reward and the tampered
    rows."""
    gen = torch.Generator().manual_seed(seed + 7)
    steps = {key: [] for key in STEP_KEYS + ("action",)}
    while not bool(td["done"].all()):
        if first is not None and not steps["action"]:
            action = first
        else:
            action = choose(td, policy, gen)
        td["action"] = action
        td = env._step(td)
        steps["action"].append(action.clone())
        for key in STEP_KEYS:
            steps[key].append(td[key].clone())
    out = {}
    for key, rows in steps.items():
        stacked = torch.stack(rows)
        out["step_" + key] = pack(stacked) if key in PACKED else stacked
    actions = torch.stack(steps["action"], 1)
    out["get_reward"] = env.get_reward(td, actions)  # runs the reference's validity check
    out.update(tamper(env, td, actions))
    return out


def tamper(env, td, actions):
    """Row TAMPER_ROW with its first pickup and that pickup's delivery swapped; and with one
    node written over its neighbour."""
    r = TAMPER_ROW
    h = (td["locs"].shape[-2] - 1) // 2
    row = actions[r].tolist()
    pickup = next(a for a in row if 1 <= a <= h)
    swapped = actions.clone()
    swapped[r, row.index(pickup)], swapped[r, row.index(pickup + h)] = pickup + h, pickup
    doubled = actions.clone()
    doubled[r, -1] = doubled[r, -2]
    out = {}
    for name, bad in (("swap", swapped), ("double", doubled)):
        try:
            env.check_solution_validity(td, bad)
            raise RuntimeError("the reference accepted the tampered row")
        except AssertionError as exc:
            out[f"tamper_{name}_actions"] = bad
            out[f"tamper_{name}_message"] = str(exc)
    return out


def run_case(mods, n, b, seed):
    env = mods["rl4co.envs.routing.pdp.env"].PDPEnv(generator_params=dict(num_loc=n))
    torch.manual_seed(seed)
    inst = env.generator(b)
    out = {"seed": seed}
    for key in GEN_KEYS:
        out["gen_" + key] = inst[key].clone()
    for policy in POLICIES:
        td = env.reset(inst.clone(), batch_size=[b])
        if policy == POLICIES[0]:
            for key in ("current_node", "i", "done"):
                out["reset_" + key] = td[key].clone()
            for key in PACKED:
                out["reset_" + key] = pack(td[key])
        for key, value in run_policy(env, td, policy, seed).items():
            out[f"{policy}/{key}"] = value
    return out


def run_multistart(mods, n, b, seed):
    batchify = mods["rl4co.utils.ops"].batchify
    env = mods["rl4co.envs.routing.pdp.env"].PDPEnv(generator_params=dict(num_loc=n))
    torch.manual_seed(seed)
    inst = env.generator(b)
    td = env.reset(inst.clone(), batch_size=[b])
    starts = env.get_num_starts(td)
    first = env.select_start_nodes(td, starts)
    td = batchify(td, starts)
    out = {"seed": seed, "num_starts": starts, "start_nodes": first.clone()}
    for key in GEN_KEYS:
        out["gen_" + key] = inst[key].clone()
    for key, value in run_policy(env, td, "random", seed, first=first).items():
        out["random/" + key] = value
    return out


def record(mods):
    rec = {}

    def keep(case, out):
        for name, value in out.items():
            if isinstance(value, torch.Tensor):
                value = small(value.detach().cpu().contiguous()).numpy().copy()
            rec[f"pdp/{case}/{name}"] = np.asarray(value)

    for n, b in CASES:
        keep(case_name(n, b), run_case(mods, n, b, 3000 + n))
    n, b = MULTISTART
    keep(case_name(n, b) + "_multistart", run_multistart(mods, n, b, 3500 + n))
    return rec


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    out_dir = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(
        os.path.dirname(os.path.abspath(__file__)), "pdp")
    os.makedirs(out_dir, exist_ok=True)
    mods = load_env_module()
    torch.set_num_threads(1)
    rec = record(mods)
    path = os.path.join(out_dir, "ref_pdp.npz")
    write_npz(path, rec)
    print(path, os.path.getsize(path), "bytes,", len(rec), "arrays")


if __name__ == "__main__":
    main()
