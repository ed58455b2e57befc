"""Recorder of tests/golden/op/ref_op.npz (a folder of its own: tests/test_golden.py pins the
``ref_*.npz`` set beside this file): what the reference's own ``OPEnv`` and ``OPGenerator``
(``rl4co/envs/routing/op/``) return over seeded episodes.  Runs in a process of its own
(``python tests/golden/record_op.py [--out DIR]``): ``oracle.reference.load()`` imports the
reference's modules from a checkout through stand-ins, and this file adds the two that loader
lacks for OP (a package path for ``rl4co.envs.routing.op`` and a stand-in for its ``render``
module).  Nothing of the reference is copied -- only arrays and key names are stored, node
indices as uint8, masks and ``visited`` bit-packed.

Keys are ``op/<case>/<name>`` for what a case's policies share (the generator's output from
its seed, the reset state) and ``op/<case>/<policy>/<name>`` per policy; per-step arrays are
stacked ``[T, ...]``.  The reset ``locs`` are not stored: they are ``cat(depot, locs)``.

Policies, drawn here and stored: ``random`` = ``torch.multinomial`` on the mask, seeded;
``nearest`` = the nearest open customer, else the depot.

A condition on the inputs, not a tolerance.  The product's leg differs from torch's ``norm``
by up to 2 ulp (include/co_env.h, CVRPTW), so a recorded mask binds the product only where the
length compare is not close.  For every live compare of an episode (a column that is
unvisited, not the depot, in a row not yet done) the recorder requires
``|tour_length + dist - max_length| >= 8 x (T + 2) x 7.2e-7`` with T the episode's steps: 7.2e-7 is 2 ulp of a leg below 2 plus one rounding on each side of a sum
below 8, the ``+ 2`` covers the compare's own add and the reset's ``max_length``, the 8 is the
reserve CVRPTW's recorder keeps.  The seed is re-drawn (at most 400 times) until both policies
of a case are clear; the seed and the smallest gap are stored.

Two tampered action rows per case and policy, with the ``AssertionError`` text the reference
raises: one customer written over its neighbour (``Duplicates``), and the untouched tours with
one row's ``max_length`` lowered by 0.5 (``Max length exceeded``; the row whose tour comes
closest to its budget -- a seed on which the reference still accepts it is re-drawn too).
"""
import importlib
import logging
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import reference  # noqa: E402
from oracle.record_reference import write_npz  # noqa: E402

# (N, B, prize_type)
CASES = [(5, 16, "dist"), (20, 16, "dist"), (50, 16, "dist"), (70, 8, "dist"),
         (20, 16, "unif"), (20, 16, "const")]
POLICIES = ("random", "nearest")
STEP_KEYS = ("action_mask", "visited", "current_node", "i", "done", "reward", "tour_length",
             "current_total_prize")
PACKED = ("action_mask", "visited")
GEN_KEYS = ("locs", "depot", "prize", "max_length")
RESET_KEYS = ("current_node", "i", "tour_length", "current_total_prize", "max_length", "prize")
UNIT = 7.2e-7
RESERVE = 8
MAX_DRAWS = 400


def case_name(n, b, prize_type):
    return f"n{n}b{b}_{prize_type}"


def load_env_module():
    mods = reference.load()

    def unavailable(*args, **kwargs):
        raise RuntimeError("not available in the reference loader")

    pkg = "rl4co.envs.routing.op"
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


def choose(td, policy, gen):
    mask = td["action_mask"]
    assert bool(mask.any(-1).all())
    if policy == "random":
        return torch.multinomial(mask.float(), 1, generator=gen).squeeze(-1)
    locs = td["locs"]
    cur = locs.gather(1, td["current_node"][..., None].expand(-1, 1, 2))
    dist = (locs - cur).norm(p=2, dim=-1)
    open_ = mask.clone()
    open_[:, 0] = False  # the depot only when no customer is open
    near = dist.masked_fill(~open_, float("inf")).argmin(-1)
    return torch.where(open_.any(-1), near, torch.zeros_like(near))


def live_gap(td, finished):
    """The smallest |tour_length + dist - max_length| over the live compares of a state."""
    locs = td["locs"]
    cur = locs.gather(1, td["current_node"][..., None].expand(-1, 1, 2))
    lhs = td["tour_length"][..., None] + (locs - cur).norm(p=2, dim=-1)
    live = ~td["visited"] & ~finished[:, None]
    live[:, 0] = False
    gap = (lhs - td["max_length"]).abs()[live]
    return float(gap.min()) if gap.numel() else float("inf")


def run_policy(env, td, policy, seed):
    """One episode from the reset td -> (the per-step states, the reward and the tampered
    rows; the smallest live gap; the steps)."""
    gen = torch.Generator().manual_seed(seed + 7)
    steps = {key: [] for key in STEP_KEYS + ("action",)}
    finished = torch.zeros(td["locs"].shape[0], dtype=torch.bool)
    gap = live_gap(td, finished)
    while not bool(finished.all()):
        action = choose(td, policy, gen)
        td["action"] = action
        td = env._step(td)
        finished = finished | td["done"]
        gap = min(gap, live_gap(td, finished))
        steps["action"].append(action.clone())
        for key in STEP_KEYS:
            steps[key].append(td[key].clone())
    out = {}
    for key, rows in steps.items():
        stacked = torch.stack(rows)
        out["step_" + key] = pack(stacked) if key in PACKED else stacked
    actions = torch.stack(steps["action"], 1)
    out["get_reward"] = env.get_reward(td, actions)  # runs the reference's validity check
    bad = tamper(env, td, actions)
    if bad is None:
        gap = -1.0  # not a usable seed
    else:
        out.update(bad)
    return out, gap, len(steps["action"])


def tamper(env, td, actions):
    """The first row with a customer, that customer written over its neighbour; and the
    untouched tours with ``max_length`` lowered by 0.5 in the row whose tour comes closest to
    its budget.  None when the reference accepts either (no row with a customer, or every
    tour more than 0.5 short of its budget): the caller draws another seed."""
    rows = actions.tolist()
    r = next((i for i, row in enumerate(rows) if any(row[:-1])), None)
    if r is None:
        return None
    k = next(t for t in range(len(rows[r]) - 1) if rows[r][t] != 0)
    doubled = actions.clone()
    doubled[r, k + 1] = doubled[r, k]
    pts = td["locs"].gather(1, actions[..., None].expand(-1, -1, 2))
    length = (pts - pts.roll(-1, 1)).norm(p=2, dim=-1).sum(-1)
    slack = (td["max_length"] + (td["locs"][:, :1] - td["locs"]).norm(p=2, dim=-1)
             - length[:, None]).min(-1)[0]
    short = td.clone()
    ml = short["max_length"].clone()
    ml[int(slack.argmin())] -= 0.5
    short["max_length"] = ml
    out = {"tamper_short_max_length": ml}
    for name, bad_td, bad in (("double", td, doubled), ("short", short, actions)):
        try:
            env.check_solution_validity(bad_td, bad)
            return None
        except AssertionError as exc:
            out[f"tamper_{name}_actions"] = bad
            out[f"tamper_{name}_message"] = str(exc)
    return out


def run_case(mods, n, b, prize_type, seed):
    """-> (the case's arrays, its smallest gap, its margin) for one seed."""
    env = mods["rl4co.envs.routing.op.env"].OPEnv(
        generator_params=dict(num_loc=n, prize_type=prize_type, prize_distribution="dist"),
        prize_type=prize_type)  # "dist": no prize sampler (torch refuses the default's
    # Uniform(1, 1)); _generate never draws from one
    # the reference's _generate reads self.device for "unif" and "const" and nothing sets
    # it: None is torch's default device
    env.generator.device = None
    torch.manual_seed(seed)
    inst = env.generator(b)
    out = {"seed": seed}
    for key in GEN_KEYS:
        out["gen_" + key] = inst[key].clone()
    gap, margin = float("inf"), 0.0
    for policy in POLICIES:
        td = env.reset(inst.clone(), batch_size=[b])
        if policy == POLICIES[0]:
            for key in RESET_KEYS:
                out["reset_" + key] = td[key].clone()
            for key in PACKED:
                out["reset_" + key] = pack(td[key])
        res, g, t_steps = run_policy(env, td, policy, seed)
        gap = min(gap, g)
        margin = max(margin, RESERVE * (t_steps + 2) * UNIT)
        for key, value in res.items():
            out[f"{policy}/{key}"] = value
    out["gap"], out["margin"] = gap, margin
    return out, gap, margin


def record(mods):
    rec = {}
    logging.disable(logging.WARNING)  # the generator's nearest-size notice, once a draw
    for n, b, prize_type in CASES:
        base = 4000 + n + {"dist": 0, "unif": 1000, "const": 2000}[prize_type]
        for draw in range(MAX_DRAWS):
            out, gap, margin = run_case(mods, n, b, prize_type, base + 10000 * draw)
            if gap >= margin:
                break
        else:
            raise RuntimeError(f"no clear seed for {(n, b, prize_type)}: shrink its batch")
        out["draws"] = draw + 1
        print(case_name(n, b, prize_type), "seed", out["seed"], "draws", draw + 1, "gap", gap,
              "margin", margin, "steps", out["random/step_action"].shape[0],
              out["nearest/step_action"].shape[0])
        for name, value in out.items():
            if isinstance(value, torch.Tensor):
                value = small(value.detach().cpu().contiguous()).numpy().copy()
            rec[f"op/{case_name(n, b, prize_type)}/{name}"] = np.asarray(value)
    return rec


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    out_dir = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(
        os.path.dirname(os.path.abspath(__file__)), "op")
    os.makedirs(out_dir, exist_ok=True)
    mods = load_env_module()
    torch.set_num_threads(1)
    rec = record(mods)
    path = os.path.join(out_dir, "ref_op.npz")
    write_npz(path, rec)
    print(path, os.path.getsize(path), "bytes,", len(rec), "arrays")


if __name__ == "__main__":
    main()
