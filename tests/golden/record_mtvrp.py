"""Recorder of tests/golden/mtvrp/ref_mtvrp.npz (a folder of its own: tests/test_golden.py
pins the ``ref_*.npz`` set beside this file): what the reference's own ``MTVRPEnv`` and
``MTVRPGenerator`` (``rl4co/envs/routing/mtvrp/``) return over seeded episodes.  Runs in a
process of its own (``python tests/golden/record_mtvrp.py [--out DIR]``):
``oracle.reference.load()`` imports the reference's modules from a checkout through
stand-ins, and this file adds the two that loader lacks for MTVRP (a package path for
``rl4co.envs.routing.mtvrp`` and a no-op ``rl4co.data.utils.save_tensordict_to_npz``).
Nothing of the reference is copied -- only arrays and key names are stored, node indices as
uint8, masks and visited sets bit-packed.

Keys are ``mtvrp/<case>/<name>`` for what a case's policies share (the kept rows of the
generator's pool -- at N = 20 the first two clear rows of each of the 16 variant names, else
clear rows taken round-robin over the variant names -- the reset state, the variant names)
and ``mtvrp/<case>/<policy>/<name>`` per policy; per-step arrays are stacked ``[T, ...]``, T
cut where the last kept row is done.
``mtvrp/gen_<preset>/<key>`` is the generator's whole output, unfiltered, at B = 8, N = 10.

Policies, drawn here on the whole pool and stored: ``random`` = ``torch.multinomial`` on the
mask, seeded; ``nearest`` = argmin of the reference's own ``get_distance`` over the mask.

Condition on the inputs (not a tolerance of the tests).  A pool of POOL rows is drawn with
``variant_preset="all"`` and only *clear* rows are kept: rows for which, over both policies'
whole episodes, (1) every one of the mask's three float compares -- ``arrival < late``
(reach), ``(max(arrival, early) + service + d_j0 / speed) * ~open < late_depot`` (depot_ok)
and ``length + d_ij + d_j0 * ~open > limit`` (over) -- keeps ``|lhs - rhs| >= MARGIN`` on
every not-yet-visited column of every mask call, a compare with an infinite side counting as
clear, and (2) no mask call of the row is empty.

MARGIN.  The product's leg differs from torch's ``norm`` by at most one ulp of a value below
sqrt(2), 1.2e-7.  Times and lengths stay below 8 (``max_time`` 4.6, ``distance_limit`` 3 plus
one leg), where an f32 addition rounds by at most half an ulp, 2.4e-7, so the two sides'
sums may part by one ulp, 4.8e-7, per addition.  A step adds into the time twice (the leg,
the service time) and into the length once: at most 1.2e-7 + 2 * 4.8e-7 = 1.1e-6 of drift
per leg.  A route ends at the depot, which resets both sums; its legs are bounded by the
capacity: the smallest demand is 1 and the largest capacity here 50 (N = 100), so 51 legs,
5.6e-5, plus the compare's own three operations, 1.5e-6.  MARGIN = 1e-3 keeps a seventeenfold
reserve over that 5.8e-5 (at least eightfold is asked).  It and the smallest kept gap are
stored.

Tampered rows, one per case and kind, with the ``AssertionError`` text the reference raises
on the kept rows: ``deadline`` -- in the first kept row without time windows the window end of
the row's first customer is set to half its depot distance, below the validity scan's
arrival; ``limit`` -- the first kept row's distance limit is set to half its first leg;
``repeat`` -- the first kept row's second action is replaced by its first, a repeated
customer.
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

MARGIN = 1e-3
POOL = 256
CASES = [(5, 8), (20, 32), (50, 16), (100, 8)]  # (N, kept rows)
POLICIES = ("random", "nearest")
GEN_KEYS = ("locs", "demand_backhaul", "demand_linehaul", "distance_limit", "time_windows",
            "service_time", "vehicle_capacity", "capacity_original", "open_route", "speed")
STATE_KEYS = ("current_node", "current_time", "current_route_length",
              "used_capacity_linehaul", "used_capacity_backhaul", "done")
GEN_PRESETS = ("all", "single_feat", "single_feat_otw", "cvrp", "vrptw", "ovrpbltw", None)
VARIANTS = ("CVRP", "OVRP", "VRPB", "VRPL", "VRPTW", "OVRPTW", "OVRPB", "OVRPL", "VRPBL",
            "VRPBTW", "VRPLTW", "OVRPBL", "OVRPBTW", "OVRPLTW", "VRPBLTW", "OVRPBLTW")


def load_env_module():
    mods = reference.load()
    sys.modules["rl4co.data.utils"].save_tensordict_to_npz = lambda *args, **kwargs: None
    pkg = "rl4co.envs.routing.mtvrp"
    reference._module(pkg).__path__ = [os.path.join(reference.reference_path(), *pkg.split("."))]
    mods[pkg + ".env"] = importlib.import_module(pkg + ".env")
    mods[pkg + ".generator"] = sys.modules[pkg + ".generator"]
    return mods


def pack(t):
    """A 0/1 tensor bit-packed along its last axis."""
    return np.packbits(t.to(torch.uint8).numpy(), axis=-1)


def small(t):
    if t.dtype == torch.int64 and t.numel() and 0 <= int(t.min()) and int(t.max()) < 256:
        return t.to(torch.uint8)
    return t


def row_gaps(td):
    """Per row, the smallest |lhs - rhs| of the three compares of the td's mask call over
    the not-yet-visited columns; +inf where a side is infinite."""
    get_distance = sys.modules["rl4co.utils.ops"].get_distance
    locs = td["locs"]
    cur = locs[torch.arange(locs.shape[0]), td["current_node"]]
    d_ij = get_distance(cur[:, None, :], locs)
    d_j0 = get_distance(locs, locs[:, 0:1, :])
    early, late = td["time_windows"][..., 0], td["time_windows"][..., 1]
    closed = ~td["open_route"]
    arrival = td["current_time"] + d_ij / td["speed"]
    pairs = ((arrival, late),
             ((torch.max(arrival, early) + td["service_time"] + d_j0 / td["speed"]) * closed,
              late[:, 0:1].expand_as(late)),
             (td["current_route_length"] + d_ij + d_j0 * closed,
              td["distance_limit"].expand_as(late)))
    gap = torch.full(late.shape, float("inf"))
    for lhs, rhs in pairs:
        g = (lhs - rhs).abs()
        finite = torch.isfinite(lhs) & torch.isfinite(rhs)
        g = torch.where(finite, g, torch.full_like(g, float("inf")))
        gap = torch.minimum(gap, g)
    gap = gap.masked_fill(td["visited"], float("inf"))
    return gap.min(-1).values


def run_policy(env, td, policy, seed):
    """One episode of the whole pool: (per-step states, actions [T, B], per-row smallest
    gap, per-row "some mask call was empty")."""
    get_distance = sys.modules["rl4co.utils.ops"].get_distance
    b = td["locs"].shape[0]
    gen = torch.Generator().manual_seed(seed + 7)
    gaps = row_gaps(td)
    empty = ~td["action_mask"].any(-1)
    steps = {key: [] for key in STATE_KEYS + ("action", "action_mask", "visited")}
    done = torch.zeros(b, dtype=torch.bool)
    while not bool(done.all()):
        mask = td["action_mask"]
        pick = mask.clone()
        pick[~mask.any(-1), 0] = True  # an empty row (not kept) goes to the depot
        if policy == "random":
            action = torch.multinomial(pick.float(), 1, generator=gen).squeeze(-1)
        else:
            cur = td["locs"][torch.arange(b), td["current_node"]]
            dist = get_distance(cur[:, None, :], td["locs"])
            action = dist.masked_fill(~pick, float("inf")).argmin(-1)
        td["action"] = action
        td = env._step(td)
        done = td["done"]
        gaps = torch.minimum(gaps, row_gaps(td))
        empty |= ~td["action_mask"].any(-1)
        steps["action"].append(action.clone())
        for key in steps:
            if key != "action":
                steps[key].append(td[key].clone())
    return {k: torch.stack(v) for k, v in steps.items()}, gaps, empty


def message_of(env, td, actions):
    try:
        env.check_solution_validity(td, actions)
    except AssertionError as exc:
        return str(exc)
    raise RuntimeError("the reference accepted the tampered row")


def tampers(env, td, actions, has_tw):
    """The three tampered rows of the kept td (reset state) and the reference's messages."""
    get_distance = sys.modules["rl4co.utils.ops"].get_distance
    out = {}
    r = int((~has_tw).nonzero()[0])  # fails loudly when every kept row has windows
    a0 = int(actions[r, 0])
    assert a0 != 0
    end = get_distance(td["locs"][r, 0], td["locs"][r, a0]) * 0.5
    bad = td.clone()
    bad["time_windows"][r, a0, 1] = end
    out.update(deadline_row=r, deadline_node=a0, deadline_end=bad["time_windows"][r, a0, 1].clone(),
               deadline_message=message_of(env, bad, actions))
    a0 = int(actions[0, 0])
    assert a0 != 0
    bad = td.clone()
    bad["distance_limit"][0, 0] = get_distance(td["locs"][0, 0], td["locs"][0, a0]) * 0.5
    out.update(limit_row=0, limit_value=bad["distance_limit"][0, 0].clone(),
               limit_message=message_of(env, bad, actions))
    acts = actions.clone()
    assert int(acts[0, 0]) != 0
    acts[0, 1] = acts[0, 0]
    out.update(repeat_row=0, repeat_message=message_of(env, td, acts))
    return out


def run_case(mods, n, keep, seed):
    env_mod = mods["rl4co.envs.routing.mtvrp.env"]
    env = env_mod.MTVRPEnv(generator_params=dict(num_loc=n, variant_preset="all"),
                           check_solution=True)
    torch.manual_seed(seed)
    pool = env.generator(POOL)
    names = np.array(env.get_variant_names(pool))
    runs, gaps, empty = {}, torch.full((POOL,), float("inf")), torch.zeros(POOL, dtype=torch.bool)
    reset = None
    for policy in POLICIES:
        td = env.reset(pool.clone(), batch_size=[POOL])
        if reset is None:
            reset = {k: td[k].clone() for k in STATE_KEYS[:-1] + ("action_mask", "visited")}
        runs[policy], g, e = run_policy(env, td, policy, seed)
        gaps, empty = torch.minimum(gaps, g), empty | e
    clear = ((gaps >= MARGIN) & ~empty).numpy()
    if n == 20:  # the first two clear rows of each of the 16 variant names
        rows = []
        for v in VARIANTS:
            mine = np.nonzero(clear & (names == v))[0]
            assert len(mine) >= 2, f"n{n}: fewer than two clear {v} rows in the pool"
            rows += mine[:2].tolist()
    else:  # round-robin over the variant names, so the kept rows mix the features
        mine = [np.nonzero(clear & (names == v))[0].tolist() for v in VARIANTS]
        rows = [m[k] for k in range(keep) for m in mine if k < len(m)][:keep]
    assert len(rows) == keep, f"n{n}: {len(rows)} clear rows, {keep} wanted"
    idx = torch.tensor(rows)
    out = {"seed": seed, "margin": np.float64(MARGIN), "min_gap": float(gaps[idx].min()),
           "clear_share": float(clear.mean()), "variant_names": names[rows]}
    for key in GEN_KEYS:
        out["gen_" + key] = pool[key][idx].clone()
    for key, value in reset.items():
        value = value[idx]
        out["reset_" + key] = pack(value) if key in ("action_mask", "visited") else value
    kept = pool[idx]
    has_tw = env.check_variants(kept)[1]
    for policy in POLICIES:
        steps = {k: v[:, idx] for k, v in runs[policy].items()}
        t_end = int(steps["done"].all(-1).float().argmax()) + 1  # the last kept row is done
        steps = {k: v[:t_end] for k, v in steps.items()}
        for key, value in steps.items():
            packed = key in ("action_mask", "visited")
            out[f"{policy}/step_{key}"] = pack(value) if packed else value
        actions = steps["action"].t().contiguous()
        td = env.reset(kept.clone(), batch_size=[keep])
        out[f"{policy}/get_reward"] = env.get_reward(td, actions)  # the reference's check is on
        for key, value in tampers(env, td, actions, has_tw).items():
            out[f"{policy}/tamper_{key}"] = value
    return out


def record_generator(mods):
    gen_mod = mods["rl4co.envs.routing.mtvrp.generator"]
    rec = {}
    for i, preset in enumerate(GEN_PRESETS):
        seed = 4200 + i
        torch.manual_seed(seed)
        gen = gen_mod.MTVRPGenerator(num_loc=10, variant_preset=preset,
                                     subsample=preset is not None)
        td = gen(8)
        name = f"mtvrp/gen_{preset if preset is not None else 'nosubsample'}/"
        rec[name + "seed"] = np.asarray(seed)
        for key in GEN_KEYS:
            rec[name + key] = td[key].clone().numpy()
    return rec


def record(mods):
    rec = record_generator(mods)
    for n, keep in CASES:
        out = run_case(mods, n, keep, 2000 + n)
        for name, value in out.items():
            if isinstance(value, torch.Tensor):
                value = small(value.detach().cpu().contiguous()).numpy().copy()
            rec[f"mtvrp/n{n}b{keep}/{name}"] = np.asarray(value)
    return rec


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    out_dir = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(
        os.path.dirname(os.path.abspath(__file__)), "mtvrp")
    os.makedirs(out_dir, exist_ok=True)
    mods = load_env_module()
    torch.set_num_threads(1)
    rec = record(mods)
    path = os.path.join(out_dir, "ref_mtvrp.npz")
    write_npz(path, rec)
    print(path, os.path.getsize(path), "bytes,", len(rec), "arrays")


if __name__ == "__main__":
    main()
