"""Shared inputs and checks of tests/test_host_mtvrp.py (host build) and
tests/test_gpu_mtvrp.py (device): the recording tests/golden/mtvrp/ref_mtvrp.npz, seeded
mixed-variant instances with a random-feasible and a directed rollout of the restatement
(tests/mtvrp_ref.py; computed once per shape and shared), thin wrappers over the C ABI
entries, and the comparisons.  The restatement uses the product's own formulas (the header's
``dist``), so the product is held to it bit for bit whatever the compares' gaps; the
recording is the reference's own arithmetic and keeps the recorder's margin instead.  A
check takes the device it runs on: CPU tensors go to the host build, CUDA tensors to the
kernels, through the same ``_native.call``."""
import functools
import os

import numpy as np
import torch

import mtvrp_ref as ref
from cvrptw_cases import same_bits
from ref_recordings import check_close, check_equal

from rl4co_slap_amd import TensorDict, _native as nat
from rl4co_slap_amd.envs import MTVRPEnv, MTVRPGenerator

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mtvrp")
POLICIES = ("random", "nearest")
GEN_KEYS = ("locs", "demand_backhaul", "demand_linehaul", "distance_limit", "time_windows",
            "service_time", "vehicle_capacity", "capacity_original", "open_route", "speed")
GEN_PRESETS = ("all", "single_feat", "single_feat_otw", "cvrp", "vrptw", "ovrpbltw", None)
SHAPES = [(n, b) for n in (1, 5, 20, 63, 64, 70, 200) for b in (1, 3, 16, 257)]
# N + 1 on both sides of every switch of mt_launch: the lanes per row G (8 / 16 / 32 / 64 at
# 16, 32, 64) and the columns per lane U (2 / 4 / 8 / 16 at 128, 256, 512); B = 3
SWITCH_SIZES = (15, 16, 31, 32, 62, 63, 64, 127, 128, 255, 256, 511, 512)
# (N, B) of the directed rollouts, one per U >= 4 instantiation (and N = 300, 1023)
DIRECTED_SHAPES = [(128, 4), (256, 4), (300, 4), (512, 4), (1023, 4)]
STATE = ("cur", "time", "length", "used_l", "used_b", "visited", "action_mask")
SCALARS = ("vehicle_capacity", "speed", "distance_limit", "open_route")


# ------------------------------------------------------------------ the recording
@functools.lru_cache(maxsize=None)
def recording(directory=GOLDEN):
    with np.load(os.path.join(directory, "ref_mtvrp.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def recorded_cases():
    return sorted({k.split("/")[1] for k in recording() if not k.split("/")[1].startswith("gen_")})


def recorded(case, directory=GOLDEN):
    """One case: uint8 index arrays back as int64, packed bits unpacked to NC columns,
    strings as str / lists of str, 0-d numbers as Python numbers."""
    raw = {k.split("/", 2)[2]: v for k, v in recording(directory).items()
           if k.split("/")[1] == case}
    assert raw, case
    nc = raw["gen_locs"].shape[1] if "gen_locs" in raw else raw["locs"].shape[1]
    out = {}
    for name, v in raw.items():
        leaf = name.split("/")[-1]
        if v.dtype.kind == "U":
            out[name] = str(v) if v.ndim == 0 else v.tolist()
        elif leaf in ("reset_action_mask", "reset_visited", "step_action_mask", "step_visited"):
            out[name] = torch.from_numpy(np.unpackbits(v, axis=-1)[..., :nc].copy()).bool()
        elif v.ndim == 0 and v.dtype.kind in "iu":
            out[name] = int(v)
        elif v.ndim == 0:
            out[name] = float(v)
        else:
            t = torch.from_numpy(v.copy())
            out[name] = t.long() if t.dtype == torch.uint8 else t
    return out


def recorded_instance(r, device):
    return TensorDict({k: r["gen_" + k].clone().to(device) for k in GEN_KEYS},
                      batch_size=[r["gen_locs"].shape[0]])


def env_for(device, n=20, check=True):
    return MTVRPEnv(generator_params=dict(num_loc=n, variant_preset="all"), device=device,
                    check_solution=check)


def raises_prefix(fn, message, what):
    """``fn`` raises an AssertionError whose text equals the recorded one up to any colon."""
    try:
        fn()
    except AssertionError as exc:
        assert str(exc).split(":")[0] == message.split(":")[0], (what, str(exc), message)
    else:
        raise AssertionError(f"{what}: the tampered row raised nothing")


def check_recorded_case(case, policy, device):
    """The product's env on a recorded episode of the reference's: integers, masks, visited
    sets, ``done`` and the capacities bit for bit, ``current_time`` / ``current_route_length``
    / ``get_reward`` within 1e-5 relative; ``step_many`` equals the single steps with every
    recorded action feasible; each tampered row raises the recorded message."""
    r = recorded(case)
    b = r["gen_locs"].shape[0]
    env = env_for(device)
    td = env.reset(recorded_instance(r, device), batch_size=[b])
    assert env.get_variant_names(td) == r["variant_names"], case
    for key in ("current_node", "action_mask", "visited", "current_time", "current_route_length",
                "used_capacity_linehaul", "used_capacity_backhaul"):
        check_equal(td[key].cpu(), r["reset_" + key], f"{case} reset {key}")
    p = policy + "/"
    acts = r[p + "step_action"]
    for t in range(acts.shape[0]):
        td.set("action", acts[t].to(device))
        td = env.step(td)["next"]
        what = f"{case} {policy} step {t}"
        for key in ("action_mask", "visited", "current_node", "done", "used_capacity_linehaul",
                    "used_capacity_backhaul"):
            check_equal(td[key].cpu(), r[p + "step_" + key][t], f"{what} {key}")
        assert td["reward"].dtype == torch.float32 and not bool(td["reward"].any()), what
        for key in ("current_time", "current_route_length"):
            check_close(td[key].cpu(), r[p + "step_" + key][t], f"{what} {key}")
    actions = acts.t().contiguous().to(device)
    check_close(env.get_reward(td, actions).cpu(), r[p + "get_reward"], case + " get_reward")
    env.check_solution_validity(td, actions)  # the untampered rows raise nothing
    many = env.reset(recorded_instance(r, device), batch_size=[b])
    feasible, times, lengths = env.step_many(many, actions)
    assert bool(feasible.all()), case + ": a recorded action is infeasible for co_mtvrp_steps"
    for key in ("action_mask", "visited", "current_node", "done", "current_time",
                "current_route_length", "used_capacity_linehaul", "used_capacity_backhaul"):
        check_equal(many[key].cpu(), td[key].cpu(), f"{case} {policy} step_many {key}")
    check_close(times.cpu(), r[p + "step_current_time"].reshape(times.shape), case + " times")
    check_close(lengths.cpu(), r[p + "step_current_route_length"].reshape(lengths.shape),
                case + " lengths")
    # the tampered rows
    bad = td.clone()
    tw = bad["time_windows"].clone()
    row, node = r[p + "tamper_deadline_row"], r[p + "tamper_deadline_node"]
    tw[row, node, 1] = r[p + "tamper_deadline_end"]
    bad.set("time_windows", tw)
    raises_prefix(lambda: env.check_solution_validity(bad, actions),
                  r[p + "tamper_deadline_message"], f"{case} {policy} deadline")
    bad = td.clone()
    lim = bad["distance_limit"].clone()
    lim[r[p + "tamper_limit_row"], 0] = r[p + "tamper_limit_value"]
    bad.set("distance_limit", lim)
    raises_prefix(lambda: env.check_solution_validity(bad, actions),
                  r[p + "tamper_limit_message"], f"{case} {policy} limit")
    rep = actions.clone()
    rep[r[p + "tamper_repeat_row"], 1] = rep[r[p + "tamper_repeat_row"], 0]
    raises_prefix(lambda: env.check_solution_validity(td, rep), r[p + "tamper_repeat_message"],
                  f"{case} {policy} repeat")


def check_generator(preset):
    """The generator's whole output from the recorded seed, bit for bit."""
    r = recorded("gen_" + (preset if preset is not None else "nosubsample"))
    torch.manual_seed(r["seed"])
    td = MTVRPGenerator(num_loc=10, variant_preset=preset, subsample=preset is not None)([8])
    for key in GEN_KEYS:
        assert td[key].dtype == r[key].dtype, key
        check_equal(td[key], r[key], f"{preset} {key}")


# ------------------------------------------------------------------ seeded instances
@functools.lru_cache(maxsize=None)
def instance(n, b, seed=0):
    """A generated instance (CPU numpy arrays, the restatement's layout) that mixes all four
    flags per row: every row is drawn with every feature, then row r loses the open route,
    the windows, the limit and the backhauls by bits 0..3 of r + seed -- all 16 variants
    over 16 rows."""
    torch.manual_seed(9000 + 31 * n + b + seed)
    td = MTVRPGenerator(num_loc=n, variant_preset=None, subsample=False)([b])
    r = torch.arange(b) + seed
    td = MTVRPGenerator._default_open(td, (r & 1) != 0)
    td = MTVRPGenerator._default_time_window(td, (r & 2) != 0)
    td = MTVRPGenerator._default_distance_limit(td, (r & 4) != 0)
    td = MTVRPGenerator._default_backhaul(td, (r & 8) != 0)
    out = {k: td[k].numpy().copy() for k in ref.INSTANCE}
    for k in SCALARS:
        out[k] = out[k][:, 0]
    return out


def group_lanes(n):
    """The lanes that own a row of N customers (csrc/mtvrp.hip, mt_launch): lane sl holds
    the columns sl + G j, so column c sits in register slot c // G."""
    nc = n + 1
    return 8 if nc <= 16 else 16 if nc <= 32 else 32 if nc <= 64 else 64


def episode_len(n, b):
    """The full episode, cut to 40 steps at N = 200 on the larger batches and to 12 on the
    rows of 4 to 16 columns per lane (the same paths; the restatement's per-step cost grows
    with B * N).  A row that cannot finish keeps taking the depot, so every rollout is also
    cut at 3 N + 4 steps."""
    return 12 if n > 200 else 40 if n >= 200 and b > 16 else 3 * n + 4


@functools.lru_cache(maxsize=None)
def rollout(n, b, max_steps=None, directed=False):
    """The restatement's random-feasible episode: (states after reset and every step,
    actions [T, B]).  A row without a feasible customer takes the depot.  ``directed``: among
    the feasible columns a row prefers one whose register slot has not been its action yet,
    and every second row prefers column N, the last live one, above all."""
    st = ref.reset(instance(n, b))
    g = np.random.default_rng(n * 7 + b)
    states, actions = [st], []
    slot = np.arange(n + 1) // group_lanes(n)
    unseen = np.ones((b, int(slot[-1]) + 1), bool)
    last = (np.arange(n + 1) == n)[None, :] & (np.arange(b) % 2 == 0)[:, None]
    max_steps = episode_len(n, b) if max_steps is None else max_steps
    while not st.get("done", np.zeros(1, bool)).all() and len(actions) < max_steps:
        m = st["action_mask"]
        score = g.random(m.shape)
        if directed:
            score = score + 2.0 * unseen[:, slot] + 4.0 * last
        score = np.where(m, score, -1.0)
        a = np.where(m.any(1), score.argmax(1), 0).astype(np.int64)
        unseen[np.arange(b), slot[a]] = False
        st, bits = ref.step(st, a)
        assert bits == 0
        states.append(st)
        actions.append(a)
    return states, np.stack(actions)


def check_directed_inputs(n, b):
    """The condition on the inputs of a directed case, from the restatement's rollout alone:
    every register slot 0 .. ceil((N + 1) / G) - 1 is the action's at least once in the
    batch, and column N is visited in at least one row."""
    states, actions = rollout(n, b, None, True)
    g = group_lanes(n)
    slots = set((actions // g).ravel().tolist())
    want = set(range(-(-(n + 1) // g)))
    assert slots == want, f"n{n} b{b}: slots {sorted(want - slots)} are never the action"
    assert (actions == n).any() and states[-1]["visited"][:, n].any(), f"n{n} b{b}: column N"


def check_mixed_flags(n=20, b=16):
    """Every restatement batch mixes the four flags: 16 rows hold all 16 variants."""
    inst = instance(n, b)
    td = TensorDict({k: torch.from_numpy(inst[k] if k not in SCALARS else inst[k][:, None])
                     for k in ref.INSTANCE}, batch_size=[b])
    assert len(set(MTVRPEnv.get_variant_names(td))) == 16


# ------------------------------------------------------------------ the C ABI
def to_dev(inst, device):
    """The instance's arrays as the entries take them (row scalars [B, 1])."""
    out = {k: torch.as_tensor(np.ascontiguousarray(inst[k]), device=device) for k in ref.INSTANCE}
    for k in SCALARS:
        out[k] = out[k].reshape(-1, 1).contiguous()
    return out


def inst_table(st):
    """The co_mtvrp_instance table of a product state; the caller keeps it referenced until
    the call has returned."""
    return nat.mtvrp_instance(*(st[k] for k in ref.INSTANCE))


def state_ptrs(st):
    return [nat.ptr(st[k]) for k in ("cur", "time", "length", "used_l", "used_b", "visited")]


def fresh_state(b, nc, device):
    e = functools.partial(torch.empty, device=device)
    return {"cur": e(b, dtype=torch.int64), "time": e((b, 1)), "length": e((b, 1)),
            "used_l": e((b, 1)), "used_b": e((b, 1)), "visited": e((b, nc), dtype=torch.uint8)}


def abi_reset(inst, device):
    """co_mtvrp_reset -> a product state (torch tensors on ``device``)."""
    st = to_dev(inst, device)
    b, nc = st["locs"].shape[:2]
    st.update(fresh_state(b, nc, device), action_mask=torch.empty((b, nc), dtype=torch.bool,
                                                                  device=device))
    table = inst_table(st)
    nat.call("co_mtvrp_reset", b, nc - 1, table.address, *state_ptrs(st),
             nat.ptr(st["action_mask"]), nat.stream_of(st["locs"]))
    return st


def abi_state(rs, device):
    """A restatement state as a product state on ``device``."""
    st = to_dev(rs, device)
    t = functools.partial(torch.as_tensor, device=device)
    st["cur"] = t(rs["cur"]).contiguous()
    for k in ("time", "length", "used_l", "used_b"):
        st[k] = t(rs[k])[:, None].contiguous()
    st["visited"] = t(rs["visited"]).contiguous()
    st["action_mask"] = t(rs["action_mask"]).contiguous()
    return st


def abi_mask(st):
    b, nc = st["locs"].shape[:2]
    out = dict(st, action_mask=torch.empty((b, nc), dtype=torch.bool, device=st["locs"].device))
    table = inst_table(st)
    nat.call("co_mtvrp_action_mask", b, nc - 1, table.address, *state_ptrs(st),
             nat.ptr(out["action_mask"]), nat.stream_of(st["locs"]))
    return out


def abi_step(st, action, status=None, not_done=None, inplace=False):
    """co_mtvrp_step into fresh tensors (``inplace``: visited updated in place)."""
    b, nc = st["locs"].shape[:2]
    dev = st["locs"].device
    e = functools.partial(torch.empty, device=dev)
    out = dict(st, **fresh_state(b, nc, dev))
    if inplace:
        out["visited"] = st["visited"]
    out.update(done=e(b, dtype=torch.bool), reward=e(b), action_mask=e((b, nc), dtype=torch.bool))
    action = torch.as_tensor(action, device=dev).long().contiguous()
    table = inst_table(st)
    nat.call("co_mtvrp_step", b, nc - 1, nat.ptr(action), table.address, *state_ptrs(st),
             *state_ptrs(out), nat.ptr(out["done"]), nat.ptr(out["reward"]),
             nat.ptr(out["action_mask"]), nat.ptr(status), nat.ptr(not_done),
             nat.stream_of(st["locs"]))
    return out


def abi_steps(st, actions, status=None, not_done=None, want=True):
    """co_mtvrp_steps on clones of the state: ``actions`` is a [T, B] view of any strides.
    Returns (state, feasible, time, length), the last three [T, B]."""
    b, nc = st["locs"].shape[:2]
    dev = st["locs"].device
    t = actions.shape[0]
    e = functools.partial(torch.empty, device=dev)
    out = dict(st, **{k: st[k].clone() for k in ("cur", "time", "length", "used_l", "used_b",
                                                 "visited")})
    out.update(done=e(b, dtype=torch.bool), reward=e(b), action_mask=e((b, nc), dtype=torch.bool))
    feasible = e((t, b), dtype=torch.bool) if want else None
    times = e((t, b)) if want else None
    lengths = e((t, b)) if want else None
    table = inst_table(st)
    nat.call("co_mtvrp_steps", b, nc - 1, t, nat.ptr(actions), actions.stride(0),
             actions.stride(1), table.address, *state_ptrs(out), nat.ptr(out["done"]),
             nat.ptr(out["reward"]), nat.ptr(out["action_mask"]), nat.ptr(feasible),
             nat.ptr(times), nat.ptr(lengths), nat.ptr(status), nat.ptr(not_done),
             nat.stream_of(st["locs"]))
    return out, feasible, times, lengths


def abi_reward(st, actions):
    """co_mtvrp_reward for actions [B, T] (any strides)."""
    b, t = actions.shape
    out = torch.empty(b, device=st["locs"].device)
    nat.call("co_mtvrp_reward", b, st["locs"].shape[1] - 1, t, nat.ptr(st["locs"]),
             nat.ptr(actions), actions.stride(0), actions.stride(1), nat.ptr(st["open_route"]),
             nat.ptr(out), None, nat.stream_of(st["locs"]))
    return out


def abi_check(st, actions):
    """co_mtvrp_check's status bits for actions [B, T] (any strides)."""
    status = torch.zeros(1, dtype=torch.int32, device=st["locs"].device)
    b, t = actions.shape
    table = inst_table(st)
    nat.call("co_mtvrp_check", b, st["locs"].shape[1] - 1, t, table.address, nat.ptr(actions),
             actions.stride(0), actions.stride(1), nat.ptr(status), nat.stream_of(st["locs"]))
    return int(status.item())


# ------------------------------------------------------------------ comparisons
def check_state(got, want, what, keys=STATE):
    """A product state against a restatement state, bit for bit."""
    for key in keys + tuple(k for k in ("done", "reward") if k in want and k in got):
        same_bits(got[key], want[key], f"{what} {key}")


def check_states_equal(a, b, what, keys=STATE + ("done", "reward")):
    for key in keys:
        same_bits(a[key], b[key].detach().cpu().numpy(), f"{what} {key}")


def check_shape(n, b, device, directed=False):
    """Reset, mask, every single step, co_mtvrp_steps (T = 1, 7, the episode; both action
    layouts) and the reward against the restatement's rollout (random-feasible or
    ``directed``), bit for bit."""
    inst = instance(n, b)
    states, actions = rollout(n, b, None, directed)
    what = f"n{n} b{b}" + (" directed" if directed else "")
    st = abi_reset(inst, device)
    check_state(st, states[0], what + " reset")
    start = st
    singles = {}
    for t, a in enumerate(actions):
        st = abi_step(st, a)
        check_state(st, states[t + 1], f"{what} step {t}")
        singles[t + 1] = st
    mid = len(actions) // 2
    check_state(abi_mask(abi_state(states[mid], device)), states[mid], what + " mask entry")
    acts = torch.from_numpy(actions).to(device)  # [T, B]
    row_major = acts.t().contiguous().t()  # the [B, T] buffer viewed step-major
    _, want_f, want_t, want_l, _ = ref.steps(states[0], actions)
    for steps in sorted({1, min(7, len(actions)), len(actions)}):
        for layout, view in (("step-major", acts[:steps]), ("row-major", row_major[:steps])):
            got, feasible, times, lengths = abi_steps(start, view)
            tag = f"{what} T{steps} {layout}"
            check_states_equal(got, singles[steps], tag)
            same_bits(feasible, want_f[:steps], tag + " feasible")
            same_bits(times, want_t[:steps], tag + " time")
            same_bits(lengths, want_l[:steps], tag + " route_length")
    want_r = ref.reward(inst, actions.T)
    for view in (acts.t(), row_major.t()):
        same_bits(abi_reward(start, view), want_r, what + " reward")


# ------------------------------------------------------------------ hand-made rows
# depot (0, 0); c1 (3, 0), c2 (0, 0.5), c3 (1, 0).  Rows, one per feature:
#   0  closed, depot deadline 4: c1 cannot be served and left for the depot in time (3 + 3)
#   1  the same row open: depot_ok is 0 < 4 for every column, c1 can be visited
#   2  c2 is a backhaul: after the pickup the linehauls c1, c3 lock until the depot
#   3  limit 2.0: c3 (1 out, 1 back) is exactly at the limit and allowed (over is a strict >)
#   4  limit just below 2.0: c3 is over
#   5  the current time is NaN: no customer can be reached
def hand_instance():
    b = 6
    inf = np.float32(np.inf)
    locs = np.tile(np.array([[0, 0], [3, 0], [0, 0.5], [1, 0]], np.float32), (b, 1, 1))
    tw = np.tile(np.array([[0, inf]] * 4, np.float32), (b, 1, 1))
    tw[:2, 0, 1] = 4
    dl = np.tile(np.array([0, 0.3, 0.3, 0.3], np.float32), (b, 1))
    db = np.zeros((b, 4), np.float32)
    dl[2, 2], db[2, 2] = 0, 0.3
    limit = np.full(b, inf, np.float32)
    limit[3] = 2.0
    limit[4] = np.nextafter(np.float32(2.0), np.float32(0))
    opened = np.zeros(b, bool)
    opened[1] = True
    return {"locs": locs, "time_windows": tw, "service_time": np.zeros((b, 4), np.float32),
            "demand_linehaul": dl, "demand_backhaul": db,
            "vehicle_capacity": np.ones(b, np.float32), "speed": np.ones(b, np.float32),
            "distance_limit": limit, "open_route": opened}


HAND_ACTIONS = np.array([[2, 0, 3], [1, 0, 3], [2, 1, 0], [3, 0, 1], [3, 0, 1], [0, 1, 0]]).T.copy()
HAND_FEASIBLE = np.array([[1, 1, 1], [1, 1, 1], [1, 0, 1], [1, 1, 0], [0, 1, 0], [1, 0, 1]], bool).T


def check_hand_made(device):
    """The known answers, asserted on the restatement first and then on the product."""
    inst = hand_instance()
    rs = ref.reset(inst)
    rs["time"][5] = np.nan
    rs = ref.mask(rs)
    t, f = True, False
    assert rs["action_mask"].tolist() == [
        [f, f, t, t],   # closed: c1 cannot get back by the depot's deadline
        [f, t, t, t],   # open: the same c1 can be visited
        [f, t, t, t],   # the backhaul may be picked up first
        [f, f, t, t],   # c1 (3 + 3) is over the limit, c3 at it is not
        [f, f, t, f],   # just below: c3 is over
        [t, f, f, f]]   # NaN time: nothing reachable, the depot column stays open
    want = [rs]
    for a in HAND_ACTIONS:
        want.append(ref.step(want[-1], a)[0])
    assert want[1]["action_mask"][2].tolist() == [t, f, f, f]  # linehauls lock after the pickup
    assert want[3]["action_mask"][2].tolist() == [f, f, f, t]  # and open again at the depot
    assert np.isnan(want[1]["time"][5]) and np.isnan(want[3]["time"][5])  # 0 * NaN
    _, feas, times, lengths, _ = ref.steps(rs, HAND_ACTIONS)
    assert (feas == HAND_FEASIBLE).all(), feas.T
    start = abi_state(rs, device)
    check_state(abi_mask(start), rs, "hand mask")
    st = start
    for k, a in enumerate(HAND_ACTIONS):
        st = abi_step(st, a)
        check_state(st, want[k + 1], f"hand step {k}")
    acts = torch.from_numpy(HAND_ACTIONS).to(device)
    for view in (acts, acts.t().contiguous().t()):
        got, feasible, tm, ln = abi_steps(start, view)
        check_states_equal(got, st, "hand steps")
        same_bits(feasible, HAND_FEASIBLE, "hand feasible")
        same_bits(tm, times, "hand time")
        same_bits(ln, lengths, "hand route_length")


def check_depot_to_depot(device):
    """`feasible` of a depot -> depot action: false while some customer can be visited, true
    once none can (rows 0..2 of a finished episode stay at the depot)."""
    n, b = 5, 3
    states, actions = rollout(n, b)
    start = abi_reset(instance(n, b), device)
    zeros = torch.zeros((2, b), dtype=torch.int64, device=device)
    _, feasible, _, _ = abi_steps(start, zeros)
    assert not feasible.any()  # at the depot with customers open
    _, want_f, _, _, _ = ref.steps(states[0], np.zeros((2, b), np.int64))
    same_bits(feasible, want_f, "depot -> depot at reset")
    done = abi_state(states[-1], device)
    assert states[-1]["done"].all()
    tail = np.zeros((3, b), np.int64)
    _, feasible, _, _ = abi_steps(done, torch.from_numpy(tail).to(device))
    _, want_f, _, _, _ = ref.steps(states[-1], tail)
    same_bits(feasible, want_f, "depot -> depot when done")
    assert feasible[1:].all()


def check_edges(device):
    """In-place visited, the not_done counter, an empty batch and an out-of-range action."""
    n, b = 20, 16
    states, actions = rollout(n, b)
    t = len(actions) - 6  # some rows done, some not
    st = abi_state(states[t], device)
    fresh = abi_step(st, actions[t])
    cnt = torch.zeros(1, dtype=torch.int32, device=device)
    held = dict(st, visited=st["visited"].clone())
    inplace = abi_step(held, actions[t], not_done=cnt, inplace=True)
    assert inplace["visited"] is held["visited"]
    check_states_equal(inplace, fresh, "in-place visited")
    left = int((~states[t + 1]["done"]).sum())
    assert int(cnt.item()) == left
    cnt.zero_()
    acts = torch.from_numpy(actions).to(device)
    abi_steps(abi_state(states[0], device), acts[:t + 1], not_done=cnt)
    assert int(cnt.item()) == left
    # an empty batch is a no-op, whatever the pointers
    s = nat.stream_of(st["locs"])
    nat.call("co_mtvrp_reset", 0, n, *([None] * 8), s)
    nat.call("co_mtvrp_step", 0, n, *([None] * 19), s)
    nat.call("co_mtvrp_action_mask", 0, n, *([None] * 8), s)
    nat.call("co_mtvrp_steps", 0, n, 3, None, 1, 1, *([None] * 15), s)
    nat.call("co_mtvrp_reward", 0, n, 3, None, None, 3, 1, None, None, None, s)
    nat.call("co_mtvrp_check", 0, n, 3, None, None, 3, 1, None, s)
    # an action outside 0..N: CO_ST_INDEX_RANGE, the row's state as it was
    bad = actions[t].copy()
    bad[0], bad[1] = n + 1, -1
    want, bits = ref.step(states[t], bad)
    assert bits == nat.ST_INDEX_RANGE
    for k in ("cur", "time", "length", "used_l", "used_b", "visited"):
        assert (want[k][:2] == states[t][k][:2]).all(), k
    status = torch.zeros(1, dtype=torch.int32, device=device)
    check_state(abi_step(st, bad, status=status), want, "bad action")
    assert int(status.item()) == nat.ST_INDEX_RANGE
    status.zero_()
    _, feasible, _, _ = abi_steps(st, torch.as_tensor(bad, device=device)[None], status=status)
    assert int(status.item()) == nat.ST_INDEX_RANGE and not feasible[0, :2].any()


MT_BITS = (nat.ST_MT_LIMIT_NEGATIVE | nat.ST_MT_TW_NEGATIVE | nat.ST_MT_SERVICE_NEGATIVE
           | nat.ST_MT_TW_INFEASIBLE | nat.ST_MT_DEPOT_RETURN | nat.ST_MT_ROUTE_LIMIT
           | nat.ST_MT_DEADLINE | nat.ST_MT_OVER_LINEHAUL | nat.ST_MT_OVER_BACKHAUL
           | nat.ST_INVALID_TOUR)


def check_check_bits(device):
    """co_mtvrp_check on B = 300 (five 64-thread blocks, the last partial), actions
    step-major and row-major, against the restatement's ``check``: the finished episodes
    raise nothing, and each status bit is provoked in one row (287, a plain CVRP row; 279, a
    VRPB row, for the backhaul capacity) with every other row clean -- the provoked bit is
    the first in the reference's order that the row sets."""
    n, b, r, rb = 20, 300, 287, 279
    inst = instance(n, b)
    states, actions = rollout(n, b)  # [T, B]
    assert states[-1]["done"].all()
    assert not inst["open_route"][r] and np.isinf(inst["distance_limit"][r]) \
        and np.isinf(inst["time_windows"][r, 1:, 1]).all() and not inst["demand_backhaul"][r].any()
    mine = actions[:, r]
    first = int(mine[0])
    pick = int(np.nonzero(inst["demand_backhaul"][rb] > 0)[0][0])
    assert first != 0

    def both(want, what, acts_=actions, **edits):
        cur = dict(inst)
        for key, (index, value) in edits.items():
            arr = cur[key].copy()
            arr[index] = value
            cur[key] = arr
        rows = ref.check(cur, acts_.T)
        hit = np.nonzero(rows)[0].tolist()
        expect = int(np.bitwise_or.reduce(rows))
        if want == 0:
            assert expect == 0, (what, hit)
        else:
            assert len(hit) == 1 and expect & want, (what, hit, expect)
            low = expect & MT_BITS
            assert low & -low == want or want == nat.ST_INDEX_RANGE, (what, expect)
        st = to_dev(cur, device)
        a = torch.from_numpy(acts_).to(device)
        for layout, view in (("step-major", a.t()), ("row-major", a.t().contiguous())):
            got = abi_check(st, view)
            assert got == expect, (what, layout, got, expect)

    def edited(arr, index, value):
        out = arr.copy()
        out[index] = value
        return out

    d_first = float(ref.dist(inst["locs"][r, 0], inst["locs"][r, first]))
    both(0, "untouched")
    both(nat.ST_INVALID_TOUR, "a customer left out", acts_=edited(actions, (0, r), 0))
    both(nat.ST_INVALID_TOUR, "a repeated customer",
         acts_=edited(actions, (1, r), first) if mine[1] != 0 else edited(actions, (2, r), first))
    both(nat.ST_MT_LIMIT_NEGATIVE, "negative limit", distance_limit=(r, -1.0))
    both(nat.ST_MT_TW_NEGATIVE, "negative window", time_windows=((r, first, 0), -0.5))
    both(nat.ST_MT_SERVICE_NEGATIVE, "negative service", service_time=((r, first), -0.01))
    both(nat.ST_MT_TW_INFEASIBLE, "empty window",
         time_windows=((r, first), np.array([5, 5], np.float32)))
    both(nat.ST_MT_DEPOT_RETURN, "no return in time",
         time_windows=((r, slice(0, first + 1, first)), np.array([[0, 100], [99.95, np.inf]],
                                                                np.float32)))
    both(nat.ST_MT_ROUTE_LIMIT, "route over the limit", distance_limit=(r, 0.5 * d_first))
    both(nat.ST_MT_DEADLINE, "missed deadline", time_windows=((r, first, 1), 0.5 * d_first))
    both(nat.ST_MT_OVER_LINEHAUL, "linehaul over capacity", demand_linehaul=((r, first), 2.0))
    both(nat.ST_MT_OVER_BACKHAUL, "backhaul over capacity", demand_backhaul=((rb, pick), 2.0))
    both(nat.ST_INDEX_RANGE, "action out of range", acts_=edited(actions, (3, r), n + 1))


def check_invalid_arguments(lib):
    """CO_E_INVAL on N > 1023, a missing table, table member or required pointer and steps <
    1; CO_E_ALIGN on a misaligned pair array -- decided before any launch, so this runs
    without a device."""
    one = torch.zeros(64)
    p = one.data_ptr()
    full = nat.mtvrp_instance(*([one] * 9))
    holed = nat.mtvrp_instance(*([one] * 3), None, *([one] * 5))
    skew = nat.MtvrpInstance(p + 4, *([p] * 8))
    no_speed = nat.mtvrp_instance(*([one] * 6), None, one, one)
    t = full.address
    reset = [2, 3, t] + [p] * 7 + [None]
    assert lib.co_mtvrp_reset(2, 1024, *reset[2:]) == -1
    assert lib.co_mtvrp_reset(2, 0, *reset[2:]) == -1
    assert lib.co_mtvrp_reset(2, 3, None, *reset[3:]) == -1
    assert lib.co_mtvrp_reset(2, 3, holed.address, *reset[3:]) == -1
    assert lib.co_mtvrp_reset(2, 3, no_speed.address, *reset[3:]) == -1
    assert lib.co_mtvrp_reset(*reset[:4], None, *reset[5:]) == -1
    assert lib.co_mtvrp_reset(2, 3, skew.address, *reset[3:]) == -2
    step = [2, 3, p, t] + [p] * 15 + [None, None, None]
    assert lib.co_mtvrp_step(2, 1024, *step[2:]) == -1
    assert lib.co_mtvrp_step(*step[:2], None, *step[3:]) == -1
    assert lib.co_mtvrp_step(*step[:3], holed.address, *step[4:]) == -1
    mask = [2, 3, t] + [p] * 7 + [None]
    assert lib.co_mtvrp_action_mask(2, 1024, *mask[2:]) == -1
    assert lib.co_mtvrp_action_mask(*mask[:9], None, None) == -1
    steps = [2, 3, 4, p, 2, 1, t] + [p] * 9 + [None] * 6
    assert lib.co_mtvrp_steps(2, 1024, *steps[2:]) == -1
    assert lib.co_mtvrp_steps(2, 3, 0, *steps[3:]) == -1
    assert lib.co_mtvrp_steps(*steps[:3], None, *steps[4:]) == -1
    assert lib.co_mtvrp_steps(*steps[:6], None, *steps[7:]) == -1
    rew = [2, 3, 4, p, p, 4, 1, p, p, None, None]
    assert lib.co_mtvrp_reward(2, 1024, *rew[2:]) == -1
    assert lib.co_mtvrp_reward(*rew[:8], None, None, None) == -1
    chk = [2, 3, 4, t, p, 4, 1, p, None]
    assert lib.co_mtvrp_check(2, 1024, *chk[2:]) == -1
    assert lib.co_mtvrp_check(*chk[:7], None, None) == -1
    assert lib.co_mtvrp_check(2, 3, 4, holed.address, *chk[4:]) == -1
    assert lib.co_mtvrp_check(2, 3, 4, skew.address, *chk[4:]) == -2
