"""Record what the reference's own code computes -- TEST INFRASTRUCTURE ONLY.

``python -m oracle.record_reference [--out DIR]`` loads the reference's modules through
``oracle/reference.py``, calls its functions on small fixed inputs and writes inputs and
outputs as plain arrays to ``DIR/ref_<group>.npz`` (default ``tests/golden``).  The inputs are
drawn with seeded generators and stored next to the outputs, so no test depends on an RNG
stream.  A key is ``<reference function>/<case>/<array>``; a file holds arrays and key names
only and is written with fixed zip timestamps, so two runs give identical bytes.

Two things are not the reference's installed stack: ``tensordict`` / ``torchrl`` are the
stand-ins of ``oracle/reference.py`` (the recorded functions only read and write entries), and
real ``numba`` was not available: ``njit`` is the identity, so the 2-opt of
``rl4co/envs/routing/tsp/local_search.py`` runs as plain Python on the same numpy ``float32``
scalars (its ``delta`` stays a ``float32`` where numba would widen it to ``float64``; the two
differ only for a change within one f32 ulp of the ``-1e-6`` threshold).

Sampling's draw is not recorded: it follows torch's generator stream.

Run it in a process of its own (see ``oracle/reference.py``).
"""
from __future__ import annotations

import argparse
import hashlib
import io
import math
import os
import platform
import types
import zipfile

import numpy as np
import torch

from . import reference

GROUPS = ("ops", "transforms", "tsp", "cvrp", "slap", "decoding", "two_opt", "pomo")
MAX_BYTES = 256 * 1024


def _np(x):
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().contiguous().numpy().copy()
    if isinstance(x, str):
        return np.array(x)
    return np.asarray(x)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


class _Rec(dict):
    def put(self, fn, case, **arrays):
        for name, value in arrays.items():
            key = f"{fn}/{case}/{name}"
            assert key not in self, key
            self[key] = _np(value)


def write_npz(path, arrays):
    """``np.load``-compatible archive with sorted members and a fixed timestamp."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.require(arrays[key], requirements="C"), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def machine_fingerprint():
    """What decides the bits of ATen's CPU float kernels: the tests ask the oracle for the
    recorded floats bit for bit only where this matches (tests/ref_recordings.py)."""
    text = "|".join((torch.__version__, np.__version__, platform.machine(),
                     torch.backends.cpu.get_cpu_capability()))
    return np.frombuffer(hashlib.sha256(text.encode()).digest(), dtype=np.uint8).copy()


def _error_text(fn, *args):
    try:
        fn(*args)
    except AssertionError as exc:
        return str(exc)
    raise RuntimeError("the reference accepted an invalid solution")


# ---------------------------------------------------------------------------
# ops / transforms
# ---------------------------------------------------------------------------
GATHER_CASES = [  # tests/test_gpu_ops.py
    ((64, 100, 2), (64, 100), torch.float32),
    ((33, 20), (33, 1), torch.float32),
    ((17, 21, 128), (17,), torch.float32),
    ((9, 7), (9,), torch.float32),
    ((5, 11, 3), (5, 4), torch.int64),
    ((6, 13, 3), (6, 2), torch.bool),
]


def record_ops(mods):
    ops, TD = mods["rl4co.utils.ops"], reference.TensorDict
    rec = _Rec()
    rec.put("recorded_on", "machine", fingerprint=machine_fingerprint())
    for c, (shape, idx_shape, dtype) in enumerate(GATHER_CASES):
        g = _gen(c)
        # 12-bit values (a gather only moves them): the archive stays small
        src = torch.randint(0, 4096, shape, generator=g)
        src = src > 2048 if dtype == torch.bool else (src / 8).to(dtype)
        idx = torch.randint(0, shape[1], idx_shape, generator=g)
        rec.put("gather_by_index", f"c{c}", src=src, idx=idx,
                out_squeeze=ops.gather_by_index(src, idx, squeeze=True),
                out_nosqueeze=ops.gather_by_index(src, idx, squeeze=False))
    locs = torch.rand(9, 13, 2, generator=_gen(10))
    rec.put("get_tour_length", "b9n13", locs=locs, out=ops.get_tour_length(locs))
    for shape in ((3, 20), (2, 5, 7)):
        locs = torch.rand(*shape, 2, generator=_gen(11 + len(shape)))
        rec.put("get_distance_matrix", "x".join(map(str, shape)), locs=locs,
                out=ops.get_distance_matrix(locs))
    s, b, t = 5, 7, 9
    g = _gen(12)
    x = torch.randint(0, 100, (b, t), generator=g)
    xs = torch.randint(0, 100, (s * b, t), generator=g)
    m = torch.randint(0, s, (b,), generator=g)
    rec.put("batchify", "s5b7t9", x=x, out=ops.batchify(x, s))
    rec.put("unbatchify", "s5b7t9", x=xs, out=ops.unbatchify(xs, s))
    rec.put("unbatchify_and_gather", "s5b7t9", x=xs, idx=m,
            out=ops.unbatchify_and_gather(xs, m, s))
    for name, n_actions, num_loc in (("tsp", 7, 7), ("cvrp", 8, 7)):
        env = types.SimpleNamespace(name=name, generator=types.SimpleNamespace(num_loc=num_loc))
        td = TD({"action_mask": torch.ones(3, n_actions, dtype=torch.bool)}, batch_size=[3])
        n = ops.get_num_starts(td, name)
        rec.put("get_num_starts", name, action_mask=td["action_mask"], out=n)
        rec.put("select_start_nodes", name, num_starts=n, num_loc=num_loc, batch=3,
                out=ops.select_start_nodes(td, env, n))
        # more starts than nodes: the modulo by num_loc
        rec.put("select_start_nodes", name + "_wrap", num_starts=n + 3, num_loc=num_loc, batch=3,
                out=ops.select_start_nodes(td, env, n + 3))
    return rec


def record_transforms(mods):
    tr = mods["rl4co.data.transforms"]
    rec = _Rec()
    for b, n in ((5, 20), (1, 1)):
        xy = torch.rand(b, n, 2, generator=_gen(20 + n))
        rec.put("dihedral_8_augmentation", f"b{b}n{n}", xy=xy, out=tr.dihedral_8_augmentation(xy))
    xy = torch.rand(6, 7, 2, generator=_gen(22))
    phi = torch.tensor([0.0, 1.0, 2 * math.pi, 6.2831855, 7.5, 12.0])[:, None, None]
    rec.put("symmetric_transform", "b6n7", xy=xy, phi=phi,
            out=tr.symmetric_transform(xy[..., [0]], xy[..., [1]], phi))
    return rec


# ---------------------------------------------------------------------------
# envs
# ---------------------------------------------------------------------------
def _stack_states(rec, fn, case, states, ragged=()):
    for key in states[0]:
        if key in ragged:
            for t, s in enumerate(states):
                rec.put(fn, case, **{f"after_{key}_t{t:02d}": s[key]})
        else:
            rec.put(fn, case, **{f"after_{key}": torch.stack([s[key] for s in states])})


def _snapshot(td, keys):
    return {k: td[k].clone() for k in keys}


TSP_STATE = ("first_node", "current_node", "i", "action_mask", "reward", "done")


def record_tsp(mods):
    TD = reference.TensorDict
    TSPEnv = mods["rl4co.envs.routing.tsp.env"].TSPEnv
    rec = _Rec()
    for b, n in ((5, 7), (33, 20)):
        case = f"b{b}n{n}"
        g = _gen(100 + n)
        env = TSPEnv(generator_params=dict(num_loc=n), seed=0)
        locs = torch.rand(b, n, 2, generator=g)
        actions = torch.rand(b, n, generator=g).argsort(1)
        td = TD({"locs": locs}, batch_size=[b])
        out = env._reset(td, batch_size=[b])
        rec.put("TSPEnv._reset", case, locs=locs, **{"out_" + k: v for k, v in out.items()})
        td.update(out)
        states = []
        for t in range(n):
            td["action"] = actions[:, t]
            td = env._step(td)
            states.append(_snapshot(td, TSP_STATE))
        rec.put("TSPEnv._step", case, locs=locs, actions=actions)
        _stack_states(rec, "TSPEnv._step", case, states)
        rec.put("TSPEnv.get_reward", case, locs=locs, actions=actions,
                out=env.get_reward(td, actions))
        if n == 7:
            bad = actions.clone()
            bad[2, 3] = bad[2, 4]
            rec.put("TSPEnv.check_solution_validity", "duplicate", actions=bad,
                    error=_error_text(env.check_solution_validity, td, bad))
    # one step from states with mixed / all-positive step counters: the first node follows
    # the action for the whole batch as soon as any row has i == 0
    b, n = 5, 7
    for case, i in (("mixed_i", [0, 1, 0, 2, 3]), ("positive_i", [1, 1, 2, 2, 3]),
                    ("zero_i", [0, 0, 0, 0, 0])):
        g = _gen(150)
        mask = torch.rand(b, n, generator=g) > 0.4
        mask[:, 5] = True
        td = TD({"first_node": torch.full((b,), 6), "current_node": torch.full((b,), 6),
                 "i": torch.tensor(i)[:, None], "action_mask": mask,
                 "action": torch.tensor([5, 1, 2, 3, 4])}, batch_size=[b])
        rec.put("TSPEnv._step", case, **{"before_" + k: v for k, v in td.items()})
        td = TSPEnv._step(td)
        rec.put("TSPEnv._step", case, **{"after_" + k: td[k] for k in TSP_STATE})
    return rec


CVRP_STATE = ("current_node", "used_capacity", "visited", "action_mask", "reward", "done")


def _cvrp_episode(env, td, actions=None, g=None):
    states, taken = [], []
    t = 0
    while True:
        if actions is None:
            act = torch.multinomial(td["action_mask"].float(), 1, generator=g).squeeze(1)
        else:
            act = actions[:, t]
        td["action"] = act
        td = env._step(td)
        taken.append(act)
        states.append(_snapshot(td, CVRP_STATE))
        t += 1
        if (actions is None and bool(td["done"].all())) or (actions is not None and t == actions.size(1)):
            return td, torch.stack(taken, 1), states


def record_cvrp(mods):
    TD = reference.TensorDict
    CVRPEnv = mods["rl4co.envs.routing.cvrp.env"].CVRPEnv
    rec = _Rec()
    for b, n in ((5, 7), (33, 20)):
        case = f"b{b}n{n}"
        g = _gen(200 + n)
        env = CVRPEnv(generator_params=dict(num_loc=n), seed=0)
        cap = env.generator.capacity
        inp = {"locs": torch.rand(b, n, 2, generator=g), "depot": torch.rand(b, 2, generator=g),
               "demand": torch.randint(1, 10, (b, n), generator=g).float() / cap}
        td = TD(dict(inp), batch_size=[b])
        out = env._reset(td, batch_size=[b])
        rec.put("CVRPEnv._reset", case, **inp, **{"out_" + k: v for k, v in out.items()})
        td.update(out)
        td, actions, states = _cvrp_episode(env, td, g=g)
        rec.put("CVRPEnv._step", case, **inp, actions=actions)
        _stack_states(rec, "CVRPEnv._step", case, states)
        rec.put("CVRPEnv.get_reward", case, **inp, actions=actions, out=env.get_reward(td, actions))
        if n == 7:
            bad = actions.clone()
            first = int((bad[1] != 0).nonzero()[0])
            bad[1, first] = 0  # a customer is never served
            rec.put("CVRPEnv.check_solution_validity", "not_a_permutation", **inp, actions=bad,
                    error=_error_text(env.check_solution_validity, td, bad))
            over = torch.arange(1, n + 1).repeat(b, 1)  # every customer in one trip
            rec.put("CVRPEnv.check_solution_validity", "over_capacity", **inp, actions=over,
                    error=_error_text(env.check_solution_validity, td, over))
    # demands that fill the vehicle exactly: 0.5 + 0.5 and 0.25 + 0.25 + 0.5 are not "> 1"
    env = CVRPEnv(generator_params=dict(num_loc=4), seed=0)
    inp = {"locs": torch.rand(2, 4, 2, generator=_gen(250)), "depot": torch.rand(2, 2, generator=_gen(251)),
           "demand": torch.tensor([[0.5, 0.25, 0.25, 0.5], [0.25, 0.5, 0.5, 0.25]])}
    actions = torch.tensor([[1, 4, 0, 2, 3, 0], [1, 4, 2, 0, 3, 0]])
    td = TD(dict(inp), batch_size=[2])
    td.update(env._reset(td, batch_size=[2]))
    td, _, states = _cvrp_episode(env, td, actions=actions)
    rec.put("CVRPEnv._step", "exact_fill", **inp, actions=actions)
    _stack_states(rec, "CVRPEnv._step", "exact_fill", states)
    # the mask alone, on arbitrary states
    b, n = 33, 20
    g = _gen(260)
    state = {"demand": torch.randint(1, 10, (b, n), generator=g).float() / 30.0,
             "used_capacity": torch.randint(0, 31, (b, 1), generator=g).float() / 30.0,
             "vehicle_capacity": torch.ones(b, 1),
             "visited": (torch.rand(b, n + 1, generator=g) > 0.5).to(torch.uint8),
             "current_node": torch.randint(0, 3, (b, 1), generator=g)}
    state["visited"][:4, 1:] = 1  # every customer served
    rec.put("CVRPEnv.get_action_mask", "b33n20", **state,
            out=CVRPEnv.get_action_mask(TD(state, batch_size=[b])))
    return rec


SLAP_STATE = ("assignment", "to_choose", "action_mask", "i", "reward", "done")


def record_slap(mods):
    TD = reference.TensorDict
    SLAPEnv = mods["rl4co.envs.warehousing.slap.env"].SLAPEnv
    SLAPGenerator = mods["rl4co.envs.warehousing.slap.generator"].SLAPGenerator
    rec = _Rec()
    for case, b, kw in (("default", 1, {}),
                        ("a7l9", 2, dict(n_aisles=7, n_locs=9, inter_loc_dist=0.7,
                                         inter_aisle_dist=3.1))):
        gen = SLAPGenerator(**kw)
        locs = gen._calc_coordinates([b])
        dist = gen._get_distance_matrix(locs)
        rec.put("SLAPGenerator._calc_coordinates", case, batch=b, n_aisles=gen.n_aisles,
                n_locs=gen.n_locs, inter_loc_dist=gen.inter_loc_dist,
                inter_aisle_dist=gen.inter_aisle_dist, out=locs)
        rec.put("SLAPGenerator._get_distance_matrix", case, locs=locs, out=dist,
                depot_loc_dist=dist[:, 0, :])
    for case, b, kw in (("default_b9", 9, {}),
                        ("a4l5p19_b5", 5, dict(n_products=19, n_aisles=4, n_locs=5, max_orders=6,
                                               max_products_in_order=4))):
        g = _gen(300 + b)
        gen = SLAPGenerator(**kw)
        env = SLAPEnv(generator=gen, seed=0)
        p = gen.n_products
        locs = gen._calc_coordinates([b])
        dist = gen._get_distance_matrix(locs)
        inp = {"freq": torch.rand(b, p, 1, generator=g) * 19 + 1, "locs": locs,
               "assignment": torch.full((b, p), -1, dtype=torch.int),
               "picklist": torch.randint(0, p, (b, gen.max_orders, gen.max_products_in_order),
                                         generator=g),
               "depot_loc_dist": dist[:, 0, :]}
        td = TD(dict(inp), batch_size=[b])
        out = env._reset(td, batch_size=[b])
        rec.put("SLAPEnv._reset", case, **inp, **{"out_" + k: v for k, v in out.items()})
        td.update(out)
        states, taken = [], []
        for t in range(p):
            act = torch.multinomial(td["action_mask"].float(), 1, generator=g).squeeze(1)
            td["action"] = act
            td = env._step(td)
            taken.append(act)
            states.append(_snapshot(td, SLAP_STATE))
            if t == p // 2:  # unassigned products are -1 and index the last location
                rec.put("SLAPEnv._get_reward", case + "_partial", locs=locs,
                        picklist=inp["picklist"], assignment=td["assignment"],
                        out=env._get_reward(td, None))
        actions = torch.stack(taken, 1)
        rec.put("SLAPEnv._step", case, actions=actions, n_aisles=gen.n_aisles, n_locs=gen.n_locs)
        _stack_states(rec, "SLAPEnv._step", case, states, ragged=("to_choose",))
        rec.put("SLAPEnv._get_reward", case, locs=locs, picklist=inp["picklist"],
                assignment=td["assignment"], out=env._get_reward(td, actions))
    return rec


# ---------------------------------------------------------------------------
# decoding
# ---------------------------------------------------------------------------
SETTINGS = {
    "noclip": {},
    "clip10": dict(tanh_clipping=10.0),
    "temp0.8": dict(temperature=0.8),
    "topk5": dict(top_k=5),
    "topp0.9": dict(top_p=0.9),
    "topk10_topp0.7": dict(top_k=10, top_p=0.7),
}


def _mask(b, n, g):
    m = torch.rand(b, n, generator=g) > 0.3
    m[torch.arange(b), torch.randint(0, n, (b,), generator=g)] = True
    return m


def record_decoding(mods):
    dec = mods["rl4co.utils.decoding"]
    TD = reference.TensorDict
    rec = _Rec()
    b = 16
    for n in (20, 37, 100):
        g = _gen(400 + n)
        logits = torch.randn(b, n, generator=g) * 3
        mask = _mask(b, n, g)
        ties = (torch.randn(b, n, generator=g) * 2).round()
        one = torch.zeros(b, n, dtype=torch.bool)
        one[torch.arange(b), torch.randint(0, n, (b,), generator=g)] = True
        one[b // 2:] = mask[b // 2:]
        inputs = {"rand": (logits, mask), "ties": (ties, mask), "one": (logits, one)}
        for iname, (lg, mk) in inputs.items():
            # tanh: torch.tanh as process_logits calls it (MKL's on the CPU, not always the
            # correctly rounded value the product evaluates)
            rec.put("process_logits", f"n{n}_{iname}", logits=lg, mask=mk, tanh=torch.tanh(lg))
            for sname, kw in SETTINGS.items():
                rec.put("process_logits", f"n{n}_{iname}", **{
                    "out_" + sname: dec.process_logits(lg.clone(), mk, **kw)})
        given = torch.multinomial(mask.float(), 1, generator=g).squeeze(1)
        for cname, clip in (("noclip", 0.0), ("clip10", 10.0)):
            for kind, cls in (("Greedy", dec.Greedy), ("Evaluate", dec.Evaluate)):
                strat = cls(tanh_clipping=clip)
                td = strat.step(logits.clone(), mask, TD({}, batch_size=[b]),
                                action=given if kind == "Evaluate" else None)
                rec.put(kind + ".step", f"n{n}_{cname}", logits=logits, mask=mask, given=given,
                        action=td["action"], logprobs=strat.logprobs[-1])
    g = _gen(450)
    lp = torch.log_softmax(torch.randn(8, 6, 11, generator=g), -1)
    acts = torch.randint(0, 11, (8, 6), generator=g)
    keep = torch.rand(8, 6, generator=g) > 0.3
    rec.put("get_log_likelihood", "b8t6n11", logprobs=lp, actions=acts, mask=keep,
            out_sum=dec.get_log_likelihood(lp.clone(), acts, None, True),
            out_masked_sum=dec.get_log_likelihood(lp.clone(), acts, keep, True),
            out_steps=dec.get_log_likelihood(lp.clone(), acts, None, False))
    # beam step: random scores, and scores with exact ties inside a beam and across beams
    bsz, bw, n = 3, 4, 10
    g = _gen(460)
    lg = torch.randn(bw * bsz, n, generator=g) * 2
    lg[torch.rand(bw * bsz, n, generator=g) < 0.3] = float("-inf")
    lg[:, 0] = 0.0
    rand_lp = torch.log_softmax(lg, -1)
    rand_parent = -torch.rand(bw * bsz, 1, generator=g) * 3
    tie_lp = torch.log_softmax((torch.randn(bsz, n, generator=g)).round(), -1).repeat(bw, 1)
    tie_parent = torch.tensor([-1.0, -1.0, -2.0, -1.0]).repeat_interleave(bsz)[:, None]
    for case, logp, parent in (("rand", rand_lp, rand_parent), ("ties", tie_lp, tie_parent)):
        bs = dec.BeamSearch(beam_width=bw)
        bs.parent_beam_logprobs = parent.clone()
        selected, idx = bs._make_beam_step(logp.clone())
        rec.put("BeamSearch._make_beam_step", f"b{bsz}w{bw}n{n}_{case}", logprobs=logp,
                parent=parent, beam_width=bw, selected=selected, batch_beam_idx=idx,
                beam_parent=bs.beam_path[-1], score=bs.parent_beam_logprobs)
    return rec


# ---------------------------------------------------------------------------
# 2-opt
# ---------------------------------------------------------------------------
def _perms(b, n, seed):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(np.stack([rng.permutation(n) for _ in range(b)]).astype(np.int64))


def record_two_opt(mods):
    ls = mods["rl4co.envs.routing.tsp.local_search"]
    dist = mods["rl4co.utils.ops"].get_distance_matrix
    TD = reference.TensorDict
    rec = _Rec()

    def run(case, locs, tours, **kw):
        td = TD({"locs": locs}, batch_size=[locs.shape[0]])
        rec.put("local_search", case, locs=locs, tours=tours, distances=dist(locs),
                max_iterations=kw.get("max_iterations", 1000), out=ls.local_search(td, tours, **kw))

    b = 8
    for n in (5, 12, 20):
        locs = torch.rand(b, n, 2, generator=_gen(500 + n))
        tours = _perms(b, n, 510 + n)
        run(f"b{b}n{n}", locs, tours)
        if n == 20:
            for it in (1, 3):
                run(f"b{b}n{n}_it{it}", locs, tours, max_iterations=it)
    # the 4 x 4 integer grid of tests/two_opt_cases.py: many moves tie bit for bit
    pts = torch.tensor([(x, y) for x in range(4) for y in range(4)], dtype=torch.float32)
    run("grid4x4", pts.repeat(32, 1, 1), _perms(32, 16, 5))
    # a tour that visits one node twice (not next to each other) and misses another: the only
    # inputs on which the reference's skip test (node_prev == node_j or node_next == node_i)
    # acts.  With a single repeated node the skipped moves are exactly those that would put
    # the two copies side by side, so the 1e9 diagonal the reference adds is never read.
    n = 12
    locs = torch.rand(b, n, 2, generator=_gen(560))
    tours = _perms(b, n, 561)
    for r in range(b):
        tours[r, (r + 5) % n] = tours[r, r % n]
    run("repeated_node", locs, tours)
    return rec


# ---------------------------------------------------------------------------
# POMO
# ---------------------------------------------------------------------------
def record_pomo(mods):
    pomo = reference.load_pomo()
    if pomo is None:
        return None
    baselines, reinforce, scaler = pomo
    ops = mods["rl4co.utils.ops"]
    rec = _Rec()
    b, s = 8, 5
    g = _gen(600)
    reward_flat = -torch.rand(s * b, generator=g) * 10
    ll_flat = -torch.rand(s * b, generator=g) * 20
    reward, ll = ops.unbatchify(reward_flat, s), ops.unbatchify(ll_flat, s)
    bl, bl_loss = baselines.SharedBaseline().eval(None, reward)
    rec.put("SharedBaseline.eval", "b8s5", reward=reward, out=bl, bl_loss=bl_loss)
    me = types.SimpleNamespace(baseline=baselines.SharedBaseline(), env=None,
                               advantage_scaler=scaler.RewardScaler(None))
    out = reinforce.REINFORCE.calculate_loss(me, None, {}, {}, reward, ll)
    rec.put("REINFORCE.calculate_loss", "b8s5", reward_flat=reward_flat, log_likelihood_flat=ll_flat,
            num_starts=s, loss=out["loss"], bl_val=out["bl_val"], max_reward=reward.max(dim=-1)[0])
    return rec


RECORDERS = {"ops": record_ops, "transforms": record_transforms, "tsp": record_tsp,
             "cvrp": record_cvrp, "slap": record_slap, "decoding": record_decoding,
             "two_opt": record_two_opt, "pomo": record_pomo}


def record(out_dir):
    torch.set_num_threads(1)
    mods = reference.load()
    os.makedirs(out_dir, exist_ok=True)
    written = {}
    for group in GROUPS:
        rec = RECORDERS[group](mods)
        if rec is None:
            print(f"ref_{group}: left out (its reference module does not load)")
            continue
        path = os.path.join(out_dir, f"ref_{group}.npz")
        write_npz(path, rec)
        size = os.path.getsize(path)
        assert size <= MAX_BYTES, (path, size)
        written[group] = size
        print(f"ref_{group}.npz: {len(rec)} arrays, {size} bytes")
    return written


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    default = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                           "tests", "golden")
    ap.add_argument("--out", default=default)
    record(ap.parse_args(argv).out)


if __name__ == "__main__":
    main()
