"""The kernels against recordings of the reference's own code (tests/golden/ref_<group>.npz,
see tests/ref_recordings.py for the rules and tests/test_reference_recordings.py for the
oracle and the host build): no oracle in between, and only the fixtures are read.

First through the env classes and the utils (the checks the CPU implementations pass),
then through ``nat.call`` on the C ABI for the per-step entry points and the fused or K-step
ones that claim identical output.  Every launch ends at ``torch.cuda.synchronize()`` and a
look at its status word."""
import pytest
import torch

import ref_recordings as rr
import rl4co_slap_amd as ra
from rl4co_slap_amd import _native as nat

pytestmark = pytest.mark.gpu

DEVICE = rr.ProductImpl("cuda")
EPISODES = ["b5n7", "b33n20"]  # N % 4 != 0: the single-step fallbacks; N % 4 == 0: lane groups
GREEDY, EVALUATE = 0, 2


def _status(dev):
    return torch.zeros(1, dtype=torch.int32, device=dev)


def _finish(st, want=0):
    torch.cuda.synchronize()
    assert int(st.item()) == want
    ra.check_errors()


def _new(dev, shape, dtype):
    """An output that starts as a pattern no result holds."""
    t = torch.empty(shape, dtype=dtype, device=dev)
    return t.fill_({torch.bool: True, torch.uint8: 179}.get(dtype, -77))


# -- through the env classes and utils --------------------------------------------------
@pytest.mark.parametrize("case", EPISODES)
def test_tsp_episode(dev, case):
    rr.check_tsp_episode(DEVICE, case)


@pytest.mark.parametrize("case", ["mixed_i", "positive_i", "zero_i"])
def test_tsp_first_node_rule_is_batch_wide(dev, case):
    rr.check_tsp_single_step(DEVICE, case)


def test_tsp_duplicate_is_invalid(dev):
    rr.check_tsp_validity(DEVICE)


@pytest.mark.parametrize("case", EPISODES)
def test_cvrp_episode(dev, case):
    rr.check_cvrp_episode(DEVICE, case)


def test_cvrp_exact_fill_stays_feasible(dev):
    rr.check_cvrp_exact_fill(DEVICE)


def test_cvrp_action_mask(dev):
    rr.check_cvrp_action_mask(DEVICE)


@pytest.mark.parametrize("case", ["not_a_permutation", "over_capacity"])
def test_cvrp_invalid_solutions(dev, case):
    rr.check_cvrp_validity(DEVICE, case)


@pytest.mark.parametrize("case", ["default", "a7l9"])
def test_slap_generate(dev, case):
    rr.check_slap_generator(DEVICE, case)


@pytest.mark.parametrize("case", ["default_b9", "a4l5p19_b5"])
def test_slap_episode(dev, case):
    rr.check_slap_episode(DEVICE, case)


@pytest.mark.parametrize("case", rr.cases("ops", "gather_by_index"))
def test_gather_by_index(dev, case):
    rr.check_gather(DEVICE, case)


def test_tour_length_and_batchify(dev):
    rr.check_ops(DEVICE)


@pytest.mark.parametrize("case", ["3x20", "2x5x7"])
def test_distance_matrix(dev, case):
    rr.check_distance_matrix(DEVICE, case)


@pytest.mark.parametrize("name", ["tsp", "cvrp"])
def test_start_nodes(dev, name):
    rr.check_starts(DEVICE, name)


@pytest.mark.parametrize("case", ["b5n20", "b1n1"])
def test_dihedral_augmentation(dev, case):
    rr.check_dihedral(DEVICE, case)


def test_symmetric_transform(dev):
    rr.check_symmetric(DEVICE, bitwise=False)


@pytest.mark.parametrize("setting", list(rr.SETTINGS))
@pytest.mark.parametrize("inputs", ["rand", "ties", "one"])
@pytest.mark.parametrize("n", [20, 37, 100])
def test_process_logits(dev, n, inputs, setting):
    rr.check_process_logits(DEVICE, n, inputs, setting)


@pytest.mark.parametrize("clip", ["noclip", "clip10"])
@pytest.mark.parametrize("n", [20, 37, 100])
def test_greedy_and_evaluate_step(dev, n, clip):
    rr.check_decode_step(DEVICE, n, clip)


def test_get_log_likelihood(dev):
    rr.check_log_likelihood(DEVICE)


@pytest.mark.parametrize("case", [c for c in rr.TWO_OPT_CASES if c != "repeated_node"])
def test_two_opt_local_search(dev, case):
    r = rr.two_opt_recording(case)
    b, n = r["tours"].shape
    env = DEVICE.tsp(n)
    for src in ("locs", "distances"):
        got = env.local_search(DEVICE.td({src: r[src]}, b), r["tours"].to(dev),
                               max_iterations=r["max_iterations"])
        rr.sync(DEVICE)
        rr.check_equal(got, r["out"], f"{case} from {src}")


def test_two_opt_rejects_a_repeated_node(dev):
    """Deliberate difference: the reference searches a row that is not a
    permutation unchecked; co_tsp_two_opt flags it and copies it unchanged with 0 sweeps."""
    r = rr.two_opt_recording("repeated_node")
    b, n = r["tours"].shape
    with pytest.raises(AssertionError, match="Invalid tour"):
        DEVICE.tsp(n).local_search(DEVICE.td({"locs": r["locs"]}, b), r["tours"].to(dev))
    locs, tours = r["locs"].to(dev), r["tours"].to(dev)
    out, sweeps, st = _new(dev, (b, n), torch.int64), _new(dev, b, torch.int32), _status(dev)
    nat.call("co_tsp_two_opt", b, n, nat.ptr(locs), None, b, nat.ptr(tours), n, 1, 1000,
             nat.ptr(out), nat.ptr(sweeps), nat.ptr(st), nat.stream_of(tours))
    _finish(st, nat.ST_INVALID_TOUR)
    rr.check_equal(out, r["tours"], "copied unchanged")
    assert not sweeps.any()


# -- the C ABI: 2-opt, beam ranking -------------------------------------------------------
@pytest.mark.parametrize("layout", ["row_major", "step_major"])
@pytest.mark.parametrize("case", ["b8n12", "b8n20_it3", "grid4x4"])
def test_co_tsp_two_opt(dev, case, layout):
    r = rr.two_opt_recording(case)
    b, n = r["tours"].shape
    locs = r["locs"].to(dev)
    if layout == "row_major":
        acts, sb, stt = r["tours"].to(dev), n, 1
    else:
        acts, sb, stt = r["tours"].t().contiguous().to(dev), 1, b
    out, sweeps, st = _new(dev, (b, n), torch.int64), _new(dev, b, torch.int32), _status(dev)
    nat.call("co_tsp_two_opt", b, n, nat.ptr(locs), None, b, nat.ptr(acts), sb, stt,
             r["max_iterations"], nat.ptr(out), nat.ptr(sweeps), nat.ptr(st), nat.stream_of(acts))
    _finish(st)
    rr.check_equal(out, r["out"], case)
    assert ((sweeps >= 1) & (sweeps <= r["max_iterations"])).all()


@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("case", rr.BEAM_CASES)
def test_co_beam_select(dev, case, with_mask):
    r, want = rr.beam_recording(case)
    e, n = r["logprobs"].shape
    bw = r["beam_width"]
    logp, par = r["logprobs"].to(dev), r["parent"].squeeze(1).contiguous().to(dev)
    mask = r["logprobs"].isfinite().to(dev) if with_mask else None
    sel, bpar = _new(dev, e, torch.int64), _new(dev, e, torch.int32)
    rows, score, st = _new(dev, e, torch.int64), _new(dev, e, torch.float32), _status(dev)
    nat.call("co_beam_select", e // bw, bw, n, nat.ptr(logp), logp.stride(0), nat.ptr(par),
             nat.ptr(mask), nat.ptr(sel), nat.ptr(bpar), nat.ptr(rows), nat.ptr(score), nat.ptr(st),
             nat.stream_of(logp))
    _finish(st)
    got = (sel, bpar, rows, score)
    if case.endswith("ties"):
        rr.check_beam_ties(got, r, case)
    else:
        rr.check_beam(got, want, case)


# -- the C ABI: TSP -------------------------------------------------------------------------
def _tsp_episode(case):
    r = rr.get("tsp", "TSPEnv._reset", case)
    s = rr.get("tsp", "TSPEnv._step", case)
    start = {k: r["out_" + k] for k in ("action_mask", "i", "first_node")}
    return r["locs"], s["actions"], [start] + rr.stacked_states(s, rr.TSP_STATE)


@pytest.mark.parametrize("t0,k", [(0, 1), (0, 2), (0, None), (2, 3)])
@pytest.mark.parametrize("case", EPISODES)
def test_co_tsp_steps(dev, case, t0, k):
    """K steps in one launch from the recorded state before step ``t0``: both ping-pong
    buffers hold the recorded states after the last two steps."""
    locs, actions, states = _tsp_episode(case)
    b, n = actions.shape
    k = k or n
    acts = actions.t().contiguous()[t0:t0 + k].contiguous().to(dev)  # step-major [K, B]
    before = states[t0]
    mask = [before["action_mask"].to(dev), _new(dev, (b, n), torch.bool)]
    i = [before["i"].to(dev), _new(dev, (b, 1), torch.int64)]
    first = [before["first_node"].to(dev), _new(dev, b, torch.int64)]
    cur, done, rew = _new(dev, b, torch.int64), _new(dev, b, torch.bool), _new(dev, b, torch.bool)
    st = _status(dev)
    nat.call("co_tsp_steps", b, n, k, nat.ptr(acts), b, nat.ptr(mask[0]), nat.ptr(i[0]),
             nat.ptr(first[0]), nat.ptr(mask[1]), nat.ptr(i[1]), nat.ptr(first[1]), nat.ptr(cur),
             nat.ptr(done), nat.ptr(rew), int(t0 == 0), nat.ptr(st), nat.stream_of(acts))
    _finish(st)
    for back in range(min(k, 2)):  # step t reads buffer t % 2 and writes the other
        want, j = states[t0 + k - back], (k - back) % 2
        rr.check_equal(mask[j], want["action_mask"], f"mask after step {t0 + k - back}")
        rr.check_equal(i[j], want["i"], "i")
        rr.check_equal(first[j], want["first_node"], "first_node")
    last = states[t0 + k]
    rr.check_equal(cur, last["current_node"], "current_node")
    rr.check_equal(done, last["done"], "done")
    rr.check_equal(rew, last["reward"], "reward")


@pytest.mark.parametrize("layout", ["row_major", "step_major"])
@pytest.mark.parametrize("case", EPISODES)
def test_co_tsp_rollout_ex(dev, case, layout):
    locs, actions, states = _tsp_episode(case)
    b, n = actions.shape
    if layout == "row_major":
        acts, sb, stt = actions.to(dev), n, 1
    else:
        acts, sb, stt = actions.t().contiguous().to(dev), 1, b
    locs = locs.to(dev)
    mask, first, cur = (_new(dev, (b, n), torch.bool), _new(dev, b, torch.int64),
                        _new(dev, b, torch.int64))
    i, done, srew = (_new(dev, (b, 1), torch.int64), _new(dev, b, torch.bool),
                     _new(dev, b, torch.bool))
    reward, st = _new(dev, b, torch.float32), _status(dev)
    nat.call("co_tsp_rollout_ex", b, n, nat.ptr(locs), nat.ptr(acts), sb, stt, None, nat.ptr(mask),
             nat.ptr(first), nat.ptr(cur), nat.ptr(i), nat.ptr(done), nat.ptr(srew),
             nat.ptr(reward), 1, nat.ptr(st), nat.stream_of(locs))
    _finish(st)
    want = states[-1]
    for name, got in (("action_mask", mask), ("first_node", first), ("current_node", cur),
                      ("i", i), ("done", done), ("reward", srew)):
        rr.check_equal(got, want[name], f"{case} {layout} {name}")
    rr.check_close(reward, rr.get("tsp", "TSPEnv.get_reward", case)["out"], "episode reward")


def _logits_for(actions_t, width, seed, greedy):
    """Seeded logits [B, width]; for greedy the recorded action's column holds the row's
    only maximum, so the kernel's own argmax must pick it."""
    lg = torch.randn(actions_t.shape[0], width, generator=torch.Generator().manual_seed(seed))
    if greedy:
        lg[torch.arange(actions_t.shape[0]), actions_t] = lg.max() + 1.0
    return lg


def _unfused_logp(dev, logits, mask, action):
    """co_decode_step's log-probability of ``action`` (pinned to the recordings above)."""
    from rl4co_slap_amd.utils.decoding import decode_step

    _, lp, _ = decode_step(logits, mask, "evaluate", action=action)
    torch.cuda.synchronize()
    return lp.cpu()


@pytest.mark.parametrize("mode", [GREEDY, EVALUATE], ids=["greedy", "evaluate"])
@pytest.mark.parametrize("case", EPISODES)
def test_co_tsp_decode_step(dev, case, mode):
    """Every step of the recorded episode through the fused decode + step launch."""
    locs, actions, states = _tsp_episode(case)
    b, n = actions.shape
    for t in range(n):
        before, want = states[t], states[t + 1]
        logits = _logits_for(actions[:, t], n, 900 + t, mode == GREEDY).to(dev)
        mask_in, i_in = before["action_mask"].to(dev), before["i"].to(dev)
        first_in = before["first_node"].to(dev)
        ain = actions[:, t].contiguous().to(dev) if mode == EVALUATE else None
        act, lp = _new(dev, b, torch.int64), _new(dev, b, torch.float32)
        mask, i, first = (_new(dev, (b, n), torch.bool), _new(dev, (b, 1), torch.int64),
                          _new(dev, b, torch.int64))
        done, rew, st = _new(dev, b, torch.bool), _new(dev, b, torch.bool), _status(dev)
        nat.call("co_tsp_decode_step", b, n, nat.ptr(logits), n, nat.ptr(mask_in), 0.0, 1.0, mode,
                 nat.ptr(ain), nat.ptr(act), nat.ptr(lp), 0, 0, nat.ptr(mask), nat.ptr(i_in),
                 nat.ptr(i), None if t == 0 else nat.ptr(first_in), nat.ptr(first), int(t == 0),
                 nat.ptr(done), nat.ptr(rew), None, nat.ptr(st), nat.stream_of(logits))
        _finish(st)
        if mode == GREEDY:
            rr.check_equal(act, actions[:, t], f"step {t} action")
        for name, got in (("action_mask", mask), ("i", i), ("first_node", first), ("done", done),
                          ("reward", rew)):
            rr.check_equal(got, want[name], f"step {t} {name}")
        rr.check_equal(lp, _unfused_logp(dev, logits, mask_in, actions[:, t].to(dev)),
                       f"step {t} logp")


# -- the C ABI: CVRP ------------------------------------------------------------------------
def _cvrp_episode(case):
    r = rr.get("cvrp", "CVRPEnv._reset", case)
    s = rr.get("cvrp", "CVRPEnv._step", case)
    start = {k: r["out_" + k] for k in ("current_node", "used_capacity", "visited", "action_mask")}
    fixed = {k: r["out_" + k] for k in ("locs", "demand", "vehicle_capacity")}
    return fixed, s["actions"], [start] + rr.stacked_states(s, rr.CVRP_STATE)


CVRP_OUT = ("used_capacity", "visited", "current_node", "done", "reward", "action_mask")


def _cvrp_outputs(dev, b, n):
    return {"used_capacity": _new(dev, (b, 1), torch.float32),
            "visited": _new(dev, (b, n + 1), torch.uint8),
            "current_node": _new(dev, (b, 1), torch.int64), "done": _new(dev, b, torch.bool),
            "reward": _new(dev, b, torch.bool), "action_mask": _new(dev, (b, n + 1), torch.bool)}


def _check_cvrp(o, want, what, rows=None):
    for name in CVRP_OUT:
        g, w = o[name].cpu(), want[name]
        if rows is not None:
            g, w = g[rows], w[rows]
        rr.check_equal(g, w, f"{what} {name}")


@pytest.mark.parametrize("case", EPISODES + ["exact_fill"])
def test_co_cvrp_step(dev, case):
    if case == "exact_fill":
        s = rr.get("cvrp", "CVRPEnv._step", case)
        b, n = s["demand"].shape
        start = {"current_node": torch.zeros(b, 1, dtype=torch.int64),
                 "used_capacity": torch.zeros(b, 1), "visited": torch.zeros(b, n + 1, dtype=torch.uint8)}
        fixed = {"demand": s["demand"], "vehicle_capacity": torch.ones(b, 1)}
        actions, states = s["actions"], [start] + rr.stacked_states(s, rr.CVRP_STATE)
    else:
        fixed, actions, states = _cvrp_episode(case)
    b, n = fixed["demand"].shape
    demand, vcap = fixed["demand"].to(dev), fixed["vehicle_capacity"].to(dev)
    for t in range(actions.shape[1]):
        before = states[t]
        act = actions[:, t].contiguous().to(dev)
        used, vis = before["used_capacity"].to(dev), before["visited"].to(dev)
        o, st = _cvrp_outputs(dev, b, n), _status(dev)
        nat.call("co_cvrp_step", b, n, nat.ptr(act), nat.ptr(demand), nat.ptr(used),
                 nat.ptr(o["used_capacity"]), nat.ptr(vcap), nat.ptr(vis), nat.ptr(o["visited"]),
                 nat.ptr(o["current_node"]), nat.ptr(o["done"]), nat.ptr(o["reward"]),
                 nat.ptr(o["action_mask"]), nat.ptr(st), None, nat.stream_of(act))
        _finish(st)
        _check_cvrp(o, states[t + 1], f"{case} step {t}")


@pytest.mark.parametrize("case", EPISODES)
def test_co_cvrp_nearest_step_where_it_takes_the_recorded_action(dev, case):
    """The nearest-feasible policy fused with the step, from every recorded state: on the
    rows where its action is the recorded one, the recorded next state."""
    fixed, actions, states = _cvrp_episode(case)
    b, n = fixed["demand"].shape
    locs, demand, vcap = (fixed[k].to(dev) for k in ("locs", "demand", "vehicle_capacity"))
    compared = 0
    for t in range(actions.shape[1]):
        before = states[t]
        used, vis = before["used_capacity"].to(dev), before["visited"].to(dev)
        mask_in = before["action_mask"].to(dev)
        cur_in = before["current_node"].squeeze(1).contiguous().to(dev)
        act = _new(dev, b, torch.int64)
        o, st = _cvrp_outputs(dev, b, n), _status(dev)
        nat.call("co_cvrp_nearest_step", b, n, nat.ptr(locs), nat.ptr(demand), nat.ptr(used),
                 nat.ptr(o["used_capacity"]), nat.ptr(vcap), nat.ptr(vis), nat.ptr(o["visited"]),
                 nat.ptr(mask_in), nat.ptr(cur_in), nat.ptr(act), nat.ptr(o["current_node"]),
                 nat.ptr(o["done"]), nat.ptr(o["reward"]), nat.ptr(o["action_mask"]), nat.ptr(st),
                 None, nat.stream_of(locs))
        _finish(st)
        act = act.cpu()
        assert before["action_mask"].gather(1, act[:, None]).all(), "an infeasible action"
        rows = act == actions[:, t]
        compared += int(rows.sum())
        if rows.any():
            _check_cvrp(o, states[t + 1], f"{case} step {t}", rows)
    assert compared >= b  # the forced depot steps at least


@pytest.mark.parametrize("mode", [GREEDY, EVALUATE], ids=["greedy", "evaluate"])
@pytest.mark.parametrize("case", EPISODES)
def test_co_cvrp_decode_step(dev, case, mode):
    fixed, actions, states = _cvrp_episode(case)
    b, n = fixed["demand"].shape
    demand, vcap = fixed["demand"].to(dev), fixed["vehicle_capacity"].to(dev)
    for t in range(actions.shape[1]):
        before = states[t]
        logits = _logits_for(actions[:, t], n + 1, 1900 + t, mode == GREEDY).to(dev)
        mask_in = before["action_mask"].to(dev)
        used, vis = before["used_capacity"].to(dev), before["visited"].to(dev)
        ain = actions[:, t].contiguous().to(dev) if mode == EVALUATE else None
        act, lp = _new(dev, b, torch.int64), _new(dev, b, torch.float32)
        o, st = _cvrp_outputs(dev, b, n), _status(dev)
        nat.call("co_cvrp_decode_step", b, n, nat.ptr(logits), n + 1, nat.ptr(mask_in), 0.0, 1.0,
                 mode, nat.ptr(ain), nat.ptr(act), nat.ptr(lp), 0, 0, nat.ptr(demand),
                 nat.ptr(used), nat.ptr(o["used_capacity"]), nat.ptr(vcap), nat.ptr(vis),
                 nat.ptr(o["visited"]), nat.ptr(o["current_node"]), nat.ptr(o["done"]),
                 nat.ptr(o["reward"]), nat.ptr(o["action_mask"]), None, nat.ptr(st),
                 nat.stream_of(logits))
        _finish(st)
        if mode == GREEDY:
            rr.check_equal(act, actions[:, t], f"step {t} action")
        _check_cvrp(o, states[t + 1], f"{case} step {t}")
        rr.check_equal(lp, _unfused_logp(dev, logits, mask_in, actions[:, t].to(dev)),
                       f"step {t} logp")


# -- the C ABI: SLAP ------------------------------------------------------------------------
SLAP_EPISODES = ["default_b9", "a4l5p19_b5"]


def _slap_episode(case):
    r = rr.get("slap", "SLAPEnv._reset", case)
    s = rr.get("slap", "SLAPEnv._step", case)
    start = {k: r["out_" + k] for k in ("assignment", "to_choose", "action_mask", "i")}
    return r, s["actions"], [start] + rr.stacked_states(s, rr.SLAP_STATE)


@pytest.mark.parametrize("case", SLAP_EPISODES)
def test_co_slap_rollout_teacher_forced(dev, case):
    r, actions, states = _slap_episode(case)
    b, p = actions.shape
    l = r["locs"].shape[1]
    o_, k_ = r["picklist"].shape[1:]
    locs, pick, depot, asg0 = (r[k].contiguous().to(dev) for k in
                               ("locs", "picklist", "depot_loc_dist", "assignment"))
    acts = actions.t().contiguous().to(dev)  # step-major [P, B]
    mask, asg, i = (_new(dev, (b, l), torch.bool), _new(dev, (b, p), torch.int32),
                    _new(dev, (b, 1), torch.int64))
    done, srew = _new(dev, (b, 1), torch.bool), _new(dev, (b, 1), torch.bool)
    reward, ratio, st = _new(dev, b, torch.float32), _new(dev, (b, l), torch.float32), _status(dev)
    nat.call("co_slap_rollout", b, l, p, o_, k_, nat.ptr(locs), nat.ptr(pick), nat.ptr(depot),
             nat.ptr(asg0), nat.ptr(acts), None, nat.ptr(mask), nat.ptr(asg), nat.ptr(i),
             nat.ptr(done), nat.ptr(srew), nat.ptr(reward), nat.ptr(ratio), nat.ptr(st),
             nat.stream_of(locs))
    _finish(st)
    want = states[-1]
    for name, got in (("action_mask", mask), ("assignment", asg), ("i", i), ("done", done),
                      ("reward", srew)):
        rr.check_equal(got, want[name], f"{case} {name}")
    rr.check_equal(ratio, r["out_ratio"], "ratio")
    rr.check_close(reward, rr.get("slap", "SLAPEnv._get_reward", case)["out"], "episode reward")


@pytest.mark.parametrize("mode", [GREEDY, EVALUATE], ids=["greedy", "evaluate"])
@pytest.mark.parametrize("case", SLAP_EPISODES)
def test_co_slap_decode_step(dev, case, mode):
    r, actions, states = _slap_episode(case)
    b, p = actions.shape
    l = r["locs"].shape[1]
    for t in range(p):
        before, want = states[t], states[t + 1]
        logits = _logits_for(actions[:, t], l, 2900 + t, mode == GREEDY).to(dev)
        mask_in, i_in = before["action_mask"].to(dev), before["i"].to(dev)
        tc, asg_in = before["to_choose"].contiguous().to(dev), before["assignment"].to(dev)
        ain = actions[:, t].contiguous().to(dev) if mode == EVALUATE else None
        act, lp = _new(dev, b, torch.int64), _new(dev, b, torch.float32)
        asg, mask, i = (_new(dev, (b, p), torch.int32), _new(dev, (b, l), torch.bool),
                        _new(dev, (b, 1), torch.int64))
        done, rew, st = _new(dev, (b, 1), torch.bool), _new(dev, (b, 1), torch.bool), _status(dev)
        nat.call("co_slap_decode_step", b, l, p, nat.ptr(logits), l, nat.ptr(mask_in), 0.0, 1.0,
                 mode, nat.ptr(ain), nat.ptr(act), nat.ptr(lp), 0, 0, nat.ptr(tc), tc.stride(0),
                 nat.ptr(asg_in), nat.ptr(asg), nat.ptr(mask), nat.ptr(i_in), nat.ptr(i),
                 nat.ptr(done), nat.ptr(rew), None, nat.ptr(st), nat.stream_of(logits))
        _finish(st)
        if mode == GREEDY:
            rr.check_equal(act, actions[:, t], f"step {t} action")
        for name, got in (("assignment", asg), ("action_mask", mask), ("i", i), ("done", done),
                          ("reward", rew)):
            rr.check_equal(got, want[name], f"{case} step {t} {name}")
        rr.check_equal(lp, _unfused_logp(dev, logits, mask_in, actions[:, t].to(dev)),
                       f"step {t} logp")
