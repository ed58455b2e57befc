"""The orienteering env (OPEnv, ``op``) without a GPU: the host build of the C ABI is held to
the recording of the reference's own OPEnv (tests/golden/op/ref_op.npz: masks, ``visited``,
nodes, ``i``, ``done`` and ``current_total_prize`` bit for bit, ``tour_length`` and
``max_length`` within the recorder's drift bound, ``get_reward`` within the project's 1e-5
relative, the tampered rows raising the recorded messages) and, bit for bit on every output,
floats included, to the restatement tests/op_ref.py written from the header: reset / step /
the mask alone / co_op_steps in both action layouts with ``feasible`` and ``length`` at N = 1
(a row of 2), at N + 1 on both sides of every switch of op_launch and of the fused step's row
engines (16 | 17, 32 | 33, 64 | 65, 128 | 129, 256 | 257, 512 | 513) and at the largest N
the entries take (1023, CO_OP_MAX_N), with B = 1, 3, 16 and 257; the directed episodes (the
depot at step 0, the depot after customers and steps after ``done``, every column the action
once, a row closed by the length test alone, a NaN coordinate, actions out of range); the
reward and its status bits on 300 rows, T = 1 and the multistart layout.  The generator
reproduces the reference's draws for the three prize types, and the Python surface (registry,
td contract, decode loops, multistart, evaluate_policy, bindings) is checked.
tests/test_gpu_op.py runs the same checks on the device, and the fused decode step."""
import os
import re

import pytest
import torch

import op_cases as oc
from ref_recordings import check_equal

import rl4co_slap_amd as ra
from rl4co_slap_amd import TensorDict, _native as nat
from rl4co_slap_amd.data import TensorDictDataset
from rl4co_slap_amd.envs import (ENV_REGISTRY, IMPROVEMENT_ENV_REGISTRY, MULTITASK_ENV_REGISTRY,
                                 ORIENTEERING_ENV_REGISTRY, PICKUP_DELIVERY_ENV_REGISTRY,
                                 ROUTING_VARIANT_ENV_REGISTRY, OPEnv, OPGenerator, get_env)
from rl4co_slap_amd.rollout import ConstructivePolicy
from rl4co_slap_amd.rollout.constructive import LogitsDecoder
from rl4co_slap_amd.tasks import eval as ev
from rl4co_slap_amd.utils.decoding import Greedy, random_policy, rollout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("co_op_reset", "co_op_step", "co_op_action_mask", "co_op_steps", "co_op_reward")


@pytest.mark.parametrize("policy", oc.POLICIES)
@pytest.mark.parametrize("case", oc.recorded_cases())
def test_host_matches_the_recording(case, policy):
    oc.check_recorded_case(case, policy, "cpu")


def test_recorded_cases():
    """(N, B) = (5, 16), (20, 16), (50, 16), (70, 8) with ``dist`` prizes, (20, 16) with
    ``unif`` and ``const``; both policies; every case clear of the recorder's margin."""
    assert oc.recorded_cases() == ["n20b16_const", "n20b16_dist", "n20b16_unif", "n50b16_dist",
                                   "n5b16_dist", "n70b8_dist"]
    for case in oc.recorded_cases():
        r = oc.recorded(case)
        b = r["gen_locs"].shape[0]
        assert r["draws"] <= 400
        for policy in oc.POLICIES:
            acts = r[policy + "/step_action"]
            assert acts.shape[1] == b and (acts[-1] == 0).all()
            assert r["margin"] >= 8 * (acts.shape[0] + 2) * 7.2e-7 and r["gap"] >= r["margin"]
            assert r[policy + "/tamper_double_message"] == "Duplicates"
            assert r[policy + "/tamper_short_message"].startswith("Max length exceeded")


@pytest.mark.parametrize("case", oc.recorded_cases())
def test_generator_reproduces_the_reference_draws(case):
    r = oc.recorded(case)
    b, n = r["gen_locs"].shape[:2]
    torch.manual_seed(r["seed"])
    with pytest.warns(UserWarning, match="max length") if n not in (20, 50, 100) \
            else oc._quiet():
        gen = OPGenerator(num_loc=n, prize_type=case.rsplit("_", 1)[1])
    td = gen([b])
    for key in ("locs", "depot", "prize", "max_length"):
        assert td[key].dtype == r["gen_" + key].dtype, key
        check_equal(td[key], r["gen_" + key], f"{case} {key}")


def test_generator_arguments():
    with pytest.warns(UserWarning, match="closest max length: 3.0 with 50"):
        assert OPGenerator(num_loc=70).max_length == 3.0
    assert OPGenerator(num_loc=100).max_length == 4.0
    assert OPGenerator(num_loc=100, max_length=2.5).max_length == 2.5
    budget = torch.tensor([1.0, 2.0, 3.0])
    torch.manual_seed(1)
    td = OPGenerator(num_loc=20, max_length=budget, prize_type="const")([3])
    assert td["max_length"] is budget and bool((td["prize"] == 1).all())
    torch.manual_seed(1)
    both = Uniform01(21)
    assert torch.equal(td["depot"], both[:, 0]) and torch.equal(td["locs"], both[:, 1:])
    torch.manual_seed(1)
    split = OPGenerator(num_loc=20, depot_distribution="uniform")([3])
    assert split["locs"].shape == (3, 20, 2) and not torch.equal(split["locs"], td["locs"])
    with pytest.raises(ValueError, match="Invalid prize_type"):
        OPGenerator(num_loc=20, prize_type="other")([2])
    with pytest.raises(AssertionError, match="Invalid prize_type"):
        OPEnv(prize_type="other")


def Uniform01(rows):
    return torch.distributions.Uniform(0.0, 1.0).sample((3, rows, 2))


@pytest.mark.parametrize("b", oc.BATCHES)
@pytest.mark.parametrize("n", oc.SIZES)
def test_host_matches_the_restatement(n, b):
    oc.check_shape(n, b, "cpu")


@pytest.mark.parametrize("n", oc.SIZES)
def test_every_column_is_the_action_once(n):
    oc.check_every_column(n, "cpu")


def test_hand_made_rows():
    oc.check_hand_made("cpu")


def test_reward_and_status_bits_over_two_blocks():
    oc.check_reward_two_blocks("cpu")


def test_reward_sizes_and_multistart_layout():
    oc.check_reward_sizes("cpu")
    oc.check_multistart_reward("cpu")


@pytest.mark.parametrize("which", ["host", "device"])
def test_invalid_arguments(which):
    oc.check_invalid_arguments(nat.load_host() if which == "host" else nat.load())


def test_header_native_and_host_bindings():
    header = open(os.path.join(ROOT, "include", "co_env.h")).read()
    declared = set(re.findall(r"\bint\s+(co_\w+)\s*\(", header))
    for name in SYMBOLS + ("co_op_decode_step",):
        assert name in declared and name in nat._SIGS, name
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header).group(1)
        assert len(nat._SIGS[name]) == decl.count(",") + 1, name
        assert hasattr(nat.load(), name)
        kinds = [nat._KIND[t] for t in nat._SIGS[name]]
        assert sum(k == "i" for k in kinds) <= 28, name  # the fast-call trampoline's limit
    for name in SYMBOLS:
        assert name in nat.HOST_SYMBOLS and hasattr(nat.load_host(), name), name
    assert "co_op_decode_step" not in nat.HOST_SYMBOLS  # the host loop takes the two calls
    assert f"#define CO_OP_MAX_N {nat.OP_MAX_N}" in header and nat.OP_MAX_N >= 1023
    assert f"#define CO_ST_OP_DUPLICATE {nat.ST_OP_DUPLICATE}" in header
    assert f"#define CO_ST_OP_LENGTH {nat.ST_OP_LENGTH}" in header
    assert f"#define CO_ST_OP_SINGLE_NONZERO {nat.ST_OP_SINGLE_NONZERO}" in header
    assert (nat.ST_OP_DUPLICATE, nat.ST_OP_LENGTH) == (4194304, 8388608)
    bits = [int(v) for v in re.findall(r"#define CO_ST_\w+ (\d+)", header)]
    assert len(bits) == len(set(bits)) and all(v & (v - 1) == 0 for v in bits)
    fast = nat._fastcall()
    assert fast is not None
    for name in SYMBOLS:
        assert len(fast.table("host")[name][1]) == len(nat._SIGS[name]), name
    # the fused entry through the trampoline itself: a NULL instance table is refused by the
    # entry (CO_E_INVAL), not by the call path
    kinds = fast.table("dev")["co_op_decode_step"]
    assert len(kinds[1]) == len(nat._SIGS["co_op_decode_step"])
    assert fast.invoke(kinds[0], kinds[1], 1, 4, 0, 5, 0, 0.0, 1.0, 0, *([0] * 22)) == -1
    assert fast.invoke(kinds[0], kinds[1], 0, 4, 0, 5, 0, 0.0, 1.0, 0, *([0] * 22)) == 0
    assert isinstance(nat.op_instance(None, None, None).address, int)


def test_registry_and_api():
    registries = (ENV_REGISTRY, IMPROVEMENT_ENV_REGISTRY, ROUTING_VARIANT_ENV_REGISTRY,
                  MULTITASK_ENV_REGISTRY, PICKUP_DELIVERY_ENV_REGISTRY, ORIENTEERING_ENV_REGISTRY)
    names = [k for reg in registries for k in reg]
    assert len(names) == len(set(names)) == 8  # disjoint
    assert ORIENTEERING_ENV_REGISTRY == {"op": OPEnv}
    for name in ("OPEnv", "OPGenerator", "ORIENTEERING_ENV_REGISTRY"):
        assert getattr(ra, name) is getattr(ra.envs, name) and name in ra.__all__
    n, b = 20, 6
    env = get_env("op", generator_params=dict(num_loc=n), device="cpu", seed=11)
    assert isinstance(env, OPEnv) and env.name == "op" and env.prize_type == "dist"
    assert isinstance(get_env("op", device="cpu").generator, OPGenerator)  # the defaults
    with pytest.raises(ValueError):
        get_env("pctsp")
    td = env.reset(batch_size=[b])
    want = {"locs": (torch.float32, (b, n + 1, 2)), "prize": (torch.float32, (b, n + 1)),
            "tour_length": (torch.float32, (b,)), "max_length": (torch.float32, (b, n + 1)),
            "current_node": (torch.int64, (b, 1)), "visited": (torch.bool, (b, n + 1)),
            "current_total_prize": (torch.float32, (b,)), "i": (torch.int64, (b,)),
            "action_mask": (torch.bool, (b, n + 1)), "done": (torch.bool, (b, 1)),
            "terminated": (torch.bool, (b, 1))}
    for key, (dtype, shape) in want.items():
        assert td[key].dtype == dtype and tuple(td[key].shape) == shape, key
    assert "reward" not in td and env.min_steps_to_done(td) == 2
    assert bool(td["action_mask"][:, 0].all()) and not bool(td["visited"].any())
    assert bool((td["prize"][:, 0] == 0).all())
    check_equal(env.get_action_mask(td), td["action_mask"], "get_action_mask")
    before = {k: td[k] for k in ("visited", "action_mask", "i", "tour_length")}
    kept = {k: v.clone() for k, v in before.items()}
    td = env.step(random_policy(td))["next"]
    for k, v in before.items():  # fresh output tensors per step
        assert td[k] is not v and torch.equal(v, kept[k]), k
    step = {"tour_length": (torch.float32, (b,)), "current_node": (torch.int64, (b, 1)),
            "visited": (torch.bool, (b, n + 1)), "current_total_prize": (torch.float32, (b,)),
            "i": (torch.int64, (b,)), "reward": (torch.bool, (b,)), "done": (torch.bool, (b,)),
            "action_mask": (torch.bool, (b, n + 1))}
    for key, (dtype, shape) in step.items():
        assert td[key].dtype == dtype and tuple(td[key].shape) == shape, key
    assert env.min_steps_to_done(td) == 0
    check_equal(env.get_action_mask(td), td["action_mask"], "get_action_mask after a step")
    assert env.get_num_starts(td) == n
    assert env.select_start_nodes(env.reset(batch_size=[b]), 5).tolist() == \
        [s % n + 1 for s in range(5) for _ in range(b)]
    with pytest.raises(NotImplementedError, match="op"):
        env.local_search(td, torch.zeros(b, 3, dtype=torch.int64))
    with pytest.raises(NotImplementedError, match="op"):
        env.improve(td, torch.zeros(b, 3, dtype=torch.int64))
    assert env.native_decode_and_step() is None and callable(env.decode_and_step)
    # an action outside 0..N: torch's scatter raises; here step_many and the reward do
    with pytest.raises(RuntimeError, match="index out of range"):
        env.step_many(env.reset(batch_size=[b]), torch.full((b, 2), n + 1))
    with pytest.raises(RuntimeError, match="index out of range"):
        env._get_reward(td, torch.full((b, 3), n + 1), check=False)
    with pytest.raises(AssertionError, match="Duplicates"):
        env.check_solution_validity(td, torch.tensor([[3, 3, 0]] * b))
    with pytest.raises(AssertionError, match="Max length exceeded"):
        short = td.clone()
        short.set("max_length", td["max_length"] - 100)
        env.check_solution_validity(short, torch.tensor([[3, 4, 0]] * b))
    with pytest.raises(AssertionError, match="they should be zero"):
        env.get_reward(td, torch.ones(b, 1, dtype=torch.int64))
    assert env.get_reward(td, torch.zeros(b, 1, dtype=torch.int64)).tolist() == [0.0] * b
    with pytest.raises(ValueError):
        env.step_many(env.reset(batch_size=[b]), torch.zeros(b + 1, 2, dtype=torch.int64))


def test_select_start_nodes_redraws_when_a_row_has_too_few_open_customers():
    """``ops.py:164-174``: a hand-made mask with two open customers in row 1 and five starts:
    every row's starts are then drawn (with replacement) from its own open customers."""
    n, b, starts = 8, 3, 5
    env = get_env("op", generator_params=dict(num_loc=n, max_length=2.0), device="cpu")
    td = env.reset(batch_size=[b])
    mask = torch.ones(b, n + 1, dtype=torch.bool)
    mask[1, 1:] = False
    mask[1, [2, 7]] = True
    td.set("action_mask", mask)
    torch.manual_seed(3)
    sel = env.select_start_nodes(td, starts)
    torch.manual_seed(3)
    want = torch.multinomial(mask[:, 1:].float(), starts, replacement=True) + 1
    assert torch.equal(sel, want.t().reshape(-1)) and sel.shape == (starts * b,)
    assert set(sel.reshape(starts, b)[:, 1].tolist()) <= {2, 7}
    assert bool(mask.gather(1, sel.reshape(starts, b).t()).all()) and bool((sel >= 1).all())
    td.set("action_mask", torch.ones(b, n + 1, dtype=torch.bool))  # enough everywhere: POMO's
    assert env.select_start_nodes(td, starts).tolist() == \
        [s % n + 1 for s in range(starts) for _ in range(b)]


def stand_in_logits(seed=0):
    """A small seeded stand-in policy: minus the distance to the current node plus a seeded
    linear score of the coordinates and the prize; the depot scores low."""
    w = torch.randn(2, generator=torch.Generator().manual_seed(seed))

    def logits(td):
        locs, cur = td["locs"], td["current_node"].reshape(-1)
        here = locs[torch.arange(locs.shape[0], device=locs.device), cur]
        out = locs @ w.to(locs.device) - (locs - here[:, None]).norm(dim=-1) + td["prize"]
        out[:, 0] = -3.0
        return out.contiguous()

    return logits


def _policy(seed=0):
    return ConstructivePolicy(None, LogitsDecoder(stand_in_logits(seed)), env_name="op")


def run_decode_loops(device, n=20, b=8, fused=False):
    """rollout with the random policy, the constructive loop (greedy, sampling, POMO
    multistart with select_start_nodes) and evaluate_policy's multistart_greedy all finish
    with valid solutions (check_solution=True) although the rows finish at different steps;
    with ``fused`` the device loop takes co_op_decode_step, else the two calls."""
    env = get_env("op", generator_params=dict(num_loc=n), device=device, seed=5,
                  check_solution=True)
    env.fused_step = fused
    torch.manual_seed(5)
    reward, td, acts = rollout(env, env.reset(batch_size=[b]), random_policy)
    env.check_solution_validity(td, acts)
    assert reward.shape == (b,) and bool(td["done"].all()) and bool((acts[:, -1] == 0).all())
    s = Greedy()
    td = env.reset(batch_size=[b])
    took = s.step_env_fused(stand_in_logits()(td), td["action_mask"], td, env)
    assert (took is not None) == (fused and device != "cpu")
    results = {}
    for kind, kw in (("greedy", {}), ("sampling", {}), ("multistart_greedy", dict(num_starts=4))):
        torch.manual_seed(100 + len(results))  # the same instances on every device
        td = env.reset(batch_size=[b])
        inst = td.clone()
        out = _policy()(td, env, phase="test", decode_type=kind, return_actions=True, **kw)
        rows = b * (4 if kw else 1)
        acts = out["actions"]
        assert acts.shape[0] == rows and out["reward"].shape == (rows,), kind
        assert bool((out["reward"] > 0).all()) and bool((acts[:, -1] == 0).all())
        ends = (acts == 0).int().argmax(1)  # rows finish at different steps, padded with 0
        assert len(set(ends.tolist())) > 1 or kind != "greedy"
        assert all(bool((acts[r, e:] == 0).all()) for r, e in enumerate(ends.tolist()))
        if kw:
            assert acts[:, 0].tolist() == [s_ + 1 for s_ in range(4) for _ in range(b)]
        else:
            check_equal(out["reward"].cpu(), env.get_reward(inst, acts).cpu(), kind)
        results[kind] = out
    torch.manual_seed(7)
    data = env.generator([5])
    res = ev.evaluate_policy(env, _policy(), TensorDictDataset(data), method="multistart_greedy",
                             auto_batch_size=False, batch_size=2, progress=False)
    assert res["rewards"].shape == (5,) and res["actions"].shape[0] == 5
    cpu_env = OPEnv(generator_params=dict(num_loc=n), device="cpu", check_solution=True)
    td_all = cpu_env.reset(TensorDict({k: v.clone().cpu() for k, v in data.items()}, [5]))
    got = cpu_env.get_reward(td_all, res["actions"].cpu())  # valid, and scores to its reward
    assert torch.allclose(got, res["rewards"].cpu(), rtol=1e-5, atol=1e-6)
    return results


def test_decode_loops():
    run_decode_loops("cpu")


def test_step_many_matches_single_steps():
    n, b = 20, 5
    env = get_env("op", generator_params=dict(num_loc=n), device="cpu", seed=3)
    torch.manual_seed(3)
    inst = env.generator([b])
    _, one, acts = rollout(env, env.reset(inst.clone()), random_policy)
    for step_major in (False, True):
        td = env.reset(inst.clone())
        held = td["visited"]
        feasible, length = env.step_many(td, acts.t() if step_major else acts,
                                         step_major=step_major)
        assert bool(feasible.all()) and feasible.shape == length.shape == acts.t().shape
        assert td["visited"] is not held and not bool(held.any())
        check_equal(length[-1], one["tour_length"], "length")
        for key in ("current_node", "visited", "tour_length", "current_total_prize", "i",
                    "action_mask", "done", "reward"):
            check_equal(td[key].reshape(one[key].shape), one[key], key)
    # the depot first closes every customer: the second action is infeasible, still stepped
    td = env.reset(inst.clone())
    feasible, _ = env.step_many(td, torch.tensor([[0, 4, 0]] * b))
    assert feasible.t().tolist() == [[True, False, True]] * b and bool(td["done"].all())
