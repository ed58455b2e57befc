"""The pickup-and-delivery env (PDPEnv, ``pdp``) without a GPU: the host build of the C ABI is
held to the recording of the reference's own PDPEnv (tests/golden/pdp/ref_pdp.npz: masks, the
two sets, nodes, counters and coordinates bit for bit, ``get_reward`` within the project's
1e-5 relative, the tampered rows raising the recorded messages) and, bit for bit on every
output, to the restatement tests/pdp_ref.py written from the header: reset / step /
co_pdp_steps in both action layouts at N = 2 (a row of 3), at N + 1 on both sides of every
switch of pdp_launch (the lanes per row double at N + 1 = 32, 64, 128, 256, 512, 1024, so
N = 30 | 32, 62 | 64, 126 | 128, 254 | 256, 510 | 512, 1022 | 1024) and at the largest N the
entries take (2046, CO_PDP_MAX_N), with B = 1, 3, 16 and 257; full episodes in which every
column is the action's and the pair's; hand-made rows; the reward and its validity bits on 300
rows.  The generator reproduces the reference's draws, and the Python surface (registry, td
contract, decode loops, multistart, evaluate_policy, bindings) is checked.
tests/test_gpu_pdp.py runs the same checks on the device, and the fused decode step."""
import os
import re

import pytest
import torch

import pdp_cases as pc
from ref_recordings import check_equal

import rl4co_slap_amd as ra
from rl4co_slap_amd import TensorDict, _native as nat
from rl4co_slap_amd.data import TensorDictDataset
from rl4co_slap_amd.envs import (ENV_REGISTRY, IMPROVEMENT_ENV_REGISTRY, MULTITASK_ENV_REGISTRY,
                                 PICKUP_DELIVERY_ENV_REGISTRY, ROUTING_VARIANT_ENV_REGISTRY,
                                 CVRPEnv, CVRPTWEnv, MTVRPEnv, PDPEnv, PDPGenerator, SLAPEnv,
                                 TSPEnv, TSPkoptEnv, get_env)
from rl4co_slap_amd.rollout import ConstructivePolicy
from rl4co_slap_amd.rollout.constructive import LogitsDecoder
from rl4co_slap_amd.tasks import eval as ev
from rl4co_slap_amd.utils.decoding import Greedy, random_policy, rollout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("co_pdp_reset", "co_pdp_step", "co_pdp_steps", "co_pdp_reward")
EPISODES = [c for c in pc.recorded_cases() if not c.endswith("_multistart")]


@pytest.mark.parametrize("policy", pc.POLICIES)
@pytest.mark.parametrize("case", EPISODES)
def test_host_matches_the_recording(case, policy):
    pc.check_recorded_case(case, policy, "cpu")


def test_host_matches_the_recorded_multistart_episode():
    pc.check_recorded_multistart("cpu")


def test_recorded_cases():
    """N = 2, 4, 20, 50, 70 with 16 rows (8 at N = 70), both policies, and the multistart
    episode whose first action is a pickup taken from the reset state."""
    assert pc.recorded_cases() == ["n20b16", "n20b4_multistart", "n2b16", "n4b16", "n50b16",
                                   "n70b8"]
    for case in EPISODES:
        r = pc.recorded(case)
        b, n = r["gen_locs"].shape[:2]
        for policy in pc.POLICIES:
            assert r[policy + "/step_action"].shape == (n + 1, b)
            assert (r[policy + "/step_action"][0] == 0).all()
    r = pc.recorded("n20b4_multistart")
    first = r["random/step_action"][0]
    assert ((first >= 1) & (first <= 10)).all() and r["random/step_action"].shape == (21, 40)


@pytest.mark.parametrize("case", pc.recorded_cases())
def test_generator_reproduces_the_reference_draws(case):
    r = pc.recorded(case)
    b, n = r["gen_locs"].shape[:2]
    torch.manual_seed(r["seed"])
    td = PDPGenerator(num_loc=n)([b])
    for key in ("locs", "depot"):
        assert td[key].dtype == r["gen_" + key].dtype, key
        check_equal(td[key], r["gen_" + key], f"{case} {key}")


@pytest.mark.parametrize("b", pc.BATCHES)
@pytest.mark.parametrize("n", pc.SIZES)
def test_host_matches_the_restatement(n, b):
    pc.check_shape(n, b, "cpu")


@pytest.mark.parametrize("n", pc.SIZES)
def test_every_column_is_the_action_and_the_pair(n):
    """The full episode: every column -- every bit position of every lane's word -- is the
    action's and the pair's at least once, asserted from the restatement before any entry is
    compared, through single steps and co_pdp_steps in both action layouts."""
    pc.check_directed_inputs(n, 2)
    pc.check_shape(n, 2, "cpu", full=True)


def test_hand_made_rows():
    pc.check_hand_made("cpu")


def test_reward_and_validity_bits_over_two_blocks():
    pc.check_reward_two_blocks("cpu")


def test_reward_sizes_and_multistart_layout():
    pc.check_reward_sizes("cpu")
    pc.check_multistart_reward("cpu")


@pytest.mark.parametrize("which", ["host", "device"])
def test_invalid_arguments(which):
    pc.check_invalid_arguments(nat.load_host() if which == "host" else nat.load())


def test_header_native_and_host_bindings():
    header = open(os.path.join(ROOT, "include", "co_env.h")).read()
    declared = set(re.findall(r"\bint\s+(co_\w+)\s*\(", header))
    for name in SYMBOLS + ("co_pdp_decode_step",):
        assert name in declared and name in nat._SIGS, name
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header).group(1)
        assert len(nat._SIGS[name]) == decl.count(",") + 1, name
        assert hasattr(nat.load(), name)
        kinds = [nat._KIND[t] for t in nat._SIGS[name]]
        assert sum(k == "i" for k in kinds) <= 28, name  # the fast-call trampoline's limit
    for name in SYMBOLS:
        assert name in nat.HOST_SYMBOLS and hasattr(nat.load_host(), name), name
    assert "co_pdp_decode_step" not in nat.HOST_SYMBOLS  # the host loop takes the two calls
    assert f"#define CO_PDP_MAX_N {nat.PDP_MAX_N}" in header and nat.PDP_MAX_N >= 1022
    assert f"#define CO_ST_PDP_NOT_ALL_NODES {nat.ST_PDP_NOT_ALL_NODES}" in header
    assert f"#define CO_ST_PDP_PRECEDENCE {nat.ST_PDP_PRECEDENCE}" in header
    assert (nat.ST_PDP_NOT_ALL_NODES, nat.ST_PDP_PRECEDENCE) == (1048576, 2097152)
    fast = nat._fastcall()
    assert fast is not None
    for name in SYMBOLS:
        assert len(fast.table("host")[name][1]) == len(nat._SIGS[name]), name


def test_registry_and_api():
    assert set(ENV_REGISTRY) == {"tsp", "cvrp", "slap"}
    assert ENV_REGISTRY == {"cvrp": CVRPEnv, "tsp": TSPEnv, "slap": SLAPEnv}
    assert IMPROVEMENT_ENV_REGISTRY == {"tsp_kopt": TSPkoptEnv}
    assert ROUTING_VARIANT_ENV_REGISTRY == {"cvrptw": CVRPTWEnv}
    assert MULTITASK_ENV_REGISTRY == {"mtvrp": MTVRPEnv}
    assert PICKUP_DELIVERY_ENV_REGISTRY == {"pdp": PDPEnv}
    for name in ("PDPEnv", "PDPGenerator", "PICKUP_DELIVERY_ENV_REGISTRY"):
        assert getattr(ra, name) is getattr(ra.envs, name) and name in ra.__all__
    n, b = 8, 6
    env = get_env("pdp", generator_params=dict(num_loc=n), device="cpu", seed=11)
    assert isinstance(env, PDPEnv) and env.name == "pdp"
    with pytest.raises(ValueError):
        get_env("mpdp")
    with pytest.warns(UserWarning, match="must be even"):
        assert PDPGenerator(num_loc=7).num_loc == 8
    td = env.reset(batch_size=[b])
    want = {"locs": (torch.float32, (b, n + 1, 2)), "depot": (torch.float32, (b, 2)),
            "current_node": (torch.int64, (b, 1)), "i": (torch.int64, (b, 1)),
            "available": (torch.bool, (b, n + 1)), "to_deliver": (torch.bool, (b, n + 1)),
            "action_mask": (torch.bool, (b, n + 1)), "done": (torch.bool, (b, 1)),
            "terminated": (torch.bool, (b, 1))}
    for key, (dtype, shape) in want.items():
        assert td[key].dtype == dtype and tuple(td[key].shape) == shape, key
    assert "reward" not in td and env.min_steps_to_done(td) == n + 1
    assert td["action_mask"].tolist() == [[True] + [False] * n] * b
    assert td["to_deliver"].tolist() == [[True] * (n // 2 + 1) + [False] * (n // 2)] * b
    before = {k: td[k] for k in ("available", "to_deliver", "action_mask", "i")}
    kept = {k: v.clone() for k, v in before.items()}
    td = env.step(random_policy(td))["next"]
    for k, v in before.items():  # fresh output tensors per step
        assert td[k] is not v and torch.equal(v, kept[k]), k
    assert env.min_steps_to_done(td) == n and td["done"].shape == (b,)
    assert env.get_action_mask(td) is td["action_mask"]
    assert env.get_num_starts(td) == n // 2
    assert env.select_start_nodes(td, 5).tolist() == [s % 4 + 1 for s in range(5) for _ in range(b)]
    with pytest.raises(NotImplementedError, match="pdp"):
        env.local_search(td, torch.zeros(b, 3, dtype=torch.int64))
    with pytest.raises(NotImplementedError, match="pdp"):
        env.improve(td, torch.zeros(b, 3, dtype=torch.int64))
    assert env.native_decode_and_step() is None and callable(env.decode_and_step)
    # an action outside 0..N: torch's scatter raises; here step_many and the reward do
    with pytest.raises(RuntimeError, match="index out of range"):
        env.step_many(env.reset(batch_size=[b]), torch.full((b, 2), n + 1))
    with pytest.raises(RuntimeError, match="index out of range"):
        env._get_reward(td, torch.full((b, n + 1), n + 1), check=False)
    with pytest.raises(AssertionError, match="Not visiting all nodes"):  # the check comes first
        env.get_reward(td, torch.full((b, n + 1), n + 1))
    with pytest.raises(ValueError):
        env.step_many(env.reset(batch_size=[b]), torch.zeros(b + 1, 2, dtype=torch.int64))


def stand_in_logits(seed=0):
    """A small seeded stand-in policy: minus the distance to the current node plus a seeded
    linear score of the coordinates."""
    w = torch.randn(2, generator=torch.Generator().manual_seed(seed))

    def logits(td):
        locs, cur = td["locs"], td["current_node"].reshape(-1)
        here = locs[torch.arange(locs.shape[0], device=locs.device), cur]
        return (locs @ w.to(locs.device) - (locs - here[:, None]).norm(dim=-1)).contiguous()

    return logits


def _policy(seed=0):
    return ConstructivePolicy(None, LogitsDecoder(stand_in_logits(seed)), env_name="pdp")


def run_decode_loops(device, n=12, b=8):
    """rollout with the random policy, the constructive loop (greedy, sampling, POMO
    multistart with select_start_nodes) and evaluate_policy's multistart_greedy all finish
    with valid solutions (check_solution=True); on the device the loop takes the fused
    co_pdp_decode_step, on the host the two calls."""
    env = get_env("pdp", generator_params=dict(num_loc=n), device=device, seed=5,
                  check_solution=True)
    torch.manual_seed(5)
    reward, td, acts = rollout(env, env.reset(batch_size=[b]), random_policy)
    env.check_solution_validity(td, acts)
    assert reward.shape == (b,) and bool(td["done"].all()) and acts.shape == (b, n + 1)
    s = Greedy()
    td = env.reset(batch_size=[b])
    logits = stand_in_logits()(td)
    fused = s.step_env_fused(logits, td["action_mask"], td, env)
    assert (fused is not None) == (device != "cpu")
    if fused is not None:  # the first step is the depot, whatever the logits
        assert td["action"].tolist() == [0] * b and int(td["i"][0]) == 1
        assert env.min_steps_to_done(td) == n
    results = {}
    for kind, kw in (("greedy", {}), ("sampling", {}),
                     ("multistart_greedy", dict(num_starts=n // 2))):
        torch.manual_seed(100 + len(results))  # the same instances on every device
        td = env.reset(batch_size=[b])
        inst = td.clone()
        out = _policy()(td, env, phase="test", decode_type=kind, return_actions=True, **kw)
        rows = b * (n // 2 if kw else 1)
        assert out["actions"].shape == (rows, n + 1) and out["reward"].shape == (rows,), kind
        assert bool((out["reward"] < 0).all())
        if kw:  # the first action of start s is pickup s + 1, then the depot comes later
            assert out["actions"][:, 0].tolist() == [s + 1 for s in range(n // 2) for _ in range(b)]
            assert bool((out["actions"][:, 1:] == 0).any(1).all())
        else:
            assert out["actions"][:, 0].tolist() == [0] * b
            check_equal(out["reward"].cpu(), env.get_reward(inst, out["actions"]).cpu(), kind)
        results[kind] = out
    torch.manual_seed(7)
    data = env.generator([5])
    res = ev.evaluate_policy(env, _policy(), TensorDictDataset(data), method="multistart_greedy",
                             auto_batch_size=False, batch_size=2, progress=False)
    assert res["rewards"].shape == (5,) and res["actions"].shape == (5, n + 1)
    cpu_env = PDPEnv(generator_params=dict(num_loc=n), device="cpu", check_solution=True)
    td_all = cpu_env.reset(TensorDict({k: v.clone().cpu() for k, v in data.items()}, [5]))
    got = cpu_env.get_reward(td_all, res["actions"].cpu())  # valid, and scores to its reward
    assert torch.allclose(got, res["rewards"].cpu(), rtol=1e-5, atol=1e-6)
    return results


def test_decode_loops():
    run_decode_loops("cpu")


def test_step_many_matches_single_steps():
    n, b = 12, 5
    env = get_env("pdp", generator_params=dict(num_loc=n), device="cpu", seed=3)
    torch.manual_seed(3)
    inst = env.generator([b])
    _, one, acts = rollout(env, env.reset(inst.clone()), random_policy)
    for step_major in (False, True):
        td = env.reset(inst.clone())
        held = td["available"]
        feasible = env.step_many(td, acts.t() if step_major else acts, step_major=step_major)
        assert bool(feasible.all()) and feasible.shape == acts.t().shape
        assert td["available"] is not held and bool(held.all())
        assert env.min_steps_to_done(td) == 0
        for key in ("current_node", "available", "to_deliver", "i", "action_mask", "done",
                    "reward"):
            check_equal(td[key].reshape(one[key].shape), one[key], key)
    # a delivery before its pickup: infeasible, reported and still stepped
    td = env.reset(inst.clone())
    feasible = env.step_many(td, torch.tensor([[0, n, 1]] * b))
    assert feasible.t().tolist() == [[True, False, True]] * b
