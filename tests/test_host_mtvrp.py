"""The multi-task VRP (MTVRPEnv, ``mtvrp``) without a GPU: the host build of the C ABI is
held to the recording of the reference's own MTVRPEnv (tests/golden/mtvrp/ref_mtvrp.npz:
masks, visited sets, nodes, ``done`` and the capacities bit for bit, ``current_time`` /
``current_route_length`` / ``get_reward`` within the project's 1e-5 relative; the tampered
rows raise the reference's messages) and, bit for bit on every output, to the restatement
tests/mtvrp_ref.py written from the header, on batches that mix all four flags per row; the
generator reproduces the reference's draws for seven presets; and the Python surface
(registry, bindings, td contract, decode loops on the two-call path, ``step_many``) is
checked.  tests/test_gpu_mtvrp.py runs the same checks on the device."""
import os
import subprocess
import sys

import pytest
import torch

import mtvrp_cases as mc
from ref_recordings import check_equal

import rl4co_slap_amd as ra
from rl4co_slap_amd import _native as nat
from rl4co_slap_amd.envs import (ENV_REGISTRY, IMPROVEMENT_ENV_REGISTRY, MULTITASK_ENV_REGISTRY,
                                 ROUTING_VARIANT_ENV_REGISTRY, CVRPTWEnv, MTVRPEnv,
                                 MTVRPGenerator, TSPkoptEnv, get_env)
from rl4co_slap_amd.envs.mtvrp import VARIANT_GENERATION_PRESETS, get_vehicle_capacity
from rl4co_slap_amd.rollout import ConstructivePolicy
from rl4co_slap_amd.rollout.constructive import LogitsDecoder
from rl4co_slap_amd.utils.decoding import Greedy, random_policy, rollout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("co_mtvrp_reset", "co_mtvrp_step", "co_mtvrp_action_mask", "co_mtvrp_steps",
           "co_mtvrp_reward", "co_mtvrp_check")


@pytest.mark.parametrize("policy", mc.POLICIES)
@pytest.mark.parametrize("case", mc.recorded_cases())
def test_host_matches_the_recording(case, policy):
    mc.check_recorded_case(case, policy, "cpu")


def test_recording_keeps_the_recorders_condition():
    """Four cases of 8 / 32 / 16 / 8 rows; the stored smallest gap of every compare is at
    least the stored margin; N = 20 holds two rows of each of the 16 variants; the archive
    is at most 256 KiB."""
    assert mc.recorded_cases() == ["n100b8", "n20b32", "n50b16", "n5b8"]
    for case in mc.recorded_cases():
        r = mc.recorded(case)
        assert r["margin"] == 1e-3 and r["min_gap"] >= r["margin"], case
        assert r["gen_locs"].shape[0] == int(case.split("b")[1]) == len(r["variant_names"])
        assert len(set(r["variant_names"])) >= 6, case
    names = mc.recorded("n20b32")["variant_names"]
    assert set(names) == {v.upper() for v in MTVRPGenerator.available_variants()}
    assert all(names.count(v) == 2 for v in set(names)) and len(set(names)) == 16
    assert os.path.getsize(os.path.join(mc.GOLDEN, "ref_mtvrp.npz")) <= 256 * 1024


@pytest.mark.parametrize("preset", mc.GEN_PRESETS)
def test_generator_reproduces_the_reference_draws(preset):
    mc.check_generator(preset)


def test_generator_surface():
    assert [get_vehicle_capacity(n) for n in (10, 20, 50, 100, 2000)] == [30, 30, 40, 50, 260]
    assert list(VARIANT_GENERATION_PRESETS)[:3] == ["all", "single_feat", "single_feat_otw"]
    assert len(MTVRPGenerator.available_variants()) == 16
    assert VARIANT_GENERATION_PRESETS["single_feat_otw"]["OTW"] == 0.5
    with pytest.raises(AssertionError, match="Cannot use subsample"):
        MTVRPGenerator(num_loc=5)
    with pytest.raises(AssertionError, match="not found"):
        MTVRPGenerator(num_loc=5, variant_preset="nope")
    gen = MTVRPGenerator(num_loc=5, variant_preset="vrpb")
    assert gen.use_combinations is False and gen.capacity == 30
    torch.manual_seed(0)
    td = MTVRPGenerator(num_loc=12, variant_preset="ovrptw")([6])
    assert MTVRPEnv.get_variant_names(td) == ["OVRPTW"] * 6


@pytest.mark.parametrize("n,b", mc.SHAPES)
def test_host_matches_the_restatement(n, b):
    mc.check_shape(n, b, "cpu")


@pytest.mark.parametrize("n", mc.SWITCH_SIZES)
def test_both_sides_of_every_launch_switch(n):
    """N + 1 below and at 16, 32, 64 (lanes per row) and 128, 256, 512 (columns per lane)."""
    mc.check_shape(n, 3, "cpu")


@pytest.mark.parametrize("n,b", mc.DIRECTED_SHAPES)
def test_every_register_slot_is_the_action(n, b):
    """The directed rollout: every register slot a row's lanes hold is the action's at
    least once and column N is visited -- asserted from the restatement before the product
    is compared -- through single steps and co_mtvrp_steps in both action layouts."""
    mc.check_directed_inputs(n, b)
    mc.check_shape(n, b, "cpu", directed=True)


def test_restatement_batches_mix_the_flags():
    mc.check_mixed_flags()


def test_hand_made_rows():
    mc.check_hand_made("cpu")


def test_depot_to_depot_feasible():
    mc.check_depot_to_depot("cpu")


def test_kernel_edges():
    mc.check_edges("cpu")


def test_check_bits_over_300_rows():
    mc.check_check_bits("cpu")


@pytest.mark.parametrize("which", ["host", "device"])
def test_invalid_arguments(which):
    mc.check_invalid_arguments(nat.load_host() if which == "host" else nat.load())


def test_registry_and_bindings():
    assert MULTITASK_ENV_REGISTRY == {"mtvrp": MTVRPEnv}
    assert set(ENV_REGISTRY) == {"tsp", "cvrp", "slap"}
    assert IMPROVEMENT_ENV_REGISTRY == {"tsp_kopt": TSPkoptEnv}
    assert ROUTING_VARIANT_ENV_REGISTRY == {"cvrptw": CVRPTWEnv}
    assert ra.MTVRPEnv is MTVRPEnv and ra.MTVRPGenerator is MTVRPGenerator
    assert ra.MULTITASK_ENV_REGISTRY is MULTITASK_ENV_REGISTRY
    with open(os.path.join(ROOT, "include", "co_env.h")) as f:
        header = f.read()
    for s in SYMBOLS:
        assert s in nat._SIGS and s in nat.HOST_SYMBOLS and f"int {s}(" in header, s
    for name in ("LIMIT_NEGATIVE", "TW_NEGATIVE", "SERVICE_NEGATIVE", "TW_INFEASIBLE",
                 "DEPOT_RETURN", "ROUTE_LIMIT", "DEADLINE", "OVER_LINEHAUL", "OVER_BACKHAUL"):
        assert f"#define CO_ST_MT_{name} {getattr(nat, 'ST_MT_' + name)} " in header, name
    assert f"#define CO_MTVRP_MAX_N {nat.MTVRP_MAX_N}\n" in header
    with pytest.raises(ValueError):
        get_env("evrptw")


def test_env_surface():
    n, b = 9, 6
    env = get_env("mtvrp", generator_params=dict(num_loc=n, variant_preset="all"), device="cpu",
                  seed=11)
    assert isinstance(env, MTVRPEnv) and env.name == "mtvrp" and env.check_solution is False
    td = env.reset(batch_size=[b])
    assert td["current_node"].shape == (b,) and td["current_node"].dtype == torch.int64
    for key in ("current_time", "current_route_length", "used_capacity_linehaul",
                "used_capacity_backhaul"):
        assert td[key].shape == (b, 1) and td[key].dtype == torch.float32, key
    assert td["visited"].dtype == torch.bool and td["action_mask"].shape == (b, n + 1)
    assert td["done"].shape == (b, 1) and "capacity_original" in td
    before = {k: td[k] for k in ("visited", "current_time", "used_capacity_linehaul")}
    kept = {k: v.clone() for k, v in before.items()}
    td = env.step(random_policy(td))["next"]
    for k, v in before.items():  # fresh output tensors per step
        assert td[k] is not v and torch.equal(v, kept[k]), k
    assert td["reward"].dtype == torch.float32 and td["done"].shape == (b,)
    assert torch.equal(env.get_action_mask(td), td["action_mask"])
    assert env.get_num_starts(td) == n + 1  # "mtvrp" is not in the reference's depot list
    assert env.select_start_nodes(td, 4).tolist() == [1] * b + [2] * b + [3] * b + [4] * b
    assert len(env.get_variant_names(td)) == b and len(env.check_variants(td)) == 4
    assert env.decode_and_step is None and env.native_decode_and_step() is None
    with pytest.raises(NotImplementedError):
        env.improve(td, torch.zeros(b, 3, dtype=torch.int64))
    with pytest.raises(NotImplementedError):
        env.solve(td, 1.0)


def test_load_data_scales_the_demands(tmp_path):
    env = get_env("mtvrp", generator_params=dict(num_loc=6, variant_preset="all",
                                                 scale_demand=False), device="cpu", seed=2)
    td = env.generator([4])
    path = os.path.join(str(tmp_path), "inst.npz")
    MTVRPGenerator.save_data(td, path)
    plain, scaled = env.load_data(path), env.load_data(path, scale=True)
    check_equal(plain["demand_linehaul"], td["demand_linehaul"])
    check_equal(scaled["demand_backhaul"], td["demand_backhaul"] / td["capacity_original"])
    assert plain["open_route"].dtype == torch.bool


def _policy():
    return ConstructivePolicy(None, LogitsDecoder(lambda td: td["locs"][..., 0].contiguous()),
                              env_name="mtvrp")


def run_decode_loops(device, n=12, b=8):
    """rollout with the random policy and the constructive loop (greedy, sampling) finish
    with valid solutions on the two-call path, on a mixed batch."""
    env = get_env("mtvrp", generator_params=dict(num_loc=n, variant_preset="all"), device=device,
                  seed=5, check_solution=True)
    torch.manual_seed(5)
    reward, td, acts = rollout(env, env.reset(batch_size=[b]), random_policy)
    env.check_solution_validity(td, acts)
    assert reward.shape == (b,) and bool(td["done"].all())
    s = Greedy()
    td = env.reset(batch_size=[b])
    assert s.step_env_fused(td["locs"][..., 0].contiguous(), td["action_mask"], td, env) is None
    assert s._fused[0] is env and s._fused[1] is None and s._fused[2] is None
    for kind in ("greedy", "sampling"):
        td = env.reset(batch_size=[b])
        out = _policy()(td, env, phase="test", decode_type=kind, return_actions=True)
        assert out["actions"].shape[0] == b and out["reward"].shape == (b,), kind
        assert bool((out["reward"] < 0).all())


def test_decode_loops_take_the_two_call_path():
    run_decode_loops("cpu")


def test_step_many_matches_single_steps():
    n, b = 12, 5
    env = get_env("mtvrp", generator_params=dict(num_loc=n, variant_preset="all"), device="cpu",
                  seed=3)
    torch.manual_seed(3)
    inst = env.generator([b])
    _, one, acts = rollout(env, env.reset(inst.clone()), random_policy)
    for step_major in (False, True):
        td = env.reset(inst.clone())
        held = td["visited"]
        feasible, times, lengths = env.step_many(td, acts.t() if step_major else acts,
                                                 step_major=step_major)
        assert bool(feasible.all()) and times.shape == lengths.shape == acts.t().shape
        assert td["visited"] is not held and not bool(held.any())
        for key in ("current_node", "used_capacity_linehaul", "used_capacity_backhaul", "visited",
                    "current_time", "current_route_length", "action_mask", "done", "reward"):
            check_equal(td[key], one[key], key)
    with pytest.raises(RuntimeError, match="index out of range"):
        env.step_many(env.reset(inst.clone()), torch.full((b, 2), n + 1))
    with pytest.raises(ValueError):
        env.step_many(env.reset(inst.clone()), acts[:2])


def test_recording_is_what_the_reference_returns(tmp_path):
    """With a reference checkout at hand ($RL4CO_REFERENCE): re-recording in a child
    process reproduces the committed archive byte for byte."""
    env = dict(os.environ, PYTHONPATH=ROOT, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    probe = subprocess.run([sys.executable, "-c",
                            "from oracle import reference as r; print(int(r.available()))"],
                           cwd=ROOT, env=env, capture_output=True, text=True, check=True)
    if probe.stdout.strip() != "1":
        pytest.skip("no reference checkout (set RL4CO_REFERENCE)")
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "record_mtvrp.py"),
                    "--out", str(tmp_path)], cwd=ROOT, env=env, check=True, capture_output=True)
    with open(os.path.join(str(tmp_path), "ref_mtvrp.npz"), "rb") as f:
        new = f.read()
    with open(os.path.join(mc.GOLDEN, "ref_mtvrp.npz"), "rb") as f:
        assert new == f.read()
