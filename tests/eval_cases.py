"""What tests/test_eval.py (host build) and tests/test_gpu_eval.py (device) share: the
scripted policy that drove the reference's evaluators when tests/golden/eval/ref_eval.npz was
recorded (tests/golden/record_eval.py), the recording's loader and the checks (not a test
module).  Rewards are compared with the project's 1e-5 relative convention; actions and the
winning index exactly (the recorder made sure that no winner is within 1e-4 of the second
best)."""
import os

import numpy as np
import torch

from rl4co_slap_amd import TensorDict
from rl4co_slap_amd.data import TensorDictDataset
from rl4co_slap_amd.envs import CVRPEnv, SLAPEnv, TSPEnv
from rl4co_slap_amd.envs.base import RL4COEnvBase
from rl4co_slap_amd.rollout.constructive import ConstructivePolicy, LogitsDecoder
from rl4co_slap_amd.tasks import eval as ev
from rl4co_slap_amd.utils.transforms import StateAugmentation

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval",
                      "ref_eval.npz")
METHODS = ["greedy", "sampling", "multistart_greedy", "augment_dihedral_8", "augment",
           "multistart_greedy_augment_dihedral_8", "multistart_greedy_augment"]
# (evaluator class, recorded case, constructor arguments)
INNER_CASES = [
    ("GreedyEval", "tsp_b3n7", {}),
    ("AugmentationEval", "tsp_b3n7", dict(num_augment=8)),
    ("GreedyMultiStartEval", "tsp_b3n7", dict(num_starts=7)),
    ("GreedyMultiStartAugmentEval", "tsp_b3n7", dict(num_starts=7, num_augment=8)),
    ("GreedyMultiStartAugmentEval", "tsp_b4n20", dict(num_starts=20, num_augment=8)),
    ("AugmentationEval", "cvrp_b3n10", dict(num_augment=8)),
    ("GreedyMultiStartAugmentEval", "cvrp_b3n10", dict(num_starts=10, num_augment=8)),
]

_cache = {}


def recording(fn, case):
    """{name: array} of one recorded call (loaded once, never modified)."""
    if "all" not in _cache:
        with np.load(GOLDEN, allow_pickle=False) as z:
            _cache["all"] = {k: z[k] for k in z.files}
    pre = f"{fn}/{case}/"
    return {k[len(pre):]: v for k, v in _cache["all"].items() if k.startswith(pre)}


def cases_of(fn):
    recording("", "")
    return sorted({k.split("/")[1] for k in _cache["all"] if k.startswith(fn + "/")})


class ScriptedPolicy:
    """Returns the preset ``[K*B, T]`` action rows of the batches in order (and a reward
    nobody may use: NaN), whatever it is asked."""

    def __init__(self, rows, device):
        self.rows = [torch.as_tensor(np.asarray(r, dtype=np.int64)).to(device) for r in rows]
        self.calls = 0

    def __call__(self, td, **kwargs):
        rows = self.rows[self.calls]
        self.calls += 1
        return {"actions": rows, "reward": torch.full((rows.shape[0],), float("nan"),
                                                      device=rows.device)}


def close(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return bool((np.abs(got - want) <= 1e-5 * np.maximum(np.abs(want), 1.0)).all())


def make_env(case, device, fused=None):
    name, n = ("tsp", int(case.split("n")[-1])) if case.startswith("tsp") else ("cvrp", 10)
    env = (TSPEnv if name == "tsp" else CVRPEnv)(generator_params=dict(num_loc=n), device=device)
    if fused is not None:  # TSP: force co_tsp_best_of (True) or the composition (False)
        env._BEST_OF_FORCE = bool(fused)
    return env


def identity_augmentation(num_augment):
    """The host build has no augmentation kernel; the scripted policy does not look at the
    augmented td, so the CPU tests replicate the instances unchanged."""
    return StateAugmentation(num_augment=num_augment, augment_fn=lambda xy, n: xy.clone())


def run_inner(cls, case, kwargs, device, fused=None):
    r = recording(cls + "._inner", case)
    env = make_env(case, device, fused)
    keys = ("locs",) if case.startswith("tsp") else ("locs", "depot", "demand")
    b = r["locs"].shape[0]
    td = env.reset(TensorDict({k: torch.as_tensor(r[k].copy()) for k in keys}, [b]).to(device))
    evaluator = getattr(ev, cls)(env, progress=False, **kwargs)
    if torch.device(device).type == "cpu" and hasattr(evaluator, "augmentation"):
        evaluator.augmentation = identity_augmentation(kwargs["num_augment"])
    policy = ScriptedPolicy([r["rows"]], device)
    actions, rewards = evaluator._inner(policy, td)
    assert policy.calls == 1
    return r, actions.cpu(), rewards.cpu()


def check_inner(cls, case, kwargs, device, fused=None):
    r, actions, rewards = run_inner(cls, case, kwargs, device, fused)
    assert (r["margins"] > 1e-4).all()  # the recorder's condition on its inputs
    assert actions.dtype == torch.int64
    assert np.array_equal(actions.numpy(), r["out_actions"].astype(np.int64))
    assert close(rewards.numpy(), r["out_rewards"])


def check_fused_equals_composition(cls, case, kwargs, device):
    _, a_f, r_f = run_inner(cls, case, kwargs, device, fused=True)
    _, a_c, r_c = run_inner(cls, case, kwargs, device, fused=False)
    import best_of_ref as ref

    assert torch.equal(a_f, a_c)
    assert ref.ulp_distance(r_f.numpy(), r_c.numpy()).max() <= 1


def check_whole_call(device):
    r = recording("EvalBase.__call__", "tsp_d5n7_bs2")
    env = make_env("tsp_n7", device)
    ds = TensorDictDataset(TensorDict({"locs": torch.as_tensor(r["locs"].copy())}, [5]))
    loader = torch.utils.data.DataLoader(ds, batch_size=int(r["batch_size"]), shuffle=False,
                                         collate_fn=ds.collate_fn)
    rows = r["rows"].astype(np.int64)
    policy = ScriptedPolicy([rows[:14], rows[14:28], rows[28:]], device)
    policy.parameters = lambda: iter([torch.zeros(1, device=device)])
    out = ev.GreedyMultiStartEval(env, num_starts=7, progress=False)(policy, loader)
    assert policy.calls == 3
    assert sorted(out) == ["actions", "avg_reward", "inference_time", "rewards"]
    assert close(out["rewards"].numpy(), r["out_rewards"])
    assert close(out["avg_reward"].numpy(), r["out_avg_reward"])
    assert out["actions"].shape == (5, 7) and out["actions"].device.type == "cpu"
    assert out["inference_time"] > 0
    # every returned row is its instance's winner: it re-scores to the returned reward
    cpu_env = make_env("tsp_n7", "cpu")
    td = cpu_env.reset(TensorDict({"locs": torch.as_tensor(r["locs"].copy())}, [5]))
    assert close(cpu_env.get_reward(td, out["actions"]).numpy(), out["rewards"].numpy())


def check_batch_sizes():
    import types

    for case in cases_of("get_automatic_batch_size"):
        r = recording("get_automatic_batch_size", case)
        fn = types.SimpleNamespace(**{k: int(r[k]) for k in ("num_starts", "num_augment",
                                                             "samples") if int(r[k]) >= 0})
        assert ev.get_automatic_batch_size(fn) == int(r["out"]), case
    # below 10 starts the reference divides by zero; here the divisor is 1
    assert ev.get_automatic_batch_size(types.SimpleNamespace(num_starts=7)) == 4096
    assert ev.get_automatic_batch_size(types.SimpleNamespace(num_starts=7, num_augment=8)) == 1024


def nearest_logits(td):
    """The negative distance to the current node."""
    locs, cur = td["locs"], td["current_node"].reshape(-1)
    here = locs[torch.arange(locs.shape[0], device=locs.device), cur]
    return -(locs - here[:, None]).norm(dim=-1)


def real_policy(name, logits_fn=nearest_logits):
    return ConstructivePolicy(None, LogitsDecoder(logits_fn), env_name=name)


def end_to_end(name, device, methods):
    """evaluate_policy for the given method keys on 5 instances at batch size 2: the
    returned dict, [5, T_max] actions that re-score to their rewards, and multistart no
    worse than greedy.  Returns {method: result}."""
    n = 7 if name == "tsp" else 10
    env = (TSPEnv if name == "tsp" else CVRPEnv)(generator_params=dict(num_loc=n), device=device)
    torch.manual_seed(7)
    data = env.generator([5])
    ds = TensorDictDataset(data)
    policy = real_policy(name)
    cpu_env = (TSPEnv if name == "tsp" else CVRPEnv)(generator_params=dict(num_loc=n),
                                                     device="cpu")
    td_all = cpu_env.reset(TensorDict({k: v.clone().cpu() for k, v in data.items()}, [5]))
    res = {}
    for m in methods:
        torch.manual_seed(11)
        out = ev.evaluate_policy(env, policy, ds, method=m, auto_batch_size=False, batch_size=2,
                                 samples=4, progress=False)
        assert sorted(out) == ["actions", "avg_reward", "inference_time", "rewards"], m
        assert out["rewards"].shape == (5,) and out["actions"].dim() == 2, m
        assert out["actions"].shape[0] == 5 and out["actions"].dtype == torch.int64, m
        assert close(cpu_env.get_reward(td_all, out["actions"]).numpy(), out["rewards"].numpy()), m
        assert close(out["avg_reward"].numpy(), out["rewards"].mean().numpy()), m
        res[m] = out
    if "multistart_greedy" in res and "greedy" in res:
        assert (res["multistart_greedy"]["rewards"] >= res["greedy"]["rewards"] - 1e-6).all()
    return res


def check_sampling_beats_its_mean(env, policy, td):
    """SamplingEval(samples=4): per instance the returned reward is the maximum of the four
    samples' rewards (drawn again with the same torch seed), hence >= their mean."""
    samples = 4
    torch.manual_seed(5)
    actions, rewards = ev.SamplingEval(env, samples=samples, progress=False)._inner(policy, td)
    torch.manual_seed(5)
    every = policy(td.clone(), env=env, decode_type="sampling", num_starts=samples,
                   multisample=True, return_actions=True, select_best=False)
    per = every["reward"].view(samples, -1)
    assert rewards.shape == (td.batch_size[0],) and actions.shape[0] == td.batch_size[0]
    assert close(rewards.cpu().numpy(), per.max(0).values.cpu().numpy())
    assert (rewards >= per.mean(0) - 1e-6).all()


def check_slap(device):
    env = SLAPEnv(device=device)
    np.random.seed(3)
    torch.manual_seed(3)
    policy = real_policy("slap", lambda td: -td["depot_loc_dist"])
    data = env.generator([3])
    td = env.reset(TensorDict({k: v.clone() for k, v in data.items()}, [3]).to(device))
    # GreedyEval returns the rollout's own reward (the reference scores the reset state)
    actions, rewards = ev.GreedyEval(env, progress=False)._inner(policy, td)
    out = policy(td.clone(), env=env, decode_type="greedy", return_actions=True)
    assert torch.equal(actions, out["actions"]) and torch.equal(rewards, out["reward"])
    assert (rewards < 0).all()
    check_sampling_beats_its_mean(env, policy, td)
    # the K-candidate path scores with the rollout's rewards (rewards=): multistart on SLAP
    k = 3
    got_a, got_r = ev.GreedyMultiStartEval(env, num_starts=k, progress=False)._inner(policy, td)
    full = policy(td.clone(), env=env, decode_type="multistart_greedy", num_starts=k,
                  return_actions=True)
    want_r, want_i = full["reward"].view(k, -1).max(0)
    assert torch.equal(got_r, want_r)
    rows = full["actions"].view(k, 3, -1)
    assert torch.equal(got_a, rows[want_i, torch.arange(3, device=rows.device)])


def base_best_of(env, td, actions, k, rewards=None):
    return RL4COEnvBase.best_of(env, td, actions, k, rewards)
