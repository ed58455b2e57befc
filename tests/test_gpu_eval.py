"""rl4co_slap_amd.tasks.eval on the device: the recorded evaluator results with the real
augmentation kernels in the loop, co_tsp_best_of against the composition, and
``evaluate_policy`` end to end for every method key."""
import pytest
import torch

import eval_cases as ec

pytestmark = pytest.mark.gpu

IDS = [f"{c[0]}-{c[1]}" for c in ec.INNER_CASES]


@pytest.mark.parametrize("cls,case,kwargs", ec.INNER_CASES, ids=IDS)
def test_evaluators_reproduce_the_recording(dev, cls, case, kwargs):
    ec.check_inner(cls, case, kwargs, dev)
    if case.startswith("tsp"):
        ec.check_inner(cls, case, kwargs, dev, fused=True)
        ec.check_fused_equals_composition(cls, case, kwargs, dev)


def test_whole_call_reproduces_the_recording(dev):
    ec.check_whole_call(dev)


@pytest.mark.parametrize("name", ["tsp", "cvrp"])
def test_evaluate_policy_end_to_end(dev, name):
    res = ec.end_to_end(name, dev, ec.METHODS)
    # every augmented variant contains the un-augmented instance (the first augmentation of
    # the symmetric transform is the identity; dihedral's first is (x, y))
    assert (res["multistart_greedy_augment"]["rewards"]
            >= res["multistart_greedy"]["rewards"] - 1e-5).all()
    assert (res["augment_dihedral_8"]["rewards"] >= res["greedy"]["rewards"] - 1e-5).all()


def test_one_identity_augmentation_is_greedy(dev):
    from rl4co_slap_amd.tasks import eval as ev

    env = ec.make_env("tsp_n7", dev)
    torch.manual_seed(7)
    ds = ec.TensorDictDataset(env.generator([5]))
    kw = dict(auto_batch_size=False, batch_size=2, progress=False)
    greedy = ev.evaluate_policy(env, ec.real_policy("tsp"), ds, method="greedy", **kw)
    one = ev.evaluate_policy(env, ec.real_policy("tsp"), ds, method="augment", num_augment=1, **kw)
    assert torch.equal(one["actions"], greedy["actions"])
    assert ec.close(one["rewards"].numpy(), greedy["rewards"].numpy())


def test_sampling_eval_returns_the_best_sample(dev):
    from rl4co_slap_amd.envs import TSPEnv

    env = TSPEnv(generator_params=dict(num_loc=7), device=dev)
    torch.manual_seed(2)
    td = env.reset(batch_size=[6])
    ec.check_sampling_beats_its_mean(env, ec.real_policy("tsp"), td)


def test_slap_scores_with_the_rollouts_reward(dev):
    ec.check_slap(dev)
