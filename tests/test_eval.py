"""rl4co_slap_amd.tasks.eval on the host build (CPU TensorDicts): the evaluators driven by
the recorder's scripted policy reproduce the reference's own evaluators
(tests/golden/eval/ref_eval.npz), the TSP fused path equals the base-class composition, and
``evaluate_policy`` runs end to end with a real constructive policy.  The augmentation
kernels have no host build: the scripted cases replicate the instances unchanged (the
policy does not look at them) and the end-to-end augment keys say what is missing;
tests/test_gpu_eval.py runs them on the device."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import eval_cases as ec
import rl4co_slap_amd as ra
from rl4co_slap_amd import TensorDict
from rl4co_slap_amd.envs import TSPEnv
from rl4co_slap_amd.tasks import eval as ev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [f"{c[0]}-{c[1]}" for c in ec.INNER_CASES]


def test_public_surface():
    for name in ("EvalBase", "GreedyEval", "AugmentationEval", "SamplingEval",
                 "GreedyMultiStartEval", "GreedyMultiStartAugmentEval",
                 "get_automatic_batch_size", "evaluate_policy"):
        assert getattr(ra, name) is getattr(ev, name) and name in ra.__all__
    names = {ev.EvalBase: "base", ev.GreedyEval: "greedy", ev.AugmentationEval: "augmentation",
             ev.SamplingEval: "sampling", ev.GreedyMultiStartEval: "multistart_greedy",
             ev.GreedyMultiStartAugmentEval: "multistart_greedy_augment"}
    for cls, name in names.items():
        assert cls.name == name
    env = TSPEnv(generator_params=dict(num_loc=7), device="cpu")
    with pytest.raises(AssertionError, match="Must specify num_starts"):
        ev.GreedyMultiStartEval(env)
    with pytest.raises(AssertionError, match="Cannot force dihedral 8"):
        ev.GreedyMultiStartAugmentEval(env, num_starts=7, num_augment=4, force_dihedral_8=True)
    with pytest.raises(AssertionError, match="not found"):
        ev.evaluate_policy(env, None, None, method="nope")
    with pytest.raises(AssertionError, match="Cannot specify batch_size"):
        ev.evaluate_policy(env, None, None, method="greedy", batch_size=4)
    s = ev.SamplingEval(env, samples=16)
    assert (s.samples, s.softmax_temp, s.select_best, s.temperature, s.top_p, s.top_k) == \
        (16, None, True, 1.0, 0.0, 0)
    assert ev.AugmentationEval(env).num_augment == 8


@pytest.mark.parametrize("cls,case,kwargs", ec.INNER_CASES, ids=IDS)
def test_evaluators_reproduce_the_recording(cls, case, kwargs):
    ec.check_inner(cls, case, kwargs, "cpu")
    if case.startswith("tsp"):  # both dispatch sides of TSPEnv.best_of
        ec.check_inner(cls, case, kwargs, "cpu", fused=True)
        ec.check_inner(cls, case, kwargs, "cpu", fused=False)


@pytest.mark.parametrize("cls,case,kwargs", [c for c in ec.INNER_CASES if c[1].startswith("tsp")
                                             and c[0] != "GreedyEval"],
                         ids=[i for i in IDS if "-tsp" in i and not i.startswith("GreedyEval")])
def test_fused_path_equals_the_composition(cls, case, kwargs):
    ec.check_fused_equals_composition(cls, case, kwargs, "cpu")


def test_whole_call_reproduces_the_recording():
    ec.check_whole_call("cpu")


def test_automatic_batch_size():
    ec.check_batch_sizes()


@pytest.mark.parametrize("name", ["tsp", "cvrp"])
def test_evaluate_policy_end_to_end(name):
    ec.end_to_end(name, "cpu", ["greedy", "sampling", "multistart_greedy"])
    env = ec.make_env("tsp_n7" if name == "tsp" else "cvrp", "cpu")
    ds = ec.TensorDictDataset(env.generator([5]))
    for m in ec.METHODS:
        if "augment" in m:  # no augmentation kernel in the host build: said, not computed
            with pytest.raises(NotImplementedError, match="no host"):
                ev.evaluate_policy(env, ec.real_policy(name), ds, method=m,
                                   auto_batch_size=False, batch_size=2, progress=False)


def test_sampling_eval_returns_the_best_sample():
    env = TSPEnv(generator_params=dict(num_loc=7), device="cpu")
    torch.manual_seed(2)
    td = env.reset(batch_size=[6])
    ec.check_sampling_beats_its_mean(env, ec.real_policy("tsp"), td)


def test_slap_scores_with_the_rollouts_reward():
    ec.check_slap("cpu")


def test_no_replica_of_the_instances_on_the_tsp_path():
    """TSPEnv.best_of reads the un-replicated locs: batchify is never called."""
    from rl4co_slap_amd.utils import ops

    r = ec.recording("GreedyMultiStartAugmentEval._inner", "tsp_b4n20")
    env = ec.make_env("tsp_b4n20", "cpu", fused=True)
    td = env.reset(TensorDict({"locs": torch.as_tensor(r["locs"].copy())}, [4]))
    calls = []
    orig = ops.batchify
    ops.batchify = lambda *a, **k: calls.append(a) or orig(*a, **k)
    try:
        best_r, best_i, best_a = env.best_of(
            td, torch.as_tensor(r["rows"].astype(np.int64)), (8, 20))
    finally:
        ops.batchify = orig
    assert not calls
    assert np.array_equal(best_a.numpy(), r["out_actions"].astype(np.int64))


def test_recording_is_fresh(tmp_path):
    """With a reference checkout at hand: the recorder, in a process of its own, reproduces
    the committed archive byte for byte."""
    env = dict(os.environ, PYTHONPATH=ROOT, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    probe = subprocess.run([sys.executable, "-c",
                            "from oracle import reference as r; print(int(r.available()))"],
                           cwd=ROOT, env=env, capture_output=True, text=True, check=True)
    if probe.stdout.strip() != "1":
        pytest.skip("no reference checkout (set RL4CO_REFERENCE)")
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "record_eval.py"),
                    "--out", str(tmp_path)], cwd=ROOT, env=env, check=True, capture_output=True)
    assert os.path.getsize(ec.GOLDEN) < 100 * 1024
    import ref_recordings as rr

    with np.load(os.path.join(str(tmp_path), "ref_eval.npz")) as new, np.load(ec.GOLDEN) as old:
        assert sorted(new.files) == sorted(old.files)
        same = rr.same_machine()  # else ATen's float kernels may round differently here
        for key in old.files:
            a, b = new[key], old[key]
            assert a.dtype == b.dtype and a.shape == b.shape, key
            if same or a.dtype.kind != "f":
                assert a.tobytes() == b.tobytes(), key
            else:
                assert np.allclose(a, b, rtol=1e-5, atol=1e-6), key
    if same:
        with open(os.path.join(str(tmp_path), "ref_eval.npz"), "rb") as f, \
                open(ec.GOLDEN, "rb") as g:
            assert f.read() == g.read()
