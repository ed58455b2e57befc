"""Policy evaluation of ``rl4co/tasks/eval.py:18-416`` on the MI355X engine: the five
evaluators and ``evaluate_policy`` with the reference's names, ``name`` attributes,
constructor arguments, defaults, method keys and returned dict.

The K-candidate evaluators (augmentation, multistart, both) hand the policy's ``K*B``
action rows to ``env.best_of(td_init, actions, K)``: on TSP one ``co_tsp_best_of`` launch
(where it measured faster than the composition, ``TSPEnv._best_of_fused``) scores every row against its un-replicated instance, takes ``max`` over the ``[K, B]``
layout and copies the winning rows -- the reference's ``batchify`` -> ``get_reward`` ->
``unbatchify`` -> ``max(dim=1)`` -> ``gather_by_index`` without the ``[K*B]`` copy of the
instances; other envs score through the lazy multistart td and select with
``co_best_of``.

Deliberate deviations:
* ``actions`` is every batch's rows, zero-padded to the longest and concatenated
  (``[dataset, T_max]``); the reference iterates over the last batch's rows
  (``eval.py:56-63``) and returns a flat tensor of that batch only.
* the policy is called with ``env=self.env`` (the reference lets it build a default env
  from its ``env_name``) and with ``calc_reward`` only where the rollout's reward is used.
* the device is that of ``next(policy.parameters())``, or the env's for a policy without
  parameters.
* ``inference_time`` is read after a device synchronise; there is no ``empty_cache()``.
* the batches run under ``torch.no_grad()``, not ``torch.inference_mode()``: the envs key
  their host-side knowledge of a state tensor on its version counter, which inference
  tensors do not have.
* ``get_automatic_batch_size`` divides by ``max(1, num_starts // 10)`` (the reference
  divides by zero for ``num_starts < 10``).
* SLAP's reward ignores ``actions`` and reads ``td["assignment"]``, so for SLAP the
  evaluators score with the rollout's own ``out["reward"]``; the reference scores the
  reset state's all ``-1`` assignment and gets 0 for everything.
"""
from __future__ import annotations

import time

import numpy as np
import torch
from torch.utils.data import DataLoader

from ..utils.ops import sample_n_random_actions
from ..utils.transforms import StateAugmentation

try:  # the reference's progress bar, when installed
    from tqdm.auto import tqdm
except ImportError:  # pragma: no cover
    class tqdm:  # noqa: N801
        def __init__(self, it, **kwargs):
            self.it = it

        def __iter__(self):
            return iter(self.it)

        @staticmethod
        def write(s):
            print(s)


def check_unused_kwargs(class_, kwargs):
    """``eval.py:13-15``."""
    if len(kwargs) > 0 and not (len(kwargs) == 1 and "progress" in kwargs):
        print(f"Warning: {class_.__class__.__name__} does not use kwargs {kwargs}")


def _rollout_scores(env) -> bool:
    """Whether the env's reward is a function of the rollout's final state, not of the
    action rows (SLAP: ``slap/env.py:131-143`` reads ``td["assignment"]``): the evaluators
    then score with the rollout's own reward."""
    return getattr(env, "name", None) == "slap"


class EvalBase:
    """``eval.py:18-85``."""

    name = "base"

    def __init__(self, env, progress=True, **kwargs):
        check_unused_kwargs(self, kwargs)
        self.env = env
        self.progress = progress

    def _device(self, policy):
        params = getattr(policy, "parameters", None)
        first = next(params(), None) if params is not None else None
        return first.device if first is not None else self.env.device

    def __call__(self, policy, dataloader, **kwargs):
        device = self._device(policy)
        start = time.time()
        with torch.no_grad():  # not inference_mode: see the module docstring
            rewards_list, actions_list = [], []
            for batch in tqdm(dataloader, disable=not self.progress, desc=f"Running {self.name}"):
                td = self.env.reset(batch.to(device))
                actions, rewards = self._inner(policy, td, **kwargs)
                rewards_list.append(rewards)
                actions_list.append(actions)
            rewards = torch.cat(rewards_list)
            # pad every batch's rows to the longest with zeros
            max_length = max(a.size(-1) for a in actions_list)
            actions = torch.cat([torch.nn.functional.pad(a, (0, max_length - a.size(-1)))
                                 for a in actions_list], 0)
            if rewards.device.type == "cuda":
                torch.cuda.synchronize(rewards.device)
        inference_time = time.time() - start
        tqdm.write(f"Mean reward for {self.name}: {rewards.mean():.4f}")
        tqdm.write(f"Time: {inference_time:.4f}s")
        return {"actions": actions.cpu(), "rewards": rewards.cpu(),
                "inference_time": inference_time, "avg_reward": rewards.cpu().mean()}

    def _inner(self, policy, td):
        raise NotImplementedError("Implement in subclass")

    def _best(self, td_init, out, num_candidates):
        """The best candidate per instance: ``(actions [B, T], rewards [B])``."""
        rewards = out["reward"] if _rollout_scores(self.env) else None
        best_reward, _, best_actions = self.env.best_of(td_init, out["actions"], num_candidates,
                                                        rewards=rewards)
        return best_actions, best_reward


class GreedyEval(EvalBase):
    """``eval.py:88-105``: greedy decoding, one trajectory."""

    name = "greedy"

    def __init__(self, env, **kwargs):
        check_unused_kwargs(self, kwargs)
        super().__init__(env, kwargs.get("progress", True))

    def _inner(self, policy, td):
        own = _rollout_scores(self.env)
        out = policy(td.clone(), env=self.env, decode_type="greedy", num_starts=0,
                     return_actions=True, calc_reward=own)
        rewards = out["reward"] if own else self.env.get_reward(td, out["actions"])
        return out["actions"], rewards


class AugmentationEval(EvalBase):
    """``eval.py:108-148``: the best of ``num_augment`` state augmentations."""

    name = "augmentation"

    def __init__(self, env, num_augment=8, force_dihedral_8=False, feats=None, **kwargs):
        check_unused_kwargs(self, kwargs)
        super().__init__(env, kwargs.get("progress", True))
        self.augmentation = StateAugmentation(
            num_augment=num_augment,
            augment_fn="dihedral8" if force_dihedral_8 else "symmetric", feats=feats)

    def _inner(self, policy, td, num_augment=None):
        if num_augment is None:
            num_augment = self.augmentation.num_augment
        td_init = td.clone()
        td = self.augmentation(td)
        out = policy(td.clone(), env=self.env, decode_type="greedy", num_starts=0,
                     return_actions=True, calc_reward=_rollout_scores(self.env))
        return self._best(td_init, out, num_augment)

    @property
    def num_augment(self):
        return self.augmentation.num_augment


class SamplingEval(EvalBase):
    """``eval.py:151-201``: the best of ``samples`` samples (the strategy's
    ``select_best``)."""

    name = "sampling"

    def __init__(self, env, samples, softmax_temp=None, select_best=True, temperature=1.0,
                 top_p=0.0, top_k=0, **kwargs):
        check_unused_kwargs(self, kwargs)
        super().__init__(env, kwargs.get("progress", True))
        self.samples = samples
        self.softmax_temp = softmax_temp
        self.temperature = temperature
        self.select_best = select_best
        self.top_p = top_p
        self.top_k = top_k

    def _inner(self, policy, td):
        out = policy(td.clone(), env=self.env, decode_type="sampling", num_starts=self.samples,
                     temperature=self.temperature, top_p=self.top_p, top_k=self.top_k,
                     multisample=True, return_actions=True, softmax_temp=self.softmax_temp,
                     select_best=self.select_best,
                     select_start_nodes_fn=lambda td, _, n: sample_n_random_actions(td, n))
        return out["actions"], out["reward"]


class GreedyMultiStartEval(EvalBase):
    """``eval.py:204-238``: the best of ``num_starts`` greedy multistarts."""

    name = "multistart_greedy"

    def __init__(self, env, num_starts=None, **kwargs):
        check_unused_kwargs(self, kwargs)
        super().__init__(env, kwargs.get("progress", True))
        assert num_starts is not None, "Must specify num_starts"
        self.num_starts = num_starts

    def _inner(self, policy, td):
        td_init = td.clone()
        out = policy(td.clone(), env=self.env, decode_type="multistart_greedy",
                     num_starts=self.num_starts, return_actions=True,
                     calc_reward=_rollout_scores(self.env))
        return self._best(td_init, out, self.num_starts)


class GreedyMultiStartAugmentEval(EvalBase):
    """``eval.py:241-305``: the best of ``num_augment`` augmentations x ``num_starts``
    greedy multistarts."""

    name = "multistart_greedy_augment"

    def __init__(self, env, num_starts=None, num_augment=8, force_dihedral_8=False, feats=None,
                 **kwargs):
        check_unused_kwargs(self, kwargs)
        super().__init__(env, kwargs.get("progress", True))
        assert num_starts is not None, "Must specify num_starts"
        self.num_starts = num_starts
        assert not (num_augment != 8 and force_dihedral_8), \
            "Cannot force dihedral 8 when num_augment != 8"
        self.augmentation = StateAugmentation(
            num_augment=num_augment,
            augment_fn="dihedral8" if force_dihedral_8 else "symmetric", feats=feats)

    def _inner(self, policy, td, num_augment=None):
        if num_augment is None:
            num_augment = self.augmentation.num_augment
        td_init = td.clone()
        td = self.augmentation(td)
        out = policy(td.clone(), env=self.env, decode_type="multistart_greedy",
                     num_starts=self.num_starts, return_actions=True,
                     calc_reward=_rollout_scores(self.env))
        return self._best(td_init, out, (num_augment, self.num_starts))

    @property
    def num_augment(self):
        return self.augmentation.num_augment


def get_automatic_batch_size(eval_fn, start_batch_size=8192, max_batch_size=4096):
    """``eval.py:308-336``; the multistart divisor is ``max(1, num_starts // 10)``."""
    batch_size = start_batch_size
    effective_ratio = 1
    if hasattr(eval_fn, "num_starts"):
        div = max(1, eval_fn.num_starts // 10)
        batch_size = batch_size // div
        effective_ratio *= div
    if hasattr(eval_fn, "num_augment"):
        batch_size = batch_size // eval_fn.num_augment
        effective_ratio *= eval_fn.num_augment
    if hasattr(eval_fn, "samples"):
        batch_size = batch_size // eval_fn.samples
        effective_ratio *= eval_fn.samples
    batch_size = min(batch_size, max_batch_size)
    batch_size = 2 ** int(np.log2(batch_size))  # the closest power of 2 below
    print(f"Effective batch size: {batch_size} (ratio: {effective_ratio})")
    return batch_size


def evaluate_policy(env, policy, dataset, method="greedy", batch_size=None, max_batch_size=4096,
                    start_batch_size=8192, auto_batch_size=True, samples=1280, softmax_temp=1.0,
                    num_augment=8, force_dihedral_8=True, **kwargs):
    """``eval.py:339-416``."""
    num_loc = getattr(env.generator, "num_loc", None)
    methods_mapping = {
        "greedy": {"func": GreedyEval, "kwargs": {}},
        "sampling": {"func": SamplingEval,
                     "kwargs": {"samples": samples, "softmax_temp": softmax_temp}},
        "multistart_greedy": {"func": GreedyMultiStartEval, "kwargs": {"num_starts": num_loc}},
        "augment_dihedral_8": {"func": AugmentationEval,
                               "kwargs": {"num_augment": num_augment,
                                          "force_dihedral_8": force_dihedral_8}},
        "augment": {"func": AugmentationEval, "kwargs": {"num_augment": num_augment}},
        "multistart_greedy_augment_dihedral_8": {
            "func": GreedyMultiStartAugmentEval,
            "kwargs": {"num_augment": num_augment, "force_dihedral_8": force_dihedral_8,
                       "num_starts": num_loc}},
        "multistart_greedy_augment": {
            "func": GreedyMultiStartAugmentEval,
            "kwargs": {"num_augment": num_augment, "num_starts": num_loc}},
    }
    assert method in methods_mapping, "Method {} not found".format(method)
    eval_settings = methods_mapping[method]
    func, kwargs_ = eval_settings["func"], eval_settings["kwargs"]
    kwargs_.update(kwargs)  # the caller's arguments override the method's defaults
    eval_fn = func(env, **kwargs_)
    if auto_batch_size:
        assert batch_size is None, "Cannot specify batch_size when auto_batch_size is True"
        batch_size = get_automatic_batch_size(eval_fn, max_batch_size=max_batch_size,
                                              start_batch_size=start_batch_size)
        print("Using automatic batch size: {}".format(batch_size))
    dataloader = DataLoader(dataset, batch_size=batch_size, shuffle=False, num_workers=0,
                            collate_fn=dataset.collate_fn)
    return eval_fn(policy, dataloader)
