"""Pickup-and-delivery problem: env + generator on the gfx950 kernels
(``rl4co/envs/routing/pdp/``).  ``include/co_env.h`` (PDP) states the arithmetic."""
from __future__ import annotations

import warnings
from typing import Callable, Union

import torch
from torch.distributions import Uniform

from .. import _native as nat
from ..td import RepeatedRows, TensorDict, set_many
from .base import RL4COEnvBase
from .common import Generator, device_uniform, get_sampler


class PDPGenerator(Generator):
    """``pdp/generator.py:14-88``: a depot, ``num_loc / 2`` pickups and as many deliveries,
    uniform on ``[min_loc, max_loc]^2``.  Without a depot distribution one draw of
    ``[*B, num_loc + 1, 2]`` is split into the depot (row 0) and the locations, as the
    reference does -- on the CPU the reference's draw on the same global stream.  An odd
    ``num_loc`` is raised by one with a warning.  ``_get_initial_solutions`` belongs to the
    ruin-repair env and is not built."""

    def __init__(self, num_loc: int = 20, min_loc: float = 0.0, max_loc: float = 1.0,
                 init_sol_type: str = "random",
                 loc_distribution: Union[int, float, str, type, Callable] = Uniform,
                 depot_distribution: Union[int, float, str, type, Callable] = None, **kwargs):
        self.num_loc, self.min_loc, self.max_loc = num_loc, min_loc, max_loc
        self.init_sol_type = init_sol_type
        self.device = kwargs.get("device")
        if num_loc % 2 != 0:
            warnings.warn("Number of locations must be even. Adding 1 to the number of "
                          "locations.", UserWarning, stacklevel=2)
            self.num_loc += 1
        self.loc_sampler = kwargs.get("loc_sampler") or get_sampler(
            "loc", loc_distribution, min_loc, max_loc, **kwargs)
        self.depot_sampler = kwargs.get("depot_sampler") or (
            get_sampler("depot", depot_distribution, min_loc, max_loc, **kwargs)
            if depot_distribution is not None else None)

    def _sample(self, sampler, shape):
        x = device_uniform(sampler, shape, self.device) if self.device else None
        return sampler.sample(shape) if x is None else x

    def _generate(self, batch_size) -> TensorDict:
        if self.depot_sampler is not None:
            depot = self._sample(self.depot_sampler, (*batch_size, 2))
            locs = self._sample(self.loc_sampler, (*batch_size, self.num_loc, 2))
        else:  # the depot is the first of num_loc + 1 drawn locations
            locs = self._sample(self.loc_sampler, (*batch_size, self.num_loc + 1, 2))
            depot, locs = locs[..., 0, :], locs[..., 1:, :]
        return TensorDict({"locs": locs, "depot": depot}, batch_size=batch_size)


class PDPEnv(RL4COEnvBase):
    """``pdp/env.py:20-234``: every pickup (nodes ``1..N/2``) before its delivery (the node
    ``N/2`` further), each node once, from and back to the depot.  One launch per reset /
    step; ``step_many`` runs preset steps in one launch, ``decode_and_step`` fuses the decode
    step with the env step (``co_pdp_decode_step``)."""

    name = "pdp"
    _MESSAGES = [(nat.ST_PDP_NOT_ALL_NODES, AssertionError, "Not visiting all nodes"),
                 (nat.ST_PDP_PRECEDENCE, AssertionError, "Deliverying without pick-up")]
    _RANGE = (nat.ST_INDEX_RANGE, RuntimeError, "index out of range in gather (actions)")

    def __init__(self, generator: PDPGenerator = None, generator_params: dict = {}, **kwargs):
        super().__init__(**kwargs)
        self.generator = generator if generator is not None else PDPGenerator(**generator_params)

    def native_decode_and_step(self):
        """No step glue for this env (``csrc/pycall/co_torchstep.cpp`` is not extended):
        the decode loop calls ``decode_and_step``."""
        return None

    def _reset(self, td=None, batch_size=None) -> TensorDict:
        """``pdp/env.py:108-151`` in one ``co_pdp_reset`` launch, ``done`` / ``terminated``
        included."""
        depot, locs = td["depot"], td["locs"]
        nat.require_device(depot, locs)
        depot, locs = depot.float().contiguous(), locs.float().contiguous()
        b, n = locs.shape[0], locs.shape[-2]
        dev = locs.device
        locs_out = torch.empty((b, n + 1, 2), dtype=torch.float32, device=dev)
        rows = torch.empty((3, b, n + 1), dtype=torch.bool, device=dev)
        words = torch.empty((2, b, 1), dtype=torch.int64, device=dev)
        flags = torch.empty((2, b, 1), dtype=torch.bool, device=dev)
        nat.call("co_pdp_reset", b, n, nat.ptr(depot), nat.ptr(locs), nat.ptr(locs_out),
                 nat.ptr(rows[0]), nat.ptr(rows[1]), nat.ptr(rows[2]), nat.ptr(words[0]),
                 nat.ptr(words[1]), nat.ptr(flags[0]), nat.ptr(flags[1]), nat.stream_of(locs))
        available, i = rows[0], words[1]
        self._remember_lb(available, n + 1)  # N + 1 ones; a step clears at most one
        self._remember_i(i, 0)
        return TensorDict({"locs": locs_out, "current_node": words[0], "to_deliver": rows[1],
                           "available": available, "i": i, "action_mask": rows[2],
                           "done": flags[0], "terminated": flags[1]}, batch_size=batch_size)

    @staticmethod
    def _state(td):
        """The td's state tensors as the step entries take them."""
        available, to_deliver, i = td["available"], td["to_deliver"], td["i"]
        nat.require_device(available, to_deliver, i)
        if available.shape != to_deliver.shape or available.dim() != 2:
            raise ValueError("td['available'] and td['to_deliver'] must both be [B, N+1], got "
                             f"{tuple(available.shape)} and {tuple(to_deliver.shape)}")
        return available.contiguous(), to_deliver.contiguous(), i.contiguous()

    def _step(self, td: TensorDict) -> TensorDict:
        """``pdp/env.py:67-106`` in one ``co_pdp_step`` launch; every output is a fresh
        tensor (the reference's scatter is out of place).  An action outside ``0..N``, on
        which torch's scatter raises at once, edits nothing here and raises with the
        rollout's ``get_reward`` (or in ``step_many``), as in the other envs."""
        action = td["action"]
        available, to_deliver, i = self._state(td)
        nat.require_device(action, available)
        if action.dtype != torch.int64:
            action = action.long()
        action = action.contiguous()
        b, nc = available.shape
        dev = available.device
        s = nat.stream_of(available)
        av_out = self._out((b, nc), torch.bool, dev, s)
        td_out = self._out((b, nc), torch.bool, dev, s)
        mask = self._out((b, nc), torch.bool, dev, s)
        i_out = self._out((b, 1), torch.int64, dev, s)
        cur = self._out((b, 1), torch.int64, dev, s)
        done = self._out((b,), torch.bool, dev, s)
        reward = self._out((b,), torch.bool, dev, s)
        nat.call("co_pdp_step", b, nc - 1, nat.ptr(action), nat.ptr(available),
                 nat.ptr(to_deliver), nat.ptr(av_out), nat.ptr(td_out), nat.ptr(mask), nat.ptr(i),
                 nat.ptr(i_out), nat.ptr(cur), nat.ptr(done), nat.ptr(reward), None, s)
        return self._after_step(td, td["available"], av_out, td_out, mask, i_out, cur, done,
                                reward)

    def _after_step(self, td, av_in, av_out, td_out, mask, i_out, cur, done, reward, extra=None):
        lb = self._known_lb(av_in)
        if lb is not None:  # a step makes at most one more node unavailable
            self._remember_lb(av_out, lb - 1)
        out = {"current_node": cur, "available": av_out, "to_deliver": td_out, "i": i_out,
               "action_mask": mask, "reward": reward, "done": done}
        if extra:
            out.update(extra)
        set_many(td, out)
        return td

    def step_many(self, td, actions, step_major: bool = False):
        """T preset steps in one ``co_pdp_steps`` launch: ``actions`` is ``[B, T]`` (a
        rollout's layout) or, with ``step_major``, ``[T, B]``; any strides.  Leaves ``td`` as
        the T ``step`` calls would, bit for bit, in fresh tensors, and returns ``feasible
        [T, B]``: whether ``action_mask[b, a_t]`` held before step t.  An action outside
        ``0..N`` raises."""
        available, to_deliver, i = self._state(td)
        mask_in = td["action_mask"]
        nat.require_device(actions, mask_in, available)
        if actions.dtype != torch.int64:
            actions = actions.long()
        b, nc = available.shape
        if actions.dim() != 2 or actions.shape[0 if not step_major else 1] != b:
            raise ValueError(f"actions must be [{b}, T] (or [T, {b}] with step_major), got "
                             f"{tuple(actions.shape)}")
        if not step_major:
            actions = actions.t()
        t = actions.shape[0]
        if t == 0:
            raise ValueError("step_many needs at least one step")
        dev = available.device
        lb = self._known_lb(td["available"])
        mask_in = mask_in.contiguous()
        available, to_deliver, i = available.clone(), to_deliver.clone(), i.long().clone()
        cur = torch.empty((b, 1), dtype=torch.int64, device=dev)
        mask = torch.empty((b, nc), dtype=torch.bool, device=dev)
        done = torch.empty(b, dtype=torch.bool, device=dev)
        reward = torch.empty(b, dtype=torch.bool, device=dev)
        feasible = torch.empty((t, b), dtype=torch.bool, device=dev)
        status = self.status_word(dev)
        nat.call("co_pdp_steps", b, nc - 1, t, nat.ptr(actions), actions.stride(0),
                 actions.stride(1), nat.ptr(mask_in), nat.ptr(available), nat.ptr(to_deliver),
                 nat.ptr(mask), nat.ptr(i), nat.ptr(cur), nat.ptr(done), nat.ptr(reward),
                 nat.ptr(feasible), nat.ptr(status), nat.stream_of(available))
        self.raise_for_status(status, [(nat.ST_INDEX_RANGE, RuntimeError,
                                        "index out of range in step_many (actions)")])
        if lb is not None:
            self._remember_lb(available, lb - t)
        set_many(td, {"action": actions[-1], "current_node": cur, "available": available,
                      "to_deliver": to_deliver, "i": i, "action_mask": mask, "reward": reward,
                      "done": done})
        return feasible

    def decode_and_step(self, td, logits, mode, temperature, tanh_clipping, action_in, seed,
                        offset, status, key="action"):
        """``DecodingStrategy.step`` + ``_step`` (``decoding.py:327-369``,
        ``pdp/env.py:67-106``) in one ``co_pdp_decode_step`` launch: the same selection,
        log-probability, RNG use and state as the two calls.  Returns ``(action, logp)``, or
        None when it does not apply (CPU tensors, non-f32 logits, rows past the entries'
        limit)."""
        mask = td["action_mask"]
        ops = self._fused_operands(logits, action_in, mask)
        if ops is None or mask.shape[1] - 1 > nat.PDP_MAX_N or mask.shape[1] % 2 == 0:
            return None
        b, nc, ain, act, logp, sel, s = ops
        av_in = td["available"]
        available, to_deliver, i = self._state(td)
        dev = mask.device
        m = mask.contiguous()
        av_out = self._out((b, nc), torch.bool, dev, s)
        td_out = self._out((b, nc), torch.bool, dev, s)
        mask_out = self._out((b, nc), torch.bool, dev, s)
        i_out = self._out((b, 1), torch.int64, dev, s)
        cur = self._out((b, 1), torch.int64, dev, s)
        done = self._out((b,), torch.bool, dev, s)
        reward = self._out((b,), torch.bool, dev, s)
        nat.call("co_pdp_decode_step", b, nc - 1, nat.ptr(logits), logits.stride(0), nat.ptr(m),
                 float(tanh_clipping), float(temperature), mode, nat.ptr(ain), nat.ptr(act),
                 nat.ptr(logp), seed, offset, nat.ptr(available), nat.ptr(to_deliver),
                 nat.ptr(av_out), nat.ptr(td_out), nat.ptr(mask_out), nat.ptr(i), nat.ptr(i_out),
                 nat.ptr(cur), nat.ptr(done), nat.ptr(reward), None, nat.ptr(status), s)
        self._after_step(td, av_in, av_out, td_out, mask_out, i_out, cur, done, reward,
                         extra={key: sel})
        return sel, logp

    def _get_reward(self, td, actions, check: bool = False) -> torch.Tensor:
        """``pdp/env.py:189-216``: minus the closed length of ``[depot, locs[actions]]``,
        fused with the two validity tests (``co_pdp_reward``).  A multistart td's
        un-replicated ``locs`` (``RepeatedRows``) is read in place: env ``e`` uses
        coordinate row ``e % B`` (the kernel's ``locs_batch``)."""
        raw = td.get_raw("locs") if hasattr(td, "get_raw") else td["locs"]
        locs = raw.source() if isinstance(raw, RepeatedRows) else raw
        nat.require_device(locs, actions)
        locs = locs.contiguous()
        if actions.dtype != torch.int64:
            actions = actions.long()
        b, t = actions.shape
        reward = torch.empty(b, dtype=torch.float32, device=locs.device)
        status = self.status_word(locs.device)
        nat.call("co_pdp_reward", b, locs.shape[-2] - 1, t, nat.ptr(locs), locs.shape[0],
                 nat.ptr(actions), actions.stride(0), actions.stride(1), int(check),
                 nat.ptr(reward), nat.ptr(status), nat.stream_of(locs))
        self.raise_for_status(status, (self._MESSAGES if check else []) + [self._RANGE])
        return reward

    def check_solution_validity(self, td, actions) -> None:
        """``pdp/env.py:201-216``: the first failing message, in the reference's order."""
        self._get_reward(td, actions, check=True)

    def get_action_mask(self, td):
        return td["action_mask"]

    def get_num_starts(self, td):
        """``pdp/env.py:218-220``: only the pickups can be start nodes."""
        return (td["locs"].shape[-2] - 1) // 2

    def select_start_nodes(self, td, num_starts):
        """``pdp/env.py:222-230``: the pickups ``1 .. num_loc / 2``, start-major."""
        possible = (td["locs"].shape[-2] - 1) // 2
        return torch.arange(num_starts, device=td.device).repeat_interleave(td.shape[0]) \
            % possible + 1

    def min_steps_to_done(self, td) -> int:
        """done = no node available (``pdp/env.py:89``), and a step takes one node."""
        return self._known_lb(td.get_raw("available") if hasattr(td, "get_raw")
                              else td["available"]) or 0

    def local_search(self, td, actions, **kwargs):
        raise NotImplementedError(
            "local_search is not built for pdp: the TSP and CVRP searches know no "
            "pickup-before-delivery order")

    def improve(self, td, actions, *args, **kwargs):
        raise NotImplementedError(
            "improve is not built for pdp: the ruin-repair env (PDPRuinRepairEnv) and a "
            "precedence-aware local search are out of scope")
