"""Orienteering problem: env + generator on the gfx950 kernels
(``rl4co/envs/routing/op/``).  ``include/co_env.h`` (OP) states the arithmetic."""
from __future__ import annotations

import warnings
from typing import Callable, Union

import torch
from torch.distributions import Uniform

from .. import _native as nat
from ..td import TensorDict, set_many
from .base import RL4COEnvBase
from .common import Generator, device_uniform, get_sampler

# Kool et al. 2019 (``op/generator.py:14``)
MAX_LENGTHS = {20: 2.0, 50: 3.0, 100: 4.0}


class OPGenerator(Generator):
    """``op/generator.py:17-149``: a depot and ``num_loc`` customers uniform on ``[min_loc,
    max_loc]^2``, a prize per customer and a ``max_length`` per instance, drawn in the
    reference's order (the locations, then ``unif``'s ``randint``).  Without a depot
    distribution one draw of ``[*B, num_loc + 1, 2]`` is split into the depot (row 0) and the
    customers.  ``prize_type``: ``const`` (1), ``unif`` ((1 + randint(0, 100)) / 100) or
    ``dist`` (by the distance to the depot, the farthest customer 1.0) -- torch arithmetic on
    the drawn tensors, exactly the reference's expressions.  ``max_length`` is a float, a
    ``[B]`` tensor (heterogeneous instances) or None: the ``MAX_LENGTHS`` table, and for a
    ``num_loc`` it does not hold the nearest size's value with a ``UserWarning`` (the
    reference logs one)."""

    def __init__(self, num_loc: int = 20, min_loc: float = 0.0, max_loc: float = 1.0,
                 loc_distribution: Union[int, float, str, type, Callable] = Uniform,
                 depot_distribution: Union[int, float, str, type, Callable] = None,
                 min_prize: float = 1.0, max_prize: float = 1.0,
                 prize_distribution: Union[int, float, type, Callable] = Uniform,
                 prize_type: str = "dist", max_length: Union[float, torch.Tensor] = None,
                 **kwargs):
        self.num_loc, self.min_loc, self.max_loc = num_loc, min_loc, max_loc
        self.min_prize, self.max_prize, self.prize_type = min_prize, max_prize, prize_type
        self.device = kwargs.get("device")
        self.loc_sampler = kwargs.get("loc_sampler") or get_sampler(
            "loc", loc_distribution, min_loc, max_loc, **kwargs)
        self.depot_sampler = kwargs.get("depot_sampler") or (
            get_sampler("depot", depot_distribution, min_loc, max_loc, **kwargs)
            if depot_distribution is not None else None)
        # kept as the reference keeps it, though _generate never draws from it; the
        # reference's default Uniform(1, 1) is a sampler torch refuses to build: None
        if kwargs.get("prize_sampler") is not None:
            self.prize_sampler = kwargs["prize_sampler"]
        elif prize_distribution == "dist" or (
                prize_distribution in (Uniform, "uniform") and min_prize >= max_prize):
            self.prize_sampler = None
        else:
            self.prize_sampler = get_sampler("prize", prize_distribution, min_prize, max_prize,
                                             **kwargs)
        self.max_length = max_length if max_length is not None else MAX_LENGTHS.get(num_loc)
        if self.max_length is None:
            closest = min(MAX_LENGTHS.keys(), key=lambda x: abs(x - num_loc))
            self.max_length = MAX_LENGTHS[closest]
            warnings.warn(f"The max length for {num_loc} locations is not defined. Using the "
                          f"closest max length: {self.max_length} with {closest} locations.",
                          UserWarning, stacklevel=2)

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
        dev = locs.device
        # Fischetti et al. (1998), Kool et al. (2019): op/generator.py:115-133
        if self.prize_type == "const":
            prize = torch.ones(*batch_size, self.num_loc, device=dev)
        elif self.prize_type == "unif":
            prize = (1 + torch.randint(0, 100, (*batch_size, self.num_loc), device=dev)
                     .float()) / 100
        elif self.prize_type == "dist":
            prize = (depot[..., None, :] - locs).norm(p=2, dim=-1)
            prize = (1 + (prize / prize.max(dim=-1, keepdim=True)[0] * 99).int()).float() / 100
        else:
            raise ValueError(f"Invalid prize_type: {self.prize_type}")
        if not isinstance(self.max_length, torch.Tensor):
            max_length = torch.full((*batch_size,), self.max_length)
        else:
            max_length = self.max_length
        return TensorDict({"locs": locs, "depot": depot, "prize": prize,
                           "max_length": max_length}, batch_size=batch_size)


class OPEnv(RL4COEnvBase):
    """``op/env.py:24-262``: collect prizes on a tour from and back to the depot no longer
    than ``max_length``; the episode of a row ends when the policy returns to the depot
    (action 0 after the first step).  One launch per reset / step; ``step_many`` runs preset
    steps in one launch (``co_op_steps``), ``decode_and_step`` fuses the decode step with the
    env step (``co_op_decode_step``) when ``fused_step`` is set."""

    name = "op"
    # Whether the decode loop takes co_op_decode_step or the pair co_decode_step +
    # co_op_step: the measurement of tools/bench_op.py (DESIGN.md section 4 "Orienteering":
    # 22.3 against 56.6 us a step at B = 32,768, 8.27 against 19.9 at B = 1,024, OP-100).
    fused_step = True
    _MESSAGES = [(nat.ST_OP_DUPLICATE, AssertionError, "Duplicates"),
                 (nat.ST_OP_LENGTH, AssertionError, "Max length exceeded")]
    _SINGLE = (nat.ST_OP_SINGLE_NONZERO, AssertionError,
               "If all length 1 tours, they should be zero")
    _RANGE = (nat.ST_INDEX_RANGE, RuntimeError, "index out of range in gather (actions)")

    def __init__(self, generator: OPGenerator = None, generator_params: dict = {},
                 prize_type: str = "dist", **kwargs):
        super().__init__(**kwargs)
        self.generator = generator if generator is not None else OPGenerator(**generator_params)
        self.prize_type = prize_type
        assert self.prize_type in ["dist", "unif", "const"], \
            f"Invalid prize_type: {self.prize_type}"

    def native_decode_and_step(self):
        """No step glue for this env (``csrc/pycall/co_torchstep.cpp`` is not extended):
        the decode loop calls ``decode_and_step``, the fused launch while ``fused_step`` is
        set (the default, by measurement); unset, the loop takes the pair."""
        return None

    def _reset(self, td=None, batch_size=None) -> TensorDict:
        """``op/env.py:110-151`` in one ``co_op_reset`` launch."""
        depot, locs, prize, max_length = td["depot"], td["locs"], td["prize"], td["max_length"]
        nat.require_device(depot, locs, prize, max_length)
        depot, locs = depot.float().contiguous(), locs.float().contiguous()
        prize = prize.float().contiguous()
        b, n = locs.shape[0], locs.shape[-2]
        max_length = max_length.float().reshape(-1).contiguous()
        if max_length.numel() != b or prize.shape != (b, n):
            raise ValueError(f"td['max_length'] must be [{b}] and td['prize'] [{b}, {n}], got "
                             f"{tuple(td['max_length'].shape)} and {tuple(prize.shape)}")
        dev = locs.device
        locs_out = torch.empty((b, n + 1, 2), dtype=torch.float32, device=dev)
        cols = torch.empty((2, b, n + 1), dtype=torch.float32, device=dev)
        scal = torch.empty((2, b), dtype=torch.float32, device=dev)
        cur = torch.empty((b, 1), dtype=torch.int64, device=dev)
        i = torch.empty((b,), dtype=torch.int64, device=dev)
        rows = torch.empty((2, b, n + 1), dtype=torch.bool, device=dev)
        nat.call("co_op_reset", b, n, nat.ptr(depot), nat.ptr(locs), nat.ptr(prize),
                 nat.ptr(max_length), nat.ptr(locs_out), nat.ptr(cols[0]), nat.ptr(cols[1]),
                 nat.ptr(scal[0]), nat.ptr(scal[1]), nat.ptr(cur), nat.ptr(i), nat.ptr(rows[0]),
                 nat.ptr(rows[1]), nat.stream_of(locs))
        self._remember_i(i, 0)
        return TensorDict({"locs": locs_out, "prize": cols[0], "tour_length": scal[0],
                           "max_length": cols[1], "current_node": cur, "visited": rows[0],
                           "current_total_prize": scal[1], "i": i, "action_mask": rows[1]},
                          batch_size=batch_size)

    @staticmethod
    def _state(td):
        """The td's instance and state tensors as the step entries take them."""
        keys = ("locs", "prize", "max_length", "visited", "tour_length", "current_total_prize",
                "current_node", "i")
        ts = [td[k] for k in keys]
        nat.require_device(*ts)
        visited = ts[3]
        if visited.dim() != 2 or ts[0].shape[:2] != visited.shape:
            raise ValueError("td['visited'] must be [B, N+1] beside td['locs'] [B, N+1, 2], got "
                             f"{tuple(visited.shape)} and {tuple(ts[0].shape)}")
        return [t.contiguous() for t in ts]

    def _step(self, td: TensorDict) -> TensorDict:
        """``op/env.py:74-108`` in one ``co_op_step`` launch; every output is a fresh tensor
        (the reference's scatter is out of place).  An action outside ``0..N``, on which
        torch's scatter raises at once, edits nothing here and raises with the rollout's
        ``get_reward`` (or in ``step_many``), as in the other envs."""
        action = td["action"]
        locs, prize, ml, visited, tl, pz, cur, i = self._state(td)
        nat.require_device(action, visited)
        if action.dtype != torch.int64:
            action = action.long()
        action = action.contiguous()
        b, nc = visited.shape
        dev = visited.device
        s = nat.stream_of(visited)
        outs = self._step_outputs(b, nc, dev, s)
        vis_out, mask, tl_out, pz_out, cur_out, i_out, done, reward = outs
        nat.call("co_op_step", b, nc - 1, nat.ptr(action), nat.ptr(locs), nat.ptr(prize),
                 nat.ptr(ml), nat.ptr(visited), nat.ptr(vis_out), nat.ptr(tl), nat.ptr(tl_out),
                 nat.ptr(pz), nat.ptr(pz_out), nat.ptr(cur), nat.ptr(cur_out), nat.ptr(i),
                 nat.ptr(i_out), nat.ptr(done), nat.ptr(reward), nat.ptr(mask), None, s)
        return self._after_step(td, *outs)

    def _step_outputs(self, b, nc, dev, s):
        return (self._out((b, nc), torch.bool, dev, s), self._out((b, nc), torch.bool, dev, s),
                self._out((b,), torch.float32, dev, s), self._out((b,), torch.float32, dev, s),
                self._out((b, 1), torch.int64, dev, s), self._out((b,), torch.int64, dev, s),
                self._out((b,), torch.bool, dev, s), self._out((b,), torch.bool, dev, s))

    @staticmethod
    def _after_step(td, vis_out, mask, tl_out, pz_out, cur_out, i_out, done, reward, extra=None):
        out = {"tour_length": tl_out, "current_node": cur_out, "visited": vis_out,
               "current_total_prize": pz_out, "i": i_out, "reward": reward, "done": done,
               "action_mask": mask}
        if extra:
            out.update(extra)
        set_many(td, out)
        return td

    def step_many(self, td, actions, step_major: bool = False):
        """T preset steps in one ``co_op_steps`` launch: ``actions`` is ``[B, T]`` (a
        rollout's layout) or, with ``step_major``, ``[T, B]``; any strides.  Leaves ``td`` as
        the T ``step`` calls would, bit for bit, in fresh tensors, and returns ``(feasible,
        length)``, both ``[T, B]``: whether ``action_mask[b, a_t]`` held before step t, and
        the tour length after it.  An action outside ``0..N`` raises."""
        locs, prize, ml, visited, tl, pz, cur, i = self._state(td)
        mask_in = td["action_mask"]
        nat.require_device(actions, mask_in, visited)
        if actions.dtype != torch.int64:
            actions = actions.long()
        b, nc = visited.shape
        if actions.dim() != 2 or actions.shape[0 if not step_major else 1] != b:
            raise ValueError(f"actions must be [{b}, T] (or [T, {b}] with step_major), got "
                             f"{tuple(actions.shape)}")
        if not step_major:
            actions = actions.t()
        t = actions.shape[0]
        if t == 0:
            raise ValueError("step_many needs at least one step")
        dev = visited.device
        mask_in = mask_in.contiguous()
        visited, tl, pz = visited.clone(), tl.clone(), pz.clone()
        cur, i = cur.long().clone(), i.long().clone()
        mask = torch.empty((b, nc), dtype=torch.bool, device=dev)
        done = torch.empty(b, dtype=torch.bool, device=dev)
        reward = torch.empty(b, dtype=torch.bool, device=dev)
        feasible = torch.empty((t, b), dtype=torch.bool, device=dev)
        length = torch.empty((t, b), dtype=torch.float32, device=dev)
        status = self.status_word(dev)
        nat.call("co_op_steps", b, nc - 1, t, nat.ptr(actions), actions.stride(0),
                 actions.stride(1), nat.ptr(locs), nat.ptr(prize), nat.ptr(ml), nat.ptr(mask_in),
                 nat.ptr(visited), nat.ptr(tl), nat.ptr(pz), nat.ptr(cur), nat.ptr(i),
                 nat.ptr(done), nat.ptr(reward), nat.ptr(mask), nat.ptr(feasible),
                 nat.ptr(length), nat.ptr(status), nat.stream_of(visited))
        self.raise_for_status(status, [(nat.ST_INDEX_RANGE, RuntimeError,
                                        "index out of range in step_many (actions)")])
        self._after_step(td, visited, mask, tl, pz, cur, i, done, reward,
                         extra={"action": actions[-1]})
        return feasible, length

    def decode_and_step(self, td, logits, mode, temperature, tanh_clipping, action_in, seed,
                        offset, status, key="action"):
        """``DecodingStrategy.step`` + ``_step`` (``decoding.py:327-369``,
        ``op/env.py:74-108``) in one ``co_op_decode_step`` launch: the same selection,
        log-probability, RNG use and state as the two calls.  Returns ``(action, logp)``, or
        None when it does not apply (``fused_step`` unset, CPU tensors, non-f32 logits, rows
        past the entries' limit): the loop then takes the two calls."""
        if not self.fused_step:
            return None
        mask = td["action_mask"]
        ops = self._fused_operands(logits, action_in, mask)
        if ops is None or mask.shape[1] - 1 > nat.OP_MAX_N or mask.shape[1] < 2:
            return None
        b, nc, ain, act, logp, sel, s = ops
        locs, prize, ml, visited, tl, pz, cur, i = self._state(td)
        dev = mask.device
        m = mask.contiguous()
        outs = self._step_outputs(b, nc, dev, s)
        vis_out, mask_out, tl_out, pz_out, cur_out, i_out, done, reward = outs
        inst = nat.op_instance(locs, prize, ml)  # referenced until the call returns
        nat.call("co_op_decode_step", b, nc - 1, nat.ptr(logits), logits.stride(0), nat.ptr(m),
                 float(tanh_clipping), float(temperature), mode, nat.ptr(ain), nat.ptr(act),
                 nat.ptr(logp), seed, offset, inst.address, nat.ptr(visited), nat.ptr(vis_out), nat.ptr(tl), nat.ptr(tl_out), nat.ptr(pz),
                 nat.ptr(pz_out), nat.ptr(cur), nat.ptr(cur_out), nat.ptr(i), nat.ptr(i_out),
                 nat.ptr(done), nat.ptr(reward), nat.ptr(mask_out), None, nat.ptr(status), s)
        self._after_step(td, *outs, extra={key: sel})
        return sel, logp

    def _get_reward(self, td, actions, check: bool = False) -> torch.Tensor:
        """``op/env.py:171-180``: the prizes of the visited nodes, fused with the two
        validity tests (``co_op_reward``).  A multistart td's un-replicated rows
        (``RepeatedRows``) are read in place: env ``e`` uses instance row ``e % B`` (the
        kernel's ``prize_batch`` / ``locs_batch``)."""
        prize, = self._instance_entries(td, ("prize",))
        nat.require_device(prize, actions)
        prize = prize.contiguous()
        locs = ml = None
        if check:
            locs, ml = self._instance_entries(td, ("locs", "max_length"))
            nat.require_device(locs, ml, actions)
            locs, ml = locs.contiguous(), ml.contiguous()
        if actions.dtype != torch.int64:
            actions = actions.long()
        b, t = actions.shape
        reward = torch.empty(b, dtype=torch.float32, device=prize.device)
        status = self.status_word(prize.device)
        nat.call("co_op_reward", b, prize.shape[-1] - 1, t, nat.ptr(prize), prize.shape[0],
                 nat.ptr(locs), nat.ptr(ml), locs.shape[0] if check else 1, nat.ptr(actions),
                 actions.stride(0), actions.stride(1), int(check), nat.ptr(reward),
                 nat.ptr(status), nat.stream_of(prize))
        self.raise_for_status(status, (self._MESSAGES if check else [])
                              + [self._SINGLE, self._RANGE])
        return reward

    def check_solution_validity(self, td, actions) -> None:
        """``op/env.py:182-214``: the first failing message, in the reference's order."""
        self._get_reward(td, actions, check=True)

    def get_action_mask(self, td):
        """``op/env.py:153-169`` from the td's state (``co_op_action_mask``)."""
        locs, _, ml, visited, tl, _, cur, _ = self._state(td)
        b, nc = visited.shape
        mask = torch.empty((b, nc), dtype=torch.bool, device=visited.device)
        nat.call("co_op_action_mask", b, nc - 1, nat.ptr(locs), nat.ptr(ml), nat.ptr(visited),
                 nat.ptr(tl), nat.ptr(cur), nat.ptr(mask), nat.stream_of(visited))
        return mask

    def get_num_starts(self, td):
        """``ops.py:126-136``: the depot cannot be a start node."""
        return td["action_mask"].shape[-1] - 1

    def select_start_nodes(self, td, num_starts):
        """``ops.py:139-174``: customer ``s % num_loc + 1`` for start ``s``, start-major --
        unless a row has fewer open customers than starts: then every row's starts are drawn
        with replacement from its open customers (``torch.multinomial`` on the mask)."""
        num_loc = self.generator.num_loc
        sel = torch.arange(num_starts, device=td.device).repeat_interleave(td.shape[0]) \
            % num_loc + 1
        open_ = td["action_mask"][..., 1:].float()
        if (open_.sum(-1) < num_starts).any():
            sel = torch.multinomial(open_, num_starts, replacement=True) + 1
            sel = sel.t().reshape(-1)  # "b n -> (n b)"
        return sel

    def min_steps_to_done(self, td) -> int:
        """done = action 0 with ``i > 0`` (``op/env.py:91``): from a reset state no row can
        be done before its second step."""
        i = td.get_raw("i") if hasattr(td, "get_raw") else td["i"]
        return 2 if isinstance(i, torch.Tensor) and self._known_i(i) == 0 else 0

    def local_search(self, td, actions, **kwargs):
        raise NotImplementedError(
            "local_search is not built for op: the TSP and CVRP searches visit every node and "
            "know no prize or length budget")

    def improve(self, td, actions, *args, **kwargs):
        raise NotImplementedError(
            "improve is not built for op: a prize-collecting local search is out of scope")
