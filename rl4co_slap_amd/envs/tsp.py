"""TSP env + generator on the gfx950 kernels (``rl4co/envs/routing/tsp/``)."""
from __future__ import annotations

from typing import Callable, Union

import torch
from torch.distributions import Uniform

from .. import _native as nat
from ..td import RepeatedRows, TensorDict, set_many
from .base import RL4COEnvBase
from .common import Generator, device_uniform, get_sampler


class TSPGenerator(Generator):
    """``tsp/generator.py:14-60``: ``locs ~ Uniform(min_loc, max_loc)`` drawn from
    torch's global CPU RNG (seeded by the env), shape ``[*B, num_loc, 2]``.  With
    ``device="cuda"`` a Uniform sampler draws on the GPU instead (``common.device_uniform``:
    same value grid, Philox stream keyed from the CPU RNG)."""

    def __init__(self, num_loc: int = 20, min_loc: float = 0.0, max_loc: float = 1.0,
                 init_sol_type: str = "random",
                 loc_distribution: Union[int, float, str, type, Callable] = Uniform, **kwargs):
        self.num_loc, self.min_loc, self.max_loc = num_loc, min_loc, max_loc
        self.init_sol_type = init_sol_type
        self.device = kwargs.get("device")
        self.loc_sampler = kwargs.get("loc_sampler") or get_sampler(
            "loc", loc_distribution, min_loc, max_loc, **kwargs)

    def _generate(self, batch_size) -> TensorDict:
        shape = (*batch_size, self.num_loc, 2)
        locs = device_uniform(self.loc_sampler, shape, self.device) if self.device else None
        if locs is None:
            locs = self.loc_sampler.sample(shape)
        return TensorDict({"locs": locs}, batch_size=batch_size)

    def _get_initial_solutions(self, coordinates) -> torch.Tensor:
        """``tsp/generator.py:62-99`` (the improvement MDP's start): a linked list ``rec``
        ``[B, N]`` on the coordinates' device.  ``"random"``: the tour
        ``torch.rand(B, N).argsort()`` from the global CPU RNG -- the reference's draw, so
        the same seed gives the same ``rec`` -- linked by ``co_tsp_linked_list``;
        ``"greedy"``: the nearest-neighbour tour from node 0 (``co_tsp_nearest_rec``)."""
        b = coordinates.shape[0]
        if self.init_sol_type == "random":
            from .tsp_kopt import ImprovementEnvBase

            tour = torch.rand(b, self.num_loc).argsort().long()
            return ImprovementEnvBase._get_linked_list_solution(tour.to(coordinates.device))
        if self.init_sol_type == "greedy":
            nat.require_device(coordinates)
            locs = coordinates.float().contiguous()
            rec = torch.empty((b, self.num_loc), dtype=torch.int64, device=locs.device)
            nat.call("co_tsp_nearest_rec", b, self.num_loc, nat.ptr(locs), nat.ptr(rec),
                     nat.stream_of(locs))
            return rec
        raise NotImplementedError()


class TSPEnv(RL4COEnvBase):
    """``tsp/env.py:29-173`` with ``_step``/``_reset``/``get_reward`` on the device."""

    name = "tsp"

    def __init__(self, generator: TSPGenerator = None, generator_params: dict = {}, **kwargs):
        super().__init__(**kwargs)
        self.generator = generator if generator is not None else TSPGenerator(**generator_params)

    def _reset(self, td=None, batch_size=None) -> TensorDict:
        """``tsp/env.py:95-120``: one fused reset kernel."""
        locs = td["locs"]
        nat.require_device(locs)
        b, n = locs.shape[0], locs.shape[-2]
        dev = locs.device
        cur = torch.empty(b, dtype=torch.int64, device=dev)  # first_node aliases it (env.py:113-114)
        mask = torch.empty((b, n), dtype=torch.bool, device=dev)
        i = torch.empty((b, 1), dtype=torch.int64, device=dev)
        reward = torch.empty((b, 1), dtype=torch.float32, device=dev)
        nat.call("co_tsp_reset", b, n, nat.ptr(mask), nat.ptr(cur), nat.ptr(cur), nat.ptr(i),
                 nat.ptr(reward), nat.stream_of(locs))
        self._remember_i(i, 0)
        self._remember_lb(mask, n)  # N ones; a step clears at most one
        return TensorDict({"locs": locs, "first_node": cur, "current_node": cur, "i": i,
                           "action_mask": mask, "reward": reward}, batch_size=batch_size)

    def _step(self, td: TensorDict) -> TensorDict:
        """``tsp/env.py:67-93`` in one kernel launch.  ``current_node`` aliases the
        action tensor exactly as the reference does."""
        action, mask, i = td["action"], td["action_mask"], td["i"]
        nat.require_device(action, mask, i)
        if action.dtype != torch.int64:
            action = action.long()
        action, mask, i = action.contiguous(), mask.contiguous(), i.contiguous()
        b, n = mask.shape
        dev = mask.device
        known = self._known_i(td["i"])
        first_in = td.get("first_node", None)
        flag = None
        if known is not None:
            mode = 1 if known == 0 else 0
        else:  # unknown provenance: batch-wide any(i == 0) on the device
            flag = torch.empty(1, dtype=torch.int32, device=dev)
            nat.call("co_any_eq_i64", nat.ptr(i), i.numel(), 0, nat.ptr(flag), nat.stream_of(i))
            mode = 2
        if first_in is None:
            first_in = action
        first_in = first_in.contiguous()
        s = nat.stream_of(mask)
        mask_out = self._out(mask.shape, mask.dtype, dev, s)
        i_out = self._out(i.shape, i.dtype, dev, s)
        first_out = self._out(action.shape, torch.int64, dev, s)
        done = self._out((b,), torch.bool, dev, s)
        reward = self._out((b,), torch.bool, dev, s)
        nat.call("co_tsp_step", b, n, nat.ptr(action), nat.ptr(mask), nat.ptr(mask_out),
                 nat.ptr(i), nat.ptr(i_out), nat.ptr(first_in), nat.ptr(first_out), None,
                 nat.ptr(done), nat.ptr(reward), mode, nat.ptr(flag), None, s)
        if known is not None:
            self._remember_i(i_out, known + 1)
        lb = self._known_lb(td["action_mask"])
        if lb is not None:
            self._remember_lb(mask_out, lb - 1)
        td.update({"first_node": first_out, "current_node": td["action"], "i": i_out,
                   "action_mask": mask_out, "reward": reward, "done": done})
        return td

    def native_decode_and_step(self):
        """``decode_and_step`` in one native call (``tsp_step_td``, bookkeeping included),
        which a decoding strategy's loop tries first: see ``_bound_glue``."""
        return self._bound_glue("tsp_step_td")

    def decode_and_step(self, td, logits, mode, temperature, tanh_clipping, action_in, seed,
                        offset, status, key="action"):
        """``DecodingStrategy.step`` + ``_step`` (``decoding.py:327-369``, ``tsp/env.py:67-93``)
        in one ``co_tsp_decode_step`` launch: the same selection, log-probability, state
        and aliasing (``current_node`` is the action tensor) as the two calls.  Returns
        ``(action, logp)``, or None when it does not apply (CPU tensors, unknown ``i``
        provenance for the batch-wide first-node test, non-f32 logits)."""
        mask, i = td["action_mask"], td["i"]
        known = self._known_i(i)
        if known is None:
            return None
        first_in = td.get("first_node", None)
        take = 1 if known == 0 else 0
        if not take and first_in is None:
            return None
        ts = nat.torchstep()
        if ts is not None:  # output allocation + launch in one native call
            r = nat.glue_result("co_tsp_decode_step", ts.tsp_decode_step(
                logits, mask, i, None if take else first_in, action_in, status,
                float(tanh_clipping), float(temperature), mode, seed, offset, take))
            if r is not None:
                act, logp, mask_out, i_out, first_out, done, reward = r
                return self._after_decode_step(td, key, act if action_in is None else action_in,
                                               logp, mask, mask_out, i_out, first_out, done,
                                               reward, known)
        ops = self._fused_operands(logits, action_in, mask)
        if ops is None:
            return None
        b, n, ain, act, logp, sel, s = ops
        dev = mask.device
        m, i = mask.contiguous(), i.contiguous()
        first_in = first_in.contiguous() if (first_in is not None and not take) else None
        mask_out = self._out(m.shape, m.dtype, dev, s)
        i_out = self._out(i.shape, i.dtype, dev, s)
        first_out = self._out((b,), torch.int64, dev, s)
        done = self._out((b,), torch.bool, dev, s)
        reward = self._out((b,), torch.bool, dev, s)
        nat.call("co_tsp_decode_step", b, n, nat.ptr(logits), logits.stride(0), nat.ptr(m),
                 float(tanh_clipping), float(temperature), mode, nat.ptr(ain), nat.ptr(act),
                 nat.ptr(logp), seed, offset, nat.ptr(mask_out), nat.ptr(i), nat.ptr(i_out),
                 nat.ptr(first_in), nat.ptr(first_out), take, nat.ptr(done), nat.ptr(reward),
                 None, nat.ptr(status), s)
        return self._after_decode_step(td, key, sel, logp, mask, mask_out, i_out, first_out,
                                       done, reward, known)

    def _after_decode_step(self, td, key, sel, logp, mask, mask_out, i_out, first_out, done,
                           reward, known):
        self._remember_i(i_out, known + 1)
        lb = self._known_lb(mask)
        if lb is not None:
            self._remember_lb(mask_out, lb - 1)
        set_many(td, {key: sel, "first_node": first_out, "current_node": sel, "i": i_out,
                      "action_mask": mask_out, "reward": reward, "done": done})
        return sel, logp

    def _get_reward(self, td, actions, check: bool = False) -> torch.Tensor:
        """``tsp/env.py:157-173``: -tour length, fused with the permutation check.  A
        multistart td's un-replicated ``locs`` (``RepeatedRows``) is read in place: env
        ``e`` uses coordinate row ``e % B`` (the kernel's ``locs_batch``)."""
        raw = td.get_raw("locs") if hasattr(td, "get_raw") else td["locs"]
        locs = raw.source() if isinstance(raw, RepeatedRows) else raw
        nat.require_device(locs, actions)
        locs = locs.contiguous()
        if actions.dtype != torch.int64:
            actions = actions.long()
        b, t = actions.shape
        reward = torch.empty(b, dtype=torch.float32, device=locs.device)
        status = self.status_word(locs.device)
        nat.call("co_tsp_reward", b, locs.shape[-2], t, nat.ptr(locs), locs.shape[0],
                 nat.ptr(actions),
                 actions.stride(0), actions.stride(1), int(check), nat.ptr(reward),
                 nat.ptr(status), nat.stream_of(locs))
        msgs = [(nat.ST_INVALID_TOUR, AssertionError, "Invalid tour")] if check else []
        msgs.append((nat.ST_INDEX_RANGE, RuntimeError, "index out of range in gather (actions)"))
        self.raise_for_status(status, msgs)
        return reward

    # TSPEnv.best_of's dispatch (DESIGN.md section 4 has the measurements): co_tsp_best_of
    # where it measured faster than reward + max + gather -- tours of more than 20 nodes
    # whose K candidates fit one round of the kernel's block (K lane groups in 1024
    # threads); elsewhere the two measured level and the composition stays.  True / False
    # forces one side (tests, tools/bench_best_of.py).
    _BEST_OF_MIN_LOC = 21
    _BEST_OF_FORCE = None

    def _best_of_fused(self, n: int, k: int) -> bool:
        if self._BEST_OF_FORCE is not None:
            return bool(self._BEST_OF_FORCE) and n <= 1024
        lanes = 4 if n <= 32 else 8 if n <= 64 else 16 if n <= 128 else 32 if n <= 256 else 64
        return self._BEST_OF_MIN_LOC <= n <= 1024 and k * lanes <= 1024

    def best_of(self, td, actions, num_candidates, rewards=None):
        """``RL4COEnvBase.best_of`` in one ``co_tsp_best_of`` launch: every candidate row
        scored against its instance's un-replicated coordinates (read once for its K
        candidates), the maximum taken and the winning row copied.  Applies when the rows
        are tours of ``num_loc`` steps (``20 < num_loc <= 1024``) over ``td["locs"]``
        ``[B, N, 2]`` and K fits one round of the kernel's block (``_best_of_fused``: e.g.
        K <= 64 at TSP-100); otherwise (or with ``rewards`` given) the base composition
        runs, which measured as fast there.
        ``check_solution`` checks every candidate row, as ``get_reward`` does."""
        k = 1
        for s in ([num_candidates] if isinstance(num_candidates, int) else num_candidates):
            k *= s if s > 0 else 1
        raw = td.get_raw("locs") if hasattr(td, "get_raw") else td["locs"]
        locs = raw.source() if isinstance(raw, RepeatedRows) else raw
        if (rewards is not None or locs.dim() != 3 or actions.dim() != 2
                or actions.shape[0] != k * locs.shape[0] or actions.shape[1] != locs.shape[1]
                or locs.shape[0] == 0 or not self._best_of_fused(locs.shape[1], k)):
            return super().best_of(td, actions, num_candidates, rewards)
        nat.require_device(locs, actions)
        locs = locs.contiguous().float()
        if actions.dtype != torch.int64:
            actions = actions.long()
        b, n = locs.shape[0], locs.shape[1]
        dev = locs.device
        best_r = torch.empty(b, dtype=torch.float32, device=dev)
        best_i = torch.empty(b, dtype=torch.int64, device=dev)
        best_a = torch.empty((b, n), dtype=torch.int64, device=dev)
        check = self.check_solution
        status = self.status_word(dev)
        nat.call("co_tsp_best_of", b, n, k, nat.ptr(locs), nat.ptr(actions), actions.stride(0),
                 actions.stride(1), int(check), None, nat.ptr(best_r), nat.ptr(best_i),
                 nat.ptr(best_a), nat.ptr(status), nat.stream_of(locs))
        msgs = [(nat.ST_INVALID_TOUR, AssertionError, "Invalid tour")] if check else []
        msgs.append((nat.ST_INDEX_RANGE, RuntimeError, "index out of range in gather (actions)"))
        self.raise_for_status(status, msgs)
        return best_r, best_i, best_a

    def check_solution_validity(self, td, actions) -> None:
        """``tsp/env.py:165-173``."""
        self._get_reward(td, actions, check=True)

    def local_search(self, td, actions, max_iterations: int = 1000, *,
                     return_sweeps: bool = False, operators=("two_opt",)):
        """``tsp/env.py:192-197`` (``tsp/local_search.py:14-74``): best-improvement 2-opt on
        every row of ``actions`` in one ``co_tsp_local_search`` launch
        (``ops.tsp_local_search``), on ``td["distances"]``
        when present, else the Euclidean distances of ``td["locs"]`` (a multistart td's
        un-replicated ``locs`` read in place, as ``_get_reward`` does).  Returns int64
        ``[B, N]`` on the actions' device; with ``return_sweeps`` also the sweeps per row.
        A row that is not a permutation raises ``AssertionError("Invalid tour")`` (the
        reference does not check).  ``operators=("two_opt", "or_opt")`` adds the Or-opt
        neighbourhood to the descent."""
        from ..utils.ops import tsp_local_search

        dist, = self._instance_entries(td, ["distances"])
        locs, = self._instance_entries(td, ["locs"]) if dist is None else (None,)
        status = self.status_word(actions.device)
        res = tsp_local_search(actions, locs=locs, distances=dist, operators=operators,
                               max_iterations=max_iterations, return_sweeps=return_sweeps,
                               status=status)
        self.raise_for_status(status, [(nat.ST_INVALID_TOUR, AssertionError, "Invalid tour")])
        return res

    def get_action_mask(self, td):
        return td["action_mask"]

    def min_steps_to_done(self, td) -> int:
        """done = no unvisited node (``tsp/env.py:78``), and a step clears one node."""
        return self._known_lb(td.get_raw("action_mask") if hasattr(td, "get_raw")
                              else td["action_mask"]) or 0

    def replace_selected_actions(self, cur_actions, new_actions, selection_mask):
        cur_actions[selection_mask] = new_actions[selection_mask]
        return cur_actions
