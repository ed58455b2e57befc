"""The k-opt improvement MDP of TSP on the gfx950 kernels: ``ImprovementEnvBase``
(``rl4co/envs/common/base.py:336-403``) and ``TSPkoptEnv`` (``rl4co/envs/routing/tsp/env.py:
204-549``), the env the reference's improvement policies (DACT, N2S, NeuOpt) step.

A solution is a linked list ``rec`` (int64 ``[B, N]``, ``rec[i] = j``: edge i -> j).  Every
method is one call of the C ABI (``csrc/tsp_kopt.hip``; CPU tensors: the host build); there
is no torch path.  ``improve_steps`` runs T steps with preset actions in one
``co_tsp_kopt_steps`` launch.  Data-dependent failures (an action index out of range, a
``rec`` that is not one N-cycle) are read from a status word after the call and raised.
"""
from __future__ import annotations

import abc

import torch

from .. import _native as nat
from ..td import TensorDict
from .base import RL4COEnvBase
from .tsp import TSPGenerator

_INVALID = (nat.ST_INVALID_TOUR, AssertionError, "Not visiting all nodes")
_RANGE = (nat.ST_INDEX_RANGE, RuntimeError, "index out of range in gather (action)")


def _raise(status, messages=(_INVALID, _RANGE)):
    bits, = nat.read_status([status], status.device)
    nat.release_status(status, (bits,))
    for bit, exc, msg in messages:
        if bits & bit:
            raise exc(msg)


def _rows(t: torch.Tensor, dtype=torch.int64) -> torch.Tensor:
    return (t if t.dtype == dtype else t.to(dtype)).contiguous()


class ImprovementEnvBase(RL4COEnvBase, metaclass=abc.ABCMeta):
    """``envs/common/base.py:336-403``: solutions in the linked-list format."""

    @abc.abstractmethod
    def _step(self, td, solution_to=None):
        raise NotImplementedError

    def step_to_solution(self, td, solution):
        return self._step(td, solution_to=solution)

    @staticmethod
    def _get_reward(td, actions):
        raise NotImplementedError(
            "This function is not used for improvement tasks since the reward is computed per step"
        )

    @staticmethod
    def get_costs(coordinates, rec):
        """``base.py:361-369``: the length of every row's tour (``co_tsp_kopt_reset``
        without the visiting times)."""
        nat.require_device(coordinates, rec)
        locs, rec = _rows(coordinates, torch.float32), _rows(rec)
        b, n = rec.shape
        cost = torch.empty(b, dtype=torch.float32, device=rec.device)
        status = nat.scratch_status(rec.device)
        nat.call("co_tsp_kopt_reset", b, n, nat.ptr(locs), locs.shape[0], nat.ptr(rec),
                 nat.ptr(cost), None, nat.ptr(status), nat.stream_of(rec))
        _raise(status)
        return cost

    @staticmethod
    def _get_real_solution(rec):
        """``base.py:371-384``: the visiting order ``[0, rec[0], rec[rec[0]], ...]``."""
        nat.require_device(rec)
        rec = _rows(rec)
        b, n = rec.shape
        out = torch.empty_like(rec)
        status = nat.scratch_status(rec.device)
        nat.call("co_tsp_real_solution", b, n, nat.ptr(rec), nat.ptr(out), nat.ptr(status),
                 nat.stream_of(rec))
        _raise(status)
        return out

    @staticmethod
    def _get_linked_list_solution(solution):
        """``base.py:386-393``: ``rec[t[k]] = t[(k+1) % N]`` of every tour row (any strides)."""
        nat.require_device(solution)
        if solution.dtype != torch.int64:
            solution = solution.long()
        b, n = solution.shape
        rec = torch.empty((b, n), dtype=torch.int64, device=solution.device)
        status = nat.scratch_status(solution.device)
        nat.call("co_tsp_linked_list", b, n, nat.ptr(solution), solution.stride(0),
                 solution.stride(1), nat.ptr(rec), nat.ptr(status), nat.stream_of(solution))
        _raise(status)
        return rec

    @classmethod
    def get_best_solution(cls, td):
        return cls._get_real_solution(td["rec_best"])

    @classmethod
    def get_current_solution(cls, td):
        return cls._get_real_solution(td["rec_current"])


class TSPkoptEnv(ImprovementEnvBase):
    """``tsp/env.py:204-549``: ``k_max == 2`` is the 2-opt MDP of DACT (action ``[B, 2]`` =
    first, second), ``k_max > 2`` the k-opt MDP of NeuOpt (action ``[B, 3*k_max]`` = index |
    left | right).  The reward of a step is the reduction of the best-so-far cost."""

    name = "tsp_kopt"

    def __init__(self, generator: TSPGenerator = None, generator_params: dict = {},
                 k_max: int = 2, **kwargs):
        super().__init__(**kwargs)
        self.generator = generator if generator is not None else TSPGenerator(**generator_params)
        if not 2 <= k_max <= nat.KOPT_MAX_K:
            raise ValueError(f"k_max must lie in 2..{nat.KOPT_MAX_K}, got {k_max}")
        self.k_max = k_max
        self.two_opt_mode = k_max == 2

    def _reset(self, td=None, batch_size=None) -> TensorDict:
        """``tsp/env.py:304-331``: the generator's initial solution, then its cost and
        visiting times in one ``co_tsp_kopt_reset`` launch."""
        locs = td["locs"]
        rec = self.generator._get_initial_solutions(locs).to(locs.device)
        nat.require_device(locs, rec)
        locs_c = _rows(locs, torch.float32)
        b, n = rec.shape
        dev = rec.device
        cost = torch.empty(b, dtype=torch.float32, device=dev)
        vt = torch.empty((b, n), dtype=torch.int64, device=dev)
        status = self.status_word(dev)
        nat.call("co_tsp_kopt_reset", b, n, nat.ptr(locs_c), locs_c.shape[0], nat.ptr(rec),
                 nat.ptr(cost), nat.ptr(vt), nat.ptr(status), nat.stream_of(rec))
        self.raise_for_status(status, [_INVALID])
        return TensorDict({"locs": locs, "cost_current": cost, "cost_bsf": cost.clone(),
                           "rec_current": rec, "rec_best": rec.clone(), "visited_time": vt,
                           "i": torch.zeros((*batch_size, 1), dtype=torch.int64, device=dev)},
                          batch_size=batch_size)

    def _action_width(self) -> int:
        return 2 if self.two_opt_mode else 3 * self.k_max

    def _step(self, td, solution_to=None):
        """``tsp/env.py:259-302`` in one ``co_tsp_kopt_step`` launch.  ``td["rec_best"]`` is
        updated in place, as the reference does; every other entry is a new tensor.

        When a row fails (an action index out of range, a list that is not one N-cycle) the
        error is raised after the launch, from the status word: only the failing row is
        unspecified, so the kernel has by then overwritten the ``td["rec_best"]`` rows of
        the other rows that improved, while no other entry of ``td`` is updated.  A caller
        that goes on after such an error resets, or restores ``rec_best`` from a copy."""
        best, locs, bsf = td["rec_best"], td["locs"], td["cost_bsf"]
        given = td["rec_current"] if solution_to is None else solution_to
        action = td["action"] if solution_to is None else None
        nat.require_device(best, locs, bsf, given, action)
        if best.dtype != torch.int64 or not best.is_contiguous():
            raise ValueError("td['rec_best'] must be a contiguous int64 tensor: the step "
                             "updates it in place")
        locs, bsf, given = _rows(locs, torch.float32), _rows(bsf, torch.float32), _rows(given)
        b, n = best.shape
        dev = best.device
        i_in = i_out = None
        sb = sa = 0
        if action is not None:
            if action.dtype != torch.int64:
                action = action.long()
            if action.dim() != 2 or action.shape != (b, self._action_width()):
                raise ValueError(f"action must be [{b}, {self._action_width()}] for k_max = "
                                 f"{self.k_max}, got {tuple(action.shape)}")
            sb, sa = action.stride()
            i_in = _rows(td["i"])
            i_out = torch.empty_like(i_in)
        rec = torch.empty((b, n), dtype=torch.int64, device=dev)
        cost = torch.empty(b, dtype=torch.float32, device=dev)
        now_bsf = torch.empty(b, dtype=torch.float32, device=dev)
        reward = torch.empty(b, dtype=torch.float32, device=dev)
        vt = torch.empty((b, n), dtype=torch.int64, device=dev)
        status = self.status_word(dev)
        nat.call("co_tsp_kopt_step", b, n, self.k_max, nat.ptr(locs), locs.shape[0],
                 nat.ptr(given), nat.ptr(action), sb, sa, nat.ptr(rec), nat.ptr(cost),
                 nat.ptr(bsf), nat.ptr(now_bsf), nat.ptr(reward), nat.ptr(best), nat.ptr(vt),
                 nat.ptr(i_in), nat.ptr(i_out), nat.ptr(status), nat.stream_of(best))
        self.raise_for_status(status, [_INVALID, _RANGE])
        td.update({"cost_current": cost, "cost_bsf": now_bsf, "rec_current": rec,
                   "rec_best": best, "visited_time": vt,
                   "i": td["i"] if action is None else i_out, "reward": reward})
        return td

    def improve_steps(self, td, actions):
        """T consecutive steps with the preset ``actions [T, B, A]`` (any strides) in one
        ``co_tsp_kopt_steps`` launch: returns the rewards ``[T, B]`` and leaves ``td`` as the
        T ``step`` calls would (bit for bit; ``reward`` is the last step's).

        A failing row raises after the launch as in ``_step``: ``td["rec_best"]`` then
        already holds the improved rows of the rows that did not fail (written in place),
        and nothing else of ``td`` is updated."""
        best, locs = td["rec_best"], td["locs"]
        nat.require_device(best, locs, actions, td["rec_current"], td["cost_bsf"])
        if best.dtype != torch.int64 or not best.is_contiguous():
            raise ValueError("td['rec_best'] must be a contiguous int64 tensor: the steps "
                             "update it in place")
        if actions.dtype != torch.int64:
            actions = actions.long()
        b, n = best.shape
        if actions.dim() != 3 or actions.shape[1:] != (b, self._action_width()):
            raise ValueError(f"actions must be [T, {b}, {self._action_width()}] for k_max = "
                             f"{self.k_max}, got {tuple(actions.shape)}")
        t = actions.shape[0]
        dev = best.device
        locs = _rows(locs, torch.float32)
        rec = _rows(td["rec_current"]).clone()
        bsf = _rows(td["cost_bsf"], torch.float32).clone()
        i = _rows(td["i"]).clone()
        cost = torch.empty(b, dtype=torch.float32, device=dev)
        vt = torch.empty((b, n), dtype=torch.int64, device=dev)
        rewards = torch.empty((t, b), dtype=torch.float32, device=dev)
        status = self.status_word(dev)
        nat.call("co_tsp_kopt_steps", b, n, self.k_max, t, nat.ptr(locs), locs.shape[0],
                 nat.ptr(actions), *actions.stride(), nat.ptr(rec), nat.ptr(cost), nat.ptr(bsf),
                 nat.ptr(best), nat.ptr(vt), nat.ptr(i), nat.ptr(rewards), None,
                 nat.ptr(status), nat.stream_of(best))
        self.raise_for_status(status, [_INVALID, _RANGE])
        td.update({"cost_current": cost, "cost_bsf": bsf, "rec_current": rec, "rec_best": best,
                   "visited_time": vt, "i": i})
        if t:
            td.update({"reward": rewards[-1], "action": actions[-1]})
        return rewards

    def check_solution_validity(self, td, actions=None):
        """``tsp/env.py:441-453``: the best-so-far list visits every node."""
        solution = td["rec_best"]
        n = solution.shape[1]
        assert (torch.arange(n, device=solution.device).view(1, -1).expand_as(solution)
                == solution.sort(1)[0]).all(), "Not visiting all nodes"

    def get_mask(self, td):
        """``tsp/env.py:455-464``."""
        bs, gs = td["visited_time"].shape
        if self.two_opt_mode:
            eye = torch.eye(gs, device=td["visited_time"].device).view(1, gs, gs)
            return ~eye.expand(bs, gs, gs).bool()
        assert False, "The masks for NeuOpt are handled within its policy"
