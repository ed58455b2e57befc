"""CVRP with time windows: env + generator on the gfx950 kernels
(``rl4co/envs/routing/cvrptw/``).  ``include/co_env.h`` (CVRPTW) states the arithmetic."""
from __future__ import annotations

from typing import Callable, Union

import torch
from torch.distributions import Uniform

from .. import _native as nat
from ..td import TensorDict, set_many
from .base import RL4COEnvBase
from .cvrp import CVRPEnv, CVRPGenerator

_DT = {torch.float32: nat.DT_F32, torch.int32: nat.DT_I32, torch.int64: nat.DT_I64}


def _timed(x):
    """A durations / time_windows tensor as the kernels take it: contiguous, in its own
    dtype when that is f32 / i32 / i64 (cast to f32 on load), else converted to f32."""
    if x.dtype not in _DT:
        x = x.float()
    return x.contiguous(), _DT[x.dtype]


class CVRPTWGenerator(CVRPGenerator):
    """``cvrptw/generator.py:12-162``: CVRP instances on ``[0, max_loc = 150]^2`` plus zero
    service durations and integer windows inside ``[depot distance, max_time - depot
    distance]``; the depot's window is ``[0, max_time]``.  ``scale=True`` divides
    durations, windows and coordinates by ``max_time`` (the windows become f32).  On the
    CPU the draws and every operation are the reference's, on the same global stream; with
    ``device="cuda"`` the CVRP part draws on the device as ``CVRPGenerator`` does and the
    window arithmetic runs there."""

    def __init__(self, num_loc: int = 20, min_loc: float = 0.0, max_loc: float = 150.0,
                 loc_distribution: Union[int, float, str, type, Callable] = Uniform,
                 depot_distribution: Union[int, float, str, type, Callable] = None,
                 min_demand: int = 1, max_demand: int = 10,
                 demand_distribution: Union[int, float, type, Callable] = Uniform,
                 vehicle_capacity: float = 1.0, capacity: float = None, max_time: float = 480,
                 scale: bool = False, **kwargs):
        super().__init__(num_loc=num_loc, min_loc=min_loc, max_loc=max_loc,
                         loc_distribution=loc_distribution,
                         depot_distribution=depot_distribution, min_demand=min_demand,
                         max_demand=max_demand, demand_distribution=demand_distribution,
                         vehicle_capacity=vehicle_capacity, capacity=capacity, **kwargs)
        self.min_time, self.max_time, self.scale = 0.0, max_time, scale

    def _generate(self, batch_size) -> TensorDict:
        td = super()._generate(batch_size)
        dev = td["locs"].device
        shape = (*batch_size, self.num_loc + 1)
        durations = torch.zeros(shape, dtype=torch.float32, device=dev)
        # depot -> customer distances with a leading 0 for the depot (generator.py:95-96)
        dist = (td["depot"] - td["locs"].transpose(0, 1)).norm(p=2, dim=-1).transpose(0, 1)
        dist = torch.cat((torch.zeros(*batch_size, 1, device=dev), dist), dim=1)
        upper = self.max_time - dist - durations  # latest start that still gets back in time
        u1 = torch.rand(shape, device=dev)
        u2 = torch.rand(shape, device=dev)
        a = (dist + (upper - dist) * u1).int()
        b = (dist + (upper - dist) * u2).int()
        lo, hi = torch.min(a, b), torch.max(a, b)
        lo[..., :, 0] = 0.0
        hi[..., :, 0] = self.max_time
        # an empty window (generator.py:119-137): open it one unit earlier, not before the
        # depot distance; if still empty, close it one unit later, within the upper bound
        empty = lo == hi
        if torch.any(empty):
            lo2 = lo.clone()
            lo2[empty] = torch.max(dist[empty].int(), lo2[empty] - 1)
            lo = lo2
            empty = lo == hi
            if torch.any(empty):
                hi2 = hi.clone()
                hi2[empty] = torch.min(torch.floor(upper[empty]).int(),
                                       torch.max(torch.ceil(lo2[empty] + durations[empty]).int(),
                                                 hi2[empty] + 1))
                hi = hi2
        if self.scale:
            durations = durations / self.max_time
            lo = lo / self.max_time
            hi = hi / self.max_time
            td["depot"] = td["depot"] / self.max_time
            td["locs"] = td["locs"] / self.max_time
        assert torch.all(lo < hi), ("Please make sure the relation between max_loc and max_time "
                                    "allows for feasible solutions.")
        durations[:, 0] = 0.0
        td.update({"durations": durations, "time_windows": torch.stack((lo, hi), dim=-1)})
        return td


class CVRPTWEnv(CVRPEnv):
    """``cvrptw/env.py:21-291``: CVRP whose customers must be reached before their window
    closes.  One launch per reset / step (time update + CVRP step + mask); ``step_many``
    runs preset steps in one launch."""

    name = "cvrptw"
    # the fused co_cvrp_decode_step knows no windows: the decode loop takes the two-call
    # path (co_decode_step, then this env's step)
    decode_and_step = None

    def __init__(self, generator: CVRPTWGenerator = None, generator_params: dict = {}, **kwargs):
        RL4COEnvBase.__init__(self, **kwargs)
        self.generator = generator if generator is not None else CVRPTWGenerator(**generator_params)

    def native_decode_and_step(self):
        return None

    def _reset(self, td=None, batch_size=None) -> TensorDict:
        """``cvrptw/env.py:136-165`` in one ``co_cvrptw_reset`` launch."""
        depot, locs, demand = td["depot"], td["locs"], td["demand"]
        durations, tw = td["durations"], td["time_windows"]
        nat.require_device(depot, locs, demand, durations, tw)
        depot, locs, demand = depot.contiguous(), locs.contiguous(), demand.contiguous()
        twc, tw_dt = _timed(tw)
        b, n = demand.shape
        dev = demand.device
        locs_out = torch.empty((b, n + 1, 2), dtype=torch.float32, device=dev)
        cur = torch.empty((b, 1), dtype=torch.int64, device=dev)
        time = torch.empty((b, 1), dtype=torch.float32, device=dev)
        used = torch.empty((b, 1), dtype=torch.float32, device=dev)
        vcap = torch.empty((b, 1), dtype=torch.float32, device=dev)
        visited = torch.empty((b, n + 1), dtype=torch.uint8, device=dev)
        cur_loc = torch.empty((b, 2), dtype=torch.float32, device=dev)
        dist = torch.empty((b, n + 1), dtype=torch.float32, device=dev)
        mask = torch.empty((b, n + 1), dtype=torch.bool, device=dev)
        nat.call("co_cvrptw_reset", b, n, nat.ptr(depot), nat.ptr(locs), nat.ptr(demand),
                 float(self.generator.vehicle_capacity), nat.ptr(twc), tw_dt, nat.ptr(locs_out),
                 nat.ptr(cur), nat.ptr(time), nat.ptr(used), nat.ptr(vcap), nat.ptr(visited),
                 nat.ptr(cur_loc), nat.ptr(dist), nat.ptr(mask), nat.stream_of(demand))
        self._remember_lb(visited, n + 1)
        return TensorDict({"locs": locs_out, "demand": demand, "current_node": cur,
                           "current_time": time, "used_capacity": used,
                           "vehicle_capacity": vcap, "visited": visited,
                           "durations": durations, "time_windows": tw, "current_loc": cur_loc,
                           "distances": dist, "action_mask": mask}, batch_size=batch_size)

    def _state(self, td):
        """The td's state tensors as the step entries take them."""
        locs, demand, used, vcap, visited, time, dist = (
            td["locs"], td["demand"], td["used_capacity"], td["vehicle_capacity"], td["visited"],
            td["current_time"], td["distances"])
        durations, tw = td["durations"], td["time_windows"]
        nat.require_device(locs, demand, used, vcap, visited, time, dist, durations, tw)
        if dist.shape != visited.shape:
            raise ValueError("td['distances'] must be the [B, N+1] vector the last mask call "
                             f"stored, got {tuple(dist.shape)}")
        return (*(x.contiguous() for x in (locs, demand, used, vcap, visited, time, dist)),
                *_timed(durations), *_timed(tw))

    def _step(self, td: TensorDict) -> TensorDict:
        """``cvrptw/env.py:117-134`` + CVRP's step + ``get_action_mask`` in one
        ``co_cvrptw_step`` launch; every output is a fresh tensor."""
        action = td["action"]
        locs, demand, used, vcap, visited, time, dist_in, dur, dur_dt, tw, tw_dt = self._state(td)
        nat.require_device(action, demand)
        if action.dtype != torch.int64:
            action = action.long()
        action = action.contiguous()
        b, n = demand.shape
        dev = demand.device
        s = nat.stream_of(demand)
        used_out = self._out(used.shape, used.dtype, dev, s)
        visited_out = self._out(visited.shape, visited.dtype, dev, s)
        time_out = self._out((b, 1), torch.float32, dev, s)
        cur = self._out((b, 1), torch.int64, dev, s)
        done = self._out((b,), torch.bool, dev, s)
        reward = self._out((b,), torch.bool, dev, s)
        cur_loc = self._out((b, 2), torch.float32, dev, s)
        dist = self._out((b, n + 1), torch.float32, dev, s)
        mask = self._out((b, n + 1), torch.bool, dev, s)
        nat.call("co_cvrptw_step", b, n, nat.ptr(action), nat.ptr(locs), nat.ptr(demand),
                 nat.ptr(used), nat.ptr(used_out), nat.ptr(vcap), nat.ptr(visited),
                 nat.ptr(visited_out), nat.ptr(time), nat.ptr(dist_in), nat.ptr(dur), dur_dt,
                 nat.ptr(tw), tw_dt, nat.ptr(time_out), nat.ptr(cur), nat.ptr(done),
                 nat.ptr(reward), nat.ptr(cur_loc), nat.ptr(dist), nat.ptr(mask), None, None,
                 s)
        set_many(td, {"current_time": time_out, "current_loc": cur_loc, "distances": dist})
        return self._after_step(td, used_out, visited_out, cur, done, reward, mask)

    def step_many(self, td, actions, step_major: bool = False):
        """T preset steps in one ``co_cvrptw_steps`` launch: ``actions`` is ``[B, T]`` (a
        rollout's layout) or, with ``step_major``, ``[T, B]``; any strides.  Leaves ``td``
        as the T ``step`` calls would, bit for bit, in fresh tensors, and returns
        ``(feasible, time)``, both ``[T, B]``: whether ``action_mask[b, a_t]`` held before
        step t, and ``current_time`` after it.  An action outside ``0..N`` raises."""
        locs, demand, used, vcap, visited, time, dist_in, dur, dur_dt, tw, tw_dt = self._state(td)
        cur = td["current_node"]
        nat.require_device(actions, cur, demand)
        if actions.dtype != torch.int64:
            actions = actions.long()
        b, n = demand.shape
        if actions.dim() != 2 or actions.shape[0 if not step_major else 1] != b:
            raise ValueError(f"actions must be [{b}, T] (or [T, {b}] with step_major), got "
                             f"{tuple(actions.shape)}")
        if not step_major:
            actions = actions.t()
        t = actions.shape[0]
        if t == 0:
            raise ValueError("step_many needs at least one step")
        dev = demand.device
        used, visited, time = used.clone(), visited.clone(), time.clone()
        cur = cur.long().contiguous().clone()
        done = torch.empty(b, dtype=torch.bool, device=dev)
        reward = torch.empty(b, dtype=torch.bool, device=dev)
        cur_loc = torch.empty((b, 2), dtype=torch.float32, device=dev)
        dist = torch.empty((b, n + 1), dtype=torch.float32, device=dev)
        mask = torch.empty((b, n + 1), dtype=torch.bool, device=dev)
        feasible = torch.empty((t, b), dtype=torch.bool, device=dev)
        times = torch.empty((t, b), dtype=torch.float32, device=dev)
        status = self.status_word(dev)
        nat.call("co_cvrptw_steps", b, n, t, nat.ptr(actions), actions.stride(0),
                 actions.stride(1), nat.ptr(locs), nat.ptr(demand), nat.ptr(used), nat.ptr(vcap),
                 nat.ptr(visited), nat.ptr(time), nat.ptr(cur), nat.ptr(dist_in), nat.ptr(dur),
                 dur_dt, nat.ptr(tw), tw_dt, nat.ptr(done), nat.ptr(reward), nat.ptr(cur_loc),
                 nat.ptr(dist), nat.ptr(mask), nat.ptr(feasible), nat.ptr(times),
                 nat.ptr(status), None, nat.stream_of(demand))
        self.raise_for_status(status, [(nat.ST_INDEX_RANGE, RuntimeError,
                                        "index out of range in step_many (actions)")])
        set_many(td, {"action": actions[-1], "current_time": time, "current_loc": cur_loc,
                      "distances": dist, "current_node": cur, "used_capacity": used,
                      "visited": visited, "reward": reward, "done": done, "action_mask": mask})
        return feasible, times

    @staticmethod
    def get_action_mask(td: TensorDict) -> torch.Tensor:
        """``cvrptw/env.py:103-115``; like the reference it also stores ``current_loc`` and
        ``distances`` in ``td``."""
        locs, demand, used, vcap, visited, cur, time = (
            td["locs"], td["demand"], td["used_capacity"], td["vehicle_capacity"], td["visited"],
            td["current_node"], td["current_time"])
        tw, tw_dt = _timed(td["time_windows"])
        nat.require_device(locs, demand, used, vcap, visited, cur, time, tw)
        locs, demand, used, vcap, visited, cur, time = (
            x.contiguous() for x in (locs, demand, used, vcap, visited, cur, time))
        b, n = demand.shape
        dev = demand.device
        cur_loc = torch.empty((b, 2), dtype=torch.float32, device=dev)
        dist = torch.empty((b, n + 1), dtype=torch.float32, device=dev)
        mask = torch.empty((b, n + 1), dtype=torch.bool, device=dev)
        nat.call("co_cvrptw_action_mask", b, n, nat.ptr(locs), nat.ptr(demand), nat.ptr(used),
                 nat.ptr(vcap), nat.ptr(visited), nat.ptr(cur), nat.ptr(time), nat.ptr(tw), tw_dt,
                 nat.ptr(cur_loc), nat.ptr(dist), nat.ptr(mask), nat.stream_of(demand))
        td.update({"current_loc": cur_loc, "distances": dist})
        return mask

    _TW_MESSAGES = [
        (nat.ST_TW_NEGATIVE, AssertionError, "Time windows must be non-negative."),
        (nat.ST_TW_DEPOT_RETURN, AssertionError,
         "vehicle cannot perform service and get back to depot in time."),
        (nat.ST_DURATION_NEGATIVE, AssertionError, "Service durations must be non-negative."),
        (nat.ST_TW_INFEASIBLE, AssertionError, "there are unfeasible time windows"),
        (nat.ST_TW_DEADLINE, AssertionError, "vehicle cannot start service before deadline"),
        (nat.ST_INDEX_RANGE, RuntimeError, "index out of range in gather (actions)")]

    def _get_reward(self, td, actions, check: bool = False) -> torch.Tensor:
        """``cvrptw/env.py:167-218``: CVRP's reward; with ``check`` CVRP's validity first,
        then the time-window checks (``co_cvrptw_check``), the first failing message in the
        reference's order."""
        reward = super()._get_reward(td, actions, check=check)
        if check:
            locs = td["locs"].contiguous()
            dur, dur_dt = _timed(td["durations"])
            tw, tw_dt = _timed(td["time_windows"])
            nat.require_device(locs, actions, dur, tw)
            if actions.dtype != torch.int64:
                actions = actions.long()
            b, t = actions.shape
            status = self.status_word(locs.device)
            nat.call("co_cvrptw_check", b, locs.shape[1] - 1, t, nat.ptr(locs), nat.ptr(actions),
                     actions.stride(0), actions.stride(1), nat.ptr(dur), dur_dt, nat.ptr(tw),
                     tw_dt, nat.ptr(status), nat.stream_of(locs))
            self.raise_for_status(status, self._TW_MESSAGES)
        return reward

    def improve(self, td, actions, *args, **kwargs):
        raise NotImplementedError(
            "improve is not built for cvrptw: the CVRP local search knows no deadlines")

    @staticmethod
    def load_data(name, solomon: bool = False, path_instances: str = None, type: str = None,
                  compute_edge_weights: bool = False):
        """``cvrptw/env.py:224-244``: an npz file as a td.  Solomon files are read by
        ``vrplib`` in the reference, which is not a dependency here."""
        if solomon:
            raise NotImplementedError("Solomon instance files need vrplib, which is not a "
                                      "dependency; build the instance dict and use "
                                      "extract_from_solomon")
        return RL4COEnvBase.load_data(name)

    def extract_from_solomon(self, instance: dict, batch_size: int = 1):
        """``cvrptw/env.py:246-291``: the reset td of a Solomon instance dict
        (``node_coord``, ``demand``, ``capacity``, ``service_time``, ``time_window``);
        durations and windows are int64 there."""
        import numpy as np

        coord, demand = np.asarray(instance["node_coord"]), np.asarray(instance["demand"])
        window = np.asarray(instance["time_window"])
        self.min_demand, self.max_demand = demand[1:].min(), demand[1:].max()
        self.vehicle_capacity = instance["capacity"]
        self.min_loc, self.max_loc = coord[1:].min(), coord[1:].max()
        self.min_time, self.max_time = window[:, 0].min(), window[:, 1].max()
        assert self.min_time == 0, "Time window of depot must start at 0."
        assert self.max_time == window[0, 1], "Depot must have latest end time."

        def rows(x, dtype, *rep):
            return torch.tensor(x, dtype=dtype, device=self.device).repeat(batch_size, *rep)

        td = TensorDict({"depot": rows(coord[0], torch.float32, 1),
                         "locs": rows(coord[1:], torch.float32, 1, 1),
                         "demand": rows(demand[1:], torch.float32, 1),
                         "durations": rows(np.asarray(instance["service_time"]), torch.int64, 1),
                         "time_windows": rows(window, torch.int64, 1, 1)},
                        batch_size=[batch_size])
        return self.reset(td, batch_size=[batch_size])
