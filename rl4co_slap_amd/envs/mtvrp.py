"""Multi-task VRP: env + generator on the gfx950 kernels (``rl4co/envs/routing/mtvrp/``).
Capacity plus any combination of open routes (O), backhauls (B), a route-length limit (L)
and time windows (TW); every row of a batch may be another of the 16 variants.
``include/co_env.h`` (MTVRP) states the arithmetic."""
from __future__ import annotations

from typing import Callable, Tuple, Union

import torch
from torch.distributions import Uniform

from .. import _native as nat
from ..td import TensorDict, set_many
from .base import RL4COEnvBase
from .common import Generator, get_sampler


def get_vehicle_capacity(num_loc: int) -> int:
    """``mtvrp/generator.py:16-28``: 30 + N / 5 above 20 customers (Liu et al. 2024), plus
    one per 33.3 customers above 1000 (Ye et al. 2024); the demand scaler."""
    if num_loc > 1000:
        extra_cap = 1000 // 5 + (num_loc - 1000) // 33.3
    elif num_loc > 20:
        extra_cap = num_loc // 5
    else:
        extra_cap = 0
    return 30 + extra_cap


def _variant(o, tw, l, b):
    return {"O": float(o), "TW": float(tw), "L": float(l), "B": float(b)}


# mtvrp/generator.py:31-51, in the reference's key order (available_variants slices it)
VARIANT_GENERATION_PRESETS = {
    "all": _variant(0.5, 0.5, 0.5, 0.5),
    "single_feat": _variant(0.5, 0.5, 0.5, 0.5),
    "single_feat_otw": dict(_variant(0.5, 0.5, 0.5, 0.5), OTW=0.5),
    "cvrp": _variant(0, 0, 0, 0), "ovrp": _variant(1, 0, 0, 0), "vrpb": _variant(0, 0, 0, 1),
    "vrpl": _variant(0, 0, 1, 0), "vrptw": _variant(0, 1, 0, 0), "ovrptw": _variant(1, 1, 0, 0),
    "ovrpb": _variant(1, 0, 0, 1), "ovrpl": _variant(1, 0, 1, 0), "vrpbl": _variant(0, 0, 1, 1),
    "vrpbtw": _variant(0, 1, 0, 1), "vrpltw": _variant(0, 1, 1, 0),
    "ovrpbl": _variant(1, 0, 1, 1), "ovrpbtw": _variant(1, 1, 0, 1),
    "ovrpltw": _variant(1, 1, 1, 0), "vrpbltw": _variant(0, 1, 1, 1),
    "ovrpbltw": _variant(1, 1, 1, 1),
}
_MIXED_PRESETS = ("all", "cvrp", "single_feat", "single_feat_otw")


class MTVRPGenerator(Generator):
    """``mtvrp/generator.py:54-436``: every instance is drawn with all four features and the
    features a row does not keep are then set to their neutral values (``subsample``), so a
    batch mixes variants.  On the CPU the draws and every operation are the reference's, on
    the same global stream; with ``device="cuda"`` the same torch operations draw there."""

    def __init__(self, num_loc: int = 20, min_loc: float = 0.0, max_loc: float = 1.0,
                 loc_distribution: Union[int, float, str, type, Callable] = Uniform,
                 capacity: float = None, min_demand: int = 1, max_demand: int = 10,
                 min_backhaul: int = 1, max_backhaul: int = 10, scale_demand: bool = True,
                 max_time: float = 4.6, backhaul_ratio: float = 0.2, distance_limit: float = 3.0,
                 speed: float = 1.0, prob_open: float = 0.5, prob_time_window: float = 0.5,
                 prob_limit: float = 0.5, prob_backhaul: float = 0.5, variant_preset=None,
                 use_combinations=True, subsample=True, **kwargs) -> None:
        self.num_loc, self.min_loc, self.max_loc = num_loc, min_loc, max_loc
        self.device = kwargs.get("device")
        if kwargs.get("loc_sampler", None) is not None:
            self.loc_sampler = kwargs["loc_sampler"]
        else:
            self.loc_sampler = get_sampler("loc", loc_distribution, min_loc, max_loc, **kwargs)
        if capacity is None:
            capacity = get_vehicle_capacity(num_loc)
        self.capacity = capacity
        self.min_demand, self.max_demand = min_demand, max_demand
        self.min_backhaul, self.max_backhaul = min_backhaul, max_backhaul
        self.scale_demand, self.backhaul_ratio = scale_demand, backhaul_ratio
        self.max_time, self.distance_limit, self.speed = max_time, distance_limit, speed
        assert not (subsample and (variant_preset is None)), (
            "Cannot use subsample if variant_preset is not specified. ")
        if variant_preset is not None:
            variant_probs = VARIANT_GENERATION_PRESETS.get(variant_preset)
            assert variant_probs is not None, (
                f"Variant generation preset {variant_preset} not found. Available presets are "
                f"{VARIANT_GENERATION_PRESETS.keys()} with probabilities "
                f"{VARIANT_GENERATION_PRESETS.values()}")
        else:
            variant_probs = {"O": prob_open, "TW": prob_time_window, "L": prob_limit,
                             "B": prob_backhaul}
        for key, prob in variant_probs.items():
            assert 0 <= prob <= 1, f"Probability {key} must be between 0 and 1"
        self.variant_probs, self.variant_preset = variant_probs, variant_preset
        if isinstance(variant_preset, str) and variant_preset != "all":
            use_combinations = False  # a named variant or single_feat: no feature combination
        self.use_combinations, self.subsample = use_combinations, subsample

    # -- draws ------------------------------------------------------------------
    def _uniform(self, shape, low=0.0, high=1.0):
        out = torch.empty(tuple(shape), dtype=torch.float32, device=self.device)
        return out.uniform_(low, high)

    def _rand(self, *shape):
        return torch.rand(*shape, device=self.device)

    def _generate(self, batch_size) -> TensorDict:
        dev = self.device
        locs = self.generate_locations(batch_size=batch_size, num_loc=self.num_loc)
        vehicle_capacity = torch.full((*batch_size, 1), self.capacity, dtype=torch.float32,
                                      device=dev)
        capacity_original = vehicle_capacity.clone()
        demand_linehaul, demand_backhaul = self.generate_demands(batch_size=batch_size,
                                                                 num_loc=self.num_loc)
        zero = torch.zeros(size=(*batch_size, 1), device=dev)
        demand_linehaul = torch.cat([zero, demand_linehaul], dim=1)
        demand_backhaul = torch.cat([zero, demand_backhaul], dim=1)
        open_route = self.generate_open_route(shape=(*batch_size, 1))
        speed = self.generate_speed(shape=(*batch_size, 1))
        time_windows, service_time = self.generate_time_windows(locs=locs, speed=speed)
        distance_limit = self.generate_distance_limit(shape=(*batch_size, 1), locs=locs)
        if self.scale_demand:
            demand_backhaul /= vehicle_capacity
            demand_linehaul /= vehicle_capacity
            vehicle_capacity /= vehicle_capacity
        td = TensorDict({"locs": locs, "demand_backhaul": demand_backhaul,
                         "demand_linehaul": demand_linehaul, "distance_limit": distance_limit,
                         "time_windows": time_windows, "service_time": service_time,
                         "vehicle_capacity": vehicle_capacity,
                         "capacity_original": capacity_original, "open_route": open_route,
                         "speed": speed}, batch_size=batch_size)
        return self.subsample_problems(td) if self.subsample else td

    def subsample_problems(self, td):
        """``generator.py:231-283``: a feature is removed from a row when its draw says so;
        the higher a feature's probability the likelier the row keeps it."""
        batch_size = td.batch_size[0]
        dev = self.device
        variant_probs = torch.tensor(list(self.variant_probs.values()), device=dev)
        if self.use_combinations:
            keep_mask = self._rand(batch_size, 4) >= variant_probs  # O, TW, L, B
        else:
            named = self.variant_preset in VARIANT_GENERATION_PRESETS \
                and self.variant_preset not in _MIXED_PRESETS
            cvrp_prob = 0 if named else 0.5
            if self.variant_preset in _MIXED_PRESETS:
                probs = torch.Tensor(list(self.variant_probs.values()) + [cvrp_prob])[None] \
                    .repeat(batch_size, 1)
                indices = torch.distributions.Categorical(probs.to(dev)).sample()
                rows = torch.arange(batch_size, device=dev)
                if self.variant_preset == "single_feat_otw":
                    keep_mask = torch.zeros((batch_size, 6), dtype=torch.bool, device=dev)
                    keep_mask[rows, indices] = True
                    keep_mask[:, :2] |= keep_mask[:, 4:5]  # OTW keeps both O and TW
                else:
                    keep_mask = torch.zeros((batch_size, 5), dtype=torch.bool, device=dev)
                    keep_mask[rows, indices] = True
            else:  # a named variant keeps the features of probability > 0
                keep_mask = torch.zeros((batch_size, 4), dtype=torch.bool, device=dev)
                keep_mask[:, torch.nonzero(variant_probs).squeeze()] = True
        td = self._default_open(td, ~keep_mask[:, 0])
        td = self._default_time_window(td, ~keep_mask[:, 1])
        td = self._default_distance_limit(td, ~keep_mask[:, 2])
        td = self._default_backhaul(td, ~keep_mask[:, 3])
        return td

    @staticmethod
    def _default_open(td, remove):
        td["open_route"][remove] = False
        return td

    @staticmethod
    def _default_time_window(td, remove):
        default_tw = torch.zeros_like(td["time_windows"])
        default_tw[..., 1] = float("inf")
        td["time_windows"][remove] = default_tw[remove]
        td["service_time"][remove] = torch.zeros_like(td["service_time"][remove])
        return td

    @staticmethod
    def _default_distance_limit(td, remove):
        td["distance_limit"][remove] = float("inf")
        return td

    @staticmethod
    def _default_backhaul(td, remove):
        # a backhaul customer has no linehaul demand: its pickup becomes a delivery
        td["demand_linehaul"][remove] = (td["demand_linehaul"][remove]
                                         + td["demand_backhaul"][remove])
        td["demand_backhaul"][remove] = 0
        return td

    def generate_locations(self, batch_size, num_loc) -> torch.Tensor:
        """``[B, N + 1, 2]``, the depot first."""
        return self._uniform((*batch_size, num_loc + 1, 2), self.min_loc, self.max_loc)

    def generate_demands(self, batch_size, num_loc) -> Tuple[torch.Tensor, torch.Tensor]:
        """Integer demands 1..10 as in Kool et al. (2019), each customer either a linehaul
        (delivery) or, with ``backhaul_ratio``, a backhaul (pickup): ``[B, N]`` each."""
        linehaul = (self._uniform((*batch_size, num_loc), self.min_demand - 1,
                                  self.max_demand - 1).int() + 1).float()
        backhaul = (self._uniform((*batch_size, num_loc), self.min_backhaul - 1,
                                  self.max_backhaul - 1).int() + 1).float()
        is_linehaul = self._rand(*batch_size, num_loc) > self.backhaul_ratio
        return linehaul * is_linehaul, backhaul * ~is_linehaul

    def generate_time_windows(self, locs, speed):
        """``generator.py:354-396`` (Liu et al. 2024): service times in [0.15, 0.18], window
        lengths in [0.18, 0.2], starts such that the depot is reached again by ``max_time``;
        the depot's window is ``[0, max_time]`` and its service time 0."""
        batch_size, n_loc = locs.shape[0], locs.shape[1] - 1
        dev = self.device
        a, b, c = 0.15, 0.18, 0.2
        service_time = a + (b - a) * self._rand(batch_size, n_loc)
        tw_length = b + (c - b) * self._rand(batch_size, n_loc)
        d_0i = (locs[:, 0:1] - locs[:, 1:]).norm(p=2, dim=-1)
        h_max = (self.max_time - service_time - tw_length) / d_0i * speed - 1
        tw_start = (1 + (h_max - 1) * self._rand(batch_size, n_loc)) * d_0i / speed
        tw_end = tw_start + tw_length
        time_windows = torch.stack(
            (torch.cat((torch.zeros(batch_size, 1, device=dev), tw_start), -1),
             torch.cat((torch.full((batch_size, 1), self.max_time, device=dev), tw_end), -1)),
            dim=-1)
        service_time = torch.cat((torch.zeros(batch_size, 1, device=dev), service_time), dim=-1)
        return time_windows, service_time

    def generate_distance_limit(self, shape, locs) -> torch.Tensor:
        dist_to_depot = torch.cdist(locs, locs[:, 0:1, :], p=2)
        assert (dist_to_depot * 2 < self.distance_limit).all(), (
            "Distance limit too low, not all nodes can be reached from the depot.")
        return torch.full(shape, self.distance_limit, dtype=torch.float32, device=self.device)

    def generate_open_route(self, shape):
        return torch.ones(shape, dtype=torch.bool, device=self.device)

    def generate_speed(self, shape):
        return torch.full(shape, self.speed, dtype=torch.float32, device=self.device)

    @staticmethod
    def save_data(td, path, compress: bool = False):
        import numpy as np

        save = np.savez_compressed if compress else np.savez
        save(path, **{k: td[k].cpu().numpy() for k in td.keys()})

    @staticmethod
    def print_presets():
        for key, value in VARIANT_GENERATION_PRESETS.items():
            print(f"{key}: {value}")

    @staticmethod
    def available_variants(*args, **kwargs):
        return list(VARIANT_GENERATION_PRESETS.keys())[3:]  # without all / single_feat(_otw)


_INSTANCE = ("locs", "time_windows", "service_time", "demand_linehaul", "demand_backhaul",
             "vehicle_capacity", "speed", "distance_limit", "open_route")
_STATE = ("current_node", "current_time", "current_route_length", "used_capacity_linehaul",
          "used_capacity_backhaul", "visited")


def _f32c(x):
    return (x if x.dtype == torch.float32 else x.float()).contiguous()


def _instance(td):
    """The td's instance tensors as the MTVRP entries take them: f32 and contiguous, the
    open-route flags as bytes."""
    out = [_f32c(td[k]) for k in _INSTANCE[:-1]]
    opened = td["open_route"]
    out.append((opened if opened.dtype in (torch.bool, torch.uint8) else opened != 0).contiguous())
    nat.require_device(*out)
    return out


def _state(td):
    cur, vis = td["current_node"], td["visited"]
    out = [(cur if cur.dtype == torch.int64 else cur.long()).contiguous()]
    out += [_f32c(td[k]) for k in _STATE[1:-1]]
    out.append((vis if vis.dtype in (torch.bool, torch.uint8) else vis != 0).contiguous())
    nat.require_device(*out)
    return out


class MTVRPEnv(RL4COEnvBase):
    """``mtvrp/env.py:23-503``.  One launch per reset / step (update + mask) /
    ``get_action_mask``; ``step_many`` runs preset steps in one launch.  The decode loop
    takes the two-call path (``co_decode_step``, then this env's step)."""

    name = "mtvrp"
    decode_and_step = None

    def __init__(self, generator: MTVRPGenerator = None, generator_params: dict = {},
                 check_solution: bool = False, **kwargs):
        super().__init__(check_solution=check_solution, **kwargs)
        self.generator = generator if generator is not None else MTVRPGenerator(**generator_params)

    def native_decode_and_step(self):
        return None

    def _reset(self, td=None, batch_size=None) -> TensorDict:
        """``mtvrp/env.py:164-209`` in one ``co_mtvrp_reset`` launch."""
        inst = _instance(td)
        locs = inst[0]
        b, nc = locs.shape[0], locs.shape[1]
        dev = locs.device
        cur = torch.empty((b,), dtype=torch.int64, device=dev)
        time, rlen, used_l, used_b = (torch.empty((b, 1), dtype=torch.float32, device=dev)
                                      for _ in range(4))
        visited = torch.empty((b, nc), dtype=torch.bool, device=dev)
        mask = torch.empty((b, nc), dtype=torch.bool, device=dev)
        table = nat.mtvrp_instance(*inst)
        nat.call("co_mtvrp_reset", b, nc - 1, table.address, nat.ptr(cur),
                 nat.ptr(time), nat.ptr(rlen), nat.ptr(used_l), nat.ptr(used_b),
                 nat.ptr(visited), nat.ptr(mask), nat.stream_of(locs))
        out = {k: td[k] for k in ("locs", "demand_backhaul", "demand_linehaul", "distance_limit",
                                  "service_time", "open_route", "time_windows",
                                  "vehicle_capacity", "capacity_original", "speed")}
        out.update({"current_node": cur, "current_route_length": rlen, "current_time": time,
                    "used_capacity_backhaul": used_b, "used_capacity_linehaul": used_l,
                    "visited": visited, "action_mask": mask})
        return TensorDict(out, batch_size=batch_size)

    def _step(self, td: TensorDict) -> TensorDict:
        """``mtvrp/env.py:100-162`` + ``get_action_mask`` in one ``co_mtvrp_step`` launch;
        every output is a fresh tensor."""
        inst, state = _instance(td), _state(td)
        action = td["action"]
        nat.require_device(action)
        action = (action if action.dtype == torch.int64 else action.long()).contiguous()
        locs = inst[0]
        b, nc = locs.shape[0], locs.shape[1]
        dev, s = locs.device, nat.stream_of(locs)
        cur = self._out((b,), torch.int64, dev, s)
        time, rlen, used_l, used_b = (self._out((b, 1), torch.float32, dev, s) for _ in range(4))
        visited = self._out((b, nc), torch.bool, dev, s)
        done = self._out((b,), torch.bool, dev, s)
        reward = self._out((b,), torch.float32, dev, s)
        mask = self._out((b, nc), torch.bool, dev, s)
        table = nat.mtvrp_instance(*inst)
        nat.call("co_mtvrp_step", b, nc - 1, nat.ptr(action), table.address,
                 *(nat.ptr(x) for x in state), nat.ptr(cur), nat.ptr(time), nat.ptr(rlen),
                 nat.ptr(used_l), nat.ptr(used_b), nat.ptr(visited), nat.ptr(done),
                 nat.ptr(reward), nat.ptr(mask), None, None, s)
        set_many(td, {"current_node": cur, "current_route_length": rlen, "current_time": time,
                      "done": done, "reward": reward, "used_capacity_linehaul": used_l,
                      "used_capacity_backhaul": used_b, "visited": visited,
                      "action_mask": mask})
        return td

    def step_many(self, td, actions, step_major: bool = False):
        """T preset steps in one ``co_mtvrp_steps`` launch: ``actions`` is ``[B, T]`` (a
        rollout's layout) or, with ``step_major``, ``[T, B]``; any strides.  Leaves ``td`` as
        the T ``step`` calls would, bit for bit, in fresh tensors, and returns ``(feasible,
        time, route_length)``, each ``[T, B]``: whether ``action_mask[b, a_t]`` held before
        step t, and ``current_time`` / ``current_route_length`` after it.  An action outside
        ``0..N`` raises."""
        inst, state = _instance(td), _state(td)
        nat.require_device(actions)
        if actions.dtype != torch.int64:
            actions = actions.long()
        locs = inst[0]
        b, nc = locs.shape[0], locs.shape[1]
        if actions.dim() != 2 or actions.shape[0 if not step_major else 1] != b:
            raise ValueError(f"actions must be [{b}, T] (or [T, {b}] with step_major), got "
                             f"{tuple(actions.shape)}")
        if not step_major:
            actions = actions.t()
        t = actions.shape[0]
        if t == 0:
            raise ValueError("step_many needs at least one step")
        dev = locs.device
        state = [x.clone() for x in state]
        done = torch.empty(b, dtype=torch.bool, device=dev)
        reward = torch.empty(b, dtype=torch.float32, device=dev)
        mask = torch.empty((b, nc), dtype=torch.bool, device=dev)
        feasible = torch.empty((t, b), dtype=torch.bool, device=dev)
        times = torch.empty((t, b), dtype=torch.float32, device=dev)
        lengths = torch.empty((t, b), dtype=torch.float32, device=dev)
        status = self.status_word(dev)
        table = nat.mtvrp_instance(*inst)
        nat.call("co_mtvrp_steps", b, nc - 1, t, nat.ptr(actions), actions.stride(0),
                 actions.stride(1), table.address, *(nat.ptr(x) for x in state),
                 nat.ptr(done), nat.ptr(reward), nat.ptr(mask), nat.ptr(feasible),
                 nat.ptr(times), nat.ptr(lengths), nat.ptr(status), None, nat.stream_of(locs))
        self.raise_for_status(status, [(nat.ST_INDEX_RANGE, RuntimeError,
                                        "index out of range in step_many (actions)")])
        cur, time, rlen, used_l, used_b, visited = state
        set_many(td, {"action": actions[-1], "current_node": cur, "current_route_length": rlen,
                      "current_time": time, "done": done, "reward": reward,
                      "used_capacity_linehaul": used_l, "used_capacity_backhaul": used_b,
                      "visited": visited, "action_mask": mask})
        return feasible, times, lengths

    @staticmethod
    def get_action_mask(td: TensorDict) -> torch.Tensor:
        """``mtvrp/env.py:212-279`` in one ``co_mtvrp_action_mask`` launch."""
        inst, state = _instance(td), _state(td)
        locs = inst[0]
        b, nc = locs.shape[0], locs.shape[1]
        mask = torch.empty((b, nc), dtype=torch.bool, device=locs.device)
        table = nat.mtvrp_instance(*inst)
        nat.call("co_mtvrp_action_mask", b, nc - 1, table.address,
                 *(nat.ptr(x) for x in state), nat.ptr(mask), nat.stream_of(locs))
        return mask

    _MESSAGES = [
        (nat.ST_INVALID_TOUR, AssertionError, "Invalid tour"),
        (nat.ST_MT_LIMIT_NEGATIVE, AssertionError, "Distance limits must be non-negative."),
        (nat.ST_MT_TW_NEGATIVE, AssertionError, "Time windows must be non-negative."),
        (nat.ST_MT_SERVICE_NEGATIVE, AssertionError, "Service time must be non-negative."),
        (nat.ST_MT_TW_INFEASIBLE, AssertionError, "there are unfeasible time windows"),
        (nat.ST_MT_DEPOT_RETURN, AssertionError,
         "vehicle cannot perform service and get back to depot in time."),
        (nat.ST_MT_ROUTE_LIMIT, AssertionError, "Route exceeds distance limit"),
        (nat.ST_MT_DEADLINE, AssertionError, "vehicle cannot start service before deadline"),
        (nat.ST_MT_OVER_LINEHAUL, AssertionError, "Used more than capacity for demand_linehaul"),
        (nat.ST_MT_OVER_BACKHAUL, AssertionError, "Used more than capacity for demand_backhaul"),
        (nat.ST_INDEX_RANGE, RuntimeError, "index out of range in gather (actions)")]

    @staticmethod
    def _actions(actions):
        nat.require_device(actions)
        if actions.dim() != 2:
            raise ValueError(f"actions must be [B, T], got {tuple(actions.shape)}")
        return actions if actions.dtype == torch.int64 else actions.long()

    def check_solution_validity(self, td, actions):
        """``mtvrp/env.py:294-365`` in one ``co_mtvrp_check`` launch: the first failing
        message in the reference's order (the capacity messages end at the feature name)."""
        inst = _instance(td)
        locs, table = inst[0], nat.mtvrp_instance(*inst)
        actions = self._actions(actions)
        b, t = actions.shape
        status = self.status_word(locs.device)
        nat.call("co_mtvrp_check", b, locs.shape[1] - 1, t, table.address, nat.ptr(actions),
                 actions.stride(0), actions.stride(1), nat.ptr(status), nat.stream_of(locs))
        self.raise_for_status(status, self._MESSAGES)

    def _get_reward(self, td, actions, check: bool = False) -> torch.Tensor:
        """``mtvrp/env.py:281-291``: minus the tour length, a leg back to the depot not
        counted on an open row; with ``check`` the validity checks first."""
        if check:
            self.check_solution_validity(td, actions)
        locs = _f32c(td["locs"])
        opened = td["open_route"]
        opened = (opened if opened.dtype in (torch.bool, torch.uint8) else opened != 0).contiguous()
        nat.require_device(locs, opened)
        actions = self._actions(actions)
        b, t = actions.shape
        reward = torch.empty(b, dtype=torch.float32, device=locs.device)
        status = self.status_word(locs.device)
        nat.call("co_mtvrp_reward", b, locs.shape[1] - 1, t, nat.ptr(locs), nat.ptr(actions),
                 actions.stride(0), actions.stride(1), nat.ptr(opened), nat.ptr(reward),
                 nat.ptr(status), nat.stream_of(locs))
        self.raise_for_status(status, [(nat.ST_INDEX_RANGE, RuntimeError,
                                        "index out of range in gather (actions)")])
        return reward

    def select_start_nodes(self, td, num_starts):
        """``mtvrp/env.py:390-398``: ``num_loc`` from the td, not from the generator."""
        num_loc = td["locs"].shape[-2] - 1
        return torch.arange(num_starts, device=td.device).repeat_interleave(td.shape[0]) \
            % num_loc + 1

    @staticmethod
    def check_variants(td):
        """``mtvrp/env.py:466-473``: per row, which features the instance has."""
        has_open = td["open_route"].squeeze(-1)
        has_tw = (td["time_windows"][:, :, 1] != float("inf")).any(-1)
        has_limit = (td["distance_limit"] != float("inf")).squeeze(-1)
        has_backhaul = (td["demand_backhaul"] != 0).any(-1)
        return has_open, has_tw, has_limit, has_backhaul

    @staticmethod
    def get_variant_names(td):
        """``mtvrp/env.py:475-500``: CVRP, or [O]VRP[B][L][TW], per row."""
        flags = [f.cpu().tolist() for f in MTVRPEnv.check_variants(td)]
        names = []
        for o, tw, l_, b in zip(*flags):
            if not (o or b or l_ or tw):
                names.append("CVRP")
            else:
                names.append(("O" if o else "") + "VRP" + ("B" if b else "") + ("L" if l_ else "")
                             + ("TW" if tw else ""))
        return names

    def print_presets(self):
        self.generator.print_presets()

    def load_data(self, fpath, batch_size=[], scale=False):
        """``mtvrp/env.py:367-381``: an npz file as a td; ``scale`` divides the demands by
        ``capacity_original``."""
        td = RL4COEnvBase.load_data(fpath, batch_size)
        if scale:
            td.set("demand_linehaul", td["demand_linehaul"] / td["capacity_original"])
            td.set("demand_backhaul", td["demand_backhaul"] / td["capacity_original"])
        return td

    def improve(self, td, actions, *args, **kwargs):
        raise NotImplementedError("improve is not built for mtvrp: the CVRP local search knows "
                                  "no backhauls, limits or deadlines")

    @staticmethod
    def solve(instances, max_runtime, num_procs: int = 1, solver: str = "pyvrp", **kwargs):
        raise NotImplementedError("solve is not built for mtvrp: PyVRP, OR-Tools and LKH are "
                                  "not dependencies")
