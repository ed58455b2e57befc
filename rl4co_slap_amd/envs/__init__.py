"""Env registry (``rl4co/envs/__init__.py:38-83``) for the three hot-path envs, the
k-opt improvement env of TSP, the routing variants built on them, the multi-task VRP, the
pickup-and-delivery problem and the orienteering problem.

Only ``tsp``, ``cvrp`` and ``slap`` (constructive, ``ENV_REGISTRY``), ``tsp_kopt``
(improvement, ``IMPROVEMENT_ENV_REGISTRY``), ``cvrptw`` (``ROUTING_VARIANT_ENV_REGISTRY``),
``mtvrp`` (the 16 variants CVRP ... OVRPBLTW in mixed batches, ``MULTITASK_ENV_REGISTRY``)
``pdp`` (``PICKUP_DELIVERY_ENV_REGISTRY``) and ``op`` (``ORIENTEERING_ENV_REGISTRY``,
consulted last) are built MI355X-native;
asking for any other reference env raises the reference's ``ValueError``.
"""
from .base import RL4COEnvBase
from .common import Generator, get_sampler
from .cvrp import CVRPEnv, CVRPGenerator
from .cvrptw import CVRPTWEnv, CVRPTWGenerator
from .mtvrp import MTVRPEnv, MTVRPGenerator
from .op import OPEnv, OPGenerator
from .pdp import PDPEnv, PDPGenerator
from .slap import SLAPEnv, SLAPGenerator
from .tsp import TSPEnv, TSPGenerator
from .tsp_kopt import ImprovementEnvBase, TSPkoptEnv

ENV_REGISTRY = {"cvrp": CVRPEnv, "tsp": TSPEnv, "slap": SLAPEnv}
IMPROVEMENT_ENV_REGISTRY = {"tsp_kopt": TSPkoptEnv}
ROUTING_VARIANT_ENV_REGISTRY = {"cvrptw": CVRPTWEnv}
MULTITASK_ENV_REGISTRY = {"mtvrp": MTVRPEnv}
PICKUP_DELIVERY_ENV_REGISTRY = {"pdp": PDPEnv}
ORIENTEERING_ENV_REGISTRY = {"op": OPEnv}


def get_env(env_name: str, *args, **kwargs) -> RL4COEnvBase:
    env_cls = ENV_REGISTRY.get(env_name, None) or IMPROVEMENT_ENV_REGISTRY.get(env_name, None) \
        or ROUTING_VARIANT_ENV_REGISTRY.get(env_name, None) \
        or MULTITASK_ENV_REGISTRY.get(env_name, None) \
        or PICKUP_DELIVERY_ENV_REGISTRY.get(env_name, None) \
        or ORIENTEERING_ENV_REGISTRY.get(env_name, None)
    if env_cls is None:
        raise ValueError(
            f"Unknown environment {env_name}. Available environments: {ENV_REGISTRY.keys()}")
    return env_cls(*args, **kwargs)


__all__ = ["RL4COEnvBase", "Generator", "get_sampler", "TSPEnv", "TSPGenerator", "CVRPEnv",
           "CVRPGenerator", "SLAPEnv", "SLAPGenerator", "ENV_REGISTRY", "get_env",
           "ImprovementEnvBase", "TSPkoptEnv", "IMPROVEMENT_ENV_REGISTRY",
           "CVRPTWEnv", "CVRPTWGenerator", "ROUTING_VARIANT_ENV_REGISTRY",
           "MTVRPEnv", "MTVRPGenerator", "MULTITASK_ENV_REGISTRY",
           "PDPEnv", "PDPGenerator", "PICKUP_DELIVERY_ENV_REGISTRY",
           "OPEnv", "OPGenerator", "ORIENTEERING_ENV_REGISTRY"]
