"""Loader for the reference's own modules -- TEST INFRASTRUCTURE ONLY.

``load()`` imports a handful of modules of the reference checkout (``rl4co``) in a process
that has none of its dependencies: ``tensordict``, ``torchrl``, ``lightning`` and ``numba``
are replaced by the small stand-ins below, written for this project, and the ``rl4co``
packages are empty modules whose ``__path__`` points into the checkout, so submodules load
from there and no ``__init__.py`` of the reference runs.  Nothing of the reference is copied
here; ``oracle/record_reference.py`` calls the loaded functions and stores what they return.

The checkout is found through ``$RL4CO_REFERENCE`` (default ``/root/reference``).

A module named ``tensordict`` in ``sys.modules`` would change how ``rl4co_slap_amd`` behaves
(it uses the real one when present), so this loader refuses to run next to the product and
must only be used in a process of its own: never import it from a test.
"""
from __future__ import annotations

import importlib
import os
import sys
import types

import torch

from .td import TD

ENV_VAR = "RL4CO_REFERENCE"
DEFAULT_PATH = "/root/reference"

MODULES = (
    "rl4co.utils.ops",
    "rl4co.envs.common.base",
    "rl4co.utils.decoding",
    "rl4co.data.transforms",
    "rl4co.envs.routing.tsp.generator",
    "rl4co.envs.routing.tsp.local_search",
    "rl4co.envs.routing.tsp.env",
    "rl4co.envs.routing.cvrp.generator",
    "rl4co.envs.routing.cvrp.env",
    "rl4co.envs.warehousing.slap.generator",
    "rl4co.envs.warehousing.slap.env",
)

PACKAGES = (
    "rl4co", "rl4co.utils", "rl4co.data", "rl4co.envs", "rl4co.envs.common",
    "rl4co.envs.routing", "rl4co.envs.routing.tsp", "rl4co.envs.routing.cvrp",
    "rl4co.envs.warehousing", "rl4co.envs.warehousing.slap", "rl4co.models",
    "rl4co.models.rl", "rl4co.models.rl.common", "rl4co.models.rl.reinforce",
)


def reference_path():
    return os.environ.get(ENV_VAR, DEFAULT_PATH)


def available():
    return os.path.isfile(os.path.join(reference_path(), "rl4co", "utils", "ops.py"))


# ---------------------------------------------------------------------------
# stand-ins
# ---------------------------------------------------------------------------
class TensorDict(TD):
    """``oracle.td.TD`` with the constructor and the few tensor-like methods the loaded
    modules use on a TensorDict (``shape``, ``get`` with a default, row indexing and the
    ``expand`` / ``contiguous`` / ``view`` / ``permute`` chain of ``batchify``)."""

    def __init__(self, source=None, batch_size=(), device=None, **unused):
        super().__init__(source, batch_size if batch_size is not None else ())

    @property
    def shape(self):
        return self.batch_size

    def _map(self, fn, batch_size):
        return TensorDict({k: fn(v) for k, v in self.items()}, batch_size)

    def __getitem__(self, key):
        if isinstance(key, str):
            return dict.__getitem__(self, key)
        probe = torch.empty(self.batch_size)[key]
        return self._map(lambda v: v[key], probe.shape)

    def clone(self):
        return self._map(lambda v: v.clone(), self.batch_size)

    def to(self, *unused, **unused_kw):
        return self

    def expand(self, *shape):
        nb = len(self.batch_size)
        return self._map(lambda v: v.expand(*shape, *v.shape[nb:]), shape)

    def contiguous(self):
        return self._map(lambda v: v.contiguous(), self.batch_size)

    def view(self, *shape):
        nb = len(self.batch_size)
        return self._map(lambda v: v.reshape(*shape, *v.shape[nb:]), shape)

    def permute(self, *dims):
        nb = len(self.batch_size)
        dims = dims[:nb]
        shape = [self.batch_size[d] for d in dims]
        return self._map(lambda v: v.permute(*dims, *range(nb, v.dim())), shape)


class EnvBase:
    """The part of TorchRL's ``EnvBase`` the reference's envs touch: the constructor
    arguments, ``set_seed`` -> ``_set_seed``, ``to`` and the ``reset`` merge described in
    ``oracle/td.py``."""

    def __init__(self, device="cpu", batch_size=None, **unused):
        self.device = device
        self.batch_size = torch.Size(batch_size if batch_size is not None else ())

    def set_seed(self, seed=None):
        self._set_seed(seed)
        return seed

    def to(self, device):
        return self

    def reset(self, td=None, batch_size=None):
        out = self._reset(td, batch_size=batch_size)
        td.update(out)
        for key in ("done", "terminated"):
            if key not in td:
                td[key] = torch.zeros((*batch_size, 1), dtype=torch.bool)
        return td


class _Anything:
    """A spec class: accepts any arguments, indexing and calls."""

    def __init__(self, *args, **kwargs):
        pass

    def __call__(self, *args, **kwargs):
        return self

    def __getitem__(self, item):
        return self

    def __class_getitem__(cls, item):
        return cls


def _njit(*args, **kwargs):
    if len(args) == 1 and callable(args[0]) and not isinstance(args[0], _Anything) and not kwargs:
        return args[0]
    return lambda fn: fn


def _module(name, **attrs):
    mod = types.ModuleType(name)
    mod.__dict__.update(attrs)
    sys.modules[name] = mod
    parent, _, leaf = name.rpartition(".")
    if parent and parent in sys.modules:
        setattr(sys.modules[parent], leaf, mod)
    return mod


def _unavailable(*args, **kwargs):
    raise RuntimeError("not available in the reference loader")


def _install(root):
    _module("tensordict", TensorDict=TensorDict)
    _module("tensordict.tensordict", TensorDict=TensorDict)
    _module("torchrl")
    _module("torchrl.envs", EnvBase=EnvBase)
    _module("torchrl.data", **{n: _Anything for n in (
        "BoundedTensorSpec", "CompositeSpec", "UnboundedContinuousTensorSpec",
        "UnboundedDiscreteTensorSpec")})
    for name in ("lightning", "lightning.pytorch", "lightning.pytorch.utilities"):
        _module(name)
    _module("lightning.pytorch.utilities.rank_zero", rank_zero_only=lambda fn: fn)
    anything = _Anything()
    _module("numba", njit=_njit, float32=anything, uint16=anything, int64=anything)
    for name in PACKAGES:
        _module(name).__path__ = [os.path.join(root, *name.split("."))]
    _module("rl4co.data.dataset", TensorDictDataset=_Anything)
    _module("rl4co.data.utils", load_npz_to_tensordict=_unavailable)
    _module("rl4co.envs.routing.tsp.render", render=_unavailable, render_improvement=_unavailable)
    _module("rl4co.envs.routing.cvrp.render", render=_unavailable)
    _module("rl4co.models.rl.common.critic", CriticNetwork=_Anything,
            create_critic_from_actor=_unavailable)


def load():
    """Install the stand-ins and import the reference modules; returns ``{dotted name:
    module}``.  Raises when the product is already imported in this process."""
    if "rl4co_slap_amd" in sys.modules:
        raise RuntimeError("oracle.reference must run in a process of its own: rl4co_slap_amd "
                           "is imported here and would see the stand-in tensordict")
    for name in ("tensordict", "torchrl", "rl4co"):
        if name in sys.modules:
            raise RuntimeError(f"{name} is already imported in this process")
    root = reference_path()
    if not available():
        raise FileNotFoundError(f"no reference checkout at {root!r} (set ${ENV_VAR})")
    _install(root)
    out = {}
    for name in MODULES:
        out[name] = importlib.import_module(name)
        if name == "rl4co.envs.common.base":  # ``from rl4co.envs import RL4COEnvBase``
            sys.modules["rl4co.envs"].RL4COEnvBase = out[name].RL4COEnvBase
    return out


def load_pomo():
    """The reference's ``baselines``, ``reinforce`` and ``RewardScaler`` modules after
    ``load()``, with the Lightning module they build on replaced by an empty class; ``None``
    when they do not import with these stand-ins."""
    for name in ("lightning.fabric", "lightning.fabric.utilities", "lightning.pytorch.core"):
        _module(name)
    _module("lightning.fabric.utilities.types", _MAP_LOCATION_TYPE=object, _PATH=object)
    _module("lightning.pytorch.core.saving", _load_from_checkpoint=_unavailable)
    _module("rl4co.models.rl.common.base", RL4COLitModule=_Anything)
    _module("rl4co.utils.lightning", get_lightning_device=_unavailable)
    try:
        return tuple(importlib.import_module("rl4co.models.rl." + name) for name in (
            "reinforce.baselines", "reinforce.reinforce", "common.utils"))
    except Exception:  # noqa: BLE001 - any missing dependency of the reference
        return None
