"""The step glue's host side without a GPU (csrc/pycall/co_torchstep.cpp, _native.py): the
three ``*_step_td`` entries step aside -- None, the td untouched -- before any device call
for operands they cannot take, every entry keeps its arity error, and the Python helpers
around the glue's return convention and the status read behave as their callers expect."""
import numpy as np
import pytest
import torch

from rl4co_slap_amd import _native as nat
from rl4co_slap_amd.envs import CVRPEnv, SLAPEnv, TSPEnv
from rl4co_slap_amd.td import TensorDict

B = 3


@pytest.fixture(scope="module")
def ts():
    glue = nat.torchstep()
    if glue is None:
        pytest.skip("step glue module not built")
    return glue


def _cpu_td(name):
    """(env, its reset td of CPU tensors, the logits width)"""
    torch.manual_seed(3)
    np.random.seed(3)
    if name == "tsp":
        env = TSPEnv(generator_params=dict(num_loc=5), device="cpu", seed=3)
        width = 5
    elif name == "cvrp":
        env = CVRPEnv(generator_params=dict(num_loc=4), device="cpu", seed=3)
        width = 5
    else:
        env = SLAPEnv(generator_params=dict(n_aisles=2, n_locs=3, n_products=4), device="cpu",
                      seed=3)
        width = 6
    td = env.reset(batch_size=[B])
    assert type(td) is TensorDict and td["action_mask"].shape == (B, width)
    return env, td, width


@pytest.mark.parametrize("case", ["cpu_td", "not_a_dict", "no_action_mask", "key_not_str"])
@pytest.mark.parametrize("name", ["tsp", "cvrp", "slap"])
def test_step_td_steps_aside_before_any_device_call(ts, name, case):
    env, td, width = _cpu_td(name)
    native = env.native_decode_and_step()
    assert native is not None and native.func is getattr(ts, name + "_step_td").func
    logits = torch.zeros(B, width)
    status = torch.zeros(2, dtype=torch.int32)
    key = "action"
    arg = td
    if case == "not_a_dict":
        arg = object()
    elif case == "no_action_mask":
        dict.pop(td, "action_mask")
    elif case == "key_not_str":
        key = 5
    before = list(dict.items(td))
    assert native(arg, logits, 0, 1.0, 0.0, None, 0, 0, status, key) is None
    after = list(dict.items(td))
    assert [k for k, _ in after] == [k for k, _ in before]
    assert all(x is y for (_, x), (_, y) in zip(before, after))
    assert status.tolist() == [0, 0]


@pytest.mark.parametrize("fn, msg", [("tsp_step_td", "tsp_step_td: 12 arguments"),
                                     ("decode_step", "decode_step: 11 arguments"),
                                     ("slab_fresh", "slab_fresh: 1 argument")])
def test_wrong_arity_is_a_type_error(ts, fn, msg):
    with pytest.raises(TypeError) as e:
        getattr(ts, fn)(1, 2, 3)
    assert str(e.value) == msg


def test_glue_result():
    """An int is a C-ABI status (raised through check_rc when nonzero), anything else is
    the glue's result and comes back as it is."""
    assert nat.glue_result("co_x", 0) == 0
    with pytest.raises(RuntimeError, match="co_x failed with status 5"):
        nat.glue_result("co_x", 5)
    pair = (1, 2)
    assert nat.glue_result("co_x", pair) is pair
    assert nat.glue_result("co_x", None) is None
    assert nat.glue_result("co_x", True) is True


def test_read_status_is_one_host_read(monkeypatch):
    calls = []
    real = torch.Tensor.tolist
    monkeypatch.setattr(torch.Tensor, "tolist", lambda t: calls.append(1) or real(t))
    dev = torch.device("cpu")
    assert nat.pending_deferred(dev) is None  # the CPU never has a deferred word
    two = torch.tensor([4, 0], dtype=torch.int32)
    assert nat.read_status([two], dev) == [4, 0]
    assert len(calls) == 1
    words = [torch.tensor(7, dtype=torch.int32), torch.tensor(1, dtype=torch.int32)]
    assert nat.read_status(words, dev) == [7, 1]
    assert len(calls) == 2
    vals = nat.read_status([torch.zeros(1, dtype=torch.int32)], dev)
    assert vals == [0] and type(vals[0]) is int
