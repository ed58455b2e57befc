"""What a fused decode + env step leaves in the td, whichever tier ran it: the native
``*_step_td`` glue (csrc/pycall/co_torchstep.cpp) and the env's Python ``decode_and_step``
store the same keys in the same order, tensors of equal dtype, shape and bits, and the same
host-side records (``_co_i``, the done lower bound) on the new state tensors.  Driven
through ``DecodingStrategy.step_env_fused`` as the drop-in loop does."""
import pytest
import torch

from rl4co_slap_amd import TensorDict
from rl4co_slap_amd import _native as nat
from rl4co_slap_amd.envs import CVRPEnv, SLAPEnv, TSPEnv
from rl4co_slap_amd.utils.decoding import Evaluate, Greedy

from test_gpu_dropin_slap import _slap_instance
from test_gpu_torchstep import python_path  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

B = 33
# the keys a fused step adds to the reset td, in the order it sets them (dict order)
NEW_KEYS = {"tsp": ["action"], "cvrp": ["action", "reward"], "slap": ["action"]}


def _cvrp_data(n):
    g = torch.Generator().manual_seed(8)
    return {"depot": torch.rand(B, 2, generator=g), "locs": torch.rand(B, n, 2, generator=g),
            "demand": ((torch.rand(B, n, generator=g) * 9).int() + 1).float() / 30.0}


def _make(name, dev):
    """(env, reset td, logits width)"""
    if name == "tsp":
        data = {"locs": torch.rand(B, 12, 2, generator=torch.Generator().manual_seed(4))}
        env, width = TSPEnv(generator_params=dict(num_loc=12), device=dev), 12
    elif name == "cvrp":
        data = _cvrp_data(7)
        env, width = CVRPEnv(generator_params=dict(num_loc=7), device=dev), 8
    else:
        data = dict(_slap_instance(B, 21).items())
        env, width = SLAPEnv(device=dev), 100
    td = env.reset(TensorDict({k: v.clone().to(dev) for k, v in data.items()}, [B]))
    return env, td, width


_TABLES = {}


def _logits(width, dev):
    """One table of per-step logits per width, made once and never written."""
    if width not in _TABLES:
        _TABLES[width] = torch.randn(24, B, width,
                                     generator=torch.Generator().manual_seed(12)).to(dev)
    return _TABLES[width]


def _records(env, name, td):
    raw = lambda k: dict.get(td, k)  # noqa: E731
    if name == "tsp":
        return (env._known_i(raw("i")), env._known_lb(raw("action_mask")))
    if name == "cvrp":
        return (env._known_lb(raw("visited")),)
    return (env._known_i(raw("i")), env._known_lb(raw("i")), env._known_i(raw("done")))


def _snapshot(env, name, td):
    keys = list(dict.keys(td))
    vals = {k: v.clone() for k, v in dict.items(td) if isinstance(v, torch.Tensor)}
    return keys, vals, _records(env, name, td)


def _episode(name, dev, mode, steps, tier, monkeypatch, acts=None):
    """Steps ``steps`` fused steps (None: until every instance is done); tier "glue" must
    run every step in the native glue, tier "python" has ``native_decode_and_step``
    patched to return None.  -> (per-step snapshots, actions [T, B], td, status words)"""
    env, td, width = _make(name, dev)
    tab = _logits(width, dev)
    took = []
    if tier == "glue":
        native = env.native_decode_and_step()
        assert native is not None, "the step glue must load on the GPU box"
        counted = lambda *a: took.append(native(*a)) or took[-1]  # noqa: E731
        monkeypatch.setattr(env, "native_decode_and_step", lambda: counted)
    elif tier == "python":
        monkeypatch.setattr(env, "native_decode_and_step", lambda: None)
    strat = (Greedy if mode == "greedy" else Evaluate)(tanh_clipping=10.0)
    snaps, k = [], 0
    while k < (steps if steps is not None else tab.shape[0]):
        a = acts[k] if mode == "evaluate" else None
        out = strat.step_env_fused(tab[k], dict.get(td, "action_mask"), td, env, action=a)
        assert out is td, "the fused step must apply"
        snaps.append(_snapshot(env, name, td))
        k += 1
        if steps is None and bool(td["done"].all()):
            break
    if tier == "glue":
        assert len(took) == k and all(type(r) is tuple for r in took)
    return snaps, torch.stack(strat.actions, 0), td, strat._status


def _assert_same(a, b, name):
    (ka, va, ra), (kb, vb, rb) = a, b
    assert ka == kb and ka[-len(NEW_KEYS[name]):] == NEW_KEYS[name]
    assert ra == rb
    for k in va:
        x, y = va[k], vb[k]
        assert x.dtype == y.dtype and x.shape == y.shape, k
        assert torch.equal(x.view(torch.uint8) if x.dtype == torch.bool else
                           x.view(torch.int32) if x.dtype == torch.float32 else x,
                           y.view(torch.uint8) if y.dtype == torch.bool else
                           y.view(torch.int32) if y.dtype == torch.float32 else y), k


@pytest.fixture(scope="module")
def greedy_episodes(dev):
    """Per env: the greedy glue run taken to the end of the episode (shared, read-only)."""
    mp = pytest.MonkeyPatch()
    try:
        return {name: _episode(name, dev, "greedy", None, "glue", mp)
                for name in ("tsp", "cvrp", "slap")}
    finally:
        mp.undo()


@pytest.mark.parametrize("mode", ["greedy", "evaluate"])
@pytest.mark.parametrize("name", ["tsp", "cvrp", "slap"])
def test_glue_and_python_tier_leave_the_same_td(dev, monkeypatch, greedy_episodes, name, mode):
    full_snaps, acts, _, _ = greedy_episodes[name]
    if mode == "greedy":
        glue = full_snaps[:3]
    else:
        glue = _episode(name, dev, mode, 3, "glue", monkeypatch, acts)[0]
    py = _episode(name, dev, mode, 3, "python", monkeypatch, acts)[0]
    for a, b in zip(glue, py):
        _assert_same(a, b, name)
    assert glue[2][2][0] is not None  # the records are there to compare


@pytest.mark.parametrize("mode", ["greedy", "evaluate"])
def test_tsp_glue_and_glue_less_python_path_leave_the_same_td(dev, monkeypatch, python_path,
                                                              greedy_episodes, mode):
    """TSP with the glue module off altogether: the env's pure-Python fused step."""
    full_snaps, acts, _, _ = greedy_episodes["tsp"]
    glue = (full_snaps[:3] if mode == "greedy"
            else _episode("tsp", dev, mode, 3, "glue", monkeypatch, acts)[0])
    with python_path():
        py = _episode("tsp", dev, mode, 3, "off", monkeypatch, acts)[0]
    for a, b in zip(glue, py):
        _assert_same(a, b, "tsp")


@pytest.mark.parametrize("name", ["tsp", "cvrp", "slap"])
def test_greedy_glue_episode_ends_done_and_clean(dev, greedy_episodes, name):
    snaps, acts, td, status = greedy_episodes[name]
    torch.cuda.synchronize()
    assert bool(td["done"].all())
    assert status.tolist() == [0, 0]
    steps = {"tsp": 12, "slap": 20}.get(name)
    assert steps is None or len(snaps) == steps
    assert acts.shape == (len(snaps), B) and acts.dtype == torch.int64


def test_cvrp_unfused_step_glue_equals_python_step(dev, python_path):
    """``ts.cvrp_step`` (CVRPEnv._step's native tier) against the Python ``_step``: the six
    outputs bit for bit over two steps, and the glue's outputs distinct aligned regions."""
    ts = nat.torchstep()
    assert ts is not None
    n = 7
    a1 = torch.randint(1, n + 1, (B,), generator=torch.Generator().manual_seed(2)).to(dev)
    acts = [a1, a1 % n + 1]
    out_keys = ("used_capacity", "visited", "current_node", "done", "reward", "action_mask")

    def two_steps():
        env, td, _ = _make("cvrp", dev)
        seen = []
        for a in acts:
            td.set("action", a)
            td = env._step(td)
            seen.append({k: td[k].clone() for k in out_keys} | {"lb": env._known_lb(td["visited"])})
        return seen

    glue = two_steps()
    with python_path():
        py = two_steps()
    for g, p in zip(glue, py):
        assert g.pop("lb") == p.pop("lb") is not None
        for k in out_keys:
            assert g[k].dtype == p[k].dtype and g[k].shape == p[k].shape, k
            assert torch.equal(g[k].view(torch.uint8), p[k].view(torch.uint8)), k
    env, td, _ = _make("cvrp", dev)
    r = ts.cvrp_step(acts[0], td["demand"], td["used_capacity"], td["vehicle_capacity"],
                     td["visited"])
    assert type(r) is tuple and len(r) == 6
    ptrs = sorted(t.data_ptr() for t in r)
    assert len(set(ptrs)) == 6 and all(p % 256 == 0 for p in ptrs)
    torch.cuda.synchronize()
