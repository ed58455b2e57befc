"""co_best_of and co_tsp_best_of on the device, through the C ABI into guarded buffers:
the same cases and assertions as tests/test_host_best_of.py (selection exact on the
kernel's own rewards against tests/best_of_ref.py, every reward within 1 f32 ulp of
co_tsp_reward, untouched guard bytes), the device's results against the host build's, and
the Python layer on device tensors."""
import numpy as np
import pytest
import torch

import best_of_cases as bc
import best_of_ref as ref
from rl4co_slap_amd import TensorDict
from rl4co_slap_amd.envs import TSPEnv
from rl4co_slap_amd.envs.base import RL4COEnvBase
from rl4co_slap_amd.utils import ops
from test_host_best_of import bc_status_cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("layout", bc.LAYOUTS)
@pytest.mark.parametrize("case", bc.CASES, ids=bc.case_id)
def test_tsp_best_of_device(dev, case, layout):
    B, K, N = case
    for mode in bc.MODES:
        allr, best, idx, rows = bc.check_tsp_case(B, K, N, layout, mode, device=dev)
        # the host build on the same case
        locs, acts, _ = bc.make_tsp_case(B, K, N, mode)
        h_all, h_best, h_idx, h_rows, _, _ = bc.run_tsp_best_of(
            locs, bc.lay_out(acts, layout), K, check=1)
        assert ref.ulp_distance(allr, h_all).max() <= 1
        assert ref.ulp_distance(best, h_best).max() <= 1
        assert np.array_equal(idx, h_idx) and np.array_equal(rows, h_rows)


@pytest.mark.parametrize("kind", bc.REWARD_KINDS)
@pytest.mark.parametrize("case", bc.CASES, ids=bc.case_id)
def test_best_of_device(dev, case, kind):
    B, K, N = case
    r = bc.make_rewards(B, K, kind)
    T = min(N, 9)
    acts = np.random.default_rng(K).integers(-5, 1 << 40, size=(K * B, T))
    want_r, want_i, want_rows = ref.best_of(r, acts, B, K)
    for layout in bc.LAYOUTS:
        best, idx, rows, intact = bc.run_best_of(r, bc.lay_out(acts, layout, dev), B, K, dev)
        assert intact
        assert np.array_equal(idx, want_i) and np.array_equal(rows, want_rows)
        assert bc.bits_equal(best, want_r)
        h_best, h_idx, h_rows, _ = bc.run_best_of(r, bc.lay_out(acts, layout), B, K)
        assert bc.bits_equal(best, h_best) and np.array_equal(idx, h_idx)
        assert np.array_equal(rows, h_rows)
    best, idx, rows, intact = bc.run_best_of(r, None, B, K, dev)
    assert intact and rows is None and np.array_equal(idx, want_i)


@pytest.mark.parametrize("check", [0, 1])
def test_status_bits_device(dev, check):
    bc_status_cases(dev, check)


def test_empty_batch_is_a_no_op(dev):
    from rl4co_slap_amd import _native as nat

    lib = nat.load()
    assert lib.co_tsp_best_of(0, 5, 3, None, None, 5, 1, 0, None, None, None, None, None,
                              None) == 0
    assert lib.co_best_of(0, 3, 5, None, None, 5, 1, None, None, None, None, None) == 0
    torch.cuda.synchronize()


def test_env_paths_on_device(dev):
    B, K, N = 5, 6, 24  # TSPEnv._best_of_fused: the fused path
    locs, acts, _ = bc.make_tsp_case(B, K, N, "random")
    env = TSPEnv(generator_params=dict(num_loc=N), device=dev)
    td = env.reset(TensorDict({"locs": torch.as_tensor(locs.copy()).to(dev)}, [B]))
    a = torch.as_tensor(acts).to(dev)
    fused = env.best_of(td, a, K)
    base = RL4COEnvBase.best_of(env, td, a, K)
    rew = env.get_reward(ops.batchify(td, K), a)
    r2, i2 = ops.unbatchify(rew, K).max(dim=1)
    rows2 = ops.gather_by_index(ops.unbatchify(a, K), i2, dim=1)
    for got in (fused, base):
        assert got[0].device == a.device
        assert torch.equal(got[1], i2) and torch.equal(got[2], rows2)
        assert ref.ulp_distance(got[0].cpu().numpy(), r2.cpu().numpy()).max() <= 1
    assert torch.equal(base[0], r2)
    step_major = a.t().contiguous().t()  # the stepwise engine's layout
    got = env.best_of(td, step_major, K)
    assert torch.equal(got[1], i2) and torch.equal(got[2], rows2)
    bad = a.clone()
    bad[0, 1] = bad[0, 0]
    with pytest.raises(AssertionError, match="Invalid tour"):
        env.best_of(td, bad, K)
