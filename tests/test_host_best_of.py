"""co_best_of and co_tsp_best_of on the host build, through the C ABI into guarded
buffers, against the numpy restatement (tests/best_of_ref.py) and co_tsp_reward; the
argument checks of both libraries (no launch, no GPU); and the Python layer on top
(``ops.best_of``, ``RL4COEnvBase.best_of``, ``TSPEnv.best_of``)."""
import numpy as np
import pytest
import torch

import best_of_cases as bc
import best_of_ref as ref
from rl4co_slap_amd import TensorDict
from rl4co_slap_amd import _native as nat
from rl4co_slap_amd.envs import CVRPEnv, TSPEnv
from rl4co_slap_amd.envs.base import RL4COEnvBase
from rl4co_slap_amd.utils import ops


def test_restatement_known_answers():
    r = np.array([1, 5, -0.0, 2, 5, 0.0], dtype=np.float32)  # K = 2, B = 3
    assert ref.select(r, 3, 2).tolist() == [1, 0, 0]
    r = np.array([1, np.nan, 3, np.nan, np.nan, 2, 9, 9, 9], dtype=np.float32)  # K = 3, B = 3
    assert ref.select(r, 3, 3).tolist() == [1, 0, 2]
    locs = np.array([[[0, 0], [3, 0], [3, 4]]], dtype=np.float32)
    assert ref.tsp_rewards(locs, np.array([[0, 1, 2], [2, 0, 1]])).tolist() == [-12.0, -12.0]
    assert ref.ulp_distance(np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(2))) == 1
    assert ref.ulp_distance(np.float32(-0.0), np.float32(0.0)) == 0


@pytest.mark.parametrize("layout", bc.LAYOUTS)
@pytest.mark.parametrize("case", bc.CASES, ids=bc.case_id)
def test_tsp_best_of_host(case, layout):
    for mode in bc.MODES:
        bc.check_tsp_case(*case, layout, mode)


@pytest.mark.parametrize("kind", bc.REWARD_KINDS)
@pytest.mark.parametrize("case", bc.CASES, ids=bc.case_id)
def test_best_of_host(case, kind):
    B, K, N = case
    r = bc.make_rewards(B, K, kind)
    T = min(N, 9)
    acts = np.random.default_rng(K).integers(-5, 1 << 40, size=(K * B, T))
    for layout in bc.LAYOUTS:
        best, idx, rows, intact = bc.run_best_of(r, bc.lay_out(acts, layout), B, K)
        want_r, want_i, want_rows = ref.best_of(r, acts, B, K)
        assert intact
        assert np.array_equal(idx, want_i) and np.array_equal(rows, want_rows)
        assert bc.bits_equal(best, want_r)
    best, idx, rows, intact = bc.run_best_of(r, None, B, K)  # no rows asked for
    assert intact and rows is None and np.array_equal(idx, ref.select(r, B, K))
    if kind.startswith("nan") and K > 1:
        assert (idx > 0).all() and np.isnan(best).all()


@pytest.mark.parametrize("check", [0, 1])
def test_status_bits_host(check):
    bc_status_cases("cpu", check)


def bc_status_cases(device, check):
    B, K, N = 3, 8, 20
    locs, acts, win = bc.make_tsp_case(B, K, N, "first")
    bad = acts.copy()
    bad[5 * B + 1, 4] = bad[5 * B + 1, 3]  # a duplicate in a losing candidate (k = 5, b = 1)
    allr, best, idx, rows, status, intact = bc.run_tsp_best_of(
        locs, bc.lay_out(bad, "rows", device), K, check=check, device=device)
    assert intact and status == (nat.ST_INVALID_TOUR if check else 0)
    assert np.array_equal(idx, win)  # the winner is not the bad row
    want = ref.best_of(allr, bad, B, K)
    assert np.array_equal(idx, want[1]) and np.array_equal(rows, want[2])
    for v in (N, -1, 1 << 33):
        oor = acts.copy()
        oor[2 * B + 0, 7] = v
        *_, status, intact = bc.run_tsp_best_of(locs, bc.lay_out(oor, "stepmajor", device), K,
                                                check=check, device=device)
        assert intact and status & nat.ST_INDEX_RANGE
        assert bool(status & nat.ST_INVALID_TOUR) == bool(check)


def abi_argument_cases(lib):
    """Every CO_E_INVAL / CO_E_ALIGN case of both entry points; none reaches a launch."""
    f32 = torch.zeros(64, dtype=torch.float32)
    i64 = torch.zeros(64, dtype=torch.int64)
    out = torch.zeros(64, dtype=torch.int64)
    st = torch.zeros(1, dtype=torch.int32)
    p, a, o, s = f32.data_ptr(), i64.data_ptr(), out.data_ptr(), st.data_ptr()

    def tsp(B=2, N=4, K=2, locs=p, acts=a, check=1, allr=p, best=p, idx=o, rows=o, status=s):
        return lib.co_tsp_best_of(B, N, K, locs, acts, N, 1, check, allr, best, idx, rows,
                                  status, None)

    INVAL, ALIGN = -1, -2
    assert tsp(B=-1) == INVAL and tsp(N=0) == INVAL and tsp(N=-3) == INVAL
    assert tsp(K=0) == INVAL and tsp(K=-1) == INVAL
    assert tsp(N=1025) == INVAL
    assert tsp(B=0, locs=None, acts=None, best=None, idx=None) == 0  # empty batch: a no-op
    assert tsp(locs=None) == INVAL and tsp(acts=None) == INVAL
    assert tsp(best=None) == INVAL and tsp(idx=None) == INVAL
    assert tsp(check=1, status=None) == INVAL
    assert tsp(rows=a) == INVAL  # best_actions aliases actions
    assert tsp(locs=p + 4) == ALIGN
    assert tsp(K=0, locs=p + 4) == INVAL  # sizes are judged first

    def sel(B=2, K=2, T=4, r=p, acts=a, best=p, idx=o, rows=o):
        return lib.co_best_of(B, K, T, r, acts, T, 1, best, idx, rows, None, None)

    assert sel(B=-1) == INVAL and sel(K=0) == INVAL and sel(K=-2) == INVAL and sel(T=-1) == INVAL
    assert sel(B=0, r=None, best=None, idx=None) == 0
    assert sel(r=None) == INVAL and sel(best=None) == INVAL and sel(idx=None) == INVAL
    assert sel(acts=None) == INVAL  # rows asked for without a source
    assert sel(rows=a) == INVAL
    assert (f32 == 0).all() and (i64 == 0).all() and (out == 0).all() and int(st) == 0


@pytest.mark.parametrize("which", ["host", "device"])
def test_argument_errors_return_codes(which):
    abi_argument_cases(nat.load_host() if which == "host" else nat.load())


def test_ops_best_of_and_env_paths():
    B, K, N = 5, 6, 24  # TSPEnv._best_of_fused: the fused path
    locs, acts, _ = bc.make_tsp_case(B, K, N, "random")
    env = TSPEnv(generator_params=dict(num_loc=N), device="cpu")
    td = env.reset(TensorDict({"locs": torch.as_tensor(locs.copy())}, [B]))
    a = torch.as_tensor(acts)
    fused = env.best_of(td, a, K)
    base = RL4COEnvBase.best_of(env, td, a, K)
    # the reference's sequence, spelled out
    rew = env.get_reward(ops.batchify(td, K), a)
    r2, i2 = ops.unbatchify(rew, K).max(dim=1)
    rows2 = ops.gather_by_index(ops.unbatchify(a, K), i2, dim=1)
    for got in (fused, base):
        assert torch.equal(got[1], i2) and torch.equal(got[2], rows2)
        assert ref.ulp_distance(got[0].numpy(), r2.numpy()).max() <= 1
    assert torch.equal(base[0], r2)
    assert torch.equal(env.best_of(td, a, (2, 3))[1], i2)  # the (num_augment, num_starts) form
    got = env.best_of(td, a, K, rewards=rew)  # rewards given: no re-scoring
    assert torch.equal(got[0], r2) and torch.equal(got[1], i2) and torch.equal(got[2], rows2)
    # a non-permutation among the losers raises as get_reward does; not with checks off
    bad = a.clone()
    bad[0, 1] = bad[0, 0]
    with pytest.raises(AssertionError, match="Invalid tour"):
        env.best_of(td, bad, K)
    TSPEnv(generator_params=dict(num_loc=N), device="cpu", check_solution=False).best_of(
        td, bad, K)
    with pytest.raises(ValueError):
        ops.best_of(rew, a, 7)
    # rows that are not tours of num_loc steps take the base path
    with pytest.raises(Exception):
        env.best_of(td, a[:, :5], K)


def test_cvrp_takes_the_composition():
    env = CVRPEnv(generator_params=dict(num_loc=6), device="cpu", check_solution=False)
    torch.manual_seed(3)
    td = env.reset(batch_size=[4])
    K = 3
    acts = torch.stack([torch.randperm(6) + 1 for _ in range(K * 4)])
    got = env.best_of(td, acts, K)
    rew = env.get_reward(ops.batchify(td, K), acts)
    r2, i2 = ops.unbatchify(rew, K).max(dim=1)
    assert torch.equal(got[0], r2) and torch.equal(got[1], i2)
    assert torch.equal(got[2], ops.gather_by_index(ops.unbatchify(acts, K), i2, dim=1))


def test_sample_n_random_actions():
    env = TSPEnv(generator_params=dict(num_loc=9), device="cpu")
    td = env.reset(batch_size=[4])
    td["action_mask"][:, 2] = False
    sel = ops.sample_n_random_actions(td, 5)
    assert sel.shape == (20,) and sel.dtype == torch.int64
    per = sel.view(5, 4)  # (n b)
    assert (per != 2).all() and ((per >= 0) & (per < 9)).all()
    for b in range(4):  # enough feasible actions: drawn without replacement
        assert per[:, b].unique().numel() == 5
    many = ops.sample_n_random_actions(td, 12).view(12, 4)  # more than feasible: with
    assert (many != 2).all()


def test_fastcall_table_has_the_entries():
    fast = nat._fastcall()
    assert fast is not None
    assert fast.table("host")["co_best_of"][1] == b"i" * 12
    assert fast.table("host")["co_tsp_best_of"][1] == b"i" * 14
