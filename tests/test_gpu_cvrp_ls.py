"""co_cvrp_local_search on the device against the numpy restatement (tests/cvrp_ls_ref.py)
and the host build: rows and sweep counts bit-equal.  The kernel runs one wavefront per row
for every size: m = 2..4 (N = 1..3) has empty or one-window strips, N = 50 at capacity 40
puts m around 60..70 on both sides of one 64-lane window, N = 56 / 57 and 100 give several
positions per lane in the load scan, N = 400 a long tour.  The distances path stages the
matrix in LDS up to N = CO_CVRP_LS_STAGE_N and reads it through L2 above, so both sides of
that cut are run.  The per-instance capacity argument is run at capacity 8 with B = 64, N =
20 and with 5 instances shared by 15 rows."""
import numpy as np
import pytest
import torch

import cvrp_ls_cases as tc
from cvrp_ls_ref import dist_from_locs, local_search
from rl4co_slap_amd import TensorDict
from rl4co_slap_amd import _native as nat
from rl4co_slap_amd.envs import CVRPEnv
from rl4co_slap_amd.utils import ops
from rl4co_slap_amd.utils.ops import batchify

pytestmark = pytest.mark.gpu

CUT = nat.CVRP_LS_STAGE_N
SHAPES = [(37, 1, 20), (37, 2, 20), (37, 3, 20), (64, 10, 20), (64, 20, 30), (16, 50, 40),
          (8, 56, 40), (8, 57, 40), (4, 100, 50)]


def _eq(got, want):
    assert np.array_equal(got[0], want[0]), "rows differ"
    assert np.array_equal(got[1], want[1]), ("sweeps differ", got[1], want[1])


@pytest.mark.parametrize("b,n,cap", SHAPES)
def test_device_equals_restatement(dev, b, n, cap):
    locs, demand, tours, ref, sweeps, _ = tc.uniform_case(b, n, cap)
    _eq(tc.run(ops.cvrp_local_search, tours, demand, locs=locs, device=dev), (ref, sweeps))


def test_long_tour_capped(dev):
    locs, demand, tours, ref, sweeps, _ = tc.uniform_case(2, 400, 50, 3)
    _eq(tc.run(ops.cvrp_local_search, tours, demand, locs=locs, device=dev, max_iterations=3),
        (ref, sweeps))
    assert (sweeps == 3).all()


@pytest.mark.parametrize("b,n,cap", [(8, 12, 20), (2, CUT, 50), (2, CUT + 1, 50)])
def test_distances_path_on_distance_matrix_output(dev, b, n, cap):
    locs, demand, tours, _, _, _ = tc.uniform_case(b, n, cap, 40)
    D = ops.get_distance_matrix(torch.as_tensor(locs.copy()).to(dev))
    ref, sweeps, _ = tc.solve(D.cpu().numpy(), demand, tours, 40)
    before = D.clone()
    out, sw = ops.cvrp_local_search(torch.as_tensor(tours.copy()).to(dev),
                                    torch.as_tensor(demand.copy()).to(dev), distances=D,
                                    max_iterations=40, return_sweeps=True)
    _eq((out.cpu().numpy(), sw.cpu().numpy()), (ref, sweeps))
    assert torch.equal(D, before) and (sweeps > 1).any()


@pytest.mark.parametrize("n", [12, 14, CUT, CUT + 1])
@pytest.mark.parametrize("symmetric", [True, False])
def test_distances_path_on_tie_matrices(dev, n, symmetric):
    b, max_it = (8 if n < 100 else 2), (1000 if symmetric else 50)
    D, demand, tours, ref, sweeps, tied = tc.int_matrix_case(b, n, symmetric, max_it)
    _eq(tc.run(ops.cvrp_local_search, tours, demand, distances=D, device=dev,
               max_iterations=max_it), (ref, sweeps))
    if symmetric:
        assert tied > 0


def test_tie_grid(dev):
    locs, demand, tours, ref, sweeps, tied = tc.grid_case()
    assert tied > 0
    _eq(tc.run(ops.cvrp_local_search, tours, demand, locs=locs, device=dev), (ref, sweeps))


@pytest.mark.parametrize("name,locs,demand,row,want,sweeps", tc.KNOWN, ids=[k[0] for k in tc.KNOWN])
def test_known_answers(dev, name, locs, demand, row, want, sweeps):
    for kw in (dict(locs=locs[None]), dict(distances=dist_from_locs(locs)[None])):
        got = tc.run(ops.cvrp_local_search, [row], [demand], device=dev, **kw)
        assert got[0].tolist() == [want] and got[1].tolist() == [sweeps]


@pytest.mark.parametrize("max_it", [0, 1, 3, 1000])
def test_max_iterations(dev, max_it):
    locs, demand, tours, ref, sweeps, _ = tc.uniform_case(16, 20, 30, max_it)
    _eq(tc.run(ops.cvrp_local_search, tours, demand, locs=locs, device=dev,
               max_iterations=max_it), (ref, sweeps))


def test_step_major_int32_and_inputs_unchanged(dev):
    locs, demand, tours, ref, sweeps, _ = tc.uniform_case(64, 20, 30)
    l, d = torch.as_tensor(locs.copy()).to(dev), torch.as_tensor(demand.copy()).to(dev)
    sm = torch.as_tensor(tours.T.copy()).to(dev)  # [T, B] storage
    view = sm.t()
    assert view.stride() == (1, 64)
    out, sw = ops.cvrp_local_search(view, d, locs=l, return_sweeps=True)
    _eq((out.cpu().numpy(), sw.cpu().numpy()), (ref, sweeps))
    assert out.is_contiguous() and out.dtype == torch.int64 and out.device == sm.device
    assert np.array_equal(sm.cpu().numpy(), tours.T) and np.array_equal(l.cpu().numpy(), locs)
    assert np.array_equal(d.cpu().numpy(), demand)
    out = ops.cvrp_local_search(torch.as_tensor(tours.astype(np.int32)).to(dev), d, locs=l)
    assert out.dtype == torch.int64 and np.array_equal(out.cpu().numpy(), ref)


def test_multistart_locs_batch_abi_and_env(dev):
    s, lb, n = 3, 5, 12
    locs, demand, tours, ref, sweeps, _ = tc.uniform_case(s * lb, n, 20, 1000, lb)
    _eq(tc.run(ops.cvrp_local_search, tours, demand, locs=locs, device=dev), (ref, sweeps))
    env = CVRPEnv(generator_params=dict(num_loc=n), device=dev)
    td = env.reset(TensorDict({"depot": torch.as_tensor(locs[:, 0].copy()).to(dev),
                               "locs": torch.as_tensor(locs[:, 1:].copy()).to(dev),
                               "demand": torch.as_tensor(demand.copy()).to(dev)}, [lb]))
    tdm = batchify(td, s)
    out, sw = env.improve(tdm, torch.as_tensor(tours.copy()).to(dev), return_sweeps=True)
    assert tdm.is_lazy("locs") and tdm.is_lazy("demand")
    _eq((out.cpu().numpy(), sw.cpu().numpy()), (ref, sweeps))


def test_capacity_argument(dev):
    """The per-instance capacity (the kernel's ``capacity[inst]`` branch and its quantised
    load bound): demands and capacity scaled by 8 (exact in f32) give the same search, with a
    [LB, 1] capacity, on one instance per row and on 5 instances shared by 15 rows."""
    for b, n, cap, lb in ((64, 20, 30, None), (15, 12, 20, 5)):
        locs, demand, tours, ref, sweeps, _ = tc.uniform_case(b, n, cap, 1000, lb)
        capacity = np.full((lb or b, 1), 8.0, dtype=np.float32)
        scaled = demand * np.float32(8)
        D = [dist_from_locs(l) for l in locs]
        want = tc.solve(D, scaled, tours, 1000, capacity[:, 0])
        _eq(want[:2], (ref, sweeps))  # the restatement itself
        _eq(tc.run(ops.cvrp_local_search, tours, scaled, locs=locs, capacity=capacity,
                   device=dev), (ref, sweeps))
        assert (sweeps > 1).any()


def test_invalid_rows_set_status_and_the_rest_is_improved(dev):
    b, n = 64, 20
    locs, demand, tours, ref, sweeps, _ = tc.uniform_case(b, n, 30)
    bad = tours.copy()
    bad[3, 1] = bad[3, 0]            # a duplicate customer
    bad[5, 0] = n + 1                # an entry out of range
    row = bad[7]
    row[np.flatnonzero(row)[2]] = 0  # a missing customer
    dem = demand.copy()
    dem[9, 4] = np.nan
    which = [3, 5, 7, 9]
    l = torch.as_tensor(locs.copy()).to(dev)
    for k in range(4):  # each kind alone sets the bit and leaves its row as it was
        one, dk = tours.copy(), demand.copy()
        one[which[k]] = bad[which[k]]
        if k == 3:
            dk[9, 4] = np.nan
        st = torch.zeros(1, dtype=torch.int32, device=dev)
        o, sw = ops.cvrp_local_search(torch.as_tensor(one).to(dev), torch.as_tensor(dk).to(dev),
                                      locs=l, return_sweeps=True, status=st)
        assert int(st.item()) == nat.ST_INVALID_TOUR
        o, sw = o.cpu().numpy(), sw.cpu().numpy()
        keep = np.arange(b) != which[k]
        assert np.array_equal(o[keep], ref[keep]) and np.array_equal(sw[keep], sweeps[keep])
        assert np.array_equal(o[~keep], one[~keep]) and (sw[~keep] == 0).all()
    t, d = torch.as_tensor(bad).to(dev), torch.as_tensor(dem).to(dev)
    with pytest.raises(AssertionError, match="Invalid tour"):
        ops.cvrp_local_search(t, d, locs=l)
    # an over-capacity but well-formed row is searched
    over = tours.copy()
    over[0] = np.concatenate([np.arange(1, 21), np.zeros(tours.shape[1] - 20, dtype=np.int64)])
    want = local_search(dist_from_locs(locs[0]), demand[0], 1.0, over[0], 1000)
    st = torch.zeros(1, dtype=torch.int32, device=dev)
    o, sw = ops.cvrp_local_search(torch.as_tensor(over).to(dev),
                                  torch.as_tensor(demand.copy()).to(dev), locs=l,
                                  return_sweeps=True, status=st)
    assert int(st.item()) == 0
    assert np.array_equal(o.cpu().numpy()[0], want[0]) and int(sw[0]) == want[1]


@pytest.mark.parametrize("b,n,cap", [(64, 20, 30), (4, 100, 50)])
def test_device_equals_host_build(dev, b, n, cap):
    locs, demand, tours, _, _, _ = tc.uniform_case(b, n, cap)
    _eq(tc.run(ops.cvrp_local_search, tours, demand, locs=locs, device=dev),
        tc.run(ops.cvrp_local_search, tours, demand, locs=locs))


def test_locs_path_equals_distances_path(dev):
    locs, demand, tours, ref, sweeps, _ = tc.uniform_case(64, 20, 30)
    l, d = torch.as_tensor(locs.copy()).to(dev), torch.as_tensor(demand.copy()).to(dev)
    t = torch.as_tensor(tours.copy()).to(dev)
    a = ops.cvrp_local_search(t, d, locs=l, return_sweeps=True)
    b = ops.cvrp_local_search(t, d, distances=ops.get_distance_matrix(l), return_sweeps=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert np.array_equal(a[0].cpu().numpy(), ref)


def test_non_default_stream(dev):
    locs, demand, tours, ref, sweeps, _ = tc.uniform_case(64, 20, 30)
    l, d = torch.as_tensor(locs.copy()).to(dev), torch.as_tensor(demand.copy()).to(dev)
    t = torch.as_tensor(tours.copy()).to(dev)
    torch.cuda.synchronize(dev)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        out, sw = ops.cvrp_local_search(t, d, locs=l, return_sweeps=True)
    stream.synchronize()
    _eq((out.cpu().numpy(), sw.cpu().numpy()), (ref, sweeps))


def test_env_improve(dev):
    b, n = 64, 20
    locs, demand, tours, ref, sweeps, _ = tc.uniform_case(b, n, 30)
    env = CVRPEnv(generator_params=dict(num_loc=n), device=dev)
    td = env.reset(TensorDict({"depot": torch.as_tensor(locs[:, 0].copy()).to(dev),
                               "locs": torch.as_tensor(locs[:, 1:].copy()).to(dev),
                               "demand": torch.as_tensor(demand.copy()).to(dev)}, [b]))
    acts = torch.as_tensor(tours.copy()).to(dev)
    before = env.get_reward(td, acts)
    out = env.improve(td, acts)
    assert out.dtype == torch.int64 and out.shape == acts.shape and out.device == acts.device
    assert np.array_equal(out.cpu().numpy(), ref)
    env.check_solution_validity(td, out)
    after = env.get_reward(td, out)
    assert (after >= before).all() and (after > before).any()
    again, sw = env.improve(td, out, return_sweeps=True)
    assert torch.equal(again, out) and (sw == 1).all()
    with pytest.raises(NotImplementedError):
        env.local_search(td, acts)
