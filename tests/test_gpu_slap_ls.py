"""co_slap_local_search on the device against the numpy restatement (tests/slap_ls_ref.py)
and the host build: rows, sweep counts and costs bit-equal.  The kernel runs one wavefront
per row: P = 1 and 2 have no or few candidates, P = 63 / L = 64 swaps only, P = 64 / 65 sit
on either side of one 64-lane pass of the swap square, L = 130 and 1024 need several passes
over the slots, P = 128 is the widest flow matrix.  Where CO_SLAP_LS_TABLE_FITS(P, L) the
table scheme runs and anywhere else the direct scheme: both sides of that cut are run at two
P, and the two schemes against each other on the same inputs."""
import numpy as np
import pytest
import torch

import slap_ls_cases as tc
from slap_ls_ref import dist_from_locs
from rl4co_slap_amd import TensorDict
from rl4co_slap_amd import _native as nat
from rl4co_slap_amd.envs import SLAPEnv
from rl4co_slap_amd.utils import ops
from rl4co_slap_amd.utils.ops import batchify

pytestmark = pytest.mark.gpu


def _eq(got, want):
    assert np.array_equal(got[0], want[0]), "rows differ"
    assert np.array_equal(got[1], want[1]), ("sweeps differ", got[1], want[1])
    assert np.array_equal(got[2], want[2]), ("costs differ", got[2], want[2])


@pytest.mark.parametrize("b,p,L,o,k,max_it", tc.SHAPES)
def test_device_equals_restatement(dev, b, p, L, o, k, max_it):
    locs, pl, rows, ref, sweeps, cost, _ = tc.coords_case(b, p, L, o, k, max_it, None, L == 100)
    _eq(tc.run(ops.slap_local_search, rows, pl, locs=locs, device=dev, max_iterations=max_it),
        (ref, sweeps, cost))


@pytest.mark.parametrize("b,p,L,o,k", [(37, 2, 3, 2, 2), (64, 5, 8, 4, 3), (16, 20, 100, 20, 5),
                                       (8, 63, 64, 20, 5)])
def test_direct_scheme_equals_table_scheme(dev, b, p, L, o, k):
    """The shapes the table scheme takes by default, with the direct scheme forced."""
    assert nat.slap_ls_table_fits(p, L)
    locs, pl, rows, ref, sweeps, cost, _ = tc.coords_case(b, p, L, o, k, 1000, None, L == 100)
    for scheme in (nat.SLAP_LS_DIRECT, nat.SLAP_LS_TABLE):
        _eq(tc.run(ops.slap_local_search, rows, pl, locs=locs, device=dev, scheme=scheme),
            (ref, sweeps, cost))


@pytest.mark.parametrize("p,L", tc.CUT_SHAPES)
def test_both_sides_of_the_cut(dev, p, L):
    """(32, 239) and (50, 147) are the last table shapes at their P, (32, 240) and (50, 148)
    the first direct ones, on both distance sources; the table shapes also run with the
    direct scheme forced.  At (50, 147) the table update's last pass owns columns on 19
    lanes only, fewer than there are rows whose coefficients are broadcast from lanes."""
    fits = nat.slap_ls_table_fits(p, L)
    assert fits == (L in (239, 147))
    locs, pl, rows, ref, sweeps, cost, _ = tc.coords_case(2, p, L, 20, 5, 30)
    _eq(tc.run(ops.slap_local_search, rows, pl, locs=locs, device=dev, max_iterations=30),
        (ref, sweeps, cost))
    D, pl, rows, ref, sweeps, cost, _ = tc.matrix_case(2, p, L, 20, 5, 30)
    _eq(tc.run(ops.slap_local_search, rows, pl, distances=D, device=dev, max_iterations=30),
        (ref, sweeps, cost))
    if fits:
        _eq(tc.run(ops.slap_local_search, rows, pl, distances=D, device=dev, max_iterations=30,
                   scheme=nat.SLAP_LS_DIRECT), (ref, sweeps, cost))
    else:
        st = torch.zeros(1, dtype=torch.int32, device=dev)
        with pytest.raises(ValueError, match="LDS budget"):
            ops.slap_local_search(torch.as_tensor(rows.copy()).to(dev),
                                  torch.as_tensor(pl.copy()).to(dev),
                                  distances=torch.as_tensor(D.copy()).to(dev), status=st,
                                  scheme=nat.SLAP_LS_TABLE)


@pytest.mark.parametrize("symmetric", [True, False])
def test_ties_follow_the_rule(dev, symmetric):
    D, pl, rows, ref, sweeps, cost, tied = tc.int_matrix_case(8, symmetric)
    assert tied > 0
    for scheme in (nat.SLAP_LS_AUTO, nat.SLAP_LS_DIRECT):
        _eq(tc.run(ops.slap_local_search, rows, pl, distances=D, device=dev, scheme=scheme),
            (ref, sweeps, cost))


def test_asymmetric_matrix(dev):
    D, pl, rows, ref, sweeps, cost, _ = tc.matrix_case(8, 12, 20, 10, 4)
    _eq(tc.run(ops.slap_local_search, rows, pl, distances=D, device=dev), (ref, sweeps, cost))


def test_distances_path_on_distance_matrix_output(dev):
    locs, pl, rows, ref, sweeps, cost, _ = tc.coords_case(16, 20, 100, 20, 5, 1000, None, True)
    D = ops.get_distance_matrix(torch.as_tensor(locs.copy()).to(dev))
    before = D.clone()
    _eq(tc.run(ops.slap_local_search, rows, pl, distances=D.cpu().numpy(), device=dev),
        (ref, sweeps, cost))
    out = ops.slap_local_search(torch.as_tensor(rows.copy()).to(dev),
                                torch.as_tensor(pl.copy()).to(dev), distances=D)
    assert np.array_equal(out.cpu().numpy(), ref) and torch.equal(D, before)


@pytest.mark.parametrize("name,locs,pl,row,want,sweeps,cost", tc.KNOWN, ids=[k[0] for k in tc.KNOWN])
def test_known_answers(dev, name, locs, pl, row, want, sweeps, cost):
    for kw in (dict(locs=locs[None]), dict(distances=dist_from_locs(locs)[None])):
        for scheme in (nat.SLAP_LS_AUTO, nat.SLAP_LS_DIRECT):
            got = tc.run(ops.slap_local_search, [row], [pl], device=dev, scheme=scheme, **kw)
            assert got[0].tolist() == [want] and got[1].tolist() == [sweeps]
            assert got[2].tolist() == [cost]


@pytest.mark.parametrize("max_it", [0, 1, 3, 2 ** 40])
def test_max_iterations(dev, max_it):
    locs, pl, rows, ref, sweeps, cost, _ = tc.coords_case(16, 20, 100, 20, 5, min(max_it, 1000),
                                                          None, True)
    _eq(tc.run(ops.slap_local_search, rows, pl, locs=locs, device=dev, max_iterations=max_it),
        (ref, sweeps, cost))


def test_dtypes_strides_and_inputs_unchanged(dev):
    locs, pl, rows, ref, sweeps, cost, _ = tc.coords_case(64, 5, 8, 4, 3)
    l, p = torch.as_tensor(locs.copy()).to(dev), torch.as_tensor(pl.copy()).to(dev)
    wide = torch.zeros(64, 10, dtype=torch.int64, device=dev)
    wide[:, ::2] = torch.as_tensor(rows.copy()).long().to(dev)
    view = wide[:, ::2]
    keep = wide.clone()
    out, sw, c = ops.slap_local_search(view, p, locs=l, return_sweeps=True, return_cost=True)
    _eq((out.cpu().numpy(), sw.cpu().numpy(), c.cpu().numpy()), (ref, sweeps, cost))
    assert out.dtype == torch.int64 and out.device == wide.device and torch.equal(wide, keep)
    assert np.array_equal(l.cpu().numpy(), locs) and np.array_equal(p.cpu().numpy(), pl)
    out = ops.slap_local_search(torch.as_tensor(rows.copy()).to(dev), p, locs=l)
    assert out.dtype == torch.int32 and np.array_equal(out.cpu().numpy(), ref)


def test_multistart_locs_batch_abi_and_env(dev):
    s, lb = 3, 5
    locs, pl, rows, ref, sweeps, cost, _ = tc.coords_case(s * lb, 5, 8, 4, 3, 1000, lb)
    _eq(tc.run(ops.slap_local_search, rows, pl, locs=locs, device=dev), (ref, sweeps, cost))
    env = SLAPEnv(generator_params=dict(n_products=5), device=dev)
    tdm = batchify(tc.slap_td(locs, pl, rows, dev), s)
    out, sw = env.improve(tdm, torch.as_tensor(rows.copy()).long().to(dev), return_sweeps=True)
    assert tdm.is_lazy("locs") and tdm.is_lazy("picklist")
    assert out.dtype == torch.int64
    assert np.array_equal(out.cpu().numpy(), ref) and np.array_equal(sw.cpu().numpy(), sweeps)


@pytest.mark.parametrize("kind", tc.ERRORS)
def test_failing_row_is_copied_and_the_rest_is_searched(dev, kind):
    _, _, _, ref, sweeps, cost, _ = tc.coords_case(64, 5, 8, 4, 3)
    rows, pl, locs, D, bit = tc.error_inputs(kind)
    kw = dict(locs=locs) if D is None else dict(distances=D)
    for scheme in (nat.SLAP_LS_AUTO, nat.SLAP_LS_DIRECT):
        st = torch.zeros(1, dtype=torch.int32, device=dev)
        out, sw, c = tc.run(ops.slap_local_search, rows, pl, device=dev, status=st,
                            scheme=scheme, **kw)
        assert int(st.item()) == bit
        keep = np.arange(64) != 3
        _eq((out[keep], sw[keep], c[keep]), (ref[keep], sweeps[keep], cost[keep]))
        assert np.array_equal(out[3], rows[3]) and sw[3] == 0 and c[3] == -1
    env = SLAPEnv(generator_params=dict(n_products=5), device=dev)
    td = tc.slap_td(locs, pl, rows, dev, dist=D)
    exc = IndexError if bit == nat.ST_INDEX_RANGE else AssertionError
    with pytest.raises(exc, match=None if exc is IndexError else "Invalid assignment"):
        env.improve(td, metric="euclidean" if D is None else "dist_mat")


@pytest.mark.parametrize("b,p,L,o,k,max_it", [(16, 20, 100, 20, 5, 1000), (8, 65, 130, 30, 5, 1000)])
def test_device_equals_host_build(dev, b, p, L, o, k, max_it):
    locs, pl, rows, _, _, _, _ = tc.coords_case(b, p, L, o, k, max_it, None, L == 100)
    _eq(tc.run(ops.slap_local_search, rows, pl, locs=locs, device=dev),
        tc.run(ops.slap_local_search, rows, pl, locs=locs))


def test_non_default_stream(dev):
    locs, pl, rows, ref, sweeps, cost, _ = tc.coords_case(64, 5, 8, 4, 3)
    l, p = torch.as_tensor(locs.copy()).to(dev), torch.as_tensor(pl.copy()).to(dev)
    a = torch.as_tensor(rows.copy()).to(dev)
    torch.cuda.synchronize(dev)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        out, sw, c = ops.slap_local_search(a, p, locs=l, return_sweeps=True, return_cost=True)
    stream.synchronize()
    _eq((out.cpu().numpy(), sw.cpu().numpy(), c.cpu().numpy()), (ref, sweeps, cost))


def test_env_improve_and_the_objective_is_the_envs(dev):
    b, p, L, o, k = 16, 20, 100, 20, 5
    locs, pl, rows, ref, sweeps, cost, _ = tc.coords_case(b, p, L, o, k, 1000, None, True)
    env = SLAPEnv(device=dev)
    td = tc.slap_td(locs, pl, rows, dev)
    before = env.get_reward(td, None)
    out = env.improve(td)
    assert out.dtype == torch.int32 and out.device == td["locs"].device
    assert np.array_equal(out.cpu().numpy(), ref)
    td.set("assignment", out)
    after = env.get_reward(td, None)
    got = torch.as_tensor(cost.astype(np.float64)).to(dev) / 2.0 ** 20
    assert ((got + after.double()).abs() <= tc.bound(after, o, k)).all()
    assert (after.double() >= before.double() - tc.bound(before, o, k)).all()
    assert (after > before).any()
    again, sw = env.improve(td, return_sweeps=True)
    assert torch.equal(again, out) and (sw == 1).all()
    with pytest.raises(NotImplementedError):
        env.local_search(td, out)


def test_env_improve_on_generated_instances_and_dist_mat(dev):
    """The generator's own td after the closest-free-slot policy's rollout: improve on the
    Euclidean metric never lowers the reward, and on td["dist_mat"] (Manhattan) equals the
    host build."""
    env = SLAPEnv(device=dev)
    torch.manual_seed(3)
    np.random.seed(3)
    td = env.generator([8])
    td = TensorDict({k: v.to(dev) for k, v in td.items()}, [8])
    order = torch.argsort(td["depot_loc_dist"][:, 1:], dim=1, stable=True)[:, :20] + 1
    td.set("assignment", order.to(torch.int32))
    before = env.get_reward(td, None)
    out = env.improve(td)
    man, sw = env.improve(td, metric="dist_mat", return_sweeps=True)
    cpu = TensorDict({k: v.cpu() for k, v in td.items()}, [8])
    hman, hsw = SLAPEnv(device="cpu").improve(cpu, metric="dist_mat", return_sweeps=True)
    assert torch.equal(man.cpu(), hman) and torch.equal(sw.cpu(), hsw)
    td.set("assignment", out)
    after = env.get_reward(td, None)
    assert (after.double() >= before.double() - tc.bound(before, 20, 5)).all()
    assert (after > before).any()
