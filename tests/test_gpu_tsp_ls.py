"""co_tsp_local_search on the device against the numpy restatement (tests/tsp_ls_ref.py) and
the host build: tours, sweeps and move counts bit-equal.  One wavefront runs a row's whole
descent for every N; the shapes cross the 64-lane window (63, 64, 65), the chunked rotation
of an Or-opt move (more than 64 positions between segment and insertion point) and, on the
distances path, the LDS staging cut at N = CO_TWO_OPT_STAGE_N."""
import numpy as np
import pytest
import torch

import tsp_ls_cases as lc
import two_opt_cases as tc
from tsp_ls_ref import OR_OPT, TWO_OPT
from rl4co_slap_amd import TensorDict
from rl4co_slap_amd import _native as nat
from rl4co_slap_amd.envs import TSPEnv
from rl4co_slap_amd.utils import ops
from rl4co_slap_amd.utils.ops import batchify

pytestmark = pytest.mark.gpu

BOTH = lc.BOTH
CUT = nat.TWO_OPT_STAGE_N
# (b, n, operators, min_or_rows): as tests/test_host_tsp_ls.py -- after 2-opt the small
# shapes rarely have an Or-opt move left, so they also run with OR_OPT alone (n = 3 has no
# improving move at all: every 3-city tour has the same length)
COORDS = [(32, 3, OR_OPT, 0.0)] + [(32, n, OR_OPT, 0.25) for n in (4, 5, 6, 7, 8)] + \
         [(32, n, BOTH, 0.0) for n in (3, 4, 5, 6, 7, 8)] + \
         [(16, 20, BOTH, 0.25), (8, 63, BOTH, 0.25), (8, 64, BOTH, 0.25), (8, 65, BOTH, 0.25),
          (8, 100, BOTH, 0.25), (4, 100, OR_OPT, 0.25)]


def _eq(got, want):
    assert np.array_equal(got[0], want[0]), "tours differ"
    assert np.array_equal(got[1], want[1]), ("sweeps differ", got[1], want[1])
    assert np.array_equal(got[2], want[2]), ("moves differ", got[2], want[2])


@pytest.mark.parametrize("b,n,operators,min_or", COORDS)
def test_device_equals_restatement(dev, b, n, operators, min_or):
    locs, tours, ref, sweeps, moves = lc.uniform_case(b, n, operators, 1000, None, min_or)
    _eq(lc.run(ops.tsp_local_search, tours, locs=locs, device=dev, operators=operators),
        (ref, sweeps, moves))


@pytest.mark.parametrize("b,n", [(8, 20), (4, CUT), (4, CUT + 1), (4, 150)])
def test_distances_path_both_sides_of_the_staging_cut(dev, b, n):
    assert CUT == 126
    D, tours, ref, sweeps, moves = lc.matrix_case(b, n)
    _eq(lc.run(ops.tsp_local_search, tours, distances=D, device=dev), (ref, sweeps, moves))


@pytest.mark.parametrize("operators", [OR_OPT, BOTH])
def test_longest_tour_capped(dev, operators):
    """N = 1024, three sweeps: with OR_OPT alone each applies an Or-opt move (rotations over
    many 64-position chunks), with both operators each applies a 2-opt move."""
    locs, tours, ref, sweeps, moves = lc.uniform_case(1, 1024, operators, 3, None,
                                                      0.25 if operators == OR_OPT else 0.0)
    _eq(lc.run(ops.tsp_local_search, tours, locs=locs, device=dev, operators=operators,
               max_iterations=3), (ref, sweeps, moves))
    assert (sweeps == 3).all() and moves.sum() == 3


@pytest.mark.parametrize("operators", [OR_OPT, BOTH])
def test_tie_grid(dev, operators):
    locs, tours, ref, sweeps, moves, tied = lc.grid_case(operators)
    assert tied > 0
    _eq(lc.run(ops.tsp_local_search, tours, locs=locs, device=dev, operators=operators),
        (ref, sweeps, moves))


@pytest.mark.parametrize("operators", [OR_OPT, BOTH])
@pytest.mark.parametrize("symmetric", [True, False])
def test_integer_matrices(dev, symmetric, operators):
    """{1, 2, 3} matrices: bit-equal changes everywhere; the asymmetric search may cycle, so
    it always runs under a small explicit cap."""
    max_it = 1000 if symmetric else 50
    D, tours, ref, sweeps, moves, tied = lc.int_matrix_case(24 if symmetric else 8, 14,
                                                            symmetric, operators, max_it)
    assert tied > 0
    _eq(lc.run(ops.tsp_local_search, tours, distances=D, device=dev, operators=operators,
               max_iterations=max_it), (ref, sweeps, moves))


@pytest.mark.parametrize("name,locs,dist,operators,tour,want,sweeps,moves", lc.KNOWN,
                         ids=[k[0] for k in lc.KNOWN])
def test_known_answers(dev, name, locs, dist, operators, tour, want, sweeps, moves):
    got = lc.run(ops.tsp_local_search, [tour], locs=None if locs is None else locs[None],
                 distances=None if dist is None else dist[None], device=dev,
                 operators=operators)
    assert got[0].tolist() == [want] and got[1].tolist() == [sweeps]
    assert got[2].tolist() == [list(moves)]


def test_two_opt_mask_equals_co_tsp_two_opt(dev):
    for b, n in ((37, 5), (16, 20), (8, 65), (9, 2)):
        locs, tours, ref, sweeps = tc.uniform_case(b, n)
        got = lc.run(ops.tsp_local_search, tours, locs=locs, device=dev, operators=TWO_OPT)
        old = tc.run(ops.two_opt, tours, locs=locs, device=dev)
        assert np.array_equal(got[0], old[0]) and np.array_equal(got[1], old[1])
        assert np.array_equal(got[0], ref) and np.array_equal(got[1], sweeps)
        assert np.array_equal(got[2][:, 0], sweeps - 1) and (got[2][:, 1] == 0).all()


@pytest.mark.parametrize("b,n", lc.TWO_OPT_ONLY_COORDS)
def test_two_opt_only_counts_moves_on_coordinates(dev, b, n):
    locs, *case = lc.uniform_case(b, n, TWO_OPT, 1000, None, 0.0)
    lc.check_two_opt_only(ops, case, dev, locs=locs)


@pytest.mark.parametrize("b,n", lc.TWO_OPT_ONLY_MATRICES)
def test_two_opt_only_counts_moves_on_distances(dev, b, n):
    assert CUT == 126
    D, *case = lc.matrix_case(b, n, TWO_OPT, 1000, 0.0)
    lc.check_two_opt_only(ops, case, dev, distances=D)


def test_two_opt_only_counts_moves_on_asymmetric_matrices(dev):
    """{1, 2, 3} matrices under a cap of 50 (such a search may cycle): every sweep applies a
    move but a last one that finds none, which only a row stopped by the cap can lack."""
    D, *case, _ = lc.int_matrix_case(8, 14, False, TWO_OPT, 50)
    sweeps, moves = lc.check_two_opt_only(ops, case, dev, 50, distances=D)
    assert ((moves[:, 0] == sweeps - 1) | ((sweeps == 50) & (moves[:, 0] == sweeps))).all()


@pytest.mark.parametrize("max_it", [0, 1, 3])
def test_two_opt_only_max_iterations(dev, max_it):
    locs, *case = lc.uniform_case(16, 20, TWO_OPT, max_it, None, 0.0)
    sweeps, moves = lc.check_two_opt_only(ops, case, dev, max_it, locs=locs)
    # a random 20-city tour is not 2-optimal after three moves: every row stops at the cap,
    # having applied a move in each sweep
    assert (sweeps == max_it).all() and np.array_equal(moves[:, 0], sweeps)
    if max_it == 0:
        assert np.array_equal(case[1], case[0])


def test_two_opt_only_invalid_rows(dev):
    lc.check_two_opt_only_invalid_rows(ops, dev, nat.ST_INVALID_TOUR)


def test_two_opt_only_null_outputs(dev):
    lc.check_two_opt_only_null_outputs(ops, dev)


@pytest.mark.parametrize("max_it", [0, 1, 14, 16])
def test_max_iterations(dev, max_it):
    locs, tours, ref, sweeps, moves = lc.uniform_case(16, 20, BOTH, max_it, None, 0.0)
    _eq(lc.run(ops.tsp_local_search, tours, locs=locs, device=dev, max_iterations=max_it),
        (ref, sweeps, moves))


def test_step_major_int32_optional_outputs_and_inputs_unchanged(dev):
    locs, tours, ref, sweeps, moves = lc.uniform_case(16, 20)
    l = torch.as_tensor(locs.copy()).to(dev)
    sm = torch.as_tensor(tours.T.copy()).to(dev)  # [N, B] storage
    view = sm.t()
    assert view.stride() == (1, 16)
    out, sw, mv = ops.tsp_local_search(view, locs=l, return_sweeps=True, return_moves=True)
    _eq((out.cpu().numpy(), sw.cpu().numpy(), mv.cpu().numpy()), (ref, sweeps, moves))
    assert out.is_contiguous() and out.dtype == torch.int64 and out.device == sm.device
    assert np.array_equal(sm.cpu().numpy(), tours.T) and np.array_equal(l.cpu().numpy(), locs)
    out = ops.tsp_local_search(view, locs=l)  # sweeps_out and moves_out both null
    assert np.array_equal(out.cpu().numpy(), ref)
    out = ops.tsp_local_search(torch.as_tensor(tours.astype(np.int32)).to(dev), locs=l)
    assert out.dtype == torch.int64 and np.array_equal(out.cpu().numpy(), ref)


def test_multistart_locs_batch_abi_and_env(dev):
    s, lb, n = 3, 5, 12
    locs, tours, ref, sweeps, moves = lc.uniform_case(s * lb, n, BOTH, 1000, lb, 0.0)
    _eq(lc.run(ops.tsp_local_search, tours, locs=locs, device=dev), (ref, sweeps, moves))
    env = TSPEnv(generator_params=dict(num_loc=n), device=dev)
    td = env.reset(TensorDict({"locs": torch.as_tensor(locs.copy()).to(dev)}, [lb]))
    tdm = batchify(td, s)
    acts = torch.as_tensor(tours.copy()).to(dev)
    out, sw = env.local_search(tdm, acts, return_sweeps=True, operators=("two_opt", "or_opt"))
    assert tdm.is_lazy("locs")
    assert np.array_equal(out.cpu().numpy(), ref) and np.array_equal(sw.cpu().numpy(), sweeps)
    before = env.get_reward(tdm, acts)
    after = env.get_reward(tdm, out)  # also checks validity
    assert (after >= before).all()


def test_invalid_row_sets_status_and_the_rest_is_improved(dev):
    locs, tours, ref, sweeps, moves = lc.uniform_case(16, 20)
    bad = tours.copy()
    bad[3, 7] = bad[3, 8]
    bad[5, 0] = 20  # out of range
    t, l = torch.as_tensor(bad).to(dev), torch.as_tensor(locs.copy()).to(dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    out, sw, mv = ops.tsp_local_search(t, locs=l, return_sweeps=True, return_moves=True,
                                       status=status)
    assert int(status.item()) == nat.ST_INVALID_TOUR
    out, sw, mv = out.cpu().numpy(), sw.cpu().numpy(), mv.cpu().numpy()
    keep = ~np.isin(np.arange(16), [3, 5])
    _eq((out[keep], sw[keep], mv[keep]), (ref[keep], sweeps[keep], moves[keep]))
    assert np.array_equal(out[~keep], bad[~keep]) and (sw[~keep] == 0).all()
    assert (mv[~keep] == 0).all()
    env = TSPEnv(generator_params=dict(num_loc=20), device=dev)
    with pytest.raises(AssertionError, match="Invalid tour"):
        env.local_search(TensorDict({"locs": l}, [16]), t, operators=("two_opt", "or_opt"))


def test_device_equals_host_build(dev):
    locs, tours, _, _, _ = lc.uniform_case(8, 100)
    _eq(lc.run(ops.tsp_local_search, tours, locs=locs, device=dev),
        lc.run(ops.tsp_local_search, tours, locs=locs))
