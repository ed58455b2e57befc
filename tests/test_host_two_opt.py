"""co_tsp_two_opt on the host build (CPU TensorDicts) against the numpy restatement
(tests/two_opt_ref.py): tours and sweep counts bit-equal on random, tied and cycling
inputs, every layout the ABI accepts, the error paths, and ``TSPEnv.local_search`` on
top.  The device library's argument validation is checked too (no launch, no GPU)."""
import numpy as np
import pytest
import torch

import two_opt_cases as tc
from two_opt_ref import dist_from_locs, two_opt, two_opt_scalar
from rl4co_slap_amd import TensorDict
from rl4co_slap_amd import _native as nat
from rl4co_slap_amd.envs import CVRPEnv, SLAPEnv, TSPEnv
from rl4co_slap_amd.utils import ops
from rl4co_slap_amd.utils.ops import batchify


def _eq(got, want):
    assert np.array_equal(got[0], want[0]), "tours differ"
    assert np.array_equal(got[1], want[1]), ("sweeps differ", got[1], want[1])


@pytest.mark.parametrize("n", [5, 8, 13])
def test_restatement_vectorised_equals_scalar(n):
    rng = np.random.default_rng(n)
    mats = [dist_from_locs(rng.random((n, 2), dtype=np.float32)),
            dist_from_locs(rng.integers(0, 3, size=(n, 2)).astype(np.float32)),
            rng.integers(1, 4, size=(n, n)).astype(np.float32)]
    for D in mats:
        for t in tc.perms(6, n, seed=n):
            for max_it in (0, 1, 2, 50):
                a, b = two_opt(D, t, max_it), two_opt_scalar(D, t, max_it)
                assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]


@pytest.mark.parametrize("name,locs,dist,tour,want,sweeps", tc.KNOWN, ids=[k[0] for k in tc.KNOWN])
def test_known_answers(name, locs, dist, tour, want, sweeps):
    r = two_opt_scalar(dist if dist is not None else dist_from_locs(locs), tour, 1000)
    assert list(r[0]) == want and r[1] == sweeps  # the restatement itself
    got = tc.run(ops.two_opt, [tour], locs=None if locs is None else locs[None],
                 distances=None if dist is None else dist[None])
    assert got[0].tolist() == [want] and got[1].tolist() == [sweeps]


@pytest.mark.parametrize("b,n", [(37, 5), (16, 20), (8, 64), (8, 65), (4, 100)])
def test_host_equals_restatement(b, n):
    locs, tours, ref, sweeps = tc.uniform_case(b, n)
    _eq(tc.run(ops.two_opt, tours, locs=locs), (ref, sweeps))
    assert (sweeps > 1).any()


@pytest.mark.parametrize("max_it", [0, 1, 3, 1000])
def test_max_iterations(max_it):
    locs, tours, ref, sweeps = tc.uniform_case(16, 20, max_it)
    _eq(tc.run(ops.two_opt, tours, locs=locs, max_iterations=max_it), (ref, sweeps))
    assert (sweeps <= max_it).all()
    if max_it == 0:
        assert np.array_equal(ref, tours)


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_tiny_n(n):
    locs, tours, ref, sweeps = tc.uniform_case(9, n)
    _eq(tc.run(ops.two_opt, tours, locs=locs), (ref, sweeps))
    if n < 3:
        assert np.array_equal(ref, tours)


def test_ties_keep_the_first_move():
    tied = 0
    locs, tours, ref, sweeps, k = tc.grid_case()
    _eq(tc.run(ops.two_opt, tours, locs=locs), (ref, sweeps))
    tied += k
    D, tours, ref, sweeps, k = tc.int_matrix_case(24, 14, True)
    _eq(tc.run(ops.two_opt, tours, distances=D), (ref, sweeps))
    tied += k
    D, tours, ref, sweeps, k = tc.int_matrix_case(8, 14, False, 50)
    _eq(tc.run(ops.two_opt, tours, distances=D, max_iterations=50), (ref, sweeps))
    D, tours, ref, sweeps, k = tc.int_matrix_case(2, 30, False, 50)
    _eq(tc.run(ops.two_opt, tours, distances=D, max_iterations=50), (ref, sweeps))
    assert tied > 0  # the tie rule was exercised


def test_distances_of_locs_equal_locs_path():
    locs, tours, ref, sweeps = tc.uniform_case(16, 20)
    D = np.stack([dist_from_locs(l) for l in locs])
    _eq(tc.run(ops.two_opt, tours, distances=D), (ref, sweeps))


def test_step_major_and_int32_actions():
    locs, tours, ref, sweeps = tc.uniform_case(16, 20)
    sm = torch.as_tensor(tours.T.copy())  # [N, B] storage
    view = sm.t()
    assert view.stride() == (1, 16)
    out, sw = ops.two_opt(view, locs=torch.as_tensor(locs.copy()), return_sweeps=True)
    _eq((out.numpy(), sw.numpy()), (ref, sweeps))
    assert out.is_contiguous() and out.dtype == torch.int64
    out = ops.two_opt(torch.as_tensor(tours.astype(np.int32)), locs=torch.as_tensor(locs.copy()))
    assert out.dtype == torch.int64 and np.array_equal(out.numpy(), ref)


def test_multistart_locs_batch_abi_and_env():
    s, lb, n = 3, 5, 12
    locs, tours, ref, sweeps = tc.uniform_case(s * lb, n, 1000, lb)
    _eq(tc.run(ops.two_opt, tours, locs=locs), (ref, sweeps))  # [LB, n, 2] under [S*LB, n]
    env = TSPEnv(generator_params=dict(num_loc=n), device="cpu")
    td = env.reset(TensorDict({"locs": torch.as_tensor(locs.copy())}, [lb]))
    tdm = batchify(td, s)
    assert tdm.is_lazy("locs")
    out, sw = env.local_search(tdm, torch.as_tensor(tours.copy()), return_sweeps=True)
    assert tdm.is_lazy("locs")  # read in place, not replicated
    _eq((out.numpy(), sw.numpy()), (ref, sweeps))


def test_invalid_row_raises_and_the_rest_is_improved():
    locs, tours, ref, sweeps = tc.uniform_case(16, 20)
    bad = tours.copy()
    bad[3, 7] = bad[3, 8]  # a duplicate
    t, l = torch.as_tensor(bad), torch.as_tensor(locs.copy())
    with pytest.raises(AssertionError, match="Invalid tour"):
        ops.two_opt(t, locs=l)
    env = TSPEnv(generator_params=dict(num_loc=20), device="cpu")
    with pytest.raises(AssertionError, match="Invalid tour"):
        env.local_search(TensorDict({"locs": l}, [16]), t)
    status = torch.zeros(1, dtype=torch.int32)
    out, sw = ops.two_opt(t, locs=l, return_sweeps=True, status=status)
    assert int(status) == nat.ST_INVALID_TOUR
    keep = np.arange(16) != 3
    assert np.array_equal(out.numpy()[keep], ref[keep])
    assert np.array_equal(sw.numpy()[keep], sweeps[keep])
    assert np.array_equal(out.numpy()[3], bad[3]) and sw[3] == 0
    out_of_range = tours.copy()
    out_of_range[0, 0] = 20
    with pytest.raises(AssertionError, match="Invalid tour"):
        ops.two_opt(torch.as_tensor(out_of_range), locs=l)


def _abi_args(lib_fn, b, n, locs, dist, lb=None):
    acts = torch.zeros(max(b, 1), max(n, 1), dtype=torch.int64)
    out = torch.zeros_like(acts)
    st = torch.zeros(1, dtype=torch.int32)
    return lib_fn(b, n, locs, dist, lb or max(b, 1), acts.data_ptr(), n, 1, 10, out.data_ptr(),
                  None, st.data_ptr(), None)


@pytest.mark.parametrize("which", ["host", "device"])
def test_argument_errors_return_codes(which):
    """Both libraries validate before any work (the device library before any launch: no
    GPU is touched)."""
    lib = nat.load_host() if which == "host" else nat.load()
    fn = lib.co_tsp_two_opt
    buf = torch.zeros(4 * 8 * 8, dtype=torch.float32)
    p = buf.data_ptr()
    assert _abi_args(fn, 4, 8, p, p) == -1  # both sources
    assert _abi_args(fn, 4, 8, None, None) == -1  # neither
    assert _abi_args(fn, 4, nat.TWO_OPT_MAX_N + 1, p, None) == -1
    assert _abi_args(fn, 4, 0, p, None) == -1
    assert _abi_args(fn, -1, 8, p, None) == -1
    assert _abi_args(fn, 4, 8, p, None, lb=3) == -1  # batch not a multiple of locs_batch
    assert _abi_args(fn, 0, 8, None, None) == 0  # an empty batch is a no-op
    a = torch.zeros(4, 8, dtype=torch.int64)
    st = torch.zeros(1, dtype=torch.int32)
    assert fn(4, 8, p, None, 4, a.data_ptr(), 8, 1, 10, a.data_ptr(), None, st.data_ptr(),
              None) == -1  # output aliases the input
    assert fn(4, 8, p, None, 4, a.data_ptr(), 8, 1, 10, None, None, st.data_ptr(), None) == -1


def test_python_rejects_bad_arguments():
    n = nat.TWO_OPT_MAX_N + 1
    with pytest.raises(ValueError, match=str(nat.TWO_OPT_MAX_N)):
        ops.two_opt(torch.arange(n)[None], locs=torch.zeros(1, n, 2))
    t, l = torch.arange(6)[None], torch.zeros(1, 6, 2)
    with pytest.raises(ValueError):
        ops.two_opt(t, locs=l, distances=torch.zeros(1, 6, 6))
    with pytest.raises(ValueError):
        ops.two_opt(t)
    with pytest.raises(ValueError):
        ops.two_opt(t, locs=torch.zeros(1, 7, 2))
    # the header's bound is the binding's
    hdr = open(nat._HERE + "/../include/co_env.h").read()
    assert f"#define CO_TWO_OPT_MAX_N {nat.TWO_OPT_MAX_N}\n" in hdr
    assert f"#define CO_TWO_OPT_STAGE_N {nat.TWO_OPT_STAGE_N}\n" in hdr
    assert nat.TWO_OPT_MAX_N >= 1024


def test_env_local_search_improves_the_reward():
    b, n = 16, 20
    locs, tours, ref, sweeps = tc.uniform_case(b, n)
    env = TSPEnv(generator_params=dict(num_loc=n), device="cpu")
    td = env.reset(TensorDict({"locs": torch.as_tensor(locs.copy())}, [b]))
    acts = torch.as_tensor(tours.copy())
    before = env.get_reward(td, acts)
    out = env.local_search(td, acts[:, :])  # default max_iterations
    assert out.dtype == torch.int64 and out.shape == (b, n) and out.device == acts.device
    assert np.array_equal(out.numpy(), ref)
    env.check_solution_validity(td, out)
    after = env.get_reward(td, out)
    assert (after >= before).all() and (after > before).all()
    assert np.array_equal(acts.numpy(), tours)  # the input is untouched
    # an already optimal tour comes back unchanged, and td["distances"] takes precedence
    again, sw = env.local_search(td, out, return_sweeps=True)
    assert torch.equal(again, out) and (sw == 1).all()
    D, dt, dref, dsw, _ = tc.int_matrix_case(b, n, True)
    td2 = TensorDict({"locs": td["locs"], "distances": torch.as_tensor(D.copy())}, [b])
    got = env.local_search(td2, torch.as_tensor(dt.copy()))
    assert np.array_equal(got.numpy(), dref)


def test_other_envs_keep_raising():
    for env in (CVRPEnv(device="cpu"), SLAPEnv(device="cpu")):
        with pytest.raises(NotImplementedError):
            env.local_search(None, None)


def test_fastcall_table_has_the_entry():
    fast = nat._fastcall()
    assert fast is not None
    assert "co_tsp_two_opt" in fast.table("host")
    assert fast.table("host")["co_tsp_two_opt"][1] == b"i" * 13
