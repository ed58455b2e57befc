"""co_slap_local_search on the host build (CPU TensorDicts) against the numpy restatement
(tests/slap_ls_ref.py): rows, sweep counts and costs bit-equal on every shape, tied inputs,
both distance sources, every layout the call accepts and the error paths, with
``ops.slap_local_search`` and ``SLAPEnv.improve`` on top.  The device library's argument
validation is checked too (no launch, no GPU)."""
import numpy as np
import pytest
import torch

import slap_ls_cases as tc
from slap_ls_ref import dist_from_locs, local_search, local_search_brute
from rl4co_slap_amd import TensorDict
from rl4co_slap_amd import _native as nat
from rl4co_slap_amd.envs import SLAPEnv
from rl4co_slap_amd.utils import ops
from rl4co_slap_amd.utils.ops import batchify


def _eq(got, want):
    assert np.array_equal(got[0], want[0]), "rows differ"
    assert np.array_equal(got[1], want[1]), ("sweeps differ", got[1], want[1])
    assert np.array_equal(got[2], want[2]), ("costs differ", got[2], want[2])


@pytest.mark.parametrize("p,L,o,k", [(1, 2, 1, 1), (2, 3, 2, 2), (3, 3, 2, 3), (5, 8, 4, 3),
                                     (7, 12, 6, 4)])
def test_restatement_table_equals_brute_force(p, L, o, k):
    rng = np.random.default_rng(p * 100 + L)
    for e in range(4):
        locs = (rng.random((L, 2), dtype=np.float32) * np.float32(10)).astype(np.float32)
        ints = rng.integers(0, 3, size=(L, L)).astype(np.float32)
        pl = rng.integers(0, p, size=(o, k))
        s = rng.permutation(L)[:p]
        for D in (dist_from_locs(locs), ints):
            for max_it in (0, 1, 2, 50):
                a = local_search(D, pl, s, max_it)
                c = local_search_brute(D, pl, s, max_it)
                assert np.array_equal(a[0], c[0]) and a[1:] == c[1:]


@pytest.mark.parametrize("name,locs,pl,row,want,sweeps,cost", tc.KNOWN, ids=[k[0] for k in tc.KNOWN])
def test_known_answers(name, locs, pl, row, want, sweeps, cost):
    D = dist_from_locs(locs)
    for form in (local_search, local_search_brute):  # the restatement itself
        r = form(D, pl, row)
        assert list(r[0]) == want and r[1:3] == (sweeps, cost)
    for kw in (dict(locs=locs[None]), dict(distances=D[None])):
        got = tc.run(ops.slap_local_search, [row], [pl], **kw)
        assert got[0].tolist() == [want] and got[1].tolist() == [sweeps]
        assert got[2].tolist() == [cost]


@pytest.mark.parametrize("b,p,L,o,k,max_it", tc.SHAPES)
def test_host_equals_restatement(b, p, L, o, k, max_it):
    locs, pl, rows, ref, sweeps, cost, _ = tc.coords_case(b, p, L, o, k, max_it, None, L == 100)
    _eq(tc.run(ops.slap_local_search, rows, pl, locs=locs, max_iterations=max_it),
        (ref, sweeps, cost))
    for r in ref:  # still an assignment
        assert len(set(r.tolist())) == p and r.min() >= 0 and r.max() < L
    if p == 1:
        assert (sweeps == 1).all()
    if p >= 5:
        assert (sweeps > 1).any()
    if max_it < 1000:
        assert (sweeps == max_it).all()


@pytest.mark.parametrize("p,L", tc.CUT_SHAPES)
def test_shapes_at_the_device_cut(p, L):
    """Either side of the device's table / direct cut at two P (the host build has one
    scheme; the restatement's answers for these shapes are the device tests' too)."""
    assert [nat.slap_ls_table_fits(*c) for c in tc.CUT_SHAPES] == [True, False, True, False]
    locs, pl, rows, ref, sweeps, cost, _ = tc.coords_case(2, p, L, 20, 5, 30)
    _eq(tc.run(ops.slap_local_search, rows, pl, locs=locs, max_iterations=30), (ref, sweeps, cost))
    D, pl, rows, ref, sweeps, cost, _ = tc.matrix_case(2, p, L, 20, 5, 30)
    _eq(tc.run(ops.slap_local_search, rows, pl, distances=D, max_iterations=30),
        (ref, sweeps, cost))


@pytest.mark.parametrize("symmetric", [True, False])
def test_ties_follow_the_rule(symmetric):
    D, pl, rows, ref, sweeps, cost, tied = tc.int_matrix_case(8, symmetric)
    assert tied > 0  # the tie rule is exercised
    _eq(tc.run(ops.slap_local_search, rows, pl, distances=D), (ref, sweeps, cost))


def test_distances_of_locs_equal_locs_path():
    locs, pl, rows, ref, sweeps, cost, _ = tc.coords_case(64, 5, 8, 4, 3)
    D = np.stack([dist_from_locs(l) for l in locs])
    _eq(tc.run(ops.slap_local_search, rows, pl, distances=D), (ref, sweeps, cost))


def test_asymmetric_matrix():
    D, pl, rows, ref, sweeps, cost, _ = tc.matrix_case(8, 12, 20, 10, 4)
    _eq(tc.run(ops.slap_local_search, rows, pl, distances=D), (ref, sweeps, cost))
    assert (sweeps > 1).any()


def test_product_on_slot_0():
    locs, pl, rows, ref, sweeps, cost, _ = tc.coords_case(64, 5, 8, 4, 3)
    assert (rows == 0).any()  # the case holds such rows
    one = np.flatnonzero((rows == 0).any(1))[:1]
    _eq(tc.run(ops.slap_local_search, rows[one], pl[one], locs=locs[one]),
        (ref[one], sweeps[one], cost[one]))


@pytest.mark.parametrize("max_it", [0, 1, 3, 1000])
def test_max_iterations(max_it):
    locs, pl, rows, ref, sweeps, cost, _ = tc.coords_case(16, 20, 100, 20, 5, max_it, None, True)
    _eq(tc.run(ops.slap_local_search, rows, pl, locs=locs, max_iterations=max_it),
        (ref, sweeps, cost))
    assert (sweeps <= max_it).all()
    if max_it == 0:
        assert np.array_equal(ref, rows)


def test_max_iterations_above_int32_is_capped():
    locs, pl, rows, ref, sweeps, cost, _ = tc.coords_case(64, 5, 8, 4, 3)
    _eq(tc.run(ops.slap_local_search, rows, pl, locs=locs, max_iterations=2 ** 40),
        (ref, sweeps, cost))


def test_dtypes_and_strides():
    locs, pl, rows, ref, sweeps, cost, _ = tc.coords_case(64, 5, 8, 4, 3)
    l, p = torch.as_tensor(locs.copy()), torch.as_tensor(pl.copy())
    for dt in (torch.int64, torch.int32, torch.int16, torch.uint8):
        out = ops.slap_local_search(torch.as_tensor(rows.copy()).to(dt), p, locs=l)
        assert out.dtype == dt and np.array_equal(out.numpy().astype(np.int32), ref)
    wide = torch.zeros(64, 10, dtype=torch.int64)
    wide[:, ::2] = torch.as_tensor(rows.copy()).long()
    view = wide[:, ::2]
    assert not view.is_contiguous()
    out, sw, c = ops.slap_local_search(view, p, locs=l, return_sweeps=True, return_cost=True)
    _eq((out.numpy(), sw.numpy(), c.numpy()), (ref, sweeps, cost))
    assert out.dtype == torch.int64 and sw.dtype == torch.int32 and c.dtype == torch.int64
    tr = torch.as_tensor(rows.T.copy()).t()  # [P, B] storage
    assert np.array_equal(ops.slap_local_search(tr, p, locs=l).numpy(), ref)
    assert np.array_equal(l.numpy(), locs) and np.array_equal(p.numpy(), pl)  # inputs untouched
    out, c = ops.slap_local_search(view, p, locs=l, return_cost=True)
    assert np.array_equal(c.numpy(), cost)


def test_multistart_locs_batch_abi_and_env():
    s, lb = 3, 5
    locs, pl, rows, ref, sweeps, cost, _ = tc.coords_case(s * lb, 5, 8, 4, 3, 1000, lb)
    _eq(tc.run(ops.slap_local_search, rows, pl, locs=locs), (ref, sweeps, cost))
    env = SLAPEnv(generator_params=dict(n_products=5), device="cpu")
    tdm = batchify(tc.slap_td(locs, pl, rows), s)
    assert tdm.is_lazy("locs") and tdm.is_lazy("picklist")
    out, sw = env.improve(tdm, torch.as_tensor(rows.copy()).long(), return_sweeps=True)
    assert tdm.is_lazy("locs") and tdm.is_lazy("picklist")  # read in place, not replicated
    assert out.dtype == torch.int64
    assert np.array_equal(out.numpy(), ref) and np.array_equal(sw.numpy(), sweeps)


@pytest.mark.parametrize("kind", tc.ERRORS)
def test_failing_row_is_copied_and_the_rest_is_searched(kind):
    _, _, _, ref, sweeps, cost, _ = tc.coords_case(64, 5, 8, 4, 3)
    rows, pl, locs, D, bit = tc.error_inputs(kind)
    kw = dict(locs=locs) if D is None else dict(distances=D)
    st = torch.zeros(1, dtype=torch.int32)
    out, sw, c = tc.run(ops.slap_local_search, rows, pl, status=st, **kw)
    assert int(st) == bit
    keep = np.arange(64) != 3
    _eq((out[keep], sw[keep], c[keep]), (ref[keep], sweeps[keep], cost[keep]))
    assert np.array_equal(out[3], rows[3]) and sw[3] == 0 and c[3] == -1
    exc = IndexError if bit == nat.ST_INDEX_RANGE else AssertionError
    with pytest.raises(exc, match=None if exc is IndexError else "Invalid assignment"):
        tc.run(ops.slap_local_search, rows, pl, **kw)
    env = SLAPEnv(generator_params=dict(n_products=5), device="cpu")
    td = tc.slap_td(locs, pl, rows, dist=D)
    with pytest.raises(exc, match=None if exc is IndexError else "Invalid assignment"):
        env.improve(td, metric="euclidean" if D is None else "dist_mat")


def test_infinite_coordinate_and_negative_distance_fail_the_row():
    rows, pl, locs, _, _ = tc.error_inputs("duplicate")
    rows = tc.coords_case(64, 5, 8, 4, 3)[2]
    for value in (np.inf, -np.inf, np.float32(2 ** 18 + 1)):
        bad = locs.copy()
        bad[9, 0, 0] = value
        st = torch.zeros(1, dtype=torch.int32)
        out, sw, c = tc.run(ops.slap_local_search, rows, pl, locs=bad, status=st)
        assert int(st) == nat.ST_INVALID_TOUR and sw[9] == 0 and c[9] == -1
    D = np.stack([dist_from_locs(l) for l in locs])
    for value in (-1.0, np.nan, np.inf):
        bad = D.copy()
        bad[9, 1, 1] = value
        st = torch.zeros(1, dtype=torch.int32)
        out, sw, c = tc.run(ops.slap_local_search, rows, pl, distances=bad, status=st)
        assert int(st) == nat.ST_INVALID_TOUR and sw[9] == 0 and c[9] == -1


def test_int64_slot_beyond_int32_fails_the_row_and_comes_back():
    locs, pl, rows, ref, sweeps, cost, _ = tc.coords_case(64, 5, 8, 4, 3)
    big = torch.as_tensor(rows.copy()).long()
    big[3, 2] = 2 ** 32 + 1  # would wrap to slot 1
    big[5, 0] = -2 ** 40
    st = torch.zeros(1, dtype=torch.int32)
    out, sw = ops.slap_local_search(big, torch.as_tensor(pl.copy()), locs=torch.as_tensor(locs.copy()),
                                    return_sweeps=True, status=st)
    assert int(st) == nat.ST_INVALID_TOUR
    keep = ~np.isin(np.arange(64), [3, 5])
    assert np.array_equal(out.numpy()[keep], ref[keep]) and torch.equal(out[~keep], big[~keep])
    assert (sw.numpy()[~keep] == 0).all()


def _abi(fn, b, L, p, o, k, locs, dist, lb=None, out_alias=False, out_null=False, pl_null=False):
    rows = torch.zeros(max(b, 1), max(p, 1), dtype=torch.int32)
    out = torch.zeros_like(rows)
    pl = torch.zeros(max(b, 1) * max(o * k, 1), dtype=torch.int64)
    st = torch.zeros(1, dtype=torch.int32)
    op = None if out_null else (rows if out_alias else out).data_ptr()
    return fn(b, L, p, o, k, locs, dist, lb or max(b, 1), None if pl_null else pl.data_ptr(),
              rows.data_ptr(), 10, op, None, None, st.data_ptr(), None)


@pytest.mark.parametrize("which", ["host", "device"])
def test_argument_errors_return_codes(which):
    """Both libraries validate before any work (the device library before any launch: no
    GPU is touched)."""
    lib = nat.load_host() if which == "host" else nat.load()
    fn = lib.co_slap_local_search
    buf = torch.zeros(4 * 16 * 16, dtype=torch.float32)
    q = buf.data_ptr()
    assert _abi(fn, 4, 8, 5, 4, 3, q, q) == -1  # both sources
    assert _abi(fn, 4, 8, 5, 4, 3, None, None) == -1  # neither
    assert _abi(fn, 4, 8, 0, 4, 3, q, None) == -1  # no product
    assert _abi(fn, 4, 8, 9, 4, 3, q, None) == -1  # more products than slots
    assert _abi(fn, 4, 1025, 5, 4, 3, q, None) == -1
    assert _abi(fn, 4, 256, 129, 4, 3, q, None) == -1
    assert _abi(fn, 4, 8, 5, 0, 3, q, None) == -1
    assert _abi(fn, 4, 8, 5, 4, 0, q, None) == -1
    assert _abi(fn, 4, 8, 5, 65536, 2, q, None) == -1  # O*K above 65536
    assert _abi(fn, -1, 8, 5, 4, 3, q, None) == -1
    assert _abi(fn, 4, 8, 5, 4, 3, q, None, lb=3) == -1  # batch not a multiple of locs_batch
    assert _abi(fn, 0, 8, 5, 4, 3, None, None) == 0  # an empty batch is a no-op
    assert _abi(fn, 4, 8, 5, 4, 3, q, None, out_alias=True) == -1
    assert _abi(fn, 4, 8, 5, 4, 3, q, None, out_null=True) == -1
    assert _abi(fn, 4, 8, 5, 4, 3, q, None, pl_null=True) == -1


def test_scheme_entry_validates_without_a_launch():
    fn = nat.load().co_slap_local_search_scheme
    rows = torch.zeros(4, 33, dtype=torch.int32)
    out = torch.zeros_like(rows)
    pl = torch.zeros(4 * 12, dtype=torch.int64)
    st = torch.zeros(1, dtype=torch.int32)
    buf = torch.zeros(16, dtype=torch.float32)

    def call(L, p, scheme):
        return fn(4, L, p, 4, 3, buf.data_ptr(), None, 4, pl.data_ptr(), rows.data_ptr(), 10,
                  out.data_ptr(), None, None, scheme, st.data_ptr(), None)

    assert call(240, 32, nat.SLAP_LS_TABLE) == -1  # the table does not fit the LDS budget
    assert call(8, 5, 3) == -1  # no such scheme
    with pytest.raises(ValueError, match="host build"):
        ops.slap_local_search(torch.zeros(1, 2, dtype=torch.int32),
                              torch.zeros(1, 1, 2, dtype=torch.int64), locs=torch.zeros(1, 3, 2),
                              scheme=nat.SLAP_LS_DIRECT)


def test_python_rejects_bad_arguments():
    a, pl, l = torch.zeros(2, 5, dtype=torch.int32), torch.zeros(2, 4, 3, dtype=torch.int64), \
        torch.zeros(2, 8, 2)
    with pytest.raises(ValueError, match="exactly one"):
        ops.slap_local_search(a, pl, locs=l, distances=torch.zeros(2, 8, 8))
    with pytest.raises(ValueError, match="exactly one"):
        ops.slap_local_search(a, pl)
    with pytest.raises(ValueError):
        ops.slap_local_search(a[0], pl, locs=l)  # assignment not [B, P]
    with pytest.raises(ValueError):
        ops.slap_local_search(a, pl[0], locs=l)  # picklist not [LB, O, K]
    with pytest.raises(ValueError):
        ops.slap_local_search(a, pl, locs=torch.zeros(2, 8, 3))
    with pytest.raises(ValueError):
        ops.slap_local_search(a, pl, distances=torch.zeros(2, 8, 7))
    with pytest.raises(ValueError):
        ops.slap_local_search(a, pl, locs=torch.zeros(2, 4, 2))  # 4 slots, 5 products
    with pytest.raises(ValueError):
        ops.slap_local_search(torch.zeros(3, 5, dtype=torch.int32), pl, locs=l)  # 3 % 2 != 0
    with pytest.raises(ValueError):
        ops.slap_local_search(a.float(), pl, locs=l)
    with pytest.raises(ValueError, match=str(nat.SLAP_LS_MAX_PRODUCTS)):
        ops.slap_local_search(torch.zeros(1, 129, dtype=torch.int32),
                              torch.zeros(1, 4, 3, dtype=torch.int64), locs=torch.zeros(1, 200, 2))
    with pytest.raises(ValueError, match=str(nat.SLAP_LS_MAX_SLOTS)):
        ops.slap_local_search(torch.zeros(1, 5, dtype=torch.int32),
                              torch.zeros(1, 4, 3, dtype=torch.int64), locs=torch.zeros(1, 1025, 2))
    env = SLAPEnv(device="cpu")
    with pytest.raises(ValueError, match="metric"):
        env.improve(TensorDict({}, [1]), metric="manhattan")
    # an empty batch is a no-op
    out = ops.slap_local_search(torch.zeros(0, 5, dtype=torch.int64), pl, locs=l)
    assert out.shape == (0, 5) and out.dtype == torch.int64
    # the header's bounds are the binding's
    hdr = open(nat._HERE + "/../include/co_env.h").read()
    for name in ("MAX_PRODUCTS", "MAX_SLOTS", "LDS_BYTES", "AUTO", "DIRECT", "TABLE"):
        assert f"#define CO_SLAP_LS_{name} {getattr(nat, 'SLAP_LS_' + name)}\n" in hdr
    assert ("#define CO_SLAP_LS_STATE_BYTES(P, L) (2 * (P) * ((P) + 1) + 4 * (P) + 8 * (L) + "
            "(L) / 8 + 64)\n") in hdr
    assert "(8 * (P) * (L) + CO_SLAP_LS_STATE_BYTES(P, L) <= CO_SLAP_LS_LDS_BYTES)\n" in hdr


def test_env_improve_and_the_objective_is_the_envs():
    b, p, L, o, k = 16, 20, 100, 20, 5
    locs, pl, rows, ref, sweeps, cost, _ = tc.coords_case(b, p, L, o, k, 1000, None, True)
    env = SLAPEnv(device="cpu")
    td = tc.slap_td(locs, pl, rows)
    before = env.get_reward(td, None)
    start = td["assignment"].clone()
    out = env.improve(td)  # actions=None: td["assignment"], default max_iterations
    assert out.dtype == torch.int32 and out.shape == (b, p) and np.array_equal(out.numpy(), ref)
    assert torch.equal(td["assignment"], start)  # the input is untouched
    td.set("assignment", out)
    after = env.get_reward(td, None)
    # cost / 2^20 is -reward: f32 summation rounding + the quantisation of O*K edges
    got = torch.as_tensor(cost.astype(np.float64)) / 2.0 ** 20
    assert ((got + after.double()).abs() <= tc.bound(after, o, k)).all()
    assert (after.double() >= before.double() - tc.bound(before, o, k)).all()
    assert (after > before).any()
    # a local optimum comes back unchanged after one sweep
    again, sw = env.improve(td, return_sweeps=True)
    assert torch.equal(again, out) and (sw == 1).all()
    # a rollout's int64 action matrix in, int64 out
    acts = torch.as_tensor(rows.copy()).long()
    got, sw = env.improve(td, acts, 3, return_sweeps=True)
    want = tc.coords_case(b, p, L, o, k, 3, None, True)
    assert got.dtype == torch.int64 and np.array_equal(got.numpy(), want[3])
    assert np.array_equal(sw.numpy(), want[4])


def test_env_improve_on_dist_mat():
    D, pl, rows, ref, sweeps, cost, _ = tc.int_matrix_case(8, False)
    env = SLAPEnv(generator_params=dict(n_products=12), device="cpu")
    td = tc.slap_td(np.zeros((8, 14, 2), dtype=np.float32), pl, rows, dist=D)
    out, sw = env.improve(td, metric="dist_mat", return_sweeps=True)
    assert np.array_equal(out.numpy(), ref) and np.array_equal(sw.numpy(), sweeps)


def test_local_search_still_raises():
    with pytest.raises(NotImplementedError):
        SLAPEnv(device="cpu").local_search(None, None)


def test_both_libraries_export_the_entry():
    assert hasattr(nat.load_host(), "co_slap_local_search")
    assert hasattr(nat.load(), "co_slap_local_search")
    assert hasattr(nat.load(), "co_slap_local_search_scheme")
    assert "co_slap_local_search" in nat.HOST_SYMBOLS
    assert "co_slap_local_search" in nat.exported_symbols()
    fast = nat._fastcall()
    assert fast is not None
    assert fast.table("host")["co_slap_local_search"][1] == b"i" * 16
