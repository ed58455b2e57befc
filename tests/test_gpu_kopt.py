"""The k-opt improvement kernels (csrc/tsp_kopt.hip) on the device: the recorded episodes of
the reference's TSPkoptEnv, the device against the host build (integers bit for bit, costs
within 1e-5 relative) and co_tsp_kopt_steps against the single-step launches (every output
bit for bit), over the sizes at which the kernel takes another path: N below, at and above
the wave width, N = 1024, batches of 1, 3 and 67 rows (more than one block per CU is not
needed: rows are independent), strided and step-major actions, locs_batch < batch, node 0
inside the reversed path, the whole-tour reversal and first == second.  k_max = 2, 3, 4 at
every shape and 5, 8, 15, 16 (CO_KOPT_MAX_K) at N = 20, 65, 130 with B = 8, T = 3, the 48-wide
row of k = 16 also with act_stride_a = 2 and from a padded buffer, and a walk at k = 16 whose
result is no cycle.  Every (first, second) of one tour at N = 3..6, 65 and 129.  Invalid rows
only set their status bit."""
import pytest
import torch

import kopt_cases as kc
import kopt_ref
from ref_recordings import check_close, check_equal

from rl4co_slap_amd import _native as nat
from rl4co_slap_amd.envs import ImprovementEnvBase, TSPGenerator

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(3, 3), (5, 1), (63, 3), (64, 3), (65, 67), (129, 3), (1024, 2)]  # (N, B)


@pytest.mark.parametrize("case", kc.recorded_cases())
def test_device_matches_the_recording(case):
    kc.check_recorded_case(case, DEV)


def _run_single(env, td, acts):
    rewards, costs = [], []
    for a in acts:
        td["action"] = a
        td = env.step(td)["next"]
        rewards.append(td["reward"])
        costs.append(td["cost_current"])
    return td, rewards, costs


@pytest.mark.parametrize("k", [2, 3, 4])
@pytest.mark.parametrize("n,b", SHAPES)
def test_device_against_host_and_fused_against_single(n, b, k):
    t = 2 if n >= 129 else 7
    locs, rec, g = kc.instance(b, n, 1000 * k + n)
    acts = kc.actions_for(g, rec, k, t)
    host_env, dev_env = kc.product_env(n, k, "cpu"), kc.product_env(n, k, DEV)
    host, _, _ = _run_single(host_env, kc.product_state(locs, rec, "cpu"), acts)
    dacts = acts.to(DEV)
    dev, rewards, _ = _run_single(dev_env, kc.product_state(locs, rec, DEV), dacts)
    for key in kc.STATE_INT:
        check_equal(dev[key], host[key], f"n{n} b{b} k{k} {key}")
    for key in kc.STATE_F32 + ("reward",):
        check_close(dev[key], host[key], f"n{n} b{b} k{k} {key}")
    check_equal(ImprovementEnvBase._get_real_solution(dev["rec_current"]),
                kopt_ref.real_solution(host["rec_current"]), "real solution")
    for steps in (1, 2, 7):
        if steps > t:
            continue
        one, r1, _ = _run_single(dev_env, kc.product_state(locs, rec, DEV), dacts[:steps])
        many = kc.product_state(locs, rec, DEV)
        got = dev_env.improve_steps(many, dacts[:steps])
        check_equal(got, torch.stack(r1).cpu(), f"T{steps} rewards")
        for key in kc.STATE_INT + kc.STATE_F32:
            check_equal(many[key], one[key].cpu(), f"n{n} b{b} k{k} T{steps} {key}")


@pytest.mark.parametrize("k,n", kc.HIGH_K)
def test_k_max_up_to_the_largest(k, n):
    """5 <= k_max <= CO_KOPT_MAX_K (16: kopt_walk fills the 16 ints of its right-node scratch,
    the last bytes of the workgroup's LDS, and the action row is 48 wide), compared as
    test_device_against_host_and_fused_against_single compares k = 2..4; every row moves and
    every improvement test is clear of the summation order (kc.high_k_case)."""
    locs, rec, acts, after = kc.high_k_case(k, n)
    assert (after[-1]["rec_current"] != rec).any(1).all(), "a row's tour did not change"
    host_env, dev_env = kc.product_env(n, k, "cpu"), kc.product_env(n, k, DEV)
    host, _, _ = _run_single(host_env, kc.product_state(locs, rec, "cpu"), acts)
    dacts = acts.to(DEV)
    dev, rewards, _ = _run_single(dev_env, kc.product_state(locs, rec, DEV), dacts)
    for key in kc.STATE_INT:
        check_equal(dev[key], host[key], f"n{n} k{k} {key}")
    for key in kc.STATE_F32 + ("reward",):
        check_close(dev[key], host[key], f"n{n} k{k} {key}")
    kc.check_state(dev, after[-1], f"n{n} k{k} restatement", kc.STEP_KEYS)
    check_equal(ImprovementEnvBase._get_real_solution(dev["rec_current"]),
                kopt_ref.real_solution(host["rec_current"]), "real solution")
    for steps in (1, 2, 3):
        one, r1, _ = _run_single(dev_env, kc.product_state(locs, rec, DEV), dacts[:steps])
        many = kc.product_state(locs, rec, DEV)
        got = dev_env.improve_steps(many, dacts[:steps])
        check_equal(got, torch.stack(r1).cpu(), f"T{steps} rewards")
        for key in kc.STATE_INT + kc.STATE_F32:
            check_equal(many[key], one[key].cpu(), f"n{n} k{k} T{steps} {key}")
    if k == 16:  # the 48-wide action row read with act_stride_a != 1 and from a padded buffer
        t, b, a_w = acts.shape
        wide = torch.full((t, b, 2 * a_w + 5), -9, dtype=torch.int64, device=DEV)
        wide[:, :, 3:3 + 2 * a_w:2] = dacts
        padded = torch.full((t, b, a_w + 5), -9, dtype=torch.int64, device=DEV)
        padded[:, :, 2:2 + a_w] = dacts
        for name, view in (("stride 2", wide[:, :, 3:3 + 2 * a_w:2]),
                           ("padded", padded[:, :, 2:2 + a_w])):
            assert not view.is_contiguous() and torch.equal(view, dacts)
            td = kc.product_state(locs, rec, DEV)
            check_equal(dev_env.improve_steps(td, view), got.cpu(), name + " rewards")
            for key in kc.STATE_INT + kc.STATE_F32:
                check_equal(td[key], many[key].cpu(), f"n{n} k16 {name} {key}")
        assert wide.stride(2) == 1 and wide[:, :, 3:3 + 2 * a_w:2].stride(2) == 2


@pytest.mark.parametrize("k", [2, 3])
def test_action_layouts_and_shared_instances(k):
    """Step-major [T, B, A] slices of a padded buffer, a [B, T, A] buffer viewed step-major,
    and 4 instances shared by 12 rows (locs_batch < batch) through the C ABI."""
    n, b, t, lb = 21, 12, 3, 4
    locs, rec, g = kc.instance(b, n, 77, lb=lb)
    acts = kc.actions_for(g, rec, k, t)
    a_w = acts.shape[2]
    env = kc.product_env(n, k, DEV)
    full = locs.repeat(b // lb, 1, 1)
    want = kc.product_state(full, rec, DEV)
    want_r = env.improve_steps(want, acts.to(DEV))
    padded = torch.full((t, b, a_w + 5), -9, dtype=torch.int64, device=DEV)
    padded[:, :, 2:2 + a_w] = acts.to(DEV)
    row_major = acts.permute(1, 0, 2).contiguous().to(DEV).permute(1, 0, 2)
    for name, view in (("padded", padded[:, :, 2:2 + a_w]), ("row-major", row_major)):
        assert not view.is_contiguous()
        td = kc.product_state(full, rec, DEV)
        check_equal(env.improve_steps(td, view), want_r.cpu(), name + " rewards")
        for key in kc.STATE_INT + kc.STATE_F32:
            check_equal(td[key], want[key].cpu(), f"{name} {key}")
    # locs_batch < batch: row b reads instance b % 4
    dl, dr = locs.to(DEV).contiguous(), rec.to(DEV).contiguous()
    best, da = dr.clone(), acts.to(DEV).contiguous()
    cost, bsf = torch.empty(b, device=DEV), want["cost_bsf"].new_empty(b)
    vt = torch.empty((b, n), dtype=torch.int64, device=DEV)
    i = torch.zeros(b, 1, dtype=torch.int64, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    s = nat.stream_of(dr)
    nat.call("co_tsp_kopt_reset", b, n, nat.ptr(dl), lb, nat.ptr(dr), nat.ptr(bsf), None,
             nat.ptr(status), s)
    rew = torch.empty((t, b), device=DEV)
    per = torch.empty((t, b), device=DEV)
    nat.call("co_tsp_kopt_steps", b, n, k, t, nat.ptr(dl), lb, nat.ptr(da), *da.stride(),
             nat.ptr(dr), nat.ptr(cost), nat.ptr(bsf), nat.ptr(best), nat.ptr(vt), nat.ptr(i),
             nat.ptr(rew), nat.ptr(per), nat.ptr(status), s)
    assert int(status.item()) == 0
    check_equal(rew, want_r.cpu(), "locs_batch rewards")
    check_equal(per[-1], want["cost_current"].cpu(), "per-step cost")
    for key, got in (("rec_current", dr), ("rec_best", best), ("visited_time", vt), ("i", i),
                     ("cost_current", cost), ("cost_bsf", bsf)):
        check_equal(got, want[key].cpu(), "locs_batch " + key)


@pytest.mark.parametrize("n", [5, 64, 65])
def test_two_opt_special_moves(n):
    """first == second, second == pred(first) (the whole tour turns round) and a path that
    holds node 0, against the restatement; the no-op keeps the cost's bits."""
    locs, rec, g = kc.instance(3, n, 5 + n)
    act = kc.two_opt_actions(g, rec, 1)[0]
    env = kc.product_env(n, 2, DEV)
    td = kc.product_state(locs, rec, DEV)
    before = td["cost_current"].clone()
    td["action"] = act.to(DEV)
    td = env.step(td)["next"]
    want = kopt_ref.step(kopt_ref.reset(locs, rec.clone()), act, 2)
    kc.check_state(td, want, f"n{n} special", kc.STEP_KEYS)
    check_equal(td["rec_current"][0], rec[0], "first == second")
    check_equal(td["cost_current"][0], before[0].cpu(), "no-op cost bits")
    assert float(td["reward"][0]) == 0.0
    check_equal(td["rec_current"][1], rec[1].argsort(), "whole-tour reversal")
    assert int(td["visited_time"][2, int(rec[2, 0])]) != 1  # node 0 was inside the path


@pytest.mark.parametrize("n", kc.PAIR_SIZES)
def test_every_two_opt_pair_on_the_device(n):
    """Every (first, second) of a seeded tour in one launch (B = N * N): the kernel's closed
    form from positions against the restatement's walk and the host build.  N = 65 and 129
    (B = 4225 and 16641) make the second and third trip of the 64-wide loops with every
    (pos[first], path length), wraps past position N - 1 with node 0 inside included."""
    pairs, locs, rec, want = kc.all_pairs(n)
    b = pairs.shape[0]
    host = kc.product_state(locs, rec, "cpu")
    host["action"] = pairs
    host = kc.product_env(n, 2, "cpu").step(host)["next"]
    env = kc.product_env(n, 2, DEV)
    td = kc.product_state(locs, rec, DEV)
    td["action"] = pairs.to(DEV)
    td = env.step(td)["next"]
    kc.check_state(td, want, f"n{n} pairs", kc.STEP_KEYS)
    for key in kc.STATE_INT:
        check_equal(td[key], host[key], f"n{n} pairs host {key}")
    many = kc.product_state(locs, rec, DEV)
    env.improve_steps(many, pairs.to(DEV)[None])
    for key in kc.STATE_INT + kc.STATE_F32:
        check_equal(many[key], td[key].cpu(), f"n{n} pairs fused {key}")


@pytest.mark.parametrize("k", [3, 4])
def test_small_tours_run_real_kopt_moves(k):
    """N = 3 and 4: the smallest k-opt shapes with moves that change the tour."""
    for n in (3, 4):
        locs, rec, g = kc.instance(9, n, 60 + n + k)
        acts = kc.kopt_actions(g, rec, k, 4)
        want, _ = kopt_ref.steps(kopt_ref.reset(locs, rec.clone()), acts, k)
        assert (want["rec_current"] != rec).any(), "no move changed a tour"
        env = kc.product_env(n, k, DEV)
        td = kc.product_state(locs, rec, DEV)
        env.improve_steps(td, acts.to(DEV))
        kc.check_state(td, want, f"k{k} n{n}")


@pytest.mark.parametrize("k,n", [(3, 6), (4, 70), (16, 70)])
def test_kopt_result_that_is_no_cycle_sets_invalid_tour(k, n):
    """rec[a] = a (index = left = right = a) is a self loop: kopt_walk's result is not one
    N-cycle.  Only row 1 is spoilt; through the C ABI the bit is set and the other rows'
    outputs are the restatement's."""
    b = 3
    locs, rec, g = kc.instance(b, n, 90 + n)
    acts = kc.kopt_actions(g, rec, k, 1)[0]
    acts[1] = 2
    assert not kopt_ref.is_cycle(kopt_ref.k_opt(rec, acts, k))[1]
    want = kopt_ref.step(kopt_ref.reset(locs, rec.clone()), acts, k)
    td = kc.product_state(locs, rec, DEV)
    out = {"rec_current": torch.full((b, n), -1, dtype=torch.int64, device=DEV),
           "cost_current": torch.empty(b, device=DEV), "cost_bsf": torch.empty(b, device=DEV),
           "reward": torch.empty(b, device=DEV), "rec_best": td["rec_best"],
           "visited_time": torch.empty((b, n), dtype=torch.int64, device=DEV),
           "i": torch.empty((b, 1), dtype=torch.int64, device=DEV)}
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    da, dl = acts.to(DEV), td["locs"].contiguous()
    nat.call("co_tsp_kopt_step", b, n, k, nat.ptr(dl), b, nat.ptr(td["rec_current"]), nat.ptr(da),
             *da.stride(), nat.ptr(out["rec_current"]), nat.ptr(out["cost_current"]),
             nat.ptr(td["cost_bsf"]), nat.ptr(out["cost_bsf"]), nat.ptr(out["reward"]),
             nat.ptr(out["rec_best"]), nat.ptr(out["visited_time"]), nat.ptr(td["i"]),
             nat.ptr(out["i"]), nat.ptr(status), nat.stream_of(da))
    assert int(status.item()) == nat.ST_INVALID_TOUR
    good = [0, 2]
    for key in kc.STEP_KEYS:
        (check_equal if want[key].dtype == torch.int64 else check_close)(
            out[key].cpu()[good], want[key][good], f"k{k} n{n} valid rows' {key}")
    env = kc.product_env(n, k, DEV)
    td = kc.product_state(locs, rec, DEV)
    td["action"] = da
    with pytest.raises(AssertionError, match="Not visiting all nodes"):
        env.step(td)
    with pytest.raises(AssertionError, match="Not visiting all nodes"):
        env.improve_steps(kc.product_state(locs, rec, DEV), da[None])


def test_step_to_solution_and_entry_points():
    n, b = 37, 5
    locs, rec, g = kc.instance(b, n, 3)
    env = kc.product_env(n, 3, DEV)
    td = kc.product_state(locs, rec, DEV)
    tour = torch.rand(b, n, generator=g).argsort(1)
    ll = ImprovementEnvBase._get_linked_list_solution(tour.to(DEV).t().contiguous().t())
    check_equal(ll, kopt_ref.linked_list(tour), "linked list (step-major tour)")
    i_before = td["i"]
    td = env.step_to_solution(td, ll)
    want = kopt_ref.step(kopt_ref.reset(locs, rec.clone()), None, 3, solution_to=kopt_ref.linked_list(tour))
    kc.check_state(td, want, "step_to_solution", kc.STEP_KEYS)
    assert td["i"] is i_before
    check_equal(ImprovementEnvBase._get_real_solution(ll), kopt_ref.real_solution(ll.cpu()), "order")
    check_close(ImprovementEnvBase.get_costs(locs.to(DEV), ll), kopt_ref.costs(locs, ll.cpu()), "costs")
    gen = TSPGenerator(num_loc=n, init_sol_type="greedy")
    for m, bb in ((n, b), (130, 3)):
        l2 = torch.rand(bb, m, 2, generator=g)
        gen.num_loc = m
        check_equal(gen._get_initial_solutions(l2.to(DEV)), kopt_ref.nearest_rec(l2), f"greedy n{m}")


def test_invalid_rows_only_set_their_status_bit():
    n, b = 70, 4
    locs, rec, _ = kc.instance(b, n, 8)
    bad_rec = rec.clone()
    bad_rec[1, 5] = bad_rec[1, 6]  # two nodes lead to one
    bad_rec[2, 0] = n + 3          # out of range
    dl, dr = locs.to(DEV), bad_rec.to(DEV)
    cost = torch.full((b,), -1.0, device=DEV)
    vt = torch.full((b, n), -1, dtype=torch.int64, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    nat.call("co_tsp_kopt_reset", b, n, nat.ptr(dl), b, nat.ptr(dr), nat.ptr(cost), nat.ptr(vt),
             nat.ptr(status), nat.stream_of(dr))
    assert int(status.item()) == nat.ST_INVALID_TOUR
    good = [0, 3]
    check_close(cost[good], kopt_ref.costs(locs, rec)[good], "valid rows' cost")
    check_equal(vt[good], kopt_ref.visited_time(rec)[good], "valid rows' visited_time")
    env = kc.product_env(n, 2, DEV)
    td = kc.product_state(locs, rec, DEV)
    td["action"] = torch.tensor([[0, 1], [2, n], [3, 4], [5, 6]], device=DEV)
    with pytest.raises(RuntimeError, match="index out of range"):
        env.step(td)
    with pytest.raises(AssertionError, match="Not visiting all nodes"):
        ImprovementEnvBase._get_real_solution(dr)
