"""The k-opt improvement env of TSP (TSPkoptEnv, ``tsp_kopt``) without a GPU: the
restatement tests/kopt_ref.py and the host build of the C ABI are held to the recording of
the reference's own TSPkoptEnv (tests/golden/kopt/ref_kopt.npz: integers bit for bit, costs
and rewards within the project's 1e-5 relative), the host build to the restatement on every
2-opt pair of one tour at N = 3..6, 65 and 129 and on k_max = 5, 8, 15, 16 (CO_KOPT_MAX_K) at
N = 20, 65, 130, and the Python surface (registry, td contract, in-place
``rec_best``, status bits, argument errors, bindings) is checked."""
import os
import re
import subprocess
import sys

import pytest
import torch

import kopt_cases as kc
import kopt_ref
from ref_recordings import check_close, check_equal

import rl4co_slap_amd as ra
from rl4co_slap_amd import TensorDict, _native as nat
from rl4co_slap_amd.envs import (ENV_REGISTRY, IMPROVEMENT_ENV_REGISTRY, ImprovementEnvBase,
                                 TSPGenerator, TSPkoptEnv, get_env)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KOPT_SYMBOLS = ("co_tsp_linked_list", "co_tsp_real_solution", "co_tsp_kopt_reset",
                "co_tsp_kopt_step", "co_tsp_kopt_steps", "co_tsp_nearest_rec")


@pytest.mark.parametrize("case", kc.recorded_cases())
def test_restatement_matches_the_recording(case):
    r = kc.recorded(case)
    k = r["k_max"]
    state = kopt_ref.reset(r["locs"], r["reset_rec_current"])
    kc.check_state(state, {key: r["reset_" + key] for key in kc.STATE_INT + kc.STATE_F32},
                   case + " reset")
    if case.endswith("greedy"):
        check_equal(kopt_ref.nearest_rec(r["locs"]), r["reset_rec_current"], case + " greedy")
    live = kc.clear_rows(r)
    for t in range(r["step_action"].shape[0]):
        state = kopt_ref.step(state, r["step_action"][t], k)
        kc.check_recorded(state, r, "step_", live[t], f"{case} step {t}", t=t)
    rows = live[-1]
    check_equal(kopt_ref.real_solution(state["rec_best"])[rows], r["best_solution"][rows],
                "best solution")
    check_equal(kopt_ref.real_solution(state["rec_current"]), r["current_solution"],
                "current solution")
    check_equal(kopt_ref.linked_list(r["tour"]), r["linked_list"], "linked list")
    state = kopt_ref.step(state, None, k, solution_to=r["linked_list"])
    off = (r["to_solution_cost_current"] - r["step_cost_bsf"][-1]).abs() \
        >= kc.MARGIN * r["step_cost_bsf"][-1]
    kc.check_recorded(state, r, "to_solution_", rows & off, case + " step_to_solution")


@pytest.mark.parametrize("case", kc.recorded_cases())
def test_host_build_matches_the_recording(case):
    kc.check_recorded_case(case, "cpu")


TIE_CASES = ("k2n5_random", "k3n5_random", "k4n5_random", "k2n20_random")


def test_recording_holds_every_case_and_meets_its_condition():
    """All twelve cases are there.  Outside TIE_CASES every recorded row-step is a no-op or
    clear of the best-so-far cost by 1e-4; in TIE_CASES (small tours, where moves that only
    turn the tour round are frequent) the margins are stored and a row's best-so-far keys are
    compared up to its first row-step that is not clear (the counts are printed)."""
    want = {f"k{k}n{n}_random" for k in (2, 3, 4) for n in (5, 20, 65)} | \
        {f"k{k}n20_greedy" for k in (2, 3, 4)}
    assert set(kc.recorded_cases()) == want
    for case in sorted(want):
        r = kc.recorded(case)
        assert r["step_action"].shape[:2] == (12, 16) and r["step_margin"].shape == (12, 16)
        live = kc.clear_rows(r)
        if case in TIE_CASES:
            assert not live.all(), case + " has no tie: record it under the strict rule"
            print(case, "row-steps with best-so-far keys compared:", int(live.sum()), "of 192")
        else:
            assert live.all(), case


def test_recording_is_what_the_reference_returns(tmp_path):
    """With a reference checkout at hand ($RL4CO_REFERENCE): re-record in a child process
    and compare with the committed archive."""
    env = dict(os.environ, PYTHONPATH=ROOT, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    probe = subprocess.run([sys.executable, "-c",
                            "from oracle import reference as r; print(int(r.available()))"],
                           cwd=ROOT, env=env, capture_output=True, text=True, check=True)
    if probe.stdout.strip() != "1":
        pytest.skip("no reference checkout (set RL4CO_REFERENCE)")
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "record_kopt.py"),
                    "--out", str(tmp_path)], cwd=ROOT, env=env, check=True, capture_output=True)
    new = kc.recording.__wrapped__(str(tmp_path))
    old = kc.recording()
    assert sorted(new) == sorted(old)
    for key in old:
        if old[key].dtype.kind == "f":
            check_close(torch.from_numpy(new[key].copy()), torch.from_numpy(old[key].copy()), key)
        else:
            assert (new[key] == old[key]).all(), key


@pytest.mark.parametrize("n", kc.PAIR_SIZES)
def test_every_two_opt_pair(n):
    """Every (first, second) on a seeded tour: the host build against the restatement.  At
    N = 65 and 129 every (pos[first], path length) occurs with the path wrapping past
    position N - 1 and node 0 inside it."""
    pairs, locs, rec, want = kc.all_pairs(n)
    env = kc.product_env(n, 2, "cpu")
    td = kc.product_state(locs, rec, "cpu")
    assert kopt_ref.is_cycle(want["rec_current"]).all()
    td["action"] = pairs
    td = env.step(td)["next"]
    kc.check_state(td, want, f"n{n} pairs", kc.STEP_KEYS)
    same = pairs[:, 0] == pairs[:, 1]
    check_equal(td["rec_current"][same], rec[same], "first == second is a no-op")


@pytest.mark.parametrize("k", [2, 3, 4])
def test_noop_step_keeps_the_cost_bits(k):
    locs, rec, _ = kc.instance(5, 11, 7)
    env = kc.product_env(11, k, "cpu")
    td = kc.product_state(locs, rec, "cpu")
    before = td["cost_current"].clone()
    td["action"] = torch.full((5, 2), 3) if k == 2 else kc.noop_action(rec, k)
    td = env.step(td)["next"]
    check_equal(td["rec_current"], rec, "rec")
    check_equal(td["cost_current"], before, "cost bits")
    check_equal(td["reward"], torch.zeros(5), "reward")
    check_equal(td["i"], torch.ones(5, 1, dtype=torch.int64), "i")


@pytest.mark.parametrize("k,n,t", [(2, 9, 5), (3, 9, 5), (4, 23, 7), (2, 65, 3), (3, 6, 0)])
def test_improve_steps_equals_single_steps(k, n, t):
    locs, rec, g = kc.instance(6, n, 100 + n)
    acts = kc.actions_for(g, rec, k, t)
    env = kc.product_env(n, k, "cpu")
    one, many = kc.product_state(locs, rec, "cpu"), kc.product_state(locs, rec, "cpu")
    rewards = []
    for a in acts:
        one["action"] = a
        one = env.step(one)["next"]
        rewards.append(one["reward"])
    best_alias = many["rec_best"]
    got = env.improve_steps(many, acts.permute(1, 0, 2).contiguous().permute(1, 0, 2))
    assert many["rec_best"] is best_alias and got.shape == (t, 6)
    for key in kc.STATE_INT + kc.STATE_F32:
        check_equal(many[key], one[key], f"k{k} n{n} {key}")
    if t:
        check_equal(got, torch.stack(rewards), "rewards")
        want, _ = kopt_ref.steps(kopt_ref.reset(locs, rec.clone()), acts, k)
        kc.check_state(many, want, f"k{k} n{n} restatement")


@pytest.mark.parametrize("k,n", kc.HIGH_K)
def test_k_max_up_to_the_largest_against_the_restatement(k, n):
    """5 <= k_max <= CO_KOPT_MAX_K (16: all of the walk's right-node scratch, an action row
    48 wide): single steps and improve_steps against the restatement; every row moves."""
    locs, rec, acts, after = kc.high_k_case(k, n)
    assert acts.shape == (3, 8, 3 * k)
    assert (after[-1]["rec_current"] != rec).any(1).all(), "a row's tour did not change"
    env = kc.product_env(n, k, "cpu")
    td = kc.product_state(locs, rec, "cpu")
    rewards = []
    for t, a in enumerate(acts):
        td["action"] = a
        td = env.step(td)["next"]
        kc.check_state(td, after[t], f"k{k} n{n} step {t}", kc.STEP_KEYS)
        rewards.append(td["reward"])
    many = kc.product_state(locs, rec, "cpu")
    got = env.improve_steps(many, acts)
    kc.check_state(many, after[-1], f"k{k} n{n} improve_steps")
    check_close(got, torch.stack([s["reward"] for s in after]), "rewards")
    check_equal(got, torch.stack(rewards), "fused against single rewards")
    for key in kc.STATE_INT + kc.STATE_F32:
        check_equal(many[key], td[key], f"k{k} n{n} fused against single {key}")


def test_registry_and_td_contract():
    assert set(ENV_REGISTRY) == {"tsp", "cvrp", "slap"}
    assert IMPROVEMENT_ENV_REGISTRY == {"tsp_kopt": TSPkoptEnv}
    assert ra.TSPkoptEnv is TSPkoptEnv and ra.ImprovementEnvBase is ImprovementEnvBase
    env = get_env("tsp_kopt", generator_params=dict(num_loc=7), k_max=3, device="cpu")
    assert isinstance(env, TSPkoptEnv) and env.name == "tsp_kopt" and not env.two_opt_mode
    with pytest.raises(ValueError):
        get_env("ffsp")
    td = env.reset(batch_size=[4])
    want = {"locs": (torch.float32, (4, 7, 2)), "cost_current": (torch.float32, (4,)),
            "cost_bsf": (torch.float32, (4,)), "rec_current": (torch.int64, (4, 7)),
            "rec_best": (torch.int64, (4, 7)), "visited_time": (torch.int64, (4, 7)),
            "i": (torch.int64, (4, 1)), "done": (torch.bool, (4, 1)),
            "terminated": (torch.bool, (4, 1))}
    assert set(td.keys()) == set(want)
    for key, (dtype, shape) in want.items():
        assert td[key].dtype == dtype and tuple(td[key].shape) == shape, key
    assert kopt_ref.is_cycle(td["rec_current"]).all() and not td["done"].any()
    check_equal(td["visited_time"], kopt_ref.visited_time(td["rec_current"]), "visited_time")


def test_initial_solutions():
    gen = TSPGenerator(num_loc=9)
    locs = torch.rand(5, 9, 2)
    torch.manual_seed(3)
    rec = gen._get_initial_solutions(locs)
    torch.manual_seed(3)
    check_equal(rec, kopt_ref.linked_list(torch.rand(5, 9).argsort()), "random")
    gen = TSPGenerator(num_loc=9, init_sol_type="greedy")
    check_equal(gen._get_initial_solutions(locs), kopt_ref.nearest_rec(locs), "greedy")
    with pytest.raises(NotImplementedError):
        TSPGenerator(num_loc=9, init_sol_type="other")._get_initial_solutions(locs)


def test_rec_best_is_updated_in_place_on_improving_rows_only():
    locs, rec, g = kc.instance(8, 12, 5)
    env = kc.product_env(12, 2, "cpu")
    td = kc.product_state(locs, rec, "cpu")
    best = td["rec_best"]
    before = best.clone()
    td["action"] = kc.two_opt_actions(g, rec, 1, special=False)[0]
    td = env.step(td)["next"]
    better = td["reward"] > 0
    assert td["rec_best"] is best and better.any() and not better.all()
    check_equal(best[better], td["rec_current"][better], "improved rows")
    check_equal(best[~better], before[~better], "other rows")


def test_status_bits_and_messages():
    locs, rec, _ = kc.instance(3, 6, 9)
    env = kc.product_env(6, 2, "cpu")
    td = kc.product_state(locs, rec, "cpu")
    td["action"] = torch.tensor([[0, 1], [2, 6], [3, 4]])
    with pytest.raises(RuntimeError, match="index out of range"):
        env.step(td)
    td = kc.product_state(locs, rec, "cpu")
    td["action"] = torch.tensor([[0, 1], [-1, 2], [3, 4]])
    with pytest.raises(RuntimeError, match="index out of range"):
        env.improve_steps(td, td["action"][None])
    two_cycles = torch.tensor([[1, 0, 3, 4, 5, 2]] * 3)
    for fn in (lambda: ImprovementEnvBase.get_costs(locs, two_cycles),
               lambda: ImprovementEnvBase._get_real_solution(two_cycles),
               lambda: ImprovementEnvBase._get_real_solution(torch.tensor([[1, 2, 3, 4, 5, 9]])),
               lambda: ImprovementEnvBase._get_linked_list_solution(torch.tensor([[0, 1, 1]]))):
        with pytest.raises(AssertionError) as exc:
            fn()
        assert str(exc.value) == "Not visiting all nodes"
    td = kc.product_state(locs, rec, "cpu")
    with pytest.raises(AssertionError, match="Not visiting all nodes"):
        env.step_to_solution(td, two_cycles)
    env.check_solution_validity(td)
    td["rec_best"] = torch.tensor([[1, 2, 3, 4, 5, 5]] * 3)  # the reference's test: a permutation
    with pytest.raises(AssertionError, match="Not visiting all nodes"):
        env.check_solution_validity(td)
    # a 3-opt action whose result is not one cycle
    env3 = kc.product_env(6, 3, "cpu")
    td = kc.product_state(locs, rec, "cpu")
    a = torch.tensor([[0, 0, 0]])
    td["action"] = torch.cat((a, a, a), 1).expand(3, 9)  # rec[0] = 0: a self loop
    with pytest.raises(AssertionError, match="Not visiting all nodes"):
        env3.step(td)
    # the same at k_max = CO_KOPT_MAX_K, one row spoilt
    locs, rec, g = kc.instance(3, 20, 9)
    acts = kc.kopt_actions(g, rec, 16, 1)[0]
    acts[1] = 2
    assert kopt_ref.is_cycle(kopt_ref.k_opt(rec, acts, 16)).tolist() == [True, False, True]
    td = kc.product_state(locs, rec, "cpu")
    td["action"] = acts
    with pytest.raises(AssertionError, match="Not visiting all nodes"):
        kc.product_env(20, 16, "cpu").step(td)


def test_argument_errors_and_the_empty_batch():
    host = nat.load_host()
    big = nat.KOPT_MAX_N + 1
    assert host.co_tsp_kopt_reset(1, big, *([None] * 1), 1, *([None] * 5)) == -1
    assert host.co_tsp_linked_list(1, big, None, 1, 1, None, None, None) == -1
    assert host.co_tsp_real_solution(1, big, None, None, None, None) == -1
    assert host.co_tsp_nearest_rec(1, big, None, None, None) == -1
    assert host.co_tsp_kopt_step(1, big, 2, None, 1, None, None, 0, 0, *([None] * 11)) == -1
    assert host.co_tsp_kopt_steps(1, big, 2, 1, None, 1, None, 0, 0, 0, *([None] * 10)) == -1
    assert host.co_tsp_kopt_steps(1, 5, 17, 1, None, 1, None, 0, 0, 0, *([None] * 10)) == -1
    assert host.co_tsp_kopt_steps(1, 5, 2, 1, None, 1, None, 0, 0, 0, *([None] * 10)) == -1  # NULLs
    assert host.co_tsp_kopt_reset(0, 5, None, 1, *([None] * 5)) == 0
    assert host.co_tsp_kopt_step(0, 5, 2, None, 1, None, None, 0, 0, *([None] * 11)) == 0
    assert host.co_tsp_kopt_steps(0, 5, 2, 3, None, 1, None, 0, 0, 0, *([None] * 10)) == 0
    assert host.co_tsp_linked_list(0, 5, None, 1, 1, None, None, None) == 0
    with pytest.raises(ValueError):
        TSPkoptEnv(generator_params=dict(num_loc=5), k_max=1, device="cpu")
    env = kc.product_env(5, 2, "cpu")
    td = env.reset(batch_size=[0])
    assert td["rec_current"].shape == (0, 5) and td["cost_current"].shape == (0,)


def test_header_native_and_fastcall_bindings():
    header = open(os.path.join(ROOT, "include", "co_env.h")).read()
    declared = set(re.findall(r"\bint\s+(co_\w+)\s*\(", header))
    for name in KOPT_SYMBOLS:
        assert name in declared and name in nat._SIGS and name in nat.HOST_SYMBOLS, name
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header).group(1)
        assert len(nat._SIGS[name]) == decl.count(",") + 1, name
        assert hasattr(nat.load_host(), name)
    assert f"#define CO_KOPT_MAX_N {nat.KOPT_MAX_N}" in header
    assert f"#define CO_KOPT_MAX_K {nat.KOPT_MAX_K}" in header
    # k_max = CO_KOPT_MAX_K is taken and one more is CO_E_INVAL: decided before the empty
    # batch returns and before any launch, so the device library answers without a device
    assert nat.KOPT_MAX_K == 16
    p = torch.zeros(64, dtype=torch.int64).data_ptr()
    for lib in (nat.load_host(), nat.load()):
        for k, want in ((2, 0), (nat.KOPT_MAX_K, 0), (nat.KOPT_MAX_K + 1, -1), (1, -1)):
            assert lib.co_tsp_kopt_steps(0, 5, k, 1, None, 1, None, 0, 0, 0, *([None] * 10)) == want
            assert lib.co_tsp_kopt_step(0, 5, k, None, 1, None, p, 0, 0, *([None] * 11)) == want
    fast = nat._fastcall()
    assert fast is not None
    for name in KOPT_SYMBOLS:
        kinds = fast.table("host")[name][1]
        assert len(kinds) == len(nat._SIGS[name]) and set(kinds) <= set(b"i"), name
