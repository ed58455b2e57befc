"""Shared inputs and checks of tests/test_host_kopt.py and tests/test_gpu_kopt.py: the
recording tests/golden/kopt/ref_kopt.npz, seeded instances, valid k-opt actions, the cases
for k_max = 5, 8, 15, 16 (HIGH_K) and every 2-opt pair of one tour (PAIR_SIZES) with the
restatement's results, and the comparison of a product state with a restatement
(tests/kopt_ref.py) state."""
import functools
import os

import numpy as np
import torch

import kopt_ref
from ref_recordings import check_close, check_equal

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kopt")
STATE_INT = ("rec_current", "rec_best", "visited_time", "i")
STATE_F32 = ("cost_current", "cost_bsf")
STEP_KEYS = ("rec_current", "visited_time", "cost_current", "cost_bsf", "reward", "rec_best", "i")
BSF_KEYS = ("cost_bsf", "reward", "rec_best")  # what depends on the improvement test
MARGIN = 1e-4


@functools.lru_cache(maxsize=None)
def recording(directory=GOLDEN):
    with np.load(os.path.join(directory, "ref_kopt.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def recorded_cases():
    return sorted({k.split("/")[1] for k in recording()})


def recorded(case, directory=GOLDEN):
    """One case: uint8 index arrays back as int64, strings as str, 0-d ints as int."""
    out = {}
    for k, v in recording(directory).items():
        if k.split("/")[1] != case:
            continue
        name = k.split("/", 2)[2]
        if v.dtype.kind == "U":
            out[name] = str(v)
        elif v.ndim == 0 and v.dtype.kind in "iu":
            out[name] = int(v)
        else:
            t = torch.from_numpy(v.copy())
            out[name] = t.long() if t.dtype == torch.uint8 else t
    assert out, case
    return out


def clear_rows(r):
    """[T, B] bool: every row-step of the row up to and including step t is clear (a no-op,
    or its cost at least 1e-4 relative off the best-so-far cost: the recorder's condition).
    The best-so-far keys of a row are compared while this holds; a 1e-5 difference in the
    summation cannot flip an improvement test there."""
    return (r["step_margin"] >= MARGIN).long().cumprod(0).bool()


def check_recorded(got, r, prefix, rows, what, keys=STEP_KEYS, t=None):
    """``got[key]`` against the recorded ``prefix + key`` (step ``t`` of a stacked array):
    the best-so-far keys on ``rows`` only, the others on every row; integers bit for bit,
    floats within 1e-5 relative."""
    for key in keys:
        want = r[prefix + key] if t is None else r[prefix + key][t]
        g = got[key].cpu()
        if key in BSF_KEYS:
            g, want = g[rows], want[rows]
        (check_close if want.is_floating_point() else check_equal)(g, want, f"{what} {key}")


def instance(b, n, seed, lb=None):
    g = torch.Generator().manual_seed(seed)
    locs = torch.rand(lb or b, n, 2, generator=g)
    tour = torch.rand(b, n, generator=g).argsort(1)
    return locs, kopt_ref.linked_list(tour), g


def noop_action(rec, k):
    """A k-opt action that re-adds an edge of the tour: index = left = a, right = rec[a]."""
    a = torch.zeros(rec.shape[0], k, dtype=torch.int64)
    return torch.cat((a, a, rec.gather(1, a)), 1)


def kopt_actions(g, rec, k, t):
    """[T, B, 3k] sequential k-opt moves on the evolving ``rec`` (CPU): a_0 anywhere, a_1 <
    ... < a_{k-1} further along the tour; left = a_0, rec[a_0], ..., rec[a_{k-2}]; right =
    a_1, ..., a_{k-1}, rec[a_{k-1}].  On a small tour (N <= 8), where that scheme has few or
    no moves, a row without a valid one tries random in-range actions and takes the first
    that gives another N-cycle.  A row left without a valid move gets the no-op, so every
    step of every row is valid."""
    b, n = rec.shape
    out = []
    for _ in range(t):
        order = kopt_ref.real_solution(rec)
        start = torch.randint(0, n, (b, 1), generator=g)
        if n - 1 >= k - 1 and n > k:
            offs = torch.rand(b, n - 2, generator=g).argsort(1)[:, :k - 1].sort(1).values + 1
        else:
            offs = torch.ones(b, k - 1, dtype=torch.int64)
        pos = torch.cat((start, (start + offs) % n), 1)
        idx = order.gather(1, pos)
        nxt = rec.gather(1, idx)
        act = torch.cat((idx, idx[:, :1], nxt[:, :-1], idx[:, 1:], nxt[:, -1:]), 1)
        new = kopt_ref.k_opt(rec, act, k)
        ok = kopt_ref.is_cycle(new)
        if n <= 8:  # a proposal that leaves the tour as it is does not count there
            ok &= (new != rec).any(1)
        for _ in range(64 if n <= 8 else 0):
            cand = torch.randint(0, n, (b, 3 * k), generator=g)
            moved = kopt_ref.k_opt(rec, cand, k)
            take = ~ok & kopt_ref.is_cycle(moved) & (moved != rec).any(1)
            act = torch.where(take[:, None], cand, act)
            new = torch.where(take[:, None], moved, new)
            ok |= take
        act = torch.where(ok[:, None], act, noop_action(rec, k))
        rec = torch.where(ok[:, None], new, rec)
        out.append(act)
    return torch.stack(out) if out else torch.zeros(0, b, 3 * k, dtype=torch.int64)


HIGH_K = [(k, n) for k in (5, 8, 15, 16) for n in (20, 65, 130)]  # up to CO_KOPT_MAX_K


@functools.lru_cache(maxsize=None)
def high_k_case(k, n, b=8, t=3):
    """(locs, rec, acts [T, B, 3k], the restatement's state after every step) of a seeded
    case for 5 <= k_max <= 16, computed once and shared: do not write to it.  The conditions
    on the inputs hold for the restatement alone: every row's tour changes, and every
    row-step is clear by the recorder's rule (a no-op, or the new cost at least MARGIN
    relative off the best-so-far cost), so no improvement test hangs on the summation order;
    a seed that misses either is passed over."""
    for seed in range(2000 * k + n, 2000 * k + n + 1000, 100):
        locs, rec, g = instance(b, n, seed)
        acts = kopt_actions(g, rec, k, t)
        state, after, clear = kopt_ref.reset(locs, rec.clone()), [], True
        for a in acts:
            bsf, before = state["cost_bsf"], state["rec_current"]
            state = kopt_ref.step(state, a, k)
            same = (state["rec_current"] == before).all(1)
            margin = (state["cost_current"] - bsf).abs() / bsf
            clear &= bool((same | (margin >= MARGIN)).all())
            after.append({key: v.clone() for key, v in state.items()})
        if clear and bool((state["rec_current"] != rec).any(1).all()):
            return locs, rec, acts, after
    raise AssertionError(f"k{k} n{n}: no seed moves every row with every row-step clear")


PAIR_SIZES = [3, 4, 5, 6, 65, 129]  # one lane does all the work; two and three trips of 64


@functools.lru_cache(maxsize=None)
def all_pairs(n):
    """Every (first, second) of one seeded tour as a batch of B = N * N rows: (pairs, locs,
    rec, the restatement's step), computed once and shared: do not write to it."""
    pairs = torch.tensor([(f, s) for f in range(n) for s in range(n)])
    b = pairs.shape[0]
    locs, rec, _ = instance(1, n, 40 + n)
    locs, rec = locs.expand(b, n, 2).contiguous(), rec.expand(b, n).contiguous()
    return pairs, locs, rec, kopt_ref.step(kopt_ref.reset(locs, rec.clone()), pairs, 2)


def two_opt_actions(g, rec, t, special=True):
    """[T, B, 2]: random pairs; with ``special`` the first rows of step 0 are first ==
    second, the whole-tour reversal (second = pred(first)) and a path across node 0."""
    b, n = rec.shape
    act = torch.randint(0, n, (t, b, 2), generator=g)
    if special and t:
        pred = rec.argsort(1)
        act[0, 0] = torch.tensor([n // 2, n // 2])
        if b > 1:
            act[0, 1] = torch.stack((torch.tensor(n - 1), pred[1, n - 1]))
        if b > 2:  # pred(0) -> rec[0]: node 0 inside the reversed path
            act[0, 2] = torch.stack((pred[2, 0], rec[2, 0]))
    return act


def actions_for(g, rec, k, t):
    return two_opt_actions(g, rec, t) if k == 2 else kopt_actions(g, rec, k, t)


def check_state(got, want, what, keys=STATE_INT + STATE_F32):
    for k in keys:
        g = got[k]
        if k in STATE_INT or want[k].dtype == torch.int64:
            check_equal(g, want[k].cpu(), f"{what} {k}")
        else:
            check_close(g, want[k].cpu(), f"{what} {k}")


def product_env(n, k, device, init="random"):
    from rl4co_slap_amd.envs import TSPkoptEnv

    return TSPkoptEnv(generator_params=dict(num_loc=n, init_sol_type=init), k_max=k,
                      device=device, seed=0)


def product_state(locs, rec, device):
    """A td as ``TSPkoptEnv.reset`` leaves it, from a given ``rec`` (through the C ABI)."""
    from rl4co_slap_amd import TensorDict
    from rl4co_slap_amd import _native as nat

    locs, rec = locs.to(device), rec.to(device).contiguous()
    b, n = rec.shape
    cost = torch.empty(b, dtype=torch.float32, device=device)
    vt = torch.empty((b, n), dtype=torch.int64, device=device)
    status = torch.zeros(1, dtype=torch.int32, device=device)
    lc = locs.contiguous()
    nat.call("co_tsp_kopt_reset", b, n, nat.ptr(lc), lc.shape[0], nat.ptr(rec), nat.ptr(cost),
             nat.ptr(vt), nat.ptr(status), nat.stream_of(rec))
    assert int(status.item()) == 0
    return TensorDict({"locs": locs, "rec_current": rec, "rec_best": rec.clone(),
                       "cost_current": cost, "cost_bsf": cost.clone(), "visited_time": vt,
                       "i": torch.zeros(b, 1, dtype=torch.int64, device=device)}, [b])


def check_recorded_case(case, device):
    """The product on ``device`` over one recorded episode: the reset under the recorded
    seed, every step, the solutions, step_to_solution, the costs and the mask."""
    import pytest
    from rl4co_slap_amd import TensorDict
    from rl4co_slap_amd.envs import ImprovementEnvBase

    r = recorded(case)
    b, n = r["locs"].shape[:2]
    k = r["k_max"]
    init = case.split("_")[1]
    env = product_env(n, k, device, init)
    torch.manual_seed(r["seed"])
    locs = torch.rand(b, n, 2)
    check_equal(locs, r["locs"], case + " locs")
    td = env.reset(TensorDict({"locs": locs}, [b]))
    for key in ("rec_current", "rec_best", "visited_time", "i"):
        check_equal(td[key], r["reset_" + key], f"{case} reset {key}")
    for key in ("cost_current", "cost_bsf"):
        check_close(td[key], r["reset_" + key], f"{case} reset {key}")
    for key in ("done", "terminated"):
        check_equal(td[key], torch.zeros(b, 1, dtype=torch.bool), f"{case} reset {key}")
    best_alias = td["rec_best"]
    live = clear_rows(r)
    for t in range(r["step_action"].shape[0]):
        td["action"] = r["step_action"][t].to(device)
        td = env.step(td)["next"]
        assert td["rec_best"] is best_alias  # updated in place
        check_recorded(td, r, "step_", live[t], f"{case} step {t}", t=t)
    rows = live[-1]
    check_equal(env.get_best_solution(td).cpu()[rows], r["best_solution"][rows],
                case + " best solution")
    check_equal(env.get_current_solution(td), r["current_solution"], case + " current solution")
    check_close(ImprovementEnvBase.get_costs(td["locs"], td["rec_best"]).cpu()[rows],
                r["costs_best"][rows], case + " get_costs")
    ll = ImprovementEnvBase._get_linked_list_solution(r["tour"].to(device))
    check_equal(ll, r["linked_list"], case + " linked list")
    td = env.step_to_solution(td, ll)
    # the recorded step_to_solution is one more row-step: clear when its cost is off the best
    off = (r["to_solution_cost_current"] - r["step_cost_bsf"][-1]).abs() >= MARGIN * r["step_cost_bsf"][-1]
    check_recorded(td, r, "to_solution_", rows & off, case + " step_to_solution")
    env.check_solution_validity(td)
    if k == 2:
        check_equal(env.get_mask(td), r["mask"], case + " mask")
    else:
        with pytest.raises(AssertionError) as exc:
            env.get_mask(td)
        assert str(exc.value) == r["mask_error"]
    with pytest.raises(NotImplementedError) as exc:
        env._get_reward(td, None)
    assert str(exc.value) == r["get_reward_error"]
