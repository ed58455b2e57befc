"""Restatement of the k-opt improvement entries of include/co_env.h (co_tsp_linked_list,
co_tsp_real_solution, co_tsp_kopt_reset / _step / _steps, co_tsp_nearest_rec) in batched
torch ops, written from the header's semantics: the tests' second opinion, and the torch
baseline of tools/bench_kopt.py (it issues O(N) gather / scatter launches per step, as the
reference's ``TSPkoptEnv`` does, on whatever device its inputs live).  Not a test module.

A state is a dict with ``locs, rec_current, rec_best, cost_current, cost_bsf, visited_time,
i``; ``step`` returns a new dict and, like the reference, writes ``rec_best`` in place."""
import torch


def linked_list(tour):
    rec = torch.empty_like(tour)
    rec.scatter_(1, tour, tour.roll(-1, 1))
    return rec


def visited_time(rec):
    """The walk from node 0: rec[0] gets 1, the next node 2, ..., node 0 gets N."""
    b, n = rec.shape
    vt = torch.zeros_like(rec)
    cur = torch.zeros(b, 1, dtype=torch.int64, device=rec.device)
    for k in range(n):
        cur = rec.gather(1, cur)
        vt.scatter_(1, cur, k + 1)
    return vt


def real_solution(rec):
    return (visited_time(rec) % rec.shape[1]).argsort(1)


def is_cycle(rec):
    """Per row: rec is one N-cycle."""
    n = rec.shape[1]
    ok = ((rec >= 0) & (rec < n)).all(1)
    vt = visited_time(rec.clamp(0, n - 1))
    return ok & (vt.sort(1).values == torch.arange(1, n + 1, device=rec.device)).all(1)


def costs(locs, rec):
    """sum over nodes of the f32 sqrt(dx*dx + dy*dy), added in f64, rounded once."""
    nxt = locs.gather(1, rec.unsqueeze(-1).expand(-1, -1, 2))
    d = nxt - locs
    edge = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).sqrt()
    return edge.double().sum(1).float()


def two_opt(rec, action):
    """Reverse the path first -> ... -> second of every row."""
    b, n = rec.shape
    first, second = action[:, :1], action[:, 1:2]
    pred = rec.argsort(1)
    before, after = pred.gather(1, first), rec.gather(1, second)
    same, whole = first == second, before == second
    out = rec.clone()
    # turn the links round: walk back from second until first
    cur = second.clone()
    for _ in range(n - 1):
        live = cur != first
        p = pred.gather(1, cur)
        out.scatter_(1, cur, torch.where(live, p, out.gather(1, cur)))
        cur = torch.where(live, p, cur)
    out.scatter_(1, first, torch.where(whole, second, after))
    out.scatter_(1, before, torch.where(whole, out.gather(1, before), second))
    return torch.where(same, rec, out)


def k_opt(rec, action, k):
    """The walk of the header: action = index | left | right."""
    b, n = rec.shape
    index, left, right = action[:, :k], action[:, k:2 * k], action[:, 2 * k:]
    pred = rec.argsort(1)
    right_nodes = rec.gather(1, index)
    out = rec.clone()
    for j in range(k):  # in order: the last write wins
        out.scatter_(1, left[:, j:j + 1], right[:, j:j + 1])
    cur = left[:, :1].clone()
    for _ in range(n - 2):
        nxt = out.gather(1, cur)
        po = pred.gather(1, nxt)
        turn = (po != cur) & ~(nxt == right_nodes).any(1, keepdim=True)
        out.scatter_(1, nxt, torch.where(turn, po, out.gather(1, nxt)))
        cur = nxt
    return out


def operator(rec, action, k_max):
    return two_opt(rec, action) if k_max == 2 else k_opt(rec, action, k_max)


def reset(locs, rec):
    cost = costs(locs, rec)
    return {"locs": locs, "rec_current": rec, "rec_best": rec.clone(), "cost_current": cost,
            "cost_bsf": cost.clone(), "visited_time": visited_time(rec),
            "i": torch.zeros(rec.shape[0], 1, dtype=torch.int64, device=rec.device)}


def step(state, action, k_max, solution_to=None):
    nxt = operator(state["rec_current"], action, k_max) if solution_to is None \
        else solution_to.clone()
    cost = costs(state["locs"], nxt)
    bsf = torch.where(cost < state["cost_bsf"], cost, state["cost_bsf"])
    reward = state["cost_bsf"] - bsf
    better = reward > 0
    state["rec_best"][better] = nxt[better]
    return {"locs": state["locs"], "rec_current": nxt, "rec_best": state["rec_best"],
            "cost_current": cost, "cost_bsf": bsf, "visited_time": visited_time(nxt),
            "i": state["i"] + 1 if solution_to is None else state["i"], "reward": reward}


def steps(state, actions, k_max):
    rewards = []
    for a in actions:
        state = step(state, a, k_max)
        rewards.append(state["reward"])
    return state, torch.stack(rewards) if rewards else torch.empty(0, state["rec_best"].shape[0])


def nearest_rec(locs):
    """Nearest-neighbour tour from node 0 as a linked list: visited nodes count as 1e5, the
    first minimum wins."""
    b, n, _ = locs.shape
    rec = torch.zeros(b, n, dtype=torch.int64, device=locs.device)
    seen = torch.zeros(b, n, dtype=torch.bool, device=locs.device)
    cur = torch.zeros(b, 1, dtype=torch.int64, device=locs.device)
    seen.scatter_(1, cur, True)
    for _ in range(n - 1):
        d = locs - locs.gather(1, cur.unsqueeze(-1).expand(-1, 1, 2))
        dist = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).sqrt()
        dist[seen] = 1e5
        # the first minimum: min over the indices that hold it
        idx = torch.arange(n, device=locs.device).expand(b, n)
        nxt = torch.where(dist == dist.min(1, keepdim=True).values, idx, n).min(1, keepdim=True).values
        rec.scatter_(1, cur, nxt)
        seen.scatter_(1, nxt, True)
        cur = nxt
    return rec


def random_two_opt_actions(gen, t, b, n):
    """[T, B, 2] with first != second."""
    first = torch.randint(0, n, (t, b, 1), generator=gen)
    second = (first + torch.randint(1, n, (t, b, 1), generator=gen)) % n
    return torch.cat((first, second), -1)
