"""numpy restatement of the PDP section of include/co_env.h (reset, step, preset steps with
``feasible``, reward, the two validity bits), written from the header alone: the host build
and the kernels are held to it bit for bit.  Not a test module."""
import numpy as np

ST_INDEX_RANGE = 8
ST_NOT_ALL_NODES = 1048576
ST_PRECEDENCE = 2097152


def reset(depot, locs_in):
    """-> the reset state of ``depot [B, 2]`` / ``locs_in [B, N, 2]`` (N even)."""
    b, n = locs_in.shape[:2]
    nc, h = n + 1, n // 2
    cols = np.arange(nc)
    return {"locs": np.concatenate((depot[:, None, :], locs_in), axis=1).astype(np.float32),
            "to_deliver": np.broadcast_to(cols <= h, (b, nc)).copy(),
            "available": np.ones((b, nc), dtype=bool),
            "action_mask": np.broadcast_to(cols == 0, (b, nc)).copy(),
            "current_node": np.zeros((b, 1), dtype=np.int64),
            "i": np.zeros((b, 1), dtype=np.int64),
            "done": np.zeros((b, 1), dtype=bool), "terminated": np.zeros((b, 1), dtype=bool)}


def step(state, action):
    """One step on ``state`` (available, to_deliver, i; left untouched) -> (the new state,
    status bits).  An action outside 0..N edits neither row."""
    av, td = state["available"] != 0, state["to_deliver"] != 0
    b, nc = av.shape
    n, h = nc - 1, (nc - 1) // 2
    a = np.asarray(action, dtype=np.int64)
    ok = (a >= 0) & (a <= n)
    rows = np.nonzero(ok)[0]
    av, td = av.copy(), td.copy()
    av[rows, a[rows]] = False
    td[rows, (a[rows] + h) % nc] = True
    out = {"available": av, "to_deliver": td, "action_mask": av & td,
           "done": ~av.any(axis=1), "reward": np.zeros(b, dtype=bool),
           "i": state["i"] + 1, "current_node": a[:, None].copy()}
    return out, (0 if ok.all() else ST_INDEX_RANGE)


def steps(state, actions):
    """``actions [T, B]`` as T steps from ``state`` (which also holds the caller's
    ``action_mask``) -> (the final state, feasible [T, B], status bits)."""
    actions = np.asarray(actions, dtype=np.int64)
    t_steps, b = actions.shape
    n = state["available"].shape[1] - 1
    feasible = np.zeros((t_steps, b), dtype=bool)
    cur = dict(state)
    mask = state["action_mask"] != 0
    bits = 0
    for t in range(t_steps):
        a = actions[t]
        ok = (a >= 0) & (a <= n)
        feasible[t] = ok & mask[np.arange(b), np.where(ok, a, 0)]
        cur, st = step(cur, a)
        mask = cur["action_mask"]
        bits |= st
    return cur, feasible, bits


def _edge(p, q):
    """dist(p, q): f32, every operation rounded on its own."""
    dx = np.float32(q[0]) - np.float32(p[0])
    dy = np.float32(q[1]) - np.float32(p[1])
    return np.sqrt(np.float32(np.float32(dx * dx) + np.float32(dy * dy)), dtype=np.float32)


def reward(locs, actions, check=False):
    """``locs [LB, NC, 2]``, ``actions [B, T]`` -> (reward [B] f32, status bits)."""
    locs = np.asarray(locs, dtype=np.float32)
    actions = np.asarray(actions, dtype=np.int64)
    b, t_steps = actions.shape
    lb, nc = locs.shape[:2]
    n, t2 = nc - 1, t_steps // 2
    out = np.zeros(b, dtype=np.float32)
    bits = 0
    for r in range(b):
        lr = locs[r % lb]
        prev, total = lr[0], 0.0
        seen = np.zeros(t_steps, dtype=bool)
        dup = prec = False
        for a in actions[r].tolist():
            if 0 <= a <= n:
                if prev is not None:
                    total += float(_edge(prev, lr[a]))
                prev = lr[a]
            else:
                bits |= ST_INDEX_RANGE
                prev = None
            if check:
                if a < 0 or a >= t_steps or seen[a]:
                    dup = True
                else:
                    if a > t2 and not seen[a - t2]:
                        prec = True
                    seen[a] = True
        if prev is not None:
            total += float(_edge(prev, lr[0]))
        out[r] = -np.float32(total)
        if check and dup:
            bits |= ST_NOT_ALL_NODES
        elif check and prec:
            bits |= ST_PRECEDENCE
    return out, bits


def check_reference(actions):
    """The reference's two asserts in its own words (sort / argsort) on ``actions [B, T]``
    with T odd -> status bits per row; what ``reward``'s scan in tour order must equal."""
    actions = np.asarray(actions, dtype=np.int64)
    b, t_steps = actions.shape
    t2 = t_steps // 2
    out = np.zeros(b, dtype=np.int64)
    for r in range(b):
        if not np.array_equal(np.sort(actions[r]), np.arange(t_steps)):
            out[r] = ST_NOT_ALL_NODES
            continue
        pos = np.argsort(actions[r], kind="stable")
        if not (pos[1:t2 + 1] < pos[t2 + 1:]).all():
            out[r] = ST_PRECEDENCE
    return out
