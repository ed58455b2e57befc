"""numpy restatement of the OP section of include/co_env.h (reset, the mask, step, preset
steps with ``feasible`` and ``length``, reward, the validity bits), written from the header
alone: the host build and the kernels are held to it bit for bit, floats included.  Every
f32 operation is one numpy f32 operation (rounded on its own, no FMA).  Not a test module."""
import numpy as np

ST_INDEX_RANGE = 8
ST_DUPLICATE = 4194304
ST_LENGTH = 8388608
ST_SINGLE_NONZERO = 16777216
F = np.float32
EPS6, EPS5 = F(1e-6), F(1e-5)


def dist(p, q):
    """dist(p, q) on arrays [..., 2]: f32, every operation rounded on its own."""
    p, q = np.asarray(p, dtype=F), np.asarray(q, dtype=F)
    dx, dy = p[..., 0] - q[..., 0], p[..., 1] - q[..., 1]
    with np.errstate(invalid="ignore", over="ignore"):
        return np.sqrt(dx * dx + dy * dy, dtype=F)


def _cur_loc(state):
    b, nc = state["visited"].shape
    cur = np.clip(state["current_node"].reshape(b), 0, nc - 1)
    return state["locs"][np.arange(b), cur]


def mask(state):
    """The mask of (visited, tour_length, current_node): false for a NaN compare."""
    vis = state["visited"] != 0
    with np.errstate(invalid="ignore"):
        exceeds = (state["tour_length"][:, None] + dist(state["locs"], _cur_loc(state)[:, None, :])
                   > state["max_length"])
    m = ~(vis | vis[:, :1] | exceeds)
    m[:, 0] = True
    return m


def reset(depot, locs_in, prize_in, max_length_in):
    """-> the reset state of ``depot [B,2]``, ``locs_in [B,N,2]``, ``prize_in [B,N]``,
    ``max_length_in [B]``."""
    depot, locs_in = np.asarray(depot, dtype=F), np.asarray(locs_in, dtype=F)
    b, n = locs_in.shape[:2]
    locs = np.concatenate((depot[:, None, :], locs_in), axis=1)
    st = {"locs": locs,
          "prize": np.concatenate((np.zeros((b, 1), dtype=F), np.asarray(prize_in, dtype=F)), 1),
          "max_length": (np.asarray(max_length_in, dtype=F)[:, None]
                         - dist(depot[:, None, :], locs)) - EPS6,
          "tour_length": np.zeros(b, dtype=F), "current_total_prize": np.zeros(b, dtype=F),
          "current_node": np.zeros((b, 1), dtype=np.int64), "i": np.zeros(b, dtype=np.int64),
          "visited": np.zeros((b, n + 1), dtype=bool)}
    st["action_mask"] = mask(st)
    return st


INSTANCE = ("locs", "prize", "max_length")


def step(state, action):
    """One step on ``state`` (left untouched) -> (the new state, status bits).  An action
    outside 0..N leaves visited, tour_length and current_total_prize unchanged."""
    vis = state["visited"] != 0
    b, nc = vis.shape
    a = np.asarray(action, dtype=np.int64).reshape(b)
    ok = (a >= 0) & (a <= nc - 1)
    ac = np.clip(a, 0, nc - 1)
    rows = np.arange(b)
    leg = dist(state["locs"][rows, ac], _cur_loc(state))
    with np.errstate(invalid="ignore"):
        tl = np.where(ok, state["tour_length"] + leg, state["tour_length"]).astype(F)
        pz = np.where(ok, state["current_total_prize"] + state["prize"][rows, ac],
                      state["current_total_prize"]).astype(F)
    vis = vis.copy()
    vis[rows[ok], a[ok]] = True
    out = {k: state[k] for k in INSTANCE}
    out.update({"visited": vis, "tour_length": tl, "current_total_prize": pz,
                "done": (a == 0) & (state["i"].reshape(b) > 0), "reward": np.zeros(b, dtype=bool),
                "i": state["i"].reshape(b) + 1, "current_node": a[:, None].copy()})
    out["action_mask"] = mask(out)
    return out, (0 if ok.all() else ST_INDEX_RANGE)


def steps(state, actions):
    """``actions [T, B]`` as T steps from ``state`` (which also holds the caller's
    ``action_mask``) -> (the final state, feasible [T, B], length [T, B], status bits)."""
    actions = np.asarray(actions, dtype=np.int64)
    t_steps, b = actions.shape
    n = state["visited"].shape[1] - 1
    feasible = np.zeros((t_steps, b), dtype=bool)
    length = np.zeros((t_steps, b), dtype=F)
    cur = dict(state)
    m = state["action_mask"] != 0
    bits = 0
    for t in range(t_steps):
        a = actions[t]
        ok = (a >= 0) & (a <= n)
        feasible[t] = ok & m[np.arange(b), np.where(ok, a, 0)]
        cur, st = step(cur, a)
        length[t] = cur["tour_length"]
        m = cur["action_mask"]
        bits |= st
    return cur, feasible, length, bits


def reward(prize, actions, locs=None, max_length=None, check=False):
    """``prize [PB, NC]``, ``actions [B, T]`` and, with ``check``, ``locs [LB, NC, 2]`` /
    ``max_length [LB, NC]`` -> (reward [B] f32, status bits)."""
    prize = np.asarray(prize, dtype=F)
    actions = np.asarray(actions, dtype=np.int64)
    b, t_steps = actions.shape
    pb, nc = prize.shape
    out = np.zeros(b, dtype=F)
    bits = 0
    for r in range(b):
        row = actions[r].tolist()
        total = 0.0
        for a in row:
            if 0 <= a < nc:
                total += float(prize[r % pb, a])
            else:
                bits |= ST_INDEX_RANGE
        out[r] = F(0) if t_steps == 1 else F(total)
        if t_steps == 1 and row[0] != 0:
            bits |= ST_SINGLE_NONZERO
        if not check:
            continue
        lr, ml = np.asarray(locs, dtype=F)[r % len(locs)], np.asarray(max_length, dtype=F)[r % len(locs)]
        inside = [a for a in row if 0 <= a < nc]
        custs = [a for a in inside if a != 0]
        if len(custs) != len(set(custs)):
            bits |= ST_DUPLICATE
            continue
        total = 0.0
        for t in range(t_steps):
            p, q = row[t], row[(t + 1) % t_steps]
            if 0 <= p < nc and 0 <= q < nc:
                total += float(dist(lr[p], lr[q]))
        bound = ((ml + dist(lr[:1], lr)) + EPS6) + EPS5
        with np.errstate(invalid="ignore"):
            if not (F(total) <= bound).all():
                bits |= ST_LENGTH
    return out, bits


def check_reference(actions, locs, max_length):
    """The reference's two asserts in its own words (sort; the closed tour against the
    bounds) on in-range ``actions [B, T]`` -> status bits per row."""
    actions = np.asarray(actions, dtype=np.int64)
    out = np.zeros(len(actions), dtype=np.int64)
    for r, row in enumerate(actions):
        s = np.sort(row)
        if not ((s[1:] == 0) | (s[1:] > s[:-1])).all():
            out[r] = ST_DUPLICATE
            continue
        pts = np.asarray(locs[r], dtype=F)[row]
        total = F(np.sum(dist(pts, np.roll(pts, -1, axis=0)).astype(np.float64)))
        bound = ((np.asarray(max_length[r], dtype=F) + dist(locs[r][:1], locs[r])) + EPS6) + EPS5
        if not (total <= bound).all():
            out[r] = ST_LENGTH
    return out
