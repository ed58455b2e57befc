"""Restatement of the CVRPTW entries of include/co_env.h in numpy, written from the header
(not from the kernels): every f32 operation is a numpy float32 array operation, so each is
rounded on its own, and the distance is the header's ``sqrt(dx*dx + dy*dy)``.  The device
and the host build are held to it bit for bit (tests/cvrptw_cases.py).

A state is a dict of numpy arrays: ``locs [B, NC, 2]``, ``demand [B, N]``, ``used [B]``,
``cap [B]``, ``visited [B, NC]`` (u8), ``cur [B]`` (i64), ``time [B]``, ``durations [B, NC]``
and ``time_windows [B, NC, 2]`` (f32 / i32 / i64), and after a mask call ``current_loc [B,
2]``, ``distances [B, NC]``, ``action_mask [B, NC]``; a step adds ``done`` and ``reward``."""
import numpy as np

F = np.float32
ST_INDEX_RANGE = 8
ST_TW_NEGATIVE, ST_TW_DEPOT_RETURN, ST_DURATION_NEGATIVE = 64, 128, 256
ST_TW_INFEASIBLE, ST_TW_DEADLINE = 512, 1024


def f32(x):
    """The plain cast to f32 on load."""
    return np.asarray(x).astype(F)


def dist(p, q):
    dx = (p[..., 0] - q[..., 0]).astype(F)
    dy = (p[..., 1] - q[..., 1]).astype(F)
    return np.sqrt((dx * dx + dy * dy).astype(F)).astype(F)


def tmax(p, s):
    """torch.max: NaN when either operand is NaN."""
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(p) | np.isnan(s), F(np.nan), np.where(p > s, p, s)).astype(F)


def trunc(x):
    """The reference's ``.int()``: toward zero; -2^31 for a NaN or a value outside int32."""
    with np.errstate(invalid="ignore"):
        ok = (x >= F(-2147483648.0)) & (x < F(2147483648.0))
        return np.where(ok, np.trunc(x), F(-2147483648.0)).astype(F)


def cvrp_mask(st):
    open_c = (st["visited"][:, 1:] == 0) & ~((st["demand"] + st["used"][:, None]).astype(F)
                                             > st["cap"][:, None])
    dep = ~((st["cur"] == 0) & open_c.any(1))
    return np.concatenate((dep[:, None], open_c), 1)


def reach(time, d, tw):
    with np.errstate(invalid="ignore"):
        return (time[:, None] + d).astype(F) <= f32(tw[..., 1])


def mask(st):
    """get_action_mask on the state: fills current_loc, distances, action_mask."""
    n = st["demand"].shape[1]
    rows = np.arange(st["locs"].shape[0])
    cl = st["locs"][rows, np.clip(st["cur"], 0, n)]
    d = dist(cl[:, None, :], st["locs"])
    st["current_loc"], st["distances"] = cl, d
    st["action_mask"] = cvrp_mask(st) & reach(st["time"], d, st["time_windows"])
    return st


def reset(depot, locs, demand, vcap, durations, time_windows):
    b, n = demand.shape
    st = {"locs": np.concatenate((depot[:, None, :], locs), 1).astype(F), "demand": f32(demand),
          "used": np.zeros(b, F), "cap": np.full(b, vcap, F),
          "visited": np.zeros((b, n + 1), np.uint8), "cur": np.zeros(b, np.int64),
          "time": np.zeros(b, F), "durations": durations, "time_windows": time_windows}
    return mask(st)


def step(st, a):
    """One step on a copy of the state; returns (state, status bits)."""
    st = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()}
    b, n = st["demand"].shape
    rows = np.arange(b)
    a = np.asarray(a, np.int64)
    bad = (a < 0) | (a > n)
    ac = np.clip(a, 0, n)
    m01 = (a != 0).astype(F)
    leg = st["distances"][rows, ac]
    arrive = (st["time"] + leg).astype(F)
    with np.errstate(invalid="ignore"):
        st["time"] = (m01 * (tmax(arrive, f32(st["time_windows"][rows, ac, 0]))
                             + f32(st["durations"][rows, ac])).astype(F)).astype(F)
    picked = st["demand"][rows, np.clip(a - 1, 0, n - 1)]
    st["used"] = ((st["used"] + picked).astype(F) * m01).astype(F)
    st["visited"][rows[~bad], a[~bad]] = 1
    st["cur"] = a
    st["done"] = st["visited"].sum(1) == n + 1
    st["reward"] = np.zeros(b, bool)
    return mask(st), (ST_INDEX_RANGE if bad.any() else 0)


def steps(st, actions):
    """T steps with actions [T, B]: (state, feasible [T, B], time [T, B], status)."""
    n = st["demand"].shape[1]
    rows = np.arange(st["demand"].shape[0])
    feasible, times, status = [], [], 0
    for a in np.asarray(actions, np.int64):
        bad = (a < 0) | (a > n)
        feasible.append(st["action_mask"][rows, np.clip(a, 0, n)] & ~bad)
        st, bits = step(st, a)
        status |= bits
        times.append(st["time"].copy())
    return st, np.stack(feasible), np.stack(times), status


def check(locs, actions, durations, time_windows):
    """The status bits of co_cvrptw_check for actions [B, T]."""
    b, nc = locs.shape[:2]
    tw, dur = f32(time_windows), f32(durations)
    d0 = dist(locs[:, :1, :], locs)
    bits = 0
    with np.errstate(invalid="ignore"):
        if (tw < 0).any():
            bits |= ST_TW_NEGATIVE
        if not (((tw[..., 0] + d0).astype(F) + dur).astype(F) <= tw[0, 0, 1]).all():
            bits |= ST_TW_DEPOT_RETURN
        if (dur < 0).any():
            bits |= ST_DURATION_NEGATIVE
        if not (tw[..., 0] < tw[..., 1]).all():
            bits |= ST_TW_INFEASIBLE
        for r in range(b):
            t, prev = F(0), 0
            for a in np.asarray(actions[r], np.int64):
                if a < 0 or a >= nc:
                    bits |= ST_INDEX_RANGE
                    break
                d = dist(locs[r, prev], locs[r, a])
                t = tmax(trunc(np.asarray(t + d, F)), tw[r, a, 0])
                if not t <= tw[r, a, 1]:
                    bits |= ST_TW_DEADLINE
                t = F(t + dur[r, a])
                if a == 0:
                    t = F(0)
                prev = a
    return bits
