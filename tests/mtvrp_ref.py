"""Restatement of the MTVRP entries of include/co_env.h in numpy, written from the header
(not from the kernels): every f32 operation is a numpy float32 array operation, so each is
rounded on its own, and the distance is the header's ``sqrt(dx*dx + dy*dy)``.  The device and
the host build are held to it bit for bit (tests/mtvrp_cases.py).

An instance is a dict of numpy arrays: ``locs [B, NC, 2]``, ``time_windows [B, NC, 2]``,
``service_time``, ``demand_linehaul``, ``demand_backhaul`` ``[B, NC]``, ``vehicle_capacity``,
``speed``, ``distance_limit`` ``[B]`` (f32) and ``open_route [B]`` (bool).  A state adds
``cur [B]`` (i64), ``time``, ``length``, ``used_l``, ``used_b`` ``[B]`` (f32), ``visited [B,
NC]`` (u8) and, after a mask call, ``action_mask [B, NC]``; a step adds ``done`` and
``reward``."""
import numpy as np

F = np.float32
ST_INVALID_TOUR, ST_INDEX_RANGE = 1, 8
ST_LIMIT_NEGATIVE, ST_TW_NEGATIVE, ST_SERVICE_NEGATIVE = 2048, 4096, 8192
ST_TW_INFEASIBLE, ST_DEPOT_RETURN, ST_ROUTE_LIMIT = 16384, 32768, 65536
ST_DEADLINE, ST_OVER_LINEHAUL, ST_OVER_BACKHAUL = 131072, 262144, 524288
INSTANCE = ("locs", "time_windows", "service_time", "demand_linehaul", "demand_backhaul",
            "vehicle_capacity", "speed", "distance_limit", "open_route")


def dist(p, q):
    dx = (p[..., 0] - q[..., 0]).astype(F)
    dy = (p[..., 1] - q[..., 1]).astype(F)
    return np.sqrt((dx * dx + dy * dy).astype(F)).astype(F)


def tmax(p, s):
    """torch.max: NaN when either operand is NaN."""
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(p) | np.isnan(s), F(np.nan), np.where(p > s, p, s)).astype(F)


def can_columns(st, d_ij, d_j0, tws, twe, svc, dl, db, vis):
    """can[c] before the depot column's overwrite, for column values of any common shape
    ``[B, ...]``; the row scalars are broadcast over the trailing axes."""
    def row(x):
        return np.asarray(x).reshape((-1,) + (1,) * (d_ij.ndim - 1))

    nopen = row((~st["open_route"]).astype(F))
    speed, cap = row(st["speed"]), row(st["vehicle_capacity"])
    with np.errstate(invalid="ignore", divide="ignore"):
        arr = (row(st["time"]) + (d_ij / speed).astype(F)).astype(F)
        reach = arr < twe
        back = ((tmax(arr, tws) + svc).astype(F) + (d_j0 / speed).astype(F)).astype(F)
        depot_ok = (back * nopen).astype(F) < row(st["time_windows"][:, 0, 1])
        over = ((row(st["length"]) + d_ij).astype(F) + (d_j0 * nopen).astype(F)).astype(F) \
            > row(st["distance_limit"])
        lhm = row(((st["visited"] == 0) & (st["demand_linehaul"] > 0)).any(1))
        rows = np.arange(len(st["cur"]))
        cbh = row(st["demand_backhaul"][rows, np.clip(st["cur"], 0, st["locs"].shape[1] - 1)] > 0)
        dem = (lhm & ~((dl + row(st["used_l"])).astype(F) > cap) & ~cbh & (dl > 0)) \
            | (~((db + row(st["used_b"])).astype(F) > cap) & (db > 0))
    return reach & depot_ok & dem & ~over & ~vis


def mask(st):
    """get_action_mask on the state: fills action_mask."""
    nc = st["locs"].shape[1]
    rows = np.arange(st["locs"].shape[0])
    cl = st["locs"][rows, np.clip(st["cur"], 0, nc - 1)]
    d_ij = dist(cl[:, None, :], st["locs"])
    d_j0 = dist(st["locs"], st["locs"][:, :1, :])
    can = can_columns(st, d_ij, d_j0, st["time_windows"][..., 0], st["time_windows"][..., 1],
                      st["service_time"], st["demand_linehaul"], st["demand_backhaul"],
                      st["visited"] != 0)
    can[:, 0] = ~((st["cur"] == 0) & can[:, 1:].any(1))
    st["action_mask"] = can
    return st


def reset(inst):
    b, nc = inst["locs"].shape[:2]
    st = dict(inst)
    st.update(cur=np.zeros(b, np.int64), time=np.zeros(b, F), length=np.zeros(b, F),
              used_l=np.zeros(b, F), used_b=np.zeros(b, F), visited=np.zeros((b, nc), np.uint8))
    return mask(st)


def step(st, a):
    """One step on a copy of the state; returns (state, status bits).  A row whose action is
    outside 0..N keeps its whole state."""
    st = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()}
    b, nc = st["locs"].shape[:2]
    rows = np.arange(b)
    a = np.asarray(a, np.int64)
    bad = (a < 0) | (a >= nc)
    ac = np.clip(a, 0, nc - 1)
    m01 = (a != 0).astype(F)
    leg = dist(st["locs"][rows, np.clip(st["cur"], 0, nc - 1)], st["locs"][rows, ac])
    with np.errstate(invalid="ignore", divide="ignore"):
        arrive = (st["time"] + (leg / st["speed"]).astype(F)).astype(F)
        time = (m01 * (tmax(arrive, st["time_windows"][rows, ac, 0])
                       + st["service_time"][rows, ac]).astype(F)).astype(F)
        length = (m01 * (st["length"] + leg).astype(F)).astype(F)
        used_l = (m01 * (st["used_l"] + st["demand_linehaul"][rows, ac]).astype(F)).astype(F)
        used_b = (m01 * (st["used_b"] + st["demand_backhaul"][rows, ac]).astype(F)).astype(F)
    for key, new in (("time", time), ("length", length), ("used_l", used_l), ("used_b", used_b),
                     ("cur", a)):
        st[key] = np.where(bad, st[key], new).astype(st[key].dtype)
    st["visited"][rows[~bad], a[~bad]] = 1
    st["done"] = (st["visited"] != 0).sum(1) == nc
    st["reward"] = np.zeros(b, F)
    return mask(st), (ST_INDEX_RANGE if bad.any() else 0)


def steps(st, actions):
    """T steps with actions [T, B]: (state, feasible, time, length -- each [T, B] --,
    status)."""
    nc = st["locs"].shape[1]
    rows = np.arange(st["locs"].shape[0])
    feasible, times, lengths, status = [], [], [], 0
    for a in np.asarray(actions, np.int64):
        bad = (a < 0) | (a >= nc)
        feasible.append(st["action_mask"][rows, np.clip(a, 0, nc - 1)] & ~bad)
        st, bits = step(st, a)
        status |= bits
        times.append(st["time"].copy())
        lengths.append(st["length"].copy())
    return st, np.stack(feasible), np.stack(times), np.stack(lengths), status


def reward(inst, actions):
    """co_mtvrp_reward for actions [B, T]: legs summed in f64, rounded once, negated."""
    locs, out = inst["locs"], []
    for r in range(locs.shape[0]):
        acc, prev = 0.0, 0
        for a in list(np.asarray(actions[r], np.int64)) + [0]:
            if not (a == 0 and inst["open_route"][r]):
                acc += float(dist(locs[r, prev], locs[r, a]))
            prev = a
        out.append(-F(acc))
    return np.array(out, F)


def check(inst, actions):
    """The status bits of co_mtvrp_check for actions [B, T], per row ([B] int)."""
    locs, tw, svc = inst["locs"], inst["time_windows"], inst["service_time"]
    b, nc = locs.shape[:2]
    d0 = dist(locs, locs[:, :1, :])
    out = np.zeros(b, np.int64)
    with np.errstate(invalid="ignore"):
        for r in range(b):
            acts = np.asarray(actions[r], np.int64)
            bits = 0
            rng = bool(((acts < 0) | (acts >= nc)).any())
            cust = acts[(acts > 0) & (acts < nc)]
            if rng:
                bits |= ST_INDEX_RANGE
            if rng or len(cust) != nc - 1 or len(set(cust.tolist())) != nc - 1:
                bits |= ST_INVALID_TOUR
            lim, cap = inst["distance_limit"][r], inst["vehicle_capacity"][r]
            if not lim >= 0:
                bits |= ST_LIMIT_NEGATIVE
            if not (tw[r] >= 0).all():
                bits |= ST_TW_NEGATIVE
            if not (svc[r] >= 0).all():
                bits |= ST_SERVICE_NEGATIVE
            if not (tw[r, :, 0] < tw[r, :, 1]).all():
                bits |= ST_TW_INFEASIBLE
            if not (((tw[r, :, 0] + d0[r]).astype(F) + svc[r]).astype(F) <= tw[r, 0, 1]).all():
                bits |= ST_DEPOT_RETURN
            if not rng:
                t = length = ul = ub = F(0)
                prev = 0
                for a in acts:
                    d = dist(locs[r, prev], locs[r, a])
                    length = F(length + F(d * F(0 if (inst["open_route"][r] and a == 0) else 1)))
                    if not length <= lim:
                        bits |= ST_ROUTE_LIMIT
                    if a == 0:
                        length = F(0)
                    t = F(tmax(np.asarray(F(t + d)), tw[r, a, 0]))
                    if not t <= tw[r, a, 1]:
                        bits |= ST_DEADLINE
                    t = F(t + svc[r, a])
                    if a == 0:
                        t = F(0)
                    m01 = F(a != 0)
                    ul = F(F(ul * m01) + inst["demand_linehaul"][r, a])
                    ub = F(F(ub * m01) + inst["demand_backhaul"][r, a])
                    if not ul <= cap:
                        bits |= ST_OVER_LINEHAUL
                    if not ub <= cap:
                        bits |= ST_OVER_BACKHAUL
                    prev = a
            out[r] = bits
    return out
