"""The second grid-stride pass of the six one-row-per-workgroup kernels: tsp_ls_kernel,
cvrp_ls_kernel, slap_ls_kernel (table scheme), kopt_kernel (k_max = 2 and 3),
linked_list_kernel and nearest_rec_kernel.  ``row_grid`` caps the grid at 2^22 workgroups, so
with B = 2^22 + 64 rows workgroup j < 64 takes row j and then row 2^22 + j on the LDS state the
first row left: the barrier before the row's first LDS write, the re-zeroed bitmaps, the
``continue`` of an invalid row, k-opt's per-row ``dirty`` / ``best`` and CVRP's rebuilt m.

The batch is an index gather, on the device, of a table of 96 distinct rows at the smallest
sizes with real work (TSP N = 5 with both operators; CVRP N = 3, T = 5; SLAP P = 3, L = 5, O =
K = 2; k-opt, linked list and nearest tour N = 5), each solved once on the CPU by the
restatements; every row has its own instance (locs_batch == batch), and the expected output
is the same gather of the table's results, compared on the device.  Table row r has kind r %
4 -- 0 and 3: a valid row that moves (k-opt: whose step improves), 1: a valid row without an
improving move (k-opt: a step that does not improve, ``rec_best`` back as given), 2: an
invalid row -- row b < 2^22 is table row b % 96 and row 2^22 + j is table row (j + 1) % 96, so
each workgroup's second row is of the next kind; the pairings are asserted from the table's
flags before any launch.  The status word is the OR of the table's bits."""
import functools

import numpy as np
import pytest
import torch

import cvrp_ls_cases as cvc
import cvrp_ls_ref
import kopt_cases as kc
import kopt_ref
import slap_ls_ref
import tsp_ls_ref
from two_opt_ref import dist_from_locs

from rl4co_slap_amd import _native as nat
from rl4co_slap_amd.utils import ops

pytestmark = pytest.mark.gpu

GRID = 1 << 22  # row_grid's cap (csrc/co_local_search.hpp)
TAIL = 64       # workgroups that take a second row
ROWS = 96       # the table; 24 of each kind
MOVES, STILL, INVALID, MOVES_TOO = 0, 1, 2, 3


def kind(r):
    return r % 4


def batch_index(device, grid=GRID):
    """[grid + TAIL] table rows: b % ROWS, then (j + 1) % ROWS for the second pass."""
    return torch.cat((torch.arange(grid, device=device) % ROWS,
                      (torch.arange(TAIL, device=device) + 1) % ROWS))


def check_pairings(valid, moved, inputs, searches=True):
    """From the table alone: what row GRID + j is to row j, the row its workgroup took first."""
    first = np.arange(TAIL) % ROWS
    second = (np.arange(TAIL) + 1) % ROWS
    v1, v2 = valid[first], valid[second]
    differs = np.zeros(TAIL, bool)
    for a in inputs:
        a = np.asarray(a).reshape(ROWS, -1)
        differs |= (a[first] != a[second]).any(1)
    assert (v1 & v2 & differs).any(), "no valid row after a valid row of another instance"
    if valid.all():
        return
    assert (~v1 & v2).any(), "no valid row after an invalid one"
    assert (v1 & ~v2).any(), "no invalid row after a valid one"
    if searches:
        assert (v1 & moved[first] & v2 & ~moved[second]).any(), "no still row after one that moved"


def tiled(table, idx, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(table)) if isinstance(table, np.ndarray) else table
    t = t.to(idx.device)
    return (t if dtype is None else t.to(dtype)).index_select(0, idx)


def same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, got.dtype)
    assert torch.equal(got, want), what


def close(got, want, what):
    """ref_recordings.check_close on the device: 1e-5 of max(|want|, 1)."""
    assert got.shape == want.shape and got.dtype == want.dtype, what
    assert bool(((got - want).abs() <= 1e-5 * want.abs().clamp(min=1)).all()), what


def status_of(device):
    return torch.zeros(1, dtype=torch.int32, device=device)


def _pool(draw, solve, count):
    """``count`` drawn inputs that ``solve`` marks as moved, with their results."""
    out = []
    for _ in range(100 * count):
        x = draw()
        res = solve(x)
        if res["moved"]:
            out.append((x, res))
            if len(out) == count:
                return out
    raise AssertionError("too few rows with an improving move")


def _search_table(draw, solve, still_of, spoil, copy_of):
    """The 96 rows of a search: (inputs, results) per row.  ``still_of(x, res)`` is the input
    whose row is the result of x (a local optimum), ``spoil(x, r)`` an invalid version of x
    and ``copy_of(x)`` what an invalid row returns."""
    pool = _pool(draw, solve, ROWS // 2)
    rows = []
    for r in range(ROWS):
        x, res = pool[2 * (r // 4) + (kind(r) in (INVALID, MOVES_TOO))]
        if kind(r) == STILL:
            x = still_of(x, res)
            res = solve(x)
            assert res["valid"] and not res["moved"], "the result of a search is no local optimum"
        elif kind(r) == INVALID:
            x = spoil(x, r)
            res = solve(x)
            assert not res["valid"]
            res = dict(copy_of(x), valid=False, moved=False)
        rows.append((x, res))
    return rows


def _stack(rows, which, key, dtype):
    return np.stack([np.asarray(r[which][key], dtype=dtype) for r in rows])


def _flags(rows):
    return (np.array([r[1]["valid"] for r in rows]), np.array([r[1]["moved"] for r in rows]))


# ------------------------------------------------------------------ TSP local search
@functools.lru_cache(maxsize=None)
def tsp_table(n=5):
    rng = np.random.default_rng(11)

    def draw():
        return {"locs": rng.random((n, 2), dtype=np.float32), "tour": rng.permutation(n)}

    def solve(x):
        t = x["tour"]
        if sorted(int(v) for v in t) != list(range(n)):
            return {"valid": False, "moved": False}
        out, sweeps, moves, _ = tsp_ls_ref.local_search(
            dist_from_locs(x["locs"]), t, tsp_ls_ref.TWO_OPT | tsp_ls_ref.OR_OPT, 1000)
        return {"out": out, "sweeps": sweeps, "moves": moves, "valid": True,
                "moved": sum(moves) > 0}

    def spoil(x, r):
        t = x["tour"].copy()
        t[1 + r % 3] = t[0] if r % 8 < 4 else n  # a duplicate; an entry out of range
        return dict(x, tour=t)

    return _search_table(draw, solve, lambda x, res: dict(x, tour=res["out"]), spoil,
                         lambda x: {"out": x["tour"], "sweeps": 0, "moves": (0, 0)})


def check_tsp_local_search(device, grid=GRID):
    rows = tsp_table()
    valid, moved = _flags(rows)
    locs, tours = _stack(rows, 0, "locs", np.float32), _stack(rows, 0, "tour", np.int64)
    check_pairings(valid, moved, (locs, tours))
    used = {k: sum(r[1]["moves"][k] > 0 for r in rows) for k in (0, 1)}
    assert used[0] and used[1], "an operator applies no move in the table"
    idx = batch_index(device, grid)
    st = status_of(device)
    out, sweeps, moves = ops.tsp_local_search(
        tiled(tours, idx), locs=tiled(locs, idx), operators=("two_opt", "or_opt"),
        return_sweeps=True, return_moves=True, status=st)
    same(out, tiled(_stack(rows, 1, "out", np.int64), idx), "tours")
    same(sweeps, tiled(_stack(rows, 1, "sweeps", np.int32), idx), "sweeps")
    same(moves, tiled(_stack(rows, 1, "moves", np.int32), idx), "moves")
    assert int(st.item()) == nat.ST_INVALID_TOUR


def test_tsp_local_search_second_row(dev):
    check_tsp_local_search(dev)


# ------------------------------------------------------------------ CVRP local search
@functools.lru_cache(maxsize=None)
def cvrp_table(n=3, t=5):
    rng = np.random.default_rng(12)

    def draw():
        demand = cvc.demands(rng, 1, n, 20)[0]
        perm = rng.permutation(n) + 1
        row = cvc.split_tour(perm, demand) if rng.random() < 0.5 else \
            [int(perm[0]), 0, int(perm[1]), 0, int(perm[2])]
        return {"locs": rng.random((n + 1, 2), dtype=np.float32), "demand": demand,
                "tour": np.asarray(row + [0] * (t - len(row)), dtype=np.int64)}

    def solve(x):
        out, sweeps, _ = cvrp_ls_ref.local_search(cvrp_ls_ref.dist_from_locs(x["locs"]),
                                                  x["demand"], 1.0, x["tour"], 1000)
        if out is None:
            return {"valid": False, "moved": False}
        return {"out": out, "sweeps": sweeps, "valid": True, "moved": sweeps > 1}

    def spoil(x, r):
        row = x["tour"].copy()
        at = np.flatnonzero(row)
        row[at[1]] = row[at[0]] if r % 8 < 4 else n + 1  # a customer twice; out of range
        return dict(x, tour=row)

    return _search_table(draw, solve, lambda x, res: dict(x, tour=res["out"]), spoil,
                         lambda x: {"out": x["tour"], "sweeps": 0})


def check_cvrp_local_search(device, grid=GRID):
    rows = cvrp_table()
    valid, moved = _flags(rows)
    locs, demand = _stack(rows, 0, "locs", np.float32), _stack(rows, 0, "demand", np.float32)
    tours = _stack(rows, 0, "tour", np.int64)
    check_pairings(valid, moved, (locs, demand, tours))
    lengths = {int(np.count_nonzero(r[1]["out"])) + int((np.diff(np.flatnonzero(r[1]["out"])) > 1).sum())
               for r in rows if r[1]["valid"]}
    assert len(lengths) > 1, "every giant tour has the same length m"
    idx = batch_index(device, grid)
    st = status_of(device)
    out, sweeps = ops.cvrp_local_search(tiled(tours, idx), tiled(demand, idx),
                                        locs=tiled(locs, idx), return_sweeps=True, status=st)
    same(out, tiled(_stack(rows, 1, "out", np.int64), idx), "rows")
    same(sweeps, tiled(_stack(rows, 1, "sweeps", np.int32), idx), "sweeps")
    assert int(st.item()) == nat.ST_INVALID_TOUR


def test_cvrp_local_search_second_row(dev):
    check_cvrp_local_search(dev)


# ------------------------------------------------------------------ SLAP local search
@functools.lru_cache(maxsize=None)
def slap_table(p=3, slots=5, o=2, k=2):
    rng = np.random.default_rng(13)

    def draw():
        return {"locs": (rng.random((slots, 2), dtype=np.float32) * np.float32(10)).astype(np.float32),
                "picklist": rng.integers(0, p, size=(o, k)).astype(np.int64),
                "row": rng.permutation(slots)[:p].astype(np.int32)}

    def solve(x):
        out, sweeps, cost, _ = slap_ls_ref.local_search(slap_ls_ref.dist_from_locs(x["locs"]),
                                                        x["picklist"], x["row"], 1000, x["locs"])
        if out is None:
            return {"valid": False, "moved": False}
        return {"out": out, "sweeps": sweeps, "cost": cost, "valid": True, "moved": sweeps > 1}

    def spoil(x, r):
        row = x["row"].copy()
        row[1 + r % 2] = row[0] if r % 8 < 4 else slots  # a slot taken twice; out of range
        return dict(x, row=row)

    return _search_table(draw, solve, lambda x, res: dict(x, row=res["out"]), spoil,
                         lambda x: {"out": x["row"], "sweeps": 0, "cost": -1})


def check_slap_local_search(device, grid=GRID, scheme=nat.SLAP_LS_TABLE):
    rows = slap_table()
    valid, moved = _flags(rows)
    locs, pl = _stack(rows, 0, "locs", np.float32), _stack(rows, 0, "picklist", np.int64)
    start = _stack(rows, 0, "row", np.int32)
    check_pairings(valid, moved, (locs, pl, start))
    idx = batch_index(device, grid)
    st = status_of(device)
    out, sweeps, cost = ops.slap_local_search(
        tiled(start, idx), tiled(pl, idx), locs=tiled(locs, idx), return_sweeps=True,
        return_cost=True, status=st, scheme=scheme)
    same(out, tiled(_stack(rows, 1, "out", np.int32), idx), "rows")
    same(sweeps, tiled(_stack(rows, 1, "sweeps", np.int32), idx), "sweeps")
    same(cost, tiled(_stack(rows, 1, "cost", np.int64), idx), "cost")
    assert int(st.item()) == nat.ST_INVALID_TOUR


def test_slap_local_search_second_row(dev):
    assert nat.slap_ls_table_fits(3, 5)
    check_slap_local_search(dev)


# ------------------------------------------------------------------ k-opt step
@functools.lru_cache(maxsize=None)
def kopt_table(k, n=5):
    """Per row: an instance, a tour, a valid action, ``cost_bsf`` = the tour's cost and a
    ``rec_best`` that is some other tour.  Kinds 0 and 3: the step lowers the cost by at
    least kc.MARGIN relative (rec_best becomes the new tour); kind 1: the step changes the
    tour and raises the cost by as much (rec_best stays as given); kind 2: a rec_in that is
    no cycle or, at k = 3 on every other such row, a walk whose result is none."""
    g = torch.Generator().manual_seed(100 + k)
    c = 64 * ROWS
    locs = torch.rand(c, n, 2, generator=g)
    rec = kopt_ref.linked_list(torch.rand(c, n, generator=g).argsort(1))
    marker = kopt_ref.linked_list(torch.rand(c, n, generator=g).argsort(1))
    act = kc.two_opt_actions(g, rec, 1, special=False)[0] if k == 2 else kc.kopt_actions(g, rec, k, 1)[0]
    state = kopt_ref.reset(locs, rec.clone())
    state["rec_best"] = marker.clone()
    want = kopt_ref.step(state, act, k)
    assert kopt_ref.is_cycle(want["rec_current"]).all()
    changed = (want["rec_current"] != rec).any(1) & (marker != want["rec_current"]).any(1)
    margin = (want["cost_current"] - state["cost_bsf"]) / state["cost_bsf"]
    better = torch.nonzero(changed & (margin <= -kc.MARGIN))[:, 0].tolist()
    worse = torch.nonzero(changed & (margin >= kc.MARGIN))[:, 0].tolist()
    assert len(better) >= ROWS // 2 and len(worse) >= ROWS // 4, (len(better), len(worse))
    pick, valid = [], []
    for r in range(ROWS):
        q = r // 4
        pick.append(worse[q] if kind(r) == STILL else better[2 * q + (kind(r) != MOVES)])
        valid.append(kind(r) != INVALID)
    pick, valid = torch.tensor(pick), torch.tensor(valid)
    table = {"locs": locs[pick], "rec_in": rec[pick].clone(), "action": act[pick].clone(),
             "bsf_in": state["cost_bsf"][pick], "best_in": marker[pick],
             "i_in": torch.arange(ROWS)[:, None].clone()}
    for r in range(ROWS):
        if kind(r) != INVALID:
            continue
        if k > 2 and r % 8 >= 4:
            table["action"][r] = 2  # index = left = right = 2: a self loop
        else:
            table["rec_in"][r, 1 + r % 3] = table["rec_in"][r, 0]  # two nodes lead to one
            assert not kopt_ref.is_cycle(table["rec_in"][r:r + 1])[0]
    ok = valid.nonzero()[:, 0]
    for key, src in (("rec_out", "rec_current"), ("cost", "cost_current"), ("bsf_out", "cost_bsf"),
                     ("reward", "reward"), ("best_out", "rec_best"), ("vt", "visited_time")):
        table[key] = want[src][pick]
    table["i_out"] = table["i_in"] + 1
    # the restatement again on the table's own rows: what it holds is what a step gives
    again = kopt_ref.step({"locs": table["locs"][ok], "rec_current": table["rec_in"][ok],
                           "rec_best": table["best_in"][ok].clone(), "cost_bsf": table["bsf_in"][ok],
                           "i": table["i_in"][ok]}, table["action"][ok], k)
    for key, src in (("rec_out", "rec_current"), ("best_out", "rec_best"), ("reward", "reward")):
        assert torch.equal(again[src], table[key][ok]), key
    bad = (~valid).nonzero()[:, 0]
    spoilt = kopt_ref.operator(table["rec_in"][bad].clamp(0, n - 1), table["action"][bad], k)
    assert not (kopt_ref.is_cycle(table["rec_in"][bad]) & kopt_ref.is_cycle(spoilt)).any()
    improved = table["reward"] > 0
    assert bool((improved == torch.tensor([kind(r) in (MOVES, MOVES_TOO) for r in range(ROWS)]))[ok].all())
    keep = valid & ~improved
    assert torch.equal(table["best_out"][keep], table["best_in"][keep])
    assert bool((table["best_out"][keep] != table["rec_out"][keep]).any(1).all())
    return table, valid.numpy(), improved.numpy()


def check_kopt_step(device, k, grid=GRID):
    table, valid, improved = kopt_table(k)
    check_pairings(valid, improved, (table["locs"].numpy(), table["rec_in"].numpy(),
                                     table["action"].numpy()))
    first, second = np.arange(TAIL) % ROWS, (np.arange(TAIL) + 1) % ROWS
    assert (valid[first] & improved[first] & valid[second] & ~improved[second]).any()
    idx = batch_index(device, grid)
    b, n = idx.shape[0], table["rec_in"].shape[1]
    given = {key: tiled(table[key], idx) for key in ("locs", "rec_in", "action", "bsf_in",
                                                     "best_in", "i_in")}
    e = functools.partial(torch.empty, device=device)
    out = {"rec_out": torch.full((b, n), -7, dtype=torch.int64, device=device),
           "cost": e(b), "bsf_out": e(b), "reward": e(b), "best_out": given["best_in"],
           "vt": e((b, n), dtype=torch.int64), "i_out": e((b, 1), dtype=torch.int64)}
    st = status_of(device)
    act = given["action"]
    nat.call("co_tsp_kopt_step", b, n, k, nat.ptr(given["locs"]), b, nat.ptr(given["rec_in"]),
             nat.ptr(act), *act.stride(), nat.ptr(out["rec_out"]), nat.ptr(out["cost"]),
             nat.ptr(given["bsf_in"]), nat.ptr(out["bsf_out"]), nat.ptr(out["reward"]),
             nat.ptr(out["best_out"]), nat.ptr(out["vt"]), nat.ptr(given["i_in"]),
             nat.ptr(out["i_out"]), nat.ptr(st), nat.stream_of(act))
    assert int(st.item()) == nat.ST_INVALID_TOUR
    rows = tiled(torch.from_numpy(valid), idx).nonzero()[:, 0]  # an invalid row's outputs are unspecified
    for key in ("rec_out", "best_out", "vt", "i_out"):
        same(out[key].index_select(0, rows), tiled(table[key], idx).index_select(0, rows), key)
    for key in ("cost", "bsf_out", "reward"):
        close(out[key].index_select(0, rows), tiled(table[key], idx).index_select(0, rows), key)
    stays = tiled(torch.from_numpy(valid & ~improved), idx).nonzero()[:, 0]
    assert bool((stays >= grid).any())
    same(out["best_out"].index_select(0, stays),
         tiled(table["best_in"], idx).index_select(0, stays), "rec_best of a row without improvement")


@pytest.mark.parametrize("k", [2, 3])
def test_kopt_step_second_row(dev, k):
    check_kopt_step(dev, k)


# ------------------------------------------------------------------ linked list, nearest tour
@functools.lru_cache(maxsize=None)
def linked_list_table(n=5):
    g = torch.Generator().manual_seed(14)
    tour = torch.rand(ROWS, n, generator=g).argsort(1)
    want = kopt_ref.linked_list(tour)
    valid = torch.tensor([kind(r) != INVALID for r in range(ROWS)])
    for r in range(ROWS):
        if kind(r) == INVALID:
            tour[r, 1 + r % 4] = tour[r, 0] if r % 8 < 4 else n
            want[r] = -7  # not written
    return tour, want, valid.numpy()


def check_linked_list(device, grid=GRID):
    tour, want, valid = linked_list_table()
    check_pairings(valid, valid, (tour.numpy(),), searches=False)
    idx = batch_index(device, grid)
    t = tiled(tour, idx)
    rec = torch.full_like(t, -7)
    st = status_of(device)
    nat.call("co_tsp_linked_list", *t.shape, nat.ptr(t), *t.stride(), nat.ptr(rec), nat.ptr(st),
             nat.stream_of(t))
    same(rec, tiled(want, idx), "rec")
    assert int(st.item()) == nat.ST_INVALID_TOUR


def test_linked_list_second_row(dev):
    check_linked_list(dev)


@functools.lru_cache(maxsize=None)
def nearest_table(n=5):
    locs = torch.rand(ROWS, n, 2, generator=torch.Generator().manual_seed(15))
    want = kopt_ref.nearest_rec(locs)
    assert len({tuple(r) for r in want.tolist()}) > 8  # many different tours
    return locs, want


def check_nearest_rec(device, grid=GRID):
    locs, want = nearest_table()
    check_pairings(np.ones(ROWS, bool), np.ones(ROWS, bool), (locs.numpy(),))
    first, second = np.arange(TAIL) % ROWS, (np.arange(TAIL) + 1) % ROWS
    assert (want[first] != want[second]).any(1).sum() > TAIL // 2, "second rows repeat the first's tour"
    idx = batch_index(device, grid)
    l = tiled(locs, idx)
    rec = torch.full((idx.shape[0], locs.shape[1]), -7, dtype=torch.int64, device=device)
    nat.call("co_tsp_nearest_rec", *rec.shape, nat.ptr(l), nat.ptr(rec), nat.stream_of(l))
    same(rec, tiled(want, idx), "rec")


def test_nearest_rec_second_row(dev):
    check_nearest_rec(dev)
