"""The cases of tests/env_step_cases.py on the CPU: the host build's entry points
(``nat.HOST_SYMBOLS``) through the same checks, against the same references, as
tests/test_gpu_env_kernels.py runs on the device -- and the case builders' own claims: the
three capacity-edge kinds occur with exact f32 sums, ties and fully masked rows occur, every
dirty row is invalid for exactly the stated reason, and every dispatch path the coverage
table of env_step_cases.py names has a case.  Runs without a GPU: the references are proven
here before a kernel is involved."""
import pytest
import torch

import env_step_cases as sc
from rl4co_slap_amd import _native as nat

CPU = torch.device("cpu")


# ------------------------------------------------------------------- the same checks
@pytest.mark.parametrize("case", sc.CVRP_STEP_CASES, ids=sc.cvrp_step_id)
def test_host_cvrp_step(case):
    sc.check_cvrp_step(CPU, case)


@pytest.mark.parametrize("hi", [True, False], ids=["hi", "lo"])
@pytest.mark.parametrize("path", list(sc.CVRP_STATUS_SHAPES))
def test_host_cvrp_step_status(path, hi):
    sc.check_cvrp_step_status(CPU, path, hi)


@pytest.mark.parametrize("b,n,off", [(1, 1, 0), (7, 5, 1), (33, 77, 3), (5, 130, 0)])
def test_host_cvrp_action_mask(b, n, off):
    sc.check_cvrp_action_mask(CPU, n, b, off)


@pytest.mark.parametrize("b,n,off,vcap", [(1, 1, 0, 1.0), (7, 5, 1, 0.77), (33, 77, 3, 0.77)])
def test_host_cvrp_reset(b, n, off, vcap):
    sc.check_cvrp_reset(CPU, n, b, off, vcap)


HOST_REWARD = [c for c in sc.CVRP_REWARD_CASES if c.t <= 1024 and c.b in (5, 65)]


@pytest.mark.parametrize("case", HOST_REWARD, ids=sc.cvrp_reward_id)
def test_host_cvrp_reward(case):
    sc.check_cvrp_reward(CPU, case)
    if case.check:
        for which in sc.CVRP_DIRTY:
            sc.check_cvrp_reward_status(CPU, case, which)


@pytest.mark.parametrize("case", sc.SLAP_STEP_CASES, ids=sc.slap_step_id)
def test_host_slap_step(case):
    sc.check_slap_step(CPU, case)


@pytest.mark.parametrize("which", sc.SLAP_STATUS_WHICH)
def test_host_slap_step_status(which):
    sc.check_slap_step_status(CPU, "group", which)
    sc.check_slap_step_status(CPU, "tile7", which)


@pytest.mark.parametrize("b,l,p,off,full", [(1, 1, 1, 0, True), (7, 5, 3, 1, True), (33, 100, 20, 0, False)])
def test_host_slap_reset(b, l, p, off, full):
    sc.check_slap_reset(CPU, b, l, p, off, full)


@pytest.mark.parametrize("case", [c for c in sc.SLAP_REWARD_CASES if c.l <= 4086], ids=sc.slap_reward_id)
def test_host_slap_reward(case):
    sc.check_slap_reward(CPU, case)


@pytest.mark.parametrize("which", sc.SLAP_REWARD_WHICH)
def test_host_slap_reward_status(which):
    sc.check_slap_reward_status(CPU, "group", which)
    sc.check_slap_reward_status(CPU, "row4", which)


@pytest.mark.parametrize("b,n,alias", [(1, 1, False), (7, 5, True), (33, 77, False)])
def test_host_tsp_reset(b, n, alias):
    sc.check_tsp_reset(CPU, b, n, alias)


@pytest.mark.parametrize("case", sc.TSP_REWARD_CASES, ids=sc.tsp_reward_id)
def test_host_tsp_reward_generic(case):
    sc.check_tsp_reward_generic(CPU, case)


@pytest.mark.parametrize("name", [n for n in sc.REJECTIONS if n in nat.HOST_SYMBOLS])
def test_host_rejections(name):
    sc.check_rejections(CPU, name)


# ------------------------------------------------------------- the builders' claims
def test_capacity_edges_occur_in_every_step_case():
    """Rows whose exact f32 ``demand + used`` is the capacity, one ulp below and one ulp
    above it, among the customers left unvisited (so the mask shows the comparison)."""
    for c in sc.CVRP_STEP_CASES:
        eq, below, above = sc.cvrp_state(c.n, c.b).edges
        if c.b * (c.n - 1) >= 9:
            assert eq > 0 and below > 0 and above > 0, sc.cvrp_step_id(c)
    # and the three kinds come out differently: feasible, feasible, masked
    st = sc.cvrp_state(20, 16)
    want = sc.cvrp_step_ref(st.demand, st.used, st.cap, st.visited, st.action)
    sel = (st.action - 1).clamp(0, 19)
    u = want["used_capacity"]
    assert torch.equal(u, (st.used + st.demand[torch.arange(16), sel]) * (st.action != 0).float())
    s = st.demand + u[:, None]
    free = want["visited"][:, 1:] == 0
    inf = torch.tensor(float("inf"))
    cap = st.cap[:, None]
    m = want["action_mask"][:, 1:]
    assert bool(m[free & (s == cap)].all()) and bool(m[free & (s == torch.nextafter(cap, -inf))].all())
    assert not bool(m[free & (s == torch.nextafter(cap, inf))].any())


def test_step_cases_hold_special_rows():
    st = sc.cvrp_state(20, 17)
    vsum = st.visited.sum(1)
    assert bool((vsum == 0).any()) and bool((vsum == 21).any()) and bool((vsum == 20).any())
    assert bool((st.action == 0).any()) and bool((st.used[st.action == 0] > 0).any())
    want = sc.cvrp_step_ref(st.demand, st.used, st.cap, st.visited, st.action)
    assert bool(want["done"].any()) and not bool(want["done"].all())
    sl = sc.slap_state(100, 7, 17)
    assert bool((~sl.mask).all(1).any()) and bool(sl.mask.all(1).any())
    assert bool((sl.action < 0).any()) and bool((sl.action >= -100).all())
    assert bool((sl.product < 0).any()) and bool((sl.product >= -7).all())
    assert bool((sl.i == 6).any()) and bool((sl.i != 6).any())
    assert bool(torch.isinf(sl.dist).any()) and bool(((sl.dist == 0) & torch.signbit(sl.dist)).any())


@pytest.mark.parametrize("n", [31, 64, 112, 128, 160, 320])
def test_policy_cases_hold_ties_and_masked_rows(n):
    ps = sc.cvrp_policy_state(n, 13, "grid")
    assert ps.ties > 0
    feas = ps.mask.clone()
    feas[:, 0] = False
    assert bool((~ps.mask).all(1).any()), "no fully masked row"
    assert bool((ps.mask[:, 0] & ~feas.any(1)).any()), "no row where only the depot is feasible"
    act = sc.cvrp_policy_ref(ps)
    assert bool((act[~feas.any(1)] == 0).all()) and bool((act[feas.any(1)] > 0).all())
    tp = sc.tsp_policy_state(n, 13, "grid")
    assert tp.ties > 0 and bool((~tp.mask).all(1).any())
    sl = sc.slap_state(n - n % 4, 7, 17)
    act = sc.slap_closest_ref(sl)
    d = sl.dist.masked_fill(~sl.mask, float("inf"))
    best = d.min(1, keepdim=True).values
    assert bool(((d == best).sum(1) > 1).any()), "no tie between free locations"
    assert bool((act[(~sl.mask).all(1)] == 0).all())


@pytest.mark.parametrize("which", sc.CVRP_DIRTY)
def test_cvrp_dirty_rows_are_invalid_for_the_stated_reason(which):
    for n, t in ((10, 14), (20, 30), (10, 1024)):
        tour = sc.cvrp_tours(n, t, 5)
        assert sc.cvrp_validity(tour, tour.acts) is None
        acts, bits, msg = sc.cvrp_dirty(tour, which)
        clean = torch.arange(5) != 1
        assert torch.equal(acts[clean], tour.acts[clean])
        in_range = (acts >= 0) & (acts <= n)
        if which == "range":
            assert int((~in_range).sum()) == 1 and bits & nat.ST_INDEX_RANGE
        else:
            assert bool(in_range.all()) and sc.cvrp_validity(tour, acts) == msg
        cust = acts[1][(acts[1] > 0) & (acts[1] <= n)]
        assert (cust.unique().numel() == n) == (which == "overload")


@pytest.mark.parametrize("which", sc.SLAP_REWARD_WHICH + sc.SLAP_STATUS_WHICH)
def test_slap_dirty_rows_are_invalid_for_the_stated_reason(which):
    if which in sc.SLAP_REWARD_WHICH:
        c = sc.SLAP_REWARD_STATUS_SHAPES["group"]
        d = sc.slap_reward_data(c)
        a, pk = sc.slap_reward_dirty(c, d, which)
        bad_a = (a < -c.l) | (a >= c.l)
        bad_p = (pk < -c.p) | (pk >= c.p)
        assert int(bad_a.sum()) + int(bad_p.sum()) == 1
        assert not bool(bad_a[torch.arange(c.b) != 1].any()) and not bool(bad_p[torch.arange(c.b) != 1].any())
        if which != "pick_hi":  # a pick names the bad entry
            prod = int(bad_a[1].nonzero())
            assert prod in torch.where(pk[1] < 0, pk[1] + c.p, pk[1]).flatten().tolist()
        with pytest.raises(IndexError):
            sc.slap_reward_ref(d, a, pk)
        return
    l, p = 100, 6
    v = sc.slap_bad_value(which, l, p)
    lim = l if which.startswith("action") else p
    assert not (-lim <= v < lim) and (-lim <= v - 1 < lim or -lim <= v + 1 < lim)
    st = sc.slap_state(l, p, 5)
    action, product = st.action.clone(), st.product.clone()
    (action if which.startswith("action") else product)[2] = v
    with pytest.raises(IndexError):
        sc.slap_step_ref(st.mask, st.i, st.assignment, action, product)


def test_every_listed_path_has_a_case():
    steps = {sc.cvrp_step_path(c.n, c.off, c.dem_off) + ("-cnt" if c.count else "")
             for c in sc.CVRP_STEP_CASES}
    assert steps >= {f"rows{k}{w}" for k in (1, 2, 3, 4) for w in ("", "-cnt")} | {"tile", "row", "tile-cnt", "row-cnt"}
    rew = {sc.cvrp_reward_path(c.n, c.t, c.b, c.check, c.step_major, c.locs_off) for c in sc.CVRP_REWARD_CASES}
    assert rew == {"row4", "row2", "row1", "tile"}
    t4, t2, t1 = sc.cvrp_reward_t_cuts(10)
    assert [sc.cvrp_reward_path(10, t, 5, 1, False) for t in (t4, t4 + 1, t2, t2 + 1, t1, t1 + 1)] == \
        ["row4", "row2", "row2", "row1", "row1", "tile"]
    assert sc.cvrp_tile_lds(104, 1) <= 80 * 1024 < sc.cvrp_tile_lds(105, 1)
    assert {sc.slap_step_path(c.l, c.mask_off) for c in sc.SLAP_STEP_CASES} == \
        {"group1", "group2", "group3", "group4", "tile"}
    assert {sc.slap_closest_path(c.l, c.mask_off, c.dist_off) for c in sc.SLAP_CASES} == \
        {"fused1", "fused2", "fused3", "fused4", "pair"}
    assert {sc.slap_reward_path(c.l, c.p, c.o, c.k) for c in sc.SLAP_REWARD_CASES} == \
        {"group", "row4", "row2", "row1", "global"}
    assert set(sc.SLAP_REWARD_STATUS_SHAPES) == {"group", "row4", "row2", "row1", "global"}
    # the group reward kernel's LDS at its limits stays inside 64 KiB: no refusal to reach
    rg = lambda l, p, s, o: (8 * l + ((4 * p + 7) & ~7) + 8 * s + 4 * o + 15) & ~15  # noqa: E731
    assert max(16 * rg(128, 32, o * k, o) for o in range(1, 129) for k in range(1, 129) if o * k <= 128) <= 65536
