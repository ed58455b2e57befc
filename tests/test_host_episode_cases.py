"""A thinned set of the cases of tests/episode_cases.py on the CPU: the host build's
stepwise entry points (co_tsp_reset / co_tsp_step / co_tsp_reward and the CVRP and SLAP
equivalents, ``nat.HOST``) driven with the oracle's actions and held to the same
references as tests/test_gpu_episode_kernels.py holds the one-launch kernels to, and the
case builders' own claims: exact fills occur, episode lengths differ, near ties are near,
ties exist, lists run dry, and every invalid row is invalid for the stated reason.  Runs
without a GPU, so the references and the cases are validated where no kernel runs."""
import pytest
import torch

import episode_cases as ec
from oracle.envs import TSPOracle
from rl4co_slap_amd import _native as nat

I64, I32, F32, U8 = torch.int64, torch.int32, torch.float32, torch.uint8
CPU = torch.device("cpu")


def _cpu(outs):
    outs.check_guards()
    return outs.cpu()


# ------------------------------------------------------------------------------ TSP
def _host_tsp(locs, acts):
    """co_tsp_reset, N x co_tsp_step in place, co_tsp_reward on the row-major actions."""
    b, n = acts.shape
    o = ec.Outs(CPU)
    st = torch.zeros(1, dtype=I32)
    mask, first, cur, i = (o.new("action_mask", (b, n), U8), o.new("first_node", b, I64),
                           o.new("current_node", b, I64), o.new("i", (b, 1), I64))
    done, srew, rew = o.new("done", b, U8), o.new("step_reward", b, U8), o.new("reward", b, F32)
    nat.call("co_tsp_reset", b, n, mask, first, cur, i, rew, nat.HOST)
    for t in range(n):
        a = acts[:, t].contiguous()
        nat.call("co_tsp_step", b, n, nat.ptr(a), mask, mask, i, i, first, first, cur, done,
                 srew, 1 if t == 0 else 0, None, nat.ptr(st), nat.HOST)
    a = acts.contiguous()
    nat.call("co_tsp_reward", b, n, n, nat.ptr(locs), b, nat.ptr(a), n, 1, 1, rew, nat.ptr(st),
             nat.HOST)
    return _cpu(o), int(st.item())


def _check_tsp(ref, family, bound):
    got, st = _host_tsp(ref.locs, ref.acts)
    assert st == 0
    for k, w in ec.tsp_expected(ref).items():
        if k != "actions":
            ec.assert_same(k, got[k], w)
    ec.assert_reward(got["reward"], ref.reward)
    f64 = ec.tour_f64(ref.locs, ref.acts)
    # the oracle's own f32 reward against the float64 restatement: both references agree
    ec.assert_reward(ref.reward, f64.float())
    ec.record("host_" + family, got["reward"], f64, bound)


@pytest.mark.parametrize("n,kind", [(33, "uniform"), (64, "grid"), (113, "grid"),
                                    (257, "circle"), (513, "circle")])
def test_host_tsp_nearest_cases(n, kind):
    rpw = ec.nearest_rows_per_wave(n)
    _check_tsp(ec.tsp_nearest_ref(kind, n, ec.batch_set(rpw, rpw)[-1]), "tsp_nearest",
               ec.BOUND_NEAREST)


@pytest.mark.parametrize("n", [1, 2, 31, 65, 112, 129, 257])
def test_host_tsp_teacher_cases(n):
    ref = ec.tsp_teacher_ref(n, ec.rows_batches(n)[-1])
    _check_tsp(ref, "tsp_teacher", ec.BOUND_TSP_TEACHER)
    b = ref.acts.shape[0]
    if n < 2 or b < 3:
        return
    # the batch with a revisit and an out-of-range action: both rows invalid for the stated
    # reason (and only those), the flag from the host build's validity check
    for which in range(3):
        d = ec.dirty_batch(ref.acts, which)
        in_range = (d.acts >= 0) & (d.acts < n)
        assert bool(in_range[d.clean].all()) and bool(in_range[d.revisit].all())
        assert int((~in_range[d.oor]).sum()) == 1
        rv = d.acts[d.revisit]
        assert rv.unique().numel() == n - 1 and d.missing not in rv.tolist()
        TSPOracle.check_solution_validity(None, d.acts[d.clean])
        for r in (d.revisit, d.oor):
            with pytest.raises(AssertionError, match="Invalid tour"):
                TSPOracle.check_solution_validity(None, d.acts[r:r + 1])
        exp = ec.revisit_expected(ref.locs[d.revisit], rv)
        assert int(exp["action_mask"].sum()) == 1 and bool(exp["action_mask"][d.missing])
        rew = torch.zeros(b)
        st = torch.zeros(1, dtype=I32)
        nat.call("co_tsp_reward", b, n, n, nat.ptr(ref.locs), b, nat.ptr(d.acts), n, 1, 1,
                 nat.ptr(rew), nat.ptr(st), nat.HOST)
        assert int(st.item()) & nat.ST_INVALID_TOUR
        ec.assert_reward(rew, ref.reward, rows=d.clean)


@pytest.mark.parametrize("n", [257, 512, 513, 1024])
def test_circle_case_is_near_tied_on_half_the_steps(n):
    """On the "circle" coordinates the two smallest squared distances are within the
    certificate's factor (so the kernel redoes the step exactly) on at least half of the
    steps of every instance."""
    rpw = ec.nearest_rows_per_wave(n)
    ref = ec.tsp_nearest_ref("circle", n, ec.batch_set(rpw, rpw)[-1])
    near = ec.near_tie_steps(ref.locs, ref.acts)
    assert bool((near >= (n - 1) // 2).all()), near.tolist()
    uni = ec.tsp_nearest_ref("uniform", n, ec.batch_set(rpw, rpw)[-1])
    assert bool((ec.near_tie_steps(uni.locs, uni.acts) < n // 8).all())


@pytest.mark.parametrize("n", ec.TSP_NEAREST_N)
def test_straddle_case_separates_squared_from_rounded_distances(n):
    """The pair's squared distances sit on either side of a 2^10-ulp step, a few ulps
    apart, with one rounded square root; the oracle takes the farther, lower-indexed node
    at step 1 where an argmin of squared distances would take the other."""
    near, far = ec.straddle_pair()
    sq = lambda p: ((p[0] - 0.5) * (p[0] - 0.5) + (p[1] - 0.5) * (p[1] - 0.5))  # noqa: E731
    sn, sf = sq(near), sq(far)
    bn, bf = int(sn.view(torch.int32)), int(sf.view(torch.int32))
    assert 0 < bf - bn <= 5 and (bf >> 10) == (bn >> 10) + 1
    assert float(sn.double().sqrt().float()) == float(sf.double().sqrt().float())
    rpw = ec.nearest_rows_per_wave(n)
    ref = ec.tsp_nearest_ref("straddle", n, ec.batch_set(rpw, rpw)[-1])
    for i in range(ref.acts.shape[0]):
        fi, ni = ec.straddle_nodes(i, n)
        assert fi < ni < n and int(ref.acts[i, 1]) == fi and int(ref.acts[i, 2]) == ni
    lanes = {ec.straddle_nodes(i, n)[1] % 32 for i in range(ref.acts.shape[0])}
    assert len(lanes) == min(2, ref.acts.shape[0]) or n < 36


@pytest.mark.parametrize("n", [32, 105, 257])
def test_grid_case_has_exact_ties(n):
    rpw = ec.nearest_rows_per_wave(n)
    ref = ec.tsp_nearest_ref("grid", n, ec.batch_set(rpw, rpw)[-1])
    assert bool((ec.near_tie_steps(ref.locs, ref.acts, 1.0) >= n // 2).all())


# ------------------------------------------------------------------------------ CVRP
def _host_cvrp(ref):
    gen = ref.gen
    b, n = gen["locs"].shape[:2]
    t_all = ref.acts.shape[1]
    o = ec.Outs(CPU)
    st = torch.zeros(1, dtype=I32)
    depot, locs, demand = (gen[k].contiguous() for k in ("depot", "locs", "demand"))
    used = [torch.zeros(b, 1), torch.zeros(b, 1)]
    locs_out, cur = o.new("locs", (b, n + 1, 2), F32), o.new("current_node", (b, 1), I64)
    vcap, vis = o.new("vehicle_capacity", (b, 1), F32), o.new("visited", (b, n + 1), U8)
    mask, done, srew = (o.new("action_mask", (b, n + 1), U8), o.new("done", b, U8),
                        o.new("step_reward", b, U8))
    rew = o.new("reward", b, F32)
    nat.call("co_cvrp_reset", b, n, nat.ptr(depot), nat.ptr(locs), nat.ptr(demand),
             float(ref.vcap), locs_out, cur, nat.ptr(used[0]), vcap, vis, mask, nat.HOST)
    for t in range(t_all):
        a = ref.acts[:, t].contiguous()
        nat.call("co_cvrp_step", b, n, nat.ptr(a), nat.ptr(demand), nat.ptr(used[t & 1]),
                 nat.ptr(used[(t + 1) & 1]), vcap, vis, vis, cur, done, srew, mask, nat.ptr(st),
                 None, nat.HOST)
    a = ref.acts.contiguous()
    nat.call("co_cvrp_reward", b, n, t_all, locs_out, nat.ptr(a), t_all, 1, nat.ptr(demand), vcap,
             1, rew, nat.ptr(st), nat.HOST)
    got = _cpu(o)
    got["used_capacity"] = used[t_all & 1]
    return got, int(st.item())


@pytest.mark.parametrize("kind", ["generator", "exactfill"])
@pytest.mark.parametrize("n", [31, 64, 112, 256])
def test_host_cvrp_cases(n, kind):
    rpw = ec.cvrp_rows_per_wave(n + 1)
    ref = ec.cvrp_ref(kind, n, ec.batch_set(rpw, rpw)[-1])
    got, st = _host_cvrp(ref)
    assert st == 0
    for k, w in ec.cvrp_expected(ref).items():
        if k not in ("actions", "lens"):
            ec.assert_same(k, got[k], w)
    ec.assert_reward(got["reward"], ref.reward)
    f64 = ec.cvrp_f64(ref.tdf["locs"], ref.acts)
    ec.assert_reward(ref.reward, f64.float())
    ec.record("host_cvrp", got["reward"], f64, ec.BOUND_NEAREST)
    # every instance's own length: done after exactly that many steps, the batch-wide
    # length the longest
    assert int(ref.lens.max()) == ref.acts.shape[1]
    assert bool((ref.acts.gather(1, (ref.lens.long() - 1)[:, None]) >= 0).all())
    rows = torch.arange(ref.acts.shape[1])[None] >= ref.lens[:, None]
    assert bool((ref.acts[rows] == 0).all()), "steps after an instance's end are depot steps"


@pytest.mark.parametrize("n", ec.CVRP_N)
def test_exactfill_case_fills_the_vehicle_exactly(n):
    """demand + used == capacity for a chosen customer, in every batch of the set."""
    rpw = ec.cvrp_rows_per_wave(n + 1)
    for b in ec.batch_set(rpw, rpw):
        if n > 300 and b != 1:
            continue  # the long rollouts once: one row fills as often as three
        assert ec.cvrp_ref("exactfill", n, b).exact_fills > 0


def test_cvrp_case_lengths_differ():
    """The "ragged" batches hold episode lengths that differ by at least 2, and a padded
    instance (shorter than the batch) that ended away from the depot with capacity in use:
    the pad kernel has actions, a current node and a used capacity to overwrite."""
    for n in ec.CVRP_PAD_N:
        ref = ec.cvrp_ref("ragged", n, ec.cvrp_rows_per_wave(n + 1) + 1)
        lens = ref.lens.long()
        assert int(lens.max() - lens.min()) >= 2, lens.tolist()
        last = ref.acts.gather(1, (lens - 1)[:, None]).view(-1)
        assert bool(((lens < lens.max()) & (last != 0)).any()), (lens.tolist(), last.tolist())
        got, st = _host_cvrp(ref)
        assert st == 0
        for k, w in ec.cvrp_expected(ref).items():
            if k not in ("actions", "lens"):
                ec.assert_same(k, got[k], w)


# ------------------------------------------------------------------------------ SLAP
def _host_slap(cfg, ref):
    gen = ref.gen
    b = ref.acts.shape[0]
    l, p, o_, k = cfg.l, cfg.p, cfg.o, cfg.k
    o = ec.Outs(CPU)
    st = torch.zeros(1, dtype=I32)
    mask, asg = o.new("action_mask", (b, l), U8), o.new("assignment", (b, p), I32)
    i = [torch.zeros(b, 1, dtype=I64), torch.zeros(b, 1, dtype=I64)]
    done, srew, rew = (o.new("done", (b, 1), U8), o.new("step_reward", (b, 1), U8),
                       o.new("reward", b, F32))
    ratio = o.new("ratio", (b, l), F32)
    tc = torch.zeros(b, p)
    o["assignment"].t.copy_(gen["assignment"])
    nat.call("co_slap_reset", b, l, p, mask, nat.ptr(tc), nat.ptr(i[0]), rew, ratio, done, None,
             nat.HOST)
    for t in range(p):
        a = ref.acts[:, t].contiguous()
        nat.call("co_slap_step", b, l, p, nat.ptr(a), None, t, asg, asg, mask, mask,
                 nat.ptr(i[t & 1]), nat.ptr(i[(t + 1) & 1]), done, srew, nat.ptr(st), nat.HOST)
    locs, pick = gen["locs"].contiguous(), gen["picklist"].contiguous()
    nat.call("co_slap_reward", b, l, p, o_, k, asg, nat.ptr(pick), nat.ptr(locs), rew,
             nat.ptr(st), nat.HOST)
    got = _cpu(o)
    got["i"] = i[p & 1]
    return got, int(st.item())


HOST_SLAP = [c for l in (20, 48, 65, 129, 256) for c in ec.slap_configs(l)
             if c.variant in ("aligned", "negative")]


@pytest.mark.parametrize("cfg", HOST_SLAP, ids=ec.slap_id)
def test_host_slap_cases(cfg):
    ref = ec.slap_ref(cfg)
    b = ref.acts.shape[0]
    got, st = _host_slap(cfg, ref)
    assert st == 0
    for k, w in ec.slap_expected(ref, b).items():
        if k != "actions":
            ec.assert_same(k, got[k], w)
    ec.assert_reward(got["reward"], ref.reward)
    f64 = ec.slap_f64(ref.gen["locs"], ref.tdf["assignment"], ref.gen["picklist"])
    ec.assert_reward(ref.reward, f64.float())
    ec.record("host_slap", got["reward"], f64, ec.bound_slap(cfg.o, cfg.k))


@pytest.mark.parametrize("l", list(ec.SLAP_GRIDS))
def test_slap_cases_claims(l):
    """Per L: O*K on both sides of the G*8 picklist entries a group holds in registers, K
    on both sides of 8, P = 1, L - 1 and P % 4 != 0 / == 0, ratio present and NULL; in the
    "ties" distances equal depot distances at chosen locations, -0.0 and +inf; a closest
    episode with P = L - 1 whose list of finite distances runs dry (the action is then
    0); negative teacher actions and picklist entries that wrap."""
    cfgs = ec.slap_configs(l)
    slots = ec.slap_lanes(l) * 8
    assert {c.o * c.k <= slots for c in cfgs} == {True, False}
    assert {c.k > 8 for c in cfgs} == {True, False} and {1, 5} <= {c.k for c in cfgs}
    ps = {c.p for c in cfgs}
    assert {1, l - 1} <= ps and any(p % 4 for p in ps - {1}) and any(p % 4 == 0 for p in ps)
    assert {c.ratio for c in cfgs} == {True, False}
    assert {c.variant for c in cfgs} == {"aligned", "negative", "locs8", "depot8", "mask1",
                                         "assign4", "ratio4"}
    assert ec.SLAP_GRIDS[l][0] * ec.SLAP_GRIDS[l][1] == l
    dry = ec.slap_ref(cfgs[0])
    assert cfgs[0].policy == "closest" and cfgs[0].p == l - 1 and cfgs[0].dist == "ties"
    dd = dry.gen["depot_loc_dist"]
    assert bool(torch.isinf(dd).any()) and bool(((dd == 0) & torch.signbit(dd)).any())
    assert bool((dry.acts == 0).any()), "no closest-free list ran dry"
    chosen = dd.gather(1, dry.acts)
    assert bool((chosen[:, 1:] == chosen[:, :-1]).any()), "no tie between chosen distances"
    neg = ec.slap_ref(cfgs[-1])
    assert cfgs[-1].variant == "negative"
    assert bool((neg.acts < 0).any()) and bool((neg.acts >= -l).all())
    pk = neg.gen["picklist"]
    assert bool((pk < 0).any()) and bool((pk >= -cfgs[-1].p).all())
    # the wrapped action is what the mask loses; the raw value is what the assignment keeps
    wrapped = torch.where(neg.acts < 0, neg.acts + l, neg.acts)
    left = torch.ones(neg.acts.shape[0], l, dtype=torch.bool)
    left[:, 0] = False
    left.scatter_(1, wrapped, False)
    assert torch.equal(neg.tdf["action_mask"], left)
    assert torch.equal(neg.tdf["assignment"], neg.acts.to(I32))
