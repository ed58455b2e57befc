"""The cases of tests/steps_cases.py on the CPU: every dispatch path its coverage table names
has cases at both ends of its range and meets every value of each case dimension; the case
builders' own claims (a row empties in the middle of a launch, a revisit exists, the lane-0
row's nearest locations are lane 0's, the short rows run out, done flips where stated, ties,
-0.0, +inf and subnormals are present among free locations); and the references themselves
against the host build's single-step entries chained K times -- co_tsp_step, and co_slap_step
given the oracle's action -- so that every expected value of tests/test_gpu_steps_kernels.py
has two independent CPU implementations.  Runs without a GPU."""
import pytest
import torch

import steps_cases as kc
from rl4co_slap_amd import _native as nat

CPU = torch.device("cpu")


# ------------------------------------------------------------------ the coverage table
def test_every_listed_path_has_a_case():
    by_path = {}
    for c in kc.TSP_STEPS_CASES:
        by_path.setdefault(kc.tsp_steps_path(c.n, max(c.off_a, c.off_b)), []).append(c)
    assert set(by_path) == {"steps8", "steps16", "steps32", "steps64", "single-group4", "single-tile"}
    for g, (lo, hi) in kc.TSP_GROUP_N.items():
        cases = by_path[f"steps{g}"]
        # both ends of the range, and one step outside either end is another path
        assert kc.tsp_steps_path(lo) == kc.tsp_steps_path(hi) == f"steps{g}"
        assert kc.tsp_steps_path(lo - 4) != f"steps{g}" != kc.tsp_steps_path(hi + 4)
        for n, ks in ((lo, kc.TSP_K_ALL), (hi, kc.TSP_K_UPPER)):
            at = [c for c in cases if c.n == n and not c.pad]
            assert {c.b for c in at} == set(kc.tsp_steps_batches(g))
            for b in kc.tsp_steps_batches(g):
                assert {(c.k, c.first_mode) for c in at if c.b == b} == {(k, fm) for k in ks for fm in (0, 1)}
        assert any(c.pad == 5 for c in cases)
    assert kc.tsp_steps_batches(8) == [1, 9, 33, 7] and kc.tsp_steps_batches(64) == [1, 2, 5]
    single = by_path["single-group4"] + by_path["single-tile"]
    assert {c.n for c in single} == {64, 70, 100, 1028}
    assert {(c.off_a, c.off_b) for c in single if c.n == 100} == {(1, 0), (0, 1)}
    assert any(c.cur_null for c in kc.TSP_STEPS_CASES)
    assert any(c.first_mode == 1 and c.k == 1 for c in single)      # first_a NULL on the fallback
    assert set(kc.TSP_STATUS_N) == set(by_path)
    assert all(kc.tsp_steps_path(n) == p for p, n in kc.TSP_STATUS_N.items())
    # co_tsp_step: G = 2 .. 64 and the tile kernel at both ends (test_gpu_envs.py's N list)
    ns = kc.TSP_STEP_N
    ends = {"group2": (4, 32), "group4": (36, 64), "group8": (68, 128), "group16": (132, 256),
            "group32": (260, 512), "group64": (516, 1024), "tile": (3, 1028)}
    for path, (lo, hi) in ends.items():
        assert lo in ns and hi in ns and kc.tsp_step_path(lo) == kc.tsp_step_path(hi) == path
    assert kc.tsp_step_path(100, 1) == "tile"

    slap = {}
    for c in kc.SLAP_STEPS_CASES:
        slap.setdefault(kc.slap_steps_path(c.l, max(c.off_a, c.off_b), c.dist_off), []).append(c)
    assert set(slap) == {"sorted1", "sorted2", "sorted3", "sorted4", "single"}
    for ku in (1, 2, 3, 4):
        cases = slap[f"sorted{ku}"]
        lo, hi = kc.SLAP_SORTED_L[2 * ku - 2], kc.SLAP_SORTED_L[2 * ku - 1]
        assert {c.l for c in cases} == {lo, hi} and kc.slap_steps_ku(lo) == kc.slap_steps_ku(hi) == ku
        assert hi == 64 * ku and (lo == hi - 60 or ku == 1)
        assert kc.slap_steps_epl(ku) == (4, 8, 16, 16)[ku - 1]
        for l in (lo, hi):
            at = [c for c in cases if c.l == l and not c.pad]
            assert {(c.b, c.p) for c in at} == {(b, p) for b in kc.SLAP_B for p in kc.SLAP_P}
        assert {c.k for c in cases} >= {1, 2, 3, 7, 20}
        assert {c.k == c.p for c in cases} == {True, False}
        assert {c.inplace for c in cases} == {True, False}
        assert {c.tc for c in cases} == set(kc.SLAP_TC)
        assert {c.kind for c in cases} == set(kc.SLAP_KINDS)
        assert any(c.pad == 3 for c in cases)
        assert any(c.tc == "nullend" and c.k < c.p for c in cases)
        assert any(not c.inplace and c.p == 20 for c in cases)     # the copy loop's second pass
        assert any(not c.inplace and c.p == 7 for c in cases)
    single = slap["single"]
    assert {c.l for c in single} == {260, 62, 100}
    assert {(c.off_a, c.off_b, c.dist_off) for c in single if c.l == 100} == {(1, 0, 0), (0, 1, 0), (0, 0, 4)}
    assert {c.tc for c in single} == set(kc.SLAP_TC) and any(c.pad for c in single)
    assert {kc.slap_steps_ku(l) for l in kc.SLAP_SPECIAL_L if l <= 256} == {1, 2, 3, 4}
    assert set(kc.SLAP_STATUS_L) == set(slap)
    assert all(kc.slap_steps_path(l) == p for p, l in kc.SLAP_STATUS_L.items())


# ------------------------------------------------------------- the builders' claims
@pytest.mark.parametrize("n", [68, 128, 512, 1024, 70])
def test_tsp_cases_hold_special_rows(n):
    b, k = 5, 17
    for fm in (0, 1):
        st = kc.tsp_steps_state(n, b, k, fm)
        assert set(st.kinds) == set(kc.TSP_KINDS)
        states, status = kc.tsp_steps_ref(st.mask, st.i, st.first, st.acts, fm)
        assert status == 0
        done = torch.stack([s["done"] for s in states[1:]])        # [K, B]
        for r, kind in enumerate(st.kinds):
            col = done[:, r].tolist()
            if kind == "empty":
                assert all(col) and not bool(st.mask[r].any())
            elif kind == "ends_at_k":                               # empties exactly at step K
                assert col == [False] * (k - 1) + [True]
                assert sorted(st.acts[:, r].tolist()) == st.mask[r].nonzero().flatten().tolist()
                assert set(kc.tsp_special_nodes(n)) <= set(st.acts[:, r].tolist())
            elif kind == "ends_mid":                                # ... at a middle step, stays done
                m = k // 2
                assert col == [False] * (m - 1) + [True] * (k - m + 1) and 1 < m < k
                assert st.acts[:, r].unique().numel() == m          # revisits from then on
            elif kind == "revisit":
                assert int(st.acts[0, r]) == int(st.acts[1, r]) and bool(st.mask[r, st.acts[0, r]])
                assert not col[-1]
        assert bool((st.i > (1 << 32)).any())
        assert bool((st.i == 0).any()) == (fm == 1)
        assert bool((st.first < 0).any()) and bool((st.first >= n).any())
        assert torch.equal(states[1]["first_node"], st.acts[0] if fm == 1 else st.first)
        assert torch.equal(states[k]["i"], st.i + k)
    sp = kc.tsp_special_nodes(n)
    assert {0, 3, n - 1} <= set(sp)
    g = kc.tsp_steps_group(n)
    if n in (128, 512, 1024):   # a byte of word sl + 3 G, a lane's last slot
        assert any(x // 4 >= 3 * g for x in sp) and (4 * 3 * g + 2) in sp


@pytest.mark.parametrize("path", list(kc.TSP_STATUS_N))
def test_tsp_status_cases_hold_one_bad_action(path):
    n = kc.TSP_STATUS_N[path]
    for which in kc.TSP_BAD:
        for step in kc.tsp_status_steps():
            _, acts = kc.tsp_status_acts(n, which, step, 0)
            bad = (acts < 0) | (acts >= n)
            assert int(bad.sum()) == 1 and bool(bad[step, kc.TSP_STATUS_ROW])
    assert kc.tsp_status_steps() == (0, 7, 8, 16)
    assert kc.TSP_BAD["big"](n) % (1 << 32) == 1                    # in range once truncated
    assert (kc.TSP_BAD["wrap"](n) >> 2) % (1 << 32) == kc.TSP_WRAP_NODE // 4
    st, acts = kc.tsp_status_acts(n, "wrap", 8, 1)
    states, _ = kc.tsp_steps_ref(st.mask, st.i, st.first, acts, 1)
    assert all(bool(s["action_mask"][kc.TSP_STATUS_ROW, kc.TSP_WRAP_NODE]) for s in states)


def _order(dist_row, mask_row):
    """The free locations in the order closest-free takes them: (distance, index)."""
    free = mask_row.nonzero().flatten().tolist()
    return sorted(free, key=lambda j: (float(dist_row[j]) + 0.0, j))


@pytest.mark.parametrize("l", kc.SLAP_SPECIAL_L)
def test_slap_special_rows(l):
    st = kc.slap_special_state(l)
    p, k = kc.SLAP_SPECIAL_P, kc.SLAP_SPECIAL_K
    rows = kc.SLAP_SPECIAL_ROWS
    assert [int(st.mask[rows[f"free{n}"]].sum()) for n in (0, 1, 5)] == [0, 1, 5] and 5 < k
    states, actions, status = kc.slap_steps_ref(st.mask, st.i, st.assignment, st.dist, st.product)
    assert status == nat.ST_INDEX_RANGE
    for n in (0, 1, 5):         # once they run out the action is 0
        assert actions[:, rows[f"free{n}"]].tolist()[n:] == [0] * (k - n)
    # the lane-0 row: its first 4 KU choices are lane 0's, nearest last, the next elsewhere
    r = rows["lane0"]
    own = kc.slap_lane0_locations(l)
    ku = kc.slap_steps_ku(min(l, 256))
    assert len(own) >= 4 * ku and k > len(own) and (l > 256 or len(own) == 4 * ku)
    if l <= 256:
        assert kc.slap_steps_epl(ku) >= len(own)
        assert all(j % 64 < 4 for j in own)
    order = _order(st.dist[r], st.mask[r])
    assert order[:len(own)] == own[::-1] and order[len(own)] not in own
    assert actions[:, r].tolist() == order[:k]
    # done flips where stated
    done = torch.stack([s["done"].view(-1) for s in states[1:]])
    for row, (i0, at) in enumerate(kc.SLAP_SPECIAL_I):
        assert int(st.i[row]) == i0
        assert done[:, row].nonzero().flatten().tolist() == ([] if at is None else [at])
    assert any(i0 >= p for i0, _ in kc.SLAP_SPECIAL_I)
    assert {at for _, at in kc.SLAP_SPECIAL_I} >= {0, 9, k - 1, None}
    # the products: wrapping, truncating, out of range
    vals = set(kc.SLAP_SPECIAL_PRODUCTS.values())
    assert vals == {-1.0, -float(p), float(p), -float(p) - 1, 2.75, -0.5}
    bad = torch.stack([kc._slap_bad_rule(st.product[:, t], p) for t in range(k)], 1)
    assert {(r_, t) for r_, t in bad.nonzero().tolist()} == \
        {rt for rt, v in kc.SLAP_SPECIAL_PRODUCTS.items() if v in (float(p), -float(p) - 1)}
    for (r_, t), v in kc.SLAP_SPECIAL_PRODUCTS.items():
        before, after = states[t]["assignment"][r_], states[t + 1]["assignment"][r_]
        if bad[r_, t]:
            assert torch.equal(before, after)
            continue
        slot = {-1.0: p - 1, -float(p): 0, 2.75: 2, -0.5: 0}[v]
        assert int(after[slot]) == int(actions[t, r_])
        assert torch.equal(before[torch.arange(p) != slot], after[torch.arange(p) != slot])


def test_slap_states_hold_ties_zeros_inf_and_subnormals():
    st = kc.slap_steps_state(128, 20, 17, 20, "ties")
    free = st.mask
    assert bool((torch.isinf(st.dist) & free).any())
    assert bool(((st.dist == 0) & torch.signbit(st.dist) & free).any())
    assert bool(((st.dist == 0) & ~torch.signbit(st.dist) & free).any())
    d = st.dist.masked_fill(~free, float("inf"))
    best = d.min(1, keepdim=True).values
    assert bool((((d == best) & free).sum(1) > 1).any()), "no tie between free locations"
    assert bool((~free).all(1).any()) and bool(free.all(1).any())
    _, actions, status = kc.slap_steps_ref(st.mask, st.i, st.assignment, st.dist, st.product)
    assert status == 0
    # a row with a free +inf location and fewer finite free ones than K: never picked
    inf_free = (torch.isinf(st.dist) & free).any(1) & ((free & ~torch.isinf(st.dist)).sum(1) < 20)
    if bool(inf_free.any()):
        r = int(inf_free.nonzero()[0])
        picked = actions[:, r]
        assert not bool(torch.isinf(st.dist[r, picked[picked > 0]]).any())
    assert bool((st.product < 0).any()) and bool((st.product != st.product.trunc()).any())
    assert bool((st.i == 19).any()) and bool((st.i != 19).any())
    fr = kc.slap_steps_state(128, 20, 17, 20, "frac")
    tiny = torch.finfo(torch.float32).tiny
    sub = (fr.dist > 0) & (fr.dist < tiny)
    assert bool((sub.sum(1) == 3).all()), "subnormal distances were flushed"
    assert bool((fr.dist < 0).any()) and bool((fr.dist != fr.dist.trunc()).any())
    assert all(fr.dist[r].unique().numel() == 128 for r in range(17))
    # mid-launch done: some row's done is true at a step before the last and false after
    states, _, _ = kc.slap_steps_ref(fr.mask, fr.i, fr.assignment, fr.dist, fr.product)
    done = torch.stack([s["done"].view(-1) for s in states[1:]])
    assert bool((done[:-1].any(0) & ~done[-1]).any())


@pytest.mark.parametrize("path", list(kc.SLAP_STATUS_L))
def test_slap_status_cases_hold_one_bad_product(path):
    l, p = kc.SLAP_STATUS_L[path], kc.SLAP_STATUS_P
    for step in kc.SLAP_STATUS_STEPS:
        _, prod = kc.slap_status_products(l, step)
        bad = torch.stack([kc._slap_bad_rule(prod[:, t], p) for t in range(prod.shape[1])], 1)
        assert bad.nonzero().tolist() == [[kc.SLAP_STATUS_ROW, step]]
        v = int(prod[kc.SLAP_STATUS_ROW, step])
        assert v in (p, -p - 1) and -p <= v - (1 if v > 0 else -1) < p


def test_uniform_products_stay_in_range():
    for c in kc.SLAP_STEPS_CASES:
        st = kc.slap_steps_state(c.l, c.p, c.b, c.k, c.kind)
        prod = kc.slap_case_products(c, st)
        assert prod.shape == (c.b, c.k)
        assert not bool(torch.stack([kc._slap_bad_rule(prod[:, t], c.p) for t in range(c.k)]).any())
        if c.tc == "nullend":
            assert int(prod[0, -1]) == c.p - 1


# ------------------------------------------ the references against the host build
@pytest.mark.parametrize("n,b,k", [(68, 9, 17), (128, 5, 9), (260, 5, 8), (1024, 5, 2), (70, 5, 7),
                                   (64, 1, 1)])
@pytest.mark.parametrize("first_mode", [0, 1])
def test_tsp_reference_equals_host_single_steps(n, b, k, first_mode):
    kc.check_tsp_ref_against_single_steps(CPU, n, b, k, first_mode)


@pytest.mark.parametrize("which", list(kc.TSP_BAD))
def test_tsp_reference_bad_action_rule_equals_host(which):
    for step in kc.tsp_status_steps():
        fm = 1 if step in (0, 8) else 0
        st, acts = kc.tsp_status_acts(100, which, step, fm)
        kc.check_tsp_ref_against_single_steps(CPU, 100, kc.TSP_STATUS_B, kc.TSP_STATUS_K, fm, acts, st)


@pytest.mark.parametrize("kind", kc.SLAP_KINDS)
@pytest.mark.parametrize("l,p,b,k", [(4, 1, 3, 3), (64, 7, 17, 7), (132, 20, 5, 20), (260, 20, 3, 3)])
def test_slap_reference_equals_host_single_steps(l, p, b, k, kind):
    st = kc.slap_steps_state(l, p, b, k, kind)
    kc.check_slap_ref_against_single_steps(CPU, st, st.product)


@pytest.mark.parametrize("l", [64, 196, 260])
def test_slap_reference_special_rows_equal_host(l):
    st = kc.slap_special_state(l)
    kc.check_slap_ref_against_single_steps(CPU, st, st.product)
    for step in kc.SLAP_STATUS_STEPS:
        st, prod = kc.slap_status_products(l if l != 196 else 256, step)
        kc.check_slap_ref_against_single_steps(CPU, st, prod)
