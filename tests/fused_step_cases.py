"""Shared by the fused decode + env-step tests (tests/test_gpu_fused_decode_env.py: the three
fused entry points co_tsp_decode_step / co_slap_decode_step / co_cvrp_decode_step on the
device; tests/test_host_fused_step_cases.py: the host build's unfused pair): the inputs, the
expected outputs and the assertions, all from the oracle on the CPU.  Not a test module.

Decode half.  Logits and the input mask are ``sampling_cases.inputs(509, R)`` (R = the row
length) with every row ``b % 8 == 5`` cut down to its first feasible column: those rows
have one possible action in every mode, so the TSP tour ends there (``done``), the CVRP
action is often the depot (column 0 is feasible on 70 % of them) and the CVRP state can
be built around the action (below).  The expected log-probabilities are
``oracle.decoding.process_logits`` with the correctly rounded tanh; greedy is
``oracle.decoding.greedy``, evaluate takes seeded feasible actions, sampling is the
float64 inverse CDF under the Philox draw, compared on the rows ``sampling_cases.
compared_rows`` keeps (its 5 % cap is asserted from the oracle before anything runs).  A
batch of one is the first row of that batch which the oracle compares under row 0's draw
(a cap of 5 % of one row leaves out none).

Env half.  ``oracle.envs`` ``_step`` applied to an arbitrary mid-episode state and the
action: the expected action on every compared row, the library's own (checked feasible)
action on the rows the sampling margin leaves out."""
import collections
import functools

import torch

import sampling_cases as sc
from oracle import decoding as odec
from oracle.envs import CVRPOracle, SLAPOracle, TSPOracle
from oracle.td import TD

B = 509  # a ragged last wave at 16, 8, 4 and 2 rows per wave
CLIP_TEMP = [(0.0, 1.0), (10.0, 0.7)]
MODES = {"greedy": 0, "sampling": 1, "evaluate": 2}
LP_TOL = 1e-5  # CO_DECODE_CERTIFIED: |lp - ref| <= LP_TOL * max(1, |ref|)
ACC_SEED = 77

Decode = collections.namedtuple("Decode", "logits mask want act rows skipped")


def _bits(t):
    return t.contiguous().view(torch.int32)


def single_rows(b):
    """The rows cut down to one feasible action."""
    return torch.arange(b) % 8 == 5


@functools.lru_cache(maxsize=2)
def _reference(b, r, clip, temp):
    logits, mask = sc.inputs(B, r)
    one = single_rows(B)
    first = mask.int().argmax(1)
    only = torch.zeros_like(mask)
    only[torch.arange(B), first] = True
    mask = torch.where(one[:, None], only, mask)
    ref = sc.make_ref(logits, mask, clip, temp)
    if b == B:
        return ref
    assert b == 1
    u0 = odec.decode_draw_u(1, sc.SEED, sc.OFFSET).expand(B)
    _, margin = odec.sample_inverse_cdf(ref.want, u0)
    k = int(((margin > odec.sample_margin_tol(r)) & ~one).nonzero()[0])
    return sc.make_ref(logits[k:k + 1].clone(), mask[k:k + 1].clone(), clip, temp)


def decode_case(b, r, mode, clip=0.0, temp=1.0):
    """The inputs and the oracle's decode of ``b`` (509 or 1) rows of length ``r``."""
    ref = _reference(b, r, float(clip), float(temp))
    rows, skipped = torch.ones(b, dtype=torch.bool), 0
    if mode == "greedy":
        act = odec.greedy(ref.want, ref.mask)
    elif mode == "evaluate":  # a feasible action per row
        g = torch.Generator().manual_seed(7000 + r)
        act = torch.rand(ref.mask.shape, generator=g).masked_fill(~ref.mask, -1.0).argmax(1)
    else:
        act = ref.act
        rows, skipped = sc.compared_rows(ref)  # asserts the cap, from the oracle alone
    return Decode(ref.logits, ref.mask, ref.want, act, rows, skipped)


def acc0(b):
    """The log-likelihood accumulated before the step (ll_accum on entry)."""
    return torch.randn(b, generator=torch.Generator().manual_seed(ACC_SEED)) * 5


def assert_decoded(case, act, lp, ll=None, certified=False):
    """Every action in range and feasible, the oracle's on the compared rows; ``lp`` the
    bits of ``want[b, act[b]]`` (certified: within LP_TOL); ``ll`` the bits of the f32
    ``acc0 + lp``.  Returns the action the env half is expected to have applied."""
    act, lp = act.cpu(), lp.cpu()
    b, n = case.want.shape
    note = f"R={n} B={b}: {case.skipped} rows left out within the margin"
    assert ((act >= 0) & (act < n)).all(), note
    assert case.mask.gather(1, act[:, None]).all(), f"{note}; a masked action was selected"
    bad = (act != case.act) & case.rows
    if bad.any():
        i = bad.nonzero().flatten()[:8]
        raise AssertionError(f"{note}; {int(bad.sum())} of {int(case.rows.sum())} compared rows "
                             f"differ: rows {i.tolist()} got {act[i].tolist()} want "
                             f"{case.act[i].tolist()}")
    want_lp = case.want.gather(1, act[:, None]).squeeze(1)
    if certified:
        assert ((lp - want_lp).abs() <= LP_TOL * want_lp.abs().clamp(min=1)).all(), \
            f"{note}; logp_sel further than {LP_TOL} from want[b, action]"
    else:
        assert torch.equal(_bits(lp), _bits(want_lp)), f"{note}; logp_sel is not want[b, action]"
    if ll is not None:
        assert torch.equal(_bits(ll.cpu()), _bits(acc0(b) + lp)), f"{note}; ll_accum"
    return act


def assert_state(want, got, rows=None):
    """Every entry of ``got`` equal to the oracle's (floats by their bits; bool outputs may
    come as bytes), on ``rows`` if given."""
    assert set(got) == set(want), (sorted(got), sorted(want))
    for k, w in want.items():
        g = got[k].cpu().reshape(w.shape)
        if w.dtype == torch.bool and g.dtype != torch.bool:
            w = w.to(g.dtype)
        assert g.dtype == w.dtype, (k, g.dtype, w.dtype)
        if w.dtype == torch.float32:
            g, w = _bits(g), _bits(w)
        if rows is not None:
            g, w = g[rows], w[rows]
        if not torch.equal(g, w):
            bad = (g != w).reshape(g.shape[0], -1).any(1).nonzero().flatten()
            raise AssertionError(f"{k}: {bad.numel()} rows differ from the oracle, first "
                                 f"{bad[:8].tolist()}")


# ------------------------------------------------------------------------------- TSP
def tsp_state(case, first_mode):
    """i[B,1] >= 1 everywhere (first_mode 0: the reference keeps first_node) or with one
    zero (first_mode 1: its batch-wide ``i.all() == 0`` takes the action); first_node."""
    b, n = case.want.shape
    g = torch.Generator().manual_seed(2000 + n)
    i = torch.randint(1, n + 1, (b, 1), generator=g)
    if first_mode:
        i[b // 2] = 0
    return {"i": i, "first_node": torch.randint(0, n, (b,), generator=g)}


def tsp_expect(case, state, action):
    b = action.shape[0]
    td = TD({"action": action, "i": state["i"].clone(), "first_node": state["first_node"].clone(),
             "action_mask": case.mask.clone()}, b)
    out = TSPOracle._step(td)
    return {k: out[k] for k in ("first_node", "i", "action_mask", "reward", "done")}


# ------------------------------------------------------------------------------ SLAP
def slap_state(case, p, product=None):
    """to_choose[B,P] (column 0: the row's product, or ``product`` on every row), a partly
    filled assignment[B,P], i[B,1] on both sides of P - 1."""
    b, n = case.want.shape
    g = torch.Generator().manual_seed(3000 + 7 * n + p)
    tc = torch.randint(0, p, (b, p), generator=g).float()
    if product is not None:
        tc[:, 0] = product
    asg = torch.randint(-1, n, (b, p), generator=g).to(torch.int32)
    i = torch.randint(0, p + 2, (b, 1), generator=g)
    i[0::3] = p - 1
    i[1::3] = max(p - 2, 0)
    i[2::6] = p
    return {"to_choose": tc, "assignment": asg, "i": i}


def slap_expect(case, state, action):
    b = action.shape[0]
    p = state["assignment"].shape[1]
    td = TD({"action": action, "to_choose": state["to_choose"].clone(),
             "assignment": state["assignment"].clone(), "i": state["i"].clone(),
             "freq": torch.zeros(b, p, 1), "action_mask": case.mask.clone()}, b)
    out = SLAPOracle._step(td)
    return {k: out[k] for k in ("assignment", "action_mask", "i", "reward", "done")}


# ------------------------------------------------------------------------------ CVRP
def cvrp_state(case):
    """Rows of N + 1 = R columns.  Demands k/30 (k = 1..9), a vehicle capacity of 1 or
    1.2, used capacity j/30 chosen so that after the selected demand the strict
    ``demand + used > capacity`` is decided within one demand of the capacity -- on the
    edge (j + k_a + k_c = 30 or 36) for about one column in nine; visited bytes 30 % set,
    some with the value 2; the single-action rows all visited except the action (the
    action completes the tour) or, every other one, except the action and one more."""
    b, r = case.want.shape
    n = r - 1
    g = torch.Generator().manual_seed(4000 + r)
    demand = torch.randint(1, 10, (b, n), generator=g).float() / 30.0
    big = torch.rand(b, 1, generator=g) < 0.5
    vcap = torch.where(big, torch.tensor(1.2), torch.tensor(1.0))
    used = (torch.randint(16, 25, (b, 1), generator=g) + 6 * big).float() / 30.0
    visited = (torch.rand(b, r, generator=g) < 0.3).to(torch.uint8)
    visited[torch.arange(b) % 16 == 3, 5 % r] = 2
    one = single_rows(b).nonzero().flatten()
    visited[one] = 1
    visited[one, case.act[one]] = 0
    visited[one[1::2], (case.act[one[1::2]] + 1) % r] = 0
    return {"demand": demand, "used_capacity": used, "vehicle_capacity": vcap,
            "visited": visited}


def cvrp_expect(case, state, action):
    b = action.shape[0]
    td = TD({"action": action, **{k: v.clone() for k, v in state.items()}}, b)
    out = CVRPOracle._step(CVRPOracle.__new__(CVRPOracle), td)
    return {k: out[k] for k in ("current_node", "used_capacity", "visited", "reward", "done",
                                "action_mask")}


def out_of_range_actions(case):
    """Evaluate actions with every sixth row out of range (negative, R, far beyond):
    -> (action_in, rows in range, a feasible stand-in action for the oracle's env step)."""
    b, r = case.want.shape
    act = case.act.clone()
    bad = torch.arange(b) % 6 == 1
    vals = torch.tensor([-1, r, -r - 1, r + 7, -2 ** 40, 2 ** 40])
    act[bad] = vals[torch.arange(int(bad.sum())) % len(vals)]
    return act, ~bad, case.act
