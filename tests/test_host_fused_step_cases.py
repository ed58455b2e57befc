"""The cases of tests/fused_step_cases.py through the host build's unfused pair on CPU
tensors: decode_step (csrc/host co_decode_step) followed by co_tsp_step / co_slap_step /
co_cvrp_step, every output equal to the oracle's.  Runs without a GPU, so it validates
the case builder and the oracle's 5 % cap that tests/test_gpu_fused_decode_env.py relies
on, and pins the host build's decode -> env-step composition to the oracle."""
import pytest
import torch

import fused_step_cases as fc
import sampling_cases as sc
from rl4co_slap_amd import _native as nat
from rl4co_slap_amd.utils.decoding import decode_step

ROW_LENGTHS = [3, 17, 100, 129, 260, 2048]
MODES = ["greedy", "sampling", "evaluate"]


def _decode(case, mode, clip, temp, action_in=None):
    """-> (the action the env step takes, status word tensor)."""
    st = torch.zeros(1, dtype=torch.int32)
    ain = None
    if mode == "evaluate":
        ain = case.act if action_in is None else action_in
    act, lp, _ = decode_step(case.logits, case.mask, mode, temp, clip, action=ain, seed=sc.SEED,
                             offset=sc.OFFSET, status=st)
    return act, lp, st


def _empty(shape, dtype):
    return torch.full(shape, 0x33, dtype=dtype)


def _tsp_step(case, state, act, first_mode, st):
    b, n = case.want.shape
    o = {"action_mask": _empty((b, n), torch.uint8), "i": _empty((b, 1), torch.int64),
         "first_node": _empty((b,), torch.int64), "done": _empty((b,), torch.uint8),
         "reward": _empty((b,), torch.uint8)}
    nat.call("co_tsp_step", b, n, nat.ptr(act), nat.ptr(case.mask), nat.ptr(o["action_mask"]),
             nat.ptr(state["i"]), nat.ptr(o["i"]),
             None if first_mode else nat.ptr(state["first_node"]), nat.ptr(o["first_node"]), None,
             nat.ptr(o["done"]), nat.ptr(o["reward"]), first_mode, None, nat.ptr(st), nat.HOST)
    return o


def _slap_step(case, state, act, st):
    b, l = case.want.shape
    p = state["assignment"].shape[1]
    o = {"assignment": _empty((b, p), torch.int32), "action_mask": _empty((b, l), torch.uint8),
         "i": _empty((b, 1), torch.int64), "done": _empty((b, 1), torch.uint8),
         "reward": _empty((b, 1), torch.uint8)}
    nat.call("co_slap_step", b, l, p, nat.ptr(act), nat.ptr(state["to_choose"]), p,
             nat.ptr(state["assignment"]), nat.ptr(o["assignment"]), nat.ptr(case.mask),
             nat.ptr(o["action_mask"]), nat.ptr(state["i"]), nat.ptr(o["i"]), nat.ptr(o["done"]),
             nat.ptr(o["reward"]), nat.ptr(st), nat.HOST)
    return o


def _cvrp_step(case, state, act, st):
    b, r = case.want.shape
    o = {"used_capacity": _empty((b, 1), torch.float32), "visited": _empty((b, r), torch.uint8),
         "current_node": _empty((b, 1), torch.int64), "done": _empty((b,), torch.uint8),
         "reward": _empty((b,), torch.uint8), "action_mask": _empty((b, r), torch.uint8)}
    nat.call("co_cvrp_step", b, r - 1, nat.ptr(act), nat.ptr(state["demand"]),
             nat.ptr(state["used_capacity"]), nat.ptr(o["used_capacity"]),
             nat.ptr(state["vehicle_capacity"]), nat.ptr(state["visited"]), nat.ptr(o["visited"]),
             nat.ptr(o["current_node"]), nat.ptr(o["done"]), nat.ptr(o["reward"]),
             nat.ptr(o["action_mask"]), nat.ptr(st), None, nat.HOST)
    return o


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("clip,temp", fc.CLIP_TEMP)
@pytest.mark.parametrize("first_mode", [0, 1])
@pytest.mark.parametrize("n", ROW_LENGTHS)
def test_host_decode_then_tsp_step_matches_oracle(n, first_mode, clip, temp, mode):
    case = fc.decode_case(fc.B, n, mode, clip, temp)
    state = fc.tsp_state(case, first_mode)
    act, lp, st = _decode(case, mode, clip, temp)
    act = fc.assert_decoded(case, act, lp)
    fc.assert_state(fc.tsp_expect(case, state, act), _tsp_step(case, state, act, first_mode, st))
    assert int(st.item()) == 0


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("clip,temp", fc.CLIP_TEMP)
@pytest.mark.parametrize("l,p", [(3, 1), (17, 5), (100, 20), (129, 40), (260, 20), (2048, 20)])
def test_host_decode_then_slap_step_matches_oracle(l, p, clip, temp, mode):
    case = fc.decode_case(fc.B, l, mode, clip, temp)
    state = fc.slap_state(case, p)
    act, lp, st = _decode(case, mode, clip, temp)
    act = fc.assert_decoded(case, act, lp)
    fc.assert_state(fc.slap_expect(case, state, act), _slap_step(case, state, act, st))
    assert int(st.item()) == 0


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("clip,temp", fc.CLIP_TEMP)
@pytest.mark.parametrize("r", ROW_LENGTHS)
def test_host_decode_then_cvrp_step_matches_oracle(r, clip, temp, mode):
    case = fc.decode_case(fc.B, r, mode, clip, temp)
    state = fc.cvrp_state(case)
    act, lp, st = _decode(case, mode, clip, temp)
    act = fc.assert_decoded(case, act, lp)
    fc.assert_state(fc.cvrp_expect(case, state, act), _cvrp_step(case, state, act, st))
    assert int(st.item()) == 0


@pytest.mark.parametrize("r", ROW_LENGTHS)
def test_host_single_row_case(r):
    """The batch of one: a row the oracle compares under row 0's draw."""
    for clip, temp in fc.CLIP_TEMP:
        case = fc.decode_case(1, r, "sampling", clip, temp)
        assert case.skipped == 0 and bool(case.rows.all())
        act, lp, st = _decode(case, "sampling", clip, temp)
        fc.assert_decoded(case, act, lp)
        assert int(st.item()) == 0


@pytest.mark.parametrize("env", ["tsp", "slap", "cvrp"])
def test_host_out_of_range_evaluate_actions_set_the_status_bit(env):
    """The rows the reference would raise on: CO_ST_INDEX_RANGE; every other row equals
    the oracle."""
    case = fc.decode_case(fc.B, 100, "evaluate", 10.0, 0.7)
    ain, ok, stand_in = fc.out_of_range_actions(case)
    act, lp, st = _decode(case, "evaluate", 10.0, 0.7, action_in=ain)
    assert int(st.item()) & nat.ST_INDEX_RANGE
    assert torch.equal(act[ok], case.act[ok])
    if env == "tsp":
        state = fc.tsp_state(case, 0)
        got, want = _tsp_step(case, state, act, 0, st), fc.tsp_expect(case, state, stand_in)
    elif env == "slap":
        state = fc.slap_state(case, 20)
        got, want = _slap_step(case, state, act, st), fc.slap_expect(case, state, stand_in)
    else:
        state = fc.cvrp_state(case)
        got, want = _cvrp_step(case, state, act, st), fc.cvrp_expect(case, state, stand_in)
    fc.assert_state(want, got, rows=ok)


def test_cases_exercise_the_edges_they_claim():
    """The CVRP state has the strict capacity comparison on the edge (demand + used equal
    to the capacity in exact arithmetic) for many columns, actions at the depot and away
    from it, and rows whose action completes the tour; the TSP case has finished rows."""
    case = fc.decode_case(fc.B, 100, "greedy", 10.0, 0.7)
    state = fc.cvrp_state(case)
    want = fc.cvrp_expect(case, state, case.act)
    k = lambda x: (x.double() * 30).round().long()
    u, d, c = k(want["used_capacity"]), k(state["demand"]), k(state["vehicle_capacity"])
    assert int((u + d == c).sum()) > fc.B * 99 // 20
    assert int((case.act == 0).sum()) >= 16 and int((case.act != 0).sum()) >= 16
    assert 8 <= int(want["done"].sum()) < fc.B // 4
    tsp = fc.tsp_expect(case, fc.tsp_state(case, 0), case.act)
    assert 8 <= int(tsp["done"].sum()) < fc.B // 4
