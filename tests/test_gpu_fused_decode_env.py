"""The three fused decode + env-step entry points (co_tsp_decode_step, co_slap_decode_step,
co_cvrp_decode_step: every step of a policy rollout) pinned to the oracle on every
dispatch path.  tests/fused_step_cases.py builds the inputs and, from oracle.decoding and
oracle.envs alone, every expected output: action, logp_sel, ll_accum, the env state, the
step reward and the status word.  Without a math flag everything is bit-equal; under
CO_DECODE_CERTIFIED (greedy) actions and state are equal and logp_sel is within
1e-5 * max(1, |logp|).

Row lengths sit on both sides of every row-length bucket of the decode engines (16 / 32 /
64 / 128 / 256 / 512 / 1024 / 2048 columns; 16, 16, 8, 4, 2, 1, 1, 1 rows per wave) and
take every load width (rows of a multiple of 4: vector; others: 4-column chunks with a
clamped tail; fewer than 4 columns: pairs).  509 rows end inside a wave at every
rows-per-wave; one row is a lone lane group.

The two-launch route (co_decode_step + the env's step kernel) that co_slap_decode_step /
co_cvrp_decode_step take when the staged env state does not fit or rows are misaligned is
not documented by include/co_env.h; the cases that take it are named here from the
launchers' conditions, give the same expected values, and return CO_E_INVAL with ll_accum.

Not asserted (include/co_env.h does not define it): any output of a row whose evaluate
action is out of range, apart from the CO_ST_INDEX_RANGE status bit."""
import pytest
import torch

import fused_step_cases as fc
import sampling_cases as sc
from rl4co_slap_amd import _native as nat
from test_gpu_decode_certified import _offset_rows

pytestmark = pytest.mark.gpu

POISON = 0xCC  # every output starts as this byte pattern: an element left unwritten differs

# mode, math flag
DECODES = [("greedy", 0), ("greedy", nat.DECODE_CERTIFIED), ("sampling", 0), ("evaluate", 0)]
DECODE_IDS = ["greedy", "greedy_certified", "sampling", "evaluate"]

TSP_N = [3, 5, 16, 17, 20, 33, 64, 65, 100, 129, 256, 260, 513, 1024, 1028, 2048]
SLAP_LP = [(3, 1), (5, 3), (16, 16), (17, 5), (20, 20), (33, 7), (64, 20), (65, 33), (100, 20),
           (129, 40), (256, 128), (260, 20), (513, 20), (1024, 64), (1028, 20), (2048, 20)]
CVRP_N = [2, 4, 15, 16, 19, 23, 32, 63, 64, 99, 100, 128, 129, 255, 259, 260, 512, 1023, 2047]
# co_cvrp_decode_step's two-launch route: (rows per wave * (N + 1)) % 4 != 0 at 128, 260
# and 512; at 2047 the four waves' stages (demand + visited rows, 41 KB) and the decode's
# 32 KB of scratch exceed the 64 KB of LDS
CVRP_TWO_LAUNCH = {128, 260, 512, 2047}


def _out(dev, shape, dtype):
    """A poisoned output with 64 guard bytes behind it -> (tensor, guard)."""
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    n = 1
    for s in shape:
        n *= s
    size = torch.empty((), dtype=dtype).element_size()
    raw = torch.full((n * size + 64,), POISON, dtype=torch.uint8, device=dev)
    return raw[:n * size].view(dtype).view(shape), raw[n * size:]


class _Outs(dict):
    """Named poisoned outputs; ``check_guards`` after the launch."""

    def __init__(self, dev):
        super().__init__()
        self.dev, self.guards = dev, {}

    def new(self, name, shape, dtype):
        self[name], self.guards[name] = _out(self.dev, shape, dtype)
        return nat.ptr(self[name])

    def check_guards(self):
        for k, g in self.guards.items():
            assert bool((g == POISON).all()), f"{k}: bytes behind the output were written"


def _place(t, dev, layout, pad=3):
    if layout == "misaligned":  # rows off a 16-byte / 4-byte boundary
        return _offset_rows(t, dev)
    if layout == "strided":  # a row stride of R + pad, as a view of a wider tensor
        b, r = t.shape
        v = torch.zeros(b, r + pad, dtype=t.dtype, device=dev)[:, :r]
        v.copy_(t)
        return v
    return t.to(dev)


def _decode_args(dev, case, mode, flag, clip, temp, o, layout="aligned", action_in=None):
    """The decode half's arguments shared by the three entry points:
    (logits, stride, mask_in, clip, temp, mode word, action_in, action_out, logp_sel, seed,
    offset) and the tensors that must outlive the launch."""
    b, r = case.want.shape
    lg = _place(case.logits, dev, layout)
    mk = _place(case.mask, dev, "misaligned" if layout == "misaligned" else "aligned")
    ain = None
    if mode == "evaluate":
        ain = (case.act if action_in is None else action_in).to(dev)
    args = (nat.ptr(lg), lg.stride(0), nat.ptr(mk), float(clip), float(temp),
            fc.MODES[mode] | flag, nat.ptr(ain), o.new("action", b, torch.int64),
            o.new("logp", b, torch.float32), sc.SEED, sc.OFFSET)
    return args, (lg, mk, ain)


def _ll(dev, b, with_ll):
    return fc.acc0(b).to(dev) if with_ll else None


def _finish(o, st, case, ll, flag, status=0):
    torch.cuda.synchronize()
    o.check_guards()
    assert int(st.item()) == status
    return fc.assert_decoded(case, o.pop("action"), o.pop("logp"), ll, certified=flag != 0)


# ------------------------------------------------------------------------------- TSP
def _tsp(dev, case, mode, flag, clip, temp, first_mode=0, layout="aligned", with_ll=True,
         action_in=None):
    b, n = case.want.shape
    state = fc.tsp_state(case, first_mode)
    o = _Outs(dev)
    dargs, keep = _decode_args(dev, case, mode, flag, clip, temp, o, layout, action_in)
    i_in, first_in = state["i"].to(dev), state["first_node"].to(dev)
    ll = _ll(dev, b, with_ll)
    st = torch.zeros(1, dtype=torch.int32, device=dev)
    nat.call("co_tsp_decode_step", b, n, *dargs, o.new("action_mask", (b, n), torch.uint8),
             nat.ptr(i_in), o.new("i", (b, 1), torch.int64),
             None if first_mode else nat.ptr(first_in), o.new("first_node", b, torch.int64),
             first_mode, o.new("done", b, torch.uint8), o.new("reward", b, torch.uint8),
             nat.ptr(ll), nat.ptr(st), nat.stream_of(i_in))
    return state, o, st, ll


@pytest.mark.parametrize("mode,flag", DECODES, ids=DECODE_IDS)
@pytest.mark.parametrize("clip,temp", fc.CLIP_TEMP)
@pytest.mark.parametrize("first_mode", [0, 1])
@pytest.mark.parametrize("n", TSP_N)
def test_tsp_decode_step_matches_oracle(dev, n, first_mode, clip, temp, mode, flag):
    case = fc.decode_case(fc.B, n, mode, clip, temp)
    state, o, st, ll = _tsp(dev, case, mode, flag, clip, temp, first_mode)
    act = _finish(o, st, case, ll, flag)
    fc.assert_state(fc.tsp_expect(case, state, act), o)


@pytest.mark.parametrize("mode,flag", DECODES, ids=DECODE_IDS)
@pytest.mark.parametrize("layout,with_ll", [("strided", True), ("misaligned", True),
                                            ("aligned", False)])
@pytest.mark.parametrize("n", [20, 100, 129])
def test_tsp_decode_step_layouts(dev, n, layout, with_ll, mode, flag):
    """A logits row stride of N + 3, logits and masks off a 16-byte boundary, and
    ll_accum = NULL: the same results on the any-alignment loads."""
    case = fc.decode_case(fc.B, n, mode, 10.0, 0.7)
    state, o, st, ll = _tsp(dev, case, mode, flag, 10.0, 0.7, 0, layout, with_ll)
    act = _finish(o, st, case, ll, flag)
    fc.assert_state(fc.tsp_expect(case, state, act), o)


@pytest.mark.parametrize("mode,flag", DECODES, ids=DECODE_IDS)
@pytest.mark.parametrize("clip,temp", fc.CLIP_TEMP)
@pytest.mark.parametrize("n", TSP_N)
def test_tsp_decode_step_single_row(dev, n, clip, temp, mode, flag):
    case = fc.decode_case(1, n, mode, clip, temp)
    state, o, st, ll = _tsp(dev, case, mode, flag, clip, temp, 1)
    act = _finish(o, st, case, ll, flag)
    fc.assert_state(fc.tsp_expect(case, state, act), o)


# ------------------------------------------------------------------------------ SLAP
def _slap(dev, case, p, mode, flag, clip, temp, in_place=False, with_ll=True, product=None,
          null_to_choose=False, action_in=None):
    b, l = case.want.shape
    state = fc.slap_state(case, p, product)
    o = _Outs(dev)
    dargs, keep = _decode_args(dev, case, mode, flag, clip, temp, o, action_in=action_in)
    tc, asg, i_in = (state[k].to(dev) for k in ("to_choose", "assignment", "i"))
    if in_place:  # assign_out == assign_in, mask_out == mask_in, i_out == i_in
        o["assignment"], o["action_mask"], o["i"] = asg, keep[1].view(torch.uint8), i_in
        outs = (nat.ptr(asg), nat.ptr(keep[1]))
        i_out = nat.ptr(i_in)
    else:
        outs = (o.new("assignment", (b, p), torch.int32), o.new("action_mask", (b, l), torch.uint8))
        i_out = o.new("i", (b, 1), torch.int64)
    ll = _ll(dev, b, with_ll)
    st = torch.zeros(1, dtype=torch.int32, device=dev)
    nat.call("co_slap_decode_step", b, l, p, *dargs,
             None if null_to_choose else nat.ptr(tc), product if null_to_choose else p,
             nat.ptr(asg), *outs, nat.ptr(i_in), i_out, o.new("done", (b, 1), torch.uint8),
             o.new("reward", (b, 1), torch.uint8), nat.ptr(ll), nat.ptr(st), nat.stream_of(tc))
    return state, o, st, ll


@pytest.mark.parametrize("mode,flag", DECODES, ids=DECODE_IDS)
@pytest.mark.parametrize("clip,temp", fc.CLIP_TEMP)
@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("l,p", SLAP_LP)
def test_slap_decode_step_matches_oracle(dev, l, p, in_place, clip, temp, mode, flag):
    """In place the assignment row is the input's apart from the written element: the
    expected row is the oracle's clone with that element set."""
    case = fc.decode_case(fc.B, l, mode, clip, temp)
    state, o, st, ll = _slap(dev, case, p, mode, flag, clip, temp, in_place)
    act = _finish(o, st, case, ll, flag)
    fc.assert_state(fc.slap_expect(case, state, act), o)


@pytest.mark.parametrize("mode,flag", DECODES, ids=DECODE_IDS)
@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("l,p,k", [(5, 3, 2), (20, 20, 0), (100, 20, 19), (129, 40, 7),
                                   (513, 20, 11)])
def test_slap_decode_step_null_to_choose(dev, l, p, k, in_place, mode, flag):
    """to_choose = NULL with tc_stride = k against a to_choose whose column 0 is k."""
    case = fc.decode_case(fc.B, l, mode, 10.0, 0.7)
    for null in (False, True):
        state, o, st, ll = _slap(dev, case, p, mode, flag, 10.0, 0.7, in_place, product=k,
                                 null_to_choose=null)
        act = _finish(o, st, case, ll, flag)
        fc.assert_state(fc.slap_expect(case, state, act), o)


@pytest.mark.parametrize("mode,flag", DECODES, ids=DECODE_IDS)
@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
def test_slap_decode_step_beyond_the_stage(dev, in_place, mode, flag):
    """L = 16, P = 300: 16 rows per wave of 304 staged dwords exceed the LDS; the two
    launches give the same results, and ll_accum is refused (CO_E_INVAL)."""
    case = fc.decode_case(fc.B, 16, mode, 10.0, 0.7)
    state, o, st, ll = _slap(dev, case, 300, mode, flag, 10.0, 0.7, in_place, with_ll=False)
    act = _finish(o, st, case, ll, flag)
    fc.assert_state(fc.slap_expect(case, state, act), o)
    with pytest.raises(RuntimeError, match="status -1$"):
        _slap(dev, case, 300, mode, flag, 10.0, 0.7, in_place, with_ll=True)


@pytest.mark.parametrize("mode,flag", DECODES, ids=DECODE_IDS)
@pytest.mark.parametrize("clip,temp", fc.CLIP_TEMP)
@pytest.mark.parametrize("l,p", SLAP_LP)
def test_slap_decode_step_single_row(dev, l, p, clip, temp, mode, flag):
    case = fc.decode_case(1, l, mode, clip, temp)
    for in_place in (False, True):
        state, o, st, ll = _slap(dev, case, p, mode, flag, clip, temp, in_place)
        act = _finish(o, st, case, ll, flag)
        fc.assert_state(fc.slap_expect(case, state, act), o)


# ------------------------------------------------------------------------------ CVRP
def _cvrp(dev, case, mode, flag, clip, temp, with_ll=True, demand_offset=False, alias=None,
          action_in=None):
    b, r = case.want.shape
    n = r - 1
    state = fc.cvrp_state(case)
    o = _Outs(dev)
    dargs, keep = _decode_args(dev, case, mode, flag, clip, temp, o, action_in=action_in)
    dem = _offset_rows(state["demand"], dev) if demand_offset else state["demand"].to(dev)
    used, vcap, vis = (state[k].to(dev) for k in ("used_capacity", "vehicle_capacity", "visited"))
    ll = _ll(dev, b, with_ll)
    st = torch.zeros(1, dtype=torch.int32, device=dev)
    used_out = o.new("used_capacity", (b, 1), torch.float32)
    vis_out = nat.ptr(vis) if alias == "visited" else o.new("visited", (b, r), torch.uint8)
    mask_out = nat.ptr(keep[1]) if alias == "mask" else o.new("action_mask", (b, r), torch.uint8)
    nat.call("co_cvrp_decode_step", b, n, *dargs, nat.ptr(dem), nat.ptr(used), used_out,
             nat.ptr(vcap), nat.ptr(vis), vis_out, o.new("current_node", (b, 1), torch.int64),
             o.new("done", b, torch.uint8), o.new("reward", b, torch.uint8), mask_out,
             nat.ptr(ll), nat.ptr(st), nat.stream_of(used))
    return state, o, st, ll


@pytest.mark.parametrize("mode,flag", DECODES, ids=DECODE_IDS)
@pytest.mark.parametrize("clip,temp", fc.CLIP_TEMP)
@pytest.mark.parametrize("n", CVRP_N)
def test_cvrp_decode_step_matches_oracle(dev, n, clip, temp, mode, flag):
    """N = 129 and 259 (two and one rows of 129 / 259 demands per wave) have the wave's
    demand block 16-byte aligned in some waves only: both DMA widths in one launch."""
    case = fc.decode_case(fc.B, n + 1, mode, clip, temp)
    state, o, st, ll = _cvrp(dev, case, mode, flag, clip, temp, with_ll=n not in CVRP_TWO_LAUNCH)
    act = _finish(o, st, case, ll, flag)
    fc.assert_state(fc.cvrp_expect(case, state, act), o)


@pytest.mark.parametrize("mode,flag", DECODES, ids=DECODE_IDS)
@pytest.mark.parametrize("n", sorted(CVRP_TWO_LAUNCH))
def test_cvrp_decode_step_two_launch_route_refuses_ll_accum(dev, n, mode, flag):
    case = fc.decode_case(fc.B, n + 1, mode, 10.0, 0.7)
    with pytest.raises(RuntimeError, match="status -1$"):
        _cvrp(dev, case, mode, flag, 10.0, 0.7, with_ll=True)


@pytest.mark.parametrize("mode,flag", DECODES, ids=DECODE_IDS)
@pytest.mark.parametrize("n", [19, 100, 129, 1023])
def test_cvrp_decode_step_demand_off_16_bytes(dev, n, mode, flag):
    """demand 4 bytes into a larger buffer: no wave's block is 16-byte aligned at N = 19
    and 100 (a multiple of 4 floats per wave), so every wave stages it dword by dword."""
    case = fc.decode_case(fc.B, n + 1, mode, 10.0, 0.7)
    state, o, st, ll = _cvrp(dev, case, mode, flag, 10.0, 0.7, demand_offset=True)
    act = _finish(o, st, case, ll, flag)
    fc.assert_state(fc.cvrp_expect(case, state, act), o)


@pytest.mark.parametrize("alias", ["mask", "visited"])
@pytest.mark.parametrize("n", [19, 128])
def test_cvrp_decode_step_refuses_in_place_rows(dev, n, alias):
    case = fc.decode_case(fc.B, n + 1, "greedy", 10.0, 0.7)
    with pytest.raises(RuntimeError, match="status -1$"):
        _cvrp(dev, case, "greedy", 0, 10.0, 0.7, with_ll=False, alias=alias)


@pytest.mark.parametrize("mode,flag", DECODES, ids=DECODE_IDS)
@pytest.mark.parametrize("clip,temp", fc.CLIP_TEMP)
@pytest.mark.parametrize("n", CVRP_N)
def test_cvrp_decode_step_single_row(dev, n, clip, temp, mode, flag):
    case = fc.decode_case(1, n + 1, mode, clip, temp)
    state, o, st, ll = _cvrp(dev, case, mode, flag, clip, temp, with_ll=n not in CVRP_TWO_LAUNCH)
    act = _finish(o, st, case, ll, flag)
    fc.assert_state(fc.cvrp_expect(case, state, act), o)


# ------------------------------------------- rows the reference would raise on
@pytest.mark.parametrize("env", ["tsp", "slap", "cvrp"])
@pytest.mark.parametrize("r", [5, 20, 100, 130, 513])
def test_out_of_range_evaluate_actions_set_the_status_bit(dev, env, r):
    """Evaluate actions that are negative or >= the row length: CO_ST_INDEX_RANGE, and
    every other row of the batch still equals the oracle.  Nothing else is asserted on the
    out-of-range rows."""
    case = fc.decode_case(fc.B, r, "evaluate", 10.0, 0.7)
    ain, ok, stand_in = fc.out_of_range_actions(case)
    if env == "tsp":
        state, o, st, ll = _tsp(dev, case, "evaluate", 0, 10.0, 0.7, action_in=ain)
        want = fc.tsp_expect(case, state, stand_in)
    elif env == "slap":
        state, o, st, ll = _slap(dev, case, 20, "evaluate", 0, 10.0, 0.7, action_in=ain)
        want = fc.slap_expect(case, state, stand_in)
    else:
        state, o, st, ll = _cvrp(dev, case, "evaluate", 0, 10.0, 0.7, action_in=ain,
                                 with_ll=r - 1 not in CVRP_TWO_LAUNCH)
        want = fc.cvrp_expect(case, state, stand_in)
    torch.cuda.synchronize()
    o.check_guards()
    assert int(st.item()) & nat.ST_INDEX_RANGE
    act, lp = o.pop("action").cpu(), o.pop("logp").cpu()
    assert torch.equal(act[ok], case.act[ok])
    want_lp = case.want.gather(1, case.act[:, None]).squeeze(1)
    assert torch.equal(lp[ok].view(torch.int32), want_lp[ok].view(torch.int32))
    if ll is not None:
        assert torch.equal(ll.cpu()[ok].view(torch.int32),
                           (fc.acc0(fc.B) + want_lp)[ok].view(torch.int32))
    fc.assert_state(want, o, rows=ok)
