"""The OP kernels (csrc/op.hip, csrc/decode_op.hip) on the device, through the C ABI and
through OPEnv: the recorded episodes of the reference's OPEnv, and reset / step / the mask
alone / co_op_steps against the restatement tests/op_ref.py bit for bit on every output,
floats included, in both action layouts with ``feasible`` and ``length``, at N = 1 (a row of
2), at N + 1 on both sides of every switch of op_launch (the lanes per row double at N + 1 =
32 | 33, 64 | 65, 128 | 129, 256 | 257, 512 | 513) and of the fused step's row engines
(16 | 17 and the same five) and at the largest N the entries take (1023), with batches of 1,
3, 16 and 257 rows (a partial group, a partial wave, more than one workgroup); the directed
episodes (the depot at step 0, the depot after customers and steps after ``done``, every
column the action once, a row closed by the length test alone, a NaN coordinate, actions out
of range); co_op_reward on 300 rows (a second block with a partial tail) with every status
bit alone, T = 1, and the multistart ``prize_batch`` layout.  co_op_decode_step equals
co_decode_step + co_op_step bit for bit and the oracle's decode (tests/fused_step_cases.py)
with the restatement's step, at row lengths 2 ... 1024 on both sides of every row-engine
switch, B = 509 and 1, greedy (exact / certified / fast), sampling and evaluate, (clip,
temperature) = (0, 1) and (10, 0.7), with and without ll_accum, on mid-episode states and the
reset state; with the mask edited in place the entry's two-launch route gives the same
outputs.  Only the archive is read, never a reference checkout."""
import pytest
import torch

import fused_step_cases as fc
import op_cases as oc
from test_host_op import run_decode_loops

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("policy", oc.POLICIES)
@pytest.mark.parametrize("case", oc.recorded_cases())
def test_device_matches_the_recording(case, policy):
    oc.check_recorded_case(case, policy, DEV)


@pytest.mark.parametrize("b", oc.BATCHES)
@pytest.mark.parametrize("n", oc.SIZES)
def test_device_matches_the_restatement(n, b):
    oc.check_shape(n, b, DEV)


@pytest.mark.parametrize("n", oc.SIZES)
def test_every_column_is_the_action_once(n):
    oc.check_every_column(n, DEV)


def test_hand_made_rows():
    oc.check_hand_made(DEV)


def test_reward_and_status_bits_over_two_blocks():
    oc.check_reward_two_blocks(DEV)


def test_reward_sizes_and_multistart_layout():
    oc.check_reward_sizes(DEV)
    oc.check_multistart_reward(DEV)


@pytest.mark.parametrize("mode,flag", oc.DECODES, ids=oc.DECODE_IDS)
@pytest.mark.parametrize("clip,temp", fc.CLIP_TEMP)
@pytest.mark.parametrize("nc", oc.DECODE_NC)
def test_decode_step_equals_the_two_launches_and_the_oracle(nc, clip, temp, mode, flag):
    """B = 509 with ll_accum and B = 1 without."""
    oc.check_decode(DEV, nc, fc.B, mode, flag, clip, temp, with_ll=True)
    oc.check_decode(DEV, nc, 1, mode, flag, clip, temp, with_ll=False)


@pytest.mark.parametrize("mode,flag", oc.DECODES, ids=oc.DECODE_IDS)
@pytest.mark.parametrize("nc", [4, 101, 513])
def test_decode_step_without_ll_accum_on_a_batch(nc, mode, flag):
    oc.check_decode(DEV, nc, fc.B, mode, flag, 10.0, 0.7, with_ll=False)
    oc.check_decode(DEV, nc, 1, mode, flag, 10.0, 0.7, with_ll=True)


@pytest.mark.parametrize("mode,flag", oc.DECODES, ids=oc.DECODE_IDS)
def test_decode_step_with_the_mask_in_place_takes_the_two_launches(mode, flag):
    oc.check_decode_in_place_mask(DEV, 101, mode, flag)


def test_decode_step_out_of_range_evaluate_actions():
    oc.check_decode_out_of_range(DEV)


@pytest.mark.parametrize("fused", [False, True], ids=["pair", "fused"])
def test_decode_loops_on_the_device(fused):
    """Greedy, sampling, POMO multistart and evaluate_policy through the two calls and
    through the fused step; the greedy rollout is the host loop's either way."""
    dev = run_decode_loops(DEV, fused=fused)
    host = run_decode_loops("cpu")
    for kind in ("greedy", "multistart_greedy"):
        assert torch.equal(dev[kind]["actions"].cpu(), host[kind]["actions"]), kind
