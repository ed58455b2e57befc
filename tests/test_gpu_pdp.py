"""The PDP kernels (csrc/pdp.hip, csrc/decode_pdp.hip) on the device, through the C ABI and
through PDPEnv: the recorded episodes of the reference's PDPEnv, and reset / step /
co_pdp_steps against the restatement tests/pdp_ref.py bit for bit on every output, in both
action layouts, at N = 2 (a row of 3), at N + 1 on both sides of every switch of pdp_launch
(the lanes per row double at N + 1 = 32, 64, 128, 256, 512, 1024: N = 30 | 32, 62 | 64,
126 | 128, 254 | 256, 510 | 512, 1022 | 1024) and at the largest N the entries take (2046),
with batches of 1, 3, 16 and 257 rows (a partial group, a partial wave, more than one
workgroup); full episodes in which every column -- every bit position a lane holds -- is the
action's and the pair's; the hand-made rows; co_pdp_reward on 300 rows (a second block with a
partial tail) with every status bit alone, and the multistart ``locs_batch`` layout.
co_pdp_decode_step equals co_decode_step + co_pdp_step bit for bit and the oracle's decode
(tests/fused_step_cases.py) with the restatement's step, at row lengths 3 ... 2047, B = 509
and 1, greedy (exact / certified / fast), sampling and evaluate, (clip, temperature) = (0, 1)
and (10, 0.7), with and without ll_accum, on mid-episode states and the reset state; with the
mask edited in place the entry's two-launch route gives the same outputs.  Only the archive is
read, never a reference checkout."""
import pytest
import torch

import fused_step_cases as fc
import pdp_cases as pc
from test_host_pdp import EPISODES, run_decode_loops

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("policy", pc.POLICIES)
@pytest.mark.parametrize("case", EPISODES)
def test_device_matches_the_recording(case, policy):
    pc.check_recorded_case(case, policy, DEV)


def test_device_matches_the_recorded_multistart_episode():
    pc.check_recorded_multistart(DEV)


@pytest.mark.parametrize("b", pc.BATCHES)
@pytest.mark.parametrize("n", pc.SIZES)
def test_device_matches_the_restatement(n, b):
    pc.check_shape(n, b, DEV)


@pytest.mark.parametrize("n", pc.SIZES)
def test_every_column_is_the_action_and_the_pair(n):
    """The full episode: every column -- every bit position of every lane's word -- is the
    action's and the pair's at least once, asserted from the restatement before any kernel is
    compared, through single steps and co_pdp_steps in both action layouts."""
    pc.check_directed_inputs(n, 2)
    pc.check_shape(n, 2, DEV, full=True)


def test_hand_made_rows():
    pc.check_hand_made(DEV)


def test_reward_and_validity_bits_over_two_blocks():
    pc.check_reward_two_blocks(DEV)


def test_reward_sizes_and_multistart_layout():
    pc.check_reward_sizes(DEV)
    pc.check_multistart_reward(DEV)


@pytest.mark.parametrize("mode,flag", pc.DECODES, ids=pc.DECODE_IDS)
@pytest.mark.parametrize("clip,temp", fc.CLIP_TEMP)
@pytest.mark.parametrize("nc", pc.DECODE_NC)
def test_decode_step_equals_the_two_launches_and_the_oracle(nc, clip, temp, mode, flag):
    """B = 509 with ll_accum and B = 1 without."""
    pc.check_decode(DEV, nc, fc.B, mode, flag, clip, temp, with_ll=True)
    pc.check_decode(DEV, nc, 1, mode, flag, clip, temp, with_ll=False)


@pytest.mark.parametrize("mode,flag", pc.DECODES, ids=pc.DECODE_IDS)
@pytest.mark.parametrize("nc", [5, 101, 513])
def test_decode_step_without_ll_accum_on_a_batch(nc, mode, flag):
    pc.check_decode(DEV, nc, fc.B, mode, flag, 10.0, 0.7, with_ll=False)
    pc.check_decode(DEV, nc, 1, mode, flag, 10.0, 0.7, with_ll=True)


@pytest.mark.parametrize("mode,flag", pc.DECODES, ids=pc.DECODE_IDS)
def test_decode_step_with_the_mask_in_place_takes_the_two_launches(mode, flag):
    pc.check_decode_in_place_mask(DEV, 101, mode, flag)


def test_decode_step_out_of_range_evaluate_actions():
    pc.check_decode_out_of_range(DEV)


def test_decode_loops_on_the_device():
    """Greedy, sampling, POMO multistart and evaluate_policy through the fused step; the
    greedy rollout is the host loop's (the two-call path on the host build)."""
    dev = run_decode_loops(DEV)
    host = run_decode_loops("cpu")
    for kind in ("greedy", "multistart_greedy"):
        assert torch.equal(dev[kind]["actions"].cpu(), host[kind]["actions"]), kind
