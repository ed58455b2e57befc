"""The MTVRP kernels (csrc/mtvrp.hip) on the device, through the C ABI: the recorded
episodes of the reference's MTVRPEnv, and reset / mask / step / co_mtvrp_steps / reward
against the restatement tests/mtvrp_ref.py bit for bit on every output, on batches that mix
all four flags per row, over the sizes at which the kernel takes another path -- N + 1 below,
at and above a lane group's two columns per lane (N = 63, 64, 70), more columns per lane (N =
200), a single customer, and batches of 1, 3, 16 and 257 rows (a partial group, a partial
wave, more than one workgroup).  N + 1 on both sides of every switch of mt_launch (N = 15,
16, 31, 32, 62, 63, 64, 127, 128, 255, 256, 511, 512; B = 3), directed rollouts at N = 128,
256, 300, 512, 1023 (B = 4) in which every register slot is the action's at least once and
column N is visited, co_mtvrp_steps at T = 1, 7 and the episode in both action layouts, a
depot -> depot action's `feasible`, co_mtvrp_check on 300 rows with each status bit provoked
in one row, the hand-made rows, the kernel edges and the decode loops.  Only the archive is
read, never a reference checkout."""
import pytest

import mtvrp_cases as mc
from test_host_mtvrp import run_decode_loops

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("policy", mc.POLICIES)
@pytest.mark.parametrize("case", mc.recorded_cases())
def test_device_matches_the_recording(case, policy):
    mc.check_recorded_case(case, policy, DEV)


@pytest.mark.parametrize("n,b", mc.SHAPES)
def test_device_matches_the_restatement(n, b):
    mc.check_shape(n, b, DEV)


@pytest.mark.parametrize("n", mc.SWITCH_SIZES)
def test_both_sides_of_every_launch_switch(n):
    """N + 1 below and at 16, 32, 64 (lanes per row) and 128, 256, 512 (columns per lane)."""
    mc.check_shape(n, 3, DEV)


@pytest.mark.parametrize("n,b", mc.DIRECTED_SHAPES)
def test_every_register_slot_is_the_action(n, b):
    """The directed rollout: every register slot a row's lanes hold is the action's at
    least once and column N is visited -- asserted from the restatement before any kernel
    is compared -- through single steps and co_mtvrp_steps in both action layouts."""
    mc.check_directed_inputs(n, b)
    mc.check_shape(n, b, DEV, directed=True)


def test_hand_made_rows():
    mc.check_hand_made(DEV)


def test_depot_to_depot_feasible():
    mc.check_depot_to_depot(DEV)


def test_kernel_edges():
    mc.check_edges(DEV)


def test_check_bits_over_300_rows():
    mc.check_check_bits(DEV)


def test_decode_loops_on_the_device():
    run_decode_loops(DEV)


def test_mixed_batch_resets_steps_and_rewards_on_the_device():
    """The issue's acceptance line: get_env("mtvrp", num_loc=50, preset "all") on the device."""
    import torch

    from rl4co_slap_amd.envs import get_env
    from rl4co_slap_amd.utils.decoding import random_policy, rollout

    env = get_env("mtvrp", generator_params=dict(num_loc=50, variant_preset="all"), device=DEV,
                  seed=1, check_solution=True)
    td = env.reset(batch_size=[64])
    assert len(set(env.get_variant_names(td))) > 4
    torch.manual_seed(1)
    reward, td, acts = rollout(env, td, random_policy)
    assert reward.is_cuda and bool((reward < 0).all()) and bool(td["done"].all())
