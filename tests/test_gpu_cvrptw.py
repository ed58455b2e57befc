"""The CVRPTW kernels (csrc/cvrptw.hip) on the device, through the C ABI: the recorded
episodes of the reference's CVRPTWEnv, and reset / mask / step / co_cvrptw_steps against the
restatement tests/cvrptw_ref.py bit for bit on every output, over the sizes at which the
kernel takes another path -- N + 1 below, at and above a lane group's two columns per lane
(N = 63, 64, 70), more columns per lane (N = 200), a single customer, and batches of 1, 3, 16
and 257 rows (a partial group, a partial wave, more than one workgroup) -- with i32, f32 and
i64 windows, the hand-made rows, and the kernel edges.  N + 1 on both sides of every switch
of tw_launch (N = 15, 16, 31, 32, 62 with 63 and 64 above, 127, 128, 255, 256, 511, 512; B =
3), directed rollouts at N = 128, 256, 300, 512, 1023 (B = 4) in which every register slot is
the action's at least once and column N is visited, and co_cvrptw_check on 300 rows (a second
block with a partial tail), step-major and row-major actions, every status bit alone in row
280 and the depot-return bound read from batch row 0.  Only the archive is read, never a
reference checkout."""
import pytest
import torch

import cvrptw_cases as cc
from test_host_cvrptw import run_decode_loops

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("policy", cc.POLICIES)
@pytest.mark.parametrize("case", cc.recorded_cases())
def test_device_matches_the_recording(case, policy):
    cc.check_recorded_case(case, policy, DEV)


@pytest.mark.parametrize("n,b", cc.SHAPES)
def test_device_matches_the_restatement(n, b):
    dtype = cc.TW_DTYPES[(cc.SHAPES.index((n, b))) % 3]
    cc.check_shape(n, b, dtype, DEV)


@pytest.mark.parametrize("n,b", cc.LARGE_SHAPES)
def test_rows_of_many_columns_per_lane(n, b):
    """N = 300 and the largest N the entries take, 1023 (CO_CVRPTW_MAX_N)."""
    cc.check_shape(n, b, torch.int32, DEV)


@pytest.mark.parametrize("n", cc.SWITCH_SIZES)
def test_both_sides_of_every_launch_switch(n):
    """N + 1 below and at 16, 32, 64 (lanes per row) and 128, 256, 512 (columns per lane)."""
    cc.check_shape(n, 3, cc.TW_DTYPES[cc.SWITCH_SIZES.index(n) % 3], DEV)


@pytest.mark.parametrize("n,b", cc.DIRECTED_SHAPES)
def test_every_register_slot_is_the_action(n, b):
    """The directed rollout: every register slot a row's lanes hold is the action's at
    least once and column N is visited -- asserted from the restatement before any kernel
    is compared -- through single steps and co_cvrptw_steps in both action layouts."""
    cc.check_directed_inputs(n, b)
    cc.check_shape(n, b, torch.int32, DEV, directed=True)


@pytest.mark.parametrize("dtype", cc.TW_DTYPES)
def test_window_dtypes(dtype):
    cc.check_shape(70, 3, dtype, DEV)
    cc.check_hand_made(DEV, dtype)


def test_hand_made_rows_and_nan():
    cc.check_hand_made(DEV)
    cc.check_nan_time(DEV)


def test_kernel_edges():
    cc.check_edges(DEV)


def test_check_bits_on_the_device():
    n, b = 20, 16
    inst = cc.instance(n, b)
    states, actions = cc.rollout(n, b)
    locs = torch.from_numpy(states[0]["locs"]).to(DEV)
    acts = torch.from_numpy(actions).to(DEV).t()
    dur = torch.from_numpy(inst["durations"]).to(DEV)
    tw = torch.from_numpy(inst["time_windows"]).to(DEV)
    assert cc.abi_check(locs, acts, dur, tw) == 0
    for edit, want in ((lambda t: t[3, 4, 0].fill_(-1), 64), (lambda t: t[0, 0, 1].fill_(100), 128),
                       (lambda t: t[2, 7, 1].copy_(t[2, 7, 0]), 512)):
        t2 = tw.clone()
        edit(t2)
        got = cc.abi_check(locs, acts, dur, t2)
        assert got == cc.ref.check(states[0]["locs"], actions.T, inst["durations"],
                                   t2.cpu().numpy()) and got & want
    a2 = acts.clone()
    a2[1, 0] = n + 1
    assert cc.abi_check(locs, a2, dur, tw) == 8
    assert cc.abi_check(locs, acts, dur.long(), tw.long()) == 0


def test_check_bits_over_two_blocks_on_the_device():
    cc.check_check_bits_two_blocks(DEV)


def test_decode_loops_on_the_device():
    run_decode_loops(DEV)
