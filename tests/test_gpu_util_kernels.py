"""The utility kernels of csrc/ops.hip at their dispatch, tie and grid-stride edges, each
against a plain CPU reference (tests/util_kernel_cases.py): the gather kernel's four unit
widths for every reason the dispatch lands on them, the POMO baseline's first-argmax rule
across lanes, every grid-stride loop entered a second time, the single-workgroup
reductions around their 16-byte path and 1,024-thread stride, and the distance matrix bit
for bit against the formula include/co_env.h states.  Direct C-ABI calls write into
sentinel-guarded outputs and read from views inside sentinel-filled parents."""
import pytest
import torch

import rl4co_slap_amd as ra
import util_kernel_cases as uc
from rl4co_slap_amd import _native as nat
from rl4co_slap_amd.utils.ops import gather_by_index

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------ gather

@pytest.mark.parametrize("case", uc.GATHER_CASES, ids=[c.name for c in uc.GATHER_CASES])
def test_gather_views(dev, case):
    uc.check_gather(case, dev, wrapper=gather_by_index)
    ra.check_errors()  # the wrapper's deferred word stayed clear


@pytest.mark.parametrize("case", uc.OOR_CASES, ids=[c.name for c in uc.OOR_CASES])
def test_gather_out_of_range(dev, case):
    uc.check_gather_out_of_range(case, dev)


def test_gather_second_grid_trip(dev):
    uc.check_gather_second_trip(dev)


@pytest.mark.parametrize("shape", uc.DIM0_SHAPES)
def test_gather_dim0(dev, shape):
    uc.check_gather_dim0(gather_by_index, dev, shape)
    ra.check_errors()


@pytest.mark.parametrize("src_shape,idx_shape,dim", uc.EMPTY_GATHERS)
def test_gather_empty_shapes(dev, src_shape, idx_shape, dim):
    uc.check_gather_empty(gather_by_index, dev, src_shape, idx_shape, dim)
    ra.check_errors()


def test_gather_empty_source_is_an_index_error(dev):
    """No element to index: every index is out of range, reported as any bad index is --
    through the deferred word, read by check_errors()."""
    out = gather_by_index(torch.rand(0, 3).to(dev), torch.tensor([0, 0], device=dev), dim=0)
    assert out.shape == (2, 3)
    with pytest.raises(RuntimeError, match="index out of range"):
        ra.check_errors()
    ra.check_errors()  # reported once
    assert (out.cpu() == 0).all()  # the zero-filled elements of a bad index


# -------------------------------------------------------------------------- reductions

@pytest.mark.parametrize("value", uc.ANY_EQ_VALUES)
@pytest.mark.parametrize("n", uc.ANY_EQ_N)
def test_any_eq(dev, n, value):
    uc.check_any_eq(dev, n, value)


@pytest.mark.parametrize("off", uc.COUNT_OFFSETS)
def test_count_not_done(dev, off):
    uc.check_count_not_done(dev, off)


@pytest.mark.parametrize("n_rows,width,stride,target", uc.ROW_DEFICIT_CASES)
def test_row_deficit_max(dev, n_rows, width, stride, target):
    uc.check_row_deficit(dev, n_rows, width, stride, target)


def test_row_deficit_max_edges(dev):
    uc.check_row_deficit_edges(dev)


# ----------------------------------------------------------------------- POMO baseline

@pytest.mark.parametrize("B,S", uc.POMO_SHAPES)
def test_pomo_shared_baseline(dev, B, S):
    """Maximum and first argmax as torch on the CPU (ties across and within lanes, NaN and
    -inf rows), adv the f32 difference to the written baseline bit for bit, and bl / adv /
    loss_terms within k * 2^-24 of f64, k = ceil(S / 64) + 8: at most ceil(S / 64) additions
    per lane, 6 in the wave reduction, one division (bl) or product (loss_terms) and the
    final rounding.  (32773, 2) takes the grid-stride loop a second time for its last five
    instances, the special rows."""
    uc.check_pomo(dev, B, S)


@pytest.mark.parametrize("B,S", [(9, 200), (3, 2)])
def test_pomo_optional_outputs(dev, B, S):
    uc.check_pomo_optional(dev, B, S)


def test_pomo_argument_checks(dev):
    case = uc.pomo_case(3, 2)
    rd, lld = case.reward.to(dev), case.ll.to(dev)
    outs = [uc.Carved((6,), torch.float32, dev) for _ in range(3)]
    bl, adv, lt = outs
    with pytest.raises(RuntimeError, match="co_pomo_shared_baseline"):  # loss_terms without ll
        nat.call("co_pomo_shared_baseline", 3, 2, rd.data_ptr(), None, bl.ptr, None, None,
                 adv.ptr, lt.ptr, nat.stream_of(rd))
    with pytest.raises(RuntimeError, match="co_pomo_shared_baseline"):  # S = 0
        nat.call("co_pomo_shared_baseline", 3, 0, rd.data_ptr(), lld.data_ptr(), bl.ptr, None,
                 None, adv.ptr, lt.ptr, nat.stream_of(rd))
    nat.call("co_pomo_shared_baseline", 0, 2, rd.data_ptr(), lld.data_ptr(), bl.ptr, None, None,
             adv.ptr, lt.ptr, nat.stream_of(rd))  # B = 0: CO_OK, nothing written
    torch.cuda.synchronize()
    for o in outs:
        o.check_untouched()


# ------------------------------------------------------- distance matrix, augmentations

@pytest.mark.parametrize("kind", uc.DIST_KINDS)
@pytest.mark.parametrize("N", uc.DIST_N)
@pytest.mark.parametrize("B", uc.DIST_B)
def test_distance_matrix_bitwise(dev, B, N, kind):
    uc.check_distance(dev, B, N, kind)


@pytest.mark.parametrize("B,N", uc.DIST_LARGE)
def test_distance_matrix_second_grid_trip(dev, B, N):
    uc.check_distance_second_trip(dev, B, N)


def test_symmetric_augment_second_grid_trip(dev):
    uc.check_symmetric(dev)


def test_dihedral8_augment_second_grid_trip(dev):
    uc.check_dihedral(dev)
