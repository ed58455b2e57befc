"""The host build's sampling decode (csrc/host co_decode_step on CPU tensors) pinned to the
deterministic reference: the inverse CDF of exp(logp) under the Philox draw keyed by
(seed, offset, row) -- oracle.decoding.decode_draw_u / sample_inverse_cdf in float64.
Runs without a GPU, so it also validates the oracle and the 5 % cap on the rows left out
(tests/sampling_cases.py) that the device tests rely on."""
import pytest
import torch

import sampling_cases as sc
from rl4co_slap_amd.utils.decoding import decode_step

B = 512


@pytest.mark.parametrize("clip,temp", sc.CLIP_TEMP)
@pytest.mark.parametrize("n", [3, 17, 129, 1025, 2048, 5000])
def test_host_sampling_matches_inverse_cdf(n, clip, temp):
    ref = sc.reference(B, n, clip, temp)
    rows, skipped = sc.compared_rows(ref)
    st = torch.zeros(1, dtype=torch.int32)
    act, lp, full = decode_step(ref.logits, ref.mask, "sampling", temp, clip, return_full=True,
                                seed=sc.SEED, offset=sc.OFFSET, status=st)
    sc.assert_sampled(ref, rows, skipped, act, lp, full)
    assert int(st.item()) == 0


def test_host_sampling_row_draw_is_independent_of_the_batch():
    """Row b draws what row b draws in any other batch size (the draw is keyed by the
    global row, not by the batch)."""
    ref = sc.reference(B, 129)
    base, _, _ = decode_step(ref.logits, ref.mask, "sampling", seed=sc.SEED, offset=sc.OFFSET)
    head, _, _ = decode_step(ref.logits[:77], ref.mask[:77], "sampling", seed=sc.SEED,
                             offset=sc.OFFSET)
    assert torch.equal(head, base[:77])
