"""Shared by the sampling-decode tests (tests/test_gpu_sampling_exact.py, the host build's
tests/test_host_sampling.py, tests/test_gpu_host_vs_device.py): the inputs, the oracle's
reference -- sampling is a deterministic function of (log-probabilities, seed, offset, row),
include/co_env.h -- and the assertions.  Not a test module.

A row is compared when the oracle's draw lies further than ``sample_margin_tol(N)`` from
every step of the oracle's CDF (then no f32 summation order can pick another action);
the rows left out are counted, reported in every assertion message and capped at 5 % of
the batch from the oracle alone, before the library under test runs."""
import collections
import functools

import torch

from oracle import decoding as odec

SEED = 0x123456789ABCDEF0  # both halves of both words matter
OFFSET = 2 ** 33 + 5
CLIP_TEMP = [(0.0, 1.0), (10.0, 1.0), (10.0, 0.7), (0.0, 2.5)]
CAP = 0.05

Ref = collections.namedtuple("Ref", "logits mask want act margin")

# The share of rows the oracle leaves out is about 2 * tol(N) * (feasible columns): every
# step of the CDF shadows 2 * tol of the draw's range.  At N = 5000 (3,500 feasible
# columns, tol 7.6e-6) that is 5.3 % for the flat distributions (no clipping), right at the
# cap, so whether a batch of 512 meets the cap depends on the batch: over eight generator
# seeds the (clip 0, temperature 1) case left out 22 ... 32 rows (cap 25).  The cap is a
# condition on the inputs, so N = 5000 takes a seed whose batch meets it for all four
# (clip, temperature) pairs: 24, 7, 10 and 21 rows.  Every other N uses 1000 + N.
_GEN_SEED = {5000: 1000 + 5000 + 3 * 7919}


def inputs(b, n, masked=True, lead_masked=0.0):
    """The base case: logits ``randn * 3`` (``* 1.5`` for the long rows, N > 2048: at
    ``* 3`` the probability mass sits on so few columns that the oracle alone leaves out
    14.8 % of the rows at N = 2049), mask ``rand > 0.3`` with one feasible column forced
    per row; ``lead_masked``: that share of every row's leading columns masked."""
    g = torch.Generator().manual_seed(_GEN_SEED.get(n, 1000 + n))
    logits = torch.randn(b, n, generator=g) * (3.0 if n <= 2048 else 1.5)
    mask = torch.rand(b, n, generator=g) > 0.3
    lead = int(lead_masked * n)
    mask[:, :lead] = False
    mask[torch.arange(b), torch.randint(lead, n, (b,), generator=g)] = True
    return logits, (mask if masked else None)


def make_ref(logits, mask, clip=0.0, temp=1.0, top_k=0, top_p=0.0):
    want = odec.process_logits(logits.clone(), mask, temp, clip, mask_logits=mask is not None,
                               top_k=top_k, top_p=top_p, tanh=odec.tanh_cr)
    u = odec.decode_draw_u(logits.shape[0], SEED, OFFSET)
    act, margin = odec.sample_inverse_cdf(want, u)
    return Ref(logits, mask, want, act, margin)


@functools.lru_cache(maxsize=2)  # one reference for the cases that differ in layout only
def reference(b, n, clip=0.0, temp=1.0, masked=True, top_k=0, top_p=0.0, lead_masked=0.0):
    logits, mask = inputs(b, n, masked, lead_masked)
    return make_ref(logits, mask, clip, temp, top_k, top_p)


def compared_rows(ref, also=None):
    """-> (rows compared, number left out); asserts the cap (a condition on the inputs)."""
    b, n = ref.want.shape
    rows = ref.margin > odec.sample_margin_tol(n)
    if also is not None:
        rows = rows & also
    skipped = b - int(rows.sum())
    assert skipped <= CAP * b, (f"N={n}: the oracle leaves out {skipped} of {b} rows "
                                f"(cap {CAP * b:g})")
    return rows, skipped


def _bits(t):
    return t.contiguous().view(torch.int32)


def assert_sampled(ref, rows, skipped, act, lp, full, full_rows=None):
    """``full`` bit-equal to the oracle's log-probabilities (on ``full_rows``), ``lp`` the
    bits of ``full[b, act[b]]``, every action feasible, and on ``rows`` the oracle's."""
    act, lp, full = act.cpu(), lp.cpu(), full.cpu()
    b, n = ref.want.shape
    note = f"N={n} B={b}: {skipped} rows left out within the margin"
    fr = slice(None) if full_rows is None else full_rows
    assert torch.equal(_bits(full[fr]), _bits(ref.want[fr])), \
        f"{note}; full log-probabilities differ from the oracle's"
    assert ((act >= 0) & (act < n)).all(), note
    assert torch.equal(_bits(lp), _bits(full.gather(1, act[:, None]).squeeze(1))), \
        f"{note}; logp_sel is not full[b, action]"
    if ref.mask is not None:
        assert ref.mask.gather(1, act[:, None]).all(), f"{note}; a masked action was sampled"
    bad = (act != ref.act) & rows
    if bad.any():
        i = bad.nonzero().flatten()[:8]
        raise AssertionError(
            f"{note}; {int(bad.sum())} of {int(rows.sum())} compared rows differ: rows "
            f"{i.tolist()} got {act[i].tolist()} want {ref.act[i].tolist()} margins "
            f"{ref.margin[i].tolist()} (tol {odec.sample_margin_tol(n):.3g})")
