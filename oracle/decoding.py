"""Restatement of the per-step decode math of ``rl4co/utils/decoding.py``
(test infrastructure only)."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from .ops import batchify, gather_by_index


def top_k_filter(logits, top_k):  # decoding.py:112-117
    remove = logits < torch.topk(logits, top_k)[0][..., -1, None]
    return logits.masked_fill(remove, float("-inf"))


def top_p_filter(logits, top_p):  # decoding.py:120-138
    if top_p <= 0.0 or top_p >= 1.0:
        return logits
    sorted_logits, sorted_indices = torch.sort(logits, descending=False, stable=True)
    cumulative_probs = sorted_logits.softmax(dim=-1).cumsum(dim=-1)
    sorted_remove = cumulative_probs <= (1 - top_p)
    remove = sorted_remove.scatter(-1, sorted_indices, sorted_remove)
    return logits.masked_fill(remove, float("-inf"))


def tanh_cr(x):
    """tanh rounded once from f64: what the device decode step evaluates (torch.tanh on
    CPU is MKL VML's, within one ulp of it; see rl4co_slap_amd/csrc/co_math.hpp)."""
    return torch.tanh(x.double()).float()


def process_logits(logits, mask=None, temperature=1.0, tanh_clipping=0.0, mask_logits=True,
                   top_k=0, top_p=0.0, tanh=torch.tanh):
    """``decoding.py:141-191`` (ties of the top-p sort in index order: stable sort).
    ``tanh`` defaults to the reference's ``torch.tanh``; tests pass ``tanh_cr`` to separate
    the tanh implementation from the rest of the math."""
    if tanh_clipping > 0:
        logits = tanh(logits) * tanh_clipping
    if mask_logits:
        assert mask is not None, "mask must be provided if mask_logits is True"
        # the reference writes -inf into the tensor it was given (with tanh_clipping == 0
        # that is the caller's logits, decoding.py:178); the product does not,
        # so the restatement works on a copy and returns the same log-probabilities
        logits = logits.clone()
        logits[~mask] = float("-inf")
    logits = logits / temperature
    if top_k > 0:
        logits = top_k_filter(logits, min(top_k, logits.size(-1)))
    if top_p > 0:
        assert top_p <= 1.0, "top-p should be in (0, 1]."
        logits = top_p_filter(logits, top_p)
    return F.log_softmax(logits, dim=-1)


def greedy(logprobs, mask=None):  # decoding.py:371-381
    sel = logprobs.argmax(dim=-1)
    if mask is not None:
        assert not (~mask).gather(1, sel.unsqueeze(-1)).data.any(), "infeasible action selected"
    return sel


def sampling(logprobs, mask=None, generator=None):  # decoding.py:383-397
    probs = logprobs.exp()
    sel = torch.multinomial(probs, 1, generator=generator).squeeze(1)
    if mask is not None:
        while (~mask).gather(1, sel.unsqueeze(-1)).data.any():
            sel = probs.multinomial(1, generator=generator).squeeze(1)
    return sel


def decode_draw_u(batch, seed, offset, row0=0):
    """The decode step's uniform draw of rows ``row0 .. row0 + batch - 1`` (include/co_env.h,
    csrc/decode_common.hpp: not torch's generator): ``u = (w >> 8) * 2^-24`` with ``w`` word
    0 of Philox-4x32-10 under key ``(seed_lo, seed_hi)`` at counter ``(offset_lo, offset_hi,
    row_lo, row_hi)``.  float64 (every value is on the f32 grid)."""
    import numpy as np

    from .generate import MASK, philox4x32_10

    rows = [(row0 + i) & 0xFFFFFFFFFFFFFFFF for i in range(batch)]
    ctr = np.empty((batch, 4), dtype=np.uint64)
    ctr[:, 0] = offset & MASK
    ctr[:, 1] = (offset >> 32) & MASK
    ctr[:, 2] = [r & MASK for r in rows]
    ctr[:, 3] = [r >> 32 for r in rows]
    key = np.array([[seed & MASK, (seed >> 32) & MASK]], dtype=np.uint64)
    w = philox4x32_10(ctr, key)[:, 0]
    return torch.from_numpy((w >> np.uint64(8)).astype(np.float64) * 2.0 ** -24)


def sample_inverse_cdf(logp, u):
    """The sampled action as a function of the draw, in float64: with ``p = exp(logp)`` and
    ``cdf = p.cumsum(-1) / p.sum(-1)``, the first index with ``p > 0`` and ``cdf > u``; the
    last index with ``p > 0`` when there is none.  Returns ``(action[B], margin[B])``,
    ``margin = min_c |cdf[c] - u|``: an f32 evaluation whose running sums are within
    ``margin`` of these picks the same action."""
    p = logp.double().exp()
    cdf = p.cumsum(-1)
    cdf = cdf / cdf[..., -1:]
    u = u.double().reshape(-1, 1)
    n = p.shape[-1]
    idx = torch.arange(n).expand_as(p)
    pos = p > 0
    hit = torch.where(pos & (cdf > u), idx, torch.full_like(idx, n)).min(-1).values
    last = torch.where(pos, idx, torch.full_like(idx, -1)).max(-1).values
    action = torch.where(hit < n, hit, last.clamp(min=0))
    margin = (cdf - u).abs().min(-1).values
    return action, margin


def sample_margin_tol(n):
    """How far an f32 inverse CDF of a row of ``n`` may be from ``sample_inverse_cdf``'s,
    in units of the total: the rounding of the longest chain of f32 additions into any
    running sum (short rows, ``n <= 2048``: the max(8, n/64) elements of a lane, then the
    6 steps of the scan; long rows: the n/256 block carries, the 6 scan steps and the 3
    wave totals), one ulp of ``expf`` per term, the rounding of the total and that of
    ``u * total`` -- each at most 2^-24 of a sum that is at most the total -- times a
    slack factor 4."""
    import math

    if n > 2048:
        return 4 * (math.ceil(n / 256) + 12) * 2.0 ** -24
    return 4 * (max(8, math.ceil(n / 64)) + 9) * 2.0 ** -24


def beam_rank(logp, parent, beam_width):
    """``decoding.py:611-641`` for one step, ties by candidate index: ``logp`` ``[BW*B, N]``
    and ``parent`` ``[BW*B]`` in the ``s*B + b`` row layout; instance ``b``'s candidate
    ``t = s*N + c`` scores ``logp[s*B + b, c] + parent[s*B + b]`` (f32 add); the ``BW`` best
    by a stable descending sort (equal scores: the lower ``t``; NaN ranks greatest, as in
    ``torch.topk``).  Returns ``(selected, beam_parent, beam_row, score)``, each ``[BW*B]``
    with rank ``j`` of instance ``b`` at row ``j*B + b``."""
    e, n = logp.shape
    b = e // beam_width
    score = logp.float() + parent.float().reshape(e, 1)
    hst = torch.cat(score.split(b), dim=1)  # [B, BW*N], column s*N + c
    vals, order = torch.sort(hst, dim=1, descending=True, stable=True)
    topv, topi = vals[:, :beam_width], order[:, :beam_width]
    flat = lambda t: torch.hstack(torch.unbind(t, 1))  # noqa: E731  ([B, BW] -> j*B + b)
    topv, topi = flat(topv), flat(topi)
    selected = topi % n
    beam_parent = (topi // n).int()
    beam_row = torch.arange(b).repeat(beam_width) + beam_parent.long() * b
    return selected, beam_parent, beam_row, topv


def get_log_likelihood(logprobs, actions=None, mask=None, return_sum=True):  # decoding.py:39-65
    if actions is not None and logprobs.dim() == 3:
        logprobs = logprobs.gather(-1, actions.unsqueeze(-1)).squeeze(-1)
    if mask is not None:
        logprobs[~mask] = 0
    assert (logprobs > -1000).data.all(), "Logprobs should not be -inf, check sampling procedure!"
    return logprobs.sum(1) if return_sum else logprobs


class Decoding:
    """``DecodingStrategy`` (``decoding.py:194-369``) for greedy / sampling /
    evaluate, with multistart (``pre_decoder_hook`` ``:265-313``)."""

    def __init__(self, kind="greedy", temperature=1.0, tanh_clipping=0.0, mask_logits=True,
                 multistart=False, num_starts=None, store_all_logp=False, tanh=torch.tanh):
        self.tanh = tanh  # tests only: odec.tanh_cr to match the device tanh
        self.kind = kind.replace("multistart_", "")
        self.multistart = multistart or kind.startswith("multistart")
        self.temperature, self.tanh_clipping, self.mask_logits = temperature, tanh_clipping, mask_logits
        self.num_starts, self.store_all_logp = num_starts, store_all_logp
        self.actions, self.logprobs = [], []

    def pre_decoder_hook(self, td, env, action=None):
        from .td import batchify_td
        if self.multistart:
            if self.num_starts is None:
                self.num_starts = env.get_num_starts(td)
        else:
            self.num_starts = 0
        if self.num_starts >= 1 and self.multistart:
            if action is None:
                action = env.select_start_nodes(td, num_starts=self.num_starts)
            td = batchify_td(td, self.num_starts)
            td["action"] = action
            td = env.step(td)["next"]
            lp = torch.zeros_like(td["action_mask"]) if self.store_all_logp else torch.zeros_like(action)
            self.logprobs.append(lp)
            self.actions.append(action)
        return td, env, self.num_starts

    def step(self, logits, mask, td, action=None):  # decoding.py:327-369
        m = mask if self.mask_logits else None
        logp = process_logits(logits, m, self.temperature, self.tanh_clipping, self.mask_logits,
                              tanh=self.tanh)
        if self.kind == "greedy":
            sel = greedy(logp, m)
        elif self.kind == "sampling":
            sel = sampling(logp, m)
        elif self.kind == "evaluate":
            sel = action
        else:
            raise ValueError(self.kind)
        if not self.store_all_logp:
            logp = gather_by_index(logp, sel, dim=1)
        td["action"] = sel
        self.actions.append(sel)
        self.logprobs.append(logp)
        return td

    def post_decoder_hook(self, td, env):  # decoding.py:315-325 (select_best off)
        assert len(self.logprobs) > 0
        return torch.stack(self.logprobs, 1), torch.stack(self.actions, 1), td, env


class BeamSearchOracle:
    """``decoding.py:500-641`` (``BeamSearch``) restated with plain torch ops on the
    oracle's TD: start nodes, then per step the top ``beam_width`` of the (beam, node)
    candidates per instance, state rows re-indexed by the beam parents, backtracking
    and best-beam selection by reward."""

    def __init__(self, beam_width=None, select_best=True, temperature=1.0, tanh_clipping=0.0,
                 mask_logits=True, **unused):
        self.beam_width, self.select_best = beam_width, select_best
        self.temperature, self.tanh_clipping, self.mask_logits = temperature, tanh_clipping, mask_logits
        self.actions, self.logprobs, self.beam_path = [], [], []
        self.parent_beam_logprobs = None

    @staticmethod
    def _rows(td, idx):
        from .td import TD
        return TD({k: v[idx] for k, v in td.items()}, [idx.shape[0]])

    def pre_decoder_hook(self, td, env):  # decoding.py:526-556
        from .td import batchify_td
        if self.beam_width is None:
            self.beam_width = env.get_num_starts(td)
        action = env.select_start_nodes(td, num_starts=self.beam_width)
        td = batchify_td(td, self.beam_width)
        td["action"] = action
        td = env.step(td)["next"]
        logprobs = torch.zeros(td["action_mask"].shape)
        self.logprobs.append(logprobs)
        self.actions.append(action)
        self.parent_beam_logprobs = logprobs.gather(1, action[..., None])
        self.beam_path.append(torch.zeros(logprobs.size(0), dtype=torch.int32))
        return td, env, self.beam_width

    def step(self, logits, mask, td, action=None):  # decoding.py:327-369, 512-524, 611-641
        m = mask if self.mask_logits else None
        logp = process_logits(logits, m, self.temperature, self.tanh_clipping, self.mask_logits)
        e, n = logp.shape
        b = e // self.beam_width
        hst = torch.cat((logp + self.parent_beam_logprobs).split(b), dim=1)
        topv, _ = torch.topk(hst, self.beam_width, dim=1)
        # torch.topk leaves the order of equal scores unspecified, and f32 sums of many
        # log-probabilities do collide (BW = 120 beams of TSP-140: several exact ties per
        # step): the candidates are ranked by beam_rank's stable sort (equal scores -> the
        # lower s*N + c, include/co_env.h); the ranked values must be topk's
        selected, parent, idx, sel_lp = beam_rank(logp, self.parent_beam_logprobs, self.beam_width)
        assert torch.equal(sel_lp.view(torch.int32),
                           torch.hstack(torch.unbind(topv, 1)).view(torch.int32))
        self.parent_beam_logprobs = sel_lp.unsqueeze(1)
        self.beam_path.append(parent)
        td = self._rows(td, idx)
        logp = logp[idx]
        if m is not None:
            assert not (~m[idx]).gather(1, selected.unsqueeze(-1)).any(), "infeasible action selected"
        td["action"] = selected
        self.actions.append(selected)
        self.logprobs.append(logp)
        return td

    def post_decoder_hook(self, td, env):  # decoding.py:558-609
        actions = torch.stack(self.actions, 1)
        logprobs = torch.stack(self.logprobs, 1)
        cur = self.beam_path[-1]
        seqs, lps = [actions[:, -1]], [logprobs[:, -1]]
        b = actions.size(0) // self.beam_width
        seq = torch.arange(0, b).repeat(self.beam_width)
        for k in reversed(range(len(self.beam_path) - 1)):
            idx = seq + cur * b
            seqs.append(actions[idx, k])
            lps.append(logprobs[idx, k])
            cur = self.beam_path[k][idx]
        actions = torch.stack(list(reversed(seqs)), dim=1)
        logprobs = torch.stack(list(reversed(lps)), dim=1)
        if not self.select_best:
            return logprobs, actions, td, env
        rewards = env.get_reward(td, actions)
        _, idx = torch.cat(rewards.unsqueeze(1).split(b), 1).max(1)
        flat = torch.arange(b) + idx * b
        return logprobs[flat], actions[flat], self._rows(td, flat), env


__all__ = ["process_logits", "greedy", "sampling", "get_log_likelihood", "Decoding",
           "BeamSearchOracle", "batchify", "decode_draw_u", "sample_inverse_cdf",
           "sample_margin_tol", "beam_rank"]
