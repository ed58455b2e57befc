"""A numpy restatement of co_best_of and co_tsp_best_of, written from the text of
include/co_env.h (not a test module).

Candidate k of instance b is row e = k*B + b.  Selection: the k whose reward is largest;
equal values (+0 / -0 included) keep the lowest k; a NaN beats every number and the first
NaN wins (torch.max(dim)).  A TSP candidate's reward is the negated f32 rounding of a
float64 sum of the f32 edge lengths sqrt(dx*dx + dy*dy) of the closed tour.
"""
import numpy as np


def select(reward, B, K):
    """best_idx [B] (int64) of f32 reward [K*B] by the header's rule."""
    r = np.asarray(reward, dtype=np.float32).reshape(K, B)
    idx = np.zeros(B, dtype=np.int64)
    for b in range(B):
        col = r[:, b]
        nan = np.flatnonzero(np.isnan(col))
        if nan.size:
            idx[b] = nan[0]
            continue
        best = 0
        for k in range(1, K):
            if col[k] > col[best]:  # equal (and +0 == -0) keeps the lower k
                best = k
        idx[b] = best
    return idx


def best_of(reward, actions, B, K):
    """(best_reward [B], best_idx [B], best_actions [B, T] or None)."""
    reward = np.asarray(reward, dtype=np.float32)
    idx = select(reward, B, K)
    rows = idx * B + np.arange(B)
    return reward[rows], idx, None if actions is None else np.asarray(actions)[rows]


def tsp_rewards(locs, actions):
    """f32 [K*B]: row e scored on instance e % B of locs [B, N, 2]."""
    locs = np.asarray(locs, dtype=np.float32)
    actions = np.asarray(actions)
    B = locs.shape[0]
    inst = np.arange(actions.shape[0]) % B
    p = locs[inst[:, None], actions]                    # [E, N, 2]
    q = np.roll(p, -1, axis=1)
    d = (q - p).astype(np.float32)
    sq = (d[..., 0] * d[..., 0]).astype(np.float32) + (d[..., 1] * d[..., 1]).astype(np.float32)
    edge = np.sqrt(sq.astype(np.float32)).astype(np.float32)
    total = edge.astype(np.float64).sum(axis=1)
    return (-(total.astype(np.float32))).astype(np.float32)


def tsp_best_of(locs, actions, K):
    """(all_reward [K*B], best_reward, best_idx, best_actions) of co_tsp_best_of."""
    B = np.asarray(locs).shape[0]
    r = tsp_rewards(locs, actions)
    return (r,) + best_of(r, actions, B, K)


def ulp_distance(a, b):
    """|a - b| in units of f32 steps (order-preserving integer keys; NaN-free inputs)."""
    def key(x):
        i = np.asarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))
