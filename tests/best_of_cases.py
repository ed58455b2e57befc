"""The case list and the C-ABI runners that tests/test_host_best_of.py and
tests/test_gpu_best_of.py share (not a test module).

Sizes: N over {2, 3, 7, 63, 64, 65, 100, 128, 129, 1024} plus both sides of every cut
between two lane-group instantiations of the device kernel (20 | 32 | 64 | 112 | 128 | 256 |
512), K over {1, 2, 7, 8, 63, 64,
65, 257, 800} (fewer candidates than lane groups of a block, more than one round),
B over {1, 3, 64, 257}; K*B*N <= ~2.5e5 per case.
"""
import numpy as np
import torch

import best_of_ref as ref
from rl4co_slap_amd import _native as nat

# (B, K, N)
CASES = [(1, 800, 100), (257, 2, 7), (3, 65, 1024), (64, 8, 100),
         (3, 1, 2), (64, 7, 3), (1, 63, 63), (3, 64, 64), (3, 257, 65), (64, 8, 128),
         (3, 63, 129), (257, 7, 64), (1, 257, 128), (64, 2, 63), (1, 1, 1024), (3, 800, 7),
         # both sides of every cut between two instantiations of the device kernel
         (3, 7, 20), (3, 7, 21), (3, 8, 32), (3, 8, 33), (3, 8, 112), (3, 8, 113),
         (3, 7, 256), (3, 7, 257), (3, 7, 512), (3, 7, 513)]
LAYOUTS = ["rows", "padded", "stepmajor"]
MODES = ["random", "first", "last", "dup"]
# the few cases the sanitizer driver and the quick variants use
SMALL = [(3, 1, 2), (64, 7, 3), (257, 2, 7), (3, 64, 64), (1, 63, 63)]

GUARD = 64
FILL = 0xA5


def case_id(c):
    return "B%d-K%d-N%d" % c


def circle_locs(B, N, rng):
    """Points in angular order on a circle (radius per instance): the identity tour is
    the convex hull, strictly shorter than any tour in another cyclic order."""
    ang = np.sort(rng.random((B, N)), axis=1) * 2 * np.pi
    rad = 0.2 + 0.3 * rng.random((B, 1))
    return np.stack([0.5 + rad * np.cos(ang), 0.5 + rad * np.sin(ang)], -1).astype(np.float32)


def make_tsp_case(B, K, N, mode, seed=0):
    """locs f32 [B, N, 2] and actions int64 [K*B, N] (row k*B + b).  mode: "random"
    (uniform instances, random tours), "first" / "last" (the hull tour at k = 0 / K - 1,
    random tours elsewhere), "dup" (the hull tour at two k: the lower must win)."""
    rng = np.random.default_rng([seed, B, K, N, MODES.index(mode)])
    acts = rng.random((K * B, N)).argsort(1).astype(np.int64)
    if mode == "random":
        return rng.random((B, N, 2), dtype=np.float32), acts, None
    locs = circle_locs(B, N, rng)
    a3 = acts.reshape(K, B, N)
    hull = np.arange(N, dtype=np.int64)
    if mode == "first":
        win = np.zeros(B, dtype=np.int64)
    elif mode == "last":
        win = np.full(B, K - 1, dtype=np.int64)
    else:
        win = rng.integers(0, max(K - 1, 1), size=B)
    for b in range(B):
        a3[win[b], b] = np.roll(hull, b % N)
        if mode == "dup" and K > 1:
            a3[rng.integers(win[b] + 1, K), b] = np.roll(hull, b % N)
    return locs, acts, win


def lay_out(acts, layout, device="cpu"):
    """The action matrix [E, T] as a strided torch view over its own storage."""
    t = torch.as_tensor(np.ascontiguousarray(acts))
    e, n = t.shape
    if layout == "rows":
        v = t.clone().to(device)
    elif layout == "padded":
        store = torch.full((e, n + 3), -7, dtype=torch.int64)
        store[:, :n] = t
        v = store.to(device)[:, :n]
        assert v.stride() == (n + 3, 1)
    else:
        v = t.t().contiguous().to(device).as_strided((e, n), (1, e))
    return v


class Guarded:
    """Output tensors inside one byte buffer with GUARD bytes of FILL around each."""

    def __init__(self, device, **specs):
        self.regions, off = {}, GUARD
        for name, (shape, dtype) in specs.items():
            nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
            self.regions[name] = (off, nbytes, shape, dtype)
            off += (nbytes + 63) // 64 * 64 + GUARD
        self.buf = torch.full((off,), FILL, dtype=torch.uint8, device=device)

    def __getitem__(self, name):
        off, nbytes, shape, dtype = self.regions[name]
        return self.buf[off:off + nbytes].view(dtype).view(shape)

    def intact(self):
        b = self.buf.cpu().numpy().copy()
        for off, nbytes, _, _ in self.regions.values():
            b[off:off + nbytes] = FILL
        return bool((b == FILL).all())


def _stream(t):
    s = nat.stream_of(t)
    return s


def run_tsp_best_of(locs, acts_view, K, check=0, device="cpu", want_all=True, want_rows=True):
    """co_tsp_best_of through the C ABI into guarded buffers.  Returns numpy
    (all_reward, best_reward, best_idx, best_actions, status, guards_intact)."""
    l = torch.as_tensor(np.ascontiguousarray(locs)).to(device)
    B, N = l.shape[0], l.shape[1]
    g = Guarded(device, all=((K * B,), torch.float32), best=((B,), torch.float32),
                idx=((B,), torch.int64), rows=((B, N), torch.int64), st=((1,), torch.int32))
    g["st"].zero_()
    nat.call("co_tsp_best_of", B, N, K, nat.ptr(l), nat.ptr(acts_view), acts_view.stride(0),
             acts_view.stride(1), int(check), nat.ptr(g["all"]) if want_all else None,
             nat.ptr(g["best"]), nat.ptr(g["idx"]), nat.ptr(g["rows"]) if want_rows else None,
             nat.ptr(g["st"]), _stream(l))
    if l.device.type == "cuda":
        torch.cuda.synchronize(l.device)
    out = [g[k].cpu().numpy().copy() for k in ("all", "best", "idx", "rows")]
    return (*out, int(g["st"].item()), g.intact())


def run_tsp_reward(locs, acts_view, device="cpu"):
    """co_tsp_reward on the same rows with locs_batch = B: f32 [K*B]."""
    l = torch.as_tensor(np.ascontiguousarray(locs)).to(device)
    B, N = l.shape[0], l.shape[1]
    e = acts_view.shape[0]
    out = torch.empty(e, dtype=torch.float32, device=l.device)
    st = torch.zeros(1, dtype=torch.int32, device=l.device)
    nat.call("co_tsp_reward", e, N, N, nat.ptr(l), B, nat.ptr(acts_view), acts_view.stride(0),
             acts_view.stride(1), 0, nat.ptr(out), nat.ptr(st), _stream(l))
    assert int(st.item()) == 0
    return out.cpu().numpy()


def run_best_of(reward, acts_view, B, K, device="cpu"):
    """co_best_of through the C ABI into guarded buffers: numpy (best_reward, best_idx,
    best_actions or None, guards_intact)."""
    r = torch.as_tensor(np.ascontiguousarray(reward, dtype=np.float32)).to(device)
    T = 0 if acts_view is None else acts_view.shape[1]
    g = Guarded(device, best=((B,), torch.float32), idx=((B,), torch.int64),
                rows=((B, max(T, 1)), torch.int64))
    sb, st = (0, 0) if acts_view is None else acts_view.stride()
    nat.call("co_best_of", B, K, T, nat.ptr(r), nat.ptr(acts_view), sb, st, nat.ptr(g["best"]),
             nat.ptr(g["idx"]), nat.ptr(g["rows"]) if T else None, None, _stream(r))
    if r.device.type == "cuda":
        torch.cuda.synchronize(r.device)
    rows = g["rows"].cpu().numpy().copy() if T else None
    if not T:  # nothing may have been written to the unused region
        assert (g["rows"].cpu().numpy().view(np.uint8) == FILL).all()
    return g["best"].cpu().numpy().copy(), g["idx"].cpu().numpy().copy(), rows, g.intact()


REWARD_KINDS = ["normal", "ties", "zeros", "nan1", "nan2", "inf"]


def make_rewards(B, K, kind, seed=0):
    """Arbitrary f32 rewards [K*B] for co_best_of."""
    rng = np.random.default_rng([seed, B, K, REWARD_KINDS.index(kind)])
    r = rng.standard_normal((K, B)).astype(np.float32)
    if kind == "ties":
        r = rng.integers(-2, 3, size=(K, B)).astype(np.float32)
    elif kind == "zeros":  # +0 / -0 (and a few negatives): signed zeros tie, lowest k wins
        r = np.where(rng.random((K, B)) < 0.5, np.float32(0.0), np.float32(-0.0))
        r = np.where(rng.random((K, B)) < 0.3, np.float32(-1.0), r).astype(np.float32)
    elif kind in ("nan1", "nan2") and K > 1:
        for b in range(B):
            ks = rng.choice(np.arange(1, K), size=min(K - 1, 1 if kind == "nan1" else 2),
                            replace=False)
            r[ks, b] = np.nan
    elif kind == "inf":
        r[rng.random((K, B)) < 0.2] = -np.inf
        r[rng.random((K, B)) < 0.1] = np.inf
    return r.reshape(-1)


def bits_equal(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32),
                          np.asarray(b, np.float32).view(np.uint32))


def check_tsp_case(B, K, N, layout, mode, device="cpu", host_result=None):
    """Run one case and assert everything the kernel tests assert; returns the outputs."""
    locs, acts, win = make_tsp_case(B, K, N, mode)
    view = lay_out(acts, layout, device)
    allr, best, idx, rows, status, intact = run_tsp_best_of(locs, view, K, check=1,
                                                            device=device)
    assert intact, "guard bytes overwritten"
    assert status == 0
    # selection exact on the kernel's own rewards
    want_r, want_i, want_rows = ref.best_of(allr, acts, B, K)
    assert np.array_equal(idx, want_i)
    assert np.array_equal(rows, want_rows)
    assert bits_equal(best, allr[idx * B + np.arange(B)])
    assert bits_equal(best, want_r)
    # per-candidate values: within 1 f32 ulp of co_tsp_reward and of the restatement
    ulp = ref.ulp_distance(allr, run_tsp_reward(locs, view, device))
    print(f"{case_id((B, K, N))} {layout} {mode}: max ulp vs co_tsp_reward {ulp.max()}")
    assert ulp.max() <= 1
    assert ref.ulp_distance(allr, ref.tsp_rewards(locs, acts)).max() <= 1
    if win is not None and N >= 63:  # the planted hull tour wins, at its lowest k
        assert np.array_equal(idx, win)
    # nullable outputs: the same selection without all_reward / best_actions
    _, best2, idx2, rows2, _, intact2 = run_tsp_best_of(locs, view, K, check=0, device=device,
                                                        want_all=False, want_rows=False)
    assert intact2 and np.array_equal(idx2, idx) and bits_equal(best2, best)
    assert (rows2.view(np.uint8) == FILL).all()
    return allr, best, idx, rows
