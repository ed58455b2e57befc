"""Shared by tests/test_gpu_episode_kernels.py (the one-launch episode kernels of
csrc/rollout.hip and csrc/nearest.hip on the device, through direct C-ABI calls and the
engine classes) and tests/test_host_episode_cases.py (the same cases through the host
build's stepwise entry points, and the case builders' own claims): inputs, expected outputs
and assertions.  Not a test module; nothing here touches a GPU.

References.  Actions and every state column come from the oracle's env-only rollout
(``oracle.rollout.rollout`` with TSPOracle / CVRPOracle / SLAPOracle and the three bench
policies) and are compared bit for bit; rewards are held to the oracle's within
``REWARD_TOL`` (1e-5 * max(|ref|, 1), the project's bound).  ``tour_f64`` / ``cvrp_f64`` /
``slap_f64`` restate the tour lengths in float64 from the f32 coordinates: the
high-precision reference of the measured reward error (``record``), set beside the bound
derived below.

Buffers.  Every output is an ``Out``: a view at byte offset PAD (+ the misalignment a
case asks for) of a 0xAB-filled parent, itself pre-filled with 0x33, so bytes written
outside the view and elements never stored both show.  Inputs are ``place``d inside
parents of NaN (floats) or 0xAB bytes (integers: a negative, out-of-range index).

Derived reward bounds (u = 2^-24, first order in u; what ``record`` prints beside the
measured error).  One edge: dx, dy are one f32 subtraction each (relative u), their squares
(1 + u)^2 (1 + u) -> 3u, the sum of the two non-negative squares keeps 3u and adds its own
rounding -> 4u, the square root halves that -> 2u and adds its rounding: u when correctly
rounded, 2u for the hardware v_sqrt_f32 (<= 1 ulp).  So an edge is within 3u (correctly
rounded) or 4u (hardware).  A sum of non-negative terms keeps the terms' relative bound;
   TSP teacher (rows and tile kernels): hardware sqrt, f64 accumulation (N * 2^-53,
     dropped), one final f32 rounding                                  -> 5u
   TSP nearest, CVRP episode: correctly rounded sqrt, f64 accumulation, one rounding
                                                                       -> 4u
   SLAP episode: hardware sqrt, the K edges of an order added in f32 in pick order
     (K - 1 additions), the O order lengths added in f32 in order (O - 1 additions), no
     further rounding                                                  -> (K + O + 2) u
all far inside the pass bar of 1e-5 = 168u.

Coverage: template instantiations named in the launch macros, and the case ids (of
tests/test_gpu_episode_kernels.py) that reach them, from reading the dispatch code of
co_internal_tsp_nearest_rollout, co_cvrp_rollout, launch_tsp_rows, launch_tsp_teacher and
co_slap_rollout.

  nearest.hip  tsp_nearest_lds_kernel<G, EPL>          test_tsp_nearest[N-kind]
    <4, 8>    N <= 32                                  32-*
    <4, 16>   33 .. 64                                 33-*, 64-*
    <4, 26>   65 .. 104                                65-*, 104-*
    <8, 14>   105 .. 112                               105-*, 112-*
    <8, 16>   113 .. 128                               113-*, 128-*
    <8, 32>   129 .. 256                               129-*, 256-*
    <16, 32>  257 .. 512                               257-*, 512-* (with -circle)
    <32, 32>  513 .. 1024                              513-*, 1024-* (with -circle)
    kinds: uniform, grid (exact ties), straddle (the certificate's edge), circle (N >= 257)
  nearest.hip  cvrp_nearest_lds_kernel<G, EPL>         test_cvrp_episode[N-demands]
    <4, 8>    N + 1 <= 32                              31-*
    <4, 16>   33 .. 64                                 32-*, 63-*
    <8, 14>   65 .. 112                                64-*, 111-*
    <8, 16>   113 .. 128                               112-*, 127-*
    <8, 32>   129 .. 256                               128-*, 255-*
    <16, 32>  257 .. 512                               256-*, 511-*, test_cvrp_truncated (300)
    <32, 32>  513 .. 1024                              512-*, 1023-*, test_cvrp_step_limit_15_bits
  nearest.hip  cvrp_pad_kernel (no template)           every CVRP case; lengths that differ
                                                       by >= 2 (asserted): test_cvrp_padding
  rollout.hip  tsp_teacher_rows_kernel<G, EPL, MODE, STATE>
    STATE = true: co_tsp_rollout_ex row-major, test_tsp_teacher_rows[N]; STATE = false:
    co_tsp_reward on the same buffers in the same test.  Per N the launches dma (MODE 3:
    contiguous, aligned), vec (MODE 1: an even row stride, N + 2 or N + 1, so an odd N
    splits the last 16-byte pair; the 7-step lanes of <16, 7> load scalars in it), scalar
    (MODE 0: the odd stride N + 1, or for odd N the base 8 bytes on), locs8 (coordinates
    8 mod 16: MODE 1 for even N, else 0) and, for N % 4 == 0, mask1 (MODE 3 with the mask
    1 byte on: byte-wise mask stores, which N % 4 != 0 takes in every launch).
    <4, 8, *>    N <= 32                               1, 2, 31, 32
    <8, 8, *>    33 .. 64                              33, 64
    <16, 7, *>   65 .. 112                             65, 97, 99, 112
    <16, 8, *>   113 .. 128                            113, 127, 128
    <32, 8, *>   129 .. 256                            129, 256
    <64, 8, *>   257 .. 512                            257, 511, 512
    <64, 16, *>  513 .. 1024                           513, 1023, 1024
  rollout.hip  tsp_teacher_kernel<NW, 4, STATE, 0>     test_tsp_teacher_tile[N]
    <1, 4, *>  N <= 64                                 64
    <2, 4, *>  65 .. 128                               65, 128
    <4, 4, *>  129 .. 256                              129, 192, 255, 256
    STATE = false is co_tsp_reward on step-major actions with B > 1 (same test).
    The dynamic-LDS attribute branch (tile + visited words > 64 KiB) is taken from
    N = 124 on: 128, 129, 192, 255, 256.
  rollout.hip  slap_group_kernel<G, 8, CLOSEST, SD>    test_slap_episode[L-...]
    <8, 8, true, true>     closest, L <= 64, L % 4 == 0, aligned     20/48/64-closest-*
    <8, 8, true, false>    closest, L <= 64, misaligned inputs       20/48/64-closest-*-locs8/depot8
    <8, 8, false, false>   teacher, L <= 64                          20/48/64-teacher-*
                           (its serial action loop, P * 8 > 1,024: 48/64-teacher-P130-*)
    <16, 8, true, true>    closest, 65 .. 128, L % 4 == 0            100/128-closest-*
    <16, 8, true, false>   closest, L = 65, or misaligned inputs     65-closest-*, 100/128-*-locs8
    <16, 8, false, false>  teacher, 65 .. 128                        65/100/128-teacher-*
    <32, 8, true, true>    closest, 129 .. 256, L % 4 == 0           180/256-closest-*
    <32, 8, true, false>   closest, L = 129, or misaligned inputs    129-closest-*, 180/256-*-locs8
    <32, 8, false, false>  teacher, 129 .. 256                       129/180/256-teacher-*
    <*, 8, false, true>    named by no launch macro branch: SD requires the closest policy
                           (`sd = closest && ...`), so no valid call reaches it.
"""
import collections
import functools
import math

import numpy as np
import torch

from oracle.envs import (CVRPOracle, SLAPOracle, TSPOracle, cvrp_nearest_action,
                         slap_closest_free_action, tsp_nearest_action)
from oracle.rollout import rollout as ref_rollout
from oracle.td import TD

SENT = 0xAB   # guard bytes around every output, and the integer inputs' parents
FILL = 0x33   # every output starts as this byte pattern
PAD = 64      # guard bytes on either side (keeps 16-byte alignment)
U = 2.0 ** -24  # unit roundoff of f32
REWARD_TOL = 1e-5

# the derived relative bounds of the module docstring
BOUND_TSP_TEACHER = 5 * U
BOUND_NEAREST = 4 * U


def bound_slap(o, k):
    return (k + o + 2) * U


# ------------------------------------------------------------------------- buffers
class Out:
    """An output of ``shape`` / ``dtype`` at byte offset ``PAD + off`` of a SENT-filled
    buffer, pre-filled with FILL bytes.  bool outputs are held as bytes."""

    def __init__(self, shape, dtype, device, off=0):
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        dtype = torch.uint8 if dtype == torch.bool else dtype
        self.start = PAD + off
        self.nbytes = math.prod(shape) * torch.empty((), dtype=dtype).element_size()
        self.buf = torch.full((self.start + self.nbytes + PAD,), SENT, dtype=torch.uint8,
                              device=device)
        assert self.buf.data_ptr() % 16 == 0
        inner = self.buf[self.start:self.start + self.nbytes]
        inner.fill_(FILL)
        self.t = inner.view(dtype).view(shape)
        self.ptr = self.buf.data_ptr() + self.start

    def check_guards(self, name=""):
        b = self.buf.cpu()
        assert bool((b[:self.start] == SENT).all()), f"{name}: bytes before the output were written"
        assert bool((b[self.start + self.nbytes:] == SENT).all()), \
            f"{name}: bytes after the output were written"

    def untouched(self):
        b = self.buf.cpu()
        return bool((b[self.start:self.start + self.nbytes] == FILL).all())


class Outs(dict):
    """Named ``Out`` buffers of one launch."""

    def __init__(self, device):
        super().__init__()
        self.device = device

    def new(self, name, shape, dtype, off=0):
        self[name] = Out(shape, dtype, self.device, off)
        return self[name].ptr

    def check_guards(self):
        for k, o in self.items():
            o.check_guards(k)

    def cpu(self):
        return {k: o.t.cpu() for k, o in self.items()}


def place(x, device, off=0, stride=None):
    """``x`` on ``device`` at byte offset ``PAD + off`` of a 16-byte aligned sentinel
    parent (NaN for floats, SENT bytes for integers); a 2-D ``x`` with ``stride`` gets that
    row stride (in elements), the gaps holding the sentinel."""
    x = x.contiguous()
    isz = x.element_size()
    n_el = x.numel() if stride is None else x.shape[0] * stride
    nbytes = n_el * isz
    total = PAD + off + nbytes + PAD
    if x.dtype.is_floating_point:
        assert off % 4 == 0 and isz == 4
        parent = torch.full(((total + 3) // 4,), float("nan"), dtype=torch.float32).view(torch.uint8)
    else:
        parent = torch.full((total,), SENT, dtype=torch.uint8)
    buf = parent.to(device) if torch.device(device).type != "cpu" else parent.clone()
    assert buf.data_ptr() % 16 == 0
    v = buf[PAD + off:PAD + off + nbytes].view(x.dtype)
    if stride is None:
        v = v.view(x.shape)
    else:
        assert x.dim() == 2 and stride >= x.shape[1]
        v = v.view(x.shape[0], stride)[:, :x.shape[1]]
    v.copy_(x)
    return v


# ---------------------------------------------------------------------- assertions
def _bits(t):
    return t.contiguous().view(torch.int32)


def assert_same(name, got, want):
    """``got`` (a CPU tensor; bool outputs come as bytes) equal to the oracle's ``want``
    bit for bit, in the oracle's shape."""
    got = got.reshape(want.shape)
    if want.dim() == 0:
        got, want = got[None], want[None]
    if want.dtype == torch.bool:
        want = want.to(torch.uint8)
    assert got.dtype == want.dtype, (name, got.dtype, want.dtype)
    g, w = (_bits(got), _bits(want)) if want.dtype == torch.float32 else (got, want)
    if not torch.equal(g, w):
        rows = (g != w).reshape(g.shape[0], -1).any(1).nonzero().flatten()
        raise AssertionError(f"{name}: {rows.numel()} rows differ from the oracle, first "
                             f"{rows[:8].tolist()}")


def assert_reward(got, ref, rows=None):
    got, ref = got.reshape(-1), ref.reshape(-1)
    if rows is not None:
        got, ref = got[rows], ref[rows]
    err = (got - ref).abs()
    ok = err <= REWARD_TOL * ref.abs().clamp(min=1)
    assert bool(ok.all()), (f"reward: {int((~ok).sum())} rows beyond {REWARD_TOL} relative, "
                            f"worst {float(err.max()):.3e}")


MEASURED = {}  # family -> (largest relative error seen in this process, its bound)


def record(family, got, ref64, bound):
    """Note (and print, for the record run) |got - f64 reference| / |f64 reference| of a
    kernel family; rows whose reference is 0 are held to an exact 0."""
    got, ref64 = got.reshape(-1).double(), ref64.reshape(-1)
    nz = ref64 != 0
    assert bool((got[~nz] == 0).all()), f"{family}: a zero-length tour has a non-zero reward"
    if not bool(nz.any()):
        return 0.0
    rel = float(((got[nz] - ref64[nz]).abs() / ref64[nz].abs()).max())
    old = MEASURED.get(family, (0.0, 0.0))
    MEASURED[family] = (max(old[0], rel), max(old[1], bound))
    print(f"EPISODE_REWARD_ERR family={family} rel={rel:.3e} ({rel / U:.2f} u) "
          f"bound={bound:.3e} ({bound / U:.0f} u)")
    return rel


def _closed_len(p):
    """Closed tour lengths of f64 points ``p [B, T, 2]``."""
    d = p - p.roll(-1, dims=1)
    return d.pow(2).sum(-1).sqrt().sum(-1)


def tour_f64(locs, acts):
    """-(closed length of locs[acts]) in float64 from the f32 coordinates."""
    p = locs.double().gather(1, acts[..., None].expand(-1, -1, 2))
    return -_closed_len(p)


def cvrp_f64(locs_full, acts):
    """-(length of depot -> locs_full[acts] -> depot), float64; locs_full [B, N + 1, 2]."""
    l64 = locs_full.double()
    p = torch.cat([l64[:, 0:1], l64.gather(1, acts[..., None].expand(-1, -1, 2))], 1)
    return -_closed_len(p)


def slap_f64(locs, assignment, picklist):
    """-(sum over the orders of the closed pick tour), float64; negative assignment and
    picklist entries wrap as python indices do."""
    b, l = locs.shape[:2]
    p = assignment.shape[1]
    pk = torch.where(picklist < 0, picklist + p, picklist)
    tot = torch.zeros(b, dtype=torch.float64)
    rows = torch.arange(b)[:, None]
    for o in range(pk.shape[1]):
        slot = assignment[rows, pk[:, o]].long()
        slot = torch.where(slot < 0, slot + l, slot)
        tot -= _closed_len(locs.double()[rows, slot])
    return tot


def batch_set(rows_per_wave, rows_per_workgroup):
    """B in {1, one wave's rows - 1, one workgroup's rows + 1} without repeats / zeros."""
    return sorted({b for b in (1, rows_per_wave - 1, rows_per_workgroup + 1) if b >= 1})


# ------------------------------------------------------------------------------ TSP
# rows per wave (= per one-wave workgroup) of the nearest episodes, read off the launch
# macros' lane-group widths: used only to size the batches
def nearest_rows_per_wave(nodes):
    return 16 if nodes <= 104 else (8 if nodes <= 256 else (4 if nodes <= 512 else 2))


def cvrp_rows_per_wave(nodes):
    return 16 if nodes <= 64 else (8 if nodes <= 256 else (4 if nodes <= 512 else 2))


TSP_NEAREST_N = [32, 33, 64, 65, 104, 105, 112, 113, 128, 129, 256, 257, 512, 513, 1024]
# The narrowest near-tie certificate among the instantiations N >= 257 reaches is a factor
# 1 + 2^-11 between the two smallest truncated squared distances (lds_nearest's kWin for
# 512 slots; 1 + 2^-10 for 1024).  Two squared distances within 1 + 2^-12 of each other
# are inside it whatever the truncation of the low key bits does (each truncation moves a
# value by less than 2^-14 relative), so such a step takes the exact redo.
NEAR_TIE_FACTOR = 1.0 + 2.0 ** -12


def tsp_kinds(n):
    return ["uniform", "grid", "straddle"] + (["circle"] if n >= 257 else [])


def _nudge(x, k):
    """f32 ``x`` (positive) moved by ``k`` ulps."""
    return (x.view(torch.int32) + k.to(torch.int32)).view(torch.float32)


@functools.lru_cache(maxsize=None)
def straddle_pair(centre=0.5):
    """Two points (near, far) whose f32 squared distances to (centre, centre) differ by a
    few ulps, lie on either side of a multiple of 2^10 ulps (so the kernels' truncated keys
    differ by exactly one step of the coarsest truncation, and of every finer one) and have
    the same correctly rounded f32 square root: the oracle's argmin over rounded distances
    takes the lower index, a scan of truncated squared distances the nearer point."""
    g = torch.Generator().manual_seed(0)
    k = torch.arange(-40, 41)
    for _ in range(4000):
        p = torch.rand(2, generator=g) * 0.5 + 0.25
        x = _nudge(p[0].expand(81).contiguous(), k)[:, None].expand(81, 81)
        y = _nudge(p[1].expand(81).contiguous(), k)[None, :].expand(81, 81)
        dx, dy = x - centre, y - centre
        s = (dx * dx + dy * dy).reshape(-1)
        if float(s.min()) < 1e-3:
            continue
        bits = s.view(torch.int32)
        root = s.double().sqrt().float()
        lo = bits & 1023
        for i in (lo >= 1021).nonzero().flatten().tolist():
            hit = ((lo <= 2) & ((bits >> 10) == (bits[i] >> 10) + 1) & (root == root[i])).nonzero()
            if hit.numel():
                j = int(hit[0])
                pts = torch.stack([x.reshape(-1), y.reshape(-1)], -1)
                return pts[i].clone(), pts[j].clone()
    raise AssertionError("no straddling pair found")


def straddle_nodes(i, n):
    """(far, near) node indices of instance ``i``: the farther point first; the nearer five
    nodes on, or a multiple of 32 nodes on (one lane of every lane-group width)."""
    far = 3
    if i % 2 == 0:
        return far, far + 5
    return far, (far + 32 * ((n - 1 - far) // 32)) if n - 1 - far >= 32 else n - 1


def tsp_locs(kind, b, n, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "straddle":  # every other node far away: the pair decides step 1
        near, far = straddle_pair()
        locs = torch.rand(b, n, 2, generator=g) * 0.01 + 5.0
        locs[:, 0] = 0.5
        for i in range(b):
            fi, ni = straddle_nodes(i, n)
            locs[i, fi], locs[i, ni] = far, near
        return locs
    if kind == "uniform":
        return torch.rand(b, n, 2, generator=g)
    if kind == "grid":  # a 4 x 4 integer grid scaled by 1/4: duplicates and exact ties
        return torch.randint(0, 4, (b, n, 2), generator=g).float() / 4
    assert kind == "circle"
    # node 0 at the centre; the others in pairs on a circle around it, one pair per angle,
    # the members of a pair and of the circle a few ulps off their place, node order
    # random.  From the centre every node is near-tied; having visited both members of a
    # pair, the two members of the next pair are near-tied.
    m = (n - 1 + 1) // 2
    ang = (torch.arange(m, dtype=torch.float64)[None] / m
           + torch.rand(b, 1, generator=g, dtype=torch.float64)) * (2 * math.pi)
    ring = torch.stack([0.5 + 0.4 * ang.cos(), 0.5 + 0.4 * ang.sin()], -1).float()
    ring = ring.repeat_interleave(2, dim=1)[:, :n - 1].contiguous()
    ring = _nudge(ring, torch.randint(-4, 5, ring.shape, generator=g))
    locs = torch.empty(b, n, 2)
    locs[:, 0] = 0.5
    for i in range(b):
        locs[i, 1:] = ring[i, torch.randperm(n - 1, generator=g)]
    return locs


TSPRef = collections.namedtuple("TSPRef", "locs acts reward tdf")


def _tsp_rollout(locs, acts=None):
    b, n = locs.shape[:2]
    env = TSPOracle(num_loc=n, seed=0)
    td = env.reset(TD({"locs": locs.clone()}, [b]))
    if acts is None:
        r, tdf, a = ref_rollout(env, td, tsp_nearest_action)
    else:
        it = iter(range(n))
        r, tdf, a = ref_rollout(env, td, lambda t: acts[:, next(it)])
    if n == 1:
        # the reference's gather_by_index squeezes a single step away and get_tour_length
        # then rolls over the batch: no per-instance value.  A one-node tour has length 0.
        r = torch.zeros(b)
    return TSPRef(locs, a, r, tdf)


@functools.lru_cache(maxsize=None)
def tsp_nearest_ref(kind, n, b):
    """The oracle's nearest-policy episode of ``b`` instances (a smaller batch is its
    first rows: instances do not interact)."""
    return _tsp_rollout(tsp_locs(kind, b, n, 1000 * n + len(kind)))


def tsp_expected(ref, b=None):
    """name -> the oracle's column, for the first ``b`` rows."""
    b = ref.locs.shape[0] if b is None else b
    n = ref.locs.shape[1]
    t = ref.tdf
    return {"action_mask": t["action_mask"][:b], "first_node": t["first_node"][:b],
            "current_node": t["current_node"][:b], "i": t["i"][:b], "done": t["done"][:b],
            "step_reward": torch.zeros(b, dtype=torch.bool),
            "actions": ref.acts[:b].reshape(b, n)}


def near_tie_steps(locs, acts, factor=NEAR_TIE_FACTOR):
    """Per instance, the number of steps t >= 1 at which the two smallest f32 squared
    distances from the current node to the unvisited nodes are within ``factor``."""
    b, n = locs.shape[:2]
    left = torch.ones(b, n, dtype=torch.bool)
    rows = torch.arange(b)
    left[rows, acts[:, 0]] = False
    count = torch.zeros(b, dtype=torch.int64)
    for t in range(1, n - 1):  # at least two candidates
        cur = locs[rows, acts[:, t - 1]]
        d = locs - cur[:, None]
        s = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).masked_fill(~left, float("inf"))
        two = s.double().topk(2, dim=1, largest=False).values
        count += (two[:, 1] <= two[:, 0] * factor).long()
        left[rows, acts[:, t]] = False
    return count


# -- teacher
TSP_ROWS_N = [1, 2, 31, 32, 33, 64, 65, 97, 99, 112, 113, 127, 128, 129, 256, 257, 511, 512,
              513, 1023, 1024]
TSP_TILE_N = [64, 65, 128, 129, 192, 255, 256]
TSP_TILE_B = [1, 63, 65, 129]


def oor_values(n):
    """Out-of-range actions: one past the end, negative, and beyond 32 bits."""
    return [n, -1, 1 << 32]


def rows_batches(n):
    """The batch set of the row kernel: 64 / G rows per wave, four waves per workgroup (G
    lanes per instance, read off launch_tsp_rows's macro)."""
    g = 4 if n <= 32 else 8 if n <= 64 else 16 if n <= 128 else 32 if n <= 256 else 64
    return batch_set(64 // g, 4 * (64 // g))


@functools.lru_cache(maxsize=None)
def tsp_teacher_ref(n, b):
    g = torch.Generator().manual_seed(7 * n + 1)
    locs = torch.rand(b, n, 2, generator=g)
    acts = torch.rand(b, n, generator=g).argsort(1)
    return _tsp_rollout(locs, acts)


Dirty = collections.namedtuple("Dirty", "acts revisit oor clean missing")


def dirty_batch(acts, which=0):
    """``acts`` [B >= 3, N >= 2] with one row revisiting a node (the node it drops is
    ``missing``) and one row holding an out-of-range action (N, -1 or 1 << 32 by
    ``which``)."""
    b, n = acts.shape
    assert b >= 3 and n >= 2
    a = acts.clone()
    revisit, oor = b // 2, b - 1
    src, dst = n // 3, max(2 * n // 3, n // 3 + 1)
    missing = int(a[revisit, dst])
    a[revisit, dst] = a[revisit, src]
    a[oor, n // 2] = oor_values(n)[which % 3]
    clean = torch.ones(b, dtype=torch.bool)
    clean[revisit] = clean[oor] = False
    return Dirty(a, revisit, oor, clean, missing)


def revisit_expected(locs_row, acts_row):
    """The final state of a row with a revisit (the reference's _step semantics: the mask
    keeps the nodes absent from the actions)."""
    n = acts_row.numel()
    left = torch.ones(n, dtype=torch.bool)
    left[acts_row] = False
    return {"action_mask": left, "first_node": acts_row[0], "current_node": acts_row[-1],
            "i": torch.tensor([n]), "done": torch.tensor(False),
            "step_reward": torch.tensor(False)}


# ------------------------------------------------------------------------------ CVRP
CVRP_N = [31, 32, 63, 64, 111, 112, 127, 128, 255, 256, 511, 512, 1023]
CVRP_PAD_N = [31, 112, 256]  # "ragged" batches: cvrp_pad_kernel has rows to pad
CVRPRef = collections.namedtuple("CVRPRef", "gen vcap acts reward tdf lens exact_fills")


def cvrp_gen(kind, n, b, seed):
    env = CVRPOracle(num_loc=n, seed=seed)
    gen = env.generate([b])
    if kind in ("exactfill", "ragged"):  # demands k/8 against a capacity of 1.0: exact sums
        g = torch.Generator().manual_seed(seed)
        gen["demand"] = torch.randint(1, 5, (b, n), generator=g).float() / 8
    if kind == "ragged":  # every third instance serves all customers in one route
        gen["demand"][0::3] = 0.5 / n
    return gen


def _cvrp_rollout(gen, vcap=1.0):
    b, n = gen["locs"].shape[:2]
    env = CVRPOracle(num_loc=n, vehicle_capacity=vcap, seed=0)
    td = env.reset(TD({k: v.clone() for k, v in gen.items()}, [b]))
    lens = torch.zeros(b, dtype=torch.int32)
    fills = [0]

    def policy(td):
        alive = ~td["done"].view(-1)
        lens.add_(alive.int())
        a = cvrp_nearest_action(td)
        # the chosen customer fills the vehicle exactly: demand + used == capacity
        d = td["demand"].gather(1, (a - 1).clamp(min=0)[:, None])
        fills[0] += int((alive & (a != 0)
                         & ((d + td["used_capacity"]) == td["vehicle_capacity"]).view(-1)).sum())
        return a

    r, tdf, a = ref_rollout(env, td, policy)
    return CVRPRef(gen, vcap, a, r, tdf, lens, fills[0])


@functools.lru_cache(maxsize=None)
def cvrp_ref(kind, n, b):
    return _cvrp_rollout(cvrp_gen(kind, n, b, 50 * n + b + len(kind)))


def cvrp_expected(ref):
    t = ref.tdf
    b = ref.acts.shape[0]
    return {"actions": ref.acts, "locs": t["locs"], "current_node": t["current_node"].view(b, 1),
            "used_capacity": t["used_capacity"].view(b, 1),
            "vehicle_capacity": t["vehicle_capacity"].view(b, 1), "visited": t["visited"],
            "action_mask": t["action_mask"], "done": t["done"].view(b),
            "step_reward": torch.zeros(b, dtype=torch.bool), "lens": ref.lens}


# ------------------------------------------------------------------------------ SLAP
SLAP_GRIDS = {20: (4, 5), 48: (6, 8), 64: (8, 8), 65: (5, 13), 100: (10, 10), 128: (8, 16),
              129: (3, 43), 180: (12, 15), 256: (16, 16)}
SlapCfg = collections.namedtuple("SlapCfg", "l policy p k o dist ratio variant")


def slap_lanes(l):
    return 8 if l <= 64 else (16 if l <= 128 else 32)


def slap_batches(l):
    """1, 256/G - 1, 256/G + 1: the last is also 1 mod 64/G (a wave whose DMA covers one
    row), the first leaves every wave but one without rows."""
    ipb = 256 // slap_lanes(l)
    return [1, ipb - 1, ipb + 1]


def slap_configs(l):
    """The (policy, P, K, O, distances, ratio, variant) of one L: both policies; P = 1,
    L - 1 and P % 4 != 0; K = 1, 4, 5, 8, 9, 12; O = 1, 7, 8, 20 (O*K on both sides of
    the G*8 picklist entries held in registers; O = 24, K = 12 for the 32-lane groups,
    whose registers hold all of 20 * 12); ratio present and NULL; each misalignment on its
    own; negative (wrapping) teacher actions and picklist entries."""
    odd = 7 if l <= 48 else 19          # P % 4 != 0
    pm = 12 if l == 20 else 20          # P % 4 == 0: the 16-byte assignment stores
    big = (24, 12) if l > 128 else (20, 12)
    out = []
    for pol in ("closest", "teacher"):
        out += [
            SlapCfg(l, pol, l - 1, 5, 20, "ties", True, "aligned"),
            SlapCfg(l, pol, 1, 1, 1, "grid", False, "aligned"),
            SlapCfg(l, pol, odd, 9, 7, "ties", True, "aligned"),
            SlapCfg(l, pol, pm, big[1], big[0], "grid", False, "aligned"),
            SlapCfg(l, pol, odd, 8, 8, "grid", True, "aligned"),
            SlapCfg(l, pol, pm, 4, 1, "ties", True, "aligned"),
            SlapCfg(l, pol, pm, 6, 20, "grid", True, "locs8"),
            SlapCfg(l, pol, pm, 5, 8, "ties", True, "mask1"),
            SlapCfg(l, pol, pm, 7, 7, "grid", True, "assign4"),
            SlapCfg(l, pol, pm, 5, 20, "grid", True, "ratio4"),
        ]
    out.append(SlapCfg(l, "closest", pm, 5, 20, "ties", True, "depot8"))
    if l in (48, 64):  # more steps than locations, P * 8 rows > the wave's 1,024 staged
        # words: the teacher path that reads the actions serially (locations repeat)
        out.append(SlapCfg(l, "teacher", 130, 5, 8, "grid", True, "aligned"))
    out.append(SlapCfg(l, "teacher", pm, 9, 8, "grid", True, "negative"))
    return out


def slap_id(c):
    return f"{c.l}-{c.policy}-P{c.p}-K{c.k}-O{c.o}-{c.dist}-{'ratio' if c.ratio else 'noratio'}-{c.variant}"


SLAPRef = collections.namedtuple("SLAPRef", "gen acts reward tdf")


def slap_gen(cfg, b):
    aisles, nlocs = SLAP_GRIDS[cfg.l]
    seed = 31 * cfg.l + 7 * cfg.p + cfg.k + cfg.o
    env = SLAPOracle(n_products=cfg.p, n_aisles=aisles, n_locs=nlocs, max_orders=cfg.o,
                     max_products_in_order=cfg.k, seed=seed)
    np.random.seed(seed)
    gen = env.generate([b])
    g = torch.Generator().manual_seed(seed)
    if cfg.dist == "ties":  # exact ties, -0.0 / +0.0 and a few +inf (never picked first)
        dd = torch.randint(0, 6, gen["depot_loc_dist"].shape, generator=g).float() * 0.5
        sel = torch.rand(dd.shape, generator=g)
        dd[(dd == 0) & (sel < 0.5)] = -0.0
        dd[sel > 0.97] = float("inf")
        gen["depot_loc_dist"] = dd
    else:
        gen["depot_loc_dist"] = gen["depot_loc_dist"].clone()
    if cfg.variant == "negative":  # python's wrap: entry - P names the same product
        pk = gen["picklist"]
        neg = torch.rand(pk.shape, generator=g) < 0.3
        gen["picklist"] = torch.where(neg, pk - cfg.p, pk)
    return env, gen, g


@functools.lru_cache(maxsize=None)
def slap_ref(cfg):
    """The oracle's episode at the largest batch of ``slap_batches`` (smaller batches are
    its first rows)."""
    b = slap_batches(cfg.l)[-1]
    env, gen, g = slap_gen(cfg, b)
    td = env.reset(TD({k: v.clone() for k, v in gen.items()}, [b]))
    if cfg.policy == "teacher":
        if cfg.p < cfg.l:
            acts = torch.stack([torch.randperm(cfg.l - 1, generator=g)[:cfg.p] + 1
                                for _ in range(b)])
        else:
            acts = torch.randint(1, cfg.l, (b, cfg.p), generator=g)
        if cfg.variant == "negative":  # a - L in [-L, -1]: the same location, wrapped
            neg = torch.rand(acts.shape, generator=g) < 0.4
            acts = torch.where(neg, acts - cfg.l, acts)
        it = iter(range(cfg.p))
        r, tdf, a = ref_rollout(env, td, lambda t: acts[:, next(it)])
    else:
        r, tdf, a = ref_rollout(env, td, slap_closest_free_action)
    return SLAPRef(gen, a, r, tdf)


def slap_expected(ref, b, ratio=True):
    t = ref.tdf
    out = {"action_mask": t["action_mask"][:b], "assignment": t["assignment"][:b], "i": t["i"][:b],
           "done": t["done"][:b], "step_reward": torch.zeros(b, 1, dtype=torch.bool),
           "actions": ref.acts[:b]}
    if ratio:
        out["ratio"] = t["ratio"][:b]
    return out
