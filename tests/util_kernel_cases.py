"""Shared by tests/test_gpu_util_kernels.py (the device library) and
tests/test_host_util_kernels.py (the host build, which exports co_gather_by_index and
co_any_eq_i64): the case tables, the plain references and the assertions for the utility
kernels of csrc/ops.hip -- gather, the three single-workgroup reductions, the POMO shared
baseline, the two augmentations and the distance matrix.  Not a test module.

Every reference is torch or numpy on the CPU (f64 where a sum is involved); every function
takes the device to run on, a CPU device meaning the host build.

Direct C-ABI calls write into a ``Carved`` output: a slice of a larger buffer filled with
0xAB whose bytes before and after the slice must come back untouched.  Inputs are views
into parents filled with a value that changes the result when a neighbour is read: NaN
for floats, 0xAB bytes for integers (an out-of-range index), True for bool -- and, for the
two kernels that search or count, the very value they look for (``reduction_input``).
"""
import collections
import functools
import math

import numpy as np
import torch

from oracle import transforms as otr
from oracle.ops import gather_by_index as oracle_gather
from rl4co_slap_amd import _native as nat

SENT = 0xAB
PAD = 64    # sentinel bytes on either side of a carved output (keeps 16-byte alignment)
LEAD = 16   # sentinel elements in front of an input view (16 * itemsize: 16-byte aligned)
EPS = 2.0 ** -24  # unit roundoff of f32


def _itemsize(dtype):
    return torch.empty((), dtype=dtype).element_size()


def _bytes(t):
    return t.contiguous().view(-1).view(torch.uint8)


def sync(device):
    if device.type == "cuda":
        torch.cuda.synchronize(device)


class Carved:
    """An output of ``shape`` / ``dtype`` at byte offset ``PAD + off`` of a 0xAB-filled
    buffer (``off``: the extra misalignment a case asks for)."""

    def __init__(self, shape, dtype, device, off=0, preset=None):
        self.off = PAD + off
        self.nbytes = math.prod(shape) * _itemsize(dtype)
        self.buf = torch.full((self.off + self.nbytes + PAD,), SENT, dtype=torch.uint8,
                              device=device)
        assert self.buf.data_ptr() % 16 == 0
        self.t = self.buf[self.off:self.off + self.nbytes].view(dtype).reshape(shape)
        if preset is not None:
            self.t.fill_(preset)
        self.ptr = self.buf.data_ptr() + self.off

    def cpu(self):
        return self.t.cpu()

    def check_guards(self):
        b = self.buf.cpu()
        assert (b[:self.off] == SENT).all(), "bytes before the output were written"
        assert (b[self.off + self.nbytes:] == SENT).all(), "bytes after the output were written"

    def check_untouched(self):
        assert (self.buf.cpu() == SENT).all(), "an output that was not passed was written"


def sentinel(n, dtype):
    """``n`` elements of the input sentinel (a tensor that owns its storage)."""
    if dtype.is_floating_point:
        return torch.full((n,), float("nan"), dtype=dtype)
    if dtype == torch.bool:
        return torch.ones(n, dtype=dtype)
    return torch.full((n * _itemsize(dtype),), SENT, dtype=torch.uint8).view(dtype).clone()


def on(device, view):
    """The CPU ``view`` (of a contiguous parent) rebuilt on ``device`` over a copy of the
    whole parent: same sizes, strides and storage offset, sentinels included."""
    base = view if view._base is None else view._base
    assert base.is_contiguous() and base.storage_offset() == 0
    b = base.clone() if device.type == "cpu" else base.to(device)
    assert b.data_ptr() % 16 == 0
    return torch.as_strided(b, view.shape, view.stride(), view.storage_offset())


def embed(x, off=3):
    """``x`` as a view at element offset ``LEAD + off`` of a sentinel-filled 1-D parent."""
    n = x.numel()
    parent = sentinel(LEAD + off + n + 8, x.dtype)
    view = parent[LEAD + off:LEAD + off + n].view(x.shape)
    view.copy_(x)
    return view


# ------------------------------------------------------------------------------ gather

GatherCase = collections.namedtuple("GatherCase", "name flat idx dst_off width")


def _values(n, dtype, seed):
    """Distinct values where the dtype can hold them (a wrong read then shows)."""
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.bool:
        return torch.rand(n, generator=g) > 0.5
    if dtype == torch.uint8:
        return torch.randint(1, 251, (n,), generator=g).to(torch.uint8)
    return (torch.randperm(n, generator=g) + 1).to(dtype)


def strided_src(dtype, outer, length, inner, s_outer, s_len, base_off, seed=0):
    """``flat [outer, length, inner]`` with element strides ``(s_outer, s_len, 1)`` at
    element offset ``LEAD + base_off`` of a sentinel-filled parent."""
    n = LEAD + base_off + (outer - 1) * s_outer + (length - 1) * s_len + inner + 8
    parent = sentinel(n, dtype)
    flat = torch.as_strided(parent, (outer, length, inner), (s_outer, s_len, 1),
                            LEAD + base_off)
    flat.copy_(_values(outer * length * inner, dtype, seed).view(outer, length, inner))
    return flat


def make_idx(outer, m, length, seed=0, layout="dense"):
    """int64 ``[outer, m]`` indices into ``0..length-1``; every row holds 0 and
    ``length - 1``.  ``transposed``: an ``[m, outer].t()`` view; ``shared``: one row with
    outer stride 0."""
    g = torch.Generator().manual_seed(1000 + seed)
    rows = 1 if layout == "shared" else outer
    idx = torch.randint(0, length, (rows, m), generator=g)
    idx[:, 0] = length - 1
    idx[:, m // 2] = 0
    parent = sentinel(LEAD + 3 + rows * m + 8, torch.int64)
    off = LEAD + 3
    if layout == "transposed":
        view = torch.as_strided(parent, (outer, m), (1, outer), off)
    elif layout == "shared":
        view = torch.as_strided(parent, (outer, m), (0, 1), off)
        parent[off:off + m] = idx[0]
        return view
    else:
        view = torch.as_strided(parent, (outer, m), (m, 1), off)
    view.copy_(idx)
    return view


def unit_width(src_ptr, dst_ptr, s_outer, s_len, inner_bytes):
    """The unit width co_gather_by_index's dispatch lands on (bytes)."""
    al = src_ptr | dst_ptr | s_outer | s_len | inner_bytes
    return 16 if al % 16 == 0 else 8 if al % 8 == 0 else 4 if al % 4 == 0 else 1


def _width_cases():
    f32, u8 = torch.float32, torch.uint8
    # name, dtype, inner, s_outer, s_len, base_off (elements), dst_off (bytes), width
    rows = [
        ("dense16", f32, 4, 96, 8, 0, 0, 16),          # the [8, 12, 8] parent, [:, :, 0:4]
        ("dense32", f32, 8, 96, 8, 0, 0, 16),          # two units per element
        ("base+8", f32, 4, 96, 8, 2, 0, 8),            # [:, :, 2:6]
        ("base+4", f32, 4, 96, 8, 1, 0, 4),            # [:, :, 1:5]
        ("s_len%16=8", f32, 4, 72, 6, 0, 0, 8),
        ("s_len%8=4", f32, 4, 60, 5, 0, 0, 4),
        ("s_outer%16=8", f32, 4, 98, 8, 0, 0, 8),      # a padded row stride
        ("s_outer%8=4", f32, 4, 97, 8, 0, 0, 4),
        ("inner_bytes=12", f32, 3, 48, 4, 0, 0, 4),
        ("inner_bytes=24", f32, 6, 96, 8, 0, 0, 8),
        ("inner_bytes=3", u8, 3, 192, 16, 0, 0, 1),
        ("bytes base+1", u8, 4, 192, 16, 1, 0, 1),
        ("dst+4", f32, 4, 96, 8, 0, 4, 4),             # direct calls only
        ("dst+8", f32, 4, 96, 8, 0, 8, 8),
    ]
    return [GatherCase(name, strided_src(dt, 8, 12, inner, so, sl, bo, seed=k),
                       make_idx(8, 5, 12, seed=k), doff, w)
            for k, (name, dt, inner, so, sl, bo, doff, w) in enumerate(rows)]


def _dtype_cases():
    out = []
    for k, dt in enumerate([torch.float16, torch.bfloat16, torch.float64, torch.int32,
                            torch.int64, torch.uint8, torch.bool]):
        for inner in (3, 4):
            name = f"{str(dt).split('.')[1]}x{inner}"
            out.append(GatherCase(name, strided_src(dt, 3, 7, inner, 7 * inner, inner, 0,
                                                    seed=50 + k),
                                  make_idx(3, 6, 7, seed=50 + k), 0, None))
    return out


def _layout_cases():
    f32 = torch.float32
    return [GatherCase("idx transposed", strided_src(f32, 6, 9, 4, 36, 4, 0, seed=70),
                       make_idx(6, 5, 9, seed=70, layout="transposed"), 0, 16),
            GatherCase("idx shared row", strided_src(f32, 6, 9, 4, 36, 4, 0, seed=71),
                       make_idx(6, 5, 9, seed=71, layout="shared"), 0, 16),
            GatherCase("idx transposed bytes", strided_src(torch.uint8, 5, 9, 3, 27, 3, 0, seed=72),
                       make_idx(5, 4, 9, seed=72, layout="transposed"), 0, 1)]


WIDTH_CASES = _width_cases()
DTYPE_CASES = _dtype_cases()
LAYOUT_CASES = _layout_cases()
GATHER_CASES = WIDTH_CASES + DTYPE_CASES + LAYOUT_CASES
OOR_CASES = [c for c in WIDTH_CASES if c.name in ("dense16", "base+8", "base+4", "inner_bytes=3")]
BAD_INDICES = [-1, None, 2 ** 40, -2 ** 63]  # None: src_len


def gather_ref(flat, idx):
    """CPU indexing: ``out[o, m] = flat[o, idx[o, m]]``, an out-of-range index giving a
    zero element; and whether any index was out of range."""
    o, length = flat.shape[:2]
    ok = (idx >= 0) & (idx < length)
    j = torch.where(ok, idx, torch.zeros_like(idx))
    out = flat[torch.arange(o)[:, None], j].clone()
    out[~ok] = 0
    return out, bool((~ok).any())


def gather_direct(src, idx, dst_off=0):
    """co_gather_by_index on ``src [outer, len, *trail]`` (any outer / len strides) and
    ``idx [outer, m]`` (any strides): the carved output, the status word, the unit width."""
    device = src.device
    es = src.element_size()
    outer, length = src.shape[:2]
    inner = math.prod(src.shape[2:])
    m = idx.shape[1]
    dst = Carved((outer, m, *src.shape[2:]), src.dtype, device, off=dst_off)
    status = torch.zeros(1, dtype=torch.int32, device=device)
    args = (src.data_ptr(), outer, length, inner * es, src.stride(0) * es, src.stride(1) * es,
            idx.data_ptr(), m, idx.stride(0), idx.stride(1), dst.ptr)
    nat.call("co_gather_by_index", *args, status.data_ptr(), nat.stream_of(src))
    sync(device)
    return dst, int(status.item()), unit_width(args[0], dst.ptr, args[4], args[5], args[3])


def check_gather(case, device, wrapper=None):
    """The direct call (exact, status 0, guards, the case's unit width) and, given the
    ``gather_by_index`` wrapper, the same views through it against the oracle."""
    src, idx = on(device, case.flat), on(device, case.idx)
    want, bad = gather_ref(case.flat, case.idx)
    assert not bad
    dst, status, width = gather_direct(src, idx, case.dst_off)
    if case.width is not None:
        assert width == case.width, f"{case.name}: lands on width {width}"
    assert status == 0
    assert torch.equal(_bytes(dst.cpu()), _bytes(want)), case.name
    dst.check_guards()
    if wrapper is not None and case.dst_off == 0:
        ref = oracle_gather(case.flat, case.idx, squeeze=False)
        got = wrapper(src, idx, squeeze=False)
        assert got.shape == ref.shape and got.dtype == ref.dtype
        assert torch.equal(_bytes(got.cpu()), _bytes(ref)), case.name


def check_gather_out_of_range(case, device):
    """One bad index in the last unit of the last row: the flag, a zero element there,
    every other element exact."""
    src = on(device, case.flat)
    length = case.flat.shape[1]
    for bad in BAD_INDICES:
        idx_cpu = case.idx.clone()
        idx_cpu[-1, -1] = length if bad is None else bad
        want, flagged = gather_ref(case.flat, idx_cpu)
        assert flagged
        dst, status, width = gather_direct(src, idx_cpu.to(device), case.dst_off)
        assert width == case.width
        assert status == nat.ST_INDEX_RANGE, (case.name, bad, status)
        got = dst.cpu()
        assert (_bytes(got[-1, -1]) == 0).all(), (case.name, bad)
        assert torch.equal(_bytes(got), _bytes(want)), (case.name, bad)
        dst.check_guards()


@functools.lru_cache(maxsize=1)
def gather_second_trip_case():
    """uint8 ``src [64, 40, 129]`` by ``idx [64, 130]``: 1,073,280 byte units, past the
    4,096 x 256 threads of the grid; the last unit holds a value found nowhere else."""
    flat = strided_src(torch.uint8, 64, 40, 129, 40 * 129, 129, 0, seed=90)
    idx = torch.randint(0, 39, (64, 130), generator=torch.Generator().manual_seed(91))
    idx[:, 0] = 39
    idx[:, 65] = 0
    idx[-1, 0] = 38   # the last row reads element 39 for its last column only
    idx[-1, -1] = 39
    flat[-1, 39, 128] = 255  # _values stays below 251
    return GatherCase("second grid trip", flat, embed(idx), 0, 1)


def check_gather_second_trip(device):
    case = gather_second_trip_case()
    check_gather(case, device)
    want, _ = gather_ref(case.flat, case.idx)
    assert int(want.reshape(-1)[-1]) == 255 and int((want == 255).sum()) == 1


DIM0_SHAPES = [(9,), (9, 5), (70, 3)]


def check_gather_dim0(wrapper, device, shape):
    """``dim=0`` as the beam search and data.py gather: ``v[:, None]`` by ``idx [K]`` for a
    vector, ``[E, T]`` by ``idx [K]`` otherwise."""
    e = shape[0]
    src = embed(_values(math.prod(shape), torch.float32, 3).view(shape))
    idx = embed(torch.tensor([e - 1, 0, e // 2, e // 2, 1]))
    sd, idd = on(device, src), on(device, idx)
    if len(shape) == 1:
        got = wrapper(sd[:, None], idd, dim=0).squeeze(-1)
        want = oracle_gather(src[:, None], idx, dim=0).squeeze(-1)
    else:
        got = wrapper(sd, idd, dim=0, squeeze=False)
        want = oracle_gather(src, idx, dim=0, squeeze=False)
    assert got.shape == want.shape and torch.equal(got.cpu(), want)


EMPTY_GATHERS = [((0, 10, 2), (0, 10), 1), ((0, 10), (0, 3), 1), ((4, 0, 2), (4, 0), 1),
                 ((4, 6, 2), (4, 0), 1), ((5, 3), (0,), 0)]


def check_gather_empty(wrapper, device, src_shape, idx_shape, dim):
    src = torch.rand(src_shape)
    idx = torch.zeros(idx_shape, dtype=torch.int64)
    for squeeze in (True, False):
        ref = oracle_gather(src, idx, dim=dim, squeeze=squeeze)
        got = wrapper(src.to(device), idx.to(device), dim=dim, squeeze=squeeze)
        assert got.shape == ref.shape and got.dtype == ref.dtype and got.device.type == device.type
        assert got.numel() == 0


# ---------------------------------------------------------------------- co_any_eq_i64

ANY_EQ_N = [0, 1, 1023, 1024, 1025, 5000]
ANY_EQ_VALUES = [0, -1, 2 ** 40]


def reduction_input(body, outside):
    """``body`` (1-D) inside a parent filled with ``outside`` -- the value whose presence
    changes the result of a search or a count over the wrong range."""
    parent = torch.full((LEAD + 3 + body.numel() + 8,), outside, dtype=body.dtype)
    view = parent[LEAD + 3:LEAD + 3 + body.numel()]
    view.copy_(body)
    return view


def check_any_eq(device, n, value):
    """Hit at the last index only, at index 1024 only, nowhere; the flag (pre-set to 77)
    comes back exactly 0 or 1.  The elements around x hold the searched value."""
    g = torch.Generator().manual_seed(n)
    hits = [None] + ([n - 1] if n > 0 else []) + ([1024] if n > 1024 else [])
    for hit in hits:
        x = torch.randint(1, 1000, (n,), generator=g) + (value if value > 0 else 0)
        assert not (x == value).any()
        if hit is not None:
            x[hit] = value
        xd = on(device, reduction_input(x, value))
        flag = Carved((1,), torch.int32, device, preset=77)
        nat.call("co_any_eq_i64", xd.data_ptr(), n, value, flag.ptr, nat.stream_of(flag.buf))
        sync(device)
        assert int(flag.cpu()) == int(hit is not None), (n, value, hit)
        flag.check_guards()


# ------------------------------------------------------------------ co_count_not_done

COUNT_N = [0, 1, 15, 16, 17, 1023, 1024, 16383, 16384, 16385, 49157]
COUNT_OFFSETS = [0, 1, 8]  # into a 16-byte aligned parent: the 16-byte path / the byte path


def check_count_not_done(device, off):
    """The count of zero bytes of ``done[off : off + n]`` over a pre-set 77, zeros placed
    first / last / everywhere / nowhere among bytes of {1, 2, 255}; the parent is zero
    outside the range, so a count over the wrong range shows."""
    g = torch.Generator().manual_seed(off)
    for n in COUNT_N:
        for where in ("first", "last", "everywhere", "nowhere"):
            body = torch.tensor([1, 2, 255], dtype=torch.uint8)[torch.randint(0, 3, (n,), generator=g)]
            if where == "everywhere":
                body.zero_()
            elif where == "first" and n:
                body[0] = 0
            elif where == "last" and n:
                body[-1] = 0
            parent = torch.zeros(LEAD + off + n + 64, dtype=torch.uint8)
            parent[LEAD + off:LEAD + off + n] = body
            pd = parent.to(device)
            assert pd.data_ptr() % 16 == 0
            count = Carved((1,), torch.int32, device, preset=77)
            nat.call("co_count_not_done", pd.data_ptr() + LEAD + off, n, count.ptr,
                     nat.stream_of(pd))
            sync(device)
            assert int(count.cpu()) == int((body == 0).sum()), (n, off, where)
            count.check_guards()


# ----------------------------------------------------------------- co_row_deficit_max

def _deficit_rows(n_rows, width, stride, target, seed):
    """0/1 bytes, every row's deficit (its zero count) at most min(3, width - 1), the
    ``target`` row's the full width; the padding columns hold 0xAB."""
    g = torch.Generator().manual_seed(seed)
    rows = torch.full((n_rows, stride), SENT, dtype=torch.uint8)
    body = torch.ones(n_rows, width, dtype=torch.uint8)
    for _ in range(min(3, width - 1)):
        body[torch.arange(n_rows), torch.randint(0, width, (n_rows,), generator=g)] = 0
    body[target] = 0
    rows[:, :width] = body
    want = int((width - body.sum(1, dtype=torch.int64)).max())
    assert want == width and int((width - body.sum(1, dtype=torch.int64) == width).sum()) == 1
    return rows, want


def _run_deficit(device, rows, n_rows, width, stride):
    view = on(device, embed(rows.reshape(-1), off=0))
    out = Carved((1,), torch.int32, device, preset=77)
    nat.call("co_row_deficit_max", view.data_ptr() if n_rows else None, n_rows, width, stride,
             out.ptr, nat.stream_of(out.buf))
    sync(device)
    out.check_guards()
    return int(out.cpu())


ROW_DEFICIT_CASES = [(16454, 17, 20, 16453), (16454, 17, 20, 16384),  # 2nd trip: rows >= 16,384
                     (70, 1, 4, 69), (70, 15, 18, 69), (70, 16, 19, 33), (70, 16, 16, 69)]


def check_row_deficit(device, n_rows, width, stride, target):
    rows, want = _deficit_rows(n_rows, width, stride, target, seed=n_rows + width + target)
    assert _run_deficit(device, rows, n_rows, width, stride) == want


def check_row_deficit_edges(device):
    full = torch.full((70, 20), 255, dtype=torch.uint8)  # sums far above the width
    assert _run_deficit(device, full, 70, 17, 20) == 0
    assert _run_deficit(device, full[:0], 0, 17, 20) == 0  # n_rows = 0 writes the 0 itself


# --------------------------------------------------------------- co_pomo_shared_baseline

POMO_SHAPES = [(1, 1), (3, 2), (5, 63), (4, 64), (7, 65), (6, 129), (9, 200), (32773, 2)]
# the special rows, assigned to instances B-1, B-2, ... while the shape has room: (name,
# smallest S it needs)
POMO_KINDS = [("tie_10_67", 68), ("tie_5_69", 70), ("all_equal", 1), ("last_only", 1),
              ("tie_first_last", 2), ("nan", 1), ("neg_inf", 1)]
PomoCase = collections.namedtuple("PomoCase", "B S reward ll kinds")


@functools.lru_cache(maxsize=None)
def pomo_case(B, S):
    """Rewards in [-25, -5] and log-likelihoods in [-40, 0] in the layout e = s*B + b."""
    g = torch.Generator().manual_seed(B * 1000 + S)
    r = -(torch.rand(S, B, generator=g) * 20 + 5)
    ll = -torch.rand(S, B, generator=g) * 40
    kinds, top = {}, -1.5
    for i, name in enumerate(k for k, need in POMO_KINDS if S >= need):
        b = B - 1 - i
        if b < 0:
            break
        kinds[name] = b
        if name == "tie_10_67":    # the later start sits in the lower lane (67 % 64 = 3)
            r[10, b] = r[67, b] = top
        elif name == "tie_5_69":   # both in lane 5
            r[5, b] = r[69, b] = top
        elif name == "all_equal":
            r[:, b] = r[0, b]
        elif name == "last_only":
            r[S - 1, b] = top
        elif name == "tie_first_last":
            r[0, b] = r[S - 1, b] = top
        elif name == "nan":
            for s in ((67, 10) if S >= 68 else (S - 1, S // 2)):
                r[s, b] = float("nan")
        elif name == "neg_inf":
            r[:, b] = float("-inf")
    return PomoCase(B, S, r.reshape(-1), ll.reshape(-1), kinds)


def _same_f32(got, want):
    """Bitwise equal, any NaN matching any NaN."""
    nan = torch.isnan(want)
    return torch.equal(torch.isnan(got), nan) and torch.equal(
        got[~nan].view(torch.int32), want[~nan].view(torch.int32))


def run_pomo(device, case, with_ll=True, with_lt=True, with_adv=True, with_max=True):
    """One launch; the outputs that are not passed stay behind as untouched buffers."""
    B, S = case.B, case.S
    rd, lld = on(device, embed(case.reward)), on(device, embed(case.ll))
    out = {"bl": Carved((B,), torch.float32, device), "max": Carved((B,), torch.float32, device),
           "best": Carved((B,), torch.int64, device),
           "adv": Carved((S * B,), torch.float32, device),
           "lt": Carved((B,), torch.float32, device)}
    p = {k: v.ptr for k, v in out.items()}
    nat.call("co_pomo_shared_baseline", B, S, rd.data_ptr(), lld.data_ptr() if with_ll else None,
             p["bl"], p["max"] if with_max else None, p["best"] if with_max else None,
             p["adv"] if with_adv else None, p["lt"] if with_lt else None, nat.stream_of(rd))
    sync(device)
    passed = {"bl": True, "max": with_max, "best": with_max, "adv": with_adv, "lt": with_lt}
    for k, v in out.items():
        v.check_guards() if passed[k] else v.check_untouched()
    return out, passed


def check_pomo(device, B, S):
    """Returns the largest observed ratio to each derived bound (bl, adv, loss_terms)."""
    case = pomo_case(B, S)
    out, _ = run_pomo(device, case)
    bl, mx, best, adv, lt = (out[k].cpu() for k in ("bl", "max", "best", "adv", "lt"))
    rw = case.reward.view(S, B).t()          # [B, S]
    llw = case.ll.view(S, B).t()
    advw = adv.view(S, B).t()
    # maximum and first argmax, as torch.max / torch.argmax on the CPU
    want_max, want_best = rw.max(1).values, rw.argmax(1)
    assert torch.equal(best, want_best), (best[-8:], want_best[-8:])
    assert _same_f32(mx, want_max)
    k = case.kinds
    for name, s in (("tie_10_67", 10), ("tie_5_69", 5), ("all_equal", 0), ("last_only", S - 1),
                    ("tie_first_last", 0), ("neg_inf", 0)):
        if name in k:
            assert int(best[k[name]]) == s, name
    if "nan" in k:
        assert int(best[k["nan"]]) == (10 if S >= 68 else S // 2) and math.isnan(mx[k["nan"]])
    if "neg_inf" in k:
        assert mx[k["neg_inf"]] == float("-inf")
    # adv is the f32 difference against the baseline that was written, in every row
    assert _same_f32(advw, rw - bl[:, None])
    fin = torch.isfinite(rw).all(1)
    assert _same_f32(bl[~fin], rw[~fin].mean(1))  # NaN / -inf, as torch on the CPU
    assert torch.isnan(lt[~fin]).all()
    # finite rows, against f64
    r64, bound_k = rw[fin].double(), math.ceil(S / 64) + 8
    mean64 = r64.mean(1)
    b_mean = bound_k * EPS * r64.abs().mean(1)
    e_bl = (bl[fin].double() - mean64).abs()
    e_adv = (advw[fin].double() - (r64 - mean64[:, None])).abs().max(1).values
    terms = advw[fin].double() * llw[fin].double()
    b_lt = bound_k * EPS * terms.abs().sum(1)
    e_lt = (lt[fin].double() - terms.sum(1)).abs()

    def ratio(err, bound):
        return float((err / bound.clamp(min=1e-300)).max()) if err.numel() else 0.0

    ratios = {"bl": ratio(e_bl, b_mean), "adv": ratio(e_adv, b_mean), "loss_terms": ratio(e_lt, b_lt)}
    print(f"pomo B={B} S={S}: largest error / bound {ratios}")
    assert (e_bl <= b_mean).all(), ratios
    assert (e_adv <= b_mean).all(), ratios
    assert (e_lt <= b_lt).all(), ratios
    return ratios


def check_pomo_optional(device, B, S):
    """NULL outputs: the buffers that were not passed stay untouched, the rest is the
    full call's, bit for bit."""
    case = pomo_case(B, S)
    full, _ = run_pomo(device, case)
    for kw in (dict(with_ll=False, with_lt=False), dict(with_adv=False), dict(with_max=False)):
        out, passed = run_pomo(device, case, **kw)
        for name, buf in out.items():
            if passed[name]:
                assert torch.equal(_bytes(buf.cpu()), _bytes(full[name].cpu())), (kw, name)


# --------------------------------------------------------------------- co_distance_matrix

DIST_N = [1, 2, 3, 4, 5, 8, 63, 64]
DIST_B = [1, 3]
DIST_KINDS = ["unit", "scaled", "coincident"]


def dist_locs(B, N, kind, seed=0):
    rng = np.random.default_rng(seed + 7 * N + B)
    locs = rng.random((B, N, 2), dtype=np.float32)
    if kind == "scaled":  # +-1000, negative values included
        locs = ((locs - np.float32(0.5)) * np.float32(2000)).astype(np.float32)
    elif kind == "coincident" and N > 1:
        locs[:, N // 2:] = locs[:, :N - N // 2]
    return locs


def dist_contract(locs):
    """include/co_env.h: f32 sqrt(dx*dx + dy*dy), every operation rounded on its own."""
    x, y = locs[..., 0], locs[..., 1]
    dx = (x[..., :, None] - x[..., None, :]).astype(np.float32)
    dy = (y[..., :, None] - y[..., None, :]).astype(np.float32)
    xx, yy = (dx * dx).astype(np.float32), (dy * dy).astype(np.float32)
    return np.sqrt((xx + yy).astype(np.float32)).astype(np.float32)


def ulp_distance(got, want):
    """Largest distance in units of the last place between non-negative f32 arrays."""
    a = np.ascontiguousarray(got, dtype=np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(want, dtype=np.float32).view(np.int32).astype(np.int64)
    return int(np.abs(a - b).max()) if a.size else 0


def run_distance(device, locs):
    B, N = locs.shape[:2]
    ld = on(device, embed(torch.from_numpy(locs), off=2))  # 8-byte aligned only
    out = Carved((B, N, N), torch.float32, device)
    nat.call("co_distance_matrix", B, N, ld.data_ptr(), out.ptr, nat.stream_of(ld))
    sync(device)
    return out


def check_distance(device, B, N, kind):
    """Returns the ulp distance to the contract (asserted 0)."""
    locs = dist_locs(B, N, kind)
    out = run_distance(device, locs)
    out.check_guards()
    got = out.cpu()
    want = dist_contract(locs)
    ulps = ulp_distance(got.numpy(), want)
    print(f"distance matrix B={B} N={N} {kind}: {ulps} ulp from the contract")
    assert ulps == 0
    assert np.array_equal(got.numpy().view(np.int32), want.view(np.int32))
    assert (got.diagonal(dim1=-2, dim2=-1) == 0).all()
    assert torch.equal(got, got.transpose(-1, -2))
    t = torch.from_numpy(locs)
    norm = (t[..., :, None, :] - t[..., None, :, :]).norm(p=2, dim=-1)
    assert torch.allclose(got, norm, rtol=2e-7, atol=1e-7)
    return ulps


DIST_LARGE = [(1060, 63), (4100, 64)]  # 4,207,140 scalar / 4,198,400 vector units > 4,194,304


def check_distance_second_trip(device, B, N):
    locs = dist_locs(B, N, "unit", seed=5)
    out = run_distance(device, locs)
    per = N * N if N % 4 else N * N // 4
    first2 = (16384 * 256) // per  # the instance the second grid trip begins in
    assert first2 < B - 1
    rows = sorted({0, 1, B // 3, B // 2, first2 - 1, first2, first2 + 1, B - 1})
    got = out.t[rows].cpu().numpy()
    want = dist_contract(locs[rows])
    assert np.array_equal(got[-1].view(np.int32), want[-1].view(np.int32)), "last instance"
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), rows
    b = out.buf
    assert (b[:out.off].cpu() == SENT).all() and (b[out.off + out.nbytes:].cpu() == SENT).all()


# ---------------------------------------------------------------------- augmentations

AUG_B, AUG_N = 2100, 1000  # 2,100,000 points > 8,192 x 256 = 2,097,152


@functools.lru_cache(maxsize=1)
def augment_case():
    g = torch.Generator().manual_seed(21)
    xy = torch.rand(AUG_B, AUG_N, 2, generator=g)
    phi = torch.rand(AUG_B, generator=g) * 4 * math.pi  # a distinct angle per row
    phi[:12] = 0.0
    phi[12] = 2 * math.pi  # the boundary of the reflection test
    phi[1000:1004] = 0.0
    phi[-1] = 5 * math.pi / 2  # the last row: a quarter turn and the axis swap
    assert phi.unique().numel() == AUG_B - 15 and int((phi > 2 * math.pi).sum()) > 500
    want = otr.symmetric_transform(xy[..., [0]], xy[..., [1]], phi[:, None, None])
    return xy, phi, want


def check_symmetric(device):
    xy, phi, want = augment_case()
    xd, pd = on(device, embed(xy, off=2)), on(device, embed(phi))
    out = Carved(tuple(xy.shape), torch.float32, device)
    nat.call("co_symmetric_augment", AUG_B, AUG_N, xd.data_ptr(), pd.data_ptr(), 0.5, out.ptr,
             nat.stream_of(xd))
    sync(device)
    out.check_guards()
    got = out.cpu()
    err = (got - want).abs()
    print(f"symmetric augment: largest error {float(err.max()):.3g}, last row "
          f"{float(err[-1].max()):.3g}")
    assert torch.allclose(got[-1], want[-1], rtol=0, atol=2e-6), "last row"
    assert torch.allclose(got, want, rtol=0, atol=2e-6)
    zero = phi == 0
    assert torch.equal(got[zero].view(torch.int32), xy[zero].view(torch.int32))


def check_dihedral(device):
    xy = augment_case()[0]
    xd = on(device, embed(xy, off=2))
    out = Carved((8 * AUG_B, AUG_N, 2), torch.float32, device)
    nat.call("co_dihedral8_augment", AUG_B, AUG_N, xd.data_ptr(), out.ptr, nat.stream_of(xd))
    sync(device)
    out.check_guards()
    want = otr.dihedral_8_augmentation(xy)
    assert torch.equal(out.cpu().view(torch.int32), want.view(torch.int32))
