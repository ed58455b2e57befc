"""Tensor helpers of ``rl4co/utils/ops.py`` for the HIP path.

``gather_by_index`` and ``get_tour_length`` run the gfx950 kernels; the batch
reshapes (``batchify``/``unbatchify``) and the multistart index generation are
view / index ops with the reference semantics (layout index ``s*B + b``).
"""
from __future__ import annotations

from typing import Union

import torch
from torch import Tensor

from .. import _native as nat
from ..td import TensorDict

# CO_EAGER_BATCHIFY=1: batchify TensorDicts with the reference's eager copy (no lazy rows)
_EAGER_BATCHIFY = bool(__import__("os").environ.get("CO_EAGER_BATCHIFY"))


def _batchify_single(x, repeats: int):
    s = x.shape
    return x.expand(repeats, *s).contiguous().view(s[0] * repeats, *s[1:])


def _batchify_td_lazy(td, repeats: int):
    """The stand-in TensorDict: every entry becomes a ``RepeatedRows`` (no copy until it
    is read, see ``td.RepeatedRows``); same keys, shapes and values as the reference's
    ``expand(...).contiguous().view(...)``."""
    from ..td import RepeatedRows

    out = TensorDict({}, batch_size=[td.batch_size[0] * repeats, *td.batch_size[1:]])
    for k in list(td.keys()):
        v = td.get_raw(k)
        if isinstance(v, RepeatedRows):  # nested batchify: materialise the inner one
            v = v.materialize()
        dict.__setitem__(out, k, RepeatedRows(v, repeats))
    return out


def batchify(x: Union[Tensor, TensorDict], shape):
    """``ops.py:19-34``: ``b ... -> (r b) ...`` (repeat-major layout).  A tensor is
    copied as in the reference; a (stand-in) TensorDict keeps its entries as lazy
    ``RepeatedRows`` (zero-copy multistart: the row-index scheme of the POMO episode)."""
    shape = [shape] if isinstance(shape, int) else shape
    for s in reversed(shape):
        if s <= 0:
            continue
        if hasattr(x, "get_raw") and len(x.batch_size) >= 1 and not _EAGER_BATCHIFY:
            x = _batchify_td_lazy(x, s)
        else:
            x = _batchify_single(x, s)
    return x


def _unbatchify_single(x, repeats: int):
    s = x.shape
    return x.view(repeats, s[0] // repeats, *s[1:]).permute(1, 0, *range(2, len(s) + 1))


def unbatchify(x: Union[Tensor, TensorDict], shape):
    """``ops.py:45-62``: ``(r b) ... -> b r ...``."""
    shape = [shape] if isinstance(shape, int) else shape
    for s in reversed(shape):
        x = _unbatchify_single(x, s) if s > 0 else x
    return x


def gather_by_index(src: Tensor, idx: Tensor, dim: int = 1, squeeze: bool = True) -> Tensor:
    """``ops.py:65-77`` on the gfx950 gather kernel.

    ``src`` is viewed as ``[outer, src.shape[dim], inner]`` (``inner`` = the product of
    the trailing dims, which must be contiguous); ``idx`` must have shape
    ``src.shape[:dim] + (M,)`` (trailing singleton dims allowed), which covers every
    call site on the hot path (rewards, CVRP demand, context embeddings, logprob
    gather, POMO best actions).  An empty batch, index or trailing block gives the empty
    tensor ``torch.gather`` gives (no launch); an empty ``src`` under a non-empty index is
    an out-of-range index like any other.
    """
    nat.require_device(src, idx)
    dim = dim % src.dim()
    if idx.dtype != torch.int64:
        idx = idx.long()
    while idx.dim() > dim + 1 and idx.shape[-1] == 1:
        idx = idx.squeeze(-1)
    lead = tuple(src.shape[:dim])
    if idx.dim() == dim:  # e.g. idx [B] for dim=1 -> one index per row
        idx = idx.unsqueeze(-1)
    if tuple(idx.shape[:dim]) != lead:
        raise RuntimeError(f"gather_by_index: index leading shape {tuple(idx.shape[:dim])} "
                           f"does not match source {lead}")
    trail = tuple(src.shape[dim + 1:])
    inner = 1
    for t in trail:
        inner *= t
    m = idx.shape[-1]
    out = torch.empty((*lead, m, *trail), dtype=src.dtype, device=src.device)
    if out.numel() == 0:  # an empty batch / index / trailing block: nothing to gather
        return out.squeeze(dim) if squeeze and m == 1 else out
    empty_src = src.shape[dim] == 0  # every index is out of range: the kernel reports it
    # the trailing block must be dense; leading dims must flatten to one stride
    if inner > 1 and not empty_src and not src[(0,) * (dim + 1)].is_contiguous():
        src = src.contiguous()
    outer = 1
    for t in lead:
        outer *= t
    if dim > 0:
        try:
            flat = src.view(outer, src.shape[dim], *trail)
        except RuntimeError:
            src = src.contiguous()
            flat = src.view(outer, src.shape[dim], *trail)
    else:
        flat = src.unsqueeze(0)
        outer = 1
    idx2 = idx.reshape(outer, m)
    es = src.element_size()
    # an empty source has no storage (a NULL pointer, which the entry point refuses) and no
    # element the kernel could read: any valid pointer stands in for it
    src_ptr = nat.ptr(out) if empty_src else nat.ptr(flat)
    # out-of-range indices: the device's deferred status word, raised at the next status
    # read (torch.gather on a HIP tensor raises a device-side assert that likewise
    # surfaces at the next sync); on the CPU (host build) the check is immediate
    host = src.device.type == "cpu"
    status = nat.scratch_status(src.device) if host else nat.deferred_status(src.device)
    nat.call("co_gather_by_index", src_ptr, outer, flat.shape[1], inner * es,
             flat.stride(0) * es, flat.stride(1) * es, nat.ptr(idx2), m, idx2.stride(0),
             idx2.stride(1), nat.ptr(out), nat.ptr(status), nat.stream_of(src))
    if host:
        nat.raise_deferred(int(status.item()), None)
    elif nat.SYNC_CHECKS:
        nat.check_deferred(src.device)
    if squeeze and m == 1:
        out = out.squeeze(dim)
    return out


def unbatchify_and_gather(x: Tensor, idx: Tensor, n: int):
    """``ops.py:80-85``."""
    x = unbatchify(x, n)
    return gather_by_index(x, idx, dim=idx.dim())


def best_of(rewards: Tensor, actions: Tensor, num_candidates: int):
    """The K-candidate evaluators' ``unbatchify`` -> ``max(dim=1)`` -> ``gather_by_index``
    (``rl4co/tasks/eval.py:137-144``) in one ``co_best_of`` launch.  ``rewards [K*B]`` and
    ``actions [K*B, T]`` (any strides, or None) are in ``batchify``'s repeat-major layout:
    candidate ``k`` of instance ``b`` is row ``k*B + b``.  Returns ``(best_reward [B],
    best_idx [B], best_actions [B, T])`` with ``torch.max``'s tie rule (the lowest ``k``;
    the first NaN wins); ``best_actions`` is None without ``actions``."""
    k = int(num_candidates)
    if k <= 0 or rewards.dim() != 1 or rewards.shape[0] % k != 0:
        raise ValueError(f"best_of: rewards of shape {tuple(rewards.shape)} do not hold "
                         f"{num_candidates} candidates per instance")
    if actions is not None and (actions.dim() != 2 or actions.shape[0] != rewards.shape[0]):
        raise ValueError(f"best_of: actions of shape {tuple(actions.shape)} do not fit rewards "
                         f"{tuple(rewards.shape)}")
    nat.require_device(rewards, actions)
    b = rewards.shape[0] // k
    rewards = rewards.contiguous().float()
    if actions is not None and actions.dtype != torch.int64:
        actions = actions.long()
    t = 0 if actions is None else actions.shape[1]
    dev = rewards.device
    best_r = torch.empty(b, dtype=torch.float32, device=dev)
    best_i = torch.empty(b, dtype=torch.int64, device=dev)
    best_a = None if actions is None else torch.empty((b, t), dtype=torch.int64, device=dev)
    if b > 0:
        sb, st = (0, 0) if actions is None else actions.stride()
        nat.call("co_best_of", b, k, t, nat.ptr(rewards), nat.ptr(actions), sb, st,
                 nat.ptr(best_r), nat.ptr(best_i), nat.ptr(best_a) if t > 0 else None, None,
                 nat.stream_of(rewards))
    return best_r, best_i, best_a


def sample_n_random_actions(td, n: int):
    """``ops.py:253-270``: ``n`` random feasible actions per instance, with replacement only
    when an instance has fewer than ``n`` (the depot column excluded from the count, as the
    reference does), flattened ``b n -> (n b)``.  Torch ops on the td's device (the
    reference draws on the CPU and moves the result); the draw follows torch's generator of
    that device and is not pinned."""
    action_mask = td["action_mask"]
    replace = bool(torch.sum(action_mask[:, 1:], 1).min() < n)
    ps = torch.rand(action_mask.shape, device=action_mask.device)
    ps[~action_mask] = -torch.inf
    ps = torch.softmax(ps, dim=1)
    selected = torch.multinomial(ps, n, replacement=replace)
    return selected.t().reshape(-1)


def get_distance(x: Tensor, y: Tensor):
    """``ops.py:88-90`` (elementwise helper, not on the timed path)."""
    return (x - y).norm(p=2, dim=-1)


def get_tour_length(ordered_locs: Tensor) -> Tensor:
    """``ops.py:93-101`` on the TSP reward kernel: closed tour over the given order."""
    nat.require_device(ordered_locs)
    b, m, _ = ordered_locs.shape
    locs = ordered_locs.contiguous().float()
    ident = torch.arange(m, device=locs.device, dtype=torch.int64)
    out = torch.empty(b, dtype=torch.float32, device=locs.device)
    nat.call("co_tsp_reward", b, m, m, nat.ptr(locs), b, nat.ptr(ident), 0, 1, 0,
             nat.ptr(out),
             None, nat.stream_of(locs))
    return -out


def get_distance_matrix(locs: Tensor) -> Tensor:
    """``ops.py:104-111``: ``[..., N, 2] -> [..., N, N]`` Euclidean distances (gfx950
    kernel, one launch)."""
    nat.require_device(locs)
    lead, n = locs.shape[:-2], locs.shape[-2]
    flat = locs.reshape(-1, n, 2).contiguous().float()
    out = torch.empty((flat.shape[0], n, n), dtype=torch.float32, device=locs.device)
    nat.call("co_distance_matrix", flat.shape[0], n, nat.ptr(flat), nat.ptr(out),
             nat.stream_of(flat))
    return out.reshape(*lead, n, n)


# -- what the batched local searches (two_opt, cvrp_local_search, slap_local_search) share --

def _pick_source(name, locs, distances):
    """Exactly one of ``locs`` and ``distances``: (the tensor, its argument's name)."""
    if (locs is None) == (distances is None):
        raise ValueError(f"{name}: give exactly one of locs and distances")
    return (locs, "locs") if locs is not None else (distances, "distances")


def _fit_source(name, src, which, lb, nodes, b, fits):
    """``src`` must be ``locs [lb, nodes, 2]`` or ``distances [lb, nodes, nodes]`` with
    ``lb > 0`` dividing the ``b`` rows.  Returns it contiguous in f32 and the C ABI's
    ``(locs, distances)`` pointer pair."""
    want = (lb, nodes, 2) if which == "locs" else (lb, nodes, nodes)
    if tuple(src.shape) != want or lb == 0 or b % lb != 0:
        raise ValueError(f"{name}: {which} of shape {tuple(src.shape)} does not fit {fits}")
    src = src.contiguous().float()
    return src, ((nat.ptr(src), None) if which == "locs" else (None, nat.ptr(src)))


def _search_outputs(shape, dtype, device, return_sweeps):
    """The rows ``[B, ...]`` and, if asked for, the sweeps per row (int32 ``[B]``)."""
    out = torch.empty(shape, dtype=dtype, device=device)
    sweeps = torch.empty(shape[0], dtype=torch.int32, device=device) if return_sweeps else None
    return out, sweeps


def _run_with_status(launch, status, device, messages):
    """``launch(status)`` on the caller's status word -- the caller reads it -- or on a
    scratch word of this call's own, read (one host sync) and raised from by ``messages``:
    ``(bit, exception, message)`` as ``RL4COEnvBase.raise_for_status`` takes them."""
    if status is not None:
        launch(status)
        return
    status = nat.scratch_status(device)
    launch(status)
    bits = int(status.item())
    nat.release_status(status, (bits,))
    for bit, exc, msg in messages:
        if bits & bit:
            raise exc(msg)


def two_opt(actions: Tensor, locs: Tensor = None, distances: Tensor = None,
            max_iterations: int = 1000, return_sweeps: bool = False, status: Tensor = None):
    """``tsp/local_search.py:14-74`` on ``co_tsp_two_opt``: best-improvement 2-opt on every
    row of ``actions [B, N]`` (any strides, any integer dtype), the whole search in one
    launch.  Exactly one of ``locs [LB, N, 2]`` and ``distances [LB, N, N]`` (f32) is
    given; row ``b`` uses instance ``b % LB`` (``LB == B`` normally; the multistart layout
    passes the un-replicated instances).  Returns int64 ``[B, N]`` on the actions' device,
    with ``return_sweeps`` also the sweeps executed per row (int32 ``[B]``).  A row that is
    not a permutation raises ``AssertionError("Invalid tour")`` -- or, with a caller-held
    ``status`` word, sets ``ST_INVALID_TOUR`` there and the caller reads it."""
    return _tsp_search("two_opt", None, actions, locs, distances, max_iterations,
                       return_sweeps, False, status)


def _tsp_search(name, mask, actions, locs, distances, max_iterations, return_sweeps,
                return_moves, status):
    """What ``two_opt`` (``mask`` None: the ``co_tsp_two_opt`` symbol) and
    ``tsp_local_search`` (``co_tsp_local_search`` with the operator ``mask``) share; ``name``
    is the caller's, for the messages."""
    src, which = _pick_source(name, locs, distances)
    nat.require_device(actions, src)
    if actions.dim() != 2:
        raise ValueError(f"{name}: actions must be [B, N], got {tuple(actions.shape)}")
    b, n = actions.shape
    if n > nat.TWO_OPT_MAX_N:
        raise ValueError(f"{name}: num_loc {n} exceeds the supported maximum "
                         f"{nat.TWO_OPT_MAX_N}")
    lb = src.shape[0] if src.dim() == 3 else 0
    src, src_ptrs = _fit_source(name, src, which, lb, n, b, f"actions {tuple(actions.shape)}")
    if actions.dtype != torch.int64:
        actions = actions.long()
    out, sweeps = _search_outputs((b, n), torch.int64, actions.device, return_sweeps)
    moves = torch.empty((b, 2), dtype=torch.int32, device=actions.device) if return_moves else None
    if b > 0 and n > 0:  # every row's counts are written
        args = (b, n, *src_ptrs, lb, nat.ptr(actions), actions.stride(0), actions.stride(1),
                int(max_iterations))
        if mask is None:
            symbol, args = "co_tsp_two_opt", args + (nat.ptr(out), nat.ptr(sweeps))
        else:
            symbol = "co_tsp_local_search"
            args += (mask, nat.ptr(out), nat.ptr(sweeps), nat.ptr(moves))
        _run_with_status(
            lambda st: nat.call(symbol, *args, nat.ptr(st), nat.stream_of(actions)),
            status, actions.device, [(nat.ST_INVALID_TOUR, AssertionError, "Invalid tour")])
    elif moves is not None:
        moves.zero_()
    res = (out,) + ((sweeps,) if return_sweeps else ()) + ((moves,) if return_moves else ())
    return res if len(res) > 1 else out


_TSP_LS_OPERATORS = {"two_opt": nat.TSP_LS_TWO_OPT, "or_opt": nat.TSP_LS_OR_OPT}


def tsp_local_search(actions: Tensor, locs: Tensor = None, distances: Tensor = None,
                     operators=("two_opt", "or_opt"), max_iterations: int = 1000,
                     return_sweeps: bool = False, return_moves: bool = False,
                     status: Tensor = None):
    """Best-improvement 2-opt + Or-opt descent on every row of ``actions [B, N]`` (any
    strides, any integer dtype) on ``co_tsp_local_search``, the whole search in one launch
    (``include/co_env.h`` states the Or-opt moves, the sweep and the tie rule).
    ``operators`` names the enabled neighbourhoods (``"two_opt"``, ``"or_opt"``); the
    distance source, the multistart layout, the result and the invalid-row behaviour are
    ``two_opt``'s.  With ``return_sweeps`` the sweeps per row (int32 ``[B]``) and with
    ``return_moves`` the applied (2-opt, Or-opt) moves per row (int32 ``[B, 2]``) follow the
    tours, in that order."""
    if isinstance(operators, str):
        operators = (operators,)
    operators = tuple(operators)
    unknown = [o for o in operators if o not in _TSP_LS_OPERATORS]
    if unknown or not operators:
        raise ValueError(f"tsp_local_search: operators must be a non-empty choice of "
                         f"{sorted(_TSP_LS_OPERATORS)}, got {operators!r}")
    mask = 0
    for o in operators:
        mask |= _TSP_LS_OPERATORS[o]
    return _tsp_search("tsp_local_search", mask, actions, locs, distances, max_iterations,
                       return_sweeps, return_moves, status)


def cvrp_local_search(actions: Tensor, demand: Tensor, locs: Tensor = None,
                      distances: Tensor = None, capacity: Tensor = None,
                      max_iterations: int = 1000, return_sweeps: bool = False,
                      status: Tensor = None):
    """Best-improvement 2-opt + relocate on the giant tour of every row of ``actions
    [B, T]`` (any strides, any integer dtype) on ``co_cvrp_local_search``, the whole search
    in one launch (``include/co_env.h`` states the moves, the integer capacity test and the
    tie rule).  ``demand [LB, N]`` and exactly one of ``locs [LB, N+1, 2]`` (depot first)
    and ``distances [LB, N+1, N+1]`` (f32) are given, ``capacity [LB]`` or ``[LB, 1]``
    optionally (default 1.0); row ``b`` uses instance ``b % LB``.  Returns int64 ``[B, T]``
    on the actions' device -- the routes separated by single zeros and padded with zeros --
    with ``return_sweeps`` also the sweeps executed per row (int32 ``[B]``).  A row that
    does not visit every customer exactly once (or whose demands / capacity are not finite
    values in [0, 4096]) raises ``AssertionError("Invalid tour")`` -- or, with a caller-held
    ``status`` word, sets ``ST_INVALID_TOUR`` there and comes back unchanged."""
    src, which = _pick_source("cvrp_local_search", locs, distances)
    nat.require_device(actions, demand, src, capacity)
    if actions.dim() != 2 or demand.dim() != 2:
        raise ValueError(f"cvrp_local_search: actions must be [B, T] and demand [LB, N], got "
                         f"{tuple(actions.shape)} and {tuple(demand.shape)}")
    b, t = actions.shape
    lb, n = demand.shape
    if n < 1 or t < n:
        raise ValueError(f"cvrp_local_search: {t} steps cannot visit {n} customers")
    if min(t, 2 * n) + 1 > nat.CVRP_LS_MAX_LEN:
        raise ValueError(f"cvrp_local_search: a giant tour of up to {min(t, 2 * n) + 1} "
                         f"positions exceeds the supported maximum {nat.CVRP_LS_MAX_LEN}")
    src, src_ptrs = _fit_source("cvrp_local_search", src, which, lb, n + 1, b,
                                f"actions {tuple(actions.shape)} and demand "
                                f"{tuple(demand.shape)}")
    if capacity is not None:
        if capacity.numel() != lb:
            raise ValueError(f"cvrp_local_search: capacity of shape {tuple(capacity.shape)} "
                             f"does not fit demand {tuple(demand.shape)}")
        capacity = capacity.reshape(lb).contiguous().float()
    demand = demand.contiguous().float()
    if actions.dtype != torch.int64:
        actions = actions.long()
    out, sweeps = _search_outputs((b, t), torch.int64, actions.device, return_sweeps)
    if b > 0:
        _run_with_status(lambda st: nat.call(
            "co_cvrp_local_search", b, n, t, *src_ptrs, nat.ptr(demand), nat.ptr(capacity), lb,
            nat.ptr(actions), actions.stride(0), actions.stride(1), int(max_iterations),
            nat.ptr(out), nat.ptr(sweeps), nat.ptr(st), nat.stream_of(actions)),
            status, actions.device, [(nat.ST_INVALID_TOUR, AssertionError, "Invalid tour")])
    return (out, sweeps) if return_sweeps else out


def slap_local_search(assignment: Tensor, picklist: Tensor, locs: Tensor = None,
                      distances: Tensor = None, max_iterations: int = 1000,
                      return_sweeps: bool = False, return_cost: bool = False,
                      status: Tensor = None, scheme: int = nat.SLAP_LS_AUTO):
    """Best-improvement product swap + move-to-free-slot on every row of ``assignment
    [B, P]`` (any strides, any integer dtype; column p is product p's slot) on
    ``co_slap_local_search``, the whole search in one launch (``include/co_env.h`` states
    the integer objective, the moves and the tie rule).  ``picklist [LB, O, K]`` and exactly
    one of ``locs [LB, L, 2]`` and ``distances [LB, L, L]`` (f32) are given; row ``b`` uses
    instance ``b % LB``.  Returns ``[B, P]`` in the input's dtype on its device, with
    ``return_sweeps`` also the sweeps executed per row (int32 ``[B]``) and with
    ``return_cost`` the integer objective of the returned row (int64 ``[B]``, distances in
    units of 2^-20; -1 for a row that failed its check).  A row with a slot outside
    ``0..L-1`` or taken twice (or a non-finite / out-of-range coordinate or distance)
    raises ``AssertionError("Invalid assignment")``, a picklist entry outside ``0..P-1``
    ``IndexError`` -- or, with a caller-held ``status`` word, sets ``ST_INVALID_TOUR`` /
    ``ST_INDEX_RANGE`` there and comes back unchanged.  ``scheme`` (device only) forces the
    direct or the table evaluation scheme; the results do not depend on it."""
    src, which = _pick_source("slap_local_search", locs, distances)
    nat.require_device(assignment, picklist, src)
    if assignment.dim() != 2 or picklist.dim() != 3:
        raise ValueError(f"slap_local_search: assignment must be [B, P] and picklist "
                         f"[LB, O, K], got {tuple(assignment.shape)} and "
                         f"{tuple(picklist.shape)}")
    if assignment.dtype.is_floating_point or assignment.dtype == torch.bool:
        raise ValueError(f"slap_local_search: assignment must hold integers, got "
                         f"{assignment.dtype}")
    b, p = assignment.shape
    lb, o, k = picklist.shape
    l = src.shape[1] if src.dim() == 3 else -1
    src, src_ptrs = _fit_source("slap_local_search", src, which, lb, l, b,
                                f"assignment {tuple(assignment.shape)} and picklist "
                                f"{tuple(picklist.shape)}")
    if not 1 <= p <= nat.SLAP_LS_MAX_PRODUCTS:
        raise ValueError(f"slap_local_search: {p} products; the supported range is 1.."
                         f"{nat.SLAP_LS_MAX_PRODUCTS}")
    if not p <= l <= nat.SLAP_LS_MAX_SLOTS:
        raise ValueError(f"slap_local_search: {l} slots cannot hold {p} products or exceed "
                         f"the supported maximum {nat.SLAP_LS_MAX_SLOTS}")
    if not 1 <= o * k <= 65536:
        raise ValueError(f"slap_local_search: {o} orders of {k} picks; 1..65536 picks are "
                         "supported")
    picklist = picklist.contiguous()
    if picklist.dtype != torch.int64:
        picklist = picklist.long()
    dtype, dev = assignment.dtype, assignment.device
    assign = assignment.contiguous() if dtype == torch.int32 else assignment.to(torch.int32)
    wild = None
    if dtype == torch.int64:  # a slot beyond int32 must not wrap into range
        wild = (assignment < -1) | (assignment > l)
        assign = torch.where(wild, -1, assignment).to(torch.int32)
    out, sweeps = _search_outputs((b, p), torch.int32, dev, return_sweeps)
    cost = torch.empty(b, dtype=torch.int64, device=dev) if return_cost else None

    def result():
        rows = out if dtype == torch.int32 else out.to(dtype)
        if wild is not None:  # such a row failed its check: it comes back as it was
            rows = torch.where(wild, assignment, rows)
        res = tuple(x for x in (rows, sweeps, cost) if x is not None)
        return res if len(res) > 1 else res[0]

    if b == 0:
        return result()
    args = (b, l, p, o, k, *src_ptrs, lb, nat.ptr(picklist), nat.ptr(assign),
            int(max_iterations), nat.ptr(out), nat.ptr(sweeps), nat.ptr(cost))

    def launch(st):
        if scheme == nat.SLAP_LS_AUTO:
            nat.call("co_slap_local_search", *args, nat.ptr(st), nat.stream_of(assign))
            return
        if dev.type == "cpu":
            raise ValueError("slap_local_search: the host build has one evaluation scheme")
        if scheme == nat.SLAP_LS_TABLE and not nat.slap_ls_table_fits(p, l):
            raise ValueError(f"slap_local_search: the table of {p} products x {l} slots does "
                             f"not fit the LDS budget of {nat.SLAP_LS_LDS_BYTES} bytes")
        nat.call("co_slap_local_search_scheme", *args, int(scheme), nat.ptr(st),
                 nat.stream_of(assign))

    _run_with_status(launch, status, dev, [
        (nat.ST_INVALID_TOUR, AssertionError, "Invalid assignment"),
        (nat.ST_INDEX_RANGE, IndexError, "index out of range in SLAP picklist")])
    return result()


def get_num_starts(td, env_name=None):
    """``ops.py:126-136``."""
    n = td["action_mask"].shape[-1]
    if env_name == "pdp":
        n = (n - 1) // 2
    elif env_name in ["cvrp", "cvrptw", "sdvrp", "mtsp", "op", "pctsp", "spctsp"]:
        n = n - 1
    return n


def select_start_nodes(td, env, num_starts):
    """``ops.py:139-163``: start action of env ``s*B + b`` is ``s % num_loc`` (TSP) or
    ``s % num_loc + 1`` (depot envs).  Envs without ``generator.num_loc`` (SLAP)
    keep the reference's ``0xFFFFFFFF`` sentinel and its off-by-one."""
    num_loc = env.generator.num_loc if hasattr(env.generator, "num_loc") else 0xFFFFFFFF
    sel = torch.arange(num_starts, device=td.device).repeat_interleave(td.shape[0]) % num_loc
    if env.name in ["tsp", "atsp", "flp", "mcp"]:
        return sel
    if env.name in ["jssp", "fjsp"]:
        raise NotImplementedError("Multistart not yet supported for FJSP/JSSP")
    return sel + 1


def get_best_actions(actions, max_idxs):
    """``ops.py:186-188``."""
    actions = unbatchify(actions, max_idxs.shape[0])
    return actions.gather(0, max_idxs[..., None, None])


def calculate_entropy(logprobs: Tensor):
    """``ops.py:114-122``: entropy of per-step log-probabilities ``[B, steps, n]``,
    summed over steps (torch ops on the device tensors; not on the timed path)."""
    logprobs = torch.nan_to_num(logprobs, nan=0.0)
    entropy = -(logprobs.exp() * logprobs).sum(dim=-1)
    entropy = entropy.sum(dim=1)
    assert entropy.isfinite().all(), "Entropy is not finite"
    return entropy
