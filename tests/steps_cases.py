"""Shared by tests/test_gpu_steps_kernels.py (the K-steps-per-launch entries co_tsp_steps of
csrc/tsp.hip and co_slap_closest_steps of csrc/slap.hip on the device, through direct C-ABI
calls) and tests/test_host_steps_cases.py (the case builders' own claims, and the references
against the host build's single-step entries chained K times): case builders, CPU references
and assertions, in the style of tests/env_step_cases.py, whose buffers (``Outs``, ``place``),
calls (``run``), assertions (``assert_same``) and SLAP state and references (``slap_state``,
``slap_step_ref``, ``slap_closest_ref``) are reused.  Not a test module; nothing here needs a
GPU.

References.  Every output is an integer or a bool and is compared bit for bit.  co_tsp_steps
is held to K applications of ``TSPOracle._step`` to the same arbitrary -- not
policy-reachable -- state on the CPU; co_slap_closest_steps to K times "the oracle's
closest-free action, then ``SLAPOracle._step``" with step t's product in column t.  The
oracle raises on an index out of range; there the references restate the rule the single-step
entries document (``_tsp_bad_rule``, ``_slap_bad_rule``): the step clears nothing (TSP) /
leaves the assignment row as it was (SLAP), the status bit is set, everything else is as
usual.  tests/test_host_steps_cases.py checks both references, these rules included, against
the host build's co_tsp_step / co_slap_step chained K times: two independent CPU
implementations of every expected value.

What a launch leaves behind.  Step t reads buffer A for even t and writes B, the reverse for
odd t.  With S_0 the given state and S_t the state after t steps, the buffer written last (B
for odd K, A for even K) holds S_K and the other one S_(K-1) -- for K = 1 the untouched
input.  current / done / reward (and the SLAP assignment) are the last step's; row t of the
SLAP ``action_out`` is step t's action.  Each K is a launch of its own, so the K lists below
make the intermediate steps visible.

Coverage: every template instantiation and kernel named in the launch code of the two
entries (and of co_tsp_step, which co_tsp_steps falls back to), the dispatch condition, and
the case ids (test function[id]) that reach it.  ``path`` in an id is what the ``*_path``
functions below compute from the same conditions; tests/test_host_steps_cases.py asserts
that every path listed here has cases at both ends of its range.

  tsp.hip  co_tsp_steps                                    test_tsp_steps[N..-path]
    W = N / 4 words per row, WG = ceil(W / 4); the group kernel iff N % 4 == 0, WG >= 5,
    W <= 256 and both masks 4-byte aligned; 64 / G rows per wave, 4 waves per workgroup,
    actions loaded 8 steps at a time
    tsp_steps_group_kernel<8>    N 68 .. 128       N68-*-steps8, N128-*-steps8, N100-*
    tsp_steps_group_kernel<16>   N 132 .. 256      N132-*-steps16, N256-*-steps16
    tsp_steps_group_kernel<32>   N 260 .. 512      N260-*-steps32, N512-*-steps32
    tsp_steps_group_kernel<64>   N 516 .. 1024     N516-*-steps64, N1024-*-steps64
      per G: B = 1, 64 / G + 1, 4 (64 / G) + 1 (a workgroup and one row), G = 8 also B = 7;
      K = 1, 2, 7, 8, 9, 17 at the lower N, 2 and 9 at the upper; first_mode 0 and 1 (with
      first_mode 1 and K = 1 first_a is NULL); -pad5: act_stride = B + 5; -nocur:
      current_out NULL
    otherwise K co_tsp_step calls (-single-<co_tsp_step's path>):
      N64-*-single-group4 (N % 4 == 0 but WG = 4), N1028-*-single-tile (W > 256),
      N70-*-single-tile (N % 4 != 0), N100-*-moffa1-*-single-tile and N100-*-moffb1-*
      (either mask one byte off 4-byte alignment)
    status: test_tsp_steps_status[path-value] (one bad action -1, N, 2^32 + 1 or 2^34 + 5
      alone, at step 0, 7, 8 and K - 1 of one row, on every G and both fallback kernels)
    rejections: test_steps_rejections[co_tsp_steps]
  tsp.hip  co_tsp_step           tests/test_gpu_envs.py test_tsp_step_kernel_paths_vs_reference[B-N]
    tsp_step_group_kernel<G>   N % 4 == 0, N <= 1024, masks 4-byte aligned; G from WG:
      <2>   N 4 .. 32        *-4, *-16, *-20, *-24, *-32
      <4>   N 36 .. 64       *-36, *-64        (and N64-*-single-group4 above)
      <8>   N 68 .. 128      *-68, *-100, *-128
      <16>  N 132 .. 256     *-132, *-252, *-256
      <32>  N 260 .. 512     *-260, *-512
      <64>  N 516 .. 1024    *-516, *-1024
    tsp_step_kernel (the 64-row tile kernel)   otherwise: *-3 (N % 4 != 0), *-1028 (N > 1024)
      (and N70 / N1028 / N100-moff -single-tile above)
  slap.hip  co_slap_closest_steps                          test_slap_steps[L..-path]
    the sorted-key kernel iff L % 4 == 0, L <= 256, dist 16-byte aligned and both masks
    4-byte aligned; 16 lanes per row, 16 rows per workgroup; KU = ceil(L / 64) units of 4
    locations per lane, EPL = 4, 8, 16, 16 sorted keys per lane (two in registers, EPL - 2
    in LDS)
    slap_closest_steps_kernel<1>   L <= 64     L4-*-sorted1 (one unit: 15 lanes clamp), L64-*
    slap_closest_steps_kernel<2>   L <= 128    L68-*-sorted2, L128-*-sorted2
    slap_closest_steps_kernel<3>   L <= 192    L132-*-sorted3, L192-*-sorted3
    slap_closest_steps_kernel<4>   L <= 256    L196-*-sorted4, L256-*-sorted4
      per L: B = 1, 3, 5, 17 (partial waves whose dead groups mirror the last row; a second
      workgroup); P = 1, 7, 20 (the out-of-place copy strides 16); K = 1, 2, 3, P; the
      assignment in place (-ip) and out of place at step 0 into a pre-filled buffer (-oop);
      to_choose per row with tc_stride = K + 2 (-tc), NULL with tc_stride 0 (-null0), NULL
      with tc_stride + K == P (-nullend); states ties / grid / frac; -pad3: act_stride B + 3
    otherwise K co_slap_closest_step calls (-single):
      L260-*-single, L62-*-single, L100-*-moffa1-*, L100-*-moffb1-*, L100-*-doff4-*
    the rows ``slap_state`` does not make (P = 20, K = 20): test_slap_steps_special[L-ip|oop]
      at L 64, 68, 128, 132, 192, 196, 256 (every KU at both ends but L = 4) and 260
    status: test_slap_steps_status[path-step-ip|oop] (one bad product alone at step 0, 1 and
      K - 1, on each KU and the fallback)
    rejections: test_steps_rejections[co_slap_closest_steps]
"""
import collections
import functools

import torch

import env_step_cases as sc
from env_step_cases import (E_INVAL, I32, I64, U8, Outs, assert_same, place, rc_of, run,
                            slap_closest_ref, slap_state, slap_step_ref, word)
from episode_cases import FILL
from oracle.envs import TSPOracle
from oracle.td import TD
from rl4co_slap_amd import _native as nat

E_MODE = -3
K_MAX = 1 << 20


def _ptr(t):
    return t.data_ptr()


def _parent(v):
    """The sentinel parent ``place`` put the input ``v`` in."""
    return v._base if v._base is not None else v


def _final(name, states, k):
    """Buffers A and B after K steps: S_K in the one written last, S_(K-1) in the other."""
    last, prev = states[k][name], states[k - 1][name]
    return (last, prev) if k % 2 == 0 else (prev, last)


# ============================================================================= TSP
def tsp_step_path(n, mask_off=0):
    """The kernel co_tsp_step launches (its dispatch conditions restated)."""
    if n % 4 == 0 and n // 4 <= 256 and mask_off % 4 == 0:
        wg = (n // 4 + 3) // 4
        return f"group{next(g for g in (2, 4, 8, 16, 32, 64) if wg <= g)}"
    return "tile"


def tsp_steps_path(n, mask_off=0):
    """The kernel co_tsp_steps launches, or ``single-`` and the kernel of the K co_tsp_step
    calls it makes instead; ``mask_off`` the byte offset of either mask from alignment."""
    w = n // 4
    wg = (w + 3) // 4
    if n % 4 == 0 and wg >= 5 and w <= 256 and mask_off % 4 == 0:
        return f"steps{next(g for g in (8, 16, 32, 64) if wg <= g)}"
    return "single-" + tsp_step_path(n, mask_off)


# the N of test_gpu_envs.py's test_tsp_step_kernel_paths_vs_reference: both ends of every
# tsp_step_group_kernel<G> and the tile kernel on either side of them
TSP_STEP_N = [3, 4, 16, 20, 24, 32, 36, 64, 68, 100, 128, 132, 252, 256, 260, 512, 516, 1024, 1028]


def tsp_steps_group(n):
    """G of the group kernel at ``n``, or 0 on the fallback."""
    p = tsp_steps_path(n)
    return int(p[5:]) if p.startswith("steps") else 0


TSP_KINDS = ("random", "empty", "ends_at_k", "ends_mid", "revisit")
TspSteps = collections.namedtuple("TspSteps", "mask i first acts kinds")


def tsp_special_nodes(n):
    """Bytes 0 and 3 of the first and of the last word of a row and, where a lane of the
    group kernel has four words (W > 3 G), a byte of lane 0's last slot, word 3 G."""
    nodes = [0, 3, n - 4, n - 1]
    g = tsp_steps_group(n)
    if g and n // 4 > 3 * g:
        nodes.append(4 * 3 * g + 2)
    return list(dict.fromkeys(x for x in nodes if 0 <= x < n))


@functools.lru_cache(maxsize=None)
def tsp_steps_state(n, b, k, first_mode):
    """An arbitrary TSP state of ``b`` rows and ``k`` actions per row.  Row r is of kind
    ``TSP_KINDS[(r + k + first_mode) % 5]`` (so a batch of five rows holds every kind, and
    one row runs through them as K changes): random mask bytes with the special nodes as its
    first actions; nothing left from the start; a mask of exactly the K distinct actions
    (the special nodes first), which empties at step K; for K >= 3 a mask of the first K / 2
    actions, which empties at that middle step and is revisited from then on; a node set in
    the mask visited at steps 0 and 1.  ``i`` is arbitrary and positive (the last row above
    2^32; with first_mode 1 row 0 has i == 0, so that the oracle's batch-wide first-step
    test agrees with the mode), ``first`` arbitrary: beyond N, negative on odd rows."""
    g = torch.Generator().manual_seed(7919 * n + 131 * b + 7 * k + first_mode)
    mask = torch.rand(b, n, generator=g) < 0.6
    acts = torch.randint(0, n, (k, b), generator=g)
    i = torch.randint(1, 1 << 20, (b, 1), generator=g)
    first = torch.randint(1 << 10, 1 << 40, (b,), generator=g) * (1 - 2 * (torch.arange(b) % 2))
    sp = tsp_special_nodes(n)
    kinds = []
    for r in range(b):
        kind = TSP_KINDS[(r + k + first_mode) % 5]
        if kind == "ends_mid" and k < 3:
            kind = "revisit"
        if kind == "revisit" and k < 2:
            kind = "random"
        rest = [x for x in torch.randperm(n, generator=g).tolist() if x not in sp]
        if kind == "random":
            for t in range(min(k, len(sp))):
                acts[t, r] = sp[(t + r) % len(sp)]
        elif kind == "empty":
            mask[r] = False
        elif kind == "ends_at_k":
            nodes = (sp + rest)[:k]
            acts[:, r] = torch.tensor(nodes)
            mask[r] = False
            mask[r, nodes] = True
        elif kind == "ends_mid":
            m = k // 2
            nodes = (rest[:1] + sp + rest[1:])[:m]
            acts[:, r] = torch.tensor([nodes[t % m] for t in range(k)])
            mask[r] = False
            mask[r, nodes] = True
        else:
            acts[1, r] = acts[0, r]
            mask[r, acts[0, r]] = True
        kinds.append(kind)
    i[b - 1] = (1 << 32) + 7 + b
    if first_mode == 1:
        i[0] = 0
    return TspSteps(mask, i, first, acts, tuple(kinds))


def _tsp_bad_rule(new, old, raw, bad, took_first):
    """An action out of range, as co_tsp_step documents it: the step clears nothing in that
    row, ``current`` (and ``first`` on a first step) is the raw action, the rest as usual."""
    new["action_mask"][bad] = old["action_mask"][bad]
    new["done"][bad] = ~old["action_mask"][bad].any(-1)
    new["current_node"][bad] = raw[bad]
    if took_first:
        new["first_node"][bad] = raw[bad]


def tsp_steps_ref(mask, i, first, acts, first_mode):
    """S_0 .. S_K: K applications of TSPOracle._step, and the status word."""
    k, b = acts.shape
    n = mask.shape[1]
    states = [{"action_mask": mask.clone(), "i": i.clone(), "first_node": first.clone()}]
    status = 0
    for t in range(k):
        old, raw = states[-1], acts[t]
        bad = (raw < 0) | (raw >= n)
        took_first = not bool(old["i"].all())  # the oracle's batch-wide test
        assert took_first == (t == 0 and first_mode == 1), "i disagrees with first_mode"
        td = TD({"action": torch.where(bad, torch.zeros_like(raw), raw), "i": old["i"],
                 "first_node": old["first_node"], "action_mask": old["action_mask"]}, [b])
        out = TSPOracle._step(td)
        new = {key: out[key].clone() for key in ("action_mask", "i", "first_node", "current_node",
                                                 "done", "reward")}
        if bool(bad.any()):
            _tsp_bad_rule(new, old, raw, bad, took_first)
            status |= nat.ST_INDEX_RANGE
        states.append(new)
    return states, status


def tsp_steps_want(states, status, k):
    """What the launch leaves in every buffer."""
    want = {"current_node": states[k]["current_node"], "done": states[k]["done"],
            "step_reward": states[k]["reward"], "status": torch.tensor([status], dtype=I32)}
    for name, key in (("mask", "action_mask"), ("i", "i"), ("first", "first_node")):
        want[name + "_a"], want[name + "_b"] = _final(key, states, k)
    return want


TspStepsCase = collections.namedtuple("TspStepsCase", "n b k first_mode off_a off_b pad cur_null")


def tsp_steps_id(c):
    return (f"N{c.n}-B{c.b}-K{c.k}-fm{c.first_mode}-"
            f"{'moffa%d-' % c.off_a if c.off_a else ''}{'moffb%d-' % c.off_b if c.off_b else ''}"
            f"{'pad%d-' % c.pad if c.pad else ''}{'nocur-' if c.cur_null else ''}"
            f"{tsp_steps_path(c.n, max(c.off_a, c.off_b))}")


TSP_K_ALL, TSP_K_UPPER = (1, 2, 7, 8, 9, 17), (2, 9)
TSP_GROUP_N = {8: (68, 128), 16: (132, 256), 32: (260, 512), 64: (516, 1024)}


def tsp_steps_batches(g):
    """B per G: one row, a wave and one row, a workgroup and one row (G = 8 also 7)."""
    return [1, 64 // g + 1, 4 * (64 // g) + 1] + ([7] if g == 8 else [])


def _tsp_steps_cases():
    out = []

    def add(n, b, k, fm, off_a=0, off_b=0, pad=0, cur_null=False):
        out.append(TspStepsCase(n, b, k, fm, off_a, off_b, pad, cur_null))

    for g, (lo, hi) in TSP_GROUP_N.items():
        for n, ks in ((lo, TSP_K_ALL), (hi, TSP_K_UPPER)):
            for b in tsp_steps_batches(g):
                for k in ks:
                    for fm in (0, 1):
                        add(n, b, k, fm)
        add(lo, 64 // g + 1, 9, 1, pad=5)
        add(hi, 64 // g + 1, 17, 0, pad=5)
    add(100, 9, 9, 0, cur_null=True)
    add(1028, 3, 2, 1, cur_null=True)
    for n in (64, 1028, 70):            # the fallback by N
        for b, k in ((1, 1), (17, 2), (5, 9)):
            for fm in (0, 1):
                add(n, b, k, fm)
    for off_a, off_b in ((1, 0), (0, 1)):   # ... and by either mask's alignment
        for b, k in ((1, 1), (9, 2), (9, 9)):
            for fm in (0, 1):
                add(100, b, k, fm, off_a, off_b)
    return out


TSP_STEPS_CASES = _tsp_steps_cases()


def _tsp_steps_call(dev, c, st, acts):
    b, n, k = c.b, c.n, c.k
    o = Outs(dev)
    ma, mb = o.new("mask_a", (b, n), U8, c.off_a), o.new("mask_b", (b, n), U8, c.off_b)
    ia, ib = o.new("i_a", (b, 1), I64), o.new("i_b", (b, 1), I64)
    o["mask_a"].t.copy_(st.mask.to(U8))
    o["i_a"].t.copy_(st.i)
    fa = None
    if not (c.first_mode == 1 and k == 1):  # the only step takes the action: first_a NULL
        fa = o.new("first_a", b, I64)
        o["first_a"].t.copy_(st.first)
    fb = o.new("first_b", b, I64)
    cur = None if c.cur_null else o.new("current_node", b, I64)
    done, rew = o.new("done", b, U8), o.new("step_reward", b, U8)
    status = word(o, "status")
    a = place(acts, dev, 0, b + c.pad if c.pad else None)
    before = _parent(a).clone()
    run(dev, "co_tsp_steps", b, n, k, _ptr(a), b + c.pad, ma, ia, fa, mb, ib, fb, cur, done, rew,
        c.first_mode, status)
    o.check_guards()
    assert torch.equal(_parent(a), before), "the actions (or their pad columns) were written"
    return o.cpu()


def _same_keys(got, want):
    for key, v in got.items():
        assert_same(key, v, want[key])


def check_tsp_steps(dev, c):
    st = tsp_steps_state(c.n, c.b, c.k, c.first_mode)
    states, status = tsp_steps_ref(st.mask, st.i, st.first, st.acts, c.first_mode)
    assert status == 0
    got = _tsp_steps_call(dev, c, st, st.acts)
    assert ("first_a" in got) == (not (c.first_mode == 1 and c.k == 1))
    assert ("current_node" in got) == (not c.cur_null)
    _same_keys(got, tsp_steps_want(states, status, c.k))


TSP_STATUS_N = {"steps8": 100, "steps16": 200, "steps32": 300, "steps64": 600,
                "single-group4": 64, "single-tile": 70}
# -1, N, 2^32 + 1 (node 1 once truncated to 32 bits) and 2^34 + 5, whose word index
# (a >> 2) truncates to word 1: a kernel that did not drop the action would clear node 5
TSP_BAD = {"neg": lambda n: -1, "n": lambda n: n, "big": lambda n: (1 << 32) + 1,
           "wrap": lambda n: (1 << 34) + 5}
TSP_WRAP_NODE = 5
TSP_STATUS_K, TSP_STATUS_B, TSP_STATUS_ROW = 17, 5, 2


def tsp_status_steps():
    return (0, 7, 8, TSP_STATUS_K - 1)


def tsp_status_acts(n, which, step, first_mode):
    """The 17 actions of five rows with one bad action alone: row 2, step ``step``.  Node 5
    of that row is unvisited and stays so, so that a bad action taken for node 5 shows."""
    st = tsp_steps_state(n, TSP_STATUS_B, TSP_STATUS_K, first_mode)
    acts, mask = st.acts.clone(), st.mask.clone()
    col = acts[:, TSP_STATUS_ROW]
    col[col == TSP_WRAP_NODE] = TSP_WRAP_NODE + 1
    mask[TSP_STATUS_ROW, TSP_WRAP_NODE] = True
    acts[step, TSP_STATUS_ROW] = TSP_BAD[which](n)
    return st._replace(mask=mask), acts


def check_tsp_steps_status(dev, path, which):
    """One out-of-range action (-1, N, 2^32 + 1 or 2^34 + 5) alone in a launch of 17 steps, at step 0,
    7, 8 or 16 of row 2: the bit, and every buffer -- the later steps of that row and every
    other row included -- as the reference has it."""
    n = TSP_STATUS_N[path]
    assert tsp_steps_path(n) == path
    for step in tsp_status_steps():
        first_mode = 1 if step in (0, 8) else 0
        st, acts = tsp_status_acts(n, which, step, first_mode)
        states, status = tsp_steps_ref(st.mask, st.i, st.first, acts, first_mode)
        assert status == nat.ST_INDEX_RANGE
        c = TspStepsCase(n, TSP_STATUS_B, TSP_STATUS_K, first_mode, 0, 0, 0, False)
        got = _tsp_steps_call(dev, c, st, acts)
        assert int(got["status"]) == nat.ST_INDEX_RANGE, (step, int(got["status"]))
        _same_keys(got, tsp_steps_want(states, status, TSP_STATUS_K))


def check_tsp_ref_against_single_steps(dev, n, b, k, first_mode, acts=None, st=None):
    """``tsp_steps_ref`` against co_tsp_step chained K times on ``dev`` (the host build)."""
    st = tsp_steps_state(n, b, k, first_mode) if st is None else st
    acts = st.acts if acts is None else acts
    states, status = tsp_steps_ref(st.mask, st.i, st.first, acts, first_mode)
    o = Outs(dev)
    bufs = [{key: o.new(f"{key}{j}", shape, dt) for key, shape, dt in
             (("mask", (b, n), U8), ("i", (b, 1), I64), ("first", b, I64))} for j in (0, 1)]
    o["mask0"].t.copy_(st.mask.to(U8))
    o["i0"].t.copy_(st.i)
    o["first0"].t.copy_(st.first)
    cur, done, rew = o.new("cur", b, I64), o.new("done", b, U8), o.new("rew", b, U8)
    status_w = word(o, "status")
    for t in range(k):
        a = place(acts[t], dev)
        s, d = bufs[t & 1], bufs[(t + 1) & 1]
        run(dev, "co_tsp_step", b, n, _ptr(a), s["mask"], d["mask"], s["i"], d["i"], s["first"],
            d["first"], cur, done, rew, first_mode if t == 0 else 0, None, status_w)
        o.check_guards()
        got, want, j = o.cpu(), states[t + 1], (t + 1) & 1
        assert_same("action_mask", got[f"mask{j}"], want["action_mask"])
        assert_same("i", got[f"i{j}"], want["i"])
        assert_same("first_node", got[f"first{j}"], want["first_node"])
        assert_same("current_node", got["cur"], want["current_node"])
        assert_same("done", got["done"], want["done"])
        assert_same("reward", got["rew"], want["reward"])
    assert int(o.cpu()["status"]) == status


# ============================================================================ SLAP
def slap_steps_ku(l):
    return (l // 4 + 15) // 16


def slap_steps_epl(ku):
    return 16 if ku == 3 else 4 * ku


def slap_steps_path(l, mask_off=0, dist_off=0):
    """The kernel co_slap_closest_steps launches, or ``single``: K co_slap_closest_step
    calls.  ``mask_off`` the byte offset of either mask from 4-byte alignment."""
    if l % 4 == 0 and l <= 256 and mask_off % 4 == 0 and dist_off % 16 == 0:
        return f"sorted{slap_steps_ku(l)}"
    return "single"


SlapSteps = collections.namedtuple("SlapSteps", "mask i assignment dist product")
SLAP_KINDS = ("ties", "grid", "frac")


def frac_dist(b, l, g):
    """Distinct f32 distances: fractional values 0.013 + 0.37 j in random order, the three
    smallest replaced by the subnormals 1e-40, 2e-40, 3e-40 and two values negative."""
    perm = torch.stack([torch.randperm(l, generator=g) for _ in range(b)]).float()
    dist = perm * 0.37 + 0.013
    dist = torch.where(perm < 3, (perm + 1) * torch.tensor(1e-40), dist)
    return torch.where((perm == 5) | (perm == 6), -dist, dist)


def _products(b, p, k, g):
    """A product per row and step: integers in [0, P), negative (python-indexed) on every
    third row, with a fraction that truncates toward zero on every fourth."""
    prod = torch.randint(0, p, (b, k), generator=g).float()
    r = torch.arange(b)[:, None].expand(b, k)
    prod = torch.where(r % 3 == 1, prod - p, prod)
    prod = torch.where(r % 4 == 2, prod + 0.75, prod)
    return torch.where((r % 4 == 3) & (prod == 0), torch.tensor(-0.5), prod)


@functools.lru_cache(maxsize=None)
def slap_steps_state(l, p, b, k, kind):
    """``slap_state``'s masks, ``i``, partial assignment and distances (kinds "ties": halves
    with exact ties, -0.0 and +inf; "grid") or distinct fractional distances with subnormals
    ("frac"), and a product per row and step."""
    g = torch.Generator().manual_seed(977 * l + 31 * p + 7 * b + k + len(kind))
    s = slap_state(l, p, b, "grid" if kind == "frac" else kind)
    dist = frac_dist(b, l, g) if kind == "frac" else s.dist
    return SlapSteps(s.mask, s.i, s.assignment, dist, _products(b, p, k, g))


def _slap_bad_rule(prod, p):
    """Rows whose product, truncated toward zero and wrapped once as python indexing does,
    is outside [0, P): the step leaves their assignment row as it was and sets the bit."""
    pi = prod.to(torch.int)
    pi = torch.where(pi < 0, pi + p, pi)
    return (pi < 0) | (pi >= p)


def slap_steps_ref(mask, i, assignment, dist, product):
    """S_0 .. S_K, the K action rows and the status word: K times the oracle's closest-free
    action, then SLAPOracle._step with column t of ``product``."""
    b, p = assignment.shape
    states = [{"action_mask": mask.clone(), "i": i.clone(), "assignment": assignment.clone()}]
    actions, status = [], 0
    for t in range(product.shape[1]):
        old = states[-1]
        act = slap_closest_ref(sc.SlapState(old["action_mask"], None, None, None, None, dist))
        bad = _slap_bad_rule(product[:, t], p)
        new = slap_step_ref(old["action_mask"], old["i"], old["assignment"], act,
                            torch.where(bad, torch.zeros(b), product[:, t]))
        new = {key: v.clone() for key, v in new.items()}
        if bool(bad.any()):
            new["assignment"][bad] = old["assignment"][bad]
            status |= nat.ST_INDEX_RANGE
        states.append(new)
        actions.append(act)
    return states, torch.stack(actions), status


def slap_steps_want(states, actions, status, k):
    want = {"assignment": states[k]["assignment"], "done": states[k]["done"],
            "step_reward": states[k]["step_reward"], "action": actions,
            "status": torch.tensor([status], dtype=I32)}
    want["mask_a"], want["mask_b"] = _final("action_mask", states, k)
    want["i_a"], want["i_b"] = _final("i", states, k)
    return want


SlapStepsCase = collections.namedtuple("SlapStepsCase",
                                       "l p b k off_a off_b dist_off inplace tc kind pad")
SLAP_TC = ("tc", "null0", "nullend")


def slap_steps_id(c):
    return (f"L{c.l}-P{c.p}-B{c.b}-K{c.k}-"
            f"{'moffa%d-' % c.off_a if c.off_a else ''}{'moffb%d-' % c.off_b if c.off_b else ''}"
            f"{'doff%d-' % c.dist_off if c.dist_off else ''}{c.kind}-"
            f"{'ip' if c.inplace else 'oop'}-{c.tc}-{'pad%d-' % c.pad if c.pad else ''}"
            f"{slap_steps_path(c.l, max(c.off_a, c.off_b), c.dist_off)}")


SLAP_SORTED_L = (4, 64, 68, 128, 132, 192, 196, 256)
SLAP_SHAPES = ([(l, 0, 0, 0) for l in SLAP_SORTED_L + (260, 62)] +
               [(100, 1, 0, 0), (100, 0, 1, 0), (100, 0, 0, 4)])
SLAP_B, SLAP_P = (1, 3, 5, 17), (1, 7, 20)


def _slap_steps_cases():
    """Per shape every (B, P); K, the assignment mode, the to_choose mode and the state kind
    rotate so that each path meets every value of each (asserted on the CPU)."""
    out = []
    for s, (l, off_a, off_b, dist_off) in enumerate(SLAP_SHAPES):
        j = s  # the rotation starts elsewhere on each shape
        for b in SLAP_B:
            for p in SLAP_P:
                k = (1, 2, 3, p)[j % 4]
                tc = SLAP_TC[(j // 2) % 3]
                if k > p:
                    tc = "tc"  # the uniform product tc_stride + t stays below P
                out.append(SlapStepsCase(l, p, b, k, off_a, off_b, dist_off, j % 2 == 0, tc,
                                         SLAP_KINDS[(j // 4 + j) % 3], 0))
                j += 1
    for l in (64, 128, 192, 256, 260):  # act_stride B + 3, once per KU and on the fallback
        out.append(SlapStepsCase(l, 7, 5, 7, 0, 0, 0, l % 128 == 0, "tc", "frac", 3))
    return out


SLAP_STEPS_CASES = _slap_steps_cases()


def slap_case_products(c, st):
    """The products the launch of ``c`` chooses: to_choose's columns, or tc_stride + t."""
    if c.tc == "tc":
        return st.product
    base = 0 if c.tc == "null0" else c.p - c.k
    return (base + torch.arange(c.k)).float().expand(c.b, c.k)


def _slap_steps_call(dev, c, st, product):
    l, p, b, k = c.l, c.p, c.b, c.k
    o = Outs(dev)
    ma, mb = o.new("mask_a", (b, l), U8, c.off_a), o.new("mask_b", (b, l), U8, c.off_b)
    ia, ib = o.new("i_a", (b, 1), I64), o.new("i_b", (b, 1), I64)
    o["mask_a"].t.copy_(st.mask.to(U8))
    o["i_a"].t.copy_(st.i)
    asg = o.new("assignment", (b, p), I32)
    keep = [place(st.dist, dev, c.dist_off)]
    if c.inplace:
        o["assignment"].t.copy_(st.assignment)
        asg_in = asg
    else:
        keep.append(place(st.assignment, dev))
        asg_in = _ptr(keep[-1])
    stride = b + c.pad
    act = o.new("action", (k, stride), I64)
    done, rew = o.new("done", (b, 1), U8), o.new("step_reward", (b, 1), U8)
    status = word(o, "status")
    if c.tc == "tc":  # the products in columns 0 .. K - 1 of a [B, K + 2] to_choose
        filler = torch.tensor([1e9, -7.0]).expand(b, 2)
        keep.append(place(torch.cat([product, filler], 1), dev))
        tc, tcs = _ptr(keep[-1]), k + 2
    else:
        tc, tcs = None, (0 if c.tc == "null0" else p - k)
    before = [_parent(v).clone() for v in keep]
    run(dev, "co_slap_closest_steps", b, l, p, k, _ptr(keep[0]), tc, tcs, asg_in, asg, ma, ia, mb,
        ib, act, stride, done, rew, status)
    o.check_guards()
    for v, was in zip(keep, before):
        assert torch.equal(_parent(v).view(U8), was.view(U8)), "an input was written"
    got = o.cpu()
    if c.pad:
        pad = got["action"][:, b:].contiguous().view(U8)
        assert bool((pad == FILL).all()), "the pad columns of action_out were written"
    got["action"] = got["action"][:, :b]
    return got


def _check_slap_launch(dev, c, st, product, status):
    states, actions, ref_status = slap_steps_ref(st.mask, st.i, st.assignment, st.dist, product)
    assert ref_status == status
    got = _slap_steps_call(dev, c, st, product)
    assert int(got["status"]) == status, int(got["status"])
    _same_keys(got, slap_steps_want(states, actions, status, c.k))


def check_slap_steps(dev, c):
    st = slap_steps_state(c.l, c.p, c.b, c.k, c.kind)
    _check_slap_launch(dev, c, st, slap_case_products(c, st), 0)


# -- the rows slap_state does not make
SLAP_SPECIAL_L = (64, 68, 128, 132, 192, 196, 256, 260)
SLAP_SPECIAL_P = SLAP_SPECIAL_K = 20
SLAP_SPECIAL_ROWS = {"free0": 0, "free1": 1, "free5": 2, "lane0": 3}
# row -> (i, the step at which done is true, or None)
SLAP_SPECIAL_I = ((19, 0), (10, 9), (0, 19), (23, None), (-1, None), (5, 14), (19, 0), (3, 16))
# (row, step) -> product; P and -P - 1 are out of range
SLAP_SPECIAL_PRODUCTS = {(0, 0): -1.0, (1, 3): -20.0, (2, 5): 20.0, (3, 7): -21.0, (4, 2): 2.75,
                         (5, 4): -0.5, (6, 0): 20.0, (7, 19): -21.0}


def slap_lane0_locations(l):
    """The locations lane 0 of a row's 16 lanes owns: units 0, 16, 32, 48 of 4 locations
    (those a row of 256 has, for the longer rows of the fallback)."""
    return [4 * u + j for u in range(0, min(l, 256) // 4, 16) for j in range(4)]


@functools.lru_cache(maxsize=None)
def slap_special_state(l):
    """Eight rows at P = K = 20 with distinct fractional distances: rows with 0, 1 and 5
    free locations (the action is 0 and byte 0 is "cleared" once they run out); a row,
    everything free, whose nearest locations are all of lane 0's (nearest last, so its sorted
    keys are popped in descending index order, through the part kept in LDS) and every other
    location further away; ``i`` that makes done true at step 0, at a middle step, at the
    last step and never (one of them >= P); and the products of SLAP_SPECIAL_PRODUCTS."""
    p, k, b = SLAP_SPECIAL_P, SLAP_SPECIAL_K, len(SLAP_SPECIAL_I)
    g = torch.Generator().manual_seed(4099 + l)
    dist = frac_dist(b, l, g)
    mask = torch.rand(b, l, generator=g) < 0.7
    mask[0] = False
    mask[1] = False
    mask[1, l - 2] = True
    mask[2] = False
    mask[2, torch.randperm(l, generator=g)[:5]] = True
    row, own = SLAP_SPECIAL_ROWS["lane0"], slap_lane0_locations(l)
    mask[row] = True
    dist[row] = torch.randperm(l, generator=g).float() * 0.37 + 100.0
    dist[row, own] = torch.arange(len(own), 0, -1).float() * 0.25
    i = torch.tensor([[v] for v, _ in SLAP_SPECIAL_I])
    assignment = torch.randint(-1, l, (b, p), generator=g).to(I32)
    prod = torch.randint(0, p, (b, k), generator=g).float()
    for (r, t), v in SLAP_SPECIAL_PRODUCTS.items():
        prod[r, t] = v
    return SlapSteps(mask, i, assignment, dist, prod)


def slap_special_case(l, inplace):
    return SlapStepsCase(l, SLAP_SPECIAL_P, len(SLAP_SPECIAL_I), SLAP_SPECIAL_K, 0, 0, 0, inplace,
                         "tc", "special", 0)


def check_slap_steps_special(dev, l, inplace):
    st = slap_special_state(l)
    _check_slap_launch(dev, slap_special_case(l, inplace), st, st.product, nat.ST_INDEX_RANGE)


SLAP_STATUS_L = {"sorted1": 64, "sorted2": 128, "sorted3": 192, "sorted4": 256, "single": 260}
SLAP_STATUS_P, SLAP_STATUS_K, SLAP_STATUS_B, SLAP_STATUS_ROW = 7, 5, 5, 2
SLAP_STATUS_STEPS = (0, 1, SLAP_STATUS_K - 1)


def slap_status_products(l, step):
    """In-range integer products with one bad one alone: row 2, step ``step`` (P at an even
    step, -P - 1 at an odd one)."""
    p = SLAP_STATUS_P
    st = slap_steps_state(l, p, SLAP_STATUS_B, SLAP_STATUS_K, "ties")
    prod = st.product.clone()
    prod[SLAP_STATUS_ROW, step] = p if step % 2 == 0 else -p - 1
    return st, prod


def check_slap_steps_status(dev, path, step, inplace):
    """One out-of-range product alone in a launch: the bit; that row's assignment untouched
    by that step; every other step and row as the reference has it."""
    l = SLAP_STATUS_L[path]
    assert slap_steps_path(l) == path
    st, prod = slap_status_products(l, step)
    c = SlapStepsCase(l, SLAP_STATUS_P, SLAP_STATUS_B, SLAP_STATUS_K, 0, 0, 0, inplace, "tc",
                      "ties", 0)
    _check_slap_launch(dev, c, st, prod, nat.ST_INDEX_RANGE)


def check_slap_ref_against_single_steps(dev, st, product):
    """``slap_steps_ref`` against co_slap_step chained K times on ``dev`` (the host build),
    each step given the oracle's closest-free action of the state it starts from: step 0 out
    of place from the starting assignment, then in place."""
    b, l = st.mask.shape
    p, k = st.assignment.shape[1], product.shape[1]
    states, actions, status = slap_steps_ref(st.mask, st.i, st.assignment, st.dist, product)
    o = Outs(dev)
    bufs = [{"mask": o.new(f"mask{j}", (b, l), U8), "i": o.new(f"i{j}", (b, 1), I64)} for j in (0, 1)]
    o["mask0"].t.copy_(st.mask.to(U8))
    o["i0"].t.copy_(st.i)
    asg = o.new("asg", (b, p), I32)
    asg_in, tc = place(st.assignment, dev), place(product, dev)
    done, rew = o.new("done", (b, 1), U8), o.new("rew", (b, 1), U8)
    status_w = word(o, "status")
    for t in range(k):
        cur = sc.SlapState(states[t]["action_mask"], None, None, None, None, st.dist)
        a = place(slap_closest_ref(cur), dev)
        assert torch.equal(a.cpu(), actions[t])
        s, d = bufs[t & 1], bufs[(t + 1) & 1]
        run(dev, "co_slap_step", b, l, p, _ptr(a), _ptr(tc) + 4 * t, k, _ptr(asg_in) if t == 0 else asg,
            asg, s["mask"], d["mask"], s["i"], d["i"], done, rew, status_w)
        o.check_guards()
        got, want, j = o.cpu(), states[t + 1], (t + 1) & 1
        assert_same("action_mask", got[f"mask{j}"], want["action_mask"])
        assert_same("i", got[f"i{j}"], want["i"])
        assert_same("assignment", got["asg"], want["assignment"])
        assert_same("done", got["done"], want["done"])
        assert_same("reward", got["rew"], want["step_reward"])
    assert int(o.cpu()["status"]) == status


# ====================================================================== rejections
def _rej_tsp_steps(dev):
    a, n, b, k = sc._Args(dev), 100, 5, 2
    st = tsp_steps_state(n, b, k, 1)
    args = [b, n, k, a.inp(st.acts), b, a.out("ma", (b, n), U8), a.out("ia", b, I64),
            a.out("fa", b, I64), a.out("mb", (b, n), U8), a.out("ib", b, I64), a.out("fb", b, I64),
            a.out("c", b, I64), a.out("d", b, U8), a.out("r", b, U8), 1, word(a.outs, "st")]
    rej = [(0, -1, E_INVAL), (1, 0, E_INVAL), (2, -1, E_INVAL), (2, K_MAX + 1, E_INVAL),
           (4, b - 1, E_INVAL), (14, 2, E_MODE), (14, -1, E_MODE),
           ((14, 7), (0, None), E_INVAL),           # first_mode 0 reads first_a
           ((2, 14, 7), (1, 0, None), E_INVAL),
           (7, None, E_INVAL)]                      # K > 1: step 1 writes first_a
    rej += [(j, None, E_INVAL) for j in (3, 5, 6, 8, 9, 10, 12, 13, 15)]
    return a, args, rej, 2


def _rej_slap_steps(dev):
    a, l, p, b, k = sc._Args(dev), 100, 6, 5, 3
    st = slap_steps_state(l, p, b, k, "ties")
    args = [b, l, p, k, a.inp(st.dist), a.inp(st.product.clamp(min=0)), k, a.inp(st.assignment),
            a.out("as", (b, p), I32), a.out("ma", (b, l), U8), a.out("ia", b, I64),
            a.out("mb", (b, l), U8), a.out("ib", b, I64), a.out("a", (k, b), I64), b,
            a.out("d", b, U8), a.out("r", b, U8), word(a.outs, "st")]
    rej = [(0, -1, E_INVAL), (1, 0, E_INVAL), (2, 0, E_INVAL), (3, -1, E_INVAL),
           (3, K_MAX + 1, E_INVAL), (14, b - 1, E_INVAL),
           ((5, 6), (None, p - k + 1), E_INVAL),    # to_choose NULL: tc_stride + K > P
           ((5, 6), (None, -1), E_INVAL)]
    rej += [(j, None, E_INVAL) for j in (4, 7, 8, 9, 10, 11, 12, 13, 15, 16, 17)]
    return a, args, rej, 3


STEPS_REJECTIONS = {"co_tsp_steps": _rej_tsp_steps, "co_slap_closest_steps": _rej_slap_steps}


def check_steps_rejections(dev, name):
    """Every documented CO_E_INVAL / CO_E_MODE return of ``name``, one at a time on an
    otherwise valid call with guarded buffers, and B = 0 and K = 0 (CO_OK): nothing written.
    The in / out buffers A are outputs left at their fill, a valid state."""
    a, args, rej, k_at = STEPS_REJECTIONS[name](dev)
    for where, value, code in rej:
        bad = list(args)
        if isinstance(where, tuple):
            for j, v in zip(where, value):
                bad[j] = v
        else:
            bad[where] = value
        assert rc_of(dev, name, *bad) == code, (name, where, value)
    for j in (0, k_at):  # an empty batch, no steps: CO_OK, nothing launched
        empty = list(args)
        empty[j] = 0
        assert rc_of(dev, name, *empty) == 0, (name, j)
    a.outs.check_guards()
    for key, o in a.outs.items():
        if key != "st":
            assert o.untouched(), f"{name}: a rejected call wrote {key}"
    assert int(a.outs["st"].t.cpu()) == 0
    assert rc_of(dev, name, *args) == 0, name  # and the call they were derived from is valid
    a.outs.check_guards()
    assert not a.outs["mb"].untouched(), name
