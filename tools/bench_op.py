"""The OP kernels' two measurements, per size (``--sizes 100:32768,100:1024``):

* env-steps/s of a whole random-feasible episode (every row until it returns to the depot,
  done rows padded with action 0): ``co_op_steps`` (one launch, ``feasible`` and ``length``
  written), against T single ``co_op_step`` launches through the C ABI (fresh output tensors
  per step, as the env's ``step`` makes them), and against the host build on the first 256
  rows (one thread, the median of three calls after a first one).  The three legs' final
  states are compared equal, floats bit for bit, in the same run.
* us per step of ``co_op_decode_step`` (greedy, certified, clip 10) against the pair it
  replaces, ``co_decode_step`` + ``co_op_step``, on a mid-episode state, outputs
  preallocated; the two sides' outputs are compared equal.  The pair is timed twice
  (``pair`` and ``pair_again``, the same calls) so that the run shows its own spread:
  ``decode_spread`` is the larger of the A/A difference and the widest (max - min) / median
  of a side's windows, and ``fused_faster_beyond_spread`` says whether the fused median is
  below the pair's by more than that.

Device legs are timed with device events around ``--inner`` back-to-back calls after a
warm-up; the sides of a comparison alternate window by window in this one process and the
median window of ``--reps`` is reported.  ``bytes_per_row_step`` is the header's arithmetic
(include/co_env.h) and ``tb_per_s`` what that traffic amounts to over the measured time,
against the 8 TB/s of HBM.  Prints one JSON line (``--out FILE`` also writes it).
Usage: ``python tools/bench_op.py [--sizes 100:32768,100:1024] [--reps 7] [--out F]``."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

import torch  # noqa: E402

from rl4co_slap_amd import _native as nat  # noqa: E402

HOST_ROWS = 256
HBM_TB_PER_S = 8.0
MAX_LENGTH = 4.0  # Kool et al.'s OP-100
INSTANCE = ("locs", "prize", "max_length")
CARRIED = ("visited", "tour_length", "current_total_prize", "current_node", "i")
STATE = CARRIED + ("action_mask", "done", "reward")


def _empty(dev):
    return lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)


def reset(n, b, dev):
    g = torch.Generator().manual_seed(100 + n)
    depot, locs = torch.rand(b, 2, generator=g).to(dev), torch.rand(b, n, 2, generator=g).to(dev)
    prize = ((1 + torch.randint(0, 100, (b, n), generator=g)).float() / 100).to(dev)
    budget = torch.full((b,), MAX_LENGTH, device=dev)
    e = _empty(dev)
    st = {"locs": e((b, n + 1, 2), torch.float32), "prize": e((b, n + 1), torch.float32),
          "max_length": e((b, n + 1), torch.float32), "tour_length": e((b,), torch.float32),
          "current_total_prize": e((b,), torch.float32), "current_node": e((b, 1), torch.int64),
          "i": e((b,), torch.int64), "visited": e((b, n + 1), torch.bool),
          "action_mask": e((b, n + 1), torch.bool)}
    nat.call("co_op_reset", b, n, nat.ptr(depot), nat.ptr(locs), nat.ptr(prize), nat.ptr(budget),
             *(nat.ptr(st[k]) for k in ("locs", "prize", "max_length", "tour_length",
                                        "current_total_prize", "current_node", "i", "visited",
                                        "action_mask")), nat.stream_of(locs))
    return st


def outputs(b, nc, dev):
    e = _empty(dev)
    return {"visited": e((b, nc), torch.bool), "action_mask": e((b, nc), torch.bool),
            "tour_length": e((b,), torch.float32), "current_total_prize": e((b,), torch.float32),
            "current_node": e((b, 1), torch.int64), "i": e((b,), torch.int64),
            "done": e((b,), torch.bool), "reward": e((b,), torch.bool)}


def env_args(st, o):
    """The state half of co_op_step / co_op_decode_step's arguments, after the instance."""
    return [nat.ptr(st["visited"]), nat.ptr(o["visited"]), nat.ptr(st["tour_length"]),
            nat.ptr(o["tour_length"]), nat.ptr(st["current_total_prize"]),
            nat.ptr(o["current_total_prize"]), nat.ptr(st["current_node"]),
            nat.ptr(o["current_node"]), nat.ptr(st["i"]), nat.ptr(o["i"]), nat.ptr(o["done"]),
            nat.ptr(o["reward"]), nat.ptr(o["action_mask"])]


def instance_args(st):
    return [nat.ptr(st[k]) for k in INSTANCE]


def step(st, action):
    """co_op_step into fresh tensors."""
    b, nc = st["visited"].shape
    out = outputs(b, nc, action.device)
    nat.call("co_op_step", b, nc - 1, nat.ptr(action), *instance_args(st), *env_args(st, out),
             None, nat.stream_of(action))
    return {**{k: st[k] for k in INSTANCE}, **out}


def steps(st, acts):
    """co_op_steps on copies of the state, feasible and length included."""
    t, b = acts.shape
    nc = st["visited"].shape[1]
    e = _empty(acts.device)
    out = {k: st[k].clone() for k in CARRIED}
    out.update({"action_mask": e((b, nc), torch.bool), "done": e((b,), torch.bool),
                "reward": e((b,), torch.bool), "feasible": e((t, b), torch.bool),
                "length": e((t, b), torch.float32)})
    nat.call("co_op_steps", b, nc - 1, t, nat.ptr(acts), acts.stride(0), acts.stride(1),
             nat.ptr(st["locs"]), nat.ptr(st["prize"]), nat.ptr(st["max_length"]),
             nat.ptr(st["action_mask"]), nat.ptr(out["visited"]), nat.ptr(out["tour_length"]),
             nat.ptr(out["current_total_prize"]), nat.ptr(out["current_node"]), nat.ptr(out["i"]),
             nat.ptr(out["done"]), nat.ptr(out["reward"]), nat.ptr(out["action_mask"]),
             nat.ptr(out["feasible"]), nat.ptr(out["length"]), None, nat.stream_of(acts))
    return out


def random_episode(start, seed):
    """Actions [T, B] of a random-feasible episode (the depot only when no customer is open),
    and the state after every step."""
    dev = start["visited"].device
    g = torch.Generator(device=dev).manual_seed(seed)
    st, acts, states = start, [], [start]
    finished = torch.zeros(start["visited"].shape[0], dtype=torch.bool, device=dev)
    while not bool(finished.all()):
        m = st["action_mask"]
        score = torch.rand(m.shape, generator=g, device=dev).masked_fill(~m, -1.0)
        score[:, 0] = -0.5
        a = score.argmax(1)
        st = step(st, a)
        finished |= st["done"]
        acts.append(a)
        states.append(st)
    return torch.stack(acts), states


def window(fn, inner, dev):
    """Seconds per call over ``inner`` back-to-back calls."""
    if dev == "cpu":  # a dry run of this tool without a device: wall clock
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        return (time.perf_counter() - t0) / inner
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / inner


def interleaved(sides, reps, inner, dev):
    """{name: every window's seconds per call}: the sides alternate window by window."""
    for fn in sides.values():  # warm-up: code objects, the allocator's blocks
        window(fn, 2, dev)
    took = {k: [] for k in sides}
    for _ in range(reps):
        for k, fn in sides.items():
            took[k].append(window(fn, inner, dev))
    return took


def decode_sides(st, dev, clip=10.0, temp=1.0):
    """The fused call and the pair on the same mid-episode state, outputs preallocated."""
    b, nc = st["visited"].shape
    logits = (torch.randn(b, nc, generator=torch.Generator().manual_seed(5)) * 3).to(dev)
    word = nat.DECODE_CERTIFIED  # greedy | certified
    s = nat.stream_of(logits)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    e = _empty(dev)
    of, op = ({**outputs(b, nc, dev), "action": e((b,), torch.int64),
               "logp": e((b,), torch.float32)} for _ in range(2))

    inst = nat.op_instance(*(st[k] for k in INSTANCE))

    def fused():
        nat.call("co_op_decode_step", b, nc - 1, nat.ptr(logits), logits.stride(0),
                 nat.ptr(st["action_mask"]), clip, temp, word, None, nat.ptr(of["action"]),
                 nat.ptr(of["logp"]), 0, 0, inst.address, *env_args(st, of), None, nat.ptr(status), s)

    def pair():
        nat.call("co_decode_step", b, nc, nat.ptr(logits), logits.stride(0),
                 nat.ptr(st["action_mask"]), clip, temp, word, None, nat.ptr(op["action"]),
                 nat.ptr(op["logp"]), None, 0, 0, nat.ptr(status), s)
        nat.call("co_op_step", b, nc - 1, nat.ptr(op["action"]), *instance_args(st),
                 *env_args(st, op),
                 nat.ptr(status), s)

    return {"fused": fused, "pair": pair, "pair_again": pair}, of, op, status


def same(a, b):
    if a.dtype == torch.float32:
        return torch.equal(a.view(torch.int32), b.view(torch.int32))
    return torch.equal(a, b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100:32768,100:1024")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = a.device
    if dev != "cpu" and not torch.cuda.is_available():
        raise SystemExit("bench_op: no GPU (pass --device cpu for a dry run of the host path)")
    out = {"bench": "op", "device": dev, "reps": a.reps, "inner": a.inner,
           "host_rows": HOST_ROWS, "hbm_tb_per_s": HBM_TB_PER_S, "max_length": MAX_LENGTH}
    med = statistics.median
    for size in a.sizes.split(","):
        n, b = (int(x) for x in size.split(":"))
        nc = n + 1
        start = reset(n, b, dev)
        acts, states = random_episode(start, 7 + n)
        t = acts.shape[0]
        got = {}

        def launch_steps():
            got["steps"] = steps(start, acts)

        def launch_single():
            st = start
            for x in acts:
                st = step(st, x)
            got["single"] = st

        took = interleaved({"steps": launch_steps, "single": launch_single}, a.reps,
                           max(1, a.inner // 10), dev)
        sec = {k: med(v) for k, v in took.items()}
        rows = min(HOST_ROWS, b)
        host_start = {k: v[:rows].cpu().contiguous() for k, v in start.items()}
        host_acts = acts[:, :rows].cpu().contiguous()
        torch.set_num_threads(1)
        host_s = []
        for _ in range(4):  # the first call loads the host library
            t0 = time.perf_counter()
            got_h = steps(host_start, host_acts)
            host_s.append(time.perf_counter() - t0)
        sec_h = med(host_s[1:])
        assert bool(got["steps"]["feasible"].all())
        for key in STATE:
            assert same(got["steps"][key], got["single"][key]), (size, key)
            assert same(got["steps"][key][:rows].cpu(), got_h[key]), (size, key, "host")
        dtook = None
        if dev != "cpu":  # the fused decode step has no host build
            sides, of, op, status = decode_sides(states[t // 2], dev)
            dtook = interleaved(sides, a.reps, a.inner, dev)
            assert int(status.item()) == 0
            for key in of:
                assert same(of[key], op[key]), (size, key, "fused decode vs the pair")
        # per row-step: the action, locs[a], prize[a], max_length[a], feasible, length; the
        # rows and the row scalars once (include/co_env.h)
        steps_bytes = 29 + (15 * nc + 58) / t
        single_bytes = 15 * nc + 78
        decode_bytes = 20 * nc + 82
        out[f"n{n}_b{b}"] = {
            "steps": t,
            "steps_launch_steps_per_s": round(b * t / sec["steps"], 1),
            "single_launches_steps_per_s": round(b * t / sec["single"], 1),
            "host_1thread_steps_per_s": round(rows * t / sec_h, 1),
            "steps_launch_ms": round(sec["steps"] * 1e3, 4),
            "single_launches_ms": round(sec["single"] * 1e3, 4),
            "final_states_equal": True,
            "steps_bytes_per_row_step": round(steps_bytes, 2),
            "steps_tb_per_s": round(steps_bytes * b * t / sec["steps"] / 1e12, 4),
            "single_step_bytes_per_row_step": single_bytes,
            "single_step_tb_per_s": round(single_bytes * b * t / sec["single"] / 1e12, 4),
            "decode_bytes_per_row_step": decode_bytes}
        if dtook is not None:
            dsec = {k: med(v) for k, v in dtook.items()}
            spread = max([abs(dsec["pair"] - dsec["pair_again"]) / dsec["pair"]]
                         + [(max(v) - min(v)) / med(v) for v in dtook.values()])
            out[f"n{n}_b{b}"].update({
                "decode_fused_us_per_step": round(dsec["fused"] * 1e6, 3),
                "decode_pair_us_per_step": round(dsec["pair"] * 1e6, 3),
                "decode_pair_again_us_per_step": round(dsec["pair_again"] * 1e6, 3),
                "decode_windows_us": {k: [round(x * 1e6, 3) for x in v]
                                      for k, v in dtook.items()},
                "decode_spread": round(spread, 4),
                "decode_outputs_equal": True,
                "decode_fused_tb_per_s": round(decode_bytes * b / dsec["fused"] / 1e12, 4),
                "fused_faster_beyond_spread":
                    dsec["fused"] < min(dsec["pair"], dsec["pair_again"]) * (1 - spread)})
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
